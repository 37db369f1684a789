"""Argument checks of the C ABI's encode and decode entry points: return code and dgpu_last_error() text of a call with
ONE fault, as literals.  The library loads without a device and every check here returns before the first HIP call, so
the pointers are small fake addresses that are never dereferenced."""
import ctypes as C

import pytest

A = 0x10000          # a fake device address, aligned to everything
TOO_LARGE = 1717538816 + 1

PROB = "probBits must be 9, 10 or 11"
BATCH = "numInBatch must be <= 65535"
FLOAT = "floatType must be float16, bfloat16 or float32"
ANS_IN = "ANS input must be 4-byte aligned"
COMP_OUT = "compressed output must be 16-byte aligned"
COMP_IN = "compressed input must be 16-byte aligned"
FLOAT_IN = "float input must be float-word aligned"
FLOAT_OUT = "float output must be float-word aligned"
OUT4 = "output must be 4-byte aligned"
SPLIT = "interior split sizes must be multiples of 4 bytes"
ANS_LARGE = "input larger than 1717538816 bytes: its maximum compressed size exceeds INT32_MAX (GpuANSEncode.cu:22)"
FLOAT_LARGE = ("tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX "
               "(GpuANSEncode.cu:22)")
RANGE_NULL = "ranged decode: null array with numInBatch > 0"
RANGE_CAP = "ranged decode: outCapacity must not exceed 0xfffff000"
CAPPED_ALIGN = "compressed output rows, their stride and their capacity must be 16-byte aligned"

# name -> parameters in the order of include/dietgpu_amd.h.  P: array of pointers, U: array of uint32, everything else
# a scalar; `used` and `err` are the tempUsed / errBatch out-parameters.
HEAD, FHEAD = "temp tempBytes used probBits useChecksum n", "temp tempBytes used floatType probBits useChecksum n"
TAIL = "outSuccess outSize stream err"
SPECS = {
    "dgpu_ans_encode_batch_stride": f"{HEAD} in_dev inSize inStride hist out_dev outStride outSize stream",
    "dgpu_ans_encode_batch_pointer": f"{HEAD} P:in U:sizes hist P:out outSize stream",
    "dgpu_ans_encode_batch_split_size": f"{HEAD} in_dev U:sizes hist out_dev outStride outSize stream",
    "dgpu_float_compress": f"{FHEAD} P:in U:sizes P:out outSize stream",
    "dgpu_float_compress_split_size": f"{FHEAD} in_dev U:sizes out_dev outStride outSize stream",
    "dgpu_float_compress_stride_capped": f"{FHEAD} in_dev inWords inStride out_dev outStride outCap outSize stream",
    "dgpu_ans_decode_batch_stride": f"{HEAD} in_dev inStride out_dev outStride outCap {TAIL}",
    "dgpu_ans_decode_batch_pointer": f"{HEAD} P:in P:out U:sizes {TAIL}",
    "dgpu_ans_decode_batch_split_size": f"{HEAD} P:in out_dev U:sizes {TAIL}",
    "dgpu_ans_decode_batch_pointer_bounded": f"{HEAD} P:in U:inBytes P:out U:sizes {TAIL}",
    "dgpu_ans_decode_batch_split_size_bounded": f"{HEAD} P:in U:inBytes out_dev U:sizes {TAIL}",
    "dgpu_float_decompress": f"{FHEAD} P:in P:out U:sizes {TAIL}",
    "dgpu_float_decompress_split_size": f"{FHEAD} P:in out_dev U:sizes {TAIL}",
    "dgpu_float_decompress_bounded": f"{FHEAD} P:in U:inBytes P:out U:sizes {TAIL}",
    "dgpu_float_decompress_split_size_bounded": f"{FHEAD} P:in U:inBytes out_dev U:sizes {TAIL}",
    "dgpu_float_decompress_stride_bounded": f"{FHEAD} in_dev inStride inBytes out_dev outStride outCap {TAIL}",
    "dgpu_ans_decode_batch_pointer_range": "temp tempBytes used probBits n P:in U:inBytes U:first U:num P:out U:sizes outSuccess outSize stream",
    "dgpu_float_decompress_range": "temp tempBytes used floatType probBits n P:in U:inBytes U:first U:num P:out U:sizes outSuccess outSize stream",
}
# a valid call of every shape (bfloat16 where there is a float type)
DEFAULTS = dict(temp=None, tempBytes=0, probBits=10, useChecksum=0, floatType=2, in_dev=A, out_dev=A, inSize=4096, inStride=8192,
                outStride=8192, outCap=4096, inBytes=8192, hist=None, outSuccess=None, outSize=None, stream=None)
DEFAULTS_OF = {"dgpu_float_compress_stride_capped": dict(inWords=8192, inStride=16384, outStride=65536, outCap=65536)}
FLOATS = [n for n in SPECS if "float" in n]
DECODERS = [n for n in SPECS if "decode" in n or "decompress" in n]
RANGED = [n for n in SPECS if n.endswith("_range")]
ANS_SPLIT_DECODERS = ["dgpu_ans_decode_batch_split_size", "dgpu_ans_decode_batch_split_size_bounded"]


def call(name, n=1, **over):
    """-> (return code, last error, tempUsed, errBatch or None).  An array given as a list is converted; an array
    given as None is passed as a null pointer."""
    import dietgpu_amd

    L = dietgpu_amd.lib()
    used, err = C.c_size_t(77), C.c_int32(5)
    args = []
    for p in SPECS[name].split():
        kind, _, key = p.rpartition(":")
        if key == "used":
            args.append(C.byref(used))
        elif key == "err":
            args.append(C.byref(err))
        elif key == "n":
            args.append(n)
        elif kind:
            ctype, fill = (C.c_void_p, A) if kind == "P" else (C.c_uint32, 4096)
            v = over.get(key, [fill] * n)
            args.append(None if v is None else (ctype * len(v))(*v))
        else:
            args.append(over.get(key, DEFAULTS_OF.get(name, {}).get(key, DEFAULTS.get(key))))
    assert not set(over) - {p.rpartition(":")[2] for p in SPECS[name].split()}, "the row names a parameter the entry point lacks"
    rc = getattr(L, name)(*args)
    return rc, L.dgpu_last_error().decode(), used.value, err.value if " err" in SPECS[name] else None


def rows():
    r = []
    for name in SPECS:
        r += [(name, 1, dict(probBits=8), PROB), (name, 1, dict(probBits=12), PROB), (name, 65536, {}, BATCH)]
    for name in FLOATS:
        r += [(name, 1, dict(floatType=0), FLOAT), (name, 1, dict(floatType=4), FLOAT)]
    # alignment of each side: a pointer, then a stride (which only counts from the second element on)
    r += [
        ("dgpu_ans_encode_batch_stride", 1, dict(in_dev=A + 2), ANS_IN),
        ("dgpu_ans_encode_batch_stride", 2, dict(inStride=8190), ANS_IN),
        ("dgpu_ans_encode_batch_stride", 1, dict(out_dev=A + 8), COMP_OUT),
        ("dgpu_ans_encode_batch_stride", 2, dict(outStride=8200), COMP_OUT),
        ("dgpu_ans_encode_batch_pointer", 2, {"in": [A, A + 2]}, ANS_IN),
        ("dgpu_ans_encode_batch_pointer", 2, dict(out=[A, A + 8]), COMP_OUT),
        ("dgpu_ans_encode_batch_split_size", 1, dict(in_dev=A + 2), ANS_IN),
        ("dgpu_ans_encode_batch_split_size", 1, dict(out_dev=A + 8), COMP_OUT),
        ("dgpu_ans_encode_batch_split_size", 2, dict(outStride=8200), COMP_OUT),
        ("dgpu_ans_encode_batch_split_size", 2, dict(sizes=[6, 4096]), SPLIT),
        ("dgpu_float_compress", 2, {"in": [A, A + 1]}, FLOAT_IN),
        ("dgpu_float_compress", 2, {"in": [A, A + 2], "floatType": 3}, FLOAT_IN),
        ("dgpu_float_compress", 2, dict(out=[A, A + 8]), COMP_OUT),
        ("dgpu_float_compress_split_size", 1, dict(out_dev=A + 8), COMP_OUT),
        ("dgpu_float_compress_split_size", 2, dict(outStride=8200), COMP_OUT),
        ("dgpu_ans_decode_batch_stride", 1, dict(in_dev=A + 8), COMP_IN),
        ("dgpu_ans_decode_batch_stride", 2, dict(inStride=8200), COMP_IN),
    ]
    for name in DECODERS:
        if "P:in" in SPECS[name]:  # an array of archive pointers
            r.append((name, 2, {"in": [A, A + 8]}, COMP_IN))
    for name in ANS_SPLIT_DECODERS:
        r += [(name, 1, dict(out_dev=A + 2), OUT4), (name, 2, dict(sizes=[6, 4096]), SPLIT)]
    # a size one past the largest the format can hold
    r += [
        ("dgpu_ans_encode_batch_stride", 1, dict(inSize=TOO_LARGE), ANS_LARGE),
        ("dgpu_ans_encode_batch_pointer", 1, dict(sizes=[TOO_LARGE]), ANS_LARGE),
        ("dgpu_ans_encode_batch_split_size", 1, dict(sizes=[TOO_LARGE]), ANS_LARGE),
        ("dgpu_float_compress", 1, dict(sizes=[TOO_LARGE]), FLOAT_LARGE),
        ("dgpu_float_compress_split_size", 1, dict(sizes=[TOO_LARGE]), FLOAT_LARGE),
        ("dgpu_float_compress_stride_capped", 1, dict(inWords=TOO_LARGE, outCap=0xfffffff0),
         "tensor larger than 1717538816 words (GpuANSEncode.cu:22)"),
    ]
    for name in RANGED:
        r.append((name, 1, dict(sizes=[0xfffff001]), RANGE_CAP))
        r += [(name, 1, {key: None}, RANGE_NULL) for key in ("in", "inBytes", "first", "num", "out", "sizes")]
    # the checks of the two stride entry points of the compressed collectives
    r += [
        ("dgpu_float_compress_stride_capped", 1, dict(in_dev=A + 1), FLOAT_IN),
        ("dgpu_float_compress_stride_capped", 2, dict(inStride=16383), FLOAT_IN),
        ("dgpu_float_compress_stride_capped", 1, dict(out_dev=A + 8), CAPPED_ALIGN),
        ("dgpu_float_compress_stride_capped", 2, dict(outStride=65544), CAPPED_ALIGN),
        ("dgpu_float_compress_stride_capped", 1, dict(outCap=65528), CAPPED_ALIGN),
        ("dgpu_float_compress_stride_capped", 2, dict(outCap=65552), "outCapacityBytes must not exceed outStrideBytes"),
        ("dgpu_float_compress_stride_capped", 1, dict(inWords=4096), "capped compression needs rows of more than one 4096-word block"),
        ("dgpu_float_compress_stride_capped", 1, dict(outCap=16),
         "outCapacityBytes is smaller than the archive's header, tables and non-compressed planes"),
        ("dgpu_float_decompress_stride_bounded", 1, dict(in_dev=A + 8), COMP_IN),
        ("dgpu_float_decompress_stride_bounded", 2, dict(inStride=8200), COMP_IN),
        ("dgpu_float_decompress_stride_bounded", 1, dict(out_dev=A + 1), FLOAT_OUT),
        ("dgpu_float_decompress_stride_bounded", 2, dict(outStride=8191), FLOAT_OUT),
        ("dgpu_float_decompress_stride_bounded", 1, dict(inBytes=0), "inBytes must be the bytes available per compressed row"),
    ]
    return r


ROWS = rows()


def test_the_table_covers_every_encode_and_decode_entry_point():
    import dietgpu_amd

    codec = {n for n in dietgpu_amd.EXPORTED_SYMBOLS
             if any(w in n for w in ("encode_batch", "decode_batch", "float_compress", "float_decompress")) and "temp_bytes" not in n}
    assert codec == set(SPECS) == {row[0] for row in ROWS}


@pytest.mark.parametrize("name,n,over,message", ROWS, ids=[f"{r[0][5:]}-{r[1]}-{'-'.join(f'{k}' for k in r[2]) or 'n'}-{i}" for i, r in enumerate(ROWS)])
def test_one_fault_gives_this_code_and_text(name, n, over, message):
    rc, text, used, err = call(name, n, **over)
    assert (rc, text) == (1, message)  # DGPU_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", list(SPECS))
def test_an_empty_batch_is_ok_and_resets_the_out_parameters(name):
    rc, _, used, err = call(name, 0)
    assert rc == 0 and used == 0
    assert err in (None, -1)
    assert (err is None) == (" err" not in SPECS[name])

"""Argument checks of dgpu_ans_delta_encode / dgpu_ans_delta_decode (one fault per call, fake addresses that are never
dereferenced: every check returns before the first HIP call) and of the ops wrappers, without a GPU."""
import ctypes as C

import pytest
import torch

import dietgpu_amd as dg

A = 0x10000  # a fake device address, aligned to everything
ENC, DEC = "dgpu_ans_delta_encode", "dgpu_ans_delta_decode"
PROB, BATCH, OVERLAP = "probBits must be 9, 10 or 11", "numInBatch must be <= 65535", "delta decode: out[i] must equal base[i] or not overlap it"


def call(name, n=1, probBits=10, **over):
    L = dg.lib()

    def arr(key, ctype, fill):  # an array given as None is passed as a null pointer
        v = over.get(key, [fill] * n)
        return None if v is None else (ctype * len(v))(*v)

    ptrs = lambda key, fill=A: arr(key, C.c_void_p, fill)
    sizes = arr("sizes", C.c_uint32, 4096)
    if name == ENC:
        rc = L.dgpu_ans_delta_encode(probBits, n, ptrs("in"), ptrs("base", 2 * A), sizes, ptrs("out", 4 * A), None, None)
    else:
        rc = L.dgpu_ans_delta_decode(probBits, n, ptrs("in"), arr("inBytes", C.c_uint32, 8192), ptrs("base", 2 * A), ptrs("out", 4 * A),
                                     sizes, None, None, None)
    return rc, L.dgpu_last_error().decode()


ROWS = [(name, 1, dict(probBits=p), PROB) for name in (ENC, DEC) for p in (8, 12)] + [(name, 65536, {}, BATCH) for name in (ENC, DEC)] + [
    (ENC, 2, {"in": [A, A + 2]}, "ANS input must be 4-byte aligned"),
    (ENC, 2, dict(base=[A, A + 2]), "delta encode: base must be 4-byte aligned"),
    (ENC, 2, dict(out=[A, A + 8]), "compressed output must be 16-byte aligned"),
    (ENC, 1, dict(sizes=[1717538816 + 1]), "input larger than 1717538816 bytes: its maximum compressed size exceeds INT32_MAX (GpuANSEncode.cu:22)"),
    (DEC, 2, {"in": [A, A + 8]}, "compressed input must be 16-byte aligned"),
    (DEC, 1, dict(base=[4 * A + 1]), OVERLAP),
    (DEC, 1, dict(base=[4 * A - 4095]), OVERLAP),
    (DEC, 1, dict(sizes=[0xFFFFF001], base=[1 << 40]),"delta decode: outCapacity must not exceed 0xfffff000"),
] + [(ENC, 1, {k: None}, "delta encode: null array with numInBatch > 0") for k in ("in", "base", "sizes", "out")] + [
    (DEC, 1, {k: None}, "delta decode: null array with numInBatch > 0") for k in ("in", "inBytes", "base", "out", "sizes")]


@pytest.mark.parametrize("name,n,over,message", ROWS, ids=[f"{r[0][9:]}-{r[1]}-{'-'.join(r[2]) or 'n'}-{i}" for i, r in enumerate(ROWS)])
def test_one_fault_gives_this_code_and_text(name, n, over, message):
    assert call(name, n, **over) == (1, message)  # DGPU_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", [ENC, DEC])
def test_an_empty_batch_is_ok(name):
    assert call(name, 0)[0] == 0


@pytest.mark.parametrize("other", [torch.zeros(8, dtype=torch.float16), torch.zeros(9, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.bfloat16)],
                         ids=["dtype", "numel", "device"])
def test_the_ops_check_every_pair_and_the_device(other):
    t, comp = torch.zeros(8, dtype=torch.bfloat16), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        dg.compress_data_delta([t], [other])
    with pytest.raises(RuntimeError):
        dg.decompress_data_delta([comp], [other], [t])
    with pytest.raises(RuntimeError):
        dg.decompress_data_delta([comp], [other])  # in place

"""Argument checks of dgpu_fp8_cast_compress / dgpu_fp8_decode_accumulate (one fault per call, fake addresses that are
never dereferenced: every check returns before the first HIP call) and of the ops wrappers, without a GPU."""
import ctypes as C

import pytest
import torch

import dietgpu_amd as dg

A = 0x10000  # a fake device address, aligned to everything
ENC, DEC = "dgpu_fp8_cast_compress", "dgpu_fp8_decode_accumulate"
WHAT = {ENC: "fp8 cast-compress", DEC: "fp8 decode-accumulate"}
PROB, BATCH, TYPE = "probBits must be 9, 10 or 11", "numInBatch must be <= 65535", "fp8Type must be DGPU_FP8_E4M3FN or DGPU_FP8_E5M2"


def call(name, n=1, probBits=10, fp8Type=0, scale=1.0, scale_dev=None, perMember=0, **over):
    L = dg.lib()

    def arr(key, ctype, fill):  # an array given as None is passed as a null pointer
        v = over.get(key, [fill] * n)
        return None if v is None else (ctype * len(v))(*v)

    ptrs = lambda key, fill=A: arr(key, C.c_void_p, fill)
    sizes = arr("sizes", C.c_uint32, 4096)
    if name == ENC:
        rc = L.dgpu_fp8_cast_compress(fp8Type, probBits, n, ptrs("in"), sizes, scale, scale_dev, perMember, ptrs("out", 4 * A), None, None)
    else:
        rc = L.dgpu_fp8_decode_accumulate(fp8Type, probBits, 1, n, ptrs("in"), arr("inBytes", C.c_uint32, 8192), scale, scale_dev, perMember,
                                          ptrs("acc", 4 * A), sizes, None, None, None)
    return rc, L.dgpu_last_error().decode()


ROWS = [(name, 1, dict(probBits=p), PROB) for name in (ENC, DEC) for p in (8, 12)] + [(name, 65536, {}, BATCH) for name in (ENC, DEC)] + [
    (name, 1, dict(fp8Type=2), TYPE) for name in (ENC, DEC)] + [
    (name, 1, dict(scale=s), WHAT[name] + ": a host scale must be finite and not zero") for name in (ENC, DEC) for s in (0.0, float("inf"))] + [
    (name, 1, dict(scale_dev=A + 2), WHAT[name] + ": scale_dev must be 4-byte aligned") for name in (ENC, DEC)] + [
    (name, 1, dict(perMember=2), WHAT[name] + ": scalePerMember must be 0 (one factor) or 1 (one per member)") for name in (ENC, DEC)] + [
    (ENC, 2, {"in": [A, A + 2]}, "fp8 cast-compress: float32 input must be 4-byte aligned"),
    (ENC, 2, dict(out=[A, A + 8]), "compressed output must be 16-byte aligned"),
    (ENC, 1, dict(sizes=[1717538816 + 1]), "tensor larger than 1717538816 words: its maximum compressed size exceeds INT32_MAX (GpuANSEncode.cu:22)"),
    (DEC, 2, {"in": [A, A + 8]}, "compressed input must be 16-byte aligned"),
    (DEC, 2, dict(acc=[A, A + 2]), "fp8 decode-accumulate: accumulators must be 4-byte aligned"),
    (DEC, 1, dict(sizes=[0xFFFFF001]), "fp8 decode-accumulate: accWords must not exceed 0xfffff000"),
] + [(ENC, 1, {k: None}, "fp8 cast-compress: null array with numInBatch > 0") for k in ("in", "sizes", "out")] + [
    (DEC, 1, {k: None}, "fp8 decode-accumulate: null array with numInBatch > 0") for k in ("in", "inBytes", "acc", "sizes")]


@pytest.mark.parametrize("name,n,over,message", ROWS, ids=[f"{r[0][9:]}-{r[1]}-{'-'.join(r[2]) or 'n'}-{i}" for i, r in enumerate(ROWS)])
def test_one_fault_gives_this_code_and_text(name, n, over, message):
    assert call(name, n, **over) == (1, message)  # DGPU_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", [ENC, DEC])
def test_an_empty_batch_is_ok(name):
    assert call(name, 0)[0] == 0


@pytest.mark.parametrize("dtype", [torch.float8_e4m3fn, torch.float8_e5m2])
def test_the_ops_reject_cpu_tensors_and_other_inputs(dtype):
    comp, acc = torch.zeros(64, dtype=torch.uint8), torch.zeros(8)
    for bad in (torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16)):  # float32 on the CPU; not float32
        with pytest.raises(RuntimeError):
            dg.compress_data_cast([bad], dtype, scale=64.0)
    with pytest.raises(RuntimeError):
        dg.decompress_data_accumulate([comp], [acc], dtype=dtype, scale=0.5)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_scale_is_rejected_for_the_16_bit_dtypes(dtype):
    with pytest.raises(RuntimeError, match="have no factor"):
        dg.compress_data_cast([torch.zeros(8)], dtype, scale=2.0)

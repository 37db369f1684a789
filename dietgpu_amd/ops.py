"""Tensor API of the codec: the ten ops of `torch.ops.dietgpu.*`.

Mirrors dietgpu/DietGpu.cpp (schema strings at DietGpu.cpp:915-937; argument
validation at :149-275, :310-522, :530-911) on PyTorch-ROCm tensors: same
names, argument order, defaults, return values and error conditions
(TORCH_CHECK -> RuntimeError).  PyTorch is only plumbing here (device memory
and the current HIP stream); all work happens in libdietgpu_amd.so through the
C ABI of include/dietgpu_amd.h.

Extra keyword `prob_bits` (default 10, as kDefaultPrecision DietGpu.cpp:114)
exposes the C++ API's ANSCodecConfig.probBits in {9, 10, 11}.

Two routes to the same C ABI.  The six codec ops are handed to `torch.ops.dietgpu.*` (csrc/torch_ops.cpp: argument
checks and pointer marshalling in C++, ~2 us of host time per call) when libdietgpu_torch.so is there -- at `prob_bits`
9 / 11 with the library's thread-local precision set around the call (the registered ops themselves fix the precision
at 10, as upstream); the ctypes route below serves builds without the op library.  256 tensors per call cost ~120 us of Python per op on the
ctypes route (profiles/r03_api_rate.txt) -- `prefer_torch_ops(False)` forces it (the test-suite runs every parity test
on both routes).  Either way the work is done by libdietgpu_amd.so: there is no CPU path.
"""
import ctypes as C
import math
import os
import threading

import torch

from ._lib import check, lib

FLOAT16, BFLOAT16, FLOAT32 = 1, 2, 3
_DTYPE_TO_FT = {torch.float16: FLOAT16, torch.bfloat16: BFLOAT16, torch.float32: FLOAT32}
_FT_TO_DTYPE = {v: k for k, v in _DTYPE_TO_FT.items()}
K_DEFAULT_PRECISION = 10
_U32_MAX = (1 << 32) - 1


_PREFER_TORCH_OPS = True
_TORCH_OPS = None  # None: not tried yet; False: libdietgpu_torch.so is not there (or stale)
_TORCH_OPS_LOCK = threading.Lock()


def prefer_torch_ops(enable=True):
    """Route the codec ops through torch.ops.dietgpu.* at prob_bits 10 (default) or force the ctypes route."""
    global _PREFER_TORCH_OPS
    _PREFER_TORCH_OPS = bool(enable)


class _OpsAtPrecision:
    """torch.ops.dietgpu.* at prob_bits 9 / 11: the op library's thread-local precision (dietgpu_amd::set_precision, an
    extra op beside the reference's ten) is set around the call and put back to the default."""

    def __init__(self, ops, prob_bits):
        self._ops, self._p = ops, prob_bits

    def __getattr__(self, name):
        fn = getattr(self._ops, name)

        def call(*args):
            torch.ops.dietgpu_amd.set_precision(self._p)
            try:
                return fn(*args)
            finally:
                torch.ops.dietgpu_amd.set_precision(K_DEFAULT_PRECISION)

        return call


def _fast_ops(prob_bits):
    global _TORCH_OPS
    if prob_bits not in (9, 10, 11) or not _PREFER_TORCH_OPS:
        return None
    if _TORCH_OPS is None:
        with _TORCH_OPS_LOCK:
            if _TORCH_OPS is None:
                _TORCH_OPS = _load_fast_ops()
    if not _TORCH_OPS:
        return None
    return _TORCH_OPS if prob_bits == K_DEFAULT_PRECISION else _OpsAtPrecision(_TORCH_OPS, prob_bits)


def _load_fast_ops():
    """torch.ops.dietgpu from the in-tree op library, or False.  An op library built against another version of the C
    ABI than the core library it finds registers NO op implementations (torch_ops.cpp: nothing may throw out of a static
    initialiser under dlopen) and says so through two plain C symbols, which are compared here: the ctypes route then
    serves the calls.  An op library from before those symbols existed is treated the same way.  (File times are NOT
    consulted: a rebuild of the core library from unchanged sources, or a copy of the tree, says nothing about the
    sources the op library was built from.)"""
    import warnings

    from .build import TORCH_LIB_PATH

    if not os.path.exists(TORCH_LIB_PATH):
        return False
    core = lib()  # libdietgpu_amd.so first (the op library links against it)
    try:
        torch.ops.load_library(TORCH_LIB_PATH)
        handle = C.CDLL(TORCH_LIB_PATH)  # (already mapped: the same handle)
    except (OSError, RuntimeError) as e:
        warnings.warn(f"{TORCH_LIB_PATH} could not be loaded ({e}): the ctypes route is used")
        return False
    try:
        handle.dgpu_torch_built_abi.restype = C.c_uint32
        built, registered = int(handle.dgpu_torch_built_abi()), int(handle.dgpu_torch_ops_registered())
    except AttributeError:
        built, registered = None, 0
    have = int(core.dgpu_abi_version())
    if built != have or not registered:
        warnings.warn(f"{TORCH_LIB_PATH} was built against C ABI version {built} of dietgpu_amd.h, libdietgpu_amd.so has "
                      f"version {have}: the ctypes route is used (rebuild: python -m dietgpu_amd.build)")
        return False
    if not hasattr(torch.ops, "dietgpu_amd") or not hasattr(torch.ops.dietgpu_amd, "set_precision"):
        return False
    return torch.ops.dietgpu


def _amd_op(prob_bits, name):
    """torch.ops.dietgpu_amd.<name> (the ops beside the reference's ten) with the op library's precision set around the
    call and put back, or None when the ctypes route serves this call: the route is off, or the library lacks the op."""
    if _fast_ops(prob_bits) is None or not hasattr(torch.ops.dietgpu_amd, name):
        return None
    op = getattr(torch.ops.dietgpu_amd, name)

    def call(*args):
        torch.ops.dietgpu_amd.set_precision(prob_bits)
        try:
            return op(*args)
        finally:
            torch.ops.dietgpu_amd.set_precision(K_DEFAULT_PRECISION)

    return call


def _check(cond, msg="argument check failed"):
    if not cond:
        raise RuntimeError(msg)


def _float_type(t):
    """getFloatTypeFromDtype, DietGpu.cpp:18-32"""
    _check(t.dtype in _DTYPE_TO_FT, "tensor must be float16, bfloat16 or float32")
    return _DTYPE_TO_FT[t.dtype]


def _total_and_max(ts):
    """getTotalAndMaxSize, DietGpu.cpp:54-73"""
    total = mx = 0
    for t in ts:
        n = t.numel()
        _check(n * t.element_size() <= _U32_MAX)
        total += n
        mx = max(mx, n)
    return total, mx


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ctypes arrays are cached by content: a loop that compresses the same tensors step after step (the steady
# state the library's parameter cache is built for) then spends its host time on one tuple hash instead of
# three array constructions per call.
_ARRAY_CACHE = {}
_ARRAY_CACHE_MAX = 256


def _cached_array(ctype, values):
    key = (ctype, values)
    arr = _ARRAY_CACHE.get(key)
    if arr is None:
        if len(_ARRAY_CACHE) >= _ARRAY_CACHE_MAX:
            _ARRAY_CACHE.clear()
        arr = (ctype * len(values))(*values)
        _ARRAY_CACHE[key] = arr
    return arr


def _ptr_array(ts):
    return _cached_array(C.c_void_p, tuple(t.data_ptr() for t in ts))


def _u32_array(vals):
    return _cached_array(C.c_uint32, tuple(vals))


def _in_bytes(ts):
    """bytes each compressed input tensor holds: the decoder rejects an archive that claims more"""
    return _cached_array(C.c_uint32, tuple(min(t.numel() * t.element_size(), _U32_MAX) for t in ts))


def _temp(temp_mem, dev):
    if temp_mem is None:
        return None, 0
    _check(temp_mem.is_cuda and temp_mem.is_contiguous())
    _check(temp_mem.get_device() == dev)
    return C.c_void_p(temp_mem.data_ptr()), temp_mem.numel() * temp_mem.element_size()


# ---------------------------------------------------------------- size queries
def max_float_compressed_output_size(ts):
    _, mx = _total_and_max(ts)
    return len(ts), _guarded(int(lib().dgpu_float_max_compressed_size(_float_type(ts[0]), mx)), mx)


def max_float_compressed_size(dtype, size):
    return _guarded(int(lib().dgpu_float_max_compressed_size(_float_type(dtype), size)), size)


def max_any_compressed_output_size(ts):
    _, mx = _total_and_max(ts)
    return len(ts), _guarded(int(lib().dgpu_ans_max_compressed_size(mx * ts[0].element_size())), mx * ts[0].element_size())


def max_any_compressed_size(nbytes):
    return _guarded(int(lib().dgpu_ans_max_compressed_size(nbytes)), nbytes)


def _guarded(size, n):
    # 0 = beyond getMaxCompressedSize's CHECK_LE(rawSize, INT32_MAX) (GpuANSEncode.cu:22; upstream aborts)
    _check(size != 0, f"input of {n} symbols: its maximum compressed size exceeds INT32_MAX (1717538816 is the largest)")
    return size


# -------------------------------------------------------------------- compress
def _validate_out(out_compressed, out_compressed_bytes, rows, cols, dev, device):
    if out_compressed is not None:
        oc = out_compressed
        _check(oc.dtype == torch.uint8 and oc.is_cuda and oc.is_contiguous() and oc.dim() == 2)
        _check(oc.size(0) >= rows and oc.size(1) >= cols and oc.get_device() == dev)
        comp = oc
    else:
        comp = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    if out_compressed_bytes is not None:
        ob = out_compressed_bytes
        _check(ob.dtype == torch.int32 and ob.is_cuda and ob.dim() == 1 and ob.is_contiguous())
        _check(ob.size(0) >= rows and ob.get_device() == dev)
        sizes = ob
    else:
        sizes = torch.empty((rows,), dtype=torch.int32, device=device)
    return comp, sizes


def compress_data(compress_as_float, ts_in, checksum=False, temp_mem=None, out_compressed=None,
                  out_compressed_bytes=None, prob_bits=K_DEFAULT_PRECISION):
    """DietGpu.cpp:149-308 -> (comp [B, maxSize] u8, sizes [B] i32, temp bytes used)."""
    fast = _fast_ops(prob_bits)
    if fast is not None:
        return fast.compress_data(compress_as_float, ts_in, checksum, temp_mem, out_compressed, out_compressed_bytes)
    _check(len(ts_in) > 0)
    dev = ts_in[0].get_device()
    rows, cols = (max_float_compressed_output_size(ts_in) if compress_as_float
                  else max_any_compressed_output_size(ts_in))
    for t in ts_in:
        _check(t.is_cuda and t.is_contiguous() and t.get_device() == dev)
        if compress_as_float:
            _check(t.dtype == ts_in[0].dtype)
            _float_type(t)
    with torch.cuda.device(dev):
        comp, sizes = _validate_out(out_compressed, out_compressed_bytes, rows, cols, dev, ts_in[0].device)
        tp, tb = _temp(temp_mem, dev)
        in_ptrs = _ptr_array(ts_in)
        row = comp.size(1)
        out_ptrs = (C.c_void_p * rows)(*[comp.data_ptr() + i * row for i in range(rows)])
        used = C.c_size_t(0)
        if compress_as_float:
            in_size = _u32_array([t.numel() for t in ts_in])
            check(lib().dgpu_float_compress(
                tp, tb, C.byref(used), _float_type(ts_in[0]), prob_bits, int(checksum), rows,
                in_ptrs, in_size, out_ptrs, _ptr(sizes), _stream()))
        else:
            in_size = _u32_array([t.numel() * t.element_size() for t in ts_in])
            check(lib().dgpu_ans_encode_batch_pointer(
                tp, tb, C.byref(used), prob_bits, int(checksum), rows, in_ptrs, in_size, None,
                out_ptrs, _ptr(sizes), _stream()))
    return comp, sizes, int(used.value)


def compress_data_split_size(compress_as_float, t_in, t_in_split_sizes, checksum=False,
                             temp_mem=None, out_compressed=None, out_compressed_bytes=None,
                             prob_bits=K_DEFAULT_PRECISION):
    """DietGpu.cpp:310-452 -> (list of compressed row views, sizes, temp bytes used)."""
    fast = _fast_ops(prob_bits)
    if fast is not None:
        return fast.compress_data_split_size(compress_as_float, t_in, t_in_split_sizes, checksum, temp_mem, out_compressed,
                                             out_compressed_bytes)
    dev = t_in.get_device()
    _check(t_in.is_cuda and t_in.is_contiguous())
    ft = _float_type(t_in) if compress_as_float else 0
    if not compress_as_float:
        _check(t_in.data_ptr() % 4 == 0, "start pointer is not aligned")
    ss = t_in_split_sizes
    _check(ss.is_contiguous() and not ss.is_cuda and ss.dtype == torch.int32)
    split = [int(v) for v in ss.tolist()]
    n = len(split)
    for i, s in enumerate(split):
        _check(s > 0)
        if not compress_as_float and i != n - 1:
            _check(s % 4 == 0, "the size of an interior split is not a multiple of the alignment")
    mx = max(split)
    cols = _guarded(int(lib().dgpu_float_max_compressed_size(ft, mx)) if compress_as_float
                    else int(lib().dgpu_ans_max_compressed_size(mx)), mx)
    with torch.cuda.device(dev):
        comp, sizes = _validate_out(out_compressed, out_compressed_bytes, n, cols, dev, t_in.device)
        tp, tb = _temp(temp_mem, dev)
        used = C.c_size_t(0)
        if compress_as_float:
            check(lib().dgpu_float_compress_split_size(
                tp, tb, C.byref(used), ft, prob_bits, int(checksum), n, _ptr(t_in),
                _u32_array(split), _ptr(comp), comp.size(1), _ptr(sizes), _stream()))
        else:
            check(lib().dgpu_ans_encode_batch_split_size(
                tp, tb, C.byref(used), prob_bits, int(checksum), n, _ptr(t_in), _u32_array(split),
                None, _ptr(comp), comp.size(1), _ptr(sizes), _stream()))
        # compressedMatrixToTensors, DietGpu.cpp:77-104
        host_sizes = sizes[:n].tolist()
        flat = comp.view(-1)
        outs = [flat.narrow(0, i * comp.size(1), host_sizes[i]) for i in range(n)]
    return outs, sizes, int(used.value)


def compress_data_simple(compress_as_float, ts_in, checksum=False, temp_mem=67108864,
                         prob_bits=K_DEFAULT_PRECISION):
    """DietGpu.cpp:454-522 -> list of exactly-sized compressed tensors."""
    fast = _fast_ops(prob_bits)
    if fast is not None:
        return fast.compress_data_simple(compress_as_float, ts_in, checksum, temp_mem)
    _check(len(ts_in) > 0)
    scratch = None
    if temp_mem is not None and temp_mem > 0:
        scratch = torch.empty((temp_mem,), dtype=torch.uint8, device=ts_in[0].device)
    comp, sizes, _ = compress_data(compress_as_float, ts_in, checksum, scratch, None, None,
                                   prob_bits=prob_bits)
    host = sizes.to("cpu").tolist()
    return [comp[i, : host[i]].clone() for i in range(len(ts_in))]


# ---------------------------------------------------------------- cast-compress
# (no reference op: dgpu_float_cast_compress, include/dietgpu_amd.h)
def compress_data_cast(ts_in, dtype, temp_mem=None, out_compressed=None, out_compressed_sizes=None,
                       prob_bits=K_DEFAULT_PRECISION):
    """Compresses float32 tensors into ordinary float16 / bfloat16 archives (`dtype`: of the archives): every word is
    rounded to `dtype` in registers -- round to nearest even, NaN to the canonical quiet NaN with its sign -- and the
    archive is byte for byte what `compress_data(True, [t.to(dtype)])` writes for the rounded tensor, without the
    16-bit scratch tensor -> (comp [B, maxSize] u8, sizes [B] i32, temp bytes used), as compress_data.  ts_in is not
    modified.  There is no `checksum`: a checksum covers the 16-bit words, which never reach memory here."""
    _check(len(ts_in) > 0)
    _check(dtype in (torch.float16, torch.bfloat16), "dtype (of the archives) must be float16 or bfloat16")
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    ft = _DTYPE_TO_FT[dtype]
    dev = ts_in[0].get_device()
    for t in ts_in:
        _check(t.is_cuda and t.is_contiguous() and t.get_device() == dev)
        _check(t.dtype == torch.float32, "the inputs of a cast call must be float32")
    op = _amd_op(prob_bits, "compress_data_cast")
    if op is not None:
        return op(ts_in, ft, temp_mem, out_compressed, out_compressed_sizes)
    _, mx = _total_and_max(ts_in)
    rows, cols = len(ts_in), _guarded(int(lib().dgpu_float_max_compressed_size(ft, mx)), mx)
    with torch.cuda.device(dev):
        comp, sizes = _validate_out(out_compressed, out_compressed_sizes, rows, cols, dev, ts_in[0].device)
        tp, tb = _temp(temp_mem, dev)
        row = comp.size(1)
        out_ptrs = (C.c_void_p * rows)(*[comp.data_ptr() + i * row for i in range(rows)])
        used = C.c_size_t(0)
        check(lib().dgpu_float_cast_compress(
            tp, tb, C.byref(used), ft, prob_bits, rows, _ptr_array(ts_in), _u32_array([t.numel() for t in ts_in]),
            out_ptrs, _ptr(sizes), _stream()))
    return comp, sizes, int(used.value)


# ------------------------------------------------------ feedback cast-compress
# (no reference op: dgpu_float_feedback_compress, include/dietgpu_amd.h)
def _validate_residuals(ts_in, ts_residual):
    _check(len(ts_residual) == len(ts_in), "one residual per tensor")
    for t, r in zip(ts_in, ts_residual):
        _check(r.dtype == torch.float32, "the residuals of a feedback call must be float32")
        _check(r.numel() == t.numel(), "a residual has its tensor's number of elements")
        _check(r.is_contiguous() and r.device == t.device, "a residual is contiguous and on its tensor's device")


def compress_data_feedback(ts_in, ts_residual, dtype, fresh=False, temp_mem=None, out_compressed=None,
                           out_compressed_sizes=None, prob_bits=K_DEFAULT_PRECISION):
    """compress_data_cast with error feedback: tensor i is compressed as `ts_in[i] + ts_residual[i]` (one float32 add)
    rounded to `dtype`, and ts_residual[i] -- float32, of the tensor's size -- is updated IN PLACE to what that rounding
    dropped (zero where the rounded word is an infinity or a NaN), for the next step.  `fresh=True`: there is no
    residual yet -- the buffers are only written and need not be initialised.  ts_in is not modified.
    -> (comp [B, maxSize] u8, sizes [B] i32, temp bytes used), as compress_data_cast."""
    _check(len(ts_in) > 0)
    _check(dtype in (torch.float16, torch.bfloat16), "dtype (of the archives) must be float16 or bfloat16")
    for t in ts_in:
        _check(t.dtype == torch.float32, "the inputs of a feedback call must be float32")
    _validate_residuals(ts_in, ts_residual)
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    ft = _DTYPE_TO_FT[dtype]
    dev = ts_in[0].get_device()
    for t in ts_in:
        _check(t.is_cuda and t.is_contiguous() and t.get_device() == dev)
    op = _amd_op(prob_bits, "compress_data_feedback")
    if op is not None:
        return op(ts_in, ts_residual, ft, bool(fresh), temp_mem, out_compressed, out_compressed_sizes)
    _, mx = _total_and_max(ts_in)
    rows, cols = len(ts_in), _guarded(int(lib().dgpu_float_max_compressed_size(ft, mx)), mx)
    with torch.cuda.device(dev):
        comp, sizes = _validate_out(out_compressed, out_compressed_sizes, rows, cols, dev, ts_in[0].device)
        tp, tb = _temp(temp_mem, dev)
        row = comp.size(1)
        out_ptrs = (C.c_void_p * rows)(*[comp.data_ptr() + i * row for i in range(rows)])
        res_ptrs = _ptr_array(ts_residual)
        used = C.c_size_t(0)
        check(lib().dgpu_float_feedback_compress(
            tp, tb, C.byref(used), ft, prob_bits, rows, _ptr_array(ts_in), _u32_array([t.numel() for t in ts_in]),
            None if fresh else res_ptrs, res_ptrs, out_ptrs, _ptr(sizes), _stream()))
    return comp, sizes, int(used.value)


# ---------------------------------------------------- stochastic cast-compress
# (no reference op: dgpu_float_stochastic_compress, include/dietgpu_amd.h)
def compress_data_stochastic(ts_in, dtype, seed, first_member=0, out_compressed=None, out_compressed_sizes=None,
                             prob_bits=K_DEFAULT_PRECISION):
    """compress_data_cast whose every rounding is STOCHASTIC: word k of float32 tensor i becomes its neighbour in `dtype`
    toward zero or the next one away from zero, the latter with probability remainder / unit -- unbiased, where round to
    nearest drops every component below half a unit the same way at every step and on every rank, and without the
    float32 residual of compress_data_feedback.  The archive is byte for byte what `compress_data(True, ...)` writes for
    `rounding.stochastic_round_` of the tensor with the random bits of (seed, first_member + i, k): an ordinary archive
    -> (comp [B, maxSize] u8, sizes [B] i32).  ts_in is not modified; no temp memory is passed (the call's temporaries
    are the stream's own); no checksum.

    The random bits are a pure function of (seed, first_member + i, k): the same tensors with the same seed give the
    same archives whatever the kernel geometry.  `seed`: an int in [0, 2^64), or a 1-element int64 CUDA tensor whose bits
    are the seed, read by the kernels when they run and never by the host -- a captured call advances the rounding by
    `seed.add_(1)` between replays (never while the call runs: both of its kernels read the word)."""
    _check(len(ts_in) > 0)
    _check(dtype in (torch.float16, torch.bfloat16), "dtype (of the archives) must be float16 or bfloat16")
    host_seed, dev_seed = _seed_arg(seed)
    _check(isinstance(first_member, int) and not isinstance(first_member, bool) and 0 <= first_member < (1 << 32),
           "first_member must be an int in [0, 2^32)")
    for t in ts_in:
        _check(t.dtype == torch.float32, "the inputs of a stochastic cast call must be float32")
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    ft = _DTYPE_TO_FT[dtype]
    dev = ts_in[0].get_device()
    _check(dev_seed is None or dev_seed.get_device() == dev, "a tensor seed must be on the tensors' GPU")
    for t in ts_in:
        _check(t.is_cuda and t.is_contiguous() and t.get_device() == dev)
    op = _amd_op(prob_bits, "compress_data_stochastic")
    if op is not None:
        return op(ts_in, ft, host_seed, dev_seed, first_member, out_compressed, out_compressed_sizes)
    _, mx = _total_and_max(ts_in)
    rows, cols = len(ts_in), _guarded(int(lib().dgpu_float_max_compressed_size(ft, mx)), mx)
    with torch.cuda.device(dev):
        comp, sizes = _validate_out(out_compressed, out_compressed_sizes, rows, cols, dev, ts_in[0].device)
        row = comp.size(1)
        out_ptrs = (C.c_void_p * rows)(*[comp.data_ptr() + i * row for i in range(rows)])
        check(lib().dgpu_float_stochastic_compress(
            ft, prob_bits, rows, _ptr_array(ts_in), _u32_array([t.numel() for t in ts_in]), host_seed & ((1 << 64) - 1),
            _ptr(dev_seed), first_member, out_ptrs, _ptr(sizes), _stream()))
    return comp, sizes


# ------------------------------------------------------- rolling-table compress
# (no reference op: dgpu_float_rolling_compress, include/dietgpu_amd.h)
def _validate_counts(counts, rows, dev, name):
    if counts is None:
        return
    _check(counts.dtype == torch.int32 and counts.is_cuda and counts.is_contiguous() and counts.get_device() == dev,
           f"{name} must be a contiguous int32 tensor on the tensors' GPU")
    _check(counts.dim() == 2 and counts.size(0) == rows and counts.size(1) == 256, f"{name} must be [len(ts_in), 256]")


def compress_data_rolling(ts_in, counts_in, counts_out, dtype=None, temp_mem=None, out_compressed=None,
                          out_compressed_sizes=None, prob_bits=K_DEFAULT_PRECISION):
    """compress_data(True, ts_in) -- or, with `dtype` given for float32 tensors, compress_data_cast(ts_in, dtype) -- for
    tensors that come back step after step.  `counts_in` (int32 [n, 256] on the GPU, or None): the exponent counts the
    last call left; the tables are made from them and no histogram pass reads the tensors.  `counts_out` (the same, or
    None): receives this call's counts, which the encoder takes while it codes.  The same tensor may be passed as both.
    Any counts give a lossless archive every decoder reads; only its size depends on how well they fit (and it is a few
    per cent above compress_data's even when they fit: every symbol keeps a probability).  With
    `counts_in` a size above `max_float_compressed_size` can be reported for tensors of millions of words whose counts
    fit nothing: that row is incomplete, compress again with counts_in=None.
    -> (comp [n, maxSize] u8, sizes [n] i32, temp bytes used), as compress_data."""
    _check(len(ts_in) > 0)
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    cast = dtype is not None
    if cast:
        _check(dtype in (torch.float16, torch.bfloat16), "dtype (of the archives) must be float16 or bfloat16")
    else:
        _check(ts_in[0].dtype in (torch.float16, torch.bfloat16), "tensors must be float16 or bfloat16 (float32: give dtype)")
    ft = _DTYPE_TO_FT[dtype if cast else ts_in[0].dtype]
    dev = ts_in[0].get_device()
    for t in ts_in:
        _check(t.is_cuda and t.is_contiguous() and t.get_device() == dev)
        _check(t.dtype == (torch.float32 if cast else ts_in[0].dtype),
               "the inputs of a cast call must be float32" if cast else "tensors must share one dtype")
    rows = len(ts_in)
    _validate_counts(counts_in, rows, dev, "counts_in")
    _validate_counts(counts_out, rows, dev, "counts_out")
    op = _amd_op(prob_bits, "compress_data_rolling")
    if op is not None:
        return op(ts_in, counts_in, counts_out, ft, cast, temp_mem, out_compressed, out_compressed_sizes)
    _, mx = _total_and_max(ts_in)
    cols = _guarded(int(lib().dgpu_float_max_compressed_size(ft, mx)), mx)
    with torch.cuda.device(dev):
        comp, sizes = _validate_out(out_compressed, out_compressed_sizes, rows, cols, dev, ts_in[0].device)
        tp, tb = _temp(temp_mem, dev)
        row = comp.size(1)
        out_ptrs = (C.c_void_p * rows)(*[comp.data_ptr() + i * row for i in range(rows)])
        used = C.c_size_t(0)
        check(lib().dgpu_float_rolling_compress(
            tp, tb, C.byref(used), ft, int(cast), prob_bits, rows, _ptr_array(ts_in), _u32_array([t.numel() for t in ts_in]),
            _ptr(counts_in), _ptr(counts_out), out_ptrs, _ptr(sizes), _stream()))
    return comp, sizes, int(used.value)


# ------------------------------------------------------------------ decompress
def _validate_status(out_status, out_sizes, n, dev):
    if out_status is not None:
        _check(out_status.is_contiguous() and out_status.is_cuda and out_status.dtype == torch.uint8)
        _check(out_status.numel() == n and out_status.get_device() == dev)
    if out_sizes is not None:
        _check(out_sizes.is_contiguous() and out_sizes.is_cuda and out_sizes.dtype == torch.int32)
        _check(out_sizes.numel() == n and out_sizes.get_device() == dev)


def _raise_checksum(rc, is_float):
    if rc == 3:  # DGPU_ERR_CHECKSUM_MISMATCH
        raise RuntimeError(
            ("floatDecompress" if is_float else "ANSDecode")
            + ": checksum mismatch seen on decoded data; archive cannot be unpacked\n"
            + lib().dgpu_last_error().decode())
    check(rc)


def _decode_capacities(compress_as_float, ts_in, ts_out, dev, same_dtype=False):
    """The per-tensor checks of a decode call -> the capacity of every output (words of floats, else bytes)."""
    caps = []
    for ti, to in zip(ts_in, ts_out):
        _check(ti.is_cuda and ti.get_device() == dev and ti.is_contiguous())
        _check(to.is_cuda and to.get_device() == dev and to.is_contiguous())
        _check(ti.dtype == torch.uint8)
        if compress_as_float:
            _float_type(to)
            _check(not same_dtype or to.dtype == ts_out[0].dtype)
        cap = to.numel() if compress_as_float else to.numel() * to.element_size()
        _check(cap <= _U32_MAX)
        caps.append(cap)
    return caps


def _header_info(compress_as_float, ts_in, tp, tb):
    """-> (sizes, float types) of the archives as host lists, read from their headers (one synchronising copy)"""
    n, device = len(ts_in), ts_in[0].device
    sizes = torch.empty((n,), dtype=torch.int32, device=device)
    types = torch.zeros((n,), dtype=torch.int32, device=device)
    if compress_as_float:
        check(lib().dgpu_float_get_compressed_info(tp, tb, _ptr_array(ts_in), n, _ptr(sizes), _ptr(types), None, _stream()))
    else:
        check(lib().dgpu_ans_get_compressed_info(tp, tb, _ptr_array(ts_in), n, _ptr(sizes), None, _stream()))
    return sizes.tolist(), types.tolist()


def decompress_data(compress_as_float, ts_in, ts_out, checksum=False, temp_mem=None,
                    out_status=None, out_decompressed_words=None, prob_bits=K_DEFAULT_PRECISION):
    """DietGpu.cpp:530-677 -> temp bytes used."""
    fast = _fast_ops(prob_bits)
    if fast is not None:
        return fast.decompress_data(compress_as_float, ts_in, ts_out, checksum, temp_mem, out_status, out_decompressed_words)
    _check(len(ts_in) > 0)
    _check(len(ts_in) == len(ts_out))
    dev = ts_in[0].get_device()
    caps = _decode_capacities(compress_as_float, ts_in, ts_out, dev)
    n = len(ts_in)
    _validate_status(out_status, out_decompressed_words, n, dev)
    with torch.cuda.device(dev):
        tp, tb = _temp(temp_mem, dev)
        used = C.c_size_t(0)
        err = C.c_int32(-1)
        if compress_as_float:
            rc = lib().dgpu_float_decompress_bounded(
                tp, tb, C.byref(used), _float_type(ts_out[0]), prob_bits, int(checksum), n,
                _ptr_array(ts_in), _in_bytes(ts_in), _ptr_array(ts_out), _u32_array(caps), _ptr(out_status),
                _ptr(out_decompressed_words), _stream(), C.byref(err))
        else:
            rc = lib().dgpu_ans_decode_batch_pointer_bounded(
                tp, tb, C.byref(used), prob_bits, int(checksum), n, _ptr_array(ts_in), _in_bytes(ts_in),
                _ptr_array(ts_out), _u32_array(caps), _ptr(out_status),
                _ptr(out_decompressed_words), _stream(), C.byref(err))
        _raise_checksum(rc, compress_as_float)
    return int(used.value)


def decompress_data_split_size(compress_as_float, ts_in, t_out, t_out_split_sizes, checksum=False,
                               temp_mem=None, out_status=None, out_decompressed_words=None,
                               prob_bits=K_DEFAULT_PRECISION):
    """DietGpu.cpp:679-816 -> temp bytes used."""
    fast = _fast_ops(prob_bits)
    if fast is not None:
        return fast.decompress_data_split_size(compress_as_float, ts_in, t_out, t_out_split_sizes, checksum, temp_mem, out_status,
                                               out_decompressed_words)
    _check(len(ts_in) > 0)
    dev = ts_in[0].get_device()
    ss = t_out_split_sizes
    _check(ss.is_contiguous() and not ss.is_cuda and ss.dtype == torch.int32)
    split = [int(v) for v in ss.tolist()]
    n = len(split)
    _check(n == len(ts_in))
    for ti, s in zip(ts_in, split):
        _check(ti.is_cuda and ti.get_device() == dev and ti.is_contiguous() and ti.dtype == torch.uint8)
        _check(s > 0)
    _check(t_out.is_cuda and t_out.get_device() == dev and t_out.is_contiguous())
    if compress_as_float:
        _float_type(t_out)
    _validate_status(out_status, out_decompressed_words, n, dev)
    with torch.cuda.device(dev):
        tp, tb = _temp(temp_mem, dev)
        used = C.c_size_t(0)
        err = C.c_int32(-1)
        if compress_as_float:
            rc = lib().dgpu_float_decompress_split_size_bounded(
                tp, tb, C.byref(used), _float_type(t_out), prob_bits, int(checksum), n,
                _ptr_array(ts_in), _in_bytes(ts_in), _ptr(t_out), _u32_array(split), _ptr(out_status),
                _ptr(out_decompressed_words), _stream(), C.byref(err))
        else:
            rc = lib().dgpu_ans_decode_batch_split_size_bounded(
                tp, tb, C.byref(used), prob_bits, int(checksum), n, _ptr_array(ts_in), _in_bytes(ts_in), _ptr(t_out),
                _u32_array(split), _ptr(out_status), _ptr(out_decompressed_words), _stream(),
                C.byref(err))
        _raise_checksum(rc, compress_as_float)
    return int(used.value)


def decompress_data_simple(compress_as_float, ts_in, checksum=False, temp_mem=67108864,
                           prob_bits=K_DEFAULT_PRECISION):
    """DietGpu.cpp:818-911 -> list of decompressed tensors (sizes/dtypes read from the headers)."""
    fast = _fast_ops(prob_bits)
    if fast is not None:
        return fast.decompress_data_simple(compress_as_float, ts_in, checksum, temp_mem)
    _check(len(ts_in) > 0)
    dev = ts_in[0].get_device()
    device = ts_in[0].device
    n = len(ts_in)
    for t in ts_in:
        _check(t.is_cuda and t.get_device() == dev and t.is_contiguous())
    with torch.cuda.device(dev):
        scratch = None
        if temp_mem is not None and temp_mem >= 256:  # kSDMAlignment, DietGpu.cpp:831-834
            scratch = torch.empty((temp_mem,), dtype=torch.uint8, device=device)
        hs, ht = _header_info(compress_as_float, ts_in, *_temp(scratch, dev))
        outs = []
        for i in range(n):
            if compress_as_float:
                _check(ht[i] == ht[0])  # must be a consistent dtype
                outs.append(torch.empty((hs[i],), dtype=_FT_TO_DTYPE[ht[i]], device=device))
            else:
                outs.append(torch.empty((hs[i],), dtype=torch.uint8, device=device))
    decompress_data(compress_as_float, ts_in, outs, checksum, scratch, None, None, prob_bits=prob_bits)
    return outs


# ------------------------------------------------------------- ranged decompress
# (no reference op: dgpu_ans_decode_batch_pointer_range / dgpu_float_decompress_range, include/dietgpu_amd.h)
BLOCK_WORDS = 4096  # the format's block: the unit a range is decoded in


def block_cover(start, count):
    """The blocks that hold words [start, start + count) of an element -> (first_block, num_blocks, offset): the range
    begins `offset` words into block `first_block`.  Pure; a count of 0 covers no block."""
    _check(start >= 0 and count >= 0, "start and count must not be negative")
    first = start // BLOCK_WORDS
    last = (start + count + BLOCK_WORDS - 1) // BLOCK_WORDS if count else first
    return first, last - first, start - first * BLOCK_WORDS


def decompress_data_range(compress_as_float, ts_in, ts_out, first_block, num_blocks, temp_mem=None, out_status=None,
                          out_decompressed_words=None, prob_bits=K_DEFAULT_PRECISION):
    """Decodes blocks [first_block[i], first_block[i] + num_blocks[i]) of archive i -- 4096 words each -- into ts_out[i],
    which holds the range (block first_block + k at word k * 4096), without reading the rest of the archive -> temp bytes
    used (0).  num_blocks[i] < 0 or 2**32 - 1: to the end of the element; a range that runs past the end is clipped.
    out_status[i] is 0 when the range begins past the end, does not fit ts_out[i] or the archive is malformed;
    out_decompressed_words[i] is the size of the clipped range.  There is no `checksum`: a checksum covers the whole
    element and is ignored here."""
    _check(len(ts_in) > 0)
    _check(len(ts_in) == len(ts_out))
    first_block, num_blocks = list(first_block), list(num_blocks)
    _check(len(first_block) == len(ts_in) and len(num_blocks) == len(ts_in), "one first_block and num_blocks per tensor")
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    op = _amd_op(prob_bits, "decompress_data_range")
    if op is not None:
        # (the op makes the per-tensor checks below itself, and raises RuntimeError like them)
        return op(compress_as_float, ts_in, ts_out, first_block, num_blocks, temp_mem, out_status, out_decompressed_words)
    dev = ts_in[0].get_device()
    for f in first_block:
        _check(0 <= f <= _U32_MAX, "first_block out of range")
    caps = _decode_capacities(compress_as_float, ts_in, ts_out, dev, same_dtype=True)
    n = len(ts_in)
    counts = [_U32_MAX if (c < 0 or c >= _U32_MAX) else c for c in num_blocks]
    _validate_status(out_status, out_decompressed_words, n, dev)
    with torch.cuda.device(dev):
        tp, tb = _temp(temp_mem, dev)
        used = C.c_size_t(0)
        if compress_as_float:
            check(lib().dgpu_float_decompress_range(
                tp, tb, C.byref(used), _float_type(ts_out[0]), prob_bits, n, _ptr_array(ts_in), _in_bytes(ts_in),
                _u32_array(first_block), _u32_array(counts), _ptr_array(ts_out), _u32_array(caps), _ptr(out_status),
                _ptr(out_decompressed_words), _stream()))
        else:
            check(lib().dgpu_ans_decode_batch_pointer_range(
                tp, tb, C.byref(used), prob_bits, n, _ptr_array(ts_in), _in_bytes(ts_in), _u32_array(first_block),
                _u32_array(counts), _ptr_array(ts_out), _u32_array(caps), _ptr(out_status), _ptr(out_decompressed_words),
                _stream()))
    return int(used.value)


# ------------------------------------------------------------- decode-accumulate
# (no reference op: dgpu_float_decode_accumulate, include/dietgpu_amd.h)
def decompress_data_accumulate(ts_in, ts_acc, accumulate=True, temp_mem=None, out_status=None, out_sizes=None,
                               prob_bits=K_DEFAULT_PRECISION, dtype=None, scale=None):
    """Decodes float archive ts_in[i], widens every word to float32 and adds it into ts_acc[i] (accumulate=True: one IEEE
    float32 add per word) or stores it there (accumulate=False: the accumulator is not read -- a 16-bit archive straight
    into float32, and the first source of a sum) -> temp bytes used (0).  ts_acc: float32 CUDA tensors that do not overlap.

    One call decodes one float type: `dtype` if given (no host synchronisation: what a caller that knows its archives,
    or captures the call into a graph, passes), else the type in the header of ts_in[0], read with one synchronising
    copy (`_header_info`).  out_status[i] is 0, and ts_acc[i] untouched, for an archive of another type, a malformed or
    truncated one, or one that does not fit ts_acc[i]; out_sizes[i] is the size its header states.  There is no
    `checksum`: a checksum covers the 16-bit words, which never reach memory here, and is ignored.

    `scale` (dgpu_float_decode_accumulate_scaled): every widened word is multiplied by a float32 factor before it is
    stored or added, ts_acc[i][k] = [ts_acc[i][k] +] fl32(widen(word) * s) -- one IEEE float32 multiply and one IEEE add,
    each rounded once, never an FMA: bit for bit this call into a scratch, `mul_` by a 0-dim float32 tensor and `add_`.
    A Python number is rounded once to float32 and must be finite and not zero (None, or one whose float32 is 1.0, is the
    call without it); a float32 CUDA tensor on the tensors' device, contiguous, with 1 element (one factor for the call)
    or len(ts_in) elements (one per archive) is read by the kernel when it runs and never by the host: it may hold any
    value (a 1 multiplies), may be the result of work enqueued before this call, and a captured call follows the value it
    holds at each replay."""
    _check(len(ts_in) > 0)
    _check(len(ts_in) == len(ts_acc))
    host, dev_scale = _scale_arg(scale, len(ts_in))
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    dev = ts_in[0].get_device()
    _check(dev_scale is None or dev_scale.get_device() == dev, "a tensor scale must be on the tensors' GPU")
    for ti, ta in zip(ts_in, ts_acc):
        _check(ti.is_cuda and ti.get_device() == dev and ti.is_contiguous() and ti.dtype == torch.uint8)
        _check(ta.is_cuda and ta.get_device() == dev and ta.is_contiguous(), "accumulators must be contiguous tensors on the GPU")
        _check(ta.dtype == torch.float32, "accumulators must be float32")
        _check(ta.numel() <= _U32_MAX)
    n = len(ts_in)
    _validate_status(out_status, out_sizes, n, dev)
    with torch.cuda.device(dev):
        tp, tb = _temp(temp_mem, dev)
        if dtype is not None:
            _check(dtype in _DTYPE_TO_FT, "dtype must be float16, bfloat16 or float32")
            ft = _DTYPE_TO_FT[dtype]
        else:
            ft = _header_info(True, ts_in[:1], tp, tb)[1][0]
            _check(ft in _FT_TO_DTYPE, "ts_in[0] is not a float archive")
        used = C.c_size_t(0)
        if host is not None:
            op = _amd_op(prob_bits, "decompress_data_accumulate_scaled")
            if op is not None:
                return op(ts_in, ts_acc, ft, bool(accumulate), host, dev_scale, temp_mem, out_status, out_sizes)
            check(lib().dgpu_float_decode_accumulate_scaled(
                tp, tb, C.byref(used), ft, prob_bits, int(bool(accumulate)), n, _ptr_array(ts_in), _in_bytes(ts_in),
                _ptr_array(ts_acc), _u32_array([t.numel() for t in ts_acc]), host, _ptr(dev_scale),
                0 if dev_scale is None or dev_scale.numel() == 1 else 1, _ptr(out_status), _ptr(out_sizes), _stream()))
            return int(used.value)
        op = _amd_op(prob_bits, "decompress_data_accumulate")
        if op is not None:
            return op(ts_in, ts_acc, ft, bool(accumulate), temp_mem, out_status, out_sizes)
        check(lib().dgpu_float_decode_accumulate(
            tp, tb, C.byref(used), ft, prob_bits, int(bool(accumulate)), n, _ptr_array(ts_in), _in_bytes(ts_in),
            _ptr_array(ts_acc), _u32_array([t.numel() for t in ts_acc]), _ptr(out_status), _ptr(out_sizes), _stream()))
    return int(used.value)


# ------------------------------------------------------------- scaled decompress
# (no reference op: dgpu_float_decode_scaled, include/dietgpu_amd.h)
def decompress_data_scaled(ts_in, ts_out, scale, temp_mem=None, out_status=None, out_decompressed_words=None,
                           prob_bits=K_DEFAULT_PRECISION):
    """decompress_data(True, ts_in, ts_out) whose every word is multiplied by a float32 factor before it is stored:
    ts_out[i][k] = round_T(fl32(widen(word) * s)) -- one IEEE float32 multiply and one rounding to the tensors' dtype T
    (nearest even, float16 denormals produced, overflow to infinity; a NaN product is a quiet NaN) -> temp bytes used (0).

    `scale`: a Python number, rounded once to float32, which must be finite and not zero (one whose float32 is 1.0, or
    None, is the plain decompress_data call); or a float32 CUDA tensor on the tensors' device, contiguous, with 1 element
    (one factor for the call) or len(ts_in) elements (one per archive).  A tensor is read by the kernel when it runs and
    never by the host: it may hold any value, it may be the result of work enqueued before this call (a clip
    coefficient), and a captured call follows the value it holds at each replay.  All ts_out share one float dtype.
    Status, sizes and the archive checks are decompress_data's.  There is no `checksum`: a checksum covers the stored
    words of the original tensor, which this call does not leave."""
    _check(len(ts_in) > 0)
    _check(len(ts_in) == len(ts_out))
    n = len(ts_in)
    host, dev_scale = _scale_arg(scale, n)
    if host is None:
        return decompress_data(True, ts_in, ts_out, False, temp_mem, out_status, out_decompressed_words, prob_bits=prob_bits)
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    dev = ts_in[0].get_device()
    _check(dev_scale is None or dev_scale.get_device() == dev, "a tensor scale must be on the tensors' GPU")
    op = _amd_op(prob_bits, "decompress_data_scaled")
    if op is not None:
        # (the op makes the per-tensor checks below itself, and raises RuntimeError like them)
        return op(ts_in, ts_out, host, dev_scale, temp_mem, out_status, out_decompressed_words)
    caps = _decode_capacities(True, ts_in, ts_out, dev, same_dtype=True)
    _validate_status(out_status, out_decompressed_words, n, dev)
    with torch.cuda.device(dev):
        tp, tb = _temp(temp_mem, dev)
        used = C.c_size_t(0)
        check(lib().dgpu_float_decode_scaled(
            tp, tb, C.byref(used), _float_type(ts_out[0]), prob_bits, n, _ptr_array(ts_in), _in_bytes(ts_in),
            _ptr_array(ts_out), _u32_array(caps), host, _ptr(dev_scale), 0 if dev_scale is None or dev_scale.numel() == 1 else 1,
            _ptr(out_status), _ptr(out_decompressed_words), _stream()))
    return int(used.value)


# ------------------------------------------------------------------ decode-update
# (no reference op: dgpu_float_decode_update, include/dietgpu_amd.h)
def _seed_arg(seed):
    """The `seed` of decode-update -> (the 64 seed bits as a signed int, device tensor or None).  An int in [0, 2^64), or a
    1-element int64 CUDA tensor whose bits are the seed and which is not read."""
    if isinstance(seed, torch.Tensor):
        _check(seed.dtype == torch.int64 and seed.numel() == 1, "a tensor seed must be a 1-element int64 tensor")
        _check(seed.is_cuda and seed.is_contiguous(), "a tensor seed must be a contiguous tensor on the tensors' GPU")
        return 0, seed
    _check(isinstance(seed, int) and not isinstance(seed, bool), "seed must be an int or a 1-element int64 tensor")
    _check(0 <= seed < (1 << 64), "seed must be in [0, 2^64)")
    return (seed - (1 << 64) if seed >= (1 << 63) else seed), None


def decompress_data_update(ts_in, ts_out, seed, scale=None, accumulate=True, first_member=0, out_status=None, out_sizes=None,
                           prob_bits=K_DEFAULT_PRECISION):
    """Decodes 16-bit float archive ts_in[i], multiplies every word by a float32 factor, adds it to the 16-bit tensor
    ts_out[i] of the archive's type (accumulate=True) or stores it there (False: the tensor is not read), and rounds the
    result STOCHASTICALLY to that type: ts_out[i][k] = sround_T([widen(ts_out[i][k]) +] fl32(widen(word) * s)) -- one
    IEEE float32 multiply and one IEEE add, never an FMA; the result is the neighbour of the sum toward zero or the next
    one away from zero, the latter with probability remainder / unit (`dietgpu_amd.rounding` restates the rule in torch)
    -> 0 (no temp memory is used).  With s = -lr * coef it is the SGD update of bfloat16 parameters without a float32
    master copy.  ts_out: float16 or bfloat16 CUDA tensors of one dtype that do not overlap.

    The random bits are a pure function of (seed, first_member + i, k): the same archives with the same seed give the
    same bits on every replica.  `seed`: an int in [0, 2^64), or a 1-element int64 CUDA tensor whose bits are the seed,
    read by the kernel when it runs -- a captured call advances the rounding by `seed.add_(1)`.  `scale`: as in
    decompress_data_scaled; None is 1.0.  out_status[i] is 0, and ts_out[i] keeps every bit, for an archive of another
    type, a malformed or truncated one, or one that does not fit; out_sizes[i] is the size its header states."""
    _check(len(ts_in) > 0)
    _check(len(ts_in) == len(ts_out))
    n = len(ts_in)
    host, dev_scale = _scale_arg(scale, n)
    if host is None:
        host = 1.0
    host_seed, dev_seed = _seed_arg(seed)
    _check(isinstance(first_member, int) and 0 <= first_member < (1 << 32), "first_member must be an int in [0, 2^32)")
    _check(ts_in[0].is_cuda, "tensors must be on the GPU")
    dev = ts_in[0].get_device()
    _check(dev_scale is None or dev_scale.get_device() == dev, "a tensor scale must be on the tensors' GPU")
    _check(dev_seed is None or dev_seed.get_device() == dev, "a tensor seed must be on the tensors' GPU")
    _check(ts_out[0].dtype in (torch.float16, torch.bfloat16), "decode-update takes float16 or bfloat16 tensors")
    op = _amd_op(prob_bits, "decompress_data_update")
    if op is not None:
        # (the op makes the per-tensor checks below itself, and raises RuntimeError like them)
        return op(ts_in, ts_out, host, dev_scale, host_seed, dev_seed, first_member, bool(accumulate), out_status, out_sizes)
    caps = _decode_capacities(True, ts_in, ts_out, dev, same_dtype=True)
    _validate_status(out_status, out_sizes, n, dev)
    with torch.cuda.device(dev):
        check(lib().dgpu_float_decode_update(
            _float_type(ts_out[0]), prob_bits, int(bool(accumulate)), n, _ptr_array(ts_in), _in_bytes(ts_in), _ptr_array(ts_out),
            _u32_array(caps), host, _ptr(dev_scale), 0 if dev_scale is None or dev_scale.numel() == 1 else 1,
            host_seed & ((1 << 64) - 1), _ptr(dev_seed), first_member, _ptr(out_status), _ptr(out_sizes), _stream()))
    return 0


# ------------------------------------------------------------------ decode-reduce
# (no reference op: dgpu_float_decode_reduce, include/dietgpu_amd.h)
MAX_REDUCE_SOURCES = 64


def _scale32(scale):
    """The `scale` keyword of the reduce calls -> None (no scale given, or one whose float32 is 1.0: the unscaled call) or
    the factor rounded ONCE to float32, which must be finite and not zero."""
    if scale is None:
        return None
    f = C.c_float(float(scale)).value
    _check(math.isfinite(f) and f != 0.0, "scale must be finite and not zero")
    return None if f == 1.0 else f


def _scale_arg(scale, n):
    """The `scale` of the scaled decode calls over n archives -> (host float, device tensor or None); (None, None): the
    call without a factor (None, or a number whose float32 is 1.0).  A tensor is float32, contiguous, on the GPU, with 1
    or n elements, and is not read; a number is rounded once to float32 and must be finite and not zero."""
    if isinstance(scale, torch.Tensor):
        _check(scale.dtype == torch.float32, "a tensor scale must be float32")
        _check(scale.numel() in (1, n), "a tensor scale holds 1 element or one per archive")
        _check(scale.is_cuda and scale.is_contiguous(), "a tensor scale must be a contiguous tensor on the tensors' GPU")
        return 1.0, scale
    try:
        return _scale32(scale), None
    except (TypeError, ValueError):
        raise RuntimeError("scale must be a number or a float32 tensor") from None


def _norm_outputs(out_sumsq, out_nonfinite, n, dev=None):
    """The `out_sumsq` / `out_nonfinite` keywords of the reduce calls -> whether either is given.  float64 [n] and int32
    [n], contiguous, on the GPU (`dev` given: on that one).  Dtype and shape are looked at first."""
    given = [(t, dt, name) for t, dt, name in ((out_sumsq, torch.float64, "out_sumsq"), (out_nonfinite, torch.int32, "out_nonfinite")) if t is not None]
    for t, dt, name in given:
        _check(isinstance(t, torch.Tensor) and t.dtype == dt, f"{name} must be a tensor of dtype {str(dt).replace('torch.', '')}")
        _check(t.dim() == 1 and t.numel() == n and t.is_contiguous(), f"{name} must be a contiguous tensor of shape [{n}], one entry per accumulator")
    for t, dt, name in given:
        _check(t.is_cuda and (dev is None or t.get_device() == dev), f"{name} must be on the GPU of the other tensors")
    return out_sumsq is not None or out_nonfinite is not None


def _mixed_sources(ts_in, ts_acc, dtype, allowed, raw_allowed=True):
    """Checks of the reduce calls -> (flat member-major sources, sources per accumulator, device, float type or None).
    A uint8 tensor is an archive; with `raw_allowed`, a 1-D tensor of the call's float dtype is a raw row.  The float type
    is `dtype`, else that of the first raw row, else None (the caller reads it from the first archive's header)."""
    _check(len(ts_in) > 0)
    _check(len(ts_in) == len(ts_acc), "one list of sources per accumulator")
    sources = len(ts_in[0])
    _check(1 <= sources <= MAX_REDUCE_SOURCES, "between 1 and 64 sources per accumulator")
    for srcs in ts_in:
        _check(len(srcs) == sources, "every accumulator takes the same number of sources")
    flat = [t for srcs in ts_in for t in srcs]  # member-major
    _check(flat[0].is_cuda, "tensors must be on the GPU")
    dev = flat[0].get_device()
    if dtype is not None and dtype not in allowed:  # (the message is not built for a call that passes)
        _check(False, "dtype must be one of " + ", ".join(str(d).replace("torch.", "") for d in allowed))
    if dtype is None:
        dtype = next((t.dtype for t in flat if t.dtype != torch.uint8), None)
    # (these two loops are most of a warm call's host time: the checks that pass make no function call)
    for ti in flat:
        if not (ti.is_cuda and ti.get_device() == dev and ti.is_contiguous()):
            raise RuntimeError("sources must be contiguous tensors on one GPU")
        if ti.dtype != torch.uint8:
            _check(raw_allowed, "sources must be uint8 archives")
            _check(ti.dtype == dtype and dtype in allowed, "a source is a uint8 archive or a raw row of the call's float dtype")
            _check(ti.dim() == 1, "a raw source must be 1-D")
            _check(ti.numel() * ti.element_size() <= _U32_MAX)
    for ta in ts_acc:
        if not (ta.is_cuda and ta.get_device() == dev and ta.is_contiguous()):
            raise RuntimeError("accumulators must be contiguous tensors on the GPU")
        if ta.dtype != torch.float32:
            raise RuntimeError("accumulators must be float32")
        _check(ta.numel() <= _U32_MAX)
    return flat, sources, dev, (_DTYPE_TO_FT[dtype] if dtype is not None else None)


def _source_kinds(flat):
    return _cached_array(C.c_uint8, tuple(0 if t.dtype == torch.uint8 else 1 for t in flat))


# (norm outputs given, scale given, raw rows allowed) -> what the names of the torch op and of the C entry point end in.
# The norm kernels are forms of the scaled ones and the scaled of the mixed, which take all-archive members as well.
_REDUCE_ENTRY = {
    (False, False, False): "", (False, False, True): "_mixed",
    (False, True, False): "_scaled", (False, True, True): "_scaled",
    (True, False, False): "_norm", (True, False, True): "_norm", (True, True, False): "_norm", (True, True, True): "_norm",
}


def _reduce_call(ts_in, ts_acc, raw_allowed, compress, accumulate, temp_mem, out_status, out_sizes, out_compressed,
                 out_compressed_sizes, prob_bits, dtype, scale, out_sumsq, out_nonfinite):
    """The eight reduce calls: dgpu_float_decode_reduce{,_mixed,_scaled,_norm}, or with `compress`
    dgpu_float_reduce_compress{,_mixed,_scaled,_norm}, through the torch op of the same name where there is one
    -> temp bytes used, or with `compress` (comp, sizes, temp bytes used).  Every argument is checked here, once."""
    scale = _scale32(scale)
    norm = _norm_outputs(out_sumsq, out_nonfinite, len(ts_acc))
    allowed = (torch.float16, torch.bfloat16) if compress else (torch.float16, torch.bfloat16, torch.float32)
    flat, sources, dev, ft = _mixed_sources(ts_in, ts_acc, dtype, allowed, raw_allowed)
    n = len(ts_acc)
    _validate_status(out_status, out_sizes, n, dev)
    if norm:  # (now that the device is known)
        _norm_outputs(out_sumsq, out_nonfinite, n, dev)
    entry = _REDUCE_ENTRY[norm, scale is not None, raw_allowed]
    factor = [] if not (norm or scale is not None) else [1.0 if scale is None else scale]
    norm_out = [out_sumsq, out_nonfinite] if norm else []
    with torch.cuda.device(dev):
        tp, tb = _temp(temp_mem, dev)
        if ft is None:
            ft = _header_info(True, flat[:1], tp, tb)[1][0]
            _check(_FT_TO_DTYPE.get(ft) in allowed, "ts_in[0][0] is not a float16 / bfloat16 archive" if compress else "ts_in[0][0] is not a float archive")
        op = _amd_op(prob_bits, ("decompress_data_reduce_compress" if compress else "decompress_data_reduce") + entry)
        if op is not None:
            return op(flat, sources, ts_acc, ft, *factor, bool(accumulate), temp_mem, out_status, out_sizes,
                      *([out_compressed, out_compressed_sizes] if compress else []), *norm_out)
        caps = _u32_array([t.numel() for t in ts_acc])
        archives, archive_sizes = [], []
        if compress:
            _, mx = _total_and_max(ts_acc)
            cols = _guarded(int(lib().dgpu_float_max_compressed_size(ft, mx)), mx)
            comp, sizes = _validate_out(out_compressed, out_compressed_sizes, n, cols, dev, ts_acc[0].device)
            row = comp.size(1)
            archives, archive_sizes = [(C.c_void_p * n)(*[comp.data_ptr() + i * row for i in range(n)])], [_ptr(sizes)]
        used = C.c_size_t(0)
        check(getattr(lib(), ("dgpu_float_reduce_compress" if compress else "dgpu_float_decode_reduce") + entry)(
            tp, tb, C.byref(used), ft, prob_bits, int(bool(accumulate)), n, sources, _ptr_array(flat), _in_bytes(flat),
            *([_source_kinds(flat)] if entry else []), *factor, _ptr_array(ts_acc), caps, *archives, _ptr(out_status), _ptr(out_sizes),
            *archive_sizes, *[_ptr(t) for t in norm_out], _stream()))
    return (comp, sizes, int(used.value)) if compress else int(used.value)


def decompress_data_reduce(ts_in, ts_acc, accumulate=False, temp_mem=None, out_status=None, out_sizes=None,
                           prob_bits=K_DEFAULT_PRECISION, dtype=None, scale=None, out_sumsq=None, out_nonfinite=None):
    """Sums SEVERAL float archives per accumulator in one launch: ts_in is a list, one entry per accumulator, of equally
    long lists of uint8 CUDA tensors (at most 64 each); ts_acc[i] = ((ts_acc[i] + x0) + x1) + ... with accumulate=True,
    (x0 + x1) + ... with accumulate=False -- the first source is then STORED, the accumulator is never read and no
    memset is needed.  Strictly left to right, one IEEE float32 add per word and source: bit for bit what one
    `decompress_data_accumulate` call per source leaves -> temp bytes used (0).

    All or nothing per accumulator: out_status[i] is 1 only if every source of ts_in[i] is a sound archive of the
    call's float type that fits ts_acc[i] and all of them hold the same number of words; otherwise it is 0 and
    ts_acc[i] keeps every bit it had.  out_sizes[i] is the size the header of ts_in[i][0] states.  `dtype` as in
    decompress_data_accumulate (given: no host synchronisation; else read from the header of ts_in[0][0]).

    `scale`: every word of a successful accumulator is left as fl32(sum * scale) -- one IEEE float32 multiply in the
    reduce kernel, on the last source's store; with accumulate=True it covers the old contents too.  None, or a value
    whose float32 is 1.0, is the unscaled call; anything else is rounded once to float32 and must be finite and not
    zero (RuntimeError).

    `out_sumsq` (float64 [n]) / `out_nonfinite` (int32 [n]), either or both: the call also leaves, per accumulator, the
    sum of squares of the FINITE float32 words it left there (the words the sources state; squares and sum in float64,
    within relative words * 2**-52 of the exact value) and the number of words that are inf or NaN -- what clipping by
    global norm and the overflow check of loss scaling otherwise read the shard again for.  A member with out_status 0
    gets 0.0 and 0.  The same call leaves the same bits every time."""
    return _reduce_call(ts_in, ts_acc, False, False, accumulate, temp_mem, out_status, out_sizes, None, None, prob_bits, dtype, scale,
                        out_sumsq, out_nonfinite)


# ---------------------------------------------------------------- reduce-compress
# (no reference op: dgpu_float_reduce_compress, include/dietgpu_amd.h)
def decompress_data_reduce_compress(ts_in, ts_acc, accumulate=False, temp_mem=None, out_status=None, out_sizes=None,
                                    out_compressed=None, out_compressed_sizes=None, prob_bits=K_DEFAULT_PRECISION, dtype=None,
                                    scale=None, out_sumsq=None, out_nonfinite=None):
    """`decompress_data_reduce(ts_in, ts_acc, accumulate)` and `compress_data_cast(ts_acc, dtype)` in ONE call: the sums
    land in the float32 accumulators and, rounded to `dtype`, in archives of the sources' own type, without the second
    read of the accumulators that the cast histogram makes -> (comp [n, maxSize] u8, sizes [n] i32, temp bytes used), as
    compress_data_cast.  ts_in, ts_acc, accumulate, out_status and out_sizes as in decompress_data_reduce, with one
    difference: every source must hold EXACTLY ts_acc[i].numel() words (fewer: out_status[i] = 0).  The accumulators
    and, for members with out_status 1, the archives are bit for bit what the two calls leave.  A failed member keeps
    its accumulator; its archive is a valid one of whatever the accumulator holds -- look at out_status.  `dtype`:
    float16 or bfloat16, of the sources and of the archives (given: no host synchronisation; else read from the header
    of ts_in[0][0]).  `scale` as in decompress_data_reduce: the accumulators hold the scaled sums, and the archives are
    those of the scaled sums, rounded once.  `out_sumsq` / `out_nonfinite` as in decompress_data_reduce, but of the words
    of the ARCHIVES -- the sums rounded to `dtype` -- which is the tensor every rank holds after the all-gather: a float32
    sum that is finite and rounds to a float16 infinity counts as non-finite."""
    return _reduce_call(ts_in, ts_acc, False, True, accumulate, temp_mem, out_status, out_sizes, out_compressed, out_compressed_sizes,
                        prob_bits, dtype, scale, out_sumsq, out_nonfinite)


# ------------------------------------------------------------------ mixed sources
# (no reference ops: dgpu_float_decode_reduce_mixed / dgpu_float_reduce_compress_mixed, include/dietgpu_amd.h)
def decompress_data_reduce_mixed(ts_in, ts_acc, accumulate=False, temp_mem=None, out_status=None, out_sizes=None,
                                 prob_bits=K_DEFAULT_PRECISION, dtype=None, scale=None, out_sumsq=None, out_nonfinite=None):
    """`decompress_data_reduce` whose sources may be UNCOMPRESSED: an entry of ts_in[i] is a uint8 archive or a raw row --
    a 1-D contiguous tensor of the call's float dtype, aligned to its element size only -- which is widened and added in
    its place in source order.  Bit for bit what decompress_data_reduce leaves when every raw row is replaced by its
    archive.  A raw row's numel() counts as the size a header states (all sources equal, at most ts_acc[i].numel(),
    reported in out_sizes[i] when it is the first source).  Raw rows must not overlap the accumulators.  `dtype`: given,
    else that of the first raw row, else read from the header of the first archive -> temp bytes used (0; with the norm
    outputs, their tile partials).  `scale`, `out_sumsq` and `out_nonfinite` as in decompress_data_reduce."""
    return _reduce_call(ts_in, ts_acc, True, False, accumulate, temp_mem, out_status, out_sizes, None, None, prob_bits, dtype, scale,
                        out_sumsq, out_nonfinite)


def decompress_data_reduce_compress_mixed(ts_in, ts_acc, accumulate=False, temp_mem=None, out_status=None, out_sizes=None,
                                          out_compressed=None, out_compressed_sizes=None, prob_bits=K_DEFAULT_PRECISION,
                                          dtype=None, scale=None, out_sumsq=None, out_nonfinite=None):
    """`decompress_data_reduce_compress` whose sources may be uncompressed rows, as in decompress_data_reduce_mixed (every
    source, raw or not, must hold EXACTLY ts_acc[i].numel() words) -> (comp, sizes, temp bytes used).  `dtype`: float16 or
    bfloat16.  `scale`, `out_sumsq` and `out_nonfinite` as in decompress_data_reduce_compress."""
    return _reduce_call(ts_in, ts_acc, True, True, accumulate, temp_mem, out_status, out_sizes, out_compressed, out_compressed_sizes,
                        prob_bits, dtype, scale, out_sumsq, out_nonfinite)


def _check_slice_args(compress_as_float, ts_in, dtype):
    _check(len(ts_in) > 0)
    for t in ts_in:
        _check(t.is_cuda, "compressed tensors must be on the GPU")
    if compress_as_float:
        _check(dtype is None or dtype in _DTYPE_TO_FT, "dtype must be float16, bfloat16 or float32")
    else:
        _check(dtype is None or dtype == torch.uint8, "archives of raw bytes decode to uint8")


def _archive_info(compress_as_float, ts_in, dtype):
    """-> (words of every archive, the dtype they decode to), read from the headers (one synchronising copy)"""
    dev = ts_in[0].get_device()
    for t in ts_in:
        _check(t.get_device() == dev and t.is_contiguous() and t.dtype == torch.uint8)
    with torch.cuda.device(dev):
        hs, ht = _header_info(compress_as_float, ts_in, None, 0)
    hs = [v & _U32_MAX for v in hs]
    if not compress_as_float:
        return hs, torch.uint8
    for t in ht:
        _check(t in _FT_TO_DTYPE and t == ht[0], "the archives must hold one float type")
    _check(dtype is None or _DTYPE_TO_FT[dtype] == ht[0], "the archives hold another float type than `dtype`")
    return hs, _FT_TO_DTYPE[ht[0]]


def _slice_known(compress_as_float, ts_in, starts, counts, sizes, out_dtype, temp_mem, prob_bits):
    device = ts_in[0].device
    covers, bufs = [], []
    for start, count, size in zip(starts, counts, sizes):
        _check(start + count <= size, f"words [{start}, {start + count}) are past the end of an element of {size}")
        first, blocks, offset = block_cover(start, count)
        covers.append((first, blocks, offset))
        words = min(size, (first + blocks) * BLOCK_WORDS) - first * BLOCK_WORDS if blocks else 0
        bufs.append(torch.empty((words,), dtype=out_dtype, device=device))
    status = torch.empty((len(ts_in),), dtype=torch.uint8, device=device)
    decompress_data_range(compress_as_float, ts_in, bufs, [c[0] for c in covers], [c[1] for c in covers], temp_mem, status, None,
                          prob_bits=prob_bits)
    bad = [i for i, ok in enumerate(status.tolist()) if not ok]
    _check(not bad, f"ranged decode failed for batch members {bad}: malformed archive")
    return [buf.narrow(0, c[2] if count else 0, count) for buf, c, count in zip(bufs, covers, counts)]


def decompress_data_slice(compress_as_float, ts_in, starts, counts, dtype=None, temp_mem=None, prob_bits=K_DEFAULT_PRECISION):
    """Words [starts[i], starts[i] + counts[i]) of every archive -> list of tensors (bytes: uint8).

    The range is decoded in the format's blocks of 4096 words: each element's covering block range (`block_cover`) goes
    into one buffer of its own, the whole batch in ONE ranged decode call, and the result is a view into that buffer --
    no copy.  The price of keeping sub-block edges out of the kernel: at most 2 x 4095 words per element are decoded
    (and held by the view's storage) beyond what was asked.  Sizes and, for floats, the dtype are read from the archive
    headers (`dtype`, if given, must match).  RuntimeError on a range past an element's end or a malformed archive."""
    starts, counts = [int(v) for v in starts], [int(v) for v in counts]
    _check(len(starts) == len(ts_in) and len(counts) == len(ts_in), "one start and count per tensor")
    _check_slice_args(compress_as_float, ts_in, dtype)
    for s0, c0 in zip(starts, counts):
        _check(s0 >= 0 and c0 >= 0, "starts and counts must not be negative")
    sizes, out_dtype = _archive_info(compress_as_float, ts_in, dtype)
    return _slice_known(compress_as_float, ts_in, starts, counts, sizes, out_dtype, temp_mem, prob_bits)

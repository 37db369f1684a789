"""Multi-GPU plumbing for the batched API: one process per GPU (torchrun),
independent batch elements sharded contiguously across ranks, no data-path
collective.  The codec has no exchange step (every element carries its own
statistics), so RCCL is used only to (a) all-gather the 4-byte compressed sizes
so every rank knows the whole batch's layout and (b) reduce timings.

Backend "nccl" is RCCL on ROCm; the same code runs on "gloo" for CPU tests.
"""
import ctypes
import inspect
import math
import os

import torch
import torch.distributed as dist


def init(backend=None, device=None):
    """Initialises torch.distributed from the torchrun environment (RANK, WORLD_SIZE, MASTER_*)."""
    if dist.is_initialized():
        return
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    kwargs = {}
    if backend == "nccl" and device is not None:
        kwargs["device_id"] = device
    dist.init_process_group(backend=backend, **kwargs)


def shard_range(num_elements, rank, world):
    """Element-contiguous partition: rank g of G owns [g*B/G, (g+1)*B/G) with the
    remainder spread over the first ranks."""
    base, rem = divmod(num_elements, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def decompress_shard(compress_as_float, ts_in, rank, world, dtype=None, temp_mem=None, prob_bits=10):
    """This rank's `shard_range` of the WORDS of every archive in `ts_in` (a compressed checkpoint every rank holds,
    each rank wanting its slice of every tensor) -> list of tensors.  Local: ops.decompress_data_slice on the ranges,
    no collective; only the blocks that cover the shard are read and decoded."""
    from . import ops

    ops._check(0 <= rank < world, "rank must be in [0, world)")
    ops._check_slice_args(compress_as_float, ts_in, dtype)
    sizes, out_dtype = ops._archive_info(compress_as_float, ts_in, dtype)
    ranges = [shard_range(n, rank, world) for n in sizes]
    return ops._slice_known(compress_as_float, ts_in, [s for s, _ in ranges], [e - s for s, e in ranges], sizes, out_dtype,
                            temp_mem, prob_bits)


def gather_sizes(local_sizes, num_elements):
    """All-gathers per-element compressed sizes (int32 tensor of this rank's shard,
    on the backend's device) into the full [num_elements] vector on every rank."""
    world = dist.get_world_size()
    counts = [shard_range(num_elements, r, world) for r in range(world)]
    width = max(e - s for s, e in counts)
    padded = torch.zeros((width,), dtype=torch.int32, device=local_sizes.device)
    padded[: local_sizes.numel()] = local_sizes
    out = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(out, padded)
    return torch.cat([o[: e - s] for o, (s, e) in zip(out, counts)])


def gather_scalars(value, device):
    """Every rank's float, in rank order, on every rank."""
    if dist.get_backend() != "nccl":
        device = "cpu"
    t = torch.tensor([value], dtype=torch.float64, device=device)
    out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [float(o.item()) for o in out]


def max_over_ranks(seconds, device):
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# ---------------------------------------------------------------------------
# Compressed all-gather (the use the reference's README
# motivates, README.md:68-72,104): every rank compresses its tensors with the
# float codec, the ranks exchange sizes and then the compressed rows over
# RCCL/xGMI, and every rank decompresses everything it received.  Two phases
# because rows are variable-length: (1) all-gather of the int32 sizes, (2) one
# all-gather of a [rows, width] byte matrix whose width is the largest
# compressed row across ranks (rounded to 16 bytes) -- not the worst-case
# capacity the codec wrote into.  xGMI is point-to-point and a ring all-gather
# is bound by one link per hop, so the bytes saved by the codec (x0.67 for bf16
# gradients/activations) translate directly into collective time.
class GpuFloatCodec:
    """Default codec of the compressed collectives: the HIP float codec through `torch.ops.dietgpu.*`
    (csrc/torch_ops.cpp over the C ABI: no per-call Python marshalling of pointer arrays).  `temp_mem`
    (optional uint8 tensor) is handed to every call, as the reference's ops take it.

    `rolling=True`: `compress` / `compress_cast` go through `ops.compress_data_rolling`.  The codec keeps one counts
    tensor per (archive dtype, cast or not, number of tensors, their sizes); the first call for such a key counts the
    usual way, every later one makes its tables from the counts the call before it left and leaves its own -- no
    histogram pass in steady state.  Any table is lossless, so what the collectives deliver is bit for bit the same;
    only the archive sizes depend on how far the tensors moved since the last call (and they are a few per cent above
    the plain codec's even then: every symbol keeps a probability).  Every rolling call after a
    key's first reads one flag back from the device ("a row is larger than its capacity": that call is then repeated
    with tables of the tensors' own), so `compress` synchronises with the stream once per call."""

    def __init__(self, temp_mem=None, rolling=False):
        from . import load_torch_ops

        self.ops = load_torch_ops()
        self.temp_mem = temp_mem
        self.dtype = None
        self.rolling = bool(rolling)
        self._rolling_state = {}  # key -> (counts int32 [n, 256], row capacities int64 [n])

    def _compress_rolling(self, tensors, dtype, cast):
        from . import ops

        key = (dtype, cast, len(tensors), tuple(t.numel() for t in tensors))
        state = self._rolling_state.get(key)
        first = state is None
        if first:
            dev = tensors[0].device
            caps = torch.tensor([ops.max_float_compressed_size(torch.empty(0, dtype=dtype), t.numel()) for t in tensors],
                                dtype=torch.int64, device=dev)
            state = self._rolling_state[key] = (torch.empty((len(tensors), 256), dtype=torch.int32, device=dev), caps)
        counts, caps = state
        comp, sizes, _ = ops.compress_data_rolling(tensors, None if first else counts, counts, dtype if cast else None, self.temp_mem)
        # a row larger than its capacity is incomplete (counts that fit nothing, tensors of millions of words): once more,
        # with tables of the tensors' own
        # (sizes are uint32 in an int32 tensor, and both they and the capacities can pass 2^31: compared as int64)
        if not first and bool(((sizes[: len(tensors)].to(torch.int64) & 0xFFFFFFFF) > caps).any().item()):
            comp, sizes, _ = ops.compress_data_rolling(tensors, None, counts, dtype if cast else None, self.temp_mem)
        return comp, sizes

    def compress(self, tensors):
        if self.rolling and tensors[0].dtype in (torch.float16, torch.bfloat16):
            self.dtype = tensors[0].dtype
            return self._compress_rolling(tensors, tensors[0].dtype, False)
        comp, sizes, _ = self.ops.compress_data(True, tensors, False, self.temp_mem)
        self.dtype = tensors[0].dtype  # (what decompress_accumulate's rows hold: the collectives exchange one dtype)
        return comp, sizes

    def compress_cast(self, tensors, dtype):
        """float32 tensors -> archives of `dtype` (float16 / bfloat16), rounded in registers: no 16-bit scratch tensor"""
        from . import ops

        self.dtype = dtype
        if self.rolling:
            return self._compress_rolling(tensors, dtype, True)
        comp, sizes, _ = ops.compress_data_cast(tensors, dtype, self.temp_mem)
        return comp, sizes

    def compress_cast_feedback(self, tensors, residuals, dtype, fresh=False):
        """compress_cast of tensors[i] + residuals[i] (float32, updated in place to the rounding error; `fresh`: no
        residual yet, the buffers are only written): ops.compress_data_feedback.  It does not use the rolling tables -- a
        `rolling=True` codec counts these tensors with the histogram pass (there is no counting form of the feedback
        encoder)."""
        from . import ops

        self.dtype = dtype
        comp, sizes, _ = ops.compress_data_feedback(tensors, residuals, dtype, fresh, self.temp_mem)
        return comp, sizes

    def compress_cast_stochastic(self, tensors, dtype, seed, first_member=0):
        """compress_cast with STOCHASTIC rounding (ops.compress_data_stochastic): tensor i is rounded with the random bits
        of member first_member + i under `seed` -- an int in [0, 2^64) or a 1-element int64 tensor on the device, never
        read by the host.  Unbiased, and without the residual of compress_cast_feedback.  It does not use the rolling
        tables (there is no counting form of the stochastic encoder)."""
        from . import ops

        self.dtype = dtype
        return ops.compress_data_stochastic(tensors, dtype, seed, first_member)

    def decompress(self, rows, outs, scale=None):
        """`scale` (a number, or a float32 tensor of 1 or len(rows) elements on the device): every word is multiplied by
        it in the decode kernel (ops.decompress_data_scaled); a tensor is never read by the host"""
        status = torch.zeros((len(rows),), dtype=torch.uint8, device=outs[0].device)
        if scale is not None:
            from . import ops

            ops.decompress_data_scaled(rows, outs, scale, self.temp_mem, status, None)
            return status
        self.ops.decompress_data(True, rows, outs, False, self.temp_mem, status, None)
        return status

    def decompress_accumulate(self, rows, accs, accumulate, scale=None):
        """rows widened to float32 and stored to (accumulate false) or added into the float32 tensors `accs` -> status.
        `scale` (a number, or a float32 tensor of 1 or len(rows) elements on the device): every widened word is multiplied
        by it in the decode kernel before the store or the add, one multiply and one add, never an FMA
        (ops.decompress_data_accumulate's `scale`); a tensor is never read by the host"""
        from . import ops

        status = torch.zeros((len(rows),), dtype=torch.uint8, device=accs[0].device)
        ops.decompress_data_accumulate(rows, accs, accumulate, self.temp_mem, status, None, dtype=self.dtype, scale=scale)
        return status

    def decompress_update(self, rows, outs, accumulate, scale=None, seed=0, first_member=0):
        """rows multiplied by `scale`, added to (accumulate) or stored over the 16-bit tensors `outs` of the rows' dtype
        and rounded stochastically, in the decode kernel (ops.decompress_data_update) -> status.  `seed`: an int in
        [0, 2^64) or a 1-element int64 tensor on the device, never read by the host; row i draws the random bits of member
        first_member + i"""
        from . import ops

        status = torch.zeros((len(rows),), dtype=torch.uint8, device=outs[0].device)
        ops.decompress_data_update(rows, outs, seed, scale, accumulate, first_member, status, None)
        return status

    def _reduce(self, name, mixed, rows_per_acc, accs, accumulate, scale, norm):
        """The reduce call `name` of ops -> (status, what it returned).  The call's float type: with `mixed`, what a raw
        row says it is; without one, what the last compress call held."""
        from . import ops

        dtype = next((t.dtype for rows in rows_per_acc for t in rows if t.dtype != torch.uint8), self.dtype) if mixed else self.dtype
        # (no `norm`: the call of ops is the one it always was)
        norm_kwargs = {} if norm is None else {"out_sumsq": norm[0], "out_nonfinite": norm[1]}
        status = torch.zeros((len(accs),), dtype=torch.uint8, device=accs[0].device)
        return status, getattr(ops, name)(rows_per_acc, accs, accumulate, self.temp_mem, status, None, dtype=dtype, scale=scale, **norm_kwargs)

    def decompress_reduce(self, rows_per_acc, accs, accumulate, scale=None, norm=None):
        """rows_per_acc[i]: equally long lists of rows, summed left to right into (accumulate) or stored as their sum to
        the float32 tensor accs[i], in ONE launch and all or nothing per accumulator -> status, one per accumulator.
        `scale` (here and in the three methods below): the sums are left multiplied by it, in the same launch.
        `norm` (here and below): a pair (float64 [len(accs)], int32 [len(accs)]) of tensors that the same launch fills
        with the squared norm of the finite words it leaves and the count of the others -- of the accumulators here,
        of the archives in the reduce-compress methods"""
        return self._reduce("decompress_data_reduce", False, rows_per_acc, accs, accumulate, scale, norm)[0]

    def decompress_reduce_compress(self, rows_per_acc, accs, accumulate, scale=None, norm=None):
        """decompress_reduce and compress_cast of the accumulators back to the rows' dtype in ONE call, without the cast's
        histogram pass over the accumulators -> (status, comp, sizes): as the two calls return them"""
        status, (comp, sizes, _) = self._reduce("decompress_data_reduce_compress", False, rows_per_acc, accs, accumulate, scale, norm)
        return status, comp, sizes

    def decompress_reduce_mixed(self, rows_per_acc, accs, accumulate, scale=None, norm=None):
        """decompress_reduce whose rows are uint8 archives or UNCOMPRESSED 1-D tensors of the rows' dtype, which are widened
        and added in their place -> status, one per accumulator"""
        return self._reduce("decompress_data_reduce_mixed", True, rows_per_acc, accs, accumulate, scale, norm)[0]

    def decompress_reduce_compress_mixed(self, rows_per_acc, accs, accumulate, scale=None, norm=None):
        """decompress_reduce_compress with rows as in decompress_reduce_mixed -> (status, comp, sizes)"""
        status, (comp, sizes, _) = self._reduce("decompress_data_reduce_compress_mixed", True, rows_per_acc, accs, accumulate, scale, norm)
        return status, comp, sizes


def compressed_all_gather(tensors, codec=None, scale=None):
    """All-gathers a list of equally-shaped float tensors per rank, moving compressed bytes.

    `tensors`: this rank's list (same count, shapes and dtype on every rank).
    Returns (gathered, stats): gathered[r][i] is rank r's i-th tensor, bit-exact;
    stats = {"raw_bytes", "wire_bytes", "payload_bytes"} per rank-to-rank copy.
    `codec` needs compress(list) -> (uint8 [n, cap], int32 [n]) and
    decompress(list of uint8 rows, list of outputs) -> uint8 status [n].

    `scale` (a number or a 0-dim / 1-element float32 tensor on the tensors' device, the same on every rank): every
    gathered word is delivered as round(fl32(word * scale)) -- one float32 multiply, one rounding to the dtype.  A codec
    whose `decompress` has a `scale` parameter applies it while it decodes (GpuFloatCodec: in the decode kernel, and a
    tensor is never read by the host -- the building block for clipping several buckets by one norm); any other codec
    is decoded as without it, and each output then takes one pass of torch.  None: nothing changes."""
    codec = codec or GpuFloatCodec()
    comp, sizes = codec.compress(tensors)
    raw = sum(t.numel() * t.element_size() for t in tensors)
    return _all_gather_archives(comp, sizes, lambda r: [torch.empty_like(t) for t in tensors], raw, codec, scale=scale)


def _scaled_decompress(codec, rows, outs, scale):
    """codec.decompress(rows, outs) with every word multiplied by `scale` (None: the call as it always was)."""
    if scale is None:
        return codec.decompress(rows, outs)
    if _takes_scale(codec.decompress):
        return codec.decompress(rows, outs, scale=scale)
    status = codec.decompress(rows, outs)
    f = torch.as_tensor(scale, dtype=torch.float32, device=outs[0].device).reshape(())
    for o in outs:
        o.copy_((o.float() * f).to(o.dtype))
    return status


def _decode_into_float32(codec, rows, accs, factor, accumulate, dtype):
    """The rows (archives of `dtype`) decoded into the float32 tensors `accs`: acc = [acc +] fl32(widen(word) * factor),
    one float32 multiply and one float32 add (factor None: the exact widening, no multiply) -> status.  A codec whose
    `decompress_accumulate` has a `scale` parameter does it in ONE call (GpuFloatCodec: in the decode kernel; a tensor
    factor is never read by the host); without a factor the method gets the three arguments it always got; a
    `decompress_accumulate` without the parameter decodes into a float32 scratch, which then takes `mul_` by the 0-dim
    factor and `copy_` / `add_`; a codec without the method decodes with `decompress` into a scratch of `dtype`, which is
    widened first.  The same bits every way."""
    method = getattr(codec, "decompress_accumulate", None)
    if callable(method):
        if factor is None:
            return method(rows, accs, accumulate)
        if _takes_scale(method):
            return method(rows, accs, accumulate, scale=factor)
        wide = [torch.empty_like(a) for a in accs]
        status = method(rows, wide, False)
    else:
        narrow = [torch.empty(a.shape, dtype=dtype, device=a.device) for a in accs]
        status = codec.decompress(rows, narrow)
        wide = [t.float() for t in narrow]
    for a, w in zip(accs, wide):
        if factor is not None:
            w.mul_(factor)
        if accumulate:
            a.add_(w)
        else:
            a.copy_(w)
    return status


def _decode_update(codec, rows, outs, factor, accumulate, seed, first_member):
    """The rows (archives of the outs' 16-bit dtype) applied to `outs` with stochastic rounding: out = sround([widen(out)
    +] fl32(widen(word) * factor)), row i with the random bits of member first_member + i (dgpu_float_decode_update;
    factor None: 1, which multiplies) -> status.  A codec with `decompress_update` does it in ONE call (GpuFloatCodec: in
    the decode kernel); any other codec decodes into a float32 scratch (_decode_into_float32), which takes the add of the
    widened tensor and the rounding from torch (rounding.update_).  The same bits either way."""
    method = getattr(codec, "decompress_update", None)
    if callable(method):
        return method(rows, outs, accumulate, scale=factor, seed=seed, first_member=first_member)
    from . import rounding

    one = torch.ones((), dtype=torch.float32, device=outs[0].device)
    wide = [torch.empty(o.shape, dtype=torch.float32, device=o.device) for o in outs]
    status = _decode_into_float32(codec, rows, wide, one if factor is None else factor, False, outs[0].dtype)
    for i, (o, w) in enumerate(zip(outs, wide)):
        rounding.update_(o, w, seed, first_member + i, accumulate)
    return status


def _all_gather_archives(comp, sizes, outs_of, raw_bytes, codec, scale=None, decode=None):
    """The exchange of compressed_all_gather for rows that are compressed already: `comp` [n, cap] / `sizes` [n] as a
    codec's compress returns them; `outs_of(r)` -> the n tensors rank r's rows are decompressed into.  `scale`: see
    compressed_all_gather.  `decode(r, rows, outs)` -> status: what decodes source rank r's rows instead of the codec's
    `decompress` (compressed_all_reduce's `out`)."""
    world = dist.get_world_size()
    n = comp.shape[0]
    sizes = sizes.to(torch.int32)

    # phase 1: sizes
    all_sizes = [torch.empty_like(sizes) for _ in range(world)]
    dist.all_gather(all_sizes, sizes)
    all_sizes = torch.stack(all_sizes)  # [world, n]
    width = int(all_sizes.max().item())
    width = (width + 15) // 16 * 16

    # phase 2: payload, trimmed to the widest compressed row
    payload = comp[:, :width].contiguous()
    gathered_payload = [torch.empty_like(payload) for _ in range(world)]
    dist.all_gather(gathered_payload, payload)

    gathered = []
    for r in range(world):
        rows = [gathered_payload[r][i, : int(all_sizes[r, i])] for i in range(n)]
        outs = outs_of(r)
        status = decode(r, rows, outs) if decode is not None else _scaled_decompress(codec, rows, outs, scale)
        if not bool(status.all().item()):
            raise RuntimeError(f"decompression of rank {r}'s rows failed")
        gathered.append(outs)
    stats = {
        "raw_bytes": raw_bytes,
        "wire_bytes": n * width,
        "payload_bytes": int(all_sizes[dist.get_rank()].sum().item()),
    }
    return gathered, stats


_MAX_REDUCE_SOURCES = 64  # of one decode-reduce call (dgpu_float_decode_reduce)


_WIRE_DTYPES = (torch.float16, torch.bfloat16)


def _check_wire(what, tensor, codec, raw_local, wire_dtype, residual):
    """The arguments of a float32 tensor on a 16-bit wire (wire_dtype, residual), before anything is exchanged."""
    if wire_dtype is None:
        if residual is not None:
            raise RuntimeError(f"{what}: a residual needs wire_dtype (float16 or bfloat16)")
        return
    if wire_dtype not in _WIRE_DTYPES:
        raise RuntimeError(f"{what}: wire_dtype must be float16 or bfloat16")
    if tensor.dtype != torch.float32:
        raise RuntimeError(f"{what}: wire_dtype is for float32 tensors (a 16-bit tensor travels as it is)")
    if raw_local:
        raise RuntimeError(f"{what}: raw_local cannot be combined with wire_dtype -- a float32 row is not a raw source of 16-bit "
                           "archives, and the rank's own shard would escape the feedback")
    if residual is None:
        return
    if (residual.dtype != torch.float32 or residual.dim() != 1 or residual.numel() != tensor.numel() or not residual.is_contiguous()
            or residual.device != tensor.device):
        raise RuntimeError(f"{what}: the residual must be a flat contiguous float32 tensor of the tensor's length on its device")
    if not callable(getattr(codec, "compress_cast_feedback", None)):
        raise RuntimeError(f"{what}: a residual needs a codec with compress_cast_feedback(tensors, residuals, dtype, fresh)")


def _check_wire_seed(what, tensor, wire_dtype, wire_seed, residual, norm, clip_norm=None, needs_wire_dtype=True):
    """The arguments of a stochastically rounded wire (wire_seed), before anything is exchanged."""
    if wire_seed is None:
        return
    if isinstance(wire_seed, torch.Tensor):
        if not (wire_seed.dtype == torch.int64 and wire_seed.numel() == 1 and wire_seed.device == tensor.device):
            raise RuntimeError(f"{what}: a tensor wire_seed must be a 1-element int64 tensor on the tensor's device")
    elif not (isinstance(wire_seed, int) and not isinstance(wire_seed, bool) and 0 <= wire_seed < (1 << 64)):
        raise RuntimeError(f"{what}: wire_seed must be an int in [0, 2^64) or a 1-element int64 tensor")
    if needs_wire_dtype and wire_dtype is None:
        raise RuntimeError(f"{what}: wire_seed needs wire_dtype -- without it nothing is rounded here")
    if residual is not None:
        raise RuntimeError(f"{what}: wire_seed cannot be combined with a residual -- error feedback and stochastic rounding are "
                           "alternatives")
    if norm or clip_norm is not None:
        raise RuntimeError(f"{what}: wire_seed cannot be combined with norm=True or clip_norm -- the statistics must describe the "
                           "archive's words, which on the stochastic path only a second pass could give")


def _compress_stochastic(codec, tensors, dtype, seed, first_member):
    """float32 tensors -> archives of `dtype`, tensor i rounded stochastically with the random bits of member
    first_member + i under `seed` (dgpu_float_stochastic_compress) -> (comp, sizes).  A codec with
    `compress_cast_stochastic` does it in ONE call (GpuFloatCodec: in the compressor's two kernels); any other codec gets
    the rounding from torch (rounding.stochastic_round_) into a 16-bit scratch and compresses that.  The same bits."""
    method = getattr(codec, "compress_cast_stochastic", None)
    if callable(method):
        return method(tensors, dtype, seed, first_member=first_member)
    from . import rounding

    scratch = [torch.empty(t.shape, dtype=dtype, device=t.device) for t in tensors]
    for i, (q, t) in enumerate(zip(scratch, tensors)):
        rounding.stochastic_round_(q, t, seed, (first_member + i) & 0xFFFFFFFF)
    return codec.compress(scratch)


def _exchange_shard_rows(tensor, codec, raw_local=False, wire_dtype=None, residual=None, residual_fresh=False, wire_seed=None):
    """The exchange half of compressed_reduce_scatter: shard j of this rank's flat tensor, compressed, goes to rank j ->
    (words per shard, recv [source rank, width] uint8, all_sizes [source rank, destination rank] int32, width).
    raw_local: the rank's own shard is not compressed (the codec gets the other world - 1, none at all in a world of one);
    its row of the exchange has size 0 and carries nothing.
    wire_dtype (float16 / bfloat16, for a float32 tensor): the shards are rounded to it by the compressor -- the codec's
    compress_cast, or, with `residual` (a flat float32 tensor of the tensor's length, updated in place), its
    compress_cast_feedback on the shards and the matching views of the residual, or, with `wire_seed`, stochastically
    (_compress_stochastic): the shard of this rank for destination j is member rank * world + j."""
    world = dist.get_world_size()
    if tensor.dim() != 1 or tensor.numel() % world != 0:
        raise RuntimeError("compressed_reduce_scatter: the tensor must be flat, its length a multiple of the world size")
    shard_words = tensor.numel() // world
    shards = list(tensor.view(world, shard_words).unbind(0))
    if raw_local:
        me = dist.get_rank()
        others = [j for j in range(world) if j != me]
        sizes = torch.zeros((world,), dtype=torch.int32, device=tensor.device)
        comp = torch.empty((world, 0), dtype=torch.uint8, device=tensor.device)
        if others:
            comp_others, sizes_others = codec.compress([shards[j] for j in others])
            at = torch.tensor(others, dtype=torch.int64, device=tensor.device)
            sizes[at] = sizes_others[: len(others)].to(torch.int32)
            comp = torch.empty((world, comp_others.shape[1]), dtype=torch.uint8, device=tensor.device)
            comp[at] = comp_others[: len(others)]
            comp[me].zero_()  # (travels to this rank itself; nothing reads it)
    elif wire_dtype is not None and residual is not None:
        comp, sizes = codec.compress_cast_feedback(shards, list(residual.view(world, shard_words).unbind(0)), wire_dtype, bool(residual_fresh))
    elif wire_dtype is not None and wire_seed is not None:
        comp, sizes = _compress_stochastic(codec, shards, wire_dtype, wire_seed, dist.get_rank() * world)
    elif wire_dtype is not None:
        comp, sizes = codec.compress_cast(shards, wire_dtype)
    else:
        comp, sizes = codec.compress(shards)  # all shards in one call
    sizes = sizes.to(torch.int32)

    # phase 1: sizes (every rank learns every row's size: the width is the widest row anywhere)
    all_sizes = [torch.empty_like(sizes) for _ in range(world)]
    dist.all_gather(all_sizes, sizes)
    all_sizes = torch.stack(all_sizes)  # [source rank, destination rank]
    width = (int(all_sizes.max().item()) + 15) // 16 * 16

    # phase 2: row j of this rank to rank j, trimmed to the widest row
    send = comp[:, :width].contiguous()
    recv = torch.empty_like(send)
    if width:  # (0: a world of one with raw_local -- every rank sees the same width)
        work = _all_to_all_flat(recv.view(-1), send.view(-1), world)
        if work is not None:
            work.wait()
    return shard_words, recv, all_sizes, width


def _rows_with_local(tensor, recv, all_sizes, me, world, raw_local):
    """The sources of this rank's shard in rank order: the received rows, with the rank's own shard uncompressed in its
    place when raw_local."""
    rows = [recv[r, : int(all_sizes[r, me])] for r in range(world)]
    if raw_local:
        rows[me] = tensor.view(world, -1)[me]
    return rows


def _reduce_factor(op, scale, world):
    """What the sum is multiplied by: (scale or 1) * (1 / world for op "avg"), rounded ONCE to float32 -> that float32
    value, or None when it is 1.0 (nothing is multiplied and nothing new is asked of the codec)."""
    if op not in ("sum", "avg"):
        raise ValueError(f'op must be "sum" or "avg", not {op!r}')
    f = ctypes.c_float((1.0 if scale is None else float(scale)) * (1.0 / world if op == "avg" else 1.0)).value
    if not math.isfinite(f) or f == 0.0:
        raise RuntimeError("the scale of a reduction must be finite and not zero")
    return None if f == 1.0 else f


def _takes_scale(method):
    """A pluggable codec is asked to scale only by a method that has a `scale` parameter."""
    try:
        return "scale" in inspect.signature(method).parameters
    except (TypeError, ValueError):
        return False


def _takes_norm(method):
    """... and to measure what it leaves only by a method that has a `norm` parameter."""
    try:
        return "norm" in inspect.signature(method).parameters
    except (TypeError, ValueError):
        return False


def _reduce_call(method, rows_per_acc, accs, factor, norm=None):
    """One reduce call of the codec, accumulate off -> (what it returns, whether `factor` is still to be applied).  Without a
    factor the call is the three positional arguments it always was.  `norm`: a pair from _norm_pair, handed to a method
    that has a `norm` parameter (and leaves the final, scaled words); norm[2] then says that it is filled."""
    kwargs = {}
    scaled_here = factor is not None and _takes_scale(method)
    if scaled_here:
        kwargs["scale"] = factor
    if norm is not None and _takes_norm(method) and (factor is None or scaled_here):
        kwargs["norm"] = (norm[0], norm[1])
        norm[2] = True
    return method(rows_per_acc, accs, False, **kwargs), factor is not None and not scaled_here


def _norm_pair(device):
    """[sumsq float64 [1], nonfinite int32 [1], filled by the codec]"""
    return [torch.zeros((1,), dtype=torch.float64, device=device), torch.zeros((1,), dtype=torch.int32, device=device), False]


def _norm_by_torch(norm, words):
    """The statistic of a codec that does not report it: one pass over `words` -- the squared norm of the finite ones in
    float64 and the count of the others."""
    finite = torch.isfinite(words)
    norm[0].copy_(torch.where(finite, words, torch.zeros((), dtype=words.dtype, device=words.device)).to(torch.float64).square().sum().reshape(1))
    norm[1].copy_((~finite).sum().to(torch.int32).reshape(1))
    norm[2] = True


def _norm_stats(stats, norm):
    stats["sumsq"] = norm[0].reshape(())
    stats["nonfinite"] = norm[1].reshape(())


def _scale_shard(shard, factor):
    # the same single float32 multiply as the kernel's: a 0-dim float32 factor, so nothing is promoted
    shard.mul_(torch.tensor(factor, dtype=torch.float32, device=shard.device))


def compressed_reduce_scatter(tensor, codec=None, raw_local=False, op="sum", scale=None, norm=False, wire_dtype=None, residual=None,
                              residual_fresh=False, wire_seed=None):
    """Reduce-scatter (sum) of a flat float tensor, moving compressed bytes and summing in float32.

    `tensor`: this rank's flat fp16 / bf16 / fp32 tensor; its length is a multiple of the world size and the same on
    every rank.  Shard j of every rank goes to rank j, compressed; rank j decodes the `world` rows it received straight
    into ONE float32 shard -- no 16-bit scratch tensor, no separate add.  A codec with decompress_reduce(rows_per_acc,
    accs, accumulate) sums all rows in ONE decode-reduce call (accumulate off: rank 0's row is stored, so the shard needs
    no memset) with one status read; a codec without it (or a world of more than 64 ranks) stores rank 0's row and makes
    one decode-accumulate call per further source rank, in ascending rank order on the current stream.  Either way the
    result is, by construction, the sequential float32 sum in rank order, ((x_0 + x_1) + x_2) + ..., of the exactly
    widened inputs: bit-identical on every run, between the two paths and to the same sum computed uncompressed.
    Returns (shard_fp32, stats), stats as `compressed_all_gather`.  RuntimeError if a row fails to decode; on the
    decode-reduce path the shard was then not partly summed (the call adds all rows or none).
    `codec` needs compress(list) -> (uint8 [n, cap], int32 [n]) and, for the shard's sum, decompress_reduce(rows_per_acc,
    accs, accumulate) -> uint8 status [len(accs)] or decompress_accumulate(rows, accs, accumulate) -> uint8 status [n];
    a world of more than 64 ranks needs decompress_accumulate (RuntimeError without it).

    raw_local=True, with a codec that has decompress_reduce_mixed(rows_per_acc, accs, accumulate) in a world of at most
    64 ranks: the rank's own shard is neither compressed nor sent to itself nor decoded -- the codec compresses the other
    world - 1 shards (none in a world of one) and the sum takes `tensor.view(world, -1)[me]` as it is, at position `me`
    of the rank order.  The result is bit-identical; stats["payload_bytes"] no longer holds the own row.  Without the
    method, or in a larger world, the call quietly takes the path above.

    op="avg" divides by the world size and `scale` multiplies by a factor of the caller's: the shard is
    fl32(sum * f), f = (scale or 1) * (1 / world if op == "avg" else 1) rounded once to float32 -- ONE float32 multiply
    of the float32 sum, made by the codec's reduce call where its method has a `scale` parameter (GpuFloatCodec: in the
    reduce kernel, at no extra pass) and by one multiply of the shard otherwise: the same bits either way.  f == 1
    changes nothing and asks nothing new of the codec.

    norm=True: stats gains "sumsq", a 0-dim float64 tensor with the sum of squares of the finite words of the returned
    float32 shard (exact squares, added in float64), and "nonfinite", a 0-dim int32 tensor with the number of its words
    that are inf or NaN -- what clipping by global norm and a loss scaler's overflow check need of the shard.  They are
    filled by the codec's reduce call where its method has a `norm` parameter (GpuFloatCodec: by the reduce kernel), and
    by one torch pass over the shard otherwise; nothing is read back to the host.  With the default the codec is called
    exactly as it always was.

    wire_dtype (float16 or bfloat16), for a float32 `tensor`: the shards travel as archives of that type instead of as
    float32 archives -- rounded inside the compressor (the codec's compress_cast), the receiving side unchanged on rows of
    wire_dtype.  With `residual` -- a flat float32 tensor of the tensor's length, this rank's, kept between steps -- the
    rounding has error feedback: the codec's compress_cast_feedback(shards, residual's shard views, wire_dtype, fresh) adds
    the residual before it rounds and stores the new rounding error back, in place.  residual_fresh=True: the first step,
    the residual is only written.  raw_local=True with wire_dtype, and a residual with a codec that has no
    compress_cast_feedback, raise RuntimeError.

    wire_seed (with wire_dtype; an int in [0, 2^64), or a 1-element int64 tensor on the device, never read by the host):
    the rounding to wire_dtype is STOCHASTIC -- unbiased, where round to nearest drops a component below half a unit at
    every step, and without a residual's 4 bytes per element.  The shard of source rank r for destination j is rounded
    with the random bits of member r * world + j (dgpu_float_stochastic_compress), so the ranks draw independent bits and
    their errors average out in the sum.  THE SEED MUST BE THE SAME ON EVERY RANK for the result to be a pure function of
    the inputs and the seed.  A codec with compress_cast_stochastic(tensors, dtype, seed, first_member) rounds in the
    compressor (GpuFloatCodec: in its two kernels); any other codec gets dietgpu_amd.rounding.stochastic_round_ into a
    16-bit scratch and its `compress`, with the same bits.  wire_seed without wire_dtype (nothing is rounded here), with
    a residual (feedback and stochastic rounding are alternatives) or with norm=True raises RuntimeError."""
    codec = codec or GpuFloatCodec()
    _check_wire("compressed_reduce_scatter", tensor, codec, raw_local, wire_dtype, residual)
    _check_wire_seed("compressed_reduce_scatter", tensor, wire_dtype, wire_seed, residual, norm)
    world = dist.get_world_size()
    me = dist.get_rank()
    factor = _reduce_factor(op, scale, world)
    pair = _norm_pair(tensor.device) if norm else None
    if raw_local and callable(getattr(codec, "decompress_reduce_mixed", None)) and world <= _MAX_REDUCE_SOURCES:
        shard_words, recv, all_sizes, width = _exchange_shard_rows(tensor, codec, True)
        shard = torch.empty((shard_words,), dtype=torch.float32, device=tensor.device)
        status, pending = _reduce_call(codec.decompress_reduce_mixed, [_rows_with_local(tensor, recv, all_sizes, me, world, True)], [shard], factor,
                                       pair)
        if not bool(status.all().item()):
            raise RuntimeError("decode-reduce of the received rows failed: a row is malformed or the rows differ in length; "
                               "the shard was not partly summed")
        if pending:
            _scale_shard(shard, factor)
        stats = {"raw_bytes": tensor.numel() * tensor.element_size(), "wire_bytes": world * width,
                 "payload_bytes": int(all_sizes[me].sum().item())}
        if norm:
            if not pair[2]:
                _norm_by_torch(pair, shard)
            _norm_stats(stats, pair)
        return shard, stats
    shard_words, recv, all_sizes, width = _exchange_shard_rows(tensor, codec, False, wire_dtype, residual, residual_fresh, wire_seed)
    shard = torch.empty((shard_words,), dtype=torch.float32, device=tensor.device)
    has_reduce = callable(getattr(codec, "decompress_reduce", None))
    if not (has_reduce and world <= _MAX_REDUCE_SOURCES) and not callable(getattr(codec, "decompress_accumulate", None)):
        raise RuntimeError(f"compressed_reduce_scatter: the codec has no decompress_accumulate, which a world of {world} ranks "
                           f"(more than {_MAX_REDUCE_SOURCES}) or a codec without decompress_reduce needs")
    if has_reduce and world <= _MAX_REDUCE_SOURCES:
        status, pending = _reduce_call(codec.decompress_reduce, [[recv[r, : int(all_sizes[r, me])] for r in range(world)]], [shard], factor, pair)
        if not bool(status.all().item()):
            raise RuntimeError("decode-reduce of the received rows failed: a row is malformed or the rows differ in length; "
                               "the shard was not partly summed")
    else:
        for r in range(world):
            status = codec.decompress_accumulate([recv[r, : int(all_sizes[r, me])]], [shard], r != 0)
            if not bool(status.all().item()):
                raise RuntimeError(f"decode-accumulate of rank {r}'s row failed")
        pending = factor is not None
    if pending:
        _scale_shard(shard, factor)
    stats = {
        "raw_bytes": tensor.numel() * tensor.element_size(),
        "wire_bytes": world * width,
        "payload_bytes": int(all_sizes[me].sum().item()),
    }
    if norm:
        if not pair[2]:
            _norm_by_torch(pair, shard)
        _norm_stats(stats, pair)
    return shard, stats


def compressed_all_reduce(tensor, codec=None, raw_local=False, op="sum", scale=None, norm=False, clip_norm=None, wire_dtype=None,
                          residual=None, residual_fresh=False, out=None, out_scale=None, out_accumulate=False, out_seed=None,
                          wire_seed=None):
    """All-reduce (sum) of a flat fp16 / bf16 tensor, moving compressed bytes both ways and summing in float32.

    Three steps: `compressed_reduce_scatter` (this rank's float32 shard of the sum), the codec's `compress_cast` of that
    shard back to the input dtype -- the rounding happens inside the compressor, the 16-bit shard never exists -- and the
    compressed all-gather of the shards.  The result is the sequential float32 sum in rank order of the exactly widened
    inputs, rounded ONCE to the input dtype (round to nearest even), bit-identical on every rank.  Returns (summed
    tensor in the input dtype, stats): the stats of the two exchanges added up.  `codec` needs what
    compressed_reduce_scatter and compressed_all_gather need, and compress_cast(list of float32, dtype) -> (uint8
    [n, cap], int32 [n]).

    A codec with decompress_reduce_compress(rows_per_acc, accs, accumulate) -> (status, comp, sizes), in a world of at most
    64 ranks, makes the middle ONE call: the received rows are summed into the shard and the shard's archive is written
    by the same call, which counts the exponents while it sums instead of reading the shard again for a histogram.  The
    result is bit-identical to the three-step path.

    raw_local=True: as in compressed_reduce_scatter -- the rank's own shard enters the sum uncompressed.  On the one-call
    path that needs the codec's decompress_reduce_compress_mixed, on the three-step path its decompress_reduce_mixed;
    without the method the path needs, today's path runs.  Bit-identical either way.

    op, scale: as in compressed_reduce_scatter -- the mean, or any multiple of the sum, rounded ONCE to the input dtype
    after the float32 multiply: a mean that is representable does not overflow because the sum would have.  The one-call
    path is taken with a factor only if the codec's method has a `scale` parameter; otherwise the three-step path runs
    with the factor in its reduce-scatter.  Bit-identical on every path and rank.

    norm=True: stats gains "sumsq" and "nonfinite" as in compressed_reduce_scatter, but of this rank's shard ROUNDED to
    the input dtype -- the words of its archive, which are the words of the returned tensor: a float32 sum that rounds
    to a float16 infinity counts as non-finite -- and "global_sumsq" (0-dim float64) and "global_nonfinite" (0-dim
    int32), their sums over the ranks from one all-reduce of a float64 [2] tensor: the squared norm and the non-finite
    count of the tensor this call returns, the same on every rank.  On the one-call path they are filled by the codec's
    reduce-compress method where it has a `norm` parameter; otherwise by one torch pass over shard.to(dtype).  No host
    read is added.

    clip_norm (a positive float): the returned tensor is clipped to that 2-norm.  It implies the statistics of norm=True,
    which describe the UNCLIPPED result (the norm is that of its finite words; "global_nonfinite" is reported as above
    and whether to take the step stays the caller's decision).  Their all-reduce is made BEFORE the all-gather;
    coef = min(clip_norm / (sqrt(global_sumsq) + 1e-6), 1.0) -- the formula of torch.nn.utils.clip_grad_norm_ -- is
    computed in float64 on the device and rounded once to float32, and the all-gather decodes with that factor
    (compressed_all_gather's `scale`: in the codec's decode kernel where its `decompress` has a `scale` parameter): every
    word is round(fl32(word * coef)), bit-identical on every rank.  stats["clip_coef"] is the 0-dim float32 tensor.  No
    pass over the tensor and no host read is added.

    wire_dtype, residual, residual_fresh: as in compressed_reduce_scatter -- a float32 `tensor` whose shards travel as
    archives of wire_dtype, with error feedback on that first rounding when a residual is given.  The call then returns
    the sum in wire_dtype.  Its second rounding -- of the float32 sum, before the all-gather -- carries NO feedback: it is
    the same on every rank and would need a residual per shard of the sum (wire_seed, below, covers it).

    out (a flat contiguous float32 tensor of the tensor's length on its device; for 16-bit tensors and for float32
    tensors with wire_dtype alike): the result is delivered in FLOAT32.  The final all-gather decodes every rank's shard
    archive straight into out.view(world, -1)[r]; no 16-bit result tensor exists, and the call returns (out, stats).
    Without a factor the widening is exact: out == (today's result).float().  The factor f is `coef` with clip_norm,
    `out_scale` with out_scale -- a number, finite and not zero, rounded once to float32, or a 0-dim / 1-element float32
    tensor on the device (-lr: the update of float32 master weights) -- and fl32(coef * out_scale) with both, one float32
    multiply of two 0-dim device tensors; nothing is read by the host.  Then out[k] = [out[k] +] fl32(widen(word_k) * f):
    one float32 multiply and, with out_accumulate=True (gradient accumulation into a float32 buffer), one float32 add,
    never fused; with a clip that is one rounding fewer than the 16-bit result has, whose bits out.to(dtype) still gives.
    A codec whose `decompress_accumulate` has a `scale` parameter makes one call per source rank (GpuFloatCodec: in the
    decode kernel); any other codec is decoded into a scratch and takes the multiply and the add from torch, with the
    same bits.  `out is tensor` is allowed without out_accumulate -- an in-place float32 all-reduce on a 16-bit wire;
    every read of `tensor` precedes the gather -- and is an error with it; `out` must not overlap `tensor` otherwise.
    out_scale or out_accumulate without out is an error.  The statistics keep their meaning: "sumsq", "nonfinite" and
    "global_*" describe the 16-bit words of the archives, unclipped and without out_scale, as without `out`.  With
    out=None the call is what it was.

    out_seed (an int in [0, 2^64), or a 1-element int64 tensor on the device, never read by the host): `out` is a flat
    contiguous tensor of the wire's 16-BIT dtype -- parameters without a float32 master copy -- and the final gather
    decodes source rank r's shard into out.view(world, -1)[r] as out[k] = sround([widen(out[k]) +] fl32(widen(word_k) *
    f)): one float32 multiply, one float32 add (out_accumulate=True), and the STOCHASTIC rounding of
    dgpu_float_decode_update with the random bits of member r and word index k within the shard.  f is as above (1
    without clip_norm and out_scale); out_scale = -lr with out_accumulate is the SGD step.  THE SEED MUST BE THE SAME ON
    EVERY RANK: the random bits are a pure function of (seed, source rank, word index), so equal seeds give every rank
    the same parameter bits, and different seeds let the replicas drift apart.  A codec with `decompress_update` makes one
    call per source rank (GpuFloatCodec: in the decode kernel); any other codec is decoded into a float32 scratch and
    takes the add and the rounding from torch (dietgpu_amd.rounding), with the same bits.  out_seed with a float32 `out`
    is an error, and so is a 16-bit `out` without out_seed; `out is tensor` follows the rules above.

    wire_seed (an int in [0, 2^64), or a 1-element int64 tensor on the device, never read by the host; THE SAME ON EVERY
    RANK): every rounding on the sending side is STOCHASTIC instead of to nearest.  The first -- of a float32 tensor's
    shards to wire_dtype -- as in compressed_reduce_scatter, member r * world + j for source rank r and destination j.
    The second -- of the float32 sum of shard `me` before the all-gather, the one that carries no feedback -- with the
    random bits of member world * world + me; for a 16-bit tensor without wire_dtype it is the only rounding.  The call
    takes the three-step path: the reduce-scatter, the codec's compress_cast_stochastic of the shard (any other codec:
    dietgpu_amd.rounding.stochastic_round_ into a 16-bit scratch and its `compress`, the same bits), the gather; the fused
    reduce-compress call rounds to nearest and is not used.  The result is a pure function of the inputs and the seed,
    bit-identical on every rank.  raw_local (for 16-bit tensors), op, scale, out and out_seed compose as without it.
    wire_seed with a residual, norm=True or clip_norm raises RuntimeError: feedback and stochastic rounding are
    alternatives, and the statistics must describe the archive's words, which on this path only a second pass could
    give.  Without wire_seed every codec call is what it was."""
    codec = codec or GpuFloatCodec()
    _check_wire("compressed_all_reduce", tensor, codec, raw_local, wire_dtype, residual)
    _check_wire_seed("compressed_all_reduce", tensor, wire_dtype, wire_seed, residual, norm, clip_norm, needs_wire_dtype=False)
    out_dtype = wire_dtype if wire_dtype is not None else tensor.dtype
    if out_dtype not in _WIRE_DTYPES:
        raise RuntimeError("compressed_all_reduce: the tensor must be float16 or bfloat16 (float32: give wire_dtype)")
    if out is None:
        if out_scale is not None or out_accumulate:
            raise RuntimeError("compressed_all_reduce: out_scale and out_accumulate need `out`")
        if out_seed is not None:
            raise RuntimeError("compressed_all_reduce: out_seed needs `out`")
    else:
        if isinstance(out, torch.Tensor) and out.dtype in _WIRE_DTYPES and out_seed is None:
            raise RuntimeError("compressed_all_reduce: out must be a flat contiguous float32 tensor of the tensor's length on its device "
                               "(a 16-bit out is rounded stochastically and needs out_seed)")
        if out_seed is not None:
            if not (isinstance(out, torch.Tensor) and out.dtype == out_dtype and out.dim() == 1 and out.is_contiguous()
                    and out.numel() == tensor.numel() and out.device == tensor.device):
                raise RuntimeError("compressed_all_reduce: with out_seed, out must be a flat contiguous tensor of the wire's 16-bit dtype, "
                                   "of the tensor's length on its device")
            if isinstance(out_seed, torch.Tensor):
                if not (out_seed.dtype == torch.int64 and out_seed.numel() == 1 and out_seed.device == tensor.device):
                    raise RuntimeError("compressed_all_reduce: a tensor out_seed must be a 1-element int64 tensor on the tensor's device")
            elif not (isinstance(out_seed, int) and not isinstance(out_seed, bool) and 0 <= out_seed < (1 << 64)):
                raise RuntimeError("compressed_all_reduce: out_seed must be an int in [0, 2^64) or a 1-element int64 tensor")
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.dim() == 1 and out.is_contiguous()
                  and out.numel() == tensor.numel() and out.device == tensor.device):
            raise RuntimeError("compressed_all_reduce: out must be a flat contiguous float32 tensor of the tensor's length on its device")
        if out is tensor and out_accumulate:
            raise RuntimeError("compressed_all_reduce: out is the tensor itself: out_accumulate is not possible")
        if isinstance(out_scale, torch.Tensor):
            if not (out_scale.dtype == torch.float32 and out_scale.numel() == 1 and out_scale.device == tensor.device):
                raise RuntimeError("compressed_all_reduce: a tensor out_scale must be a 0-dim or 1-element float32 tensor on the tensor's device")
            out_scale = out_scale.reshape(())
        elif out_scale is not None:
            f32 = ctypes.c_float(float(out_scale)).value
            if not math.isfinite(f32) or f32 == 0.0:
                raise RuntimeError("compressed_all_reduce: out_scale must be finite and not zero")
            out_scale = torch.tensor(f32, dtype=torch.float32, device=tensor.device)
    if clip_norm is not None:
        clip_norm = float(clip_norm)
        if not (math.isfinite(clip_norm) and clip_norm > 0.0):
            raise RuntimeError("compressed_all_reduce: clip_norm must be a positive finite float")
        norm = True
    world = dist.get_world_size()
    factor = _reduce_factor(op, scale, world)
    one_call = callable(getattr(codec, "decompress_reduce_compress", None)) and world <= _MAX_REDUCE_SOURCES
    mixed = one_call and raw_local and callable(getattr(codec, "decompress_reduce_compress_mixed", None))
    if wire_seed is not None:
        one_call = False  # (the fused reduce-compress kernel rounds to nearest)
    if one_call:
        reduce_compress = codec.decompress_reduce_compress_mixed if mixed else codec.decompress_reduce_compress
        one_call = factor is None or _takes_scale(reduce_compress)
    if one_call:
        shard_words, recv, all_sizes, width = _exchange_shard_rows(tensor, codec, mixed, wire_dtype, residual, residual_fresh)
        me = dist.get_rank()
        shard = torch.empty((shard_words,), dtype=torch.float32, device=tensor.device)
        pair = _norm_pair(tensor.device) if norm else None
        (status, comp, sizes), _ = _reduce_call(reduce_compress, [_rows_with_local(tensor, recv, all_sizes, me, world, mixed)], [shard], factor, pair)
        if not bool(status.all().item()):
            raise RuntimeError("reduce-compress of the received rows failed: a row is malformed or the rows differ in length")
        rs = {
            "raw_bytes": tensor.numel() * tensor.element_size(),
            "wire_bytes": world * width,
            "payload_bytes": int(all_sizes[me].sum().item()),
        }
    else:
        pair = _norm_pair(tensor.device) if norm else None
        if wire_dtype is None:
            shard, rs = compressed_reduce_scatter(tensor, codec, raw_local, scale=factor)
        elif wire_seed is not None:
            shard, rs = compressed_reduce_scatter(tensor, codec, raw_local, scale=factor, wire_dtype=wire_dtype, wire_seed=wire_seed)
        else:
            shard, rs = compressed_reduce_scatter(tensor, codec, raw_local, scale=factor, wire_dtype=wire_dtype, residual=residual,
                                                  residual_fresh=residual_fresh)
        if wire_seed is not None:
            comp, sizes = _compress_stochastic(codec, [shard], out_dtype, wire_seed, world * world + dist.get_rank())
        else:
            comp, sizes = codec.compress_cast([shard], out_dtype)
    gathered_bytes = shard.numel() * (torch.finfo(out_dtype).bits // 8)
    if out is None:
        out = torch.empty(tensor.shape, dtype=out_dtype, device=tensor.device)
        rows = out.view(world, shard.numel())

        def all_gather(coef):
            return _all_gather_archives(comp, sizes, lambda r: [rows[r]], gathered_bytes, codec, scale=coef)
    else:
        rows = out.view(world, shard.numel())

        def all_gather(coef):
            # the factor of the float32 decode: coef, out_scale, or their float32 product (0-dim tensors: nothing is read)
            f = out_scale if coef is None else (coef if out_scale is None else coef * out_scale)
            if out_seed is not None:
                return _all_gather_archives(comp, sizes, lambda r: [rows[r]], gathered_bytes, codec,
                                            decode=lambda r, rws, outs: _decode_update(codec, rws, outs, f, out_accumulate, out_seed, r))
            return _all_gather_archives(comp, sizes, lambda r: [rows[r]], gathered_bytes, codec,
                                        decode=lambda r, rws, accs: _decode_into_float32(codec, rws, accs, f, out_accumulate, out_dtype))
    if clip_norm is not None:
        # the statistics first: the coefficient is known before the gather, whose decode applies it
        if not pair[2]:  # (the words of the archive: the shard rounded as the cast rounds it)
            _norm_by_torch(pair, shard.to(out_dtype))
        both = torch.cat([pair[0], pair[1].to(torch.float64)])
        dist.all_reduce(both)
        # torch.nn.utils.clip_grad_norm_'s formula, in float64 on the device, rounded once to float32
        coef = torch.clamp(clip_norm / (both[0].sqrt() + 1e-6), max=1.0).to(torch.float32)
        _, ag = all_gather(coef)
        stats = {k: rs[k] + ag[k] for k in rs}
        _norm_stats(stats, pair)
        stats["global_sumsq"] = both[0]
        stats["global_nonfinite"] = both[1].to(torch.int32)
        stats["clip_coef"] = coef
        return out, stats
    _, ag = all_gather(None)
    stats = {k: rs[k] + ag[k] for k in rs}
    if norm:
        if not pair[2]:  # (the words of the archive: the shard rounded as the cast rounds it)
            _norm_by_torch(pair, shard.to(out_dtype))
        _norm_stats(stats, pair)
        both = torch.cat([pair[0], pair[1].to(torch.float64)])
        dist.all_reduce(both)
        stats["global_sumsq"] = both[0]
        stats["global_nonfinite"] = both[1].to(torch.int32)
    return out, stats


# ---------------------------------------------------------------------------
# Pipelined compressed all-gather: no host synchronisation between the phases, compression of chunk
# k + 1 overlapped with the exchange of chunk k (and with the decompression of chunk k - 1).
#
#   * rows are exchanged at a FIXED width W = width_fraction x the raw row bytes (rounded up to 16), so the
#     payload collective's shape is known on the host without reading the compressed sizes back.  bf16 / fp16
#     activations and gradients compress to ~0.67 (README.md:45-60 of the reference); the default 0.75
#     leaves headroom.  A row that does not fit is detected from the all-gathered sizes ON THE DEVICE;
#   * the only host synchronisation is ONE read of the "some row overflowed" flag at the very end; if it
#     is set (incompressible data) the affected chunks are gathered again uncompressed;
#   * streams: compress on `comp_stream`; every collective is asynchronous (RCCL runs it on its own
#     stream, ordered after the compress stream at the call); decompress on `dec_stream` after the
#     work handle.  On CPU tensors (gloo, the unit tests) everything degenerates to in-order execution.
def compressed_all_gather_pipelined(tensors, chunks=4, width_fraction=0.75, codec=None):
    """All-gathers a list of equally-shaped float tensors per rank, moving compressed bytes.

    Returns (gathered, stats): gathered[r][i] is rank r's i-th tensor, bit-exact;
    stats = {"raw_bytes", "wire_bytes", "overflow_chunks"} per rank-to-rank copy."""
    codec = codec or GpuFloatCodec()
    world = dist.get_world_size()
    n = len(tensors)
    dev = tensors[0].device
    on_gpu = dev.type == "cuda"
    row_bytes = tensors[0].numel() * tensors[0].element_size()
    assert all(t.shape == tensors[0].shape and t.dtype == tensors[0].dtype for t in tensors)
    # archive = 16-byte float header + non-compressed plane + ANS archive; W must at least hold the overhead
    width = (int(row_bytes * width_fraction) + 15) // 16 * 16
    bounds = [shard_range(n, k, min(chunks, n)) for k in range(min(chunks, n))]

    cur = torch.cuda.current_stream(dev) if on_gpu else None
    comp_stream = torch.cuda.Stream(dev) if on_gpu else None
    dec_stream = torch.cuda.Stream(dev) if on_gpu else None
    if on_gpu:
        comp_stream.wait_stream(cur)  # the inputs were produced on the caller's stream
        dec_stream.wait_stream(cur)

    def on(stream):
        return torch.cuda.stream(stream) if on_gpu else _NullContext()

    pending = []   # (chunk index, payload work, sizes work, gathered payloads, gathered sizes)
    keep = []      # buffers RCCL may still be reading
    for k, (lo, hi) in enumerate(bounds):
        with on(comp_stream):
            comp, sizes = codec.compress(tensors[lo:hi])
            sizes = sizes.to(torch.int32)
            w = min(width, comp.shape[1])
            payload = comp[:, :w].contiguous()
            gp = [torch.empty_like(payload) for _ in range(world)]
            gs = [torch.empty_like(sizes) for _ in range(world)]
            wp = dist.all_gather(gp, payload, async_op=True)
            ws = dist.all_gather(gs, sizes, async_op=True)
            keep.append((comp, payload, sizes))
        pending.append((k, w, wp, ws, gp, gs))

    gathered = [[None] * n for _ in range(world)]
    overflow_flags = []
    for k, w, wp, ws, gp, gs in pending:
        lo, hi = bounds[k]
        with on(dec_stream):
            wp.wait()
            ws.wait()
            all_sizes = torch.stack(gs)                      # [world, rows] on the device
            over = all_sizes > w
            overflow_flags.append(over.any())                # stays on the device
            for r in range(world):
                # rows cut off at the exchange width must not be decoded: blank their header word (device-side)
                gp[r][:, :4].masked_fill_(over[r][:, None], 0)
                rows = [gp[r][i] for i in range(hi - lo)]    # fixed-width rows; the archives say how long they are
                outs = [torch.empty_like(t) for t in tensors[lo:hi]]
                st = codec.decompress(rows, outs)
                # any row that did not decode (cut off at the exchange width, or rejected for another reason) sends
                # its chunk through the uncompressed fall-back: a failed decode never passes for a result
                overflow_flags[-1] = overflow_flags[-1] | (st == 0).any().to(overflow_flags[-1].device)
                gathered[r][lo:hi] = outs
    if on_gpu:
        cur.wait_stream(dec_stream)
        cur.wait_stream(comp_stream)

    # the one host synchronisation: did any row not fit into the fixed width?
    flags = torch.stack(overflow_flags).to("cpu")
    redo = [k for k in range(len(bounds)) if bool(flags[k])]
    for k in redo:
        lo, hi = bounds[k]
        raw = torch.stack([t.reshape(-1) for t in tensors[lo:hi]])
        got = [torch.empty_like(raw) for _ in range(world)]
        dist.all_gather(got, raw)
        for r in range(world):
            gathered[r][lo:hi] = [got[r][i].reshape(tensors[lo + i].shape) for i in range(hi - lo)]
    stats = {
        "raw_bytes": n * row_bytes,
        "wire_bytes": n * min(width, keep[0][0].shape[1]) + sum((hi - lo) * row_bytes for lo, hi in (bounds[k] for k in redo)),
        "overflow_chunks": len(redo),
        "chunks": len(bounds),
    }
    return gathered, stats


class _NullContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ---------------------------------------------------------------------------
# The same exchanges as a reusable PLAN for a fixed shard shape (a training loop moves the same buffers every
# step): every buffer and stream is created once; a step is K compress calls, K asynchronous collectives and
# K x world decompress calls straight on the C ABI -- no Python lists of tensors, no per-step allocation, no copy
# between the codec's output and the send buffer:
#
#   * rows travel at a fixed WIDTH (bytes).  The encoder writes every row straight into the send matrix at that
#     stride and stores nothing beyond it (dgpu_float_compress_stride_capped); the decoder is told how many bytes
#     a received row has and rejects a row whose archive claims more (dgpu_float_decompress_stride_bounded).  So a
#     row that did not fit shows up as status 0 on every receiver -- no size exchange on the data path at all;
#   * the width comes from the DATA: the first call probes (compresses its first chunk, one extra host sync, all
#     ranks agree through an all-reduce MAX); every call folds the largest compressed row of all ranks into the ONE
#     device-to-host read it ends with, and the next call uses that + 1/64 headroom.  Steady-state traffic has the
#     same statistics step after step (activations, gradients), so fall-backs are rare -- and cheap:
#   * fall-back is per ROW: rows with status 0 are gathered again uncompressed in one padded collective, the others
#     are not touched;
#   * all_gather(shard [n, elems]) -> [world, n, elems] and all_to_all(send [world, m, elems]) -> [world, m, elems]
#     share all of this.
# The codec is pluggable (compress rows into a strided matrix with a capacity, decompress rows with a bound), so the
# world-2 logic runs on CPU under gloo with the oracle as codec (tests/test_sharding_gloo.py).
class CAbiFloatCodec:
    """The HIP float codec through the C ABI's capped / bounded stride entry points."""

    def __init__(self, dtype, elems, max_rows, prob_bits=10, device=None):
        import ctypes as C

        from . import lib
        from .ops import _DTYPE_TO_FT

        self.C, self.L = C, lib()
        self.ft = _DTYPE_TO_FT[dtype]
        self.P = prob_bits
        self.elems = elems
        if elems <= 4096:
            # dgpu_float_compress_stride_capped takes rows of more than one 4096-word block (single-block rows go to
            # the two-elements-per-wavefront encoder, which does not clamp its copy-out); say so HERE, not at the
            # first exchange.  Rows that small gain nothing from the codec anyway (~700 bytes of tables per row).
            raise ValueError(f"compressed collectives need rows of more than 4096 elements (got {elems}): "
                             "exchange such shards uncompressed, or fold several rows into one")
        self.cap = int(self.L.dgpu_float_max_compressed_size(self.ft, elems))
        self.elem_bytes = torch.empty((), dtype=dtype).element_size()
        self.min_width = (16 + (elems + 15) // 16 * 16 * (3 if self.ft == 3 else 1) + 32 + 512 + 136 * ((elems + 4095) // 4096 + 1) + 15) // 16 * 16
        tb = max(int(self.L.dgpu_float_compress_temp_bytes(self.ft, max_rows, elems)),
                 int(self.L.dgpu_float_decompress_temp_bytes(self.ft, max_rows, elems, prob_bits)))
        # one temp region per stream: calls on different streams run concurrently
        self.temp_c = torch.empty((tb,), dtype=torch.uint8, device=device)
        self.temp_d = torch.empty((tb,), dtype=torch.uint8, device=device)
        self.err = C.c_int32(-1)

    def compress_into(self, rows, out, width, sizes, stream):
        """rows [m, elems] (contiguous) -> out [m, width] (contiguous uint8), sizes [m] int32 = full archive sizes."""
        C, L = self.C, self.L
        m = rows.shape[0]
        rc = L.dgpu_float_compress_stride_capped(
            C.c_void_p(self.temp_c.data_ptr()), self.temp_c.numel(), None, self.ft, self.P, 0, m,
            C.c_void_p(rows.data_ptr()), self.elems, self.elems * self.elem_bytes,
            C.c_void_p(out.data_ptr()), width, width, C.c_void_p(sizes.data_ptr()), C.c_void_p(stream))
        if rc:
            raise RuntimeError(L.dgpu_last_error().decode())

    def decompress_from(self, rows, width, out, status, stream):
        """rows [m, width] -> out [m, elems]; status [m] uint8 = 0 for rows that are incomplete / not decodable."""
        C, L = self.C, self.L
        m = rows.shape[0]
        rc = L.dgpu_float_decompress_stride_bounded(
            C.c_void_p(self.temp_d.data_ptr()), self.temp_d.numel(), None, self.ft, self.P, 0, m,
            C.c_void_p(rows.data_ptr()), width, width, C.c_void_p(out.data_ptr()), self.elems * self.elem_bytes,
            self.elems, C.c_void_p(status.data_ptr()), None, C.c_void_p(stream), C.byref(self.err))
        if rc:
            raise RuntimeError(L.dgpu_last_error().decode())


class CompressedExchangePlan:
    """all_gather / all_to_all of float rows that moves compressed bytes.  See the comment block above."""

    HEADROOM = 1.0 / 64.0

    def __init__(self, dtype, elems, rows, chunks=4, prob_bits=10, device=None, codec=None, initial_width=None, depth=1):
        """`depth`: buffer sets of the plan.  1: every call ends with its one host read (all_gather / all_to_all).  2: a
        step can be ENQUEUED (all_gather_async) while the previous one is still unchecked, so that the host read of step
        k (ExchangeHandle.wait) happens behind the launch of step k + 1 and a steady-state step is launch-only."""
        self.world = dist.get_world_size()
        self.dev = torch.device(device) if device is not None else torch.device("cpu")
        self.on_gpu = self.dev.type == "cuda"
        self.dtype, self.elems, self.rows = dtype, elems, rows
        self.row_bytes = elems * torch.empty((), dtype=dtype).element_size()
        self.codec = codec or CAbiFloatCodec(dtype, elems, rows, prob_bits, self.dev)
        self.cap = self.codec.cap
        self.chunks = max(1, min(chunks, rows))
        self.bounds = [shard_range(rows, k, self.chunks) for k in range(self.chunks)]
        u8 = dict(dtype=torch.uint8, device=self.dev)
        # send / receive matrices are flat and sized for the worst case; a step uses the first rows x width bytes.
        # `depth` sets of them; the attributes below (send, recv, sizes, status, stat, out) always name the set of the step
        # that is being enqueued or finished (_bind)
        self._slots = [{
            "send": torch.empty((rows * self.cap,), **u8),
            "recv": torch.empty((self.world * rows * self.cap,), **u8),
            "sizes": torch.zeros((rows,), dtype=torch.int32, device=self.dev),
            "status": torch.zeros((self.world, rows), **u8),
            "stat": torch.zeros((2,), dtype=torch.int32, device=self.dev),  # {largest archive of all ranks, rows decoded}
            "max_work": None, "out": None, "pending": None,
        } for _ in range(max(1, int(depth)))]
        self._cur = 0
        self._bind(self._slots[0])
        self.width = None if initial_width is None else self._round_width(initial_width)
        self._width_agreed = initial_width is None  # widths derived from all-reduced sizes agree by construction
        self.comp_stream = torch.cuda.Stream(self.dev) if self.on_gpu else None
        self.dec_stream = torch.cuda.Stream(self.dev) if self.on_gpu else None
        self.last = {}

    # ---- helpers
    def _bind(self, slot):
        self._slot = slot
        self.send, self.recv, self.sizes, self.status, self.stat = slot["send"], slot["recv"], slot["sizes"], slot["status"], slot["stat"]
        self._max_work, self.out = slot["max_work"], slot["out"]

    def _unbind(self):
        self._slot["max_work"], self._slot["out"] = self._max_work, self.out

    def _next_slot(self):
        """The buffer set of the step about to be enqueued; its previous step must have been waited for."""
        self._unbind()
        self._cur = (self._cur + 1) % len(self._slots)
        slot = self._slots[self._cur]
        if slot["pending"] is not None:
            slot["pending"].wait()  # (a caller that never waits: the step that used these buffers is finished first)
        self._bind(slot)
        return slot

    def _streams_of_step(self):
        """(caller's stream, compress stream, decompress stream) of the step being enqueued.  A step of ONE chunk has
        nothing to overlap between its compress and its decompress side: everything stays on the caller's stream, and
        the four stream hand-offs of the pipelined form -- an event record, a wait and ~15 us of idle GPU each at world
        1 -- are not paid (profiles/r06_collective_world1.txt)."""
        cur = torch.cuda.current_stream(self.dev) if self.on_gpu else None
        if not self.on_gpu or self.chunks == 1:
            return cur, cur, cur
        self.comp_stream.wait_stream(cur)  # the inputs were produced on the caller's stream
        self.dec_stream.wait_stream(cur)
        return cur, self.comp_stream, self.dec_stream

    def _join_streams_of_step(self, cur, cs, ds):
        if self.on_gpu and cs is not cur:
            cur.wait_stream(cs)
            cur.wait_stream(ds)

    def _round_width(self, nbytes):
        w = (int(nbytes) + 15) // 16 * 16
        return max(min(w, self.cap), min(self.codec.min_width, self.cap))

    def _stream_ptr(self, s):
        return s.cuda_stream if s is not None else 0

    def _on(self, s):
        return torch.cuda.stream(s) if s is not None else _NullContext()

    def _agree_on_width(self):
        """A caller-given initial width must be the SAME on every rank (it is the row stride of the collectives):
        the first call makes it so (MAX over ranks, one tiny all-reduce, once)."""
        if self._width_agreed or self.world == 1:
            self._width_agreed = True
            return
        w = torch.tensor([self.width], dtype=torch.int32, device=self.dev)
        dist.all_reduce(w, op=dist.ReduceOp.MAX)
        self.width = self._round_width(int(w.item()))
        self._width_agreed = True

    def _probe_width(self, rows2d):
        """First call: compress the first chunk once, all ranks agree on max(size) -> width (one host sync)."""
        lo, hi = self.bounds[0]
        m = hi - lo
        view = self.send[: m * self.cap].view(m, self.cap)
        self.codec.compress_into(rows2d[lo:hi], view, self.cap, self.sizes[lo:hi], self._stream_ptr(torch.cuda.current_stream(self.dev) if self.on_gpu else None))
        mx = self.sizes[lo:hi].max().to(torch.int32).reshape(1)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        self.width = self._round_width(int(mx.item()) * (1.0 + self.HEADROOM) + 64)
        self._width_agreed = True

    def _post_compress(self):
        """Right after the last compress call (on the compress stream): the largest archive of all ranks, as an
        asynchronous all-reduce that overlaps with the exchange and the decompression."""
        torch.amax(self.sizes, dim=0, keepdim=True, out=self.stat[0:1])
        self._max_work = dist.all_reduce(self.stat[0:1], op=dist.ReduceOp.MAX, async_op=True) if self.world > 1 else None

    def _post_decode(self):
        """The device side of a step's check, enqueued with the step (on the caller's stream, behind the decode stream):
        rows that decoded, agreed over the ranks -- the fall-back is a collective, every rank must agree on whether it
        runs (in the all-to-all only sender and receiver see a row's status; in the all-gather a local decode rejection
        must not desynchronise the ranks) -- and both statistics on their way to pinned host memory."""
        torch.sum(self.status.view(-1), dim=0, keepdim=True, dtype=torch.int32, out=self.stat[1:2])
        if self.world > 1:
            dist.all_reduce(self.stat[1:2], op=dist.ReduceOp.MIN)
        if self._max_work is not None:
            self._max_work.wait()
            self._max_work = None
        slot = self._slot
        slot["width"] = self.width
        if self.on_gpu:
            if slot.get("host") is None:
                slot["host"] = torch.empty((2,), dtype=torch.int32).pin_memory()
                slot["event"] = torch.cuda.Event()
            slot["host"].copy_(self.stat, non_blocking=True)
            slot["event"].record()

    def _finish(self, kind, fallback):
        """The ONE device-to-host read of a step: {largest archive over all ranks, rows that decoded}."""
        slot = self._slot
        if self.on_gpu:
            slot["event"].synchronize()
            largest, decoded = (int(v) for v in slot["host"].tolist())
        else:
            largest, decoded = (int(v) for v in self.stat.tolist())
        failed = self.status.numel() - decoded
        used_width = slot["width"]
        redo = fallback() if failed else 0
        self.last = {"kind": kind, "width": used_width, "largest_archive": largest, "rows_sent_uncompressed": redo,
                     "wire_bytes": self.rows * used_width + redo * self.row_bytes, "raw_bytes": self.rows * self.row_bytes}
        # next step's width: what the data needed + headroom (it only moves when the data moves)
        self.width = self._round_width(largest * (1.0 + self.HEADROOM) + 64)
        return redo

    def _handle(self, kind, fallback):
        self._post_decode()
        self._unbind()
        h = ExchangeHandle(self, self._slot, kind, fallback)
        self._slot["pending"] = h
        return h

    # ---- all-gather
    def all_gather(self, shard):
        """shard [rows, elems] -> (gathered [world, rows, elems], rows that had to be sent uncompressed)."""
        return self.all_gather_async(shard).wait()

    def all_gather_async(self, shard):
        """Enqueues the step and returns an ExchangeHandle WITHOUT reading anything back: `handle.wait()` -> (gathered,
        rows sent uncompressed) does the step's one host read and, if rows did not fit the exchange width, their
        uncompressed fall-back.  The output is complete only after wait(); `shard` must stay unchanged until then.  With
        a plan of depth 2 the wait of step k belongs behind the call that enqueues step k + 1."""
        assert shard.shape == (self.rows, self.elems) and shard.dtype == self.dtype and shard.is_contiguous()
        self._next_slot()
        if self.out is None or self.out.shape[0] != self.world or self.out.dim() != 3:
            self.out = torch.empty((self.world, self.rows, self.elems), dtype=self.dtype, device=self.dev)
        if self.width is None:
            self._probe_width(shard)
        self._agree_on_width()
        W, world = self.width, self.world
        cur, cs, ds = self._streams_of_step()
        works = []
        with self._on(cs):
            for k, (lo, hi) in enumerate(self.bounds):
                m = hi - lo
                snd = self.send[lo * W : hi * W].view(m, W)
                self.codec.compress_into(shard[lo:hi], snd, W, self.sizes[lo:hi], self._stream_ptr(cs))
                rcv = self.recv[world * lo * W : world * hi * W]
                works.append(_all_gather_flat(rcv, snd.view(-1), world))
            self._post_compress()
        with self._on(ds):
            for k, (lo, hi) in enumerate(self.bounds):
                m = hi - lo
                if works[k] is not None:
                    works[k].wait()
                rcv = self.recv[world * lo * W : world * hi * W].view(world, m, W)
                for r in range(world):
                    self.codec.decompress_from(rcv[r], W, self.out[r, lo:hi], self.status[r, lo:hi], self._stream_ptr(ds))
        self._join_streams_of_step(cur, cs, ds)

        status_of_step, out_of_step = self.status, self.out

        def fallback():
            # per ROW: the rows that failed are gathered again uncompressed, padded to the largest count of any rank.
            # Every rank decoded the same archives, so the status matrices SHOULD be equal -- but the fall-back is a
            # collective whose shapes derive from them, so they are made equal (a row is bad if ANY rank could not
            # decode it: MIN over ranks of a world x rows byte matrix) rather than assumed to be.
            agreed = status_of_step.to(torch.int32)
            if world > 1:
                dist.all_reduce(agreed, op=dist.ReduceOp.MIN)
            bad = (agreed == 0)                                       # [world, rows]
            counts = bad.sum(dim=1).tolist()
            width = max(counts)
            mine = bad[dist.get_rank()].nonzero().flatten()
            pack = torch.zeros((width, self.elems), dtype=self.dtype, device=self.dev)
            pack[: mine.numel()] = shard[mine]
            got = torch.empty((world, width, self.elems), dtype=self.dtype, device=self.dev)
            w = _all_gather_flat(got.view(-1), pack.view(-1), world)
            if w is not None:
                w.wait()
            for r in range(world):
                idx = bad[r].nonzero().flatten()
                out_of_step[r, idx] = got[r, : idx.numel()]
            return counts[dist.get_rank()]

        # (the count of decoded rows is all-reduced too: every rank must agree on WHETHER the fall-back collective runs)
        return self._handle("all_gather", fallback)

    # ---- all-to-all
    def all_to_all(self, send):
        """send [world, m, elems] (row block j goes to rank j) -> (received [world, m, elems] (block i came from rank i),
        rows of this rank's receive side that had to be sent uncompressed)."""
        return self.all_to_all_async(send).wait()

    def all_to_all_async(self, send):
        """all_to_all without the host read: see all_gather_async."""
        world = self.world
        assert send.dim() == 3 and send.shape[0] == world and send.shape[2] == self.elems and send.is_contiguous()
        m = send.shape[1]
        assert world * m == self.rows and send.dtype == self.dtype
        self._next_slot()
        if self.out is None or self.out.shape != send.shape:
            self.out = torch.empty_like(send)
        flat = send.view(world * m, self.elems)
        if self.width is None:
            self._probe_width(flat)
        self._agree_on_width()
        W = self.width
        cur, cs, ds = self._streams_of_step()
        # chunk k = rows [lo_k, hi_k) of EVERY destination block, so that each chunk is a complete all-to-all
        cb = [shard_range(m, k, min(self.chunks, m)) for k in range(min(self.chunks, m))]
        works = []
        base = 0
        with self._on(cs):
            for lo, hi in cb:
                c = hi - lo
                snd = self.send[base * W : (base + world * c) * W].view(world, c, W)
                for j in range(world):
                    self.codec.compress_into(send[j, lo:hi], snd[j], W, self.sizes[j * m + lo : j * m + hi], self._stream_ptr(cs))
                rcv = self.recv[base * W : (base + world * c) * W]
                works.append((_all_to_all_flat(rcv, snd.view(-1), world), base, lo, hi))
                base += world * c
            self._post_compress()
        st = self.status.view(-1)[: world * m].view(world, m)
        with self._on(ds):
            for wk, b0, lo, hi in works:
                c = hi - lo
                if wk is not None:
                    wk.wait()
                rcv = self.recv[b0 * W : (b0 + world * c) * W].view(world, c, W)
                for i in range(world):
                    self.codec.decompress_from(rcv[i], W, self.out[i, lo:hi], st[i, lo:hi], self._stream_ptr(ds))
        self._join_streams_of_step(cur, cs, ds)
        if world * m < self.status.numel():
            self.status.view(-1)[world * m :] = 1
        out_of_step = self.out

        def fallback():
            # per ROW.  Only sender and receiver know which rows failed: the receiver tells every sender (a tiny
            # all-gather of the status matrix), then the rows travel uncompressed in an all-to-all with uneven splits
            mine = (st == 0).to(torch.uint8)                              # [src, m] as seen by me, the receiver
            allst = torch.empty((world, world, m), dtype=torch.uint8, device=self.dev)
            w0 = _all_gather_flat(allst.view(-1), mine.reshape(-1).contiguous(), world)
            if w0 is not None:
                w0.wait()
            me = dist.get_rank()
            bad_send = allst[:, me, :].bool()                             # [dst, m]: my rows that dst could not decode
            bad_recv = mine.bool()                                        # [src, m]
            in_split = bad_send.sum(dim=1).tolist()
            out_split = bad_recv.sum(dim=1).tolist()
            pack = send[bad_send]                                         # rows ordered by destination
            got = torch.empty((sum(out_split), self.elems), dtype=self.dtype, device=self.dev)
            dist.all_to_all_single(got, pack.contiguous(), out_split, in_split)
            out_of_step[bad_recv] = got
            return sum(out_split)

        return self._handle("all_to_all", fallback)


class ExchangeHandle:
    """A step of a CompressedExchangePlan that has been enqueued but not checked.  wait() -> (output, rows that had to be
    sent uncompressed): the step's ONE device-to-host read (largest archive of all ranks, rows that decoded), the per-row
    uncompressed fall-back if rows did not fit, and the width of the next step.

    Lifetimes and ordering (the plan owns `depth` buffer sets and hands them out round robin):
      * the tensor wait() returns IS the buffer set's output: it is valid until that buffer set is used again, i.e.
        until the enqueue of step k + depth -- copy it (or pass clone=True) to keep it longer;
      * the caller's input (`shard` / `send`) must stay unchanged until wait(): the per-row fall-back reads it then;
      * wait() may run a collective (the fall-back), so every rank must wait for its handles in the SAME order relative
        to its other collectives -- in particular before enqueueing step k + depth: an enqueue that finds its buffer
        set still pending finishes that step first, and does so on every rank only if every rank left it pending."""

    def __init__(self, plan, slot, kind, fallback):
        self.plan, self.slot, self.kind, self.fallback, self.result = plan, slot, kind, fallback, None

    def wait(self, clone=False):
        if self.result is None:
            p = self.plan
            cur = p._slot
            p._unbind()
            p._bind(self.slot)
            try:
                redo = p._finish(self.kind, self.fallback)
                self.result = (p.out, redo)
            finally:
                p._unbind()
                p._bind(cur)
            self.slot["pending"] = None
        if clone:  # an output of the caller's own instead of the buffer set's (valid beyond step k + depth)
            return (self.result[0].clone(), self.result[1])
        return self.result


def _all_gather_flat(out_flat, in_flat, world):
    """all-gather of flat byte / word tensors, asynchronous where the backend can (returns the work handle or None)."""
    if dist.get_backend() == "gloo" or not in_flat.is_cuda:
        parts = list(out_flat.view(world, -1).unbind(0))
        dist.all_gather(parts, in_flat)
        return None
    return dist.all_gather_into_tensor(out_flat, in_flat, async_op=True)


def _all_to_all_flat(out_flat, in_flat, world):
    """all-to-all of equal flat slices (slice j of in_flat goes to rank j), asynchronous on RCCL."""
    if not in_flat.is_cuda or dist.get_backend() == "gloo":
        dist.all_to_all_single(out_flat, in_flat)
        return None
    return dist.all_to_all_single(out_flat, in_flat, async_op=True)


class CompressedAllGatherPlan(CompressedExchangePlan):
    """The all-gather of one [n, elems] shard (kept under its round-2 name; bench.py --collective)."""

    def __init__(self, shard, chunks=4, prob_bits=10, initial_width=None, codec=None, depth=1):
        assert shard.dim() == 2 and shard.is_contiguous()
        super().__init__(shard.dtype, shard.shape[1], shard.shape[0], chunks=chunks, prob_bits=prob_bits,
                         device=shard.device, codec=codec, initial_width=initial_width, depth=depth)

    def run(self, shard):
        return self.all_gather(shard)

    def run_async(self, shard):
        return self.all_gather_async(shard)

    @property
    def wire_bytes(self):
        return self.last.get("wire_bytes", self.rows * (self.width or self.cap))

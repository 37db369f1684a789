"""Decode-accumulate on the GPU (dgpu_float_decode_accumulate, k_ans_decode_accum): float archives decoded, widened to
float32 and stored to / added into float32 accumulators.  Every expected value is built on the host from the inputs --
the exact widening (torch on the CPU) and numpy float32 adds -- and compared BIT FOR BIT."""
import ctypes
import functools
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the smallest sizes that reach every path: one partial row (1, 31); a full block and one word into the next (4095,
# 4096, 4097); a 4-block tile with two waves' worth (2 x 4096 + 5); the last capacity of the 4-block geometry (8 x 4096)
# and the first of the 16-block one (+ 1); a second 16-block tile holding one short block (16 x 4096 + 33); 40000
SIZES = (1, 31, 4095, 4096, 4097, 2 * 4096 + 5, 8 * 4096, 8 * 4096 + 1, 16 * 4096 + 33, 40000)
DTYPES = {1: torch.float16, 2: torch.bfloat16, 3: torch.float32}
GUARD = 64
SENTINEL = np.array([0xCDCDCDCD], dtype=np.uint32).view(np.int32)[0]


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(ft, seed=0):
    """-> (tensors on the GPU, their exact float32 widening on the host as numpy), one per SIZES"""
    g = torch.Generator().manual_seed(1234 + 17 * ft + seed)
    host = [torch.randn(n, generator=g).to(DTYPES[ft]) for n in SIZES]
    return [t.to(_dev()) for t in host], [t.to(torch.float32).numpy() for t in host]


@functools.lru_cache(maxsize=None)
def _archives(ft, prob_bits, seed=0):
    import dietgpu_amd as dg

    comp, sizes, _ = dg.compress_data(True, _inputs(ft, seed)[0], False, None, prob_bits=prob_bits)
    return [comp[i, :n] for i, n in enumerate(sizes.tolist())]


class Acc:
    """A float32 accumulator of n words `offset` words past a 16-byte boundary, 64 guard words on each side."""

    def __init__(self, n, offset=0, fill=None):
        self.n, self.lo = n, GUARD + offset
        self.buf = torch.full((self.lo + n + GUARD,), 0, dtype=torch.int32, device=_dev())
        self.buf.fill_(int(SENTINEL))
        self.view = self.buf[self.lo : self.lo + n].view(torch.float32)
        assert self.view.data_ptr() % 16 == 4 * (offset % 4)
        if fill is not None:
            self.view.copy_(torch.from_numpy(fill))

    def bits(self):
        return self.buf[self.lo : self.lo + self.n].cpu().numpy().view(np.uint32)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[: self.lo] == SENTINEL).all() and (b[self.lo + self.n :] == SENTINEL).all())


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _random_acc(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 3.0).numpy()


@pytest.mark.parametrize("prob_bits", [9, 10, 11])
@pytest.mark.parametrize("ft", [1, 2, 3])
def test_widening_store(ft, prob_bits):
    import dietgpu_amd as dg

    _, wide = _inputs(ft)
    rows = _archives(ft, prob_bits)
    # every size as a batch of one, then all of them in one batch (geometry from the largest, work lists if the policy says so)
    batches = [[i] for i in range(len(SIZES))] + [list(range(len(SIZES)))]
    for members in batches:
        accs = [Acc(SIZES[i]) for i in members]
        status = torch.zeros(len(members), dtype=torch.uint8, device=_dev())
        sizes = torch.zeros(len(members), dtype=torch.int32, device=_dev())
        used = dg.decompress_data_accumulate([rows[i] for i in members], [a.view for a in accs], False, None, status, sizes,
                                             prob_bits=prob_bits)
        assert used == 0
        assert status.tolist() == [1] * len(members)
        assert sizes.tolist() == [SIZES[i] for i in members]
        for i, a in zip(members, accs):
            assert np.array_equal(a.bits(), _bits(wide[i])), f"size {SIZES[i]} in a batch of {len(members)}"
            assert a.guards_intact(), f"size {SIZES[i]} in a batch of {len(members)}: guard words overwritten"


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_accumulate_twice(ft):
    import dietgpu_amd as dg

    _, a_wide = _inputs(ft)
    _, b_wide = _inputs(ft, seed=1)
    start = [_random_acc(n, 50 + k) for k, n in enumerate(SIZES)]
    accs = [Acc(n, fill=start[k]) for k, n in enumerate(SIZES)]
    for rows in (_archives(ft, 10), _archives(ft, 10, seed=1)):
        status = torch.zeros(len(SIZES), dtype=torch.uint8, device=_dev())
        dg.decompress_data_accumulate(rows, [a.view for a in accs], True, None, status, None)
        assert status.tolist() == [1] * len(SIZES)
    for k, a in enumerate(accs):
        want = ((start[k] + a_wide[k]).astype(np.float32) + b_wide[k]).astype(np.float32)
        assert np.array_equal(a.bits(), _bits(want)), f"size {SIZES[k]}"
        assert a.guards_intact()


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("ft", [1, 2, 3])
def test_unaligned_accumulators(ft, offset):
    import dietgpu_amd as dg

    _, wide = _inputs(ft)
    rows = _archives(ft, 10)
    for accumulate in (False, True):
        start = [_random_acc(n, 90 + k) for k, n in enumerate(SIZES)]
        accs = [Acc(n, offset, fill=start[k] if accumulate else None) for k, n in enumerate(SIZES)]
        status = torch.zeros(len(SIZES), dtype=torch.uint8, device=_dev())
        dg.decompress_data_accumulate(rows, [a.view for a in accs], accumulate, None, status, None)
        assert status.tolist() == [1] * len(SIZES)
        for k, a in enumerate(accs):
            want = (start[k] + wide[k]).astype(np.float32) if accumulate else wide[k]
            assert np.array_equal(a.bits(), _bits(want)), f"size {SIZES[k]}, accumulate={accumulate}"
            assert a.guards_intact()


def _special_words(ft):
    if ft == 3:
        pats = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF,
                0x00400000, 0x00800000, 0x3F800000, 0xBF800001]
        w = np.array(pats, dtype=np.uint32)
        return torch.from_numpy(np.resize(w, 4097).view(np.int32).copy()).view(torch.float32)
    if ft == 1:
        pats = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x7BFF, 0xFBFF, 0x0001, 0x83FF, 0x0200, 0x0400, 0x3C00, 0xBC01]
    else:
        pats = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x7F7F, 0xFF7F, 0x0001, 0x807F, 0x0040, 0x0080, 0x3F80, 0xBF81]
    w = np.array(pats, dtype=np.uint16)
    return torch.from_numpy(np.resize(w, 4097).view(np.int16).copy()).view(DTYPES[ft])


@pytest.mark.parametrize("ft", [1, 2, 3])
def test_special_values(ft):
    import dietgpu_amd as dg

    n = 4097
    x = _special_words(ft)
    wide = x.to(torch.float32).numpy()
    # accumulator: finite values, float32 denormals, +-inf and +-0, at a stride co-prime to the 13 input patterns
    acc_pats = np.array([0x3F800000, 0xC0490FDB, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x00000000,
                         0x80000000, 0x7F7FFFFF, 0x00800000], dtype=np.uint32)
    start = np.resize(acc_pats, n).view(np.float32).copy()
    comp, sizes, _ = dg.compress_data(True, [x.to(_dev())], False, None)
    row = comp[0, : int(sizes[0])]
    with np.errstate(all="ignore"):
        want_sum = (start + wide).astype(np.float32)
    for accumulate, want in ((False, wide), (True, want_sum)):
        a = Acc(n, fill=start if accumulate else None)
        status = torch.zeros(1, dtype=torch.uint8, device=_dev())
        dg.decompress_data_accumulate([row], [a.view], accumulate, None, status, None)
        assert status.tolist() == [1]
        got = a.bits()
        nan = np.isnan(want)
        assert nan.any() and (~nan).any()
        assert np.isnan(got.view(np.float32)[nan]).all()
        bad = np.nonzero(got[~nan] != _bits(want)[~nan])[0]
        assert bad.size == 0, f"accumulate={accumulate}: {bad.size} words differ, first at {bad[:4]}"
        assert a.guards_intact()


def test_failures_leave_the_accumulator_alone():
    import dietgpu_amd as dg

    members = [4, 5, 9]  # 4097, 2 x 4096 + 5, 40000
    _, wide = _inputs(2)
    rows = [_archives(2, 10)[i] for i in members]
    other_type = _archives(1, 10)[5]
    n1 = SIZES[members[1]]
    cases = {
        "truncated by 16 bytes": ([rows[0], rows[1][:-16], rows[2]], n1),
        "capacity one word short": (rows, n1 - 1),
        "another float type": ([rows[0], other_type, rows[2]], n1),
    }
    for name, (ins, cap1) in cases.items():
        start = [_random_acc(SIZES[i], 70 + i) for i in members]
        accs = [Acc(SIZES[members[0]], fill=start[0]), Acc(cap1, fill=start[1][:cap1]), Acc(SIZES[members[2]], fill=start[2])]
        status = torch.full((3,), 7, dtype=torch.uint8, device=_dev())
        sizes = torch.zeros(3, dtype=torch.int32, device=_dev())
        dg.decompress_data_accumulate(ins, [a.view for a in accs], True, None, status, sizes)
        assert status.tolist() == [1, 0, 1], name
        assert sizes.tolist() == [SIZES[i] for i in members], name  # the header is valid in every case
        assert np.array_equal(accs[1].bits(), _bits(start[1][:cap1])), name + ": the failing member's accumulator changed"
        for k in (0, 2):
            want = (start[k] + wide[members[k]]).astype(np.float32)
            assert np.array_equal(accs[k].bits(), _bits(want)), name
        assert all(a.guards_intact() for a in accs), name


def test_routes_agree():
    import dietgpu_amd as dg

    _, wide = _inputs(2)
    rows = _archives(2, 10)
    start = [_random_acc(n, 20 + k) for k, n in enumerate(SIZES)]
    results = []
    try:
        for route in (False, True):
            dg.prefer_torch_ops(route)
            accs = [Acc(n, fill=start[k]) for k, n in enumerate(SIZES)]
            assert dg.decompress_data_accumulate(rows, [a.view for a in accs], True) == 0
            results.append([a.bits() for a in accs])
    finally:
        dg.prefer_torch_ops(True)
    accs = [Acc(n, fill=start[k]) for k, n in enumerate(SIZES)]
    B = len(SIZES)
    used = ctypes.c_size_t(99)
    rc = dg.lib().dgpu_float_decode_accumulate(
        None, 0, ctypes.byref(used), 2, 10, 1, B, (ctypes.c_void_p * B)(*[r.data_ptr() for r in rows]),
        (ctypes.c_uint32 * B)(*[r.numel() for r in rows]), (ctypes.c_void_p * B)(*[a.view.data_ptr() for a in accs]),
        (ctypes.c_uint32 * B)(*SIZES), None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and used.value == 0
    results.append([a.bits() for a in accs])
    for k in range(B):
        want = _bits((start[k] + wide[k]).astype(np.float32))
        for r in results:
            assert np.array_equal(r[k], want), f"size {SIZES[k]}"


def test_graph_replay_accumulates():
    import dietgpu_amd as dg

    members = [4, 9]
    _, wide = _inputs(2)
    rows = [_archives(2, 10)[i] for i in members]
    start = [_random_acc(SIZES[i], 30 + i) for i in members]
    accs = [Acc(SIZES[i], fill=start[k]) for k, i in enumerate(members)]
    views = [a.view for a in accs]
    status = torch.zeros(2, dtype=torch.uint8, device=_dev())

    def call():  # (dtype given: reading the header would synchronise, which a capture cannot hold)
        dg.decompress_data_accumulate(rows, views, True, None, status, None, dtype=torch.bfloat16)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # makes the parameter block resident
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    torch.cuda.synchronize()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert status.tolist() == [1, 1]
    for k, i in enumerate(members):
        want = start[k]
        for _ in range(3):  # the call before the capture and two replays (a capture does not execute)
            want = (want + wide[i]).astype(np.float32)
        assert np.array_equal(accs[k].bits(), _bits(want)), f"size {SIZES[i]}"
        assert accs[k].guards_intact()
    del graph
    dg.lib().dgpu_release_graph_state()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_compressed_reduce_scatter_single_rank_rccl():
    import torch.distributed as dist

    import dietgpu_amd
    from dietgpu_amd import distributed as D

    dietgpu_amd.lib()
    os.environ.update(RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dev = _dev()
    torch.cuda.set_device(dev)
    D.init(backend="nccl", device=dev)  # "nccl" is RCCL on ROCm
    try:
        g = torch.Generator(device="cpu").manual_seed(9)
        mine = torch.randn(100_000 + 33, generator=g).to(torch.bfloat16)
        shard, stats = D.compressed_reduce_scatter(mine.to(dev))
        assert shard.dtype == torch.float32 and shard.shape == mine.shape
        assert np.array_equal(shard.cpu().numpy().view(np.uint32), _bits(mine.to(torch.float32).numpy()))
        assert stats["payload_bytes"] < 0.75 * stats["raw_bytes"]
        assert stats["wire_bytes"] < 0.80 * stats["raw_bytes"]
    finally:
        dist.destroy_process_group()

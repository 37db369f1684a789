"""Decode-update on the GPU (dgpu_float_decode_update, k_ans_decode_update): 16-bit float archives multiplied by a
float32 factor, added to or stored over 16-bit tensors of the archive's type and rounded stochastically.  Every expected
word comes from tests/sr_ref.py and is compared BIT FOR BIT (the sign of a NaN masked on both sides: the contract leaves
it open).  The archives are written by compress_data, whose output the parity tests pin.  All tensors of a call lie in one
flat buffer, side by side at odd word offsets, with canary words before, between and behind them."""
import numpy as np
import pytest
import torch

import cast_ref as R
import sr_ref as S

pytestmark = pytest.mark.gpu

DTYPE = {S.FLOAT16: torch.float16, S.BFLOAT16: torch.bfloat16}
FTS = (S.FLOAT16, S.BFLOAT16)
#  (prob_bits, route): the op at the default precision, ctypes at 9 and 11 (and at 10)
ROUTES = [(10, "torch_ops"), (10, "ctypes"), (9, "ctypes"), (11, "ctypes")]
SMALL = [0, 1, 31, 4095, 4096, 4097, 3 * 4096 + 5]          # every capacity within 4 blocks: 4-block tiles
LARGE = [16 * 4096 + 4097, 70000, 5]                        # 16-block tiles, several tiles per member
CANARY = 0x5A5B
THIRD = float(np.float32(1.0) / np.float32(3.0))
DEV_FACTORS = [0.0, -0.0, float("inf"), float("nan"), THIRD, -0.25, 1.0, -1.5]
SEEDS = (0x0123456789ABCDEF, 2**64 - 1)
_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _words(ft, n, salt):
    """archive words: N(0,1) rounded to ft, with the words of cast_ref.EDGE_BITS mixed in"""
    key = ("w", ft, n, salt)
    if key not in _cache:
        rng = np.random.default_rng(1000 * salt + 10 * n + ft)
        w = R.cast_ref(rng.standard_normal(n).astype(np.float32).view(np.uint32), ft)
        edges = R.cast_ref(R.EDGE_BITS, ft)
        k = min(n // 3, len(edges))
        if k:
            w[rng.choice(n, k, replace=False)] = edges[rng.choice(len(edges), k, replace=False)]
        _cache[key] = w
    return _cache[key]


def _tensor(ft, n, salt):
    """tensor words: N(0,1), with +-0, denormals, the largest finite value, infinities and NaNs mixed in"""
    key = ("t", ft, n, salt)
    if key not in _cache:
        rng = np.random.default_rng(7000 * salt + 10 * n + ft)
        t = R.cast_ref(rng.standard_normal(n).astype(np.float32).view(np.uint32), ft)
        big, inf = (0x7BFF, 0x7C00) if ft == S.FLOAT16 else (0x7F7F, 0x7F80)
        special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0200, 0x007F, big, big | 0x8000, inf, inf | 0x8000, inf | 1, 0xFFFF, 0x7FFF],
                           dtype=np.uint16)
        k = min(n // 2, len(special))
        if k:
            t[rng.choice(n, k, replace=False)] = special[:k]
        _cache[key] = t
    return _cache[key]


def _rows(ft, sizes, prob_bits, salt=0):
    import dietgpu_amd as dg

    key = ("rows", ft, tuple(sizes), prob_bits, salt)
    if key not in _cache:
        ts = [torch.from_numpy(_words(ft, n, salt + i).view(np.int16)).to(_dev()).view(DTYPE[ft]) for i, n in enumerate(sizes)]
        _cache[key] = dg.compress_data_simple(True, ts, False, prob_bits=prob_bits)
    return _cache[key]


class Flat:
    """the tensors of one call in one buffer: canaries, then tensor 0 at word offset `lead`, 3 canaries, tensor 1, ..."""

    def __init__(self, ft, caps, lead=1, fills=None):
        self.ft, self.caps = ft, list(caps)
        self.at, pos = [], 8 + lead
        for c in caps:
            self.at.append(pos)
            pos += c + 3
        host = np.full(pos + 8, CANARY, dtype=np.uint16)
        for k, c in enumerate(caps):
            host[self.at[k] : self.at[k] + c] = fills[k] if fills is not None else 0x3333
        self.before = host.copy()
        self.buf = torch.from_numpy(host.view(np.int16)).to(_dev())
        self.views = [self.buf[a : a + c].view(DTYPE[ft]) for a, c in zip(self.at, caps)]

    def words(self, k):
        return self.buf[self.at[k] : self.at[k] + self.caps[k]].cpu().numpy().view(np.uint16)

    def canaries_intact(self):
        got = self.buf.cpu().numpy().view(np.uint16)
        mask = np.ones(len(got), dtype=bool)
        for a, c in zip(self.at, self.caps):
            mask[a : a + c] = False
        return bool((got[mask] == CANARY).all())


def _same(got, want, ft, what):
    got, want = S.mask_nan_sign(got, ft), S.mask_nan_sign(want, ft)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} words differ, first at {i}: got {int(got[i]):04x} want {int(want[i]):04x}")


def _scale(mode, B, k0):
    """-> (the `scale` argument, the factor of every member)"""
    if mode == "devn":
        fs = [DEV_FACTORS[(k0 + k) % len(DEV_FACTORS)] for k in range(B)]
        return torch.tensor(fs, dtype=torch.float32, device=_dev()), fs
    if mode == "dev1":
        f = DEV_FACTORS[k0 % len(DEV_FACTORS)]
        return torch.tensor([f], dtype=torch.float32, device=_dev()), [f] * B
    if mode == "none":
        return None, [1.0] * B
    return THIRD, [THIRD] * B


def _seed(seed, on_device):
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=_dev()) if on_device else seed


def _update(ft, prob_bits, route, sizes, members, accumulate, mode, k0, seed, seed_on_device, first_member, lead, salt=0, what=""):
    """one call for `members` of the batch `sizes`: status, sizes, every word of every tensor and the canaries -> the Flat"""
    import dietgpu_amd as dg

    rows = _rows(ft, sizes, prob_bits, salt)
    B = len(members)
    scale, fs = _scale(mode, B, k0)
    flat = Flat(ft, [sizes[i] for i in members], lead, [_tensor(ft, sizes[i], salt + i) for i in members])
    status = torch.full((B,), 7, dtype=torch.uint8, device=_dev())
    out_sizes = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    dg.prefer_torch_ops(route == "torch_ops")
    try:
        used = dg.decompress_data_update([rows[i] for i in members], flat.views, _seed(seed, seed_on_device), scale, accumulate, first_member,
                                         status, out_sizes, prob_bits=prob_bits)
    finally:
        dg.prefer_torch_ops(True)
    what = f"ft={ft} P={prob_bits} {route} accumulate={accumulate} {mode}@{k0} seed={seed:#x} dev={seed_on_device} first={first_member} lead={lead} {what}"
    assert used == 0, what
    assert status.tolist() == [1] * B, what
    assert out_sizes.tolist() == [sizes[i] for i in members], what
    for k, i in enumerate(members):
        want = S.update_ref(_words(ft, sizes[i], salt + i), ft, fs[k], seed, first_member + k, _tensor(ft, sizes[i], salt + i) if accumulate else None)
        _same(flat.words(k), want, ft, f"{what}: member {k} ({sizes[i]} words, factor {fs[k]!r})")
    assert flat.canaries_intact(), what + ": canary words overwritten"
    return flat


# ------------------------------------------------------------------------------------------------------ 0. literals
def test_the_end_to_end_literals_of_the_contract():
    import dietgpu_amd as dg

    for ft, t, w, f, _, qs in S.END_TO_END:
        n = len(qs)
        src = torch.from_numpy(np.full(n, w, dtype=np.uint16).view(np.int16)).to(_dev()).view(DTYPE[ft])
        (row,) = dg.compress_data_simple(True, [src], False)
        out = torch.from_numpy(np.full(n, t, dtype=np.uint16).view(np.int16)).to(_dev())
        status = torch.zeros(1, dtype=torch.uint8, device=_dev())
        dg.decompress_data_update([row], [out.view(DTYPE[ft])], 0, f, True, 0, status, None)
        assert status.tolist() == [1]
        assert out.cpu().numpy().view(np.uint16).tolist() == qs, ft


# ---------------------------------------------------------------------------------------------------- 1. 4-block tiles
@pytest.mark.parametrize("prob_bits,route", ROUTES)
@pytest.mark.parametrize("ft", FTS)
def test_small_members_on_four_block_tiles(ft, prob_bits, route):
    """every way to pass the factor and the seed, store and add, tensors at word offsets 0, 1 and 7"""
    everything = list(range(len(SMALL)))
    n = 0
    for accumulate in (True, False):
        for mode in ("host", "dev1", "devn", "none"):
            for on_device in (False, True):
                _update(ft, prob_bits, route, SMALL, everything, accumulate, mode, n, SEEDS[n % 2], on_device, 0, (0, 1, 7)[n % 3])
                n += 1
    for k0 in range(len(DEV_FACTORS)):  # every device factor on every member
        _update(ft, prob_bits, route, SMALL, everything, True, "dev1", k0, 5, False, 0, 1)


# --------------------------------------------------------------------------------------------------- 2. 16-block tiles
@pytest.mark.parametrize("prob_bits,route", ROUTES)
@pytest.mark.parametrize("ft", FTS)
def test_large_members_on_sixteen_block_tiles_and_the_short_member_alone(ft, prob_bits, route):
    everything = list(range(len(LARGE)))
    for n, (accumulate, mode, on_device) in enumerate([(True, "devn", True), (False, "host", False), (True, "dev1", False)]):
        k0 = 4 + n  # (devn: the short member takes a finite factor)
        flat = _update(ft, prob_bits, route, LARGE, everything, accumulate, mode, k0, SEEDS[n % 2], on_device, 0, (7, 0, 1)[n])
        # the 5-word member, alone on 4-block tiles with its factor and its member index: the same bits
        f2 = DEV_FACTORS[(k0 + 2) % len(DEV_FACTORS)] if mode == "devn" else None
        mode2, k2 = ("dev1", (k0 + 2) % len(DEV_FACTORS)) if f2 is not None else (mode, k0)
        alone = _update(ft, prob_bits, route, LARGE, [2], accumulate, mode2, k2, SEEDS[n % 2], on_device, 2, 0, what="short member alone")
        # (_update compared `alone` with member index first_member + 0 = 2 and tensor LARGE[2]: the reference of member 2)
        assert np.array_equal(S.mask_nan_sign(alone.words(0), ft), S.mask_nan_sign(flat.words(2), ft))


# ------------------------------------------------------------------------------------------------- 3. first_member
@pytest.mark.parametrize("ft", FTS)
def test_first_member_j_with_one_member_is_member_j_of_the_whole_call(ft):
    sizes = [4097, 31, 3 * 4096 + 5, 1]
    whole = _update(ft, 10, "torch_ops", sizes, [0, 1, 2, 3], True, "host", 0, 77, False, 0, 1)
    shifted = _update(ft, 10, "torch_ops", sizes, [0, 1, 2, 3], True, "host", 0, 77, True, 65531, 1)
    assert not np.array_equal(whole.words(0), shifted.words(0))
    for j in range(4):
        flat = Flat(ft, [sizes[j]], 0, [_tensor(ft, sizes[j], j)])
        import dietgpu_amd as dg

        dg.decompress_data_update([_rows(ft, sizes, 10)[j]], flat.views, 77, THIRD, True, j)
        assert np.array_equal(S.mask_nan_sign(flat.words(0), ft), S.mask_nan_sign(whole.words(j), ft)), (ft, j)


# -------------------------------------------------------------------------------- 4. capacity larger than the element
@pytest.mark.parametrize("ft", FTS)
def test_a_capacity_larger_than_the_element_leaves_the_tail_untouched(ft):
    import dietgpu_amd as dg

    sizes = [4097, 31, 70000]
    rows = _rows(ft, sizes, 10)
    for caps in ([4097 + 9, 4096 * 5, 70000 + 4096 * 17], [4096 * 20, 32, 70001]):
        for accumulate in (True, False):
            fills = [np.concatenate([_tensor(ft, n, i), np.full(c - n, 0x1234, np.uint16)]) for i, (n, c) in enumerate(zip(sizes, caps))]
            flat = Flat(ft, caps, 7, fills)
            status = torch.zeros(3, dtype=torch.uint8, device=_dev())
            out_sizes = torch.zeros(3, dtype=torch.int32, device=_dev())
            dg.decompress_data_update(rows, flat.views, 9, -0.25, accumulate, 3, status, out_sizes)
            assert status.tolist() == [1, 1, 1] and out_sizes.tolist() == sizes
            for i, n in enumerate(sizes):
                got = flat.words(i)
                want = S.update_ref(_words(ft, n, i), ft, -0.25, 9, 3 + i, _tensor(ft, n, i) if accumulate else None)
                _same(got[:n], want, ft, f"ft={ft} caps={caps} accumulate={accumulate} member {i}")
                assert (got[n:] == 0x1234).all(), (ft, caps, i)
            assert flat.canaries_intact()


# --------------------------------------------------------------------------------------------------- 5. failing members
@pytest.mark.parametrize("sizes", [[4097, 3 * 4096 + 5, 3 * 4096 + 5, 31], [70000, 16 * 4096 + 4097, 70000, 5]])
@pytest.mark.parametrize("ft", FTS)
def test_a_truncated_archive_and_one_of_the_other_type_fail_alone_and_keep_their_tensors(ft, sizes):
    import dietgpu_amd as dg

    other = S.BFLOAT16 if ft == S.FLOAT16 else S.FLOAT16
    rows = list(_rows(ft, sizes, 10))
    rows[1] = rows[1][: rows[1].numel() - 64].clone()      # truncated: the archive claims more bytes than there are
    rows[2] = _rows(other, sizes, 10)[2]                   # an archive of the other float type
    for accumulate in (True, False):
        flat = Flat(ft, sizes, 1, [_tensor(ft, n, i) for i, n in enumerate(sizes)])
        status = torch.full((4,), 7, dtype=torch.uint8, device=_dev())
        dg.decompress_data_update(rows, flat.views, SEEDS[0], torch.tensor([THIRD], device=_dev()), accumulate, 0, status, None)
        assert status.tolist() == [1, 0, 0, 1], (ft, accumulate)
        for i in (1, 2):
            assert np.array_equal(flat.words(i), _tensor(ft, sizes[i], i)), f"ft={ft} accumulate={accumulate}: failing member {i} was written"
        for i in (0, 3):
            want = S.update_ref(_words(ft, sizes[i], i), ft, THIRD, SEEDS[0], i, _tensor(ft, sizes[i], i) if accumulate else None)
            _same(flat.words(i), want, ft, f"ft={ft} accumulate={accumulate}: neighbour {i}")
        assert flat.canaries_intact()


# ---------------------------------------------------------------------------------------------------------- 6. capture
def test_a_captured_call_follows_the_seed_in_device_memory():
    """one capture with seed_dev: replay, increment the seed on the device, replay -- the reference for S and S + 1"""
    import dietgpu_amd as dg

    ft, sizes, seed0 = S.BFLOAT16, [4097, 70000], 0x00000000FFFFFFFF
    rows = _rows(ft, sizes, 10)
    flat = Flat(ft, sizes, 1, [_tensor(ft, n, i) for i, n in enumerate(sizes)])
    start = flat.buf.clone()
    status = torch.zeros(2, dtype=torch.uint8, device=_dev())
    seed = torch.tensor([seed0], dtype=torch.int64, device=_dev())
    scale = torch.tensor([-0.25], dtype=torch.float32, device=_dev())

    def call():
        dg.decompress_data_update(rows, flat.views, seed, scale, True, 0, status, None)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()  # makes the parameter block resident
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call()
    torch.cuda.synchronize()
    try:
        for step in (0, 1):
            flat.buf.copy_(start)
            status.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert status.tolist() == [1, 1]
            for i, n in enumerate(sizes):
                want = S.update_ref(_words(ft, n, i), ft, -0.25, seed0 + step, i, _tensor(ft, n, i))
                _same(flat.words(i), want, ft, f"replay {step}, member {i}")
            assert flat.canaries_intact()
            seed.add_(1)
    finally:
        del graph
        dg.lib().dgpu_release_graph_state()

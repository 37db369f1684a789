"""Decode-reduce, the parts that need no GPU: the expected-value builder of the GPU tests, the premise of their order
test, the argument checks of the C ABI entry point (code 1 and a message that names the fault, before anything touches
a device) and of the Python layer, and compressed_reduce_scatter's use of a codec that has decompress_reduce."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import accum_cases as C
import reduce_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 5008  # per shard


def test_reduce_entry_point_is_exported_and_bound():
    import dietgpu_amd
    from dietgpu_amd import distributed

    name = "dgpu_float_decode_reduce"
    raw = ctypes.CDLL(dietgpu_amd.build.LIB_PATH)
    L = dietgpu_amd.lib()
    assert name in dietgpu_amd.EXPORTED_SYMBOLS
    assert hasattr(raw, name)
    assert getattr(L, name).argtypes is not None and getattr(L, name).restype is ctypes.c_int
    assert L.dgpu_abi_version() == 8  # an added entry point does not move the version
    assert callable(dietgpu_amd.decompress_data_reduce)
    assert callable(distributed.GpuFloatCodec.decompress_reduce)


def test_expected_value_builder_sums_in_source_order():
    a = np.array([1.0, 2.0 ** 24, -3.5], np.float32)
    xs = [np.array([2.0 ** 24, 1.0, 1.25], np.float32), np.array([-(2.0 ** 24), 1.0, 0.5], np.float32)]
    with_acc = R.reduce_expected(a, xs, True)
    assert C.bits(with_acc).tolist() == C.bits(C.add(C.add(a, xs[0]), xs[1])).tolist()
    assert with_acc.tolist() == [0.0, 2.0 ** 24, -1.75]  # (1 + 2^24) rounds to 2^24; (2^24 + 1) + 1 stays 2^24
    without = R.reduce_expected(a, xs, False)  # the accumulator is not an operand
    assert C.bits(without).tolist() == C.bits(C.add(xs[0], xs[1])).tolist()
    assert without.tolist() == [0.0, 2.0, 1.75]
    # one source, no accumulator: its bits as they are (-0.0 stays -0.0: nothing was added to it)
    z = np.array([-0.0], np.float32)
    assert C.bits(R.reduce_expected(None, [z], False)).tolist() == [0x80000000]
    # the other order is another value
    assert R.reduce_expected(a, xs[::-1], True).tolist() != with_acc.tolist()


@pytest.mark.parametrize("ft", C.FTS)
def test_order_premise(ft):
    hi, lo, tiny = R.ORDER_VALUES
    wides = {v: C.widen(ft, R.constant_words(ft, v, 4)) for v in R.ORDER_VALUES}
    for v, w in wides.items():
        assert (w == np.float32(v)).all()  # exact in this type
    assert (R.reduce_expected(None, [wides[hi], wides[lo], wides[tiny]], False) == np.float32(2.0 ** -10)).all()
    assert (R.reduce_expected(None, [wides[tiny], wides[hi], wides[lo]], False) == np.float32(0.0)).all()


def test_rotated_sources_keep_the_word_count_and_change_the_blocks():
    src = R.Sources(C.Case("reduce host", C.FTS[1], [("ccrr", 77, "c", 5), ("c", 0, "c", 6)]), 3)
    for s in range(3):
        assert [w.size for w in src.words[s]] == src.sizes
    assert R.rotated("ccrr", 1) == "crrc" and R.rotated("ccrr", 6) == "rrcc" and R.rotated("", 3) == ""
    assert not np.array_equal(src.words[0][0], src.words[1][0])
    # block 1 of element 0: compressible in source 0, random in source 2
    counts = [C.float_block_words(src.ft, src.archives(10)[s][0], src.sizes[0]) for s in range(3)]
    assert counts[0][1] <= C.STAGE_WORDS < counts[2][1]


def test_reduce_argument_errors_of_the_c_abi_need_no_device():
    import dietgpu_amd

    L = dietgpu_amd.lib()
    f = L.dgpu_float_decode_reduce
    A = 0x10000
    two = (ctypes.c_uint32 * 2)(16, 16)
    one = (ctypes.c_uint32 * 1)(16)
    src = (ctypes.c_void_p * 2)(A, A)  # (sources may alias each other)
    acc = (ctypes.c_void_p * 1)(2 * A)

    def fails(message, *args):
        assert f(None, 0, None, *args, None, None, None) == 1
        assert message in L.dgpu_last_error().decode()

    #      floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, out, outCapacity
    fails("probBits must be 9, 10 or 11", 2, 12, 1, 1, 2, src, two, acc, one)
    fails("probBits must be 9, 10 or 11", 2, 8, 1, 1, 2, src, two, acc, one)
    fails("floatType", 0, 10, 1, 1, 2, src, two, acc, one)
    fails("floatType", 4, 10, 1, 1, 2, src, two, acc, one)
    fails("accumulate must be 0 or 1", 2, 10, 2, 1, 2, src, two, acc, one)
    fails("accumulate must be 0 or 1", 2, 10, -1, 1, 2, src, two, acc, one)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 0, src, two, acc, one)
    fails("numSources must be between 1 and 64", 2, 10, 1, 1, 65, src, two, acc, one)
    # (the products are checked before the arrays are read)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 32768, 2, src, two, acc, one)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 1024, 64, src, two, acc, one)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 0xFFFFFFFF, 64, src, two, acc, one)
    fails("numInBatch * numSources must be <= 65535", 2, 10, 1, 65536, 1, src, two, acc, one)
    for missing in range(4):
        arrays = [src, two, acc, one]
        arrays[missing] = None
        fails("null array", 2, 10, 1, 1, 2, *arrays)
    fails("16-byte aligned", 2, 10, 1, 1, 2, (ctypes.c_void_p * 2)(A, A + 8), two, acc, one)  # the SECOND source
    fails("16-byte aligned", 2, 10, 1, 1, 2, (ctypes.c_void_p * 2)(A + 4, A), two, acc, one)
    fails("4-byte aligned", 2, 10, 1, 1, 2, src, two, (ctypes.c_void_p * 1)(2 * A + 2), one)
    fails("outCapacity", 2, 10, 1, 1, 2, src, two, acc, (ctypes.c_uint32 * 1)(0xFFFFF001))
    # numSources == 1 is decode-accumulate, with its checks
    fails("null array", 2, 10, 1, 1, 1, None, one, acc, one)
    fails("4-byte aligned", 2, 10, 1, 1, 1, (ctypes.c_void_p * 1)(A), one, (ctypes.c_void_p * 1)(2 * A + 2), one)
    for sources in (1, 2, 64):  # an empty batch is fine and uses nothing
        used = ctypes.c_size_t(77)
        assert f(None, 0, ctypes.byref(used), 2, 10, 1, 0, sources, None, None, None, None, None, None, None) == 0
        assert used.value == 0


@pytest.mark.parametrize("torch_ops", [True, False])
def test_reduce_rejects_bad_tensors_without_a_gpu(torch_ops):
    import dietgpu_amd as dg

    dg.prefer_torch_ops(torch_ops)
    try:
        arch = torch.zeros(1024, dtype=torch.uint8)  # CPU tensors
        acc = torch.zeros(4096, dtype=torch.float32)
        with pytest.raises(RuntimeError):
            dg.decompress_data_reduce([[arch, arch]], [acc])
        with pytest.raises(RuntimeError):
            dg.decompress_data_reduce([[arch, arch]], [acc], accumulate=True, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # ragged source lists
            dg.decompress_data_reduce([[arch, arch], [arch]], [acc, acc.clone()], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # empty lists
            dg.decompress_data_reduce([], [])
        with pytest.raises(RuntimeError):
            dg.decompress_data_reduce([[]], [acc], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):  # one list of sources per accumulator
            dg.decompress_data_reduce([[arch, arch], [arch, arch]], [acc], dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            dg.decompress_data_reduce([[arch] * 65], [acc], dtype=torch.bfloat16)
        for bad in (torch.bfloat16, torch.float16, torch.float64, torch.int32):  # accumulators that are not float32
            with pytest.raises(RuntimeError):
                dg.decompress_data_reduce([[arch, arch]], [acc.to(bad)], dtype=torch.bfloat16)
    finally:
        dg.prefer_torch_ops(True)


# ------------------------------------------------------------------------------------------- reduce-scatter over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tensor_of(rank, world):
    g = torch.Generator().manual_seed(700 + rank)
    return torch.randn(world * WORDS, generator=g).to(torch.bfloat16)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    import oracle as O
    from dietgpu_amd import distributed as D
    from test_accumulate_gloo import _OracleAccumCodec

    class OracleReduceCodec(_OracleAccumCodec):
        """... with decompress_reduce: the oracle decode of every row, summed in the order given"""

        calls = []
        loop_calls = 0

        def decompress_accumulate(self, rows, accs, accumulate):
            self.loop_calls += 1
            return super().decompress_accumulate(rows, accs, accumulate)

        def decompress_reduce(self, rows_per_acc, accs, accumulate):
            self.calls.append(([len(rows) for rows in rows_per_acc], len(accs), bool(accumulate)))
            for rows, acc in zip(rows_per_acc, accs):
                for k, r in enumerate(rows):
                    _OracleAccumCodec.decompress_accumulate(self, [r], [acc], accumulate or k > 0)
            return torch.ones((len(accs),), dtype=torch.uint8)

    D.init(backend="gloo")
    codec = OracleReduceCodec(O)
    shard, stats = D.compressed_reduce_scatter(_tensor_of(rank, world), codec=codec)
    dist.barrier()
    q.put((rank, shard.numpy().view(np.uint32).copy(), codec.calls, codec.loop_calls))
    dist.destroy_process_group()


def test_compressed_reduce_scatter_makes_one_reduce_call_world2():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    inputs = [_tensor_of(r, world).view(world, WORDS) for r in range(world)]
    for rank, bits, calls, loop_calls in res:
        assert calls == [([world], 1, False)], f"rank {rank}: exactly one reduce call with `world` rows, accumulate off"
        assert loop_calls == 0, f"rank {rank}: the per-source loop ran beside the reduce call"
        want = R.reduce_expected(None, [inputs[r][rank].to(torch.float32).numpy() for r in range(world)], False)
        assert np.array_equal(bits, C.bits(want)), f"rank {rank}: the reduced shard is not the rank-order float32 sum"

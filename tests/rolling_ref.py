"""Reference of the rolling-table compress call (include/dietgpu_amd.h, dgpu_float_rolling_compress), built from the
CPU oracle: what the archive of `words` is when its table comes from OTHER counts.  Used by tests/test_rolling_host.py
(which pins the helper itself against the oracle's float archive) and tests/test_gpu_rolling*.py."""
import numpy as np

import oracle as O

FLOAT16, BFLOAT16 = O.FLOAT16, O.BFLOAT16


def smooth(counts, n):
    """c'[s] = min(max(counts[s], 1), n): every symbol gets a probability >= 1, whatever the buffer held"""
    c = np.ascontiguousarray(counts).astype(np.uint32).astype(np.uint64)
    return np.minimum(np.maximum(c, 1), max(int(n), 1)).astype(np.uint32)


def exponent_bytes(ft, words):
    """the byte of each 16-bit word the format entropy-codes: w >> 8 (float16), bits 14..7 (bfloat16)"""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    return ((w >> 8) if ft == FLOAT16 else ((w >> 7) & 0xFF)).astype(np.uint8)


def exponent_hist(ft, words):
    return np.bincount(exponent_bytes(ft, words), minlength=256).astype(np.uint32)


def sizes_blockwise(ft, words, prob_bits, counts):
    """Full size in bytes of expected_archive(...), from one oracle.encode_block per 4096-word block (each block's
    word count rounded up to 8): known before oracle.ans_encode is trusted with its output buffer."""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    n = w.size
    table = O.normalize(np.ascontiguousarray(counts, np.uint32), n, prob_bits)
    exps = exponent_bytes(ft, w)
    nb = (n + 4095) // 4096
    total_words = 0
    for b in range(nb):
        got, _ = O.encode_block(exps[b * 4096:(b + 1) * 4096], prob_bits, table)
        total_words += (got.size + 7) // 8 * 8
    return 16 + O.float_uncomp_data_size(ft, n) + O.ans_compressed_overhead(nb) + 2 * total_words


def expected_archive(ft, words, prob_bits, counts):
    """The float archive of `words` coded with the table the normalisation yields for `counts` against a total of
    len(words) -- the rolling call's archive for counts = smooth(last call's counts, len(words)): header and
    non-compressed plane of the oracle's own float archive, then the oracle's ANS archive of the exponent bytes under
    those counts.  With the data's own histogram (not smoothed) it is the oracle's float archive."""
    w = np.ascontiguousarray(words, dtype=np.uint16)
    n = w.size
    head = 16 + O.float_uncomp_data_size(ft, n)
    plain = O.float_compress(ft, w, prob_bits)
    ans = O.ans_encode(exponent_bytes(ft, w), prob_bits, counts=np.ascontiguousarray(counts, np.uint32))
    return np.concatenate([plain[:head], ans])

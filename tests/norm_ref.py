"""Expected values of the norm outputs of the reduce calls (out_sumsq / out_nonfinite), shared by the tests that check
them.  The expected squared norm is math.fsum of the float64 squares of the finite expected words -- a float32 squared is
exact in float64 and fsum is exact, so the whole bound of n * 2**-52 (twice the (n - 1) * 2**-53 of any summation order
of n non-negative doubles) is left to the code under test.  The expected non-finite count is a numpy count.

This module touches no GPU state: it is imported by tests that run without one."""
import math

import numpy as np
import torch


def stats(words):
    """float32 words (numpy) -> (exact squared norm of the finite ones, rounded once; count of the others; words)"""
    w = np.ascontiguousarray(words, dtype=np.float32)
    finite = np.isfinite(w)
    sq = w[finite].astype(np.float64)
    return math.fsum((sq * sq).tolist()), int((~finite).sum()), int(w.size)


def rounded(words, dtype):
    """float32 words rounded to `dtype` (round to nearest even, torch on the CPU) and widened again: the words of the
    archive a cast of them holds"""
    with np.errstate(invalid="ignore"):
        t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.float32).copy())
    return t.to(dtype).to(torch.float32).numpy()


def within(got, want, n):
    """|got - want| <= n * 2**-52 * want"""
    return math.isfinite(got) and abs(got - want) <= n * 2.0 ** -52 * want


def check(got_sumsq, got_nonfinite, words, what):
    """one member: prints the figures, then asserts the exact count and the bound"""
    want, bad, n = stats(words)
    err = abs(got_sumsq - want) / want if want else abs(got_sumsq)
    print(f"{what}: n={n} nonfinite {got_nonfinite} / {bad}, sumsq {got_sumsq!r} / {want!r}, relative error {err:.3e} (bound {n * 2.0 ** -52:.3e})")
    assert got_nonfinite == bad, f"{what}: nonfinite {got_nonfinite}, expected {bad}"
    assert within(got_sumsq, want, n), f"{what}: sumsq {got_sumsq!r}, expected {want!r} within {n} * 2**-52"

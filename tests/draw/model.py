"""The draws of pc_hip_select_draw (include/polycap-hip.h) in Python integers: the yardstick of tests/test_draw_cpu.py and
tests/test_gpu_draw.py.  Nothing here is shared with the library: thresholds are one big-integer expression, positions a search in a
cumulative sum of Python integers (or of uint64, which is exact as long as T < 2^64)."""
import bisect

import numpy as np


def quantise(w):
    """q(w) = round_half_even(w * 2^32) of the spot maps as uint64; what is not above zero (NaN included) counts 0"""
    v = np.asarray(w, dtype=np.float64) * 4294967296.0
    with np.errstate(invalid="ignore"):
        return np.where(v > 0., np.rint(v), 0.).astype(np.uint64)


def threshold(k, phase, T, N):
    """t_k = floor((k * 2^32 + r) * T / (N * 2^32))"""
    return ((int(k) << 32) + int(phase)) * int(T) // (int(N) << 32)


def below(c, phase, T, N):
    """K(c) = #{k in [0, N) : t_k < c}, in closed form: t_k < c  <=>  (k 2^32 + r) T < c N 2^32  <=>  k < (ceil(c N 2^32 / T) - r) / 2^32"""
    c, phase, T, N = int(c), int(phase), int(T), int(N)
    if c <= 0:
        return 0
    a = -((-(c * N << 32)) // T) - phase          # k * 2^32 < a
    if a <= 0:
        return 0
    return min(N, -((-a) >> 32))


def cumulative(V):
    """C_i as a list of Python integers"""
    out, c = [], 0
    for v in V:
        c += int(v)
        out.append(c)
    return out


def positions(V, N, phase, first=0, count=None, base=0, total=None):
    """pos_k for k in [first, first + count) that land on these entries, as (k, position) pairs; V are the entries' values, base the
    sum of the values before them and total the T of all entries (this list's own sum by default).  With base and total of its own the
    list is one member of several."""
    C = cumulative(V)
    T = (C[-1] if C else 0) if total is None else int(total)
    count = N - first if count is None else count
    out = []
    for k in range(first, first + count):
        t = threshold(k, phase, T, N) - base
        if 0 <= t < (C[-1] if C else 0):
            out.append((k, bisect.bisect_right(C, t)))
    return out


def draw(V, N, phase, first=0, count=None):
    """positions int64 [count] of the draws [first, first + count) on the entries V (a uint64 array, its sum below 2^64), and T.  The
    same as positions(), vectorised: thresholds as Python integers, the search by numpy on the exact uint64 cumulative sum."""
    V = np.asarray(V, dtype=np.uint64)
    T = sum(int(v) for v in V[V > 0])
    assert 0 < T < 1 << 64
    C = np.cumsum(V, dtype=np.uint64)
    count = N - first if count is None else count
    t = np.array([threshold(k, phase, T, N) for k in range(first, first + count)], dtype=np.uint64)
    return np.searchsorted(C, t, side="right").astype(np.int64), T

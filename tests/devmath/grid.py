"""TEST-ONLY: the inputs of the devmath tests (tests/test_devmath_cpu.py, tests/test_gpu_devmath.py) and their exact values.

Energies 1 ... 100 keV on the decks' glass and on tests.common.synthetic_constants, one energy without absorption (amu = 0:
n2_im = 0, zi2 at its 2^-200 floor); cos theta from 1e-16 to 1 at 64 points per decade, and densely around every critical
angle sqrt(d2), including the adjacent doubles where c*c - d2 changes sign; polarisation fractions 1, 0, 1/2 and random."""
import functools
import math
import os

import numpy as np

from tests.devmath import exact, pyprobe

ENERGIES = (1.0, 1.5, 3.0, 10.0, 17.4, 30.0, 60.0, 100.0)
SIG_ROUGH = (0.0, 5.0, 1.0e4)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(glass, sig_rough=0.0):
    """'deck': the xos1 deck's glass at ENERGIES; 'synthetic': tests.common.synthetic_constants at ENERGIES plus 10 keV with
    amu = 0 (last energy)."""
    import polycap_amd
    from tests.common import synthetic_constants
    deck = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")
    if glass == "deck":
        return polycap_amd.problem_from_inp(deck, energies=list(ENERGIES), sig_rough=sig_rough)
    p = polycap_amd.problem_from_inp(deck, energies=[10.0], sig_rough=sig_rough)
    E = np.array(ENERGIES + (10.0,))
    amu, scatf = synthetic_constants(E)
    amu[-1] = 0.0
    return polycap_amd.Problem(p.z, p.cap, p.ext, sig_rough, p.n_cap, p.density, E, amu, scatf, *p.source)


def log_grid(lo_decade, hi_decade, per_decade=64):
    k = np.arange((hi_decade - lo_decade) * per_decade + 1)
    return 10.0 ** (lo_decade + k / per_decade)


def critical_points(d2):
    """cosines around the critical angle sqrt(d2): relative offsets 1e-1 ... 1e-12 on both sides and the three doubles on
    either side of the one where c*c - d2 (as FORM 3 forms it) changes sign"""
    c0 = math.sqrt(d2)
    pts = [c0 * (1 + s * 10.0 ** -k) for k in range(1, 13) for s in (-1, 1)]
    pts += list(c0 * (1 + np.linspace(-0.05, 0.05, 41)))
    lo, hi = c0 * (1 - 1e-12), c0 * (1 + 1e-12)
    while np.nextafter(lo, 2.0) < hi:                # smallest double whose square (rounded) is >= d2
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if mid * mid >= d2:
            hi = mid
        else:
            lo = mid
    x = hi
    for _ in range(3):
        x = np.nextafter(x, 0.0)
    for _ in range(7):
        pts.append(x)
        x = np.nextafter(x, 2.0)
    return np.array([p for p in pts if 0.0 < p <= 1.0])


@functools.lru_cache(maxsize=None)
def fresnel_points(glass):
    """(problem, ec, e, c, st2, exact FORM 3 (Rs, Rp, cs, cp), exact FORM 0/1 (Rs, Rp, cs, cp), physical (Rs, Rp)) over every
    energy of `glass` and the cosine grid; st2 = fma(-c, c, 1) as pc_reflect_geom forms it."""
    p = problem(glass)
    ec = pyprobe.energy_consts(p)
    e, c = [], []
    base = log_grid(-16, 0)
    for k in range(p.n_energies):
        ck = np.unique(np.concatenate([base, critical_points(ec["d2"][k])]))
        e.append(np.full(ck.size, k, dtype=np.int32))
        c.append(ck)
    e, c = np.concatenate(e), np.concatenate(c)
    st2 = np.array([exact.fma_neg_sq_one(x) for x in c])
    f3 = exact.fresnel3_table(ec, e, c)
    f01 = exact.fresnel01_table(ec, e, c, st2)
    db = [exact.delta_beta(E, p.density, s, a) for E, s, a in zip(p.energies, p.scatf, p.amu)]
    ph = np.array([exact.physical(*db[k], ci) for k, ci in zip(e, c)]).T
    return p, ec, e, c, st2, f3, f01, ph


def fractions(n, seed=5):
    """(fs, fp) rows: 1/0, 0/1, 1/2, random fs with fp = 1 - fs, cycling over n points"""
    rng = np.random.default_rng(seed)
    r = rng.random(n)
    kind = np.arange(n) % 4
    fs = np.where(kind == 0, 1.0, np.where(kind == 1, 0.0, np.where(kind == 2, 0.5, r)))
    return fs, 1.0 - fs


def geometry(n, seed=7):
    """unnormalised (es2, ep2, sd2) for FORMs 0/1/3s: sd2 in [1e-3, 1], es2 a fraction of it (1, 0, 1/2, random), ep2 = sd2 - es2
    as pc_reflect_geom forms it"""
    rng = np.random.default_rng(seed)
    sd2 = 10.0 ** rng.uniform(-3, 0, n)
    fs, _ = fractions(n, seed)
    es2 = fs * sd2
    return es2, sd2 - es2, sd2

"""The sweep certificate (pc_sweep_certify, polycap_amd/csrc/hip/pc_sweep_cert.h) against mpmath, on the host.

What the logging kernel is told about a run's energies: ct_tame, the cosine above which no reflectivity comes within 1e-11 of 1, and
the one or two proxy energies that reflect best at 3 and at 30 mrad.  The function reads nothing but the per-energy constants, so the
host compile of the device headers (tests/emul) returns what a GPU context computes; tests/test_gpu_devmath.py checks that bit for
bit.  Here 1 - R_s and 1 - R_p are evaluated from the same constants with the formulas of the function's comment,
    1 - R_s = 4 c Re(g) / |c + g|^2,   1 - R_p = 4 c Re(conj(g) n^2) / |g + n^2 c|^2,   g = sqrt(n^2 - 1 + c^2),
in 40 digits."""
import os

import mpmath as mp
import numpy as np
import pytest

from tests.devmath import pyprobe
from tests.emul import pyemul

DPS = 40
FLOOR = 4e-13            # below the scanned 13 decades nothing is certified
with mp.workdps(DPS):
    LO, HI = mp.mpf("1e-11"), mp.mpf(1)
PROXY_ANGLES = ("3e-3", "3e-2")


def deck291():
    import polycap_amd
    from tests.conftest import EXAMPLE
    p = polycap_amd.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"))
    assert p.n_energies == 291
    return p


def grid12():
    import polycap_amd
    from tests.conftest import EXAMPLE
    return polycap_amd.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"), energies=np.linspace(5.0, 25.0, 12))


PROBLEMS = {"deck291": deck291, "grid12": grid12}


def one_minus_r(ec, e, c):
    """(1 - R_s, 1 - R_p) of energy e at cos theta = c (mpf), from the constants d2 = 1 - Re n^2, n2_re, n2_im"""
    d2, n2 = ec["mp"][e]
    g = mp.sqrt(mp.mpc(c*c - d2, n2.imag))
    s = 4*c*g.real / abs(c + g)**2
    p = 4*c*(mp.conj(g)*n2).real / abs(g + n2*c)**2
    return s, p


def in_range(ec, e, c):
    s, p = one_minus_r(ec, e, c)
    return LO <= s <= HI and LO <= p <= HI


def grid_point(k):
    return mp.power(10, -mp.mpf(k)/64)


@pytest.fixture(scope="module", params=sorted(PROBLEMS))
def case(request):
    p = PROBLEMS[request.param]()
    ec = pyprobe.energy_consts(p)
    ec["mp"] = [(mp.mpf(float(d2)), mp.mpc(mp.mpf(float(re)), mp.mpf(float(im)))) for d2, re, im in zip(ec["d2"], ec["n2_re"], ec["n2_im"])]
    return request.param, p, ec, pyemul.sweep_cert(p)


def test_every_grid_point_from_ct_tame_up_is_tame(case):
    name, p, ec, cert = case
    ct = cert["ct_tame"]
    assert FLOOR <= ct < 1.0, ct
    with mp.workdps(DPS):
        pts = [(k, grid_point(k)) for k in range(13*64 + 1)]
        ks = [(k, c) for k, c in pts if c >= mp.mpf(ct)]
        assert ks and ks[0][0] == 0
        worst = (mp.inf, mp.inf)
        for e in range(p.n_energies):
            for k, c in ks:
                s, q = one_minus_r(ec, e, c)
                assert LO <= s <= HI and LO <= q <= HI, (name, e, k, s, q)
                worst = min(worst, (min(s, q), k))
    print("%s: ct_tame %.6e, %d grid points x %d energies in range; smallest 1 - R %.3e at k = %d" % (
        name, ct, len(ks), p.n_energies, float(worst[0]), worst[1]))


def test_ct_tame_is_tight(case):
    """ct_tame is 4 x the largest grid point at which some energy leaves [1e-11, 1]: at that point one does"""
    name, p, ec, cert = case
    ct = cert["ct_tame"]
    if ct == FLOOR:          # nothing failed in the scanned range: there is no such point
        return
    with mp.workdps(DPS):
        k = int(mp.nint(-64*mp.log10(mp.mpf(ct)/4)))
        c = grid_point(k)
        assert 0 <= k <= 13*64 and abs(mp.mpf(ct)/4/c - 1) < mp.mpf(2)**-50, (ct, k)      # ct_tame / 4 is that grid point, as a double
        out = [e for e in range(p.n_energies) if not in_range(ec, e, c)]
    print("%s: ct_tame / 4 = 10^(-%d/64): %d of %d energies out of range" % (name, k, len(out), p.n_energies))
    assert out, (name, ct, k)


def test_proxies_reflect_best_at_3_and_30_mrad(case):
    name, p, ec, cert = case
    best = []
    with mp.workdps(DPS):
        for at in PROXY_ANGLES:
            c = mp.mpf(at)
            r = []
            for e in range(p.n_energies):
                s, q = one_minus_r(ec, e, c)
                x = mp.mpf(float(ec["rough_c"][e]))*c
                r.append((1 - (s + q)/2)*mp.exp(-x*x))
            order = sorted(range(p.n_energies), key=lambda e: r[e], reverse=True)
            # no tie: the best energy leads by far more than extended precision resolves (2^-64)
            assert r[order[0]] - r[order[1]] > mp.mpf(2)**-50 * r[order[0]], (name, at, order[:2], r[order[0]], r[order[1]])
            best.append(order[0])
    print("%s: proxies %s (certificate %s)" % (name, best, cert["proxies"]))
    assert cert["n_proxy"] == (1 if best[0] == best[1] else 2)
    assert cert["proxies"] == [best[0], best[1] if best[1] != best[0] else -1]

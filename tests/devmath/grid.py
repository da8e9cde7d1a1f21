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


# ---------------------------------------------------------------------------------------------------------------------------
# The geometric half: rows for the SEGMENT op (pyprobe.SEG_COLS) and for the GEOM / BOUNCE ops (d, E, n).  One segment, one
# photon per element; seeded generators plus explicit edge points.  Every family has a name so that the tests can say which
# points lie, on purpose, on a branch.
KQ = ((2.0 * 7 - 3) * 0.86602540378443864676, -3 * 1.5)      # (kx, ky) of capillary (q, r) = (7, -3): |k| = 10.5
SEG_SLOPES = 10.0 ** np.linspace(-6, np.log10(3e-2), 10)
SEG_LENGTHS = (1e-4, 1e-2, 1.0)
SEG_RADII = (1e-4, 1e-3, 1e-2, 1e-1)
SEG_RATES = (0.0, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3, 1.5e-2, -1.5e-2)
SEG_OFFSETS = (0.0, 0.05, 1.0)


def _seg_row(L, R0, rr, off, theta, f, phi, tau, z0=0.7, back=None):
    """A ray that meets the wall of the cone (R0 at z0, rate rr, length L, axis `off` from the optic's axis and tilted) at the
    fraction f of the segment and azimuth phi, at the grazing slope theta against the wall and the tangential slope tau; P lies
    `back` (default: half the way to the opposite wall, at least 3e-5) before the hit on the ray."""
    kx, ky = KQ
    kn = math.hypot(kx, ky)
    zh0 = off / kn
    zh1 = zh0 * (1.0 - 2e-3 * L)
    z1 = z0 + L
    R1 = R0 + rr * L
    axs = np.array([kx, ky]) * (zh1 - zh0) / (z1 - z0)
    zh = z0 + f * L
    R = R0 + rr * f * L
    rad, tan = np.array([math.cos(phi), math.sin(phi)]), np.array([-math.sin(phi), math.cos(phi)])
    H = np.array([kx, ky]) * (zh0 + (zh1 - zh0) * f) + R * rad
    s = axs + (rr + theta) * rad + tau * tan
    d = np.array([s[0], s[1], 1.0])
    d /= np.sqrt(d @ d)
    if back is None:
        back = min(max(0.5 * R / theta, 3e-5), 10.0 * L)
    P = np.array([H[0], H[1], zh]) - np.array([s[0], s[1], 1.0]) * back
    return [z0, z1, R0, R1, zh0, zh1, kx, ky, P[0], P[1], P[2], d[0], d[1], d[2]]


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def _cyl(theta=1e-3, R=1e-3, Pz=0.2, z0=1.0, z1=2.0, y=0.0, x0=0.0):
    """a ray in the plane y = const of a straight cylinder on the optic's axis, moving towards +x at slope theta from (x0, y, Pz)"""
    d = np.array([theta, 0.0, 1.0])
    d /= np.sqrt(d @ d)
    return [z0, z1, R, R, 0.0, 0.0, KQ[0], KQ[1], x0, y, Pz, d[0], d[1], d[2]]


@functools.lru_cache(maxsize=None)
def segment_rows():
    """(rows [n, 14], family [n] of str).  See the issue's list: bulk (slopes x lengths x radii x cone rates x axis offsets), the
    dense run of rates across the series switch of the normal, tangent rays, rays parallel to the wall, roots at the seams, the
    1e-5 and 1e-10 guards, both roots valid, start on the wall, rejected inputs."""
    rows, fam = [], []

    def add(name, r):
        rows.append([float(v) for v in r])
        fam.append(name)

    rng = np.random.default_rng(2024)
    for rep in range(2):
        for theta in SEG_SLOPES:
            for L in SEG_LENGTHS:
                for R0 in SEG_RADII:
                    for rr in SEG_RATES:
                        if R0 + rr * L < 0.1 * R0:
                            continue
                        for off in SEG_OFFSETS:
                            add("bulk", _seg_row(L, R0, rr, off, theta, rng.uniform(0.05, 0.95), rng.uniform(0, 2 * np.pi),
                                                 rng.uniform(-1, 1) * theta))
    # |eps| of the normal = 1e-4 at |rr| ~ 1e-2: the series below, 1/sqrt above
    for rr in np.concatenate([np.linspace(0.8e-2, 1.2e-2, 41), -np.linspace(0.8e-2, 1.2e-2, 41)]):
        for off in (0.0, 0.05):
            add("switch", _seg_row(1e-2, 1e-2, rr, off, 1e-3, rng.uniform(0.05, 0.95), rng.uniform(0, 2 * np.pi), 0.0))
    # tangent rays: cylinder of radius R, ray in the plane y = m; discr / b^2 = (R^2 - m^2) / p0x^2.  With the ray 10 radii from
    # the axis at z0, one ulp of R moves the discriminant by a fiftieth of an ulp of b^2: R is searched for the double that puts
    # the exact discriminant (of the inputs as stored) nearest to 0, +-1 and +-64 ulp of b^2
    m, p0x, th = 0.9e-3, -9e-3, 1e-2
    base = _cyl(theta=th, R=m, Pz=0.0 - 1e-3, z0=0.0, z1=1.0, y=m, x0=p0x - th * 1e-3)

    def tangent_units(R):
        r = list(base); r[2] = r[3] = R
        e = exact.segment(r)
        return float(e["discr"] / np.spacing(float(e["b2"])))

    u0 = tangent_units(m)
    per_step = tangent_units(_ulps(m, 64)) - u0
    per_step /= 64.0
    for target in (0, 1, -1, 64, -64):
        k0 = int(round((target - u0) / per_step))
        best = min(range(k0 - 2, k0 + 3), key=lambda k: abs(tangent_units(_ulps(m, k)) - target))
        r = list(base); r[2] = r[3] = _ulps(m, best)
        add("tangent", r)
    for dec in range(-12, -2):
        for sg in (1, -1):
            r = list(base); r[2] = r[3] = math.sqrt(m * m + sg * 10.0 ** dec * p0x * p0x)
            add("tangent", r)
    # rays parallel to the wall: a = sx^2 - rr^2 scaled to 0, +-1 ulp of the slope (the finest step the direction's doubles allow:
    # 2 to 4 ulp of rr^2 in a), relative 1e-15 ... 1e-6 of rr^2
    for rr in (-1e-3, 1e-3):
        rels = [0.0] + [sg * 10.0 ** dec for dec in range(-15, -5) for sg in (1, -1)]
        for rel in rels:
            for k in ((0, 1, -1) if rel == 0.0 else (0,)):
                sx = _ulps(rr * math.sqrt(1.0 + rel), k)
                d = np.array([sx, 0.0, 1.0]); d /= np.sqrt(d @ d)
                add("parallel", [0.0, 1.0, 1e-2, 1e-2 + rr, 0.0, 0.0, KQ[0], KQ[1], -0.9e-2 if rr < 0 else 0.9e-2, 0.0, 0.0 - 1e-3 * 0, d[0], d[1], d[2]])
    # the families below place a root on a threshold: the exact root of the default cylinder is independent of z0 and z1
    c = _cyl()
    zr = float(exact.segment(c)["hz"])
    for k in (0, 1, -1, 8, -8):
        r = list(c); r[1] = _ulps(zr, k)
        add("seam_z1", r)
        r = list(c); r[0] = _ulps(zr, k); r[1] = r[0] + 1.0
        add("seam_z0", r)
    th = c[11] / c[13]
    for g in (0.0, 1, -1, 1e-12, -1e-12, 1e-8, -1e-8):
        Pz = _ulps(zr - 1e-5, int(g)) if abs(g) == 1 or g == 0.0 else zr - 1e-5 - g
        r = list(c); r[10] = Pz; r[8] = th * (Pz - 0.2)
        add("guard_1e-5", r)
    for g in (0.0, 1, -1, 1e-12, -1e-12, 1e-8, -1e-8):
        t = 1e-10 * c[13]
        z0 = _ulps(zr - t, int(g)) if abs(g) == 1 or g == 0.0 else zr - (1e-10 + g) * c[13]
        r = list(c); r[0] = z0; r[1] = z0 + 1.0
        add("guard_1e-10", r)
    # both roots inside the segment and beyond the last hit: P outside the wall
    for y in np.linspace(-0.9e-3, 0.9e-3, 10):
        add("both_roots", _cyl(theta=1e-2, R=1e-3, Pz=0.2, z0=0.3, z1=1.0, y=y, x0=-3e-3))
    # P on the wall: `last` is itself a root
    for phi in np.linspace(0.55 * np.pi, 1.45 * np.pi, 10):
        add("on_wall", _cyl(theta=1e-2, R=1e-3, Pz=0.2, z0=0.1, z1=1.0, y=1e-3 * math.sin(phi), x0=1e-3 * math.cos(phi)))
    # rejected inputs
    ok = _seg_row(1e-2, 1e-3, -1e-5, 0.05, 1e-3, 0.5, 1.0, 0.0)
    for s in (1.0, 0.5, 1e-3):
        r = list(ok); r[13] = -r[13] * s
        add("dz_negative", r)
    r = list(ok); r[13] = 0.0
    add("dz_zero", r)
    r = list(ok); r[13] = -0.0
    add("dz_zero", r)
    for j in range(14):
        r = list(ok); r[j] = float("nan")
        add("nan_" + pyprobe.SEG_COLS[j], r)
    return np.array(rows), np.array(fam)


def _perp(d, rng):
    """a unit vector perpendicular to d (mpf lists)"""
    import mpmath as mp
    r = [mp.mpf(float(v)) for v in rng.normal(size=3)]
    dd = exact._dot(d, d)
    k = exact._dot(r, d) / dd
    w = [r[i] - k * d[i] for i in range(3)]
    l = mp.sqrt(exact._dot(w, w))
    return [v / l for v in w]


def _den_row(d, alfa, beta, rng, u=None, scale_n=0.0, scale_d=0.0):
    """(d, E, n) with n at cos theta = alfa to the unit vector d (mpf list) and E at the angle beta from s = n x d towards p = d x s,
    formed at high precision and rounded once; scale_n, scale_d: |n| - 1 and |d| - 1 on top of that (ulps when +-1)."""
    import mpmath as mp
    with mp.workdps(exact.GDPS):
        u = u or _perp(d, rng)
        a = mp.mpf(float(alfa))
        n = [a * d[i] + mp.sqrt(1 - a * a) * u[i] for i in range(3)]
        s = exact._cross(n, d)
        ls = mp.sqrt(exact._dot(s, s))
        s = [v / ls for v in s]
        p = exact._cross(d, s)
        b = mp.mpf(float(beta))
        E = [mp.cos(b) * s[i] + mp.sin(b) * p[i] for i in range(3)]
        out = [[float(v) for v in w] for w in (d, E, n)]
    for k, sc in ((2, scale_n), (0, scale_d)):
        if abs(sc) == 1:        # one ulp of length: move the largest component
            j = int(np.argmax(np.abs(out[k])))
            out[k][j] = _ulps(out[k][j], int(sc) * (1 if out[k][j] > 0 else -1))
        elif sc:
            out[k] = [v * (1.0 + sc) for v in out[k]]
    return out[0] + out[1] + out[2]


@functools.lru_cache(maxsize=None)
def geom_rows():
    """(rows [n, 9] = d, E, n; family [n]; target alfa [n]).  Grazing angles alfa = 1e-13 ... 1 at 16 per decade for random
    orientations with E along s, along p, near each and random; negative alfa; E within 1e-16 ... 1e-3 rad of s and of p; |n| - 1
    and |d| - 1 in {0, +-1 ulp, +-1e-12}; d and n along the coordinate axes."""
    import mpmath as mp
    rng = np.random.default_rng(77)
    rows, fam, alf = [], [], []

    def add(name, alfa, r):
        rows.append(r); fam.append(name); alf.append(alfa)

    def rand_d():
        with mp.workdps(exact.GDPS):
            v = [mp.mpf(float(t)) for t in rng.normal(size=3)]
            l = mp.sqrt(exact._dot(v, v))
            return [t / l for t in v]

    grid_a = 10.0 ** (np.arange(13 * 16 + 1) / 16.0 - 13)
    grid_a[-1] = 1.0
    half_pi = float(mp.pi) / 2
    for rep in range(4):
        d = rand_d()
        for a in grid_a:
            for name, beta in (("E_s", 0.0), ("E_p", half_pi), ("E_rand", rng.uniform(0, 2 * np.pi)), ("E_near_s", 1e-8),
                               ("E_near_p", half_pi - 1e-8)):
                if a == 1.0:
                    dd = [float(v) for v in d]
                    add("normal_incidence", a, dd + [float(v) for v in _perp(d, rng)] + dd)
                    break
                add(name, a, _den_row(d, a, beta, rng))
    d = rand_d()
    for a in -10.0 ** np.arange(-16, -2.5, 1.0):
        add("alfa_negative", a, _den_row(d, a, 0.3, rng))
    for a in (1e-3, 1e-2, 0.3):
        for dec in range(-16, -2):
            add("E_near_s", a, _den_row(d, a, 10.0 ** dec, rng))
            add("E_near_p", a, _den_row(d, a, half_pi - 10.0 ** dec, rng))
    for a in (1e-6, 1e-3, 1e-2, 0.5):
        for sn in (0.0, 1, -1, 1e-12, -1e-12):
            for sd in (0.0, 1, -1, 1e-12, -1e-12):
                add("length", a, _den_row(d, a, 0.7, rng, scale_n=sn, scale_d=sd))
    axes = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    for i in range(3):
        for j in range(3):
            for sg in (1.0, -1.0):
                for k in range(3):
                    n = [sg * v for v in axes[j]]
                    add("axes", sg * float(i == j), [float(v) for v in axes[i]] + [float(v) for v in axes[k]] + n)
        with mp.workdps(exact.GDPS):
            da = [mp.mpf(v) for v in axes[i]]
            ua = [mp.mpf(v) for v in axes[(i + 1) % 3]]
            for a in 10.0 ** np.arange(-13, 0.0, 1.0):
                add("axis_d", a, _den_row(da, a, 0.4, rng, u=ua))
    return np.array(rows, dtype=np.float64), np.array(fam), np.array(alf)

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


# ---------------------------------------------------------------------------------------------------------------------------
# The march grids (op MARCH, tests/test_devmath_march_cpu.py): whole profiles of at most 64 nodes and photons aimed at the
# places where a certificate could be wrong.  Deterministic: no random numbers at all.
#
# Geometry that shapes the rays.  Within one segment the ray's offset from the axis is linear in z and so is R, hence the gap
# R - |q| is concave there: over any stretch of a profile the closest approach to the wall lies at a node, and a closest approach
# "mid-segment" exists only as a ray parallel to that segment's wall (the gap is then delta cap all along it).  So:
#   end    the ray closes in on the wall at rate s (the grazing slope, relative to the steepest wall on its way) and is
#          delta cap from it at node t, the end of a would-be block (t = i + L - 1, i + L, i + L + 1 for L = PC_L1, PC_L2);
#          delta < 0: it has crossed the wall by |delta| cap there, i.e. just before t
#   mid    delta > 0: parallel to the wall of one segment, delta cap from it; delta < 0: crosses that segment's wall at its middle
#   kink   delta cap from the wall at the kink node, where the wall sticks into blocks whose ends look safe
#   axis   parallel to z through the capillary's centre, from z = 0, from z > 0, and flying backwards (dz < 0)
#   first  starts on the axis with P.z + 1e-5 just below, at and beyond the next node
# A row is left out where doubles cannot place it: |delta| cap below 64 times the rounding of the start point and direction.
MARCH_DELTAS = (1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 1e-1)
MARCH_SLOPES = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 3e-2)
MARCH_K = 64
M_DZ, M_CAP, M_EXT, M_NS = 0.008, 4.0e-3, 0.11, 10
M_KINK = 31
PHI = 0.7                      # radial direction of the rays of capillaries that have no preferred one


def _n_cap(ns):
    return 3 * ns * (ns + 1) + 1


def march_problem(z, cap, ext, n_cap):
    import polycap_amd
    from tests.common import synthetic_constants
    E = np.array([10.0])
    amu, scatf = synthetic_constants(E)
    return polycap_amd.Problem(z, cap, ext, 0.0, n_cap, 2.23, E, amu, scatf)


def march_profiles():
    """name -> dict(z, cap, ext, ns, kink, rays): the profiles of the issue.  `rays` names the ray families a profile gets."""
    P = {}
    n = 62                     # at most nmax + 2 passes per row (every segment on its own, one lowered stride, the exit): K = 64
    j = np.arange(n)
    z = M_DZ * j
    u = z / z[-1]
    one = np.ones(n)
    full = ("axis", "first", "end", "mid")

    def put(name, z, f_cap, f_ext=None, ns=M_NS, cap0=M_CAP, ext0=M_EXT, kink=None, rays=full):
        f_ext = f_cap if f_ext is None else f_ext
        P[name] = dict(z=np.asarray(z, dtype=np.float64), cap=cap0 * np.asarray(f_cap), ext=ext0 * np.asarray(f_ext), ns=ns,
                       kink=kink, rays=rays)

    put("cylinder", z, one)
    put("taper", z, 1 - 0.6 * u)
    put("bulge", z, 0.6 + 0.4 * np.sqrt(1 - 0.96 * (2 * u - 1) ** 2))
    f = one.copy()
    f[M_KINK] = 0.7
    put("cap_kink", z, f, one, kink=M_KINK, rays=full + ("kink",))
    # a large n_cap: |k| of the outer shells is about 500, the axis of such a capillary steps sideways by 0.3 cap at the node
    ns, cap0, ext0 = 300, 8.0e-4, 0.6
    f = one.copy()
    f[M_KINK] = 1 + 0.3 * cap0 * (ns + 1) / (ns * ext0)
    put("ext_kink", z, one, f, ns=ns, cap0=cap0, ext0=ext0, kink=M_KINK, rays=full + ("kink",))
    # neighbouring segment lengths in ratio up to 1e4
    dz = np.array([M_DZ * (1e-4, 1.0, 1e-2, 1.0, 1e-3, 0.5, 1.0)[k % 7] for k in range(n - 1)])
    zi = np.concatenate([[0.0], np.cumsum(dz)])
    put("irregular", zi, 1 - 0.3 * zi / zi[-1])
    for nm in (1, 4, 5, 6, 24, 25, 26):
        zz = M_DZ * np.arange(nm + 1)
        put("nmax%d" % nm, zz, 1 - 0.3 * zz / zz[-1], rays=("axis", "last"))
    put("tiny", z, 1 - 0.3 * u, one, cap0=1.0e-6, ext0=1.0, rays=("axis", "first", "end"))
    put("last_zero", z, 1 - u, 1 - 0.5 * u, rays=("axis", "end"))
    put("mono", z, 1 - 0.3 * u, ns=0, ext0=5.0e-3, rays=("axis", "first", "end", "mid"))
    return P


def march_capillaries(ns):
    """(name, q, r): the centre, a middle shell, the outermost shell that is still classed non-boundary, and a boundary shell
    (its centres lie on the outer hexagon)"""
    if ns == 0:
        return [("centre", 0, 0)]
    a = int(round(0.3 * ns))
    return [("centre", 0, 0), ("middle", a, a - 1), ("outer", -a, ns), ("boundary", -a, ns + 1)]


def _ulp(x):
    return float(np.spacing(abs(float(x))))


class _Builder:
    def __init__(self, name, prof):
        from fractions import Fraction as F
        self.F = F
        self.name, self.prof = name, prof
        self.z, self.cap, self.ext = prof["z"], prof["cap"], prof["ext"]
        self.nmax = len(self.z) - 1
        self.hexscale = 2.0 * 0.86602540378443864676 * (prof["ns"] + 1)
        self.zh = self.ext / self.hexscale          # as pc_build_tables forms it (asserted against the accessor by the tests)
        self.rows, self.meta = [], []

    def k(self, q, r):
        return ((2.0 * q + r) * 0.86602540378443864676, r * 1.5)

    def axis_slope(self, k, j):
        s = (self.zh[j + 1] - self.zh[j]) / (self.z[j + 1] - self.z[j])
        return np.array([k[0] * s, k[1] * s])

    def at(self, tab, zv):
        return float(np.interp(zv, self.z, tab))

    def seg_of(self, zv):
        return int(min(self.nmax - 1, max(0, np.searchsorted(self.z, zv, side="right") - 1)))

    def radial(self, capname, k):
        kn = float(np.hypot(*k))
        if kn > 0 and (capname == "boundary" or self.name == "ext_kink"):
            return np.array([-k[0] / kn, -k[1] / kn])           # towards the optic's axis: where an ext kink pushes the wall in
        return np.array([np.cos(PHI), np.sin(PHI)])

    def add(self, capname, k, fam, P, d, delta=0.0, block=(0, 0), tnode=-1, s=0.0):
        self.rows.append([P[0], P[1], P[2], d[0], d[1], d[2], 0.3, 0.5, 0.1, 0.0, float(MARCH_K)])
        self.meta.append(dict(profile=self.name, cap=capname, k=k, fam=fam, delta=delta, block=block, tnode=tnode, s=s))

    def aimed(self, capname, k, fam, zt, rt, D, zs, delta, block, tnode, s, flip=False):
        """the ray with xy slope D that is at c(zt) + e rt at z = zt, started at zs: P in rational arithmetic, rounded once"""
        F = self.F
        e = self.radial(capname, k)
        zh_t = F(self.at(self.zh, zt))
        tgt = [F(k[0]) * zh_t + F(float(e[0])) * F(rt), F(k[1]) * zh_t + F(float(e[1])) * F(rt)]
        back = F(zt) - F(zs)
        P = [float(tgt[0] - F(float(D[0])) * back), float(tgt[1] - F(float(D[1])) * back), float(zs)]
        # can doubles place it?  rounding of P, and of the direction's normalisation over the distance flown
        noise = _ulp(max(abs(P[0]), abs(P[1]), abs(rt))) + 2.0 ** -52 * float(np.hypot(*D)) * float(back)
        if delta != 0.0 and abs(delta) * self.at(self.cap, zt) < 64 * noise:
            return False
        d = [float(D[0]), float(D[1]), 1.0]
        if flip:
            d = [-v for v in d]
        self.add(capname, k, fam, P, d, delta, block, tnode, s)
        return True

    def start_for(self, capname, k, zt, rt, D, first_choice, lo_frac, need):
        """the earliest start among first_choice and the middles of the later segments at which the ray lies inside the capillary
        by at least half of what it was built to (need(zt - zs)), its offset along e no further back than lo_frac R"""
        e = self.radial(capname, k)
        cands = [first_choice] + [0.5 * (self.z[j] + self.z[j + 1]) for j in range(self.seg_of(first_choice) + 1, self.seg_of(zt))]
        cands.append(zt - 0.25 * (zt - self.z[max(0, self.seg_of(zt) - (1 if zt == self.z[self.seg_of(zt)] else 0))]))
        ct = np.array(k) * self.at(self.zh, zt)
        for zs in cands:
            if not zs < zt:
                continue
            p = ct + e * rt - np.asarray(D) * (zt - zs)
            q = p - np.array(k) * self.at(self.zh, zs)
            R = self.at(self.cap, zs)
            gap = R - float(np.hypot(*q))
            if gap > 0 and gap >= 0.5 * need(zt - zs) and float(q @ e) >= lo_frac * R:
                return zs
        return None

    def closing_rate(self, k, ja, jb, jt):
        """steepest wall seen from the ray's frame over segments [ja, jb): dR/dz plus the bend of the axis against segment jt's"""
        ct = self.axis_slope(k, jt)
        w = 0.0
        for j in range(ja, jb):
            dz = self.z[j + 1] - self.z[j]
            w = max(w, (self.cap[j + 1] - self.cap[j]) / dz + float(np.hypot(*(self.axis_slope(k, j) - ct))))
        return w


def _march_rows_of(name, prof):
    B = _Builder(name, prof)
    nmax, z, cap = B.nmax, B.z, B.cap
    L1, L2 = 5, 25
    count = 0
    for capname, q, r in march_capillaries(prof["ns"]):
        k = B.k(q, r)
        bnd = capname == "boundary"
        lo_frac = 0.05 if bnd else -0.9
        e = B.radial(capname, k)
        inward = e * (0.5 if bnd else 0.0)          # a boundary capillary's centre lies on the hexagon: stay on its inner half

        def on_axis(zs):
            c = np.array(k) * B.at(B.zh, zs) + inward * B.at(B.cap, zs)
            return [float(c[0]), float(c[1]), float(zs)]

        if "axis" in prof["rays"]:
            B.add(capname, k, "axis", on_axis(0.0), [0.0, 0.0, 1.0])
            if nmax >= 3:
                zs = 0.5 * (z[1] + z[2])
                B.add(capname, k, "axis", on_axis(zs), [0.0, 0.0, 1.0])
                B.add(capname, k, "axis_back", on_axis(zs), [0.0, 0.0, -1.0])
        if "first" in prof["rays"]:
            base = z[3] - 1.0e-5
            at = base
            for _ in range(8):                       # the double whose sum with 1e-5 rounds to the node itself
                if at + 1.0e-5 == z[3]:
                    break
                at = float(np.nextafter(at, 1.0 if at + 1.0e-5 < z[3] else 0.0))
            for zs in (base - 1e-9, float(np.nextafter(at, 0.0)), at, float(np.nextafter(at, 1.0)), base + 1e-9, base - 1.0e-5):
                D = B.axis_slope(k, 2) + 1e-4 * e
                B.add(capname, k, "first", on_axis(zs), [float(D[0]), float(D[1]), 1.0])

        def end_family(i0, t, fam, deltas):
            nonlocal count
            if t > nmax or t < 1 or not cap[t] > 0:
                return
            for delta in deltas:
                s = MARCH_SLOPES[count % len(MARCH_SLOPES)]
                count += 1
                first = 0.0 if i0 <= 1 else 0.5 * (z[i0 - 1] + z[i0])
                W = B.closing_rate(k, B.seg_of(first), t, t - 1)
                D = B.axis_slope(k, t - 1) + (W + s) * e
                rt = cap[t] * (1 - delta)
                zs = B.start_for(capname, k, z[t], rt, D, first, lo_frac, lambda back: delta * cap[t] + s * back)
                if zs is None:
                    continue
                B.aimed(capname, k, fam, z[t], rt, D, zs, delta, (B.seg_of(zs), t), t, s)
                if fam == "end_L2" and t == i0 + L2 and delta in (1e-9, -1e-9):
                    B.aimed(capname, k, fam + "_back", z[t], rt, D, zs, delta, (B.seg_of(zs), t), t, s, flip=True)

        if "end" in prof["rays"]:
            for L, i0, fam in ((L1, 1, "end_L1"), (L2, 2, "end_L2")):
                for t in (i0 + L - 1, i0 + L, i0 + L + 1):
                    end_family(i0, t, fam, MARCH_DELTAS)
        if "last" in prof["rays"]:
            end_family(0, nmax, "last", (1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3))
        if "mid" in prof["rays"]:
            js = 14
            zt = 0.5 * (z[js] + z[js + 1])
            Rt = B.at(cap, zt)
            w = (cap[js + 1] - cap[js]) / (z[js + 1] - z[js])
            for delta in MARCH_DELTAS:
                if delta > 0:
                    D = B.axis_slope(k, js) + w * e
                    rt = Rt - delta * Rt
                    first = 0.5 * (z[1] + z[2])
                    zs = B.start_for(capname, k, zt, rt, D, first, lo_frac, lambda back: delta * Rt)
                    # a tangent to a bulging wall lies outside it further back: such a ray starts in the segment itself
                    ok = zs is not None and all(
                        float(np.hypot(*(np.array(k) * B.at(B.zh, zt) + e * rt - D * (zt - zz) - np.array(k) * B.at(B.zh, zz))))
                        < B.at(cap, zz) - 0.5 * delta * Rt for zz in z[B.seg_of(zs) + 1:js + 1])
                    if not ok:
                        zs = z[js] + 0.25 * (z[js + 1] - z[js])
                    B.aimed(capname, k, "mid", zt, rt, D, zs, delta, (js, js + 1), js, 0.0)
                else:
                    s = max(MARCH_SLOPES[count % len(MARCH_SLOPES)], 4 * abs(delta) * Rt / (z[js + 1] - z[js]))
                    count += 1
                    first = 0.5 * (z[1] + z[2])
                    W = B.closing_rate(k, B.seg_of(first), js + 1, js)
                    D = B.axis_slope(k, js) + (W + s) * e
                    rt = Rt * (1 - delta)
                    zs = B.start_for(capname, k, zt, rt, D, first, lo_frac, lambda back: delta * Rt + s * back)
                    if zs is not None:
                        B.aimed(capname, k, "mid", zt, rt, D, zs, delta, (js, js + 1), js, s)
        if "kink" in prof["rays"] and not (name == "ext_kink" and capname == "centre"):      # the centre's axis has no kink
            kn = prof["kink"]
            for start_seg in (kn - 13, kn - 4):
                zs = 0.5 * (z[start_seg] + z[start_seg + 1])
                for delta in MARCH_DELTAS:
                    s = (1e-6, -1e-4, 1e-3, -1e-3, 1e-2, 1e-4)[count % 6]
                    count += 1
                    D = B.axis_slope(k, kn - 3) + s * e
                    # the start must lie inside the capillary (where nothing sticks in, a ray that leaves the wall comes from
                    # outside it)
                    q = np.array(k) * B.at(B.zh, z[kn]) + e * cap[kn] * (1 - delta) - D * (z[kn] - zs) - np.array(k) * B.at(B.zh, zs)
                    if not (float(np.hypot(*q)) < 0.95 * B.at(cap, zs) and float(q @ e) >= lo_frac * B.at(cap, zs)):
                        continue
                    B.aimed(capname, k, "kink", z[kn], cap[kn] * (1 - delta), D, zs, delta, (kn - 1, kn + 1), kn, s)
    return np.array(B.rows, dtype=np.float64).reshape(-1, 11), B.meta


@functools.lru_cache(maxsize=None)
def march_grids():
    """name -> dict(problem, profile, rows [n, 11] of pyprobe.MARCH_COLS (literal 0, K = 64), meta [n])"""
    out = {}
    for name, prof in march_profiles().items():
        rows, meta = _march_rows_of(name, prof)
        out[name] = dict(problem=march_problem(prof["z"], prof["cap"], prof["ext"], _n_cap(prof["ns"])), profile=prof, rows=rows,
                         meta=meta)
    return out

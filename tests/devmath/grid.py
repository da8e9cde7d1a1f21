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


# ---------------------------------------------------------------------------------------------------------------------------
# The leak grids (ops WALL, OUTER, HEX; tests/test_devmath_leak_cpu.py): photons in the glass aimed at the places where a skip
# certificate of pc_leak.h could be wrong.  Deterministic.  Rays are laid out in double precision in the frame of a hexagon cell and
# the graze points placed in rational arithmetic (one rounding of P); what a row really does is decided by the exact side
# (check_built of the test), never by this file.
#
# A cell (q, r) has its centre at K zz(z), K = ((2 q + r) cos30, 1.5 r), inradius cos30 zz and corners at distance zz at 30 + 60 k
# degrees; its edge k has the outward normal at 60 k degrees.  Families (meta["fam"]):
#   cap    closest approach to the cell's own capillary is cap (1 + delta), at a node, mid-segment and at the kink node
#   corner leaves the cell through an edge at delta zz from a corner
#   edge   runs parallel to an edge, delta zz inside (delta > 0) or outside (delta < 0: in the neighbouring cell) of it
#   xnode  crosses an edge within delta of a node in z
#   exit   reaches the exit plane inside the glass;  side  leaves the stack sideways
#   nbr    enters the neighbouring cell and passes its capillary at cap (1 + delta) at node t; the crossing lies in segment
#          t - L + 1, t - L or t - L - 1 for both strides L, t also the kink node and the last three nodes
#   back   dz < 0, at most 256 units;  begin  starts beyond the last node or outside the hexagon;  grid  the aligned profile's
#          axis-parallel photons whose every step lands on a node;  mono  the mono-capillary, straight to the probe
LEAK_SLOPES = (1e-4, 1e-3, 1e-2, 1e-1, 0.3)
LEAK_UNITS = 4096                  # every row ends within this many units in certified mode
C30 = 0.86602540378443864676
G14 = 2.0 ** -14


def leak_profiles():
    P = dict(march_profiles())
    for v in P.values():
        v["leak"] = "basic"
    for k in ("taper", "bulge", "cap_kink", "ext_kink", "irregular"):
        P[k]["leak"] = "full"
    P["cylinder"]["leak"] = P["tiny"]["leak"] = P["last_zero"]["leak"] = "cross"
    P["mono"]["leak"] = "mono"
    # every literal step of an axis-parallel photon lands on a node: steps of 2^-14 (cap 10 2^-14), nodes on multiples of 2^-8; in
    # the second half the radius alternates between 10 and 20 2^-14, so the step over a node is taken with another size than the
    # steps behind it
    n = 41
    j = np.arange(n)
    P["aligned"] = dict(z=64 * G14 * j, cap=10 * G14 * np.where((j >= 20) & (j % 2 == 1), 2.0, 1.0), ext=0.03 * np.ones(n), ns=10,
                        kink=None, rays=(), leak="aligned")
    # room for more than 1e6 steps in one segment (the cap on the step count m)
    z = np.array([0.0, 0.25, 0.5, 0.51, 0.52, 0.53, 0.54, 0.55])
    P["long"] = dict(z=z, cap=1.0e-6 * np.ones(8), ext=np.ones(8), ns=10, kink=None, rays=(), leak="long")
    return P


def leak_cells(ns):
    """march_capillaries' four, one more cell on the outermost shell and one just outside it"""
    if ns == 0:
        return [("centre", 0, 0)]
    return march_capillaries(ns) + [("shell", ns, -3), ("beyond", ns + 1, -3)]


def _rot(deg):
    a = np.deg2rad(deg)
    return np.array([np.cos(a), np.sin(a)])


class _LeakBuilder(_Builder):
    def __init__(self, name, prof):
        super().__init__(name, prof)
        self.ns = prof["ns"]
        self.count = 0

    def slope(self):
        self.count += 1
        return LEAK_SLOPES[self.count % len(LEAK_SLOPES)]

    def inside_stack(self, q, r):
        return abs(q) <= self.ns and abs(r) <= self.ns and abs(q + r) <= self.ns

    def forms(self, p, zv, q, r):
        """max |a_k| / zz of the point p at height zv against cell (q, r), in doubles"""
        zz = self.at(self.zh, zv)
        Q = p[0] / (2 * C30) - p[1] / 3 - q * zz
        R = p[1] * (2.0 / 3) - r * zz
        return max(abs(Q - R), abs(2 * Q + R), abs(Q + 2 * R)) / zz

    def in_glass(self, p, zv, q, r, margin=1e-3):
        k = np.array(self.k(q, r))
        if not self.forms(p, zv, q, r) < 1 - margin:
            return False
        if self.prof["ns"] and not pc_inside_outer(self.at(self.ext, zv), p):
            return False
        return (not self.inside_stack(q, r)) or float(np.hypot(*(p - k * self.at(self.zh, zv)))) > self.at(self.cap, zv) * (1 + margin)

    def exit_segment(self, P, D, q, r):
        """segment in which the ray P + (D, 1) t first leaves cell (q, r), in doubles (None: not before the last node)"""
        for j in range(self.seg_of(P[2]) + 1, self.nmax + 1):
            p = np.array(P[:2]) + np.asarray(D) * (self.z[j] - P[2])
            if self.forms(p, self.z[j], q, r) > 1:
                return j - 1
        return None

    def put(self, cell, fam, P, D, delta=0.0, zt=None, tnode=-1, block=None, literal_cap=None, flip=False, **more):
        """a row from the start P and the transverse slope D; the direction is normalised in doubles (the row's d is the ray)"""
        d = np.array([D[0], D[1], 1.0])
        d = d / np.sqrt(d @ d)
        if flip:
            d = -d
        self.rows.append([P[0], P[1], P[2], d[0], d[1], d[2], 0.0, -1.0, float(256 if flip else LEAK_UNITS)])
        m = dict(profile=self.name, cell=cell, fam=fam, delta=delta, zt=zt, tnode=tnode, block=block)
        m.update(more)
        self.meta.append(m)

    def graze_ok(self, target, zt, D, zs, zhi, K, delta, cap_t):
        """in doubles: |u|^2 - cap^2 of the ray through `target` at zt against the axis K zh is smallest at zt among the nodes and
        the middles of the segments of [zs, zhi] (a row whose closest approach lies elsewhere is not what its family means)"""
        want = delta * cap_t * (2 * cap_t + delta * cap_t)
        tg = np.array([float(target[0]), float(target[1])])
        zs_ = [zs, zhi] + [v for v in self.z if zs < v < zhi]
        zs_ += [0.5 * (a + b) for a, b in zip(sorted(zs_)[:-1], sorted(zs_)[1:])]
        zs_ += [zt + sg * f * (zhi - zs) for sg in (1, -1) for f in (1e-2, 1e-4, 1e-6, 1e-8) if zs <= zt + sg * f * (zhi - zs) <= zhi]
        for zv in zs_:
            u = tg + np.asarray(D) * (zv - zt) - np.asarray(K) * self.at(self.zh, zv)
            f = float(u @ u) - self.at(self.cap, zv) ** 2
            if f < (0.75 * want if delta > 0 else 1.5 * want):
                return False
        return True

    def through(self, cell, fam, target, zt, D, zs, delta, scale, **more):
        """the ray with transverse slope D that passes `target` (two Fractions) at z = zt, started at zs: P rounded once; left out
        where doubles cannot place a deviation of delta `scale`"""
        F = self.F
        back = F(float(zt)) - F(float(zs))
        P = [float(target[0] - F(float(D[0])) * back), float(target[1] - F(float(D[1])) * back), float(zs)]
        noise = _ulp(max(abs(P[0]), abs(P[1]))) + 2.0 ** -52 * float(np.hypot(*D)) * abs(float(back))
        if delta != 0.0 and abs(delta) * scale < 64 * noise:
            return False
        self.put(cell, fam, P, D, delta, zt=float(zt), **more)
        return True


def pc_inside_outer(ext, p):
    d = np.sqrt(ext * ext - (ext / 2) * (ext / 2))
    return max(abs(p[1]), abs(C30 * p[0] + 0.5 * p[1]), abs(C30 * p[0] - 0.5 * p[1])) < d * (1 - 1e-3)


def _wall_rows_of(name, prof):
    B = _LeakBuilder(name, prof)
    F = B.F
    z, cap, zh, nmax = B.z, B.cap, B.zh, B.nmax
    kind = prof["leak"]
    seg = lambda j: z[j + 1] - z[j]

    def centre(q, r, zv):
        return np.array(B.k(q, r)) * B.at(zh, zv)

    def centre_slope(q, r, j):
        return B.axis_slope(B.k(q, r), j)

    def zh_slope(j):
        return (zh[j + 1] - zh[j]) / seg(j)

    def cap_slope(j):
        return (cap[j + 1] - cap[j]) / seg(j)

    def inward(q, r):
        """unit vector from the cell towards the optic's axis (any direction for the centre cell)"""
        k = np.array(B.k(q, r))
        n = float(np.hypot(*k))
        return -k / n if n > 0 else _rot(20.0)

    cells = leak_cells(prof["ns"])

    # ---- every profile: a photon that flies on to the exit plane inside the glass, one flying backwards, starts that return at once
    for cell, q, r in cells[:1] + cells[2:3]:
        e = inward(q, r)
        j0 = max(0, nmax - 6)
        zs = z[j0] + 0.5 * seg(j0) if nmax > 1 else 0.25 * z[1]
        if kind in ("long", "cross") and name != "last_zero":
            zs = z[nmax - 1] + 0.5 * seg(nmax - 1)
        p = centre(q, r, zs) + 0.93 * B.at(zh, zs) * _rot(30.0 if q == r == 0 else np.rad2deg(np.arctan2(e[1], e[0])) + 30.0)
        if prof["ns"] == 0:
            p = 0.5 * (B.at(cap, zs) + B.at(B.ext, zs)) * _rot(30.0)
        if prof["ns"] == 0 or B.in_glass(p, zs, q, r, 1e-2):
            D = centre_slope(q, r, min(j0, nmax - 1)) + 1e-4 * _rot(100.0)
            B.put(cell, "exit", [p[0], p[1], zs], D)
            if kind not in ("long", "cross"):
                B.put(cell, "back", [p[0], p[1], zs], D, flip=True)
    zend = z[nmax]
    c0 = centre(0, 0, zend) + 0.93 * zh[nmax] * _rot(30.0)
    B.put("centre", "begin", [c0[0], c0[1], zend], [1e-3, 0.0], expect="beyond")
    B.put("centre", "begin", [c0[0], c0[1], float(np.nextafter(zend, 0.0))], [1e-3, 0.0], expect="in")
    B.put("centre", "begin", [1.5 * B.ext[0], 0.0, 0.5 * z[1]], [1e-3, 0.0], expect="outside")

    if kind == "aligned":
        # on the grid: d = (0, 0, 1), P.z a multiple of 2^-14, in the glass of four cells; every step lands on a multiple of 2^-14 and
        # every 64th (32nd) on a node
        for cell, q, r in cells[:3] + cells[4:5]:
            for zs in (0.0, 64 * G14, 3 * G14, 20 * 64 * G14 + G14, 37 * 64 * G14):
                p = centre(q, r, zs) + 0.93 * zh[0] * _rot(30.0)
                B.put(cell, "grid", [p[0], p[1], zs], [0.0, 0.0])
    if kind == "long":
        for cell, q, r in cells[:2]:
            for zs, s in ((0.0, 0.0), (1.0e-3, 1e-4), (0.2, 1e-3)):
                p = centre(q, r, zs) + 0.5 * zh[0] * _rot(30.0)
                B.put(cell, "exit", [p[0], p[1], zs], s * _rot(70.0))
            # grazing the capillary inside the long segment
            for delta in (1e-9, -1e-9, 1e-3, -1e-3):
                if q == r == 0:
                    e, zt = _rot(10.0), 0.1
                    D = 0.1 * _rot(100.0)
                    tgt = [F(float(e[0])) * F(float(cap[0] * (1 + delta))), F(float(e[1])) * F(float(cap[0] * (1 + delta)))]
                    B.through(cell, "cap", tgt, zt, D, zt - 4e-5, delta, cap[0], block=(zt - 4e-5, zt + 4e-5))

    # ---- crossing into the neighbour early: what gives the probe room for its widest blocks
    if kind in ("full", "cross", "aligned") and nmax >= 27:
        for cell, q, r in cells[:2]:
            for jn, deltas in ((4, MARCH_DELTAS if kind != "cross" else (1e-9, -1e-9, 1e-3)),):
                for delta in deltas:
                    s = (0.3, 0.1)[B.count % 2] if kind != "full" else max(B.slope(), 1e-3)
                    B.count += 1
                    zx = z[jn] + delta * seg(jn)
                    n_hat = _rot(0.0)
                    D = centre_slope(q, r, jn) + (s + C30 * abs(zh_slope(jn))) * n_hat
                    tgt = centre(q, r, zx) + C30 * B.at(zh, zx) * n_hat + 0.1 * B.at(zh, zx) * _rot(90.0)
                    bt = 0.3 * (C30 * B.at(zh, zx) - B.at(cap, zx))
                    zs = max(zx - bt / s, 0.5 * (z[0] + z[1]) if jn > 1 else 0.0)
                    if not zs < zx - 4 * abs(delta) * seg(jn):
                        continue
                    P = [tgt[0] - D[0] * (zx - zs), tgt[1] - D[1] * (zx - zs), zs]
                    if B.in_glass(np.array(P[:2]), zs, q, r):
                        B.through(cell, "xnode", [F(float(tgt[0])), F(float(tgt[1]))], zx, D, zs, delta, s * seg(jn), tnode=jn, nbr=(q + 1, r))
            # a shallow crossing next to a corner: the ray stays in the neighbour's glass for dozens of segments
            for delta in (1e-3, -1e-3):
                jn, s = 2, 1e-3
                zx = z[jn] + delta * seg(jn)
                n_hat = _rot(0.0)
                D = centre_slope(q, r, jn) + (s + C30 * abs(zh_slope(jn))) * n_hat
                tgt = centre(q, r, zx) + C30 * B.at(zh, zx) * n_hat + 0.47 * B.at(zh, zx) * _rot(90.0)
                zs = 0.5 * (z[0] + z[1])
                P = [tgt[0] - D[0] * (zx - zs), tgt[1] - D[1] * (zx - zs), zs]
                if B.in_glass(np.array(P[:2]), zs, q, r):
                    B.put(cell, "xnode", P, D, delta, zt=zx, tnode=jn, nbr=(q + 1, r))

    if kind == "mono":
        for t in (10, 30, 55):
            for delta in MARCH_DELTAS:
                s = B.slope()
                e = _rot(40.0 * (B.count % 9))
                rho = cap[t] * (1 + delta)
                D = s * np.array([-e[1], e[0]]) + cap_slope(t - 1) * e
                bt = min(0.8 * np.sqrt(max(B.at(B.ext, z[t]) ** 2 - rho ** 2, 0.0)), s * (z[t] - z[1]))
                zs = z[t] - bt / s
                p = rho * e - D * (z[t] - zs)
                if not (np.hypot(*p) < 0.98 * B.at(B.ext, zs) and np.hypot(*p) > 1.001 * B.at(cap, zs)):
                    continue
                tgt = [F(float(e[0])) * F(float(rho)), F(float(e[1])) * F(float(rho))]
                if not B.graze_ok(tgt, z[t], D, zs, z[min(nmax, t + 1)], (0.0, 0.0), delta, cap[t]):
                    continue
                B.through("centre", "mono", tgt, z[t], D, zs, delta, cap[t], tnode=t, block=(zs, z[min(nmax, t + 1)]), nbr=(0, 0))

    if kind != "full":
        return B

    kink = prof["kink"]
    for cell, q, r in cells:
        K = np.array(B.k(q, r))
        stack = B.inside_stack(q, r)
        away = -inward(q, r)

        # ---- cap: grazing the cell's own capillary
        if stack:
            places = [("node", 9, z[9]), ("mid", 14, 0.5 * (z[14] + z[15]))] + ([("kink", kink, z[kink])] if kink else [])
            for where, jt, zt in places:
                for delta in MARCH_DELTAS:
                    s = B.slope()
                    e = _rot(60.0 * (B.count % 6) + 11.0)
                    tng = np.array([-e[1], e[0]])
                    rho = B.at(cap, zt) * (1 + delta)
                    # the gap |u| - cap has slope 0 at zt on one side; at a node the side that makes it a minimum
                    sides = [jt] if where == "mid" else [jt, jt - 1]
                    done = False
                    for js in sides:
                        if done:
                            continue
                        w = s * tng + cap_slope(js) * e
                        D = centre_slope(q, r, js) + w
                        if where != "mid":
                            jo = jt - 1 if js == jt else jt
                            wo = D - centre_slope(q, r, jo)
                            go = float(e @ wo) - cap_slope(jo)          # slope of the gap on the other side
                            if (jo < js and go > 0) or (jo > js and go < 0):
                                continue
                        inr = C30 * B.at(zh, zt)
                        bt = min(0.5 * np.sqrt(max(inr * inr - rho * rho, 0.0)), s * (zt - 0.5 * z[1]))
                        zs = zt - bt / s
                        zhi = min(z[nmax], zt + 0.5 * bt / s)
                        p = centre(q, r, zt) + rho * e - D * (zt - zs)
                        if B.forms(p, zs, q, r) >= 1 - 1e-3 or not pc_inside_outer(B.at(B.ext, zs), p):
                            continue
                        ct = [F(K[0]) * F(B.at(zh, zt)) + F(float(e[0])) * F(float(rho)), F(K[1]) * F(B.at(zh, zt)) + F(float(e[1])) * F(float(rho))]
                        if not B.graze_ok(ct, zt, D, zs, zhi, K, delta, B.at(cap, zt)):
                            continue
                        done = B.through(cell, "cap", ct, zt, D, zs, delta, B.at(cap, zt), tnode=jt, block=(zs, zhi), where=where)

        # ---- corner, edge, xnode
        for kedge in ((0, 2, 3, 5) if cell in ("centre", "outer", "shell", "beyond") else (2,)):
            n_hat = _rot(60.0 * kedge)
            t_hat = _rot(60.0 * kedge + 90.0)
            if not stack and float(n_hat @ away) > 0.3:
                continue                      # a cell on or beyond the rim: only its inner edges lie inside the optic
            js = 20 + kedge
            zt = z[js] + 0.5 * seg(js)
            zz_t = B.at(zh, zt)
            for delta in MARCH_DELTAS:
                # corner: through the point delta zz along the edge from its corner at 60 k + 30 degrees
                s = B.slope()
                corner = zz_t * _rot(60.0 * kedge + 30.0)
                tgt = centre(q, r, zt) + corner - delta * zz_t * t_hat
                D = centre_slope(q, r, js) + (s + abs(zh_slope(js))) * n_hat
                bt = 0.3 * (zz_t - B.at(cap, zt))
                zs = max(zt - bt / s, 0.5 * z[1])
                P = [tgt[0] - D[0] * (zt - zs), tgt[1] - D[1] * (zt - zs), zs]
                if B.in_glass(np.array(P[:2]), zs, q, r, 1e-6):
                    B.put(cell, "corner", P, D, delta, zt=zt, tnode=js, kedge=kedge)
                # edge: parallel to the edge, delta zz from it
                s = B.slope()
                je = 33                       # an all-literal flight (inside the margin) from here to the end stays under LEAK_UNITS
                zs = z[je] + 0.25 * seg(je)
                zz_s = B.at(zh, zs)
                p = centre(q, r, zs) + (C30 - delta) * zz_s * n_hat - 0.3 * zz_s * t_hat
                D = centre_slope(q, r, je) + (C30 - delta) * zh_slope(je) * n_hat + s * t_hat
                if pc_inside_outer(B.at(B.ext, zs), p):
                    B.put(cell, "edge", [p[0], p[1], zs], D, delta, zt=zs, tnode=je, kedge=kedge, zb=zs + min(0.7 * seg(je), 0.4 * zz_s / s))
            for jn in (30,):
                for delta in MARCH_DELTAS:
                    s = B.slope()
                    zx = z[jn] + delta * seg(jn)
                    jx = jn if delta > 0 else jn - 1
                    D = centre_slope(q, r, jx) + (s + C30 * abs(zh_slope(jx))) * n_hat
                    tgt = centre(q, r, zx) + C30 * B.at(zh, zx) * n_hat + 0.1 * B.at(zh, zx) * t_hat
                    bt = 0.3 * (C30 * B.at(zh, zx) - B.at(cap, zx))
                    zs = max(zx - bt / s, 0.5 * z[1])
                    P = [tgt[0] - D[0] * (zx - zs), tgt[1] - D[1] * (zx - zs), zs]
                    if zs < zx - 4 * abs(delta) * seg(jn) and B.in_glass(np.array(P[:2]), zs, q, r):
                        B.through(cell, "xnode", [F(float(tgt[0])), F(float(tgt[1]))], zx, D, zs, delta, s * seg(jn), tnode=jn, kedge=kedge)

        # ---- side: out of the stack
        if cell in ("outer", "shell"):
            for s in (0.05, 0.1, 0.3):
                for zs in (z[10] + 0.3 * seg(10), z[40] + 0.3 * seg(40)):
                    p = centre(q, r, zs) + 0.9 * B.at(zh, zs) * _rot(np.rad2deg(np.arctan2(away[1], away[0])) + 30.0)
                    if B.in_glass(p, zs, q, r, 1e-2):
                        B.put(cell, "side", [p[0], p[1], zs], centre_slope(q, r, 10) + s * away)

        # ---- nbr: into the neighbour (q + 1, r), past its capillary at cap (1 + delta) at node t
        qn, rn = q + 1, r
        if stack and B.inside_stack(qn, rn):
            KN = np.array(B.k(qn, rn))
            plan = [(40, L, 40 - L + 1 - a, "L%d%+d" % (L, -a)) for L in (5, 25) for a in (0, 1, 2)]
            plan += [(t, 5, t - 5, "end") for t in (nmax - 2, nmax - 1, nmax)]
            if kink:
                plan += [(kink, 5, kink - 3, "kink"), (kink, 25, kink - 12, "kink")]
            for t, L, ic, tag in plan:
                for delta in MARCH_DELTAS:
                    zt, zx = z[t], z[ic] + 0.5 * seg(ic)
                    rho = cap[t] * (1 + delta) if cap[t] > 0 else 0.0
                    X = np.array([-C30, 0.3]) * B.at(zh, zx)                     # on the shared edge, seen from the neighbour's centre
                    d0 = float(np.hypot(*X))
                    if not rho < 0.98 * d0:
                        continue
                    th = np.arctan2(X[1], X[0]) - np.arccos(rho / d0)
                    e = np.array([np.cos(th), np.sin(th)])
                    G = rho * e
                    run = G - X
                    ell = float(np.hypot(*run))
                    sig = ell / (zt - zx)
                    tgt = [F(KN[0]) * F(B.at(zh, zt)) + F(float(e[0])) * F(float(rho)), F(KN[1]) * F(B.at(zh, zt)) + F(float(e[1])) * F(float(rho))]
                    for js in (t - 1, min(t, nmax - 1)):         # the side of the node on which the gap has slope 0: the one that makes it a minimum
                        D = B.axis_slope(KN, js) + sig * run / ell + cap_slope(js) * e
                        bt = 0.25 * (B.at(zh, zx) - B.at(cap, zx))
                        zs = max(zx - bt / sig, z[max(ic - 1, 0)] + 0.1 * seg(max(ic - 1, 0)))
                        p = KN * B.at(zh, zt) + G - D * (zt - zs)
                        if not B.in_glass(p, zs, q, r) or B.exit_segment([p[0], p[1], zs], D, q, r) != ic:
                            continue
                        if not B.graze_ok(tgt, zt, D, z[B.seg_of(zs)], z[min(nmax, t + 1)], KN, delta, cap[t]):
                            continue
                        if B.through(cell, "nbr", tgt, zt, D, zs, delta, cap[t], tnode=t, block=(zs, zt), nbr=(qn, rn), tag=tag, ic=ic, L=L):
                            break
    return B


@functools.lru_cache(maxsize=None)
def wall_grids():
    """name -> dict(problem, profile, rows [n, 9] of pyprobe.WALL_COLS (literal 0, hint -1), meta [n])"""
    out = {}
    for name, prof in leak_profiles().items():
        B = _wall_rows_of(name, prof)
        out[name] = dict(problem=march_problem(prof["z"], prof["cap"], prof["ext"], _n_cap(prof["ns"])), profile=prof,
                         rows=np.array(B.rows, dtype=np.float64).reshape(-1, 9), meta=B.meta)
    return out


# ---- OUTER: c on the exit plane outside the hexagon, dz > 0.  Going backwards along the edge with normal (0, 1):
#   dip    the ray is inside the outer hexagon by delta ext at exactly one node j (y = hexd_j (1 - delta) there, dy/dz between the
#          slopes of hexd on both sides): where the hexagon sticks out at a node (ext_kink's kink, every node of the bulge);
#          delta < 0: nowhere inside (return 0)
#   cross  the ray enters the hexagon between nodes j + 1 and j, delta ext deep at node j: on every profile
# j takes the positions 1 .. L - 1 of the blocks the scan would skip (nodes nmax - L .. nmax and the block below, both strides).  A
# row whose pattern of inside / outside nodes is not the one meant (in doubles) is left out.
OUTER_PROFILES = ("ext_kink", "bulge", "irregular", "cylinder", "taper")


@functools.lru_cache(maxsize=None)
def outer_grids():
    """name -> dict(problem, rows [n, 7] of pyprobe.OUTER_COLS (literal 0), meta [n])"""
    from fractions import Fraction as F
    out = {}
    profs = leak_profiles()
    for name in OUTER_PROFILES:
        prof = profs[name]
        z, ext = prof["z"], prof["ext"]
        nmax = len(z) - 1
        hexd = np.sqrt(ext * ext - (ext / 2) * (ext / 2))
        rows, meta = [], []
        nodes = []
        for L in (5, 25):
            for blk in (0, 1):
                hi = nmax - blk * L
                nodes += [(hi - L + pos, L, pos) for pos in range(1, L) if 1 <= hi - L + pos < nmax]
        if prof["kink"]:
            nodes.append((prof["kink"], 25, prof["kink"] - (nmax - 50)))

        def add(fam, j, L, pos, delta, yj, Dy):
            x = 0.01 * ext[j] * ((len(rows) % 5) - 2)
            y = yj + Dy * (z - z[j])                                   # at every node, in doubles
            inside = y <= hexd
            want = np.zeros(nmax + 1, dtype=bool)
            if fam == "dip":
                want[j] = delta >= 0
            else:
                want[:j + 1] = True
            lo = 0 if fam == "dip" else j
            keep = np.ones(nmax + 1, dtype=bool)
            keep[j] = delta != 0.0                                     # delta = 0: node j itself is on the edge
            if not np.array_equal((inside & keep)[lo:], (want & keep)[lo:]):
                return
            cy = float(F(float(yj)) + F(float(Dy)) * (F(float(z[nmax])) - F(float(z[j]))))
            d = np.array([0.0, Dy, 1.0])
            d /= np.sqrt(d @ d)
            rows.append([x, cy, z[nmax], d[0], d[1], d[2], 0.0])
            meta.append(dict(profile=name, fam=fam, node=j, L=L, pos=pos, delta=delta))

        seen = set()
        for j, L, pos in nodes:
            if (j, L) in seen:
                continue
            seen.add((j, L))
            sl, sr = (hexd[j] - hexd[j - 1]) / (z[j] - z[j - 1]), (hexd[j + 1] - hexd[j]) / (z[j + 1] - z[j])
            for delta in MARCH_DELTAS + (0.0, 1e-5, 1e-4):
                add("dip", j, L, pos, delta, hexd[j] * (1 - delta), 0.5 * (sl + sr))
            for delta in (1e-12, 1e-9, 1e-6, 1e-3):
                # delta ext inside at node j, as far outside at node j + 1
                add("cross", j, L, pos, delta, hexd[j] * (1 - delta), sr + 2 * delta * hexd[j] / (z[j + 1] - z[j]))
        # inside at the exit plane (here == 1) and dz < 0: literal agreement only
        for k in range(4):
            rows.append([0.1 * ext[nmax] * k, 0.2 * ext[nmax], z[nmax], 0.01, 0.02 * k, 1.0, 0.0])
            meta.append(dict(profile=name, fam="here", node=-1, L=0, pos=0, delta=0.0))
            rows.append([0.0, 1.3 * ext[0], z[nmax // 2], 0.01 * k, -0.05, -1.0, 0.0])
            meta.append(dict(profile=name, fam="down", node=-1, L=0, pos=0, delta=0.0))
        out[name] = dict(problem=march_problem(prof["z"], prof["cap"], prof["ext"], _n_cap(prof["ns"])), profile=prof,
                         rows=np.array(rows, dtype=np.float64).reshape(-1, 7), meta=meta)
    return out


# ---- HEX: points delta of a cell size inside (delta > 0) or outside (delta < 0) of each edge's middle and, along the bisector, of
# each corner; delta = 0 and +-1 ulp (the rows placed on an edge or corner on purpose) for two cells only.  A row is left out where
# doubles cannot place it (|delta| below 64 roundings of the coordinates).
HEX_ZZ = (1e-4, 1e-3, 1e-2, 0.1, 1.0)
HEX_NS = 258
HEX_CELLS = ((0, 0), (1, 0), (0, -1), (-3, 2), (77, 76), (-77, 258), (258, 0), (-258, 0), (0, -258), (129, 129), (-258, 258), (200, -258))


@functools.lru_cache(maxsize=None)
def hex_rows():
    """(rows [n, 3] = x, y, zz; meta [n])"""
    rows, meta = [], []
    for zz in HEX_ZZ:
        for q, r in HEX_CELLS:
            c = np.array([(2.0 * q + r) * C30, 1.5 * r]) * zz
            rows.append([c[0], c[1], zz])
            meta.append(dict(cell=(q, r), fam="centre", delta=1.0, k=-1))
            noise = 64 * (_ulp(max(abs(c[0]), abs(c[1]), zz)) / zz)
            on_purpose = (q, r) in ((1, 0), (-77, 258)) and zz in (1e-3, 1.0)
            for k in range(6):
                for fam, base in (("edge", C30 * _rot(60.0 * k)), ("corner", _rot(60.0 * k + 30.0))):
                    inwards = -base / np.hypot(*base)
                    for delta in MARCH_DELTAS + ((0.0, "+ulp", "-ulp") if on_purpose else ()):
                        if isinstance(delta, str):
                            p = c + base * zz
                            i = int(np.argmax(np.abs(base)))
                            p[i] = np.nextafter(p[i], np.inf if delta == "+ulp" else -np.inf)
                            dl = 0.0
                        else:
                            if delta != 0.0 and abs(delta) < noise:
                                continue
                            # outside a corner the bisector is the edge between the two neighbours: go out along edge k's normal
                            step = delta * inwards if (fam == "edge" or delta >= 0) else -delta * _rot(60.0 * k)
                            p = c + (base + step) * zz
                            dl = delta
                        rows.append([p[0], p[1], zz])
                        meta.append(dict(cell=(q, r), fam=fam, delta=dl, k=k, purpose=isinstance(delta, str) or delta == 0.0))
    return np.array(rows, dtype=np.float64).reshape(-1, 3), meta


# ---------------------------------------------------------------------------------------------------------------------------
# The flight grids (op FLIGHTS, tests/test_devmath_flights_cpu.py): photons whose flights AFTER a reflection meet the places where
# a certificate could be wrong.  Deterministic.  A later flight cannot be placed directly -- it starts where the flight before it
# ended -- so it is aimed by time reversal: the wanted flight is laid out as the _Builder families lay out a first flight, its
# ray is intersected backwards with the wall in mpmath (FLIGHT_DPS digits), mirrored there, and the earlier flight followed back to
# z = 0 or to a start inside the capillary; the start and the direction are rounded once.  What a row really does is decided by
# the exact side of the test from the P and d the probe reports for every flight, never by this file.
#
# Families (meta["fam"]):
#   aimed_end   the wanted flight starts on the wall in segment i and is delta cap from the wall at node i + L - 1, i + L, i + L + 1
#               (L = PC_L1, PC_L2; delta < 0: it has crossed the wall by |delta| cap there), as flight 1 and as flight 2
#   aimed_kink  delta cap from the wall at the kink node;  aimed_mid  parallel to the wall of one segment, delta cap from it
#   fan         from z = 0, off the axis, slopes 1e-3 ... 0.1 at eight azimuths: skew rays, which spiral from wall to wall
#   node        the first crossing on a node and 1 ulp of z either side of it (ix = i + 1; on the last node i + 1 == nmax)
#   guard       reflects eps before the node where cap_kink's wall turns inward; the second crossing lies 0.5, 1 - 1e-6, 1 + 1e-6 and 2
#               times 1e-5 beyond the first (the reference's guard drops the two nearer ones: the photon goes on outside)
#   guard0      the same four offsets on a first flight started inside the capillary
#   limit       steep photons on nmax1 and nmax4 that reach irefl > nmax
#   short       on `tiny` (cap 1e-6), started 3e-4 before a node at slopes 0.02 ... 0.1: flights of 2e-5 to 1e-4, so that flights start
#               within 1e-5 to 1e-4 of the end of their first segment and cross the wall again inside it
#   hexedge     boundary capillary of the cylinder, whose axis lies on the outer hexagon: the reflected ray passes through the axis, and
#               so meets the hexagon, at the last node but one (R / (s dz) a whole number of segments), within rounding: the march's
#               hexagon test of the ray and the literal visit's must fall on the same side, or one exits where the other ends with rc -1
FLIGHT_NB = 12
FLIGHT_K = 128
FLIGHT_DPS = 60
FLIGHT_DELTAS = tuple(d for d in MARCH_DELTAS if abs(d) >= 1e-9)
THIN_CAP = 4.0e-4
GUARD_OFFSETS = (0.5, 1 - 1e-6, 1 + 1e-6, 2.0)


def flight_profiles():
    """the 16 march profiles plus the thin variants (cap0 about 4e-4: at grazing slopes of 1e-3 to 3e-2 a photon makes 2 to 12
    flights of 3 to 40 segments within 61 segments); ext_kink (cap0 8e-4) is thin as it is"""
    P = dict(march_profiles())
    for name in ("cylinder", "taper", "bulge", "cap_kink", "irregular"):
        q = dict(P[name])
        q["cap"] = q["cap"] * (THIN_CAP / M_CAP)
        q["thin"] = True
        P[name + "_thin"] = q
    P["ext_kink"] = dict(P["ext_kink"], thin=True)
    return P


def _rot2(e, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([c * e[0] - s * e[1], s * e[0] + c * e[1]])


class _FlightBuilder(_Builder):
    """adds to _Builder the wall of one capillary in mpmath: crossings of a ray going backwards, the wall's normal, the mirror"""

    def __init__(self, name, prof):
        super().__init__(name, prof)
        from mpmath import mp, mpf
        self.mp, self.mpf = mp, mpf
        with mp.workdps(FLIGHT_DPS):
            self.mz, self.mzh, self.mcap = [mpf(float(v)) for v in self.z], [mpf(float(v)) for v in self.zh], [mpf(float(v)) for v in self.cap]

    def add(self, capname, k, fam, P, d, **meta):
        self.rows.append([float(P[0]), float(P[1]), float(P[2]), float(d[0]), float(d[1]), float(d[2]), 0.3, 0.5, 0.1, 0.0,
                          float(FLIGHT_K), float(FLIGHT_NB)])
        self.meta.append(dict(dict(profile=self.name, cap=capname, k=k, fam=fam, delta=0.0, want=0, tnode=-1, L=0, s=0.0, off=0.0), **meta))

    def centre(self, k, zv):
        return np.array(k) * self.at(self.zh, zv)

    # --- mpmath: the ray p(z) = p + D (z - zr) against segment j of capillary k
    def _quad(self, k, j, p, D, zr):
        z0, dz = self.mz[j], self.mz[j + 1] - self.mz[j]
        sl = (self.mzh[j + 1] - self.mzh[j]) / dz
        q0 = [p[c] + D[c] * (z0 - zr) - k[c] * self.mzh[j] for c in (0, 1)]
        dq = [D[c] - k[c] * sl for c in (0, 1)]
        R0, rr = self.mcap[j], (self.mcap[j + 1] - self.mcap[j]) / dz
        return dq[0] ** 2 + dq[1] ** 2 - rr * rr, 2 * (q0[0] * dq[0] + q0[1] * dq[1] - R0 * rr), q0[0] ** 2 + q0[1] ** 2 - R0 * R0, dz

    def back_cross(self, k, p, D, zr, z_from):
        """the crossing of the ray with the wall next below z_from: (z, segment, g'(z)) or None when there is none down to z = 0"""
        mp = self.mp
        j = self.seg_of(float(z_from))
        if float(z_from) <= float(self.z[j]) and j > 0:
            j -= 1
        while j >= 0:
            a, b, c, dz = self._quad(k, j, p, D, zr)
            ts = []
            if a == 0:
                if b != 0:
                    ts = [-c / b]
            else:
                disc = b * b - 4 * a * c
                if disc >= 0:
                    sq = mp.sqrt(disc)
                    ts = [(-b + sq) / (2 * a), (-b - sq) / (2 * a)]
            hi = min(dz, z_from - self.mz[j])
            ts = sorted((t for t in ts if 0 <= t <= dz and t < hi), reverse=True)
            if ts:
                return self.mz[j] + ts[0], j, 2 * a * ts[0] + b
            j -= 1
        return None

    def g_at(self, k, p, D, zr, zv):
        j = self.seg_of(float(zv))
        a, b, c, dz = self._quad(k, j, p, D, zr)
        t = zv - self.mz[j]
        return (a * t + b) * t + c

    def mirror(self, k, j, H, D):
        """xy slope of the ray that, mirrored at the wall point H of segment j, leaves along (D, 1); None when it flies backwards"""
        mp = self.mp
        dz = self.mz[j + 1] - self.mz[j]
        c0 = [k[0] * self.mzh[j], k[1] * self.mzh[j], self.mz[j]]
        cd = [k[0] * (self.mzh[j + 1] - self.mzh[j]), k[1] * (self.mzh[j + 1] - self.mzh[j]), dz]
        s3 = sum(v * v for v in cd)
        tp = sum((H[c] - c0[c]) * cd[c] for c in range(3)) / s3
        inn = [H[c] - (c0[c] + tp * cd[c]) for c in range(3)]
        il = mp.sqrt(sum(v * v for v in inn))
        tg = -(self.mcap[j + 1] - self.mcap[j]) / s3
        n = [inn[c] / il + tg * cd[c] for c in range(3)]
        nl = mp.sqrt(sum(v * v for v in n))
        n = [v / nl for v in n]
        d = [D[0], D[1], self.mpf(1)]
        nd = sum(n[c] * d[c] for c in range(3))
        di = [d[c] - 2 * nd * n[c] for c in range(3)]
        if not di[2] > 0:
            return None
        return [di[0] / di[2], di[1] / di[2]]

    def reversed_row(self, capname, k, fam, B, D, zt, want, crossed, **meta):
        """The wanted flight passes B (xy) at z = zt with xy slope D.  It is followed backwards to its start on the wall and
        through `want` mirrors in all (want = 1: it is flight 1), then to z = 0 or to the middle of the earliest flight; a row is
        dropped when a flight on the way would leave the capillary.  crossed: B lies beyond the wall (delta < 0), the first crossing
        met backwards is the wanted flight's own end."""
        mp, mpf = self.mp, self.mpf
        with mp.workdps(FLIGHT_DPS):
            km = [mpf(float(k[0])), mpf(float(k[1]))]
            p, Dm, zr = [mpf(float(B[0])), mpf(float(B[1]))], [mpf(float(D[0])), mpf(float(D[1]))], mpf(float(zt))
            z_from = zr
            if crossed:
                c = self.back_cross(km, p, Dm, zr, z_from)
                if c is None or not c[2] > 0:
                    return False
                z_from = c[0]
            elif not self.g_at(km, p, Dm, zr, zr) < 0:
                return False
            made = 0
            while True:
                c = self.back_cross(km, p, Dm, zr, z_from)
                if c is None:
                    if made == 0 or not self.g_at(km, p, Dm, zr, mpf(0)) < 0:
                        return False
                    zs = mpf(0)
                    break
                if not c[2] < 0:          # going forwards the photon would come from outside: the flight before leaves the capillary
                    return False
                if made == want:
                    zs = (c[0] + z_top) / 2
                    break
                H = [p[0] + Dm[0] * (c[0] - zr), p[1] + Dm[1] * (c[0] - zr), c[0]]
                Dn = self.mirror(km, c[1], H, Dm)
                if Dn is None:
                    return False
                p, Dm, zr, z_top = H[:2], Dn, H[2], H[2]
                z_from = zr - mpf(10) ** -9      # a crossing that close is the mirror point itself
                made += 1
            P = [float(p[0] + Dm[0] * (zs - zr)), float(p[1] + Dm[1] * (zs - zr)), float(zs)]
            d = [float(Dm[0]), float(Dm[1]), 1.0]
        self.add(capname, k, fam, P, d, want=made, **meta)
        return True


def _flight_rows_of(name, prof):
    B = _FlightBuilder(name, prof)
    nmax, z, cap = B.nmax, B.z, B.cap
    L1, L2 = 5, 25
    thin = bool(prof.get("thin"))
    small = nmax < 30
    count = 0
    for capname, q, r in march_capillaries(prof["ns"]):
        k = B.k(q, r)
        bnd = capname == "boundary"
        e = B.radial(capname, k)
        # where on the wall a flight ends (eB) and starts (eA): opposite ends of a diameter; on a boundary capillary, whose outer half
        # lies outside the optic, the two ends of a chord on its inner half (a skew ray)
        eB, eA = (_rot2(e, 50.0), _rot2(e, -50.0)) if bnd else (e, -e)
        inward = e * (0.5 if bnd else 0.0)

        def wall_pt(zv, ev, f=1.0):
            return B.centre(k, zv) + ev * (B.at(cap, zv) * f)

        # ---- aimed: end, kink, mid
        if not small and name not in ("tiny", "last_zero"):
            for L, i_s in ((L1, 22), (L2, 30)):
                for off in (-1, 0, 1):
                    t = i_s + L + off
                    if t > nmax:
                        continue
                    zA = 0.5 * (z[i_s] + z[i_s + 1])
                    for delta in FLIGHT_DELTAS:
                        Bp = wall_pt(z[t], eB, 1 - delta)
                        D = (Bp - wall_pt(zA, eA)) / (z[t] - zA)
                        for want in (1, 2):
                            B.reversed_row(capname, k, "aimed_end", Bp, D, z[t], want, delta < 0, delta=delta, tnode=t, L=L)
            if prof["kink"] is not None and not (name == "ext_kink" and capname == "centre"):
                kn = prof["kink"]
                for i_s in (kn - 6, kn - 20):
                    zA = 0.5 * (z[i_s] + z[i_s + 1])
                    for delta in FLIGHT_DELTAS:
                        Bp = wall_pt(z[kn], eB, 1 - delta)
                        D = (Bp - wall_pt(zA, eA)) / (z[kn] - zA)
                        for want in (1, 2):
                            B.reversed_row(capname, k, "aimed_kink", Bp, D, z[kn], want, delta < 0, delta=delta, tnode=kn, L=kn - i_s)
            for js in (40, 48):
                zt = 0.5 * (z[js] + z[js + 1])
                w = (cap[js + 1] - cap[js]) / (z[js + 1] - z[js])
                for delta in FLIGHT_DELTAS:
                    if delta > 0:
                        D = B.axis_slope(k, js) + w * eB
                        for want in (1, 2):
                            B.reversed_row(capname, k, "aimed_mid", wall_pt(zt, eB, 1 - delta), D, zt, want, False, delta=delta, tnode=js)
        # ---- fan
        if name in ("nmax1", "nmax4"):
            slopes, fam = (0.3, 1.5, 2.5, 4.0), "limit"
        elif name == "tiny":
            slopes, fam = (1e-5, 1e-4, 1e-3), "fan"
        else:
            slopes, fam = ((1e-3, 3e-3, 1e-2, 3e-2, 0.1) if thin else (2e-2, 5e-2, 0.1)), "fan"
        P0 = B.centre(k, 0.0) + inward * cap[0] + 0.4 * cap[0] * _rot2(e, 35.0) * (0.5 if bnd else 1.0)
        for s in slopes:
            for a in range(8):
                u = _rot2(e, 45.0 * a + 10.0)
                D = B.axis_slope(k, 0) + s * u
                B.add(capname, k, fam, [P0[0], P0[1], 0.0], [D[0], D[1], 1.0], s=s)
        # ---- node: the first crossing on a node and 1 ulp of z either side of it
        if name in ("cylinder", "taper", "irregular", "last_zero", "nmax6", "nmax25", "nmax26", "cylinder_thin", "mono"):
            F = B.F
            nodes = sorted(set(t for t in (3, nmax - 1, nmax, 33, 40, 47, 54) if 1 <= t <= nmax and cap[t] > 0))
            for t in nodes:
                for s in ((3e-3, 1e-2) if thin else (5e-2, 0.1)):
                    for du in (-1, 0, 1):
                        zw = float(z[t]) + du * _ulp(z[t])
                        Rw = F(B.at(cap, z[t]))
                        back = min(float(zw), 0.6 * float(Rw) / s)
                        zs = float(zw - back)
                        ct, cs = B.centre(k, zw), B.centre(k, zs)
                        W = [F(float(ct[c])) + F(float(eB[c])) * Rw for c in (0, 1)]
                        Dx = [F(float(eB[c])) * F(s) + F(float((ct[c] - cs[c]) / back)) for c in (0, 1)]
                        P = [float(W[c] - Dx[c] * (F(zw) - F(zs))) for c in (0, 1)] + [zs]
                        B.add(capname, k, "node", P, [float(Dx[0]), float(Dx[1]), 1.0], tnode=t, s=s, off=float(du))
        # ---- short
        if name == "tiny":
            for t in (3, 40):
                zs = float(z[t]) - 3.0e-4
                Ps = B.centre(k, zs) + inward * B.at(cap, zs) + 0.3 * B.at(cap, zs) * _rot2(e, 35.0) * (0.5 if bnd else 1.0)
                for s in (0.02, 0.05, 0.1):
                    for a in range(8):
                        D = B.axis_slope(k, t - 1) + s * _rot2(e, 45.0 * a + 10.0)
                        B.add(capname, k, "short", [Ps[0], Ps[1], zs], [D[0], D[1], 1.0], s=s, tnode=t)
        # ---- hexedge
        if name == "cylinder" and bnd:
            F = B.F
            for nseg, s in ((2, 0.25), (4, 0.125), (5, 0.1), (8, 0.0625), (10, 0.05), (20, 0.025)):
                t = nmax - 1 - nseg
                for ang in np.linspace(-80.0, 80.0, 17):
                    ev = _rot2(e, float(ang))
                    for du in (-1, 0, 1):
                        zw = float(z[t]) + du * _ulp(z[t])
                        Rw = F(float(cap[t]))
                        zs = zw - 0.6 * float(Rw) / s
                        ct = B.centre(k, z[t])
                        W = [F(float(ct[c])) + F(float(ev[c])) * Rw for c in (0, 1)]
                        Dx = [F(float(ev[c])) * F(s) for c in (0, 1)]
                        P = [float(W[c] - Dx[c] * (F(zw) - F(zs))) for c in (0, 1)] + [zs]
                        B.add(capname, k, "hexedge", P, [float(Dx[0]), float(Dx[1]), 1.0], tnode=t, s=s, off=float(du))
        # ---- guard, guard0 (cap_kink: cylinder up to node kink - 1, where the wall turns inward)
        if name in ("cap_kink", "cap_kink_thin"):
            F = B.F
            kn = prof["kink"]
            zk = F(float(z[kn - 1]))
            R = F(float(cap[kn - 1]))
            w = (R - F(float(cap[kn]))) / (F(float(z[kn])) - zk)          # the wall's inward slope beyond the node
            ex = [F(float(eB[0])), F(float(eB[1]))]
            cx = [F(float(v)) for v in B.centre(k, z[kn - 1])]            # zh is constant on cap_kink: the axis is parallel to z
            for sf in (0.1, 0.3, 0.6):
                s = F(float(w)) * F(sf)
                for offv in GUARD_OFFSETS:
                    # guard: reflected at zr = zk - eps it closes in at slope s; the wall comes in at w from zk on: they meet
                    # eps w / (w - s) beyond zr
                    eps = F(offv) * F(1.0e-5) * (w - s) / w
                    zr = zk - eps
                    back = R / s / 2
                    P = [cx[c] + ex[c] * (R - s * back) for c in (0, 1)] + [zr - back]
                    B.add(capname, k, "guard", P, [float(ex[0] * s), float(ex[1] * s), 1.0], s=float(s), off=offv, tnode=kn - 1)
                    # guard0: starts inside, s off 1e-5 from the wall, flying outwards at slope s, mid-segment and across a node
                    for zs in (F(float(0.5 * (z[10] + z[11]))), F(float(z[12])) - F(offv) * F(1.0e-5) / 2):
                        gap = s * F(offv) * F(1.0e-5)
                        P = [cx[c] + ex[c] * (R - gap) for c in (0, 1)] + [zs]
                        B.add(capname, k, "guard0", P, [float(ex[0] * s), float(ex[1] * s), 1.0], s=float(s), off=offv)
    return np.array(B.rows, dtype=np.float64).reshape(-1, 12), B.meta


@functools.lru_cache(maxsize=None)
def flight_grids():
    """name -> dict(problem, profile, rows [n, 12] of pyprobe.FLIGHTS_COLS (literal 0, K = FLIGHT_K, NB = FLIGHT_NB), meta [n])"""
    out = {}
    for name, prof in flight_profiles().items():
        rows, meta = _flight_rows_of(name, prof)
        out[name] = dict(problem=march_problem(prof["z"], prof["cap"], prof["ext"], _n_cap(prof["ns"])), profile=prof, rows=rows,
                         meta=meta)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The grids of a photon's two ends (ops SINCOS, UNIFORM, ENTER, EXIT and the sampler; tests/test_devmath_ends_cpu.py).
# Deterministic; the only random draws are the Philox streams themselves.  What a row really is -- which side of a boundary, how far
# from it -- is decided by the exact side (tests/devmath/exact.py), never by this file.
SINCOS_WORST = (0.793567278060035, 1.0650241763598487)      # the largest sine and cosine errors found on 300 000 points


@functools.lru_cache(maxsize=None)
def sincos_points():
    """the arguments of op SINCOS: 0, the smallest subnormal, 2^-1022, 2^-27, 2^-26; pi/4 +- k 2^-53 for k <= 40; the 60 doubles
    below pi/2 in steps of 2^-52; 2 pi (k / 2^53) / 4 as the sampler forms it for k in {0, 1, 2^51, 2^52 +- 1, 2^53 - 1}; 20 000
    points of a fixed lattice in [0, pi/2]; 5 000 log-spaced points in [1e-12, 1]; the two worst points known"""
    pio4, pio2 = 0.78539816339744830962, 1.57079632679489655800
    x = [0.0, 2.0 ** -1074, 2.0 ** -1022, 2.0 ** -27, 2.0 ** -26]
    x += [pio4 + k * 2.0 ** -53 for k in range(-40, 41)]
    x += [pio2 - k * 2.0 ** -52 for k in range(1, 61)]
    x += [2.0 * math.pi * (k / 2.0 ** 53) / 4. for k in (0, 1, 2 ** 51, 2 ** 52 - 1, 2 ** 52 + 1, 2 ** 53 - 1)]
    x += list((np.arange(20000) + 0.5) * (pio2 / 20000))
    x += list(10.0 ** np.linspace(-12, 0, 5000))
    x += list(SINCOS_WORST)
    return np.array(x, dtype=np.float64)


UNIFORM_SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 0x0123456789abcdef)
UNIFORM_SLOTS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 5, 2 ** 63 - 1)
UNIFORM_ATTEMPTS = (0, 1, 2 ** 32 - 1)
UNIFORM_D = (0, 1, 2, 3, 4094, 4095)


@functools.lru_cache(maxsize=None)
def uniform_streams():
    """every (seed, slot, attempt, d) of op UNIFORM, Python integers"""
    return tuple((s, t, a, d) for s in UNIFORM_SEEDS for t in UNIFORM_SLOTS for a in UNIFORM_ATTEMPTS for d in UNIFORM_D)


SAMPLER_SEED = 424242
SAMPLER_SLOTS = tuple(range(1496)) + (2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5, 2 ** 62 + 1)
# name -> (optic, source, attempt); generic: the elliptical source, sampled through libm (not bit for bit between device and host)
SAMPLER_CASES = dict(
    xos1=("xos1", (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0), 3),
    divergent=("ellip", (0.05, 0.1, 0.1, 0.2, 0.2, 0., 0., 0.5), 3),
    elliptical=("ellip", (2000., 0.2065, 0.1, 0., 0., 0.01, -0.02, 0.9), 3),
    uniform=("ellip", (5., 0.01, 0.01, -1., 0., 0., 0., 0.0), 3),
    mono=("MONO_CASE", None, 3),
    seven=("SEVEN_CASE", None, 3),
    ecc_flat=("ellip", (2000., 0.2, 0.2e-3, 0., 0., 0., 0., 0.5), 3),
    ecc_tall=("ellip", (2000., 0.2e-3, 0.2, 0., 0., 0., 0., 0.5), 3),
    pol_minus=("ellip", (2000., 0.2065, 0.2065, 0., 0., 0., 0., -1.0), 3),
    pol_zero=("ellip", (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0), 3),
    pol_plus=("ellip", (2000., 0.2065, 0.2065, 0., 0., 0., 0., 1.0), 3),
    last_attempt=("xos1", (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0), 2 ** 32 - 1),
)
SAMPLER_GENERIC = ("elliptical", "ecc_flat", "ecc_tall")


@functools.lru_cache(maxsize=None)
def sampler_case(name):
    """dict(optic, src (the oracle's), problem, source (the 8 doubles), attempt, mono, cap0, ext0)"""
    from oracle import pyoracle
    from tests import common
    pyoracle.build()
    which, source, attempt = SAMPLER_CASES[name]
    if which in ("MONO_CASE", "SEVEN_CASE"):
        c = getattr(common, which)
        optic, src, prob, _ = common.make_custom(pyoracle, c["shape"], c["n_cap"], c["source"])
        source = c["source"]
    else:
        optic, src, prob, _ = common.make_pair(pyoracle, which, source=source)
    ns = round(math.sqrt(12. * prob.n_cap - 3.) / 6. - 0.5)
    return dict(optic=optic, src=src, problem=prob, source=tuple(float(v) for v in source), attempt=attempt, mono=(ns == 0),
                cap0=float(prob.cap[0]), ext0=float(prob.ext[0]))


ENTER_PROFILES = ("taper", "ext_kink", "irregular", "tiny", "bulge", "mono", "nmax1")
ENTER_OFFSETS = (0.0, 1.0, -1.0, 3.0, -3.0, 1e5, -1e5)                      # wall, cell: units of the spacing of the doubles at the scale
ENTER_HEX_OFFSETS = (0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 1e5, -1e5)       # hexedge, hexcorner
ENTER_NORMS = (1e-3, 1.0, 1.0 - 2.0 ** -52, 1.0 + 2.0 ** -52, 1e3)
ENTER_D = (1.5e-3, -2.5e-3, 1.0)
ENTER_E = (0.3, -0.9, 0.2)
# Families (meta["fam"]): wall (150 capillaries per height, a point on the circle at ENTER_OFFSETS), cell (edges and corners of 6
# cells), hexedge / hexcorner (the outer hexagon; the circle of the mono-capillary), axis (the 150 centres), norms (40 interior points
# per height with |d| and |E| through ENTER_NORMS: 25 rows each, all decided -- with them the rows put inside a band on purpose, 5 of
# the 7 wall offsets, stay below the 45 % the test allows).
ENTER_CELLS, ENTER_NORM_CELLS, ENTER_EDGE_CELLS = 150, 40, 6
GOLDEN_ANGLE = 2.399963229728653


def enter_z(z):
    """the ten start heights of a profile: 0; node 1 and half of it; node 5 and its two neighbour doubles; node nmax - 1; the
    middle of the last segment; z[nmax] and the double below it (fewer where the profile has fewer nodes)"""
    n = len(z) - 1
    c = [0.0, float(z[1]), 0.5 * float(z[1])]
    if n >= 6:
        c += [float(z[5]), float(np.nextafter(z[5], 0.0)), float(np.nextafter(z[5], np.inf))]
    c += [float(z[n - 1]), 0.5 * (float(z[n - 1]) + float(z[n])), float(z[n]), float(np.nextafter(z[n], 0.0))]
    out = []
    for v in c:
        if v not in out:
            out.append(v)
    return out


def _ring_cell(ring, pos):
    dirs = ((1, 0), (1, -1), (0, -1), (-1, 0), (-1, 1), (0, 1))
    q, r = dirs[4][0] * ring, dirs[4][1] * ring
    k = 0
    for side in range(6):
        for _ in range(ring):
            if k == pos:
                return q, r
            q, r = q + dirs[side][0], r + dirs[side][1]
            k += 1
    return q, r


def enter_cells(ns, n=ENTER_CELLS):
    """n capillaries (q, r) of an optic of ns shells: the centre, the six corners of the outermost shell (q or r = +-ns), and a
    fixed lattice over the shells"""
    if ns == 0:
        return [(0, 0)]
    cells = [(0, 0), (ns, 0), (-ns, 0), (0, ns), (0, -ns), (ns, -ns), (-ns, ns)]
    k = 0
    while len(cells) < n:
        ring = 1 + int((ns - 0.001) * math.sqrt((k % 97 + 0.5) / 97))
        c = _ring_cell(ring, (k * 7919) % (6 * ring))
        if c not in cells:
            cells.append(c)
        k += 1
    return cells


def _enter_rows_of(name, prof):
    F = exact.Fraction
    z, cap, ext, ns = prof["z"], prof["cap"], prof["ext"], prof["ns"]
    P = exact.entrance_profile(z, cap, ext)
    nmax = len(z) - 1
    C = exact.COSPI_6
    rows, meta = [], []

    def put(fam, x, y, zv, d=ENTER_D, E=ENTER_E, **kw):
        rows.append((x, y, zv) + tuple(d) + tuple(E))
        meta.append(dict(fam=fam, **kw))

    cells = enter_cells(ns)
    for zi, zv in enumerate(enter_z(z)):
        j = 0
        if zv > 0:
            j = min(max(0, int(np.searchsorted(z, zv, side="right")) - 1), nmax - 1)
        t = (F(zv) - P["z"][j]) / (P["z"][j + 1] - P["z"][j])
        e = float(P["ext"][j] + (P["ext"][j + 1] - P["ext"][j]) * t)
        rad = float(P["cap"][j] + (P["cap"][j + 1] - P["cap"][j]) * t)
        hs = float(2 * C * (ns + 1))
        zz = e / hs

        def centre(q, r):
            return float((2 * q + r) * C) * zz, 1.5 * r * zz

        for ci, (q, r) in enumerate(cells if ns else [(0, 0)] * ENTER_CELLS):
            cx, cy = centre(q, r)
            sc = float(np.spacing(max(abs(cx) + rad, abs(cy) + rad, e)))
            a = (0.0, 0.5 * math.pi)[ci] if ci < 2 else 0.7 + GOLDEN_ANGLE * (ci + 17 * zi)
            for k in ENTER_OFFSETS:
                put("wall", cx + (rad + k * sc) * math.cos(a), cy + (rad + k * sc) * math.sin(a), zv, cell=(q, r), off=k)
            if ns or ci == 0:
                put("axis", cx, cy, zv, cell=(q, r), off=None)
            if ci < ENTER_NORM_CELLS:
                px, py = cx + 0.3 * rad * math.cos(a), cy + 0.3 * rad * math.sin(a)
                for nd in ENTER_NORMS:
                    for ne in ENTER_NORMS:
                        dn, en = math.sqrt(sum(v * v for v in ENTER_D)), math.sqrt(sum(v * v for v in ENTER_E))
                        put("norms", px, py, zv, d=[v / dn * nd for v in ENTER_D], E=[v / en * ne for v in ENTER_E], cell=(q, r), off=None)
            if ns and (ci == 0 or 7 <= ci < 6 + ENTER_EDGE_CELLS):
                for k in ENTER_OFFSETS:
                    for ed in range(3):
                        b = math.radians(60 * ed)
                        put("cell", cx + (float(C) * zz + k * sc) * math.cos(b), cy + (float(C) * zz + k * sc) * math.sin(b), zv, cell=(q, r), off=k, at="edge")
                    for co in range(2):
                        b = math.radians(30 + 60 * co)
                        put("cell", cx + (zz + k * sc) * math.cos(b), cy + (zz + k * sc) * math.sin(b), zv, cell=(q, r), off=k, at="corner")
        sc = float(np.spacing(e))
        for k in ENTER_HEX_OFFSETS:
            if ns == 0:
                for m in range(30):
                    a = 0.3 + GOLDEN_ANGLE * m if m >= 2 else (0.0, 0.5 * math.pi)[m]
                    put("hexedge", (e + k * sc) * math.cos(a), (e + k * sc) * math.sin(a), zv, off=k)
                continue
            inr = math.sqrt(3.0) / 2 * e
            for ed in range(6):
                b = math.radians(30 + 60 * ed)
                for s in (-0.8, -0.45, -0.1, 0.3, 0.7):
                    put("hexedge", (inr + k * sc) * math.cos(b) - s * 0.5 * e * math.sin(b), (inr + k * sc) * math.sin(b) + s * 0.5 * e * math.cos(b), zv, off=k)
                b = math.radians(60 * ed)
                put("hexcorner", (e + k * sc) * math.cos(b), (e + k * sc) * math.sin(b), zv, off=k)
    # the first row of every profile flies along the axis with an electric vector of length exactly 1 (pc_launch_init divides E by
    # its length only where that is not 1)
    rows[0] = rows[0][:3] + (0.0, 0.0, 1.0, 1.0, 0.0, 0.0)
    return np.array(rows, dtype=np.float64), meta


@functools.lru_cache(maxsize=None)
def enter_grids():
    """name -> dict(problem, profile, rows [n, 9] of pyprobe.ENTER_COLS, meta [n])"""
    out = {}
    profs = march_profiles()
    for name in ENTER_PROFILES:
        prof = profs[name]
        rows, meta = _enter_rows_of(name, prof)
        out[name] = dict(problem=march_problem(prof["z"], prof["cap"], prof["ext"], _n_cap(prof["ns"])), profile=prof, rows=rows, meta=meta)
    return out


EXIT_OFFSETS = ENTER_OFFSETS + (1e7, -1e7, 1e9, -1e9, 1e11, -1e11)
EXIT_DZ = (1.0, 1e-2, 1e-8)


def _exit_rows_of(name, prof):
    z, ext, ns = prof["z"], prof["ext"], prof["ns"]
    nmax = len(z) - 1
    ze, e = float(z[nmax]), float(ext[nmax])
    rows, meta = [], []
    pz = []
    for v in [float(z[max(0, nmax - k)]) for k in (3, 2, 1)] + [ze]:
        if v not in pz:
            pz.append(v)
    targets = []
    if ns == 0:
        for m in range(24):
            a = 0.3 + GOLDEN_ANGLE * m if m >= 2 else (0.0, 0.5 * math.pi)[m]
            targets.append(("circle", math.cos(a), math.sin(a), e))
    else:
        inr = math.sqrt(3.0) / 2 * e
        for ed in range(6):
            b = math.radians(30 + 60 * ed)
            for s in (-0.7, 0.0, 0.45):
                targets.append(("edge", math.cos(b), math.sin(b), inr, -s * 0.5 * e * math.sin(b), s * 0.5 * e * math.cos(b)))
            b = math.radians(60 * ed)
            targets.append(("corner", math.cos(b), math.sin(b), e))
    sc = float(np.spacing(e))
    for Pz in pz:
        for Pxy in ((0.0, 0.0), (0.3 * e, -0.2 * e)):
            for tg in targets:
                for k in EXIT_OFFSETS:
                    tx = (tg[3] + k * sc) * tg[1] + (tg[4] if len(tg) > 4 else 0.0)
                    ty = (tg[3] + k * sc) * tg[2] + (tg[5] if len(tg) > 4 else 0.0)
                    for dz in EXIT_DZ:
                        if Pz == ze:
                            if Pxy != (0.0, 0.0):
                                continue
                            rows.append((tx, ty, Pz, 1e-3 * dz, 2e-3 * dz, dz))
                        else:
                            L = ze - Pz
                            rows.append((Pxy[0], Pxy[1], Pz, (tx - Pxy[0]) / L * dz, (ty - Pxy[1]) / L * dz, dz))
                        meta.append(dict(fam=tg[0], off=k, dz=dz, t0=(Pz == ze)))
    return np.array(rows, dtype=np.float64), meta


@functools.lru_cache(maxsize=None)
def exit_grids():
    """name -> dict(problem, profile, rows [n, 6] of pyprobe.EXIT_COLS, meta [n]): photons on the last three nodes and at z_end
    itself, aimed at the exit hexagon's edges and corners (the circle for the mono-capillary)"""
    out = {}
    profs = march_profiles()
    for name in ENTER_PROFILES:
        prof = profs[name]
        rows, meta = _exit_rows_of(name, prof)
        out[name] = dict(problem=enter_grids()[name]["problem"], profile=prof, rows=rows, meta=meta)
    return out

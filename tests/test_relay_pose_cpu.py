"""Posed relays without a GPU (a tilted second optic; include/polycap-hip.h, pc_hip_pose_*): the basis of a pose against mpmath, the
per-photon arithmetic of pc_relay.h compiled for the host (tests/relay_pose/relay_pose_host.cpp) against a numpy restatement of the
contract bit for bit and against mpmath for its geometry, the zero-tilt dispatch, the two `missed` conditions at their edges, the
pose check, and the exported symbols."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_relay_cpu import build_relay_host, host_fly

HIPD = os.path.join(ROOT, "polycap_amd", "csrc", "hip")
HERE = os.path.join(ROOT, "tests", "relay_pose")
NEW_SYMBOLS = ("pc_hip_pose_basis", "pc_hip_pose_counts", "pc_hip_pose_run", "pc_hip_pose_validate")
ULP1 = 2.0 ** -52                       # an ulp of 1


# ---- the contract, restated ---------------------------------------------------------------------------------------------------
def np_fly_posed(x, y, dx, dy, ex, ey, gap, off_x, off_y, basis):
    """(out [n, 10] = start (3), direction (3), electric vector (3), flight t; hit [n]): every operation one IEEE fp64 numpy
    operation, in the contract's order; the rows of missed photons are zero"""
    f = np.float64
    u0, u1, u2, v0, v1, v2, n0, n1, n2 = (f(b) for b in basis)
    gap, off_x, off_y = f(gap), f(off_x), f(off_y)
    with np.errstate(all="ignore"):
        dz = np.sqrt((f(1.) - dx * dx) - dy * dy)
        ez = -(ex * dx + ey * dy) / dz
        nd = (n0 * dx + n1 * dy) + n2 * dz
        npl = (n0 * (off_x - x) + n1 * (off_y - y)) + n2 * gap
        hit = (nd > 0.) & (npl >= 0.)
        t = npl / nd
        r0, r1, r2 = (x + dx * t) - off_x, (y + dy * t) - off_y, dz * t - gap
        out = np.stack([(u0 * r0 + u1 * r1) + u2 * r2, (v0 * r0 + v1 * r1) + v2 * r2, np.zeros_like(r0),
                        (u0 * dx + u1 * dy) + u2 * dz, (v0 * dx + v1 * dy) + v2 * dz, nd,
                        (u0 * ex + u1 * ey) + u2 * ez, (v0 * ex + v1 * ey) + v2 * ez, (n0 * ex + n1 * ey) + n2 * ez, t], axis=1)
    out[~hit] = 0.
    return out, hit


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64).ravel(), np.ascontiguousarray(b, dtype=np.float64).ravel()
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))))


# ---- the host compile ---------------------------------------------------------------------------------------------------------
def build_pose_host(directory):
    so = os.path.join(str(directory), "relay_pose_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", HIPD,
                           os.path.join(HERE, "relay_pose_host.cpp"), "-o", so])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.relay_fly_posed_n.restype = None
    L.relay_fly_posed_n.argtypes = [C.c_int64, dp, C.c_double, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_int32)]
    L.relay_pose_basis.restype = None
    L.relay_pose_basis.argtypes = [C.c_double, C.c_double, dp]
    L.relay_pose_ok.restype = C.c_int
    L.relay_pose_ok.argtypes = [C.c_double] * 5
    L.relay_pose_plain.restype = C.c_int
    L.relay_pose_plain.argtypes = [C.c_double, C.c_double, C.c_int]
    return L


def host_fly_posed(L, six, gap, off_x, off_y, basis):
    """six [n, 6] = x, y, dx, dy, ex, ey -> (out [n, 10], zero rows for missed photons; hit [n] bool)"""
    a = np.ascontiguousarray(six, dtype=np.float64)
    b = np.ascontiguousarray(basis, dtype=np.float64)
    out = np.zeros((a.shape[0], 10))
    hit = np.zeros(a.shape[0], dtype=np.int32)
    dp = C.POINTER(C.c_double)
    L.relay_fly_posed_n(a.shape[0], a.ctypes.data_as(dp), gap, off_x, off_y, b.ctypes.data_as(dp), out.ctypes.data_as(dp),
                        hit.ctypes.data_as(C.POINTER(C.c_int32)))
    return out, hit != 0


@pytest.fixture(scope="module")
def pose_host(tmp_path_factory):
    return build_pose_host(tmp_path_factory.mktemp("relay_pose_host"))


@pytest.fixture(scope="module")
def relay_host(tmp_path_factory):
    return build_relay_host(tmp_path_factory.mktemp("relay_host"))


def basis_of(tilt):
    import polycap_amd
    return polycap_amd.relay_basis(1.0, (0., 0.), tilt)


def _beam(n, rng):
    """x, y, dx, dy, ex, ey with the ranges of a real exit beam: |dx|, |dy| up to 0.2, positions up to 0.5 cm, any electric vector"""
    a = np.zeros((n, 6))
    a[:, 0:2] = rng.uniform(-0.5, 0.5, (n, 2))
    a[:, 2:4] = rng.uniform(-0.2, 0.2, (n, 2))
    a[:, 4:6] = rng.normal(0., 1., (n, 2))
    return a


#         gap, off_x, off_y, tilt_x, tilt_y
POSES = [(1.0, 0., 0., 0.002, 0.), (1.0, 0., 0., 0., -0.005), (1.0, 0.002, 0., 0.003, 0.001), (0.5, -0.01, 0.02, 0.3, -0.2),
         (0.05, 0.1, 0., 1.5, 0.), (0.02, 0., -0.05, -1.45, 1.2), (0., 0., 0., 0.01, 0.01), (123.456, -3.25, 1e-9, -0.7, 0.9)]
TILT_GRID = [-1.5, -1.2, -0.7, -0.3, -0.01, -1e-9, 0., 3e-6, 0.002, 0.1, 0.5, 0.785, 1.0, 1.3, 1.5]


# ---- 1. the basis ---------------------------------------------------------------------------------------------------------------
def test_basis_identity_signs_and_host_compile(pose_host):
    b = basis_of((0., 0.))
    assert same_bits(b, np.eye(3).ravel()), b                     # the identity bit for bit: no minus sign on a zero
    assert np.array_equal(basis_of((-0., -0.)), np.eye(3).ravel())      # sin(-0) = -0: the identity in value
    for tx in (1e-9, 0.003, 0.7, 1.5):
        for ty in (-1.5, -0.003, 0., 0.002, 1.2):
            assert basis_of((tx, ty))[6] > 0. and basis_of((-tx, ty))[6] < 0.          # a positive tilt_x turns the axis towards +x
            if ty:
                assert math.copysign(1., basis_of((tx, ty))[7]) == math.copysign(1., ty)      # and a positive tilt_y towards +y
                assert math.copysign(1., basis_of((0., ty))[7]) == math.copysign(1., ty)
    got = np.zeros(9)
    for tx in TILT_GRID:
        for ty in TILT_GRID:
            pose_host.relay_pose_basis(tx, ty, got.ctypes.data_as(C.POINTER(C.c_double)))
            assert same_bits(got, basis_of((tx, ty))), (tx, ty)       # the library returns what the header computes


def test_basis_against_mpmath():
    """Every entry of the basis against the header's expression evaluated by mpmath at 50 digits, on a grid of tilts in [-1.5, 1.5]:
    within 4 ulp of 1.  An entry is at most one product of two of sin, cos (each below 1 in size, glibc's within 1 ulp of the
    true value) and a subtraction from 0, which is exact: 1 + 1 ulp from the factors, half an ulp from the product, so 2.5 ulp of 1
    at the most.  Measured on this grid with glibc: 0.57 ulp of 1 (Gram matrix: 1.2).  From that the Gram matrix of u, v, n as stored (evaluated
    exactly) is the identity within 6 entry errors per dot product, 24 ulp, and the second order: 32 ulp is asserted."""
    import mpmath as mp
    mp.mp.dps = 50
    worst, worst_gram = 0., 0.
    for tx in TILT_GRID:
        for ty in TILT_GRID:
            b = basis_of((tx, ty))
            sx, cx, sy, cy = mp.sin(mp.mpf(tx)), mp.cos(mp.mpf(tx)), mp.sin(mp.mpf(ty)), mp.cos(mp.mpf(ty))
            want = [cx, 0, -sx, -sx * sy, cy, -cx * sy, sx * cy, sy, cx * cy]
            worst = max(worst, max(float(abs(mp.mpf(float(g)) - w)) for g, w in zip(b, want)))
            m = mp.matrix(3, 3)
            for k in range(9):
                m[k // 3, k % 3] = mp.mpf(float(b[k]))
            g = m * m.T - mp.eye(3)
            worst_gram = max(worst_gram, max(float(abs(g[i, j])) for i in range(3) for j in range(3)))
    print("basis: largest entry error %.3g ulp of 1, largest Gram error %.3g ulp of 1" % (worst / ULP1, worst_gram / ULP1))
    assert worst <= 4. * ULP1
    assert worst_gram <= 32. * ULP1


# ---- 2. the arithmetic ----------------------------------------------------------------------------------------------------------
def test_fly_posed_is_the_contract_bit_for_bit(pose_host):
    rng = np.random.default_rng(20241)
    a = _beam(100000, rng)
    seen = set()
    for gap, ox, oy, tx, ty in POSES:
        b = basis_of((tx, ty))
        got, hit = host_fly_posed(pose_host, a, gap, ox, oy, b)
        want, hit_w = np_fly_posed(*(a[:, k] for k in range(6)), gap, ox, oy, b)
        assert np.array_equal(hit, hit_w), (gap, ox, oy, tx, ty)
        assert same_bits(got, want), (gap, ox, oy, tx, ty)
        assert not got[:, 2].any() and np.all(got[hit, 5] > 0.)
        seen.add((bool(hit.all()), bool(hit.any())))
        print((gap, ox, oy, tx, ty), "hit", int(hit.sum()), "of", len(hit))
    assert (True, True) in seen and (False, True) in seen          # poses that take every photon, and poses that miss some


def test_fly_posed_geometry_against_mpmath(pose_host):
    """2000 photons of the beam at the poses with tilts up to 0.3 rad, where nd >= cos(0.3) * 0.96 - 0.2 * 0.42 > 0.8 is far from its
    cancellation, against the exact geometry in mpmath (50 digits) of the inputs as stored -- the records and the nine basis numbers:
    the start point lies in B's entrance plane and is the exact intersection, |direction| = 1, direction . elecv = 0, |elecv| is its
    norm in A's frame.  Each within a relative 64 ulp of the scale of what was added: S = the largest of |c|, |p + d t| and 1 for
    the points, 1 for the direction, |e| for the electric vector.  The count: the longest chain is dz (3 roundings), np (5), t (1),
    r (2), the dot product (5): 16 roundings of half an ulp each of an intermediate no larger than sqrt(3) S (three terms with
    |u0| + |u1| + |u2| <= sqrt(3)), t amplified by 1 / nd <= 1.25: 16 * 0.5 * 1.73 * 1.25 = 17 ulp; the basis entries add 4 ulp each
    (test_basis_against_mpmath) in three terms: 12 ulp; together 29, and 64 leaves a factor of two."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(7)
    a = _beam(2000, rng)
    worst = [0., 0., 0., 0., 0.]
    for gap, ox, oy, tx, ty in [p for p in POSES if max(abs(p[3]), abs(p[4])) <= 0.3]:
        b = basis_of((tx, ty))
        got, hit = host_fly_posed(pose_host, a, gap, ox, oy, b)
        assert hit.sum() > 500           # (gap 0 puts half of the beam behind a tilted plane)
        U, V, Nn = (mp.matrix([mp.mpf(float(v)) for v in b[3 * k:3 * k + 3]]) for k in range(3))
        c = mp.matrix([mp.mpf(ox), mp.mpf(oy), mp.mpf(gap)])
        dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
        for i in np.flatnonzero(hit):
            x, y, dx, dy, ex, ey = (mp.mpf(float(v)) for v in a[i])
            dz = mp.sqrt(1 - dx * dx - dy * dy)
            ez = -(ex * dx + ey * dy) / dz
            p, d, e = mp.matrix([x, y, 0]), mp.matrix([dx, dy, dz]), mp.matrix([ex, ey, ez])
            t = dot(Nn, c - p) / dot(Nn, d)
            hitp = p + d * t
            S = max(mp.norm(c), mp.norm(hitp), 1)
            o = [mp.mpf(float(v)) for v in got[i]]
            # the point the computed flight t reaches, measured along B's axis: in the plane
            r_t = p + d * o[9] - c
            worst[0] = max(worst[0], float(abs(dot(Nn, r_t)) / S))
            # the start against the exact intersection, in B's coordinates
            worst[1] = max(worst[1], float(max(abs(o[0] - dot(U, hitp - c)), abs(o[1] - dot(V, hitp - c))) / S))
            dB, eB = mp.matrix(o[3:6]), mp.matrix(o[6:9])
            worst[2] = max(worst[2], float(abs(mp.norm(dB) - 1)))
            worst[3] = max(worst[3], float(abs(dot(dB, eB)) / mp.norm(e)))
            worst[4] = max(worst[4], float(abs(mp.norm(eB) - mp.norm(e)) / mp.norm(e)))
    print("in plane, start, |d| - 1, d.e, |e|: %s ulp" % ", ".join("%.3g" % (w / ULP1) for w in worst))
    assert max(worst) <= 64. * ULP1, worst


# ---- 3. zero tilt ---------------------------------------------------------------------------------------------------------------
def test_zero_tilt_is_the_plain_relay(pose_host, relay_host):
    """The general form with the identity basis gives pc_relay_fly's numbers, the sign of a zero apart (0 * dy + dx turns -0 into
    +0), which is why a pose without tilt and without a selection is dispatched to pc_relay_fly: the dispatch is pinned here."""
    rng = np.random.default_rng(3)
    a = _beam(100000, rng)
    a[:100, 2] = -0.
    a[100:200, 4:6] = 0.
    eye = basis_of((0., 0.))
    for gap, ox, oy in ((1.0, 0., 0.), (0., 0., 0.), (1.0, 0.002, -0.01), (123.456, -3.25, 1e-9)):
        got, hit = host_fly_posed(pose_host, a, gap, ox, oy, eye)
        want = host_fly(relay_host, a, gap, ox, oy)
        assert hit.all()
        g, w = got.ravel(), want.ravel()
        assert np.all((g.view(np.uint64) == w.view(np.uint64)) | ((g == 0.) & (w == 0.))), (gap, ox, oy)
    assert pose_host.relay_pose_plain(0., 0., 0) == 1 and pose_host.relay_pose_plain(-0., 0., 0) == 1
    assert pose_host.relay_pose_plain(0., 0., 1) == 0                 # a selection needs the posed kernels
    for t in (5e-324, -5e-324, 1e-300, 0.002, math.nan):
        assert pose_host.relay_pose_plain(t, 0., 0) == 0 and pose_host.relay_pose_plain(0., t, 0) == 0


# ---- 4. missed ------------------------------------------------------------------------------------------------------------------
def _walk(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def _edge(f, lo, hi):
    """the largest double v in [lo, hi) with f(v) true, for f true at lo and false at hi, by bisection on the doubles"""
    assert f(lo) and not f(hi)
    while np.nextafter(lo, hi) != hi:
        mid = lo + (hi - lo) / 2.
        if f(mid):
            lo = mid
        else:
            hi = mid
    return lo


def test_missed_on_each_side_of_its_edges(pose_host):
    # nd > 0: a second optic tilted by 1.2 rad; the photon's dx is walked through the direction that lies in the entrance plane
    b = basis_of((1.2, 0.))

    def nd(dx):
        dx = np.float64(dx)
        return (b[6] * dx + b[7] * np.float64(0.)) + b[8] * np.sqrt((np.float64(1.) - dx * dx) - np.float64(0.))

    last = _edge(lambda v: nd(v) <= 0., -0.9, 0.)                 # the last dx that still runs away from the plane
    dxs = np.array([_walk(last, k) for k in range(-40, 41)])
    six = np.zeros((len(dxs), 6))
    six[:, 2], six[:, 4] = dxs, 1.
    got, hit = host_fly_posed(pose_host, six, 1.0, 0., 0., b)
    want = np.array([nd(v) > 0. for v in dxs])
    assert np.array_equal(hit, want) and not hit[40] and hit[41] and nd(dxs[40]) <= 0. < nd(dxs[41])
    assert np.all(got[hit, 5] > 0.) and np.all(np.isfinite(got[hit]))
    # nd == 0 exactly: a photon along x into an untilted optic (dz = 0)
    assert not host_fly_posed(pose_host, [[0., 0., 1., 0., 0., 1.]], 1.0, 0., 0., basis_of((0., 0.)))[1][0]

    # np >= 0: a second optic tilted by 0.3 rad 0.01 cm behind A; the photon's x is walked through the entrance plane
    b = basis_of((0.3, 0.))
    gap = 0.01

    def npl(x):
        return (b[6] * (np.float64(0.) - np.float64(x)) + b[7] * (np.float64(0.) - np.float64(0.))) + b[8] * np.float64(gap)

    last = _edge(lambda v: npl(v) >= 0., 0., 0.5)                 # the last x in front of the plane (or in it)
    xs = np.array([_walk(last, k) for k in range(-40, 41)])
    six = np.zeros((len(xs), 6))
    six[:, 0], six[:, 4] = xs, 1.
    got, hit = host_fly_posed(pose_host, six, gap, 0., 0., b)
    want = np.array([npl(v) >= 0. for v in xs])
    assert np.array_equal(hit, want) and hit[40] and not hit[41] and npl(xs[41]) < 0. <= npl(xs[40])
    assert np.all(got[hit, 9] >= 0.)
    # np == 0 exactly: the photon starts in the entrance plane and is injected where it is, t = 0
    o, h = host_fly_posed(pose_host, [[0., 0., 0.01, 0., 0., 1.]], 0., 0., 0., b)
    assert h[0] and o[0, 9] == 0. and o[0, 0] == 0. and o[0, 1] == 0.
    # and one ulp behind it (gap 0, the photon at x = +tiny: n0 * (0 - x) < 0) it is missed
    assert not host_fly_posed(pose_host, [[1e-300, 0., 0.01, 0., 0., 1.]], 0., 0., 0., b)[1][0]


# ---- 5. the pose check ----------------------------------------------------------------------------------------------------------
HALF_PI = 1.5707963267948966
BAD_POSES = [(math.nan, 0., 0., 0., 0.), (1., math.nan, 0., 0., 0.), (1., 0., math.nan, 0., 0.), (1., 0., 0., math.nan, 0.), (1., 0., 0., 0., math.nan),
             (math.inf, 0., 0., 0., 0.), (1., -math.inf, 0., 0., 0.), (1., 0., math.inf, 0., 0.), (1., 0., 0., math.inf, 0.), (1., 0., 0., 0., -math.inf),
             (-1e-300, 0., 0., 0., 0.), (-1., 0., 0., 0.001, 0.),
             (1., 0., 0., HALF_PI, 0.), (1., 0., 0., 0., -HALF_PI), (1., 0., 0., np.nextafter(HALF_PI, 2.), 0.), (1., 0., 0., 0., 2.), (1., 0., 0., -3.2, 0.)]
GOOD_POSES = [(0., 0., 0., 0., 0.), (1., 0.002, -0.01, 0.003, 0.001), (1., 0., 0., 1.5, -1.5), (1e6, -5., 5., np.nextafter(HALF_PI, 0.), 0.),
              (5e-324, 0., 0., 0., -1.5)]


def test_validate_refuses_bad_poses(pose_host):
    import polycap_amd
    L = polycap_amd.lib()
    assert L.pc_hip_pose_validate(None) == -2 and b"pose" in L.pc_hip_last_error()
    out = np.zeros(9)
    dp = C.POINTER(C.c_double)
    for p in BAD_POSES:
        arr = np.array(p, dtype=np.float64)
        assert L.pc_hip_pose_validate(arr.ctypes.data_as(dp)) == -2, p
        assert b"tilt" in L.pc_hip_last_error() and b"gap" in L.pc_hip_last_error()
        assert L.pc_hip_pose_basis(arr.ctypes.data_as(dp), out.ctypes.data_as(dp)) == -2 and not out.any()
        assert pose_host.relay_pose_ok(*p) == 0
        if p[3] or p[4] or p[3] != p[3] or p[4] != p[4]:
            assert not polycap_amd.relay_placement_valid(p[0], p[1:3], p[3:5]), p
    for p in GOOD_POSES:
        arr = np.array(p, dtype=np.float64)
        assert L.pc_hip_pose_validate(arr.ctypes.data_as(dp)) == 0, p
        assert polycap_amd.relay_placement_valid(p[0], p[1:3], p[3:5]), p
        assert pose_host.relay_pose_ok(*p) == 1
    # an untilted placement goes the way it went
    assert polycap_amd.relay_placement_valid(1., (0.002, 0.)) and not polycap_amd.relay_placement_valid(-1., (0., 0.))


def test_posed_oracle_floors_are_the_ones_the_gpu_test_uses(oracle):
    """scripts/relay_floors.py --tilt 0.003 0.001 on the oracle (no GPU): the flip caps and weight floors of
    tests/test_gpu_relay_pose.py are its maxima, to the digits written there, as tests/test_relay_cpu.py ties the untilted ones; and
    without a tilt the script measures what it measured."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("relay_floors", os.path.join(ROOT, "scripts", "relay_floors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from tests.test_gpu_relay_pose import POSED_FLOORS, TILTED
    assert TILTED == (1.0, (0., 0.), (0.003, 0.001))
    for name, (flip_cap, c_floor) in POSED_FLOORS.items():
        flips, cs, n1 = mod.floors(oracle, name, gap=TILTED[0], tilt=TILTED[2], offset=TILTED[1])
        print(name, n1, flips, cs)
        assert abs(max(flips) - flip_cap) <= 0.1 * flip_cap, (name, flips)
        assert abs(max(cs) - c_floor) <= 0.1 * c_floor, (name, cs)
    assert mod.floors(oracle, "pinned", tilt=(0., 0.)) == mod.floors(oracle, "pinned")


def test_pose_symbols_are_exported_and_declared():
    import polycap_amd
    polycap_amd.lib()
    so = os.path.join(ROOT, "polycap_amd", "lib", "libpolycap.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    names = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    assert [n for n in names if n.startswith("pc_hip_pose")] == sorted(NEW_SYMBOLS)
    text = open(os.path.join(ROOT, "include", "polycap-hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"POLYCAP_EXTERN\s+[^;(]*?\b(\w+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared
    assert not [n for n in names if n.startswith("_Z") or "pc_relay" in n]

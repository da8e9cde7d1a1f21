"""Scans on the GPU (pc_hip_scan_*, TraceContext.scan; the contract is in include/polycap-hip.h).

The core guarantee: for every point k, a scan's counters and exact sums are bit-identical to those of a source run of n_per_point
slots on a context whose source sits at point k (ctx_k).  The rest: a scan gives the same bits however its flat range is cut into
calls, members or launch shapes; max_attempts = 1 is a budget of started photons; the physics agrees with the oracle; a scan leaves
the context's last run alone; bad arguments are refused with a message."""
import os

import numpy as np
import pytest

from tests.common import make_pair
from tests.conftest import EXAMPLE

pytestmark = pytest.mark.gpu

UNIFORM = (5., 0.01, 0.01, -1., 0., 0., 0., 0.0)          # uniform illumination point source (reference tests/leaks.c:1264)


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def _deck(pa, name, **kw):
    return pa.problem_from_inp(os.path.join(EXAMPLE, name + ".inp"), **kw)


def _at(pa, prob, point):
    """the problem with its source moved to point (d_source, src_shiftx, src_shifty)"""
    src = list(prob.source)
    src[0], src[5], src[6] = (float(v) for v in point)
    return pa.Problem(prob.z, prob.cap, prob.ext, prob.sig_rough, prob.n_cap, prob.density, prob.energies, prob.amu, prob.scatf,
                      *src)


def _points(prob):
    d, sx, sy = prob.source[0], prob.source[5], prob.source[6]
    return np.array([[d, sx, sy],                          # on axis: the context's own source
                     [d, sx + 0.02, sy], [d, sx - 0.02, sy], [d, sx, sy + 0.015],
                     [d, sx + 0.011, sy - 0.013],           # oblique
                     [d * 1.5, sx + 0.005, sy]])            # another distance


def _run_k(pa, prob, point, seed, slot0, npp, max_attempts, opts):
    with pa.TraceContext(_at(pa, prob, point)) as c:
        for k, v in opts.items():
            c.set_option(k, v)
        c.run(seed, slot0, npp, max_attempts)
        t = c.totals(check=False)
        m = c.moments() if opts.get("weight_squares") else None
    return t, m


def _check_equivalent(pa, prob, seed, slot0, npp, max_attempts, run_opts, scan_opts=None):
    pts = _points(prob)
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        for k, v in (scan_opts or {}).items():
            ctx.set_option(k, v)
        r = ctx.scan(seed, pts, npp, max_attempts=max_attempts, slot0=slot0)
    assert r["counters"].shape == (len(pts), 6) and r["sumw_fixed"].shape == (len(pts), prob.n_energies, 2)
    for k in range(len(pts)):
        t, m = _run_k(pa, prob, pts[k], seed, slot0, npp, max_attempts, dict(run_opts, weight_squares=1))
        assert np.array_equal(r["counters"][k], t["counters"]), (k, r["counters"][k], t["counters"])
        assert np.array_equal(r["sumw_fixed"][k], t["sumw_fixed"]), k
        assert np.array_equal(r["sumw2_fixed"][k], m), k
        assert np.array_equal(r["efficiencies"][k], pa.efficiencies(t["sum_weights"], t["counters"])) or t["counters"][0] + t["counters"][2] == 0
    return r


@pytest.mark.parametrize("case", ["xos1_1e", "uniform_1e", "ellip_3e", "ellip_7e", "ellip_l9_20e"])
def test_scan_equals_separate_runs(pa, oracle, case):
    lane = dict(producer=0, pool=0)
    if case == "xos1_1e":
        prob = _deck(pa, "xos1", energies=[10.0])
        r = _check_equivalent(pa, prob, 11, 5, 4000, 1 << 20, lane)
        assert r["counters"][:, 4].sum() == 0
        # default options on ctx_k (the kernels are bit-identical there) and the failed-slot regime with max_attempts = 1
        _check_equivalent(pa, prob, 12, 0, 3000, 1 << 20, {})
        r = _check_equivalent(pa, prob, 13, 100, 5000, 1, lane)
        assert r["counters"][:, 4].sum() > 0
    elif case == "uniform_1e":
        _, _, prob, _ = make_pair(oracle, "ellip", source=UNIFORM)
        _check_equivalent(pa, prob, 21, 0, 6000, 1 << 20, lane)
        _check_equivalent(pa, prob, 22, 7, 8000, 1, {})
    elif case == "ellip_3e":
        _, _, prob, _ = make_pair(oracle, "ellip", energies=(8.0, 10.0, 12.5))
        _check_equivalent(pa, prob, 31, 0, 3000, 1 << 20, lane)
        _check_equivalent(pa, prob, 32, 0, 4000, 1, lane)
    elif case == "ellip_7e":
        _, _, prob, _ = make_pair(oracle, "ellip", energies=(6.0, 8.0, 10.0, 12.5, 15.0, 20.0, 25.0))
        _check_equivalent(pa, prob, 41, 3, 3000, 1 << 20, lane)
    else:
        prob = _deck(pa, "ellip_l9", energies=np.linspace(5.0, 30.0, 20), sig_rough=5.0)
        _check_equivalent(pa, prob, 51, 0, 3000, 1 << 20, dict(lane, batch_reflections=0))
        _check_equivalent(pa, prob, 52, 0, 3000, 1, dict(lane, batch_reflections=0))


def _sum(parts):
    out = {}
    for key in ("counters", "sumw_fixed", "sumw2_fixed"):
        if key == "counters":
            out[key] = sum(p[key] for p in parts)
        else:
            v = sum(p[key].astype(object)[..., 0] + (p[key].astype(object)[..., 1] << 64) for p in parts)
            out[key] = np.stack([(v & (2 ** 64 - 1)).astype(np.uint64), (v >> 64).astype(np.uint64)], axis=-1)
    return out


def test_scan_split_invariance(pa, oracle):
    _, _, prob, _ = make_pair(oracle, "ellip", source=UNIFORM)
    pts = pa.scan_points(x=np.linspace(-0.03, 0.03, 7), y=[0.0, 0.01])
    npp, seed = 3001, 61
    total = len(pts) * npp
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        one = ctx.scan(seed, pts, npp, max_attempts=1 << 20)
        cuts = [0, 4000, 4001 + npp * 3, total]              # pieces that cut through points
        parts = [ctx.scan(seed, pts, npp, max_attempts=1 << 20, first=cuts[i], count=cuts[i + 1] - cuts[i]) for i in range(3)]
        s = _sum(parts)
        for key in ("counters", "sumw_fixed", "sumw2_fixed"):
            assert np.array_equal(s[key], one[key]), key
        for bs, bpc in ((256, 1), (128, 3)):
            ctx.set_option("block_size", bs)
            ctx.set_option("blocks_per_cu", bpc)
            r = ctx.scan(seed, pts, npp, max_attempts=1 << 20)
            for key in ("counters", "sumw_fixed", "sumw2_fixed"):
                assert np.array_equal(r[key], one[key]), (bs, bpc, key)
    for devs in ((0, 0), (0, 0, 0)):
        with pa.TraceGroup(prob, devs) as g:
            g.set_option("weight_squares", 1)
            r = g.scan(seed, pts, npp, max_attempts=1 << 20)
        for key in ("counters", "sumw_fixed", "sumw2_fixed"):
            assert np.array_equal(r[key], one[key]), (devs, key)
    # every slot its own point
    rng = np.random.default_rng(3)
    many = np.stack([np.full(5000, UNIFORM[0]), rng.uniform(-0.04, 0.04, 5000), rng.uniform(-0.04, 0.04, 5000)], axis=1)
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        a = ctx.scan(71, many, 1, max_attempts=4)
        b = _sum([ctx.scan(71, many, 1, max_attempts=4, first=f, count=c) for f, c in ((0, 1234), (1234, 5000 - 1234))])
    for key in ("counters", "sumw_fixed", "sumw2_fixed"):
        assert np.array_equal(a[key], b[key]), key
    assert np.all(a["counters"][:, 5] >= 1) and a["counters"][:, 5].sum() <= 4 * 5000
    for k in (0, 1777, 4999):                                # spot checks against one-point runs
        t, _ = _run_k(pa, prob, many[k], 71, 0, 1, 4, dict(producer=0, pool=0))
        assert np.array_equal(a["counters"][k], t["counters"]) and np.array_equal(a["sumw_fixed"][k], t["sumw_fixed"])


def test_started_photon_budget(pa):
    prob = _deck(pa, "xos1", energies=[10.0])
    d = prob.source[0]
    pts = np.array([[d, 0.0, 0.0], [d, 0.05, 0.0], [d, 1.0, 0.0], [d, 0.0, -1.0]])
    npp = 20000
    with pa.TraceContext(prob) as ctx:
        r = ctx.scan(81, pts, npp, max_attempts=1)
    c = r["counters"]
    # every slot makes exactly one attempt: it exits or is exhausted.  The efficiency's denominator counts what the reference's
    # driver counts (exit, not entered, not transmitted); a photon that leaves the optic outside its exit window is in none of them
    assert np.all(c[:, 5] == npp) and np.all(c[:, 0] + c[:, 4] == npp)
    assert np.all(c[:, 0] + c[:, 1] + c[:, 2] <= npp) and c[0, 0] + c[0, 1] + c[0, 2] > npp // 2
    assert r["efficiencies"][0, 0] > 0 and np.all(np.isfinite(r["efficiencies"]))
    assert np.all(r["efficiencies"][2:, 0] < 0.01 * r["efficiencies"][0, 0])
    assert r["kernel_ms"] > 0


def test_scan_vs_oracle(pa, oracle):
    """one shifted point at another distance against the oracle's driver with that source (tolerance of
    test_transmission_driver_vs_oracle: 1/sqrt(i_start))"""
    optic, _, prob, (E, A, S) = make_pair(oracle, "ellip")
    point = (1500.0, 0.003, -0.002)
    src = list(prob.source)
    src[0], src[5], src[6] = point
    n = 30000
    o = oracle.transmission(optic, oracle.make_source(*src), E, A, S, 20000, 0, n)
    with pa.TraceContext(prob) as ctx:
        r = ctx.scan(20000, [point], n, max_attempts=1 << 20)
    c = r["counters"][0]
    i_start = int(c[0] + c[1] + c[2])
    assert c[0] == n and c[4] == 0
    tol = 1.0 / np.sqrt(i_start)
    assert abs(i_start - o["i_start"]) / o["i_start"] < tol
    assert abs(r["efficiencies"][0, 0] - o["efficiencies"][0]) / o["efficiencies"][0] < tol


def test_mirror_symmetry(pa, oracle):
    _, _, prob, _ = make_pair(oracle, "ellip", source=UNIFORM)
    s = np.array([0.004, 0.01, 0.02, 0.03, 0.045])
    pts = pa.scan_points(x=np.concatenate([s, -s]))
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        r = ctx.scan(91, pts, 20000, max_attempts=1)
    e, se = r["efficiencies"][:, 0], r["stderr"][:, 0]
    for i in range(len(s)):
        j = i + len(s)
        assert abs(e[i] - e[j]) <= 4 * np.hypot(se[i], se[j]), (s[i], e[i], e[j], se[i], se[j])


def test_scan_leaves_the_run_alone(pa):
    prob = _deck(pa, "xos1", energies=[10.0])
    n = 140000
    win = (-0.3, 0.3, -0.3, 0.3)

    def fetch(ctx):
        spot = pa.SpotMap(ctx, [0.0, 1.0], win, (32, 32))
        spot.add("exit")
        t = ctx.totals()
        return (t["counters"], t["sumw_fixed"], ctx.moments(), ctx.images(0, n), spot.read())

    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        ctx.set_option("run_parts", 2)          # two launches on two streams: the scan is enqueued behind both
        ctx.run(6, 0, n, keep_images=True)
        r = ctx.scan(7, pa.scan_points(x=[0.0, 0.02]), 3000, max_attempts=1 << 20)
        after = fetch(ctx)
        ctx.run(6, 0, n, keep_images=True)
        ref = fetch(ctx)
        ctx.scan(7, pa.scan_points(x=[0.0, 0.02]), 3000)
        ctx.run(8, 0, 50000)
        after_scan = ctx.totals()
    with pa.TraceContext(prob) as fresh:
        fresh.set_option("weight_squares", 1)
        fresh.run(8, 0, 50000)
        ref8 = fresh.totals()
    assert r["counters"][:, 0].sum() == 6000
    for i in range(3):
        assert np.array_equal(after[i], ref[i]), i
    for k in ("images", "exit_weights", "nrefl"):
        assert np.array_equal(after[3][k], ref[3][k], equal_nan=True), k
    for k in ("bins", "outside", "n_entries"):
        assert np.array_equal(after[4][k], ref[4][k]), k
    assert np.array_equal(after_scan["counters"], ref8["counters"]) and np.array_equal(after_scan["sumw_fixed"], ref8["sumw_fixed"])


def test_scan_errors(pa):
    prob = _deck(pa, "xos1", energies=[10.0])
    d = prob.source[0]
    with pa.TraceContext(prob) as ctx:
        bad = [
            (dict(points=[[0.0, 0.0, 0.0]], n_per_point=10), "pc_hip_scan_run: point 0: d_source must be greater than 0"),
            (dict(points=[[d, 0.0, 0.0], [d, np.inf, 0.0]], n_per_point=10), "pc_hip_scan_run: point 1: src_shiftx must be finite"),
            (dict(points=[[d, 0.0, 0.0]], n_per_point=0), "pc_hip_scan_run: n_per_point must be >= 1"),
            (dict(points=np.zeros((0, 3)), n_per_point=10), "pc_hip_scan_run: n_points must be >= 1"),
            (dict(points=[[d, 0.0, 0.0]], n_per_point=10, first=5, count=6), "pc_hip_scan_run: first and count"),
            (dict(points=[[d, 0.0, 0.0]], n_per_point=10, first=-1, count=2), "pc_hip_scan_run: first and count"),
            (dict(points=[[d, 0.0, 0.0]], n_per_point=2 ** 62, slot0=2 ** 62), "pc_hip_scan_run: slot0 + n_per_point overflows int64"),
            (dict(points=[[d, 0.0, 0.0]] * 4, n_per_point=2 ** 62), "pc_hip_scan_run: n_points * n_per_point overflows int64"),
        ]
        for kw, msg in bad:
            with pytest.raises(pa.HipError) as e:
                ctx.scan(1, **kw)
            assert e.value.status == -2 and msg in str(e.value), (kw, str(e.value))
        # sumw2 of a scan made without weight_squares
        ctx.scan(1, [[d, 0.0, 0.0]], 100)
        ctx._weight_squares = True
        with pytest.raises(pa.HipError) as e:
            pa.hip._scan_fetch(ctx._L.pc_hip_scan_totals, ctx._h, 1, 1, True)
        assert e.value.status == -2 and "sumw2_fixed" in str(e.value) and "weight_squares" in str(e.value)
        ctx._weight_squares = False
        # still usable
        r = ctx.scan(1, [[d, 0.0, 0.0]], 100, max_attempts=1 << 20)
        assert r["counters"][0, 0] == 100
        t = ctx.transmission(1, 0, 1000)
        assert t["i_exit"] == 1000

"""Scans of more than 8 energies through the logging kernel (context option "scan_log" = 1; include/polycap-hip.h).

The scan's contract with nothing forced: for every point k the counters and the exact sums of the weights and of their squares are
bit-identical to those of a source run with DEFAULT options (the logging kernel) on a context whose source sits at point k -- with
roughness too, where the immediate-sweep scan differs from such a run in the last bits of the weights.  The rest: the fused
finalisation and its take-back pass add to and subtract from a point's global sums exactly; the totals do not depend on how the
flat range is cut, also with one slot per point (a flush of the per-point counters at every photon); a scan that cannot log keeps
the lane kernel; a logging scan leaves the context's last run alone."""
import numpy as np
import pytest

from tests.test_gpu_scan import _at, _deck, _points, _sum

pytestmark = pytest.mark.gpu

LOG, LANE = "pc_trace_log_kernel", "pc_trace_kernel"
KEYS = ("counters", "sumw_fixed", "sumw2_fixed")


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def _rough20(pa):
    return _deck(pa, "ellip_l9", energies=np.linspace(5.0, 30.0, 20), sig_rough=5.0)


def _scan(pa, prob, seed, pts, npp, max_attempts, opts=None, scan_log=1, **kw):
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        ctx.set_option("scan_log", scan_log)
        for k, v in (opts or {}).items():
            ctx.set_option(k, v)
        return ctx.scan(seed, pts, npp, max_attempts=max_attempts, **kw)


def _same(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (what, key)


def _equals_separate_runs(pa, prob, r, seed, slot0, pts, npp, max_attempts, run_opts=None, which=None):
    """every point of scan r against a source run at that point: default options but weight_squares (and run_opts)"""
    for k in (range(len(pts)) if which is None else which):
        with pa.TraceContext(_at(pa, prob, pts[k])) as c:
            c.set_option("weight_squares", 1)
            for o, v in (run_opts or {}).items():
                c.set_option(o, v)
            c.run(seed, slot0, npp, max_attempts)
            t = c.totals(check=False)
            m = c.moments()
            assert c.last_kernel() == LOG
        assert np.array_equal(r["counters"][k], t["counters"]), (k, r["counters"][k], t["counters"])
        assert np.array_equal(r["sumw_fixed"][k], t["sumw_fixed"]), k
        assert np.array_equal(r["sumw2_fixed"][k], m), k


# ------------------------------------------------------------------------------------------------------ 1. equals separate runs
@pytest.mark.parametrize("case", ["rough20", "rough20_one_attempt", "xos1_12", "xos1_70", "xos1_291"])
def test_logging_scan_equals_default_runs(pa, case):
    """rough20: roughness, log capacity 32 -- the case in which an immediate-sweep scan differs from a default run (~4e-14 in the
    weights); xos1_70 and xos1_291: log capacity 64; one_attempt: max_attempts = 1, slots fail"""
    seed, slot0, npp, max_attempts = 51, 0, 3000, 1 << 20
    if case.startswith("rough20"):
        prob = _rough20(pa)
        if case.endswith("one_attempt"):
            seed, max_attempts = 52, 1
    elif case == "xos1_12":
        prob, seed, slot0 = _deck(pa, "xos1", energies=np.linspace(5.0, 25.0, 12)), 53, 7
    elif case == "xos1_70":
        prob, seed = _deck(pa, "xos1", energies=np.linspace(3.0, 30.0, 70)), 54
    else:
        prob, seed, npp = _deck(pa, "xos1", energies=np.linspace(2.0, 40.0, 291)), 55, 1000
    pts = _points(prob)
    r = _scan(pa, prob, seed, pts, npp, max_attempts, slot0=slot0)
    assert r["kernel"] == LOG
    assert r["counters"].shape == (len(pts), 6) and r["sumw_fixed"].shape == (len(pts), prob.n_energies, 2)
    if max_attempts == 1:
        assert np.all(r["counters"][:, 5] == npp) and r["counters"][:, 4].sum() > 0
    else:
        assert np.all(r["counters"][:, 0] == npp) and r["counters"][:, 4].sum() == 0
    _equals_separate_runs(pa, prob, r, seed, slot0, pts, npp, max_attempts)


# ------------------------------------------------------------------------------------------------------ 2. photons that die
def test_fused_sums_and_their_take_back_per_point(pa):
    """xos1 at 12 energies up to 40 keV: photons die in the optic.  sweep_fuse 0 leaves every sum to the NEW phase, 1 lets the sweep
    of a finished photon add to its point's global sums, 2 does so whatever the proxies say, so that photons the sweep finds dead
    have their sums taken back (the 128-bit two's complement added).  Without roughness the logging kernel's products are the
    immediate sweep's, so every variant also equals the scan_log = 0 scan."""
    prob = _deck(pa, "xos1", energies=np.linspace(10.0, 40.0, 12))
    pts = _points(prob)
    seed, npp, ma = 61, 3000, 1 << 20
    lane = _scan(pa, prob, seed, pts, npp, ma, scan_log=0)
    assert lane["kernel"] == LANE
    assert lane["counters"][:, 2].sum() > 0                      # absorbed in the glass
    variants = [dict(sweep_fuse=0), dict(sweep_fuse=1), dict(sweep_fuse=2), dict(sweep_fuse=2, sweep_exact_every=3),
                dict(sweep_fuse=1, sweep_exact_every=3), dict(sweep_fuse=2, log_cap=8), dict(sweep_fuse=0, log_cap=8)]
    for opts in variants:
        r = _scan(pa, prob, seed, pts, npp, ma, opts)
        assert r["kernel"] == LOG, opts
        _same(r, lane, opts)
    # separate runs with the same log capacity
    r = _scan(pa, prob, seed, pts, npp, ma, dict(log_cap=8))
    _equals_separate_runs(pa, prob, r, seed, 0, pts, npp, ma, run_opts=dict(log_cap=8))


# ------------------------------------------------------------------------------------------------------ 3. split invariance
def test_logging_scan_split_invariance(pa):
    prob = _rough20(pa)
    pts = _points(prob)
    npp, seed, ma = 3000, 71, 1 << 20
    total = len(pts) * npp
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        ctx.set_option("scan_log", 1)
        one = ctx.scan(seed, pts, npp, max_attempts=ma)
        cuts = [0, 4000, 4001 + npp * 3, total]                  # pieces that cut through points
        parts = [ctx.scan(seed, pts, npp, max_attempts=ma, first=cuts[i], count=cuts[i + 1] - cuts[i]) for i in range(3)]
        assert one["kernel"] == LOG and all(p["kernel"] == LOG for p in parts)
        _same(_sum(parts), one, "three pieces")
    with pa.TraceGroup(prob, (0, 0)) as g:
        g.set_option("weight_squares", 1)
        g.set_option("scan_log", 1)
        r = g.scan(seed, pts, npp, max_attempts=ma)
        assert r["kernel"] == [LOG, LOG]
    _same(r, one, "group (0, 0)")
    # every slot its own point: the per-point counters are flushed at every photon
    d = prob.source[0]
    rng = np.random.default_rng(3)
    many = np.stack([np.full(5000, d), rng.uniform(-0.03, 0.03, 5000), rng.uniform(-0.03, 0.03, 5000)], axis=1)
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        ctx.set_option("scan_log", 1)
        a = ctx.scan(72, many, 1, max_attempts=4)
        b = _sum([ctx.scan(72, many, 1, max_attempts=4, first=f, count=c) for f, c in ((0, 1234), (1234, 5000 - 1234))])
        assert a["kernel"] == LOG
    _same(a, b, "two halves of 5000 points")
    assert np.all(a["counters"][:, 5] >= 1) and a["counters"][:, 5].sum() <= 4 * 5000
    assert np.all(a["counters"][:, 0] + a["counters"][:, 4] == 1)
    _equals_separate_runs(pa, prob, a, 72, 0, many, 1, 4, which=(0, 1777, 4999))


# ------------------------------------------------------------------------------------------------------ 4. fallback and errors
def test_fallback_and_errors(pa):
    for energies in ([10.0], np.linspace(6.0, 24.0, 7)):
        prob = _deck(pa, "xos1", energies=energies)
        pts = _points(prob)
        off = _scan(pa, prob, 81, pts, 2000, 1 << 20, scan_log=0)
        on = _scan(pa, prob, 81, pts, 2000, 1 << 20, scan_log=1)
        assert on["kernel"] == LANE and off["kernel"] == LANE
        _same(on, off, len(energies))
    prob = _deck(pa, "xos1", energies=np.linspace(5.0, 25.0, 12))
    with pa.TraceContext(prob) as ctx:
        assert ctx._L.pc_hip_scan_last_kernel(ctx._h) == -1
        for bad in (2, -1):
            with pytest.raises(pa.HipError) as e:
                ctx.set_option("scan_log", bad)
            assert e.value.status == -2 and "scan_log must be 0 or 1" in str(e.value)
        ctx.run(1, 0, 1000)
        assert ctx._L.pc_hip_scan_last_kernel(ctx._h) == -1       # a run is not a scan
        # the conditions of a source run: without batch_reflections the scan keeps the lane kernel
        ctx.set_option("scan_log", 1)
        ctx.set_option("batch_reflections", 0)
        assert ctx.scan(1, _points(prob)[:2], 500)["kernel"] == LANE
        assert ctx._L.pc_hip_scan_last_kernel(ctx._h) == 0
        ctx.set_option("batch_reflections", 1)
        assert ctx.scan(1, _points(prob)[:2], 500)["kernel"] == LOG
        assert ctx._L.pc_hip_scan_last_kernel(ctx._h) == 4
    with pa.TraceGroup(prob, (0, 0)) as g:
        assert [g._L.pc_hip_group_scan_last_kernel(g._h, k) for k in (0, 1, 2)] == [-1, -1, -1]
        with pytest.raises(pa.HipError) as e:
            g.set_option("scan_log", 2)
        assert e.value.status == -2 and "scan_log must be 0 or 1" in str(e.value)


# ------------------------------------------------------------------------------------------------------ 5. the run stays
def test_logging_scan_leaves_the_run_alone(pa):
    prob = _deck(pa, "xos1", energies=np.linspace(5.0, 25.0, 12))
    n = 20000

    def fetch(ctx):
        t = ctx.totals()
        return (t["counters"], t["sumw_fixed"], ctx.moments(), ctx.images(0, n), ctx.last_kernel())

    with pa.TraceContext(prob) as ctx:
        ctx.set_option("weight_squares", 1)
        ctx.set_option("scan_log", 1)
        ctx.run(6, 0, n, keep_images=True)
        r = ctx.scan(7, _points(prob), 3000, max_attempts=1 << 20)
        after = fetch(ctx)
        ctx.run(6, 0, n, keep_images=True)
        ref = fetch(ctx)
    assert r["kernel"] == LOG and r["counters"][:, 0].sum() == 6 * 3000
    assert ref[4] == LOG and after[4] == LOG
    for i in range(3):
        assert np.array_equal(after[i], ref[i]), i
    for k in ("images", "exit_weights", "nrefl"):
        assert np.array_equal(after[3][k], ref[3][k], equal_nan=True), k

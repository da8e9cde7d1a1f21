"""Standard errors on the GPU (option "weight_squares", pc_hip_transmission_moments, POLYCAP_STDERR).

Exactness: in every kernel, the sum B of the squared exit weights equals sum int((w*w) * 2^62) over the exit weights the same run
returns, and switching the option on changes nothing else (counters, the weights' sums and every exit weight bit for bit).
Invariance: B is bit-equal however the same slots are run.  Calibration: across 32 seeds, the spread of the efficiency matches the
standard error each run reports about itself."""
import os

import numpy as np
import pytest

from tests.conftest import EXAMPLE

pytestmark = pytest.mark.gpu

DECK = os.path.join(EXAMPLE, "xos1.inp")
SEED = 777


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def to_int(pairs):
    """[n_energies, 2] (lo, hi) uint64 -> list of Python ints"""
    p = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return [int(lo) + (int(hi) << 64) for lo, hi in p]


def to_pairs(ints):
    return np.array([[v & (2 ** 64 - 1), v >> 64] for v in ints], dtype=np.uint64)


def b_of(W):
    """sum over the rows of int((w*w) * 2^62), per energy, exactly: each term is below 2^63, summed as two 32-bit halves"""
    q = ((W * W) * np.float64(2.0 ** 62)).astype(np.uint64)
    lo = (q & np.uint64(0xffffffff)).sum(axis=0, dtype=np.uint64)
    hi = (q >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
    return [int(a) + (int(b) << 32) for a, b in zip(lo, hi)]


def a_of(W):
    q = (W * np.float64(2.0 ** 62)).astype(np.uint64)
    lo = (q & np.uint64(0xffffffff)).sum(axis=0, dtype=np.uint64)
    hi = (q >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
    return [int(a) + (int(b) << 32) for a, b in zip(lo, hi)]


def _deck(pa, name="xos1", **kw):
    return pa.problem_from_inp(os.path.join(EXAMPLE, name + ".inp"), **kw)


def _opts(ctx, **opts):
    for k, v in opts.items():
        ctx.set_option(k, v)


def _run(ctx, n, keep_images, leak=False, slot0=0, seed=SEED):
    r = ctx.transmission(seed, slot0, n, keep_images=keep_images, leak_calc=leak)
    r["B"] = to_int(ctx.moments())
    r["A"] = to_int(r["sumw_fixed"])
    return r


def _totals_only(ctx, n, keep_images, slot0=0, seed=SEED):
    """run + wait + totals + moments, images left on the device (plane and compact stores are fetched otherwise)"""
    ctx.run(seed, slot0, n, keep_images=keep_images)
    ctx.wait()
    r = ctx.totals()
    r["B"] = to_int(ctx.moments())
    r["A"] = to_int(r["sumw_fixed"])
    return r


def _same_run(off, on, what):
    assert np.array_equal(off["counters"], on["counters"]), what
    assert np.array_equal(off["sumw_fixed"], on["sumw_fixed"]), what
    if "exit_weights" in off:
        assert np.array_equal(off["exit_weights"], on["exit_weights"]), what


# name: (problem, n_slots, options, kernel, leak_calc)
KERNEL_CASES = {
    "producer_1e": (dict(energies=[10.0]), 60000, dict(producer=1), "pc_trace_producer_kernel", False),
    "lane_1e": (dict(energies=[10.0]), 60000, dict(producer=0), "pc_trace_kernel", False),
    "lane_3e": (dict(energies=[8.0, 12.0, 17.0]), 40000, {}, "pc_trace_kernel", False),
    "lane_7e": (dict(energies=list(np.linspace(4.0, 25.0, 7))), 40000, {}, "pc_trace_kernel", False),
    "immediate_12e": (dict(energies=list(np.linspace(3.0, 30.0, 12))), 30000, dict(batch_reflections=0), "pc_trace_kernel", False),
    "immediate_600e_global_sums": (dict(energies=list(np.linspace(3.0, 30.0, 600))), 8000, dict(batch_reflections=0), "pc_trace_kernel", False),
    "log_12e": (dict(energies=list(np.linspace(3.0, 30.0, 12))), 30000, {}, "pc_trace_log_kernel", False),
    "log_291e": ({}, 20000, {}, "pc_trace_log_kernel", False),
    "log_291e_rough_exact_every": (dict(name="ellip_l9", sig_rough=5.0), 20000, dict(sweep_exact_every=5), "pc_trace_log_kernel", False),
    "pool_1e": (dict(energies=[10.0]), 60000, dict(pool=1, producer=0), "pc_trace_pool_kernel", False),
    "leak_2e": (dict(energies=[10.0, 20.0]), 5000, {}, "pc_leak_kernel", True),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_squares_are_exact_in_every_kernel(pa, case):
    kw, n, opts, kernel, leak = KERNEL_CASES[case]
    kw = dict(kw)
    prob = _deck(pa, kw.pop("name", "xos1"), **kw)
    with pa.TraceContext(prob, 0) as ctx:
        _opts(ctx, **opts)
        off = ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=leak)
        assert ctx.last_kernel() == kernel
        with pytest.raises(pa.HipError) as e:
            ctx.moments()                    # the run was made without the option
        assert e.value.status == -2
        ctx.set_option("weight_squares", 1)
        on = _run(ctx, n, True, leak)
        assert ctx.last_kernel() == kernel
        _same_run(off, on, case)
        W = on["exit_weights"]
        assert W.shape == (n, prob.n_energies) and on["i_exit"] == n
        assert on["B"] == b_of(W), case
        assert on["A"] == a_of(W), case
        assert any(b > 0 for b in on["B"])
        if kernel == "pc_trace_log_kernel":
            # histogram-only runs: the sweep adds the sums itself (sweep_fuse 1), not at all (0), or always with the take-back of
            # the photons it finds dead (2); B equals the keep_images run's bit for bit each time
            for fuse in (0, 1, 2):
                ctx.set_option("sweep_fuse", fuse)
                h = _run(ctx, n, False)
                assert ctx.last_kernel() == kernel
                assert np.array_equal(h["counters"], on["counters"]) and h["A"] == on["A"] and h["B"] == on["B"], (case, fuse)
            ctx.set_option("sweep_fuse", 1)
        else:
            h = _run(ctx, n, False, leak)
            assert np.array_equal(h["counters"], on["counters"]) and h["A"] == on["A"] and h["B"] == on["B"], case
        # switched off again: the plain kernels, and moments() refuses
        ctx.set_option("weight_squares", 0)
        again = ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=leak)
        _same_run(off, again, case)
        with pytest.raises(pa.HipError):
            ctx.moments()


def test_squares_do_not_depend_on_the_launch(pa):
    prob = _deck(pa, energies=[10.0])
    N = 4 * 65536 + 17                  # run_parts 4 really makes 4 launches
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("weight_squares", 1)
        ref = _run(ctx, N, True)
        assert ref["B"] == b_of(ref["exit_weights"])

        def same(r, what):
            assert np.array_equal(r["counters"], ref["counters"]) and r["A"] == ref["A"] and r["B"] == ref["B"], what

        same(_run(ctx, N, False), "histogram only")
        _opts(ctx, run_parts=4)
        same(_run(ctx, N, True), "run_parts 4")
        _opts(ctx, run_parts=1, plane_images=1)
        same(_totals_only(ctx, N, True), "plane store")
        _opts(ctx, compact_images=1)
        same(_totals_only(ctx, N, True), "compact store")
        _opts(ctx, compact_images=0, plane_images=0)
        for prod in (0, 1):
            ctx.set_option("producer", prod)
            same(_run(ctx, N, False), "producer %d" % prod)
        ctx.set_option("producer", -1)
        # split slot ranges, summed exactly
        cut = [0, 50000, 50001, 200000, N]
        A, B, cnt = [0], [0], np.zeros(6, dtype=np.int64)
        for lo, hi in zip(cut[:-1], cut[1:]):
            r = _run(ctx, hi - lo, False, slot0=lo)
            A[0] += r["A"][0]
            B[0] += r["B"][0]
            cnt += r["counters"]
        assert A == ref["A"] and B == ref["B"] and np.array_equal(cnt, ref["counters"])
    # a group of two contexts on one device, summed on the host and (automatic) whatever the group can use
    with pa.TraceGroup(prob, [0, 0]) as g:
        g.set_option("weight_squares", 1)
        for reduce in (0, -1):
            r = g.transmission(SEED, N, reduce=reduce)
            assert to_int(r["sumw_fixed"]) == ref["A"] and np.array_equal(r["counters"], ref["counters"])
            assert to_int(g.moments()) == ref["B"], reduce
    if pa.device_count() >= 2:
        with pa.TraceGroup(prob, [0, 1]) as g:
            g.set_option("weight_squares", 1)
            for reduce in (0, 1):
                r = g.transmission(SEED, N, reduce=reduce)
                assert r["reduced_by_rccl"] == bool(reduce)
                assert to_int(r["sumw_fixed"]) == ref["A"] and to_int(g.moments()) == ref["B"], reduce


def test_group_leak_squares(pa):
    prob = _deck(pa, energies=[10.0, 20.0])
    n = 6000
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("weight_squares", 1)
        ref = _run(ctx, n, False, leak=True)
    with pa.TraceGroup(prob, [0, 0]) as g:
        g.set_option("weight_squares", 1)
        with pytest.raises(pa.HipError):
            g.moments()                      # no totals for the run yet
        st = g._L.pc_hip_group_run_leak(g._h, SEED, n, 1 << 20, 0)
        assert st == 0
        import ctypes as C
        cnt = np.zeros(6, dtype=np.int64)
        fx = np.zeros(4, dtype=np.uint64)
        st = g._L.pc_hip_group_totals(g._h, 0, None, cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                                      fx.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)
        assert st == 0
        assert np.array_equal(cnt, ref["counters"]) and to_int(fx) == ref["A"] and to_int(g.moments()) == ref["B"]


def _public(monkeypatch, n, binding="ctypes", **env):
    if binding == "ctypes":
        from polycap_amd import capi
    else:
        from polycap_amd.pyext import polycap as capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k in ("POLYCAP_STDERR", "POLYCAP_SPOT", "POLYCAP_IMAGES", "POLYCAP_SPOT_SHARE", "POLYCAP_HIP_DEVICES", "POLYCAP_RCCL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = capi.Source.new_from_file(DECK)
    return src, src.get_transmission_efficiencies(1, n)


@pytest.mark.parametrize("binding", ["ctypes", "cython"])
def test_public_call(pa, monkeypatch, tmp_path, binding):
    n = 50000
    _, eff0 = _public(monkeypatch, n, binding)
    src, eff1 = _public(monkeypatch, n, binding, POLYCAP_STDERR="1")
    E, F0 = eff0.data
    F1 = eff1.data[1]
    assert np.array_equal(F0, F1)
    se = eff1.efficiency_stderr()
    mo = eff1.moments()
    assert se.shape == (len(E),) and mo["sumw_fixed"].shape == (len(E), 2) and mo["sumw2_fixed"].shape == (len(E), 2)
    N = mo["n_started"]
    assert N >= n
    cnt = np.array([N, 0, 0, 0, 0, N], dtype=np.int64)    # only the sum of the first three counters enters
    assert np.array_equal(se, pa.efficiency_stderr(mo["sumw_fixed"], mo["sumw2_fixed"], cnt))
    assert np.isfinite(se).all() and (se > 0).any() and (se < F1 + 1e-300).all()
    with pytest.raises(ValueError, match="POLYCAP_STDERR"):
        eff0.efficiency_stderr()
    with pytest.raises(ValueError, match="POLYCAP_STDERR"):
        eff0.moments()
    # a group of two contexts on one device, host sum: the same moments
    _, effg = _public(monkeypatch, n, binding, POLYCAP_STDERR="1", POLYCAP_HIP_DEVICES="0,0", POLYCAP_RCCL="0")
    mg = effg.moments()
    assert mg["n_started"] == N and np.array_equal(mg["sumw_fixed"], mo["sumw_fixed"]) and np.array_equal(mg["sumw2_fixed"], mo["sumw2_fixed"])
    assert np.array_equal(effg.efficiency_stderr(), se)
    # HDF5: the same file apart from the new dataset
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    p0, p1 = str(tmp_path / "off.h5"), str(tmp_path / "on.h5")
    eff0.write_hdf5(p0)
    eff1.write_hdf5(p1)
    l0, l1 = H._listing(p0), H._listing(p1)
    assert "/Transmission_Efficiencies_StdErr" not in l0
    assert l1.pop("/Transmission_Efficiencies_StdErr") == (len(E),)
    assert l0 == l1
    got = H._read(p1, "/Transmission_Efficiencies_StdErr", str(tmp_path))
    assert np.array_equal(got, se)
    for name in l0:
        if l0[name] is not None and name.startswith("/Transmission_Efficiencies"):
            assert np.array_equal(H._read(p0, name, str(tmp_path)), H._read(p1, name, str(tmp_path))), name


def test_public_call_chunked(pa, monkeypatch):
    """POLYCAP_IMAGES=0 with POLYCAP_SPOT traced as consecutive slot ranges (a small share of device memory): the ranges' B are added
    on the host, bit-equal to one unchunked run"""
    spec = "dist=0.5;window=-0.02,0.02,-0.02,0.02;bins=16x16;energies=0"
    n = 60000
    _, e1 = _public(monkeypatch, n, POLYCAP_STDERR="1", POLYCAP_SPOT=spec, POLYCAP_IMAGES="0")
    with pa.TraceContext(_deck(pa, energies=[10.0]), 0) as ctx:
        total = ctx.device_memory()[1]
    share = (n / 4.0) * (17 + len(e1.data[0])) * 8.0 / total
    _, ec = _public(monkeypatch, n, POLYCAP_STDERR="1", POLYCAP_SPOT=spec, POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    m1, mc = e1.moments(), ec.moments()
    assert mc["n_started"] == m1["n_started"]
    assert np.array_equal(mc["sumw_fixed"], m1["sumw_fixed"]) and np.array_equal(mc["sumw2_fixed"], m1["sumw2_fixed"])
    assert np.array_equal(ec.efficiency_stderr(), e1.efficiency_stderr())
    assert np.array_equal(ec.data[1], e1.data[1])


# Calibration: 32 seeds fixed before the first run, 1e5 slots each.  The across-seed SD of the efficiency over the RMS of the
# reported standard errors lies in [0.6, 1.4] (+-3 sigma of an SD estimated from 32 samples).
CAL_SEEDS = [1009 + 7919 * k for k in range(32)]
CAL_SLOTS = 100000


def _calibrate(pa, prob, idx):
    effs, ses = [], []
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("weight_squares", 1)
        for s in CAL_SEEDS:
            r = ctx.transmission(s, 0, CAL_SLOTS)
            se = pa.efficiency_stderr(r["sumw_fixed"], ctx.moments(), r["counters"])
            effs.append(r["efficiencies"][idx])
            ses.append(se[idx])
    effs, ses = np.array(effs), np.array(ses)
    ratio = effs.std(axis=0, ddof=1) / np.sqrt((ses ** 2).mean(axis=0))
    return ratio


def test_calibration_xos1_10kev(pa):
    ratio = _calibrate(pa, _deck(pa, energies=[10.0]), [0])
    assert ((ratio >= 0.6) & (ratio <= 1.4)).all(), ratio


def test_calibration_291_energies(pa):
    prob = _deck(pa)
    assert prob.n_energies == 291
    idx = [0, 145, 290]
    ratio = _calibrate(pa, prob, idx)
    assert ((ratio >= 0.6) & (ratio <= 1.4)).all(), ratio

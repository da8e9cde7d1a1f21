"""Emit relays on the GPU (pc_hip_emit_*, TraceContext.emit): the confocal pair of tests/test_gpu_relay.py -- the ellipsoidal test optic
A and the same optic reversed, B -- with a thin sample sheet at 45 degrees in A's focus and B at 90 degrees, looking at the focus from
0.5 cm.

What carries correctness is the host round trip (test_same_photons_as_the_host_round_trip): the emit adds no arithmetic of its own
beyond the contract of include/polycap-hip.h, so its records, exact sums and counters must equal, bit for bit, the records and slot ids
of A fetched to the host, emitted by the host compile of pc_emit.h (tests/emit/emit_host.cpp), traced by pc_hip_launch_photons of B and
multiplied in numpy in the contract's order.

A CPU rehearsal with the oracle and numpy's own sampler (6000 slots, seed 20000, 10 keV) gave, of 6000 emitted photons: 579 out of B at
depth 0 (2072 absorbed, 1225 in the glass, 2112 outside), 427 / 443 at depth -+10 um, 45 at 30 um, 0 at 100 um.  The GPU's emit of the
GPU's run of A, with the contract's sampler: 572 (2185, 1154, 2075), 448 at 10 um, 27 at 30 um, 0 at 100 um; mean g 0.004299."""
import math

import numpy as np
import pytest

from tests.common import make_custom, make_pair
from tests.test_emit_cpu import INJECT, MISS_DETECTOR, MISS_SAMPLE, build_emit_host, host_emit
from tests.test_gpu_relay import SHAPE_B, SRC, as_ints, fixed_sums, problems, same_bits
from tests.test_relay_cpu import np_valid

pytestmark = pytest.mark.gpu

SEED, N = 20000, 6000
EMIT_SEED = 4242
GEOM = dict(focus=0.5, sample_angle=math.pi / 4., det_angle=math.pi / 2., wd=0.5)
COUNTER_KEYS = ("n_in", "exit", "absorbed", "glass", "outside", "error")
PINHOLE = dict(axis="r", d=0.5, centre=(0., 0.), range=(0., 0.0005))          # r < 5 um in A's focal plane


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_emit_host(tmp_path_factory.mktemp("emit_host"))


def emit(ctx_a, ctx_b, depth=0., offset=(0., 0.), seed=EMIT_SEED, **kw):
    g = dict(GEOM, **{k: kw.pop(k) for k in list(kw) if k in GEOM})
    return ctx_a.emit(ctx_b, g["focus"], g["sample_angle"], depth, g["det_angle"], g["wd"], offset, seed=seed, **kw)


def totals_key(r):
    c = r["counters"]
    return (r["counters_array"].tolist(), c["missed_sample"], c["missed_detector"], c["rejected"], as_ints(r["sumw_fixed"]),
            None if r["sumw2_fixed"] is None else as_ints(r["sumw2_fixed"]))


def round_trip(pa, host, rec_a, slots_a, ctx_b, depth=0., offset=(0., 0.), seed=EMIT_SEED, emap=None, passing=None, geom=GEOM):
    """the host round trip of an emit: records and slots of A (those at the positions `passing`, if given) -> host compile of the
    contract -> the missed ones dropped -> pc_hip_launch_photons of B -> products in the contract's order.  Returns a dict: the
    records the emit must have left, rc of the injected photons, their state, their entries in A's store, and the counts."""
    ne_b = ctx_b.problem.n_energies
    emap = np.arange(ne_b) if emap is None else np.asarray(emap)
    R = float(ctx_b.problem.ext[0])
    valid = np_valid(rec_a[:, 10], rec_a[:, 17])
    sel = np.ones(len(valid), dtype=bool)
    if passing is not None:
        sel[:] = False
        sel[passing] = True
    idx = np.flatnonzero(valid & sel)
    fr = pa.emit_frame(geom["focus"], geom["sample_angle"], depth, geom["det_angle"], geom["wd"], offset, R)["frame"]
    f, what = host_emit(host, rec_a[idx][:, [8, 9, 11, 12]], slots_a[idx].astype(np.uint64), fr, R, seed)
    hit = what == INJECT
    idx, f, ra = idx[hit], f[hit], rec_a[idx][hit]
    g = ctx_b.launch_photons(f[:, 0:3], f[:, 3:6], f[:, 6:9]) if len(idx) else None
    rc = g["rc"] if g is not None else np.zeros(0, dtype=np.int32)
    ok = rc == 1
    out = np.zeros((int(ok.sum()), 17 + ne_b))
    if g is not None:
        out[:, 0:2] = ra[ok, 0:2]
        out[:, 2:4], out[:, 4:6], out[:, 6:8] = f[ok, 0:2], f[ok, 3:5], f[ok, 6:8]
        out[:, 8:11], out[:, 11:13], out[:, 13:15] = g["exit_coords"][ok], g["exit_dir"][ok, 0:2], g["exit_elecv"][ok, 0:2]
        out[:, 15] = (ra[ok, 15].view(np.int64) + g["i_refl"][ok]).view(np.float64)
        out[:, 16] = ((ra[ok, 16] + f[ok, 9]) + f[ok, 10]) + g["d_travel"][ok]
        out[:, 17:] = (ra[ok][:, 17 + emap] * f[ok, 11][:, None]) * g["weights"][ok]
    return dict(records=out, rc=rc, state=f, entries=idx, n_in=len(idx), skipped=int((~valid).sum()), rejected=int((valid & ~sel).sum()),
                missed_sample=int((what == MISS_SAMPLE).sum()), missed_detector=int((what == MISS_DETECTOR).sum()), mean_g=float(f[:, 11].mean()) if len(f) else 0.)


def check_against_round_trip(pa, host, ctx_a, ctx_b, r, n_started, **kw):
    rec = ctx_b.records()
    t_b = ctx_b.totals()
    mom = ctx_b.moments() if r["sumw2_fixed"] is not None else None
    rec_a, slots_a = ctx_a.records(), ctx_a.slot_ids()
    w = round_trip(pa, host, rec_a, slots_a, ctx_b, **kw)              # (this launch replaces the emit on B)
    want, rc = w["records"], w["rc"]
    assert same_bits(rec, want), "emit records differ from the host round trip"
    c = r["counters"]
    for k in ("n_in", "skipped", "missed_sample", "missed_detector", "rejected"):
        assert c[k] == w[k], (k, c[k], w[k])
    assert c["missed"] == c["missed_sample"] + c["missed_detector"]
    assert c["n_in"] + c["skipped"] + c["missed_sample"] + c["missed_detector"] + c["rejected"] == rec_a.shape[0] and c["n_started_a"] == n_started
    assert (c["exit"], c["absorbed"], c["glass"], c["outside"], c["error"]) == tuple(int((rc == k).sum()) for k in (1, 0, 2, -2, -1))
    assert c["exit"] == rec.shape[0] == r["n_records"]
    A, B = fixed_sums(want[:, 17:])
    assert as_ints(r["sumw_fixed"]) == A and as_ints(t_b["sumw_fixed"]) == A
    if mom is not None:
        assert as_ints(r["sumw2_fixed"]) == B and as_ints(mom) == B
    assert list(t_b["counters"]) == [c["exit"], c["n_in"] - c["exit"] - c["absorbed"], c["absorbed"],
                                     int(want[:, 15].view(np.int64).sum()), 0, c["n_in"]]
    for e in range(len(A)):
        assert abs(r["efficiencies"][e] - A[e] / 2.0 ** 62 / n_started) <= 1e-15 * r["efficiencies"][e]
    return w


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinned", "ne12", "rough"])
def test_same_photons_as_the_host_round_trip(pa, oracle, host, name):
    _, _, prob_a, _, prob_b, _ = problems(oracle, name)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        for depth, off in ((0., (0., 0.)), (0.001, (0., 0.)), (0., (0.002, 0.))):
            r = emit(ctx_a, ctx_b, depth, off)
            assert r["efficiency_stderr"] is not None and np.all(r["efficiency_stderr"] >= 0.)
            w = check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], depth=depth, offset=off)
            print(name, depth, off, r["counters"], "eff", r["efficiencies"][:2], "+-", r["efficiency_stderr"][:2], "mean g", w["mean_g"],
                  "stage 2 ms", r["kernel_ms"])
            if depth == 0. and off == (0., 0.):
                c = r["counters"]
                assert c["exit"] > 100 and min(c[k] for k in ("absorbed", "glass", "outside")) > 0
                assert c["n_in"] == N and abs(w["mean_g"] - 0.0043) < 0.0002
        # a relay afterwards is the one it was, and says so
        plain = ctx_a.relay(ctx_b, 1.0)
        assert plain["counters"]["exit"] > 100 and "missed_sample" not in plain["counters"]


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_energy_map(pa, oracle, host):
    """excited at 20 keV, detected at three fluorescence lines: every energy of B takes A's one weight"""
    _, _, prob_a, _ = make_pair(oracle, "ellip", energies=(20.0,))
    _, _, prob_b, _ = make_custom(oracle, SHAPE_B, 200000, SRC, energies=(6.4, 8.05, 17.4))
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        r = emit(ctx_a, ctx_b, energy_map=[0, 0, 0])
        assert r["efficiencies"].shape == (3,) and r["counters"]["exit"] > 100
        check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], emap=[0, 0, 0])
        before = emit(ctx_a, ctx_b, energy_map=[0, 0, 0])
        assert totals_key(before) == totals_key(r)
        rec_before = ctx_b.records()
        for bad, match in ((None, "energy grid"), ([0, 0], "n_map"), ([0, 0, 0, 0], "n_map"), ([0, 1, 0], "map[1]"), ([0, 0, -1], "map[2]")):
            with pytest.raises(pa.HipError) as e:
                emit(ctx_a, ctx_b, energy_map=bad)
            assert e.value.status == -2 and match in str(e.value), str(e.value)
            assert totals_key(ctx_b.relay_totals()) == totals_key(before) and same_bits(ctx_b.records(), rec_before)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_launch_invariance(pa, oracle):
    """However A's run was stored and launched, the emit has bit-identical totals and counts and the same records -- in the same
    order, or after a compact run of A, whose positions are in the order of completion, as the same set: the random numbers are
    keyed by the slot, not by the position.  (4 x 65536 + 777 slots: fewer are not cut into four parts.)"""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    n = 4 * 65536 + 777
    base = None
    variants = [dict(), dict(plane_images=1, compact_images=1, slot_ids=1), dict(run_parts=4), dict(producer=1)]
    for opts in variants:
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_b.set_option("weight_squares", 1)
            for k, v in opts.items():
                ctx_a.set_option(k, v)
            ctx_a.run(SEED, 0, n, keep_images=True)
            r = emit(ctx_a, ctx_b, 0.0005)
            rec = ctx_b.records()
            if opts.get("producer"):
                assert ctx_a.KERNELS.get(int(pa.lib().pc_hip_last_kernel(ctx_a._h))) == ctx_a.KERNELS[2]
            if base is None:
                again = emit(ctx_a, ctx_b, 0.0005)
                assert totals_key(again) == totals_key(r) and same_bits(ctx_b.records(), rec)       # the same seed: the same bits
                other = emit(ctx_a, ctx_b, 0.0005, seed=EMIT_SEED + 1)
                assert other["counters"]["n_in"] == r["counters"]["n_in"] and as_ints(other["sumw_fixed"]) != as_ints(r["sumw_fixed"])
        key = totals_key(r)
        srt = rec[np.lexsort(rec.T[::-1])]                       # by src_start, then pc_start, ...
        if base is None:
            base = (key, rec, srt)
            assert r["counters"]["exit"] > 5000
            continue
        assert key == base[0], opts
        assert same_bits(srt, base[2]), opts
        if not opts.get("compact_images"):
            assert same_bits(rec, base[1]), opts


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_aperture_and_its_complement(pa, oracle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        with pa.Selection(ctx_a, [PINHOLE]) as S, pa.Selection(ctx_a, [dict(PINHOLE, **{"not": True})]) as Sn:
            tot = S.apply("exit")
            Sn.apply("exit")
            n_pass = int(tot["n_pass"][0])
            whole = emit(ctx_a, ctx_b)
            through = emit(ctx_a, ctx_b, select=S)
            around = emit(ctx_a, ctx_b, select=Sn)
            print("pinhole passes", n_pass, "whole", whole["counters"], "through", through["counters"], "around", around["counters"])
            for k in COUNTER_KEYS:
                assert through["counters"][k] + around["counters"][k] == whole["counters"][k], k
            ne = len(as_ints(whole["sumw_fixed"]))
            assert ne == 12
            for key in ("sumw_fixed", "sumw2_fixed"):
                a, b, c = as_ints(through[key]), as_ints(around[key]), as_ints(whole[key])
                assert [a[e] + b[e] for e in range(ne)] == c, key
            assert through["counters"]["exit"] > 20 and around["counters"]["exit"] > 20
            # rejected is counted, never missed: what one selection rejects is everything the other one lets to the sample
            assert whole["counters"]["rejected"] == 0
            for one, other in ((through, around), (around, through)):
                co, cn = one["counters"], other["counters"]
                assert co["rejected"] == cn["n_in"] + cn["missed_sample"] + cn["missed_detector"]
                assert co["n_in"] + co["skipped"] + co["missed_sample"] + co["missed_detector"] + co["rejected"] == N
            assert through["counters"]["rejected"] == N - whole["counters"]["skipped"] - n_pass
            for k in ("missed_sample", "missed_detector"):
                assert through["counters"][k] + around["counters"][k] == whole["counters"][k]


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_contexts_usable(pa, oracle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")

    def refused(a, b, match, **kw):
        with pytest.raises(pa.HipError) as e:
            emit(a, b, **kw)
        assert e.value.status == -2 and match in str(e.value), str(e.value)

    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b, pa.TraceContext(prob_a) as ctx_c:
        ctx_a.run(SEED, 0, N, keep_images=True)
        before = emit(ctx_a, ctx_b)
        rec_before = ctx_b.records()

        def still_the_same():
            # B still holds the emit it held, and the same emit gives the totals it gave
            assert totals_key(ctx_b.relay_totals()) == totals_key(before) and same_bits(ctx_b.records(), rec_before)
            assert totals_key(emit(ctx_a, ctx_b)) == totals_key(before)

        # an invalid spec
        for kw, match in ((dict(sample_angle=math.pi / 2.), "sample_angle"), (dict(det_angle=4.), "det_angle"), (dict(wd=0.), "wd"),
                          (dict(focus=-0.5), "focus"), (dict(depth=float("nan")), "depth"), (dict(offset=(0., float("inf"))), "off_v"),
                          (dict(target_half=0.), "target_half")):
            refused(ctx_a, ctx_b, match, **kw)
            still_the_same()
        # a compact A without its slots: the message names both remedies
        ctx_c.set_option("plane_images", 1)
        ctx_c.set_option("compact_images", 1)
        ctx_c.run(SEED, 0, N, keep_images=True)
        refused(ctx_c, ctx_b, "slot_ids")
        refused(ctx_c, ctx_b, "compact_images")
        still_the_same()
        ctx_c.set_option("slot_ids", 1)
        ctx_c.run(SEED, 0, N, keep_images=True)
        assert totals_key(emit(ctx_c, ctx_b)) == totals_key(before)      # (its records are in the compact store's order)
        assert totals_key(emit(ctx_a, ctx_b)) == totals_key(before)
        # an A whose last call was not a source run that kept images
        ctx_c.set_option("compact_images", 0)
        ctx_c.set_option("plane_images", 0)
        ctx_c.transmission(SEED, 0, N, keep_images=True, leak_calc=True)
        refused(ctx_c, ctx_b, "leak_calc")
        ctx_c.run(SEED, 0, N, keep_images=True)
        ctx_c.scan(SEED, pa.scan_points(x=(0., 0.01)), 1000)
        refused(ctx_c, ctx_b, "scan")
        ctx_a.relay(ctx_c, 1.0)
        refused(ctx_c, ctx_b, "result of a relay")
        refused(ctx_a, ctx_a, "context of its own")
        still_the_same()
        # selections
        with pa.Selection(ctx_b, [PINHOLE]) as Sb, pa.Selection(ctx_a, [PINHOLE]) as S:
            Sb.apply("exit")                                           # the emit's records on B are its kind 0
            refused(ctx_a, ctx_b, "another owner", select=Sb)
            still_the_same()
            refused(ctx_a, ctx_b, "was not applied for kind 0", select=S)
            still_the_same()
            S.apply("exit")
            good = emit(ctx_a, ctx_b, select=S)
            assert good["counters"]["rejected"] > 0 and good["counters"]["n_in"] > 0
            before, rec_before = emit(ctx_a, ctx_b), ctx_b.records()
            ctx_a.run(SEED, 0, N, keep_images=True)                    # the entries of A are replaced: the mask is stale
            refused(ctx_a, ctx_b, "mask is stale", select=S)
            still_the_same()
            S.apply("exit")
            assert totals_key(emit(ctx_a, ctx_b, select=S)) == totals_key(good)
            with pytest.raises(TypeError):
                emit(ctx_a, ctx_b, select="pinhole")
        if pa.device_count() > 1:
            with pa.TraceContext(prob_b, 1) as ctx_d:
                refused(ctx_a, ctx_d, "different devices")
        # pc_hip_emit_counts speaks of emit relays only
        emit(ctx_a, ctx_b)
        cnt = np.zeros(3, dtype=np.int64)
        import ctypes as C
        assert pa.lib().pc_hip_emit_counts(ctx_b._h, cnt.ctypes.data_as(C.POINTER(C.c_int64))) == 0
        ctx_a.relay(ctx_b, 1.0)
        assert pa.lib().pc_hip_emit_counts(ctx_b._h, cnt.ctypes.data_as(C.POINTER(C.c_int64))) == -2


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_depth_response(pa, oracle):
    """The probing volume of the pair: the response falls with the depth of the sheet behind the confocal point (the rehearsal's exit
    counts: 579, 427, 45, 0), one seed for all depths."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    depths = (0., 0.001, 0.003, 0.01)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        sc = pa.emit_depth_scan(ctx_a, ctx_b, depths, GEOM["focus"], GEOM["sample_angle"], GEOM["det_angle"], GEOM["wd"], seed=EMIT_SEED)
        single = emit(ctx_a, ctx_b, 0.001)
        inline = ctx_a.emit(ctx_b, 0.5, 0., 0., 0., 0.5, seed=EMIT_SEED)
    eff, err = sc["efficiencies"][:, 0], sc["efficiency_stderr"][:, 0]
    n_exit = [c["exit"] for c in sc["counters"]]
    print("depth", depths, "eff", eff, "+-", err, "exit", n_exit, "in line", inline["counters"])
    assert sc["depths"].shape == (4,) and sc["efficiencies"].shape == (4, 1) and len(sc["counters"]) == 4
    assert eff[1] == single["efficiencies"][0] and err[1] == single["efficiency_stderr"][0]
    assert np.all(np.diff(eff) < 0.)
    assert n_exit[0] > 100 and 20 * n_exit[3] <= n_exit[0]
    assert inline["counters"]["exit"] > 100


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_tallies_on_b(pa, oracle):
    from tests.test_gpu_beam import exact_sums
    from tests.test_gpu_hist import REGIMES, check, data_axes, record_entries
    from tests.test_gpu_spot import np_map
    from tests.test_spot_cpu import np_exit_dz
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    ze = float(prob_b.z[-1])
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.run(SEED, 0, N, keep_images=True)
        r = emit(ctx_a, ctx_b)
        rec = ctx_b.records()
        assert rec.shape[0] == r["n_records"] > 100
        window, dist = (-0.01, 0.012, -0.011, 0.01), [0., 0.3, 2.0]
        with pa.SpotMap(ctx_b, dist, window, (48, 40)) as m, pa.BeamMoments(ctx_b) as bm:
            m.add("exit")
            bm.add("exit")
            res, beam = m.read(), bm.read()
        E, W = record_entries(rec)
        axes = data_axes(E, W, ze)
        for regime in REGIMES:
            with pa.Histograms(ctx_b, axes, regime=regime) as h:
                h.add("exit")
                bins_h, out_h = check(h.read(), "exit", axes, E, W, ze, what="(emit, regime %d)" % regime)
    assert bins_h.any() and out_h.any()
    pos = rec[:, 8:11]
    dirs = np.stack([rec[:, 11], rec[:, 12], np_exit_dz(rec[:, 11], rec[:, 12])], axis=1)
    bins, out = np_map(pos, dirs, W, np.arange(W.shape[1]), [ze + d for d in dist], window, 48, 40)
    assert res["n_entries"] == rec.shape[0]
    assert np.array_equal(res["bins"], bins) and np.array_equal(res["outside"], out) and bins.sum() > 0
    lohi, outside, _ = exact_sums(pos, dirs, W, ze)
    assert np.array_equal(beam["sums"][0], lohi) and np.array_equal(beam["outside"][0], outside)
    assert int(beam["n_entries"][0]) == rec.shape[0]


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_oracle_second_stage(pa, oracle, host):
    """The injected photons of the GPU's emit (the host round trip's, bit-equal by test 1) through the oracle's B: the efficiency of
    the train from the GPU's exact sums and from the oracle's weights agree within 4 combined standard errors -- the GPU's from
    efficiency_stderr, the oracle's from its own weights over the same number of started photons."""
    _, _, prob_a, optic_b, prob_b, (E, A, S) = problems(oracle, "pinned")
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        r = emit(ctx_a, ctx_b)
        rec_a = ctx_a.records()
        w = round_trip(pa, host, rec_a, ctx_a.slot_ids(), ctx_b)
    f = w["state"]
    o = oracle.launch_batch(optic_b, E, A, S, f[:, 0:3], f[:, 3:6], f[:, 6:9])
    ok = o["rc"] == 1
    wo = (rec_a[w["entries"]][ok, 17] * f[ok, 11]) * o["weights"][ok, 0]
    n = ra["i_start"]
    eff_o = wo.sum() / n
    err_o = math.sqrt(max((wo * wo).sum() / n - eff_o * eff_o, 0.) / (n - 1))
    eff_g, err_g = r["efficiencies"][0], r["efficiency_stderr"][0]
    print("efficiency gpu %.6g +- %.2g (%d photons), oracle %.6g +- %.2g (%d photons), difference %.2f combined standard errors"
          % (eff_g, err_g, r["counters"]["exit"], eff_o, err_o, int(ok.sum()), (eff_g - eff_o) / math.hypot(err_g, err_o)))
    assert r["counters"]["exit"] > 100 and ok.sum() > 100
    assert abs(eff_g - eff_o) <= 4. * math.hypot(err_g, err_o)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_kinds_of_relay_share_one_state(pa, oracle):
    """Plain, posed and emit relays keep one state on the second context and share its scratch buffers.  A sequence of all three
    kinds into one B -- with a shorter run of A in the middle, so that every offset into the scratch shrinks -- leaves after every
    step what the same single call leaves on a B made for it: relay_totals (counters, missed, rejected, both exact sums),
    pc_hip_emit_counts (the three counts after an emit, status -2 after anything else), totals() and records(), bit for bit.
    The posed relay without a selection stands at gap 0: there the tilted entrance plane cuts A's exit face, and the photons on
    its far side miss it, so that `missed` is not zero without an aperture.  (On the MI355X: the pinhole rejects 1722 of the 2000
    and lets 278 in, of which 66 leave B; at gap 0 254 of the 500 miss and none of the other 246 leaves B; the emits inject
    every photon, 176 of 2000 and 50 of 500 leave B.)"""
    import ctypes as C
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    tilt = (0.003, 0.001)

    def state(ctx_b):
        r = ctx_b.relay_totals()
        c = r["counters"]
        el = np.zeros(3, dtype=np.int64)
        st = pa.lib().pc_hip_emit_counts(ctx_b._h, el.ctypes.data_as(C.POINTER(C.c_int64)))
        t = ctx_b.totals()
        return ((r["counters_array"].tolist(), c["missed"], c["rejected"], as_ints(r["sumw_fixed"]), as_ints(r["sumw2_fixed"])),
                (st, el.tolist() if st == 0 else None),
                (t["counters"].tolist(), as_ints(t["sumw_fixed"]), t["sum_weights"].tobytes()), ctx_b.records())

    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b, pa.Selection(ctx_a, [PINHOLE]) as S:
        ctx_b.set_option("weight_squares", 1)

        def step(name, call, acc_lds=1):
            ctx_b.set_option("relay_acc_lds", acc_lds)
            r = call(ctx_b)
            got = state(ctx_b)
            with pa.TraceContext(prob_b) as fresh:
                fresh.set_option("weight_squares", 1)
                fresh.set_option("relay_acc_lds", acc_lds)
                call(fresh)
                want = state(fresh)
            print(name, r["counters"], "emit counts", got[1])
            assert got[0] == want[0], (name, "relay_totals", got[0], want[0])
            assert got[1] == want[1], (name, "pc_hip_emit_counts", got[1], want[1])
            assert got[2] == want[2], (name, "totals", got[2], want[2])
            assert same_bits(got[3], want[3]), (name, "records")
            c = r["counters"]
            if name.startswith("emit"):
                assert got[1][0] == 0 and got[1][1] == [c["missed_sample"], c["missed_detector"], c["rejected"]]
                assert c["missed_detector"] + c["missed_sample"] >= 0 and c["n_in"] > 0
            else:
                assert got[1] == (-2, None)
            if name.startswith("posed"):
                assert c["missed"] + c["rejected"] > 0
            return r

        ctx_a.run(SEED, 0, 2000, keep_images=True)
        S.apply("exit")
        step("emit", lambda b: emit(ctx_a, b))
        r = step("posed, pinhole", lambda b: ctx_a.relay(b, 1.0, tilt=tilt, select=S))
        assert r["counters"]["rejected"] > 0 and r["counters"]["n_in"] > 0
        ctx_a.run(SEED, 0, 500, keep_images=True)
        step("emit, 500 slots", lambda b: emit(ctx_a, b))
        step("plain", lambda b: ctx_a.relay(b, 1.0))
        step("posed, no selection", lambda b: ctx_a.relay(b, 0., tilt=tilt))
        step("emit, sums to the global pairs", lambda b: emit(ctx_a, b), acc_lds=0)

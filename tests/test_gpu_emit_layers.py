"""Layered emits on the GPU (pc_hip_layers_*, TraceContext.emit with layers=): the confocal pair and the sizes of
tests/test_gpu_emit_slab.py with a stack of three layers of 5, 10 and 5 um behind the sheet, each with its own attenuation and its own
production coefficients, at +45 degrees (the emitted ray leaves through the back) and at -45 degrees (through the front).

What carries correctness is the host round trip, as for the slab: records and slot ids of A fetched to the host, emitted by the host
compile of pc_emit_layers.h (tests/emit_layers/emit_layers_host.cpp), traced by pc_hip_launch_photons of B and multiplied by the same
host compile, the prefix tables and the exponential included.  Records, exact sums, squares and counters must be equal bit for bit.
Beside it stand the identities no table-offset or layer-index error survives: exact additivity over the layers, one layer against the
slab emit, and splitting a layer."""
import math

import numpy as np
import pytest

from tests.common import make_custom, make_pair
from tests.test_emit_cpu import INJECT, MISS_DETECTOR, MISS_SAMPLE
from tests.test_emit_layers_cpu import L_A, L_B, L_CN, L_S, L_SD, Stack, build_layers_host, host_layers, host_layers_weight
from tests.test_gpu_emit import EMIT_SEED, GEOM, PINHOLE, emit, totals_key
from tests.test_gpu_emit_slab import mu_of, slab
from tests.test_gpu_relay import SHAPE_B, SRC, as_ints, fixed_sums, problems, same_bits
from tests.test_relay_cpu import np_valid

pytestmark = pytest.mark.gpu

SEED, N = 20000, 6000
TH = (0.0005, 0.001, 0.0005)                                # cm: 5, 10 and 5 um
E12 = np.linspace(5., 27., 12)
T2 = 2. ** -9                                               # cm (19.5 um): halves and quarters of it add up to it exactly


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_layers_host(tmp_path_factory.mktemp("emit_layers_host"))


def three_layers(host, en_a, en_b, production=None):
    """5, 10 and 5 um with three scales of the slab tests' table and three production rows"""
    mu_in = [mu_of(en_a, s) for s in (400., 90., 1500.)]
    mu_out = [mu_of(en_b, s) for s in (900., 200., 2500.)]
    if production is None:
        production = [np.linspace(0.5, 2., len(en_b)), np.linspace(7., 3., len(en_b)), np.full(len(en_b), 0.25)]
    return Stack(host, TH, mu_in, mu_out, production)


def layered(ctx_a, ctx_b, st, depth=0., **kw):
    return emit(ctx_a, ctx_b, depth, layers=st.as_layers(), **kw)


def round_trip(pa, host, rec_a, slots_a, ctx_b, st, depth=0., seed=EMIT_SEED, emap=None, passing=None, geom=GEOM):
    """the host round trip of a layered emit (tests/test_gpu_emit_slab.py::round_trip with the stack's state, weight and path)"""
    ne_b = ctx_b.problem.n_energies
    emap = np.arange(ne_b) if emap is None else np.asarray(emap)
    R = float(ctx_b.problem.ext[0])
    valid = np_valid(rec_a[:, 10], rec_a[:, 17])
    sel = np.ones(len(valid), dtype=bool)
    if passing is not None:
        sel[:] = False
        sel[passing] = True
    idx = np.flatnonzero(valid & sel)
    lib = pa.emit_layers_frame(geom["focus"], geom["sample_angle"], depth, geom["det_angle"], geom["wd"], (0., 0.), R, layers=st.as_layers())
    assert same_bits(lib["bounds"], st.Z) and lib["qmax"] == st.qmax
    f, what = host_layers(host, rec_a[idx][:, [8, 9, 11, 12]], slots_a[idx].astype(np.uint64), lib["frame"], R, st.Z, seed)
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
        out[:, 16] = (((ra[ok, 16] + f[ok, 9]) + f[ok, L_S]) + f[ok, 10]) + g["d_travel"][ok]
        for e in range(ne_b):
            out[:, 17 + e] = host_layers_weight(host, f[ok], ra[ok, 17 + emap[e]], g["weights"][ok, e], emap[e], e, st)
    return dict(records=out, rc=rc, state=f, entries=idx, n_in=len(idx), skipped=int((~valid).sum()), rejected=int((valid & ~sel).sum()),
                missed_sample=int((what == MISS_SAMPLE).sum()), missed_detector=int((what == MISS_DETECTOR).sum()))


def check_against_round_trip(pa, host, ctx_a, ctx_b, r, n_started, st, **kw):
    """tests/test_gpu_emit_slab.py::check_against_round_trip for a stack: the same assertions against the stack's round trip"""
    rec = ctx_b.records()
    t_b = ctx_b.totals()
    mom = ctx_b.moments() if r["sumw2_fixed"] is not None else None
    rec_a, slots_a = ctx_a.records(), ctx_a.slot_ids()
    w = round_trip(pa, host, rec_a, slots_a, ctx_b, st, **kw)                         # (this launch replaces the emit on B)
    want, rc = w["records"], w["rc"]
    assert same_bits(rec, want), "layered emit records differ from the host round trip"
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


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinned", "ne12", "rough"])
def test_same_photons_as_the_host_round_trip(pa, oracle, host, name):
    _, _, prob_a, _, prob_b, _ = problems(oracle, name)
    en = E12 if name == "ne12" else np.array([10.0])
    st = three_layers(host, en, en)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        for angle in (math.pi / 4., -math.pi / 4.):
            for depth in (0., -0.001):
                r = layered(ctx_a, ctx_b, st, depth, sample_angle=angle)
                assert r["efficiency_stderr"] is not None and np.all(r["efficiency_stderr"] >= 0.)
                w = check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], st, depth=depth, geom=dict(GEOM, sample_angle=angle))
                print(name, "angle %+.3f depth %g" % (angle, depth), r["counters"], "eff", r["efficiencies"][:2], "+-", r["efficiency_stderr"][:2])
                c = r["counters"]
                assert c["n_in"] == N and np.all(np.sign(w["state"][:, L_CN]) == (1. if angle > 0. else -1.))
                assert sorted(set(w["state"][:, 17])) == [0., 1., 2.]
                if depth == -0.001:
                    assert c["exit"] > 100 and min(c[k] for k in ("absorbed", "glass", "outside")) > 0
        plain = ctx_a.relay(ctx_b, 1.0)
        assert plain["counters"]["exit"] > 100 and "missed_sample" not in plain["counters"]


def test_energy_map(pa, oracle, host):
    """excited at 20 keV, detected at three fluorescence lines: mu_in has A's one energy, mu_out and production B's three"""
    _, _, prob_a, _ = make_pair(oracle, "ellip", energies=(20.0,))
    lines = (6.4, 8.05, 17.4)
    _, _, prob_b, _ = make_custom(oracle, SHAPE_B, 200000, SRC, energies=lines)
    st = three_layers(host, [20.], lines)
    assert st.mu_in.shape == (3, 1) and st.mu_out.shape == (3, 3)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        r = layered(ctx_a, ctx_b, st, -0.001, energy_map=[0, 0, 0])
        assert r["efficiencies"].shape == (3,) and r["counters"]["exit"] > 100
        check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], st, depth=-0.001, emap=[0, 0, 0])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def additivity(ctx_a, ctx_b, host, st, depth, min_records=100, **kw):
    """One emit with production 1 everywhere against one emit per layer with production 1 in that layer alone (qmax is 1 in every
    run, so the guard is the same): the same geometry bit for bit, every weight either the full run's double or +0, each photon's
    weights adding up bitwise and the integer sums exactly.  Returns the full run's result."""
    ones = np.ones_like(st.mu_out)
    full = layered(ctx_a, ctx_b, Stack(host, st.th, st.mu_in, st.mu_out, ones), depth, **kw)
    rec = ctx_b.records()
    assert rec.shape[0] > min_records
    acc = np.zeros_like(rec[:, 17:])
    sumw, sumw2 = [0] * st.n_out, [0] * st.n_out
    lit = []
    for j in range(st.n):
        q = np.zeros_like(st.mu_out)
        q[j] = 1.
        r = layered(ctx_a, ctx_b, Stack(host, st.th, st.mu_in, st.mu_out, q), depth, **kw)
        rj = ctx_b.records()
        assert r["counters"] == full["counters"] and same_bits(rj[:, :17], rec[:, :17])
        wj = rj[:, 17:]
        same = wj.view(np.uint64) == rec[:, 17:].view(np.uint64)
        zero = wj.view(np.uint64) == 0
        assert np.all(same | zero)
        on = ~zero.all(axis=1)
        assert np.all(same[on]), "a photon's weights come from one layer"
        lit.append(on)
        acc = acc + wj
        sumw = [a + b for a, b in zip(sumw, as_ints(r["sumw_fixed"]))]
        sumw2 = [a + b for a, b in zip(sumw2, as_ints(r["sumw2_fixed"]))]
    assert same_bits(acc, rec[:, 17:])
    assert sumw == as_ints(full["sumw_fixed"]) and sumw2 == as_ints(full["sumw2_fixed"])
    lit = np.array(lit)
    assert np.all(lit.sum(axis=0) <= 1)                                          # no photon in two layers
    if min_records > 0:
        assert np.all(lit.sum(axis=1) > 0)                                       # every layer lit
    return full


@pytest.mark.parametrize("angle", [math.pi / 4., -math.pi / 4.], ids=["back", "front"])
def test_exact_additivity_over_the_layers(pa, oracle, host, angle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    st = three_layers(host, E12, E12)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        additivity(ctx_a, ctx_b, host, st, -0.001, sample_angle=angle)


# ---- 3, 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [math.pi / 4., -math.pi / 4.], ids=["back", "front"])
def test_one_layer_is_the_slab_and_splitting_changes_nothing(pa, oracle, host, angle):
    """One layer with production 1 against the slab emit of the same contexts, which is the reference: counters equal, columns 0-16
    bit-equal; weights and efficiencies within 1e-12 relative.  The two formulas, mu*s + mu_out*s_out against (0 + mu*a)/sd + (0 +
    mu_out*b)/cn, differ by a handful of roundings, each of which moves the exponent by at most tau * 2^-53, and E is within 1e-14 of
    exp on both sides: with tau <= 10 (asserted below from the host compile's state) the true distance is below 1e-13, while a wrong
    face, layer or prefix moves a weight by percents.  With every mu zero the weights are bit-equal.  Then the same slab as two halves
    and as four quarters with identical tables (T = 2^-9 cm, so that the boundaries add up to T exactly): columns 0-16 bit-equal to the
    one-layer run, weights and efficiencies within the same 1e-12."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    mu_in, mu_out = mu_of(E12, 100.), mu_of(E12, 200.)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        ref = slab(ctx_a, ctx_b, mu_in, mu_out, -0.001, thickness=T2, sample_angle=angle)
        rec_ref = ctx_b.records()
        assert rec_ref.shape[0] > 100
        one = Stack(host, [T2], [mu_in], [mu_out])
        r1 = layered(ctx_a, ctx_b, one, -0.001, sample_angle=angle)
        rec1 = ctx_b.records()
        assert r1["counters"] == ref["counters"] and same_bits(rec1[:, :17], rec_ref[:, :17])
        assert close(rec1[:, 17:], rec_ref[:, 17:]) and close(r1["efficiencies"], ref["efficiencies"])
        # tau <= 10 for every injected photon at the softest energy, which has the largest coefficients
        R = float(ctx_b.problem.ext[0])
        rec_a = ctx_a.records()
        valid = np_valid(rec_a[:, 10], rec_a[:, 17])
        fr = pa.emit_layers_frame(GEOM["focus"], angle, -0.001, GEOM["det_angle"], GEOM["wd"], (0., 0.), R, layers=one.as_layers())["frame"]
        f, what = host_layers(host, rec_a[valid][:, [8, 9, 11, 12]], ctx_a.slot_ids()[valid].astype(np.uint64), fr, R, one.Z, EMIT_SEED)
        f = f[what == INJECT]
        tau = mu_in[0] * f[:, L_A] / f[:, L_SD] + mu_out[0] * np.where(f[:, L_CN] > 0., f[:, L_B], f[:, L_A]) / np.abs(f[:, L_CN])
        print("angle %+.3f: largest optical depth %.3f, largest relative distance of a weight from the slab's %.3g" % (
            angle, tau.max(), np.max(np.abs(rec1[:, 17:] - rec_ref[:, 17:]) / np.maximum(rec_ref[:, 17:], 1e-300))))
        assert len(f) == r1["counters"]["n_in"] and tau.max() <= 10.
        # every mu zero: bit-equal weights
        zero = np.zeros(12)
        ref0 = slab(ctx_a, ctx_b, zero, zero, -0.001, thickness=T2, sample_angle=angle)
        rec_ref0 = ctx_b.records()
        r0 = layered(ctx_a, ctx_b, Stack(host, [T2], [zero], [zero]), -0.001, sample_angle=angle)
        assert totals_key(r0) == totals_key(ref0) and same_bits(ctx_b.records(), rec_ref0)
        # splitting
        for parts in (2, 4):
            st = Stack(host, [T2 / parts] * parts, [mu_in] * parts, [mu_out] * parts)
            assert st.T == T2
            rp = layered(ctx_a, ctx_b, st, -0.001, sample_angle=angle)
            recp = ctx_b.records()
            assert rp["counters"] == r1["counters"] and same_bits(recp[:, :17], rec1[:, :17]), parts
            assert close(recp[:, 17:], rec1[:, 17:]) and close(rp["efficiencies"], r1["efficiencies"]), parts
            r0p = layered(ctx_a, ctx_b, Stack(host, [T2 / parts] * parts, [zero] * parts, [zero] * parts), -0.001, sample_angle=angle)
            assert totals_key(r0p) == totals_key(ref0) and same_bits(ctx_b.records(), rec_ref0), parts


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_launch_invariance(pa, oracle, host):
    """However A's run was stored and launched, the layered emit has bit-identical totals and counts and the same records: in the
    same order, or after a compact run of A, whose positions are in the order of completion, as the same set.  (4 x 65536 + 777
    slots: fewer are not cut into four parts.)  A compact A without slot ids is refused."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    n = 4 * 65536 + 777
    st = three_layers(host, [10.], [10.])
    base = None
    for opts in (dict(), dict(plane_images=1, compact_images=1, slot_ids=1), dict(run_parts=4), dict(plane_images=1, compact_images=1)):
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_b.set_option("weight_squares", 1)
            for k, v in opts.items():
                ctx_a.set_option(k, v)
            ctx_a.run(SEED, 0, n, keep_images=True)
            if opts.get("compact_images") and not opts.get("slot_ids"):
                with pytest.raises(pa.HipError) as e:
                    layered(ctx_a, ctx_b, st, -0.001)
                assert e.value.status == -2 and "slot_ids" in str(e.value)
                continue
            r = layered(ctx_a, ctx_b, st, -0.001)
            rec = ctx_b.records()
        key = totals_key(r)
        srt = rec[np.lexsort(rec.T[::-1])]
        if base is None:
            base = (key, rec, srt)
            assert r["counters"]["exit"] > 2000
            continue
        assert key == base[0], opts
        assert same_bits(srt, base[2]), opts
        if not opts.get("compact_images"):
            assert same_bits(rec, base[1]), opts


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_selection_as_an_aperture(pa, oracle, host):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    st = three_layers(host, E12, E12)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        with pa.Selection(ctx_a, [PINHOLE]) as Sel:
            tot = Sel.apply("exit")
            _, pos = Sel.gather(positions=True)
            assert 20 < len(pos) == int(tot["n_pass"][0]) < N
            r = layered(ctx_a, ctx_b, st, -0.001, select=Sel)
            assert r["counters"]["rejected"] > 0 and r["counters"]["n_in"] > 0
            check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], st, depth=-0.001, passing=pos)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_depth_scan(pa, oracle, host):
    """emit_depth_scan(layers=) over five depths is five emits, bit for bit in the exact sums.

    Production in the middle layer alone and every mu zero: the issue's first choice, equality with a slab emit of the middle layer
    alone placed at depth + Z_1, was NOT possible.  The shifted placement does not reproduce the frame's bits: the slab's frame holds
    the offset h_s of another plane and the thickness T_1 in the place of T, so that its photons interact at s = u3*T_1/sd behind
    another sheet, other points than the stack's u3*T/sd (asserted below: the frames differ).  The two runs estimate the same
    integral with different samples; their sums agree statistically, not bit for bit.  So the second choice is asserted: the exact
    additivity of test 2, at every depth of the scan."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    depths = (-0.002, -0.0015, -0.001, -0.0005, 0.)
    st = three_layers(host, [10.], [10.])
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        sc = pa.emit_depth_scan(ctx_a, ctx_b, depths, GEOM["focus"], GEOM["sample_angle"], GEOM["det_angle"], GEOM["wd"], seed=EMIT_SEED,
                                layers=st.as_layers())
        assert sc["efficiencies"].shape == (5, 1) and sc["efficiency_stderr"].shape == (5, 1) and len(sc["counters"]) == 5
        keys = []
        for k, d in enumerate(depths):
            r = layered(ctx_a, ctx_b, st, d)
            keys.append(as_ints(r["sumw_fixed"]))
            assert same_bits(r["efficiencies"], sc["efficiencies"][k]) and same_bits(r["efficiency_stderr"], sc["efficiency_stderr"][k])
            assert r["counters"] == sc["counters"][k]
        assert len(set(map(tuple, keys))) == 5 and max(c["exit"] for c in sc["counters"]) > 100
        # the scan's own exact sums: the last emit of the scan is what B holds
        sc2 = pa.emit_depth_scan(ctx_a, ctx_b, depths, GEOM["focus"], GEOM["sample_angle"], GEOM["det_angle"], GEOM["wd"], seed=EMIT_SEED,
                                 layers=st.as_layers())
        assert as_ints(ctx_b.relay_totals()["sumw_fixed"]) == keys[-1] and same_bits(sc2["efficiencies"], sc["efficiencies"])
        # production in the middle layer alone, no attenuation
        zero = np.zeros((3, 1))
        mid = Stack(host, TH, zero, zero, [[0.], [1.], [0.]])
        R = float(ctx_b.problem.ext[0])
        for d in depths:
            fl = pa.emit_layers_frame(GEOM["focus"], GEOM["sample_angle"], d, GEOM["det_angle"], GEOM["wd"], (0., 0.), R, layers=mid.as_layers())["frame"]
            fs = pa.emit_slab_frame(GEOM["focus"], GEOM["sample_angle"], d + mid.Z[1], GEOM["det_angle"], GEOM["wd"], (0., 0.), R, thickness=TH[1])["frame"]
            assert not same_bits(fl[:20], fs)
            full = additivity(ctx_a, ctx_b, host, Stack(host, TH, zero, zero), d, min_records=100 if d == -0.001 else 0)
            rm = layered(ctx_a, ctx_b, mid, d)
            assert rm["counters"] == full["counters"] and as_ints(rm["sumw_fixed"])[0] <= as_ints(full["sumw_fixed"])[0]
            if d == -0.001:
                assert 0 < as_ints(rm["sumw_fixed"])[0] < as_ints(full["sumw_fixed"])[0]


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_contexts_as_they_were(pa, oracle, host):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    st = three_layers(host, E12, E12)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b, pa.TraceContext(prob_a) as ctx_c:
        ctx_a.run(SEED, 0, N, keep_images=True)
        before = layered(ctx_a, ctx_b, st, -0.001)
        rec_before = ctx_b.records()
        tot_before = ctx_b.totals()
        counts_before = {k: before["counters"][k] for k in ("missed_sample", "missed_detector", "rejected")}

        def refused(a, match, layers=None, **kw):
            with pytest.raises(pa.HipError) as e:
                emit(a, ctx_b, kw.pop("depth", -0.001), layers=st.as_layers() if layers is None else layers, **kw)
            assert e.value.status == -2 and match in str(e.value), str(e.value)
            # B's totals and records are what they were, and pc_hip_emit_counts still answers for the emit before
            t = ctx_b.totals()
            now = ctx_b.relay_totals()
            assert totals_key(now) == totals_key(before) and same_bits(ctx_b.records(), rec_before)
            assert {k: now["counters"][k] for k in counts_before} == counts_before
            assert as_ints(t["sumw_fixed"]) == as_ints(tot_before["sumw_fixed"]) and list(t["counters"]) == list(tot_before["counters"])

        def changed(j, **kw):
            lay = st.as_layers()
            lay[j] = dict(lay[j], **kw)
            return lay

        refused(ctx_a, "n_mu_in", changed(0, mu_in=st.mu_in[0][:11])[:1])
        refused(ctx_a, "n_mu_out", [dict(l, mu_out=np.ones(13), production=np.ones(13)) for l in st.as_layers()])
        bad = st.mu_in[1].copy()
        bad[3] = -1.
        refused(ctx_a, "mu_in[1][3]", changed(1, mu_in=bad))
        bad = st.mu_out[2].copy()
        bad[11] = float("nan")
        refused(ctx_a, "mu_out[2][11]", changed(2, mu_out=bad))
        bad = st.prod[0].copy()
        bad[5] = float("inf")
        refused(ctx_a, "production[0][5]", changed(0, production=bad))
        refused(ctx_a, "thickness[1]", changed(1, thickness=0.))
        refused(ctx_a, "thickness[2]", changed(2, thickness=1.5))
        refused(ctx_a, "total thickness", changed(0, thickness=0.9995))
        refused(ctx_a, "n_layers", st.as_layers() * 6)
        refused(ctx_a, "n_layers", [])
        refused(ctx_a, "wd", wd=0.)
        refused(ctx_a, "map[0]", energy_map=[12] + [0] * 11)
        # a compact A without its slots
        ctx_c.set_option("plane_images", 1)
        ctx_c.set_option("compact_images", 1)
        ctx_c.run(SEED, 0, N, keep_images=True)
        refused(ctx_c, "slot_ids")
        # layers= excludes the slab's arguments
        for kw in (dict(thickness=0.002), dict(mu_in=st.mu_in[0]), dict(thickness=0.002, mu_in=st.mu_in[0], mu_out=st.mu_out[0])):
            with pytest.raises(ValueError):
                emit(ctx_a, ctx_b, layers=st.as_layers(), **kw)
        with pytest.raises(ValueError):
            pa.emit_depth_scan(ctx_a, ctx_b, (0.,), GEOM["focus"], GEOM["sample_angle"], GEOM["det_angle"], GEOM["wd"], layers=st.as_layers(), thickness=0.002)
        assert totals_key(ctx_b.relay_totals()) == totals_key(before) and same_bits(ctx_b.records(), rec_before)
        # a plain relay afterwards works and says what it is; and the same layered emit gives the totals it gave
        plain = ctx_a.relay(ctx_b, 1.0)
        assert plain["counters"]["exit"] > 100 and "missed_sample" not in plain["counters"]
        assert totals_key(layered(ctx_a, ctx_b, st, -0.001)) == totals_key(before)

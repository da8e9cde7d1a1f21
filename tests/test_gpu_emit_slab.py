"""Slab emits on the GPU (pc_hip_slab_*, TraceContext.emit with thickness, mu_in and mu_out): the confocal pair and the sizes of
tests/test_gpu_emit.py with a slab of 20 um behind the sheet, at +45 degrees (the emitted ray leaves through the back) and at -45
degrees (through the front, the reflection geometry).

What carries correctness is, as for the thin emit, the host round trip: records and slot ids of A fetched to the host, emitted by the
host compile of pc_emit.h (tests/emit_slab/emit_slab_host.cpp), traced by pc_hip_launch_photons of B and multiplied, the exponential
included, by the same host compile in the contract's order.  Records, exact sums, squares and counters must be equal bit for bit."""
import math

import numpy as np
import pytest

from tests.common import make_custom, make_pair
from tests.test_emit_cpu import INJECT, MISS_DETECTOR, MISS_SAMPLE
from tests.test_emit_slab_cpu import GL, S, SOUT, build_slab_host, host_slab, host_weight
from tests.test_gpu_emit import EMIT_SEED, GEOM, PINHOLE, emit, totals_key
from tests.test_gpu_relay import SHAPE_B, SRC, as_ints, fixed_sums, problems, same_bits
from tests.test_relay_cpu import np_valid

pytestmark = pytest.mark.gpu

SEED, N = 20000, 6000
T = 0.002                                                   # cm
E12 = np.linspace(5., 27., 12)


def mu_of(energies, scale):
    """a table that falls with the energy as attenuation does (1/cm), another number per energy; nothing physical about it"""
    return scale * (10. / np.asarray(energies, dtype=np.float64)) ** 2.7 + 3.


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_slab_host(tmp_path_factory.mktemp("emit_slab_host"))


def slab(ctx_a, ctx_b, mu_in, mu_out, depth=0., thickness=T, **kw):
    return emit(ctx_a, ctx_b, depth, thickness=thickness, mu_in=mu_in, mu_out=mu_out, **kw)


def round_trip(pa, host, rec_a, slots_a, ctx_b, mu_in, mu_out, depth=0., thickness=T, seed=EMIT_SEED, emap=None, passing=None, geom=GEOM):
    """the host round trip of a slab emit (tests/test_gpu_emit.py::round_trip with the slab's state, weight and path)"""
    ne_b = ctx_b.problem.n_energies
    emap = np.arange(ne_b) if emap is None else np.asarray(emap)
    mu_in, mu_out = np.asarray(mu_in, dtype=np.float64), np.asarray(mu_out, dtype=np.float64)
    R = float(ctx_b.problem.ext[0])
    valid = np_valid(rec_a[:, 10], rec_a[:, 17])
    sel = np.ones(len(valid), dtype=bool)
    if passing is not None:
        sel[:] = False
        sel[passing] = True
    idx = np.flatnonzero(valid & sel)
    fr = pa.emit_slab_frame(geom["focus"], geom["sample_angle"], depth, geom["det_angle"], geom["wd"], (0., 0.), R, thickness=thickness)["frame"]
    f, what = host_slab(host, rec_a[idx][:, [8, 9, 11, 12]], slots_a[idx].astype(np.uint64), fr, R, seed)
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
        out[:, 16] = (((ra[ok, 16] + f[ok, 9]) + f[ok, S]) + f[ok, 10]) + g["d_travel"][ok]
        for e in range(ne_b):
            out[:, 17 + e] = host_weight(host, ra[ok, 17 + emap[e]], f[ok, GL], mu_in[emap[e]], f[ok, S], mu_out[e], f[ok, SOUT], g["weights"][ok, e])
    return dict(records=out, rc=rc, state=f, entries=idx, n_in=len(idx), skipped=int((~valid).sum()), rejected=int((valid & ~sel).sum()),
                missed_sample=int((what == MISS_SAMPLE).sum()), missed_detector=int((what == MISS_DETECTOR).sum()))


def check_against_round_trip(pa, host, ctx_a, ctx_b, r, n_started, mu_in, mu_out, **kw):
    """tests/test_gpu_emit.py::check_against_round_trip for a slab: the same assertions against the slab's round trip"""
    rec = ctx_b.records()
    t_b = ctx_b.totals()
    mom = ctx_b.moments() if r["sumw2_fixed"] is not None else None
    rec_a, slots_a = ctx_a.records(), ctx_a.slot_ids()
    w = round_trip(pa, host, rec_a, slots_a, ctx_b, mu_in, mu_out, **kw)              # (this launch replaces the emit on B)
    want, rc = w["records"], w["rc"]
    assert same_bits(rec, want), "slab emit records differ from the host round trip"
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
    en = E12 if name == "ne12" else np.array([10.0])
    mu_in, mu_out = mu_of(en, 400.), mu_of(en, 900.)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        for angle in (math.pi / 4., -math.pi / 4.):
            for depth in (0., -0.001):
                r = slab(ctx_a, ctx_b, mu_in, mu_out, depth, sample_angle=angle)
                assert r["efficiency_stderr"] is not None and np.all(r["efficiency_stderr"] >= 0.)
                w = check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], mu_in, mu_out, depth=depth, geom=dict(GEOM, sample_angle=angle))
                print(name, "angle %+.3f depth %g" % (angle, depth), r["counters"], "eff", r["efficiencies"][:2], "+-", r["efficiency_stderr"][:2])
                c = r["counters"]
                assert c["n_in"] == N and w["state"][:, SOUT].min() >= 0.
                if depth == -0.001:
                    assert c["exit"] > 100 and min(c[k] for k in ("absorbed", "glass", "outside")) > 0
        # a relay afterwards is the one it was, and says so
        plain = ctx_a.relay(ctx_b, 1.0)
        assert plain["counters"]["exit"] > 100 and "missed_sample" not in plain["counters"]


def test_energy_map(pa, oracle, host):
    """excited at 20 keV, detected at three fluorescence lines: mu_in has A's one energy, mu_out B's three"""
    _, _, prob_a, _ = make_pair(oracle, "ellip", energies=(20.0,))
    lines = (6.4, 8.05, 17.4)
    _, _, prob_b, _ = make_custom(oracle, SHAPE_B, 200000, SRC, energies=lines)
    mu_in, mu_out = mu_of([20.], 400.), mu_of(lines, 900.)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        r = slab(ctx_a, ctx_b, mu_in, mu_out, -0.001, energy_map=[0, 0, 0])
        assert r["efficiencies"].shape == (3,) and r["counters"]["exit"] > 100
        check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], mu_in, mu_out, depth=-0.001, emap=[0, 0, 0])
        # the softest line is absorbed most on its way out
        r0 = slab(ctx_a, ctx_b, [0.], np.zeros(3), -0.001, energy_map=[0, 0, 0])
        loss = r["efficiencies"] / r0["efficiencies"]
        assert loss[0] < loss[1] < loss[2] < 1.


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_launch_invariance(pa, oracle):
    """However A's run was stored and launched, the slab emit has bit-identical totals and counts and the same records: in the same
    order, or after a compact run of A, whose positions are in the order of completion, as the same set.  (2 x 65536 + 777 slots:
    fewer are not cut into two parts.)"""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    n = 2 * 65536 + 777
    mu_in, mu_out = mu_of([10.], 400.), mu_of([10.], 900.)
    base = None
    for opts in (dict(), dict(plane_images=1, compact_images=1, slot_ids=1), dict(run_parts=2)):
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_b.set_option("weight_squares", 1)
            for k, v in opts.items():
                ctx_a.set_option(k, v)
            ctx_a.run(SEED, 0, n, keep_images=True)
            r = slab(ctx_a, ctx_b, mu_in, mu_out, -0.001)
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


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_attenuation_only_lowers_the_weights(pa, oracle):
    """One seed without and with attenuation: the geometry (every field of the records but the weights) is the same bit for bit,
    every weight is at most its value at mu = 0, and some are strictly smaller."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    zero = np.zeros(12)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.run(SEED, 0, N, keep_images=True)
        for angle in (math.pi / 4., -math.pi / 4.):
            r0 = slab(ctx_a, ctx_b, zero, zero, -0.001, sample_angle=angle)
            rec0 = ctx_b.records()
            r1 = slab(ctx_a, ctx_b, mu_of(E12, 400.), mu_of(E12, 900.), -0.001, sample_angle=angle)
            rec1 = ctx_b.records()
            assert r0["counters"] == r1["counters"] and rec0.shape == rec1.shape and rec0.shape[0] > 100
            assert same_bits(rec0[:, :17], rec1[:, :17])
            assert np.all(rec1[:, 17:] <= rec0[:, 17:]) and np.any(rec1[:, 17:] < rec0[:, 17:])
            assert np.all(r1["efficiencies"] < r0["efficiencies"])
            # the soft end of the grid loses more than the hard end
            assert r1["efficiencies"][0] / r0["efficiencies"][0] < r1["efficiencies"][11] / r0["efficiencies"][11]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_thin_emit_unchanged(pa, oracle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        first = emit(ctx_a, ctx_b, 0.001)
        rec_first = ctx_b.records()
        thick = slab(ctx_a, ctx_b, mu_of(E12, 400.), mu_of(E12, 900.), 0.001)
        assert totals_key(thick) != totals_key(first)
        third = emit(ctx_a, ctx_b, 0.001)
        assert totals_key(third) == totals_key(first) and same_bits(ctx_b.records(), rec_first)
        for k in ("efficiencies", "efficiency_stderr", "sum_weights"):
            assert same_bits(third[k], first[k]), k
        # a thin and a thick emit with one seed aim at the same target points
        slab(ctx_a, ctx_b, np.zeros(12), np.zeros(12), 0.001, thickness=1e-12)
        rec_thick = ctx_b.records()
        both = np.intersect1d(rec_thick[:, 0], rec_first[:, 0], return_indices=True)
        assert len(both[0]) > 100 and same_bits(rec_thick[both[1], 2:4], rec_first[both[2], 2:4])
        plain = ctx_a.relay(ctx_b, 1.0)
        assert plain["counters"]["exit"] > 100 and "missed_sample" not in plain["counters"]


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_selection_as_an_aperture(pa, oracle, host):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    mu_in, mu_out = mu_of(E12, 400.), mu_of(E12, 900.)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        with pa.Selection(ctx_a, [PINHOLE]) as Sel:
            tot = Sel.apply("exit")
            _, pos = Sel.gather(positions=True)
            assert 20 < len(pos) == int(tot["n_pass"][0]) < N
            r = slab(ctx_a, ctx_b, mu_in, mu_out, -0.001, select=Sel)
            assert r["counters"]["rejected"] > 0 and r["counters"]["n_in"] > 0
            check_against_round_trip(pa, host, ctx_a, ctx_b, r, ra["i_start"], mu_in, mu_out, depth=-0.001, passing=pos)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_contexts_as_they_were(pa, oracle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    mu_in, mu_out = mu_of(E12, 400.), mu_of(E12, 900.)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b, pa.TraceContext(prob_a) as ctx_c:
        ctx_a.run(SEED, 0, N, keep_images=True)
        before = slab(ctx_a, ctx_b, mu_in, mu_out, -0.001)
        rec_before = ctx_b.records()
        tot_before = ctx_b.totals()

        def refused(a, match, **kw):
            args = dict(dict(mu_in=mu_in, mu_out=mu_out, depth=-0.001), **kw)
            with pytest.raises(pa.HipError) as e:
                slab(a, ctx_b, **args)
            assert e.value.status == -2 and match in str(e.value), str(e.value)
            # B's totals and records are what they were
            t = ctx_b.totals()
            assert totals_key(ctx_b.relay_totals()) == totals_key(before) and same_bits(ctx_b.records(), rec_before)
            assert as_ints(t["sumw_fixed"]) == as_ints(tot_before["sumw_fixed"]) and list(t["counters"]) == list(tot_before["counters"])

        refused(ctx_a, "n_mu_in", mu_in=mu_in[:11])
        refused(ctx_a, "n_mu_out", mu_out=np.concatenate([mu_out, [1.]]))
        bad = mu_in.copy()
        bad[3] = -1.
        refused(ctx_a, "mu_in[3]", mu_in=bad)
        bad = mu_out.copy()
        bad[11] = float("nan")
        refused(ctx_a, "mu_out[11]", mu_out=bad)
        refused(ctx_a, "thickness", thickness=0.)
        refused(ctx_a, "thickness", thickness=1.5)
        refused(ctx_a, "wd", wd=0.)
        # a compact A without its slots
        ctx_c.set_option("plane_images", 1)
        ctx_c.set_option("compact_images", 1)
        ctx_c.run(SEED, 0, N, keep_images=True)
        refused(ctx_c, "slot_ids")
        with pytest.raises(ValueError):
            emit(ctx_a, ctx_b, thickness=T)
        with pytest.raises(ValueError):
            emit(ctx_a, ctx_b, mu_in=mu_in, mu_out=mu_out)
        # and the same slab emit gives the totals it gave
        assert totals_key(slab(ctx_a, ctx_b, mu_in, mu_out, -0.001)) == totals_key(before)
        # a depth scan forwards the three arguments
        sc = pa.emit_depth_scan(ctx_a, ctx_b, (-0.001, 0.), GEOM["focus"], GEOM["sample_angle"], GEOM["det_angle"], GEOM["wd"], seed=EMIT_SEED,
                                thickness=T, mu_in=mu_in, mu_out=mu_out)
        assert same_bits(sc["efficiencies"][0], before["efficiencies"]) and sc["efficiencies"].shape == (2, 12)

"""Relays on the GPU (pc_hip_relay_*, TraceContext.relay): the exit beam of the ellipsoidal test optic A through the same optic
reversed, B, whose entrance looks at A's focus 0.5 cm behind A's exit (a confocal pair).

What carries correctness is test_same_photons_as_the_host_round_trip: the relay adds no arithmetic of its own beyond the contract
of include/polycap-hip.h, so its records and exact totals must equal, bit for bit, the records of A fetched to the host, flown by
the host compile of pc_relay.h, traced by pc_hip_launch_photons of B and multiplied there.

Floors of the comparison with the CPU oracle (test_oracle_second_stage).  B is an optic no earlier bound was measured on, so the
oracle's own self-noise was measured on it, on the photons of the ORACLE's run of A (seed 20000, slots 0..19999, numpy transform,
gap 1 cm, aligned; oracle launch_batch on B against the same with one start coordinate moved by 1 ulp -- x up, x down, y up, y
down; the largest of the four).  scripts/relay_floors.py re-measures them (CPU only), and
tests/test_relay_cpu.py::test_oracle_floors_are_the_ones_the_gpu_test_uses keeps the constants below tied to it.  The GPU test
flies the GPU's run of A through B: the same seed and slots and so the same population of exit photons, but not photon for photon
the same (A's own trace is chaotic), which is why a floor is a share of a population, not a list of photons:
    config        rc 1    share of rc / i_refl flips    |delta| / sum * sqrt(n) of the transmitted weight (largest energy)
    pinned 10 keV 4885    0.0119                        0.0027
    12 energies   9741    0.0438                        0.0051
    rough B (5 A) 4777    0.0115                        0.0071
Entrance decisions (rc 2 / -2) were identical under every perturbation.  The kernel differs from the oracle by rounding only, so
its flip share is capped by the oracle's own; the weight bound is the floor times the margin test_explicit_photons_vs_oracle has
over its floor (1.0 against 0.25 = 4).  The flip caps are the issue's rule and leave a handful of photons of room (observed 0.01155,
0.0436, 0.0112): the runs are deterministic, but a compiler that rounds one operation of the trace kernel differently may move them
across; re-measure with the script before touching a cap."""
import os

import numpy as np
import pytest

from tests.common import make_custom, make_pair
from tests.test_relay_cpu import build_relay_host, host_fly, np_valid

pytestmark = pytest.mark.gpu

SHAPE_B = (2, 9., 0.0585, 0.2065, 9.9153e-5, 0.00035, 0.5, 1000.)      # tests/common.py:TEST_SHAPE reversed
SRC = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)
SEED, N = 20000, 20000
E12 = tuple(np.linspace(5., 27., 12))
#            energies, sig_rough of B, flip cap, weight floor
CONFIGS = {"pinned": ((10.0,), 0., 0.0119, 0.0027), "ne12": (E12, 0., 0.0438, 0.0051), "rough": ((10.0,), 5., 0.0115, 0.0071)}
PLACEMENTS = ((1.0, 0.), (1.0, 0.002), (1.0, 0.01), (0.8, 0.), (1.2, 0.))
# the oracle's table for these placements (rc 1, 0, 2, -2, -1), pinned config
ORACLE_TABLE = {(1.0, 0.): (4885, 9041, 5920, 137, 17), (1.0, 0.002): (2609, 11369, 5838, 174, 10), (1.0, 0.01): (2, 13331, 5765, 881, 21),
                (0.8, 0.): (253, 13791, 5936, 0, 20), (1.2, 0.): (357, 10264, 4534, 4813, 32)}


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_relay_host(tmp_path_factory.mktemp("relay_host"))


def problems(oracle, name):
    en, rough = CONFIGS[name][0], CONFIGS[name][1]
    optic_a, src, prob_a, eas = make_pair(oracle, "ellip", energies=en)
    optic_b, _, prob_b, _ = make_custom(oracle, SHAPE_B, 200000, SRC, energies=en, sig_rough=rough)
    return optic_a, src, prob_a, optic_b, prob_b, eas


def fixed_sums(W):
    """Python-integer sums of (uint64)(w * 2^62) and of (uint64)((w * w) * 2^62) per energy"""
    a = (W * 2.0 ** 62).astype(np.uint64)
    b = ((W * W) * 2.0 ** 62).astype(np.uint64)
    return [sum(int(v) for v in a[:, e]) for e in range(W.shape[1])], [sum(int(v) for v in b[:, e]) for e in range(W.shape[1])]


def as_ints(lohi):
    return [int(lo) + (int(hi) << 64) for lo, hi in np.asarray(lohi).reshape(-1, 2)]


def round_trip(host, rec_a, ctx_b, gap, off):
    """the host round trip: records of A -> host compile of the contract -> pc_hip_launch_photons of B -> products.
    Returns the records the relay must have left, and rc, the valid mask."""
    ne = rec_a.shape[1] - 17
    valid = np_valid(rec_a[:, 10], rec_a[:, 17])
    ra = rec_a[valid]
    f = host_fly(host, ra[:, [8, 9, 11, 12, 13, 14]], gap, off[0], off[1])
    g = ctx_b.launch_photons(f[:, 0:3], f[:, 3:6], f[:, 6:9])
    ok = g["rc"] == 1
    out = np.zeros((int(ok.sum()), 17 + ne))
    out[:, 0:2] = ra[ok, 0:2]
    out[:, 2:4], out[:, 4:6], out[:, 6:8] = f[ok, 0:2], f[ok, 3:5], f[ok, 6:8]
    out[:, 8:11], out[:, 11:13], out[:, 13:15] = g["exit_coords"][ok], g["exit_dir"][ok, 0:2], g["exit_elecv"][ok, 0:2]
    out[:, 15] = (ra[ok, 15].view(np.int64) + g["i_refl"][ok]).view(np.float64)
    out[:, 16] = (ra[ok, 16] + f[ok, 9]) + g["d_travel"][ok]
    out[:, 17:] = ra[ok, 17:] * g["weights"][ok]
    return out, g["rc"], valid


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_relay_against_round_trip(host, ctx_a, ctx_b, gap, off, r, n_started):
    rec = ctx_b.records()
    t_b = ctx_b.totals()
    mom = ctx_b.moments() if r["sumw2_fixed"] is not None else None
    want, rc, valid = round_trip(host, ctx_a.records(), ctx_b, gap, off)       # (this launch replaces the relay on B)
    assert same_bits(rec, want), "relay records differ from the host round trip"
    c = r["counters"]
    assert c["n_in"] == int(valid.sum()) and c["skipped"] == int((~valid).sum()) and c["n_started_a"] == n_started
    assert (c["exit"], c["absorbed"], c["glass"], c["outside"], c["error"]) == tuple(int((rc == k).sum()) for k in (1, 0, 2, -2, -1))
    assert c["exit"] == rec.shape[0] == r["n_records"]
    A, B = fixed_sums(want[:, 17:])
    assert as_ints(r["sumw_fixed"]) == A
    assert as_ints(t_b["sumw_fixed"]) == A
    if mom is not None:
        assert as_ints(r["sumw2_fixed"]) == B and as_ints(mom) == B
    assert list(t_b["counters"]) == [c["exit"], c["n_in"] - c["exit"] - c["absorbed"], c["absorbed"],
                                     int(want[:, 15].view(np.int64).sum()), 0, c["n_in"]]
    for e in range(len(A)):
        assert abs(r["efficiencies"][e] - A[e] / 2.0 ** 62 / n_started) <= 1e-15 * r["efficiencies"][e]
    return want, rc


@pytest.mark.parametrize("name", ["pinned", "ne12", "rough"])
def test_same_photons_as_the_host_round_trip(pa, oracle, host, name):
    _, _, prob_a, _, prob_b, _ = problems(oracle, name)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        for gap, ox in PLACEMENTS if name == "pinned" else PLACEMENTS[:2]:
            r = ctx_a.relay(ctx_b, gap, (ox, 0.))
            assert r["efficiency_stderr"] is not None and np.all(r["efficiency_stderr"] >= 0.)
            want, rc = check_relay_against_round_trip(host, ctx_a, ctx_b, gap, (ox, 0.), r, ra["i_start"])
            print(name, gap, ox, r["counters"], "eff", r["efficiencies"][:2], "+-", r["efficiency_stderr"][:2], "stage 2 ms", r["kernel_ms"])
            if (gap, ox) == (1.0, 0.):
                assert r["counters"]["exit"] > 1000 and min(r["counters"][k] for k in ("absorbed", "glass", "outside")) > 0


def test_skipped_slots_of_a_failed_run(pa, oracle, host):
    """max_attempts 1 on A: most slots fail; the relay skips and counts them, in the slot-ordered and in the compact store"""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    got = []
    for planes, compact in ((0, 0), (1, 1)):
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_a.set_option("plane_images", planes)
            ctx_a.set_option("compact_images", compact)
            ctx_a.run(SEED, 0, N, max_attempts=1, keep_images=True)
            ctx_a.wait()
            ta = ctx_a.totals(check=False)
            assert ta["failed_slots"] > N // 2
            r = ctx_a.relay(ctx_b, 1.0)
            assert r["counters"]["skipped"] == ta["failed_slots"] and r["counters"]["n_in"] == ta["i_exit"]
            assert r["counters"]["n_started_a"] == ta["i_start"] <= N
            rec = ctx_b.records()
            got.append((r, rec[np.lexsort(rec.T[::-1])]))
            if not planes:
                check_relay_against_round_trip(host, ctx_a, ctx_b, 1.0, (0., 0.), r, ta["i_start"])
    assert np.array_equal(got[0][0]["sumw_fixed"], got[1][0]["sumw_fixed"]) and same_bits(got[0][1], got[1][1])


def test_launch_invariance(pa, oracle):
    """However A's run was stored and launched and whatever the block size, the relay's totals are bit-identical and its records
    equal in the same order -- after a compact run of A, whose positions are in the order of completion, as the same set."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    n = 4 * 65536 + 777                       # enough slots for run_parts 4
    base = None
    variants = [dict(), dict(plane_images=1), dict(plane_images=1, compact_images=1), dict(run_parts=4), dict(block_size=256),
                dict(plane_images=1, run_parts=4, block_size=256), dict(relay_acc_lds=0)]
    for opts in variants:
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_b.set_option("weight_squares", 1)
            for k, v in opts.items():
                (ctx_b if k == "relay_acc_lds" else ctx_a).set_option(k, v)      # relay_acc_lds 0: sums straight to the global pairs
            if "block_size" in opts:
                ctx_b.set_option("block_size", opts["block_size"])
            ctx_a.run(SEED, 0, n, keep_images=True)
            r = ctx_a.relay(ctx_b, 1.0, (0.001, 0.))
            rec = ctx_b.records()
        key = (r["counters_array"].tolist(), as_ints(r["sumw_fixed"]), as_ints(r["sumw2_fixed"]))
        if base is None:
            base = (key, rec)
            assert r["counters"]["exit"] > 10000
            continue
        assert key == base[0], opts
        if opts.get("compact_images"):
            assert same_bits(rec[np.lexsort(rec.T[::-1])], base[1][np.lexsort(base[1].T[::-1])]), opts
        else:
            assert same_bits(rec, base[1]), opts


@pytest.mark.parametrize("name", ["pinned", "ne12", "rough"])
def test_oracle_second_stage(pa, oracle, name):
    """The same photons (the GPU run of A) through the oracle's B and through the relay: see the module docstring for the floors."""
    from tests.test_relay_cpu import np_fly
    _, _, prob_a, optic_b, prob_b, (E, A, S) = problems(oracle, name)
    flip_cap, c_floor = CONFIGS[name][2], CONFIGS[name][3]
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.transmission(SEED, 0, N, keep_images=True)
        ra = ctx_a.records()
        r = ctx_a.relay(ctx_b, 1.0)
        rec = ctx_b.records()
        f = np_fly(*(ra[:, k] for k in (8, 9, 11, 12, 13, 14)), 1.0, 0., 0.)
        g = ctx_b.launch_photons(f[:, 0:3], f[:, 3:6], f[:, 6:9])          # per-photon view of the relay's second stage (bit-equal, see above)
    o = oracle.launch_batch(optic_b, E, A, S, f[:, 0:3], f[:, 3:6], f[:, 6:9])
    ent_o = np.isin(o["rc"], (2, -2))
    assert np.array_equal(ent_o, np.isin(g["rc"], (2, -2)))
    assert np.array_equal(o["rc"][ent_o], g["rc"][ent_o])
    flips = ((o["rc"] != g["rc"]) | (o["i_refl"] != g["i_refl"])).mean()
    so = (ra[:, 17:] * o["weights"])[o["rc"] == 1].sum(axis=0)
    sg = rec[:, 17:].sum(axis=0)
    c = np.abs(sg - so) / so * np.sqrt(N)
    print(name, "flips", flips, "cap", flip_cap, "c", c.max(), "bound", 4. * c_floor, "rc 1 oracle", int((o["rc"] == 1).sum()), "relay", r["counters"]["exit"])
    assert flips <= flip_cap, (name, flips)
    assert c.max() <= 4. * c_floor, (name, c)
    assert abs(r["counters"]["exit"] - int((o["rc"] == 1).sum())) <= flip_cap * N


def test_response_shape(pa, oracle):
    """The confocal response is sharp in depth and sideways, and the GPU's counts follow the oracle's own (oracle run of A, numpy
    transform, oracle B: the table of the five placements) within the flip share of B, class by class."""
    from tests.test_relay_cpu import np_fly
    optic_a, src, prob_a, optic_b, prob_b, (E, A, S) = problems(oracle, "pinned")
    o = oracle.transmission(optic_a, src, E, A, S, SEED, 0, N, images=True)
    im = o["images"]
    counts = {}
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.run(SEED, 0, N, keep_images=True)
        for gap, ox in PLACEMENTS:
            c = ctx_a.relay(ctx_b, gap, (ox, 0.))["counters"]
            counts[(gap, ox)] = c
            f = np_fly(im[:, 8], im[:, 9], im[:, 11], im[:, 12], im[:, 13], im[:, 14], gap, ox, 0.)
            ob = oracle.launch_batch(optic_b, E, A, S, f[:, 0:3], f[:, 3:6], f[:, 6:9])
            table = tuple(int((ob["rc"] == k).sum()) for k in (1, 0, 2, -2, -1))
            assert table == ORACLE_TABLE[(gap, ox)]
            print(gap, ox, "gpu", c, "oracle", table)
            # every class, rc -1 included, within the flip share measured on B (module docstring): 238 photons of 20000
            for k, name in enumerate(("exit", "absorbed", "glass", "outside", "error")):
                assert abs(c[name] - table[k]) <= CONFIGS["pinned"][2] * N, (gap, ox, name, c[name], table[k])
    peak = counts[(1.0, 0.)]["exit"]
    for other in ((0.8, 0.), (1.2, 0.), (1.0, 0.01)):
        assert peak > 10 * counts[other]["exit"], (other, counts[other])


def test_spot_map_and_beam_moments_of_a_relay(pa, oracle):
    from tests.test_gpu_beam import exact_sums
    from tests.test_gpu_spot import np_map
    from tests.test_spot_cpu import np_exit_dz
    for name in ("pinned", "ne12"):
        _, _, prob_a, _, prob_b, _ = problems(oracle, name)
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_a.run(SEED, 0, N, keep_images=True)
            r = ctx_a.relay(ctx_b, 1.0)
            window, dist = (-0.01, 0.012, -0.011, 0.01), [0., 0.3, 2.0]
            with pa.SpotMap(ctx_b, dist, window, (48, 40)) as m, pa.BeamMoments(ctx_b) as bm:
                m.add("exit")
                bm.add("exit")
                res, beam = m.read(), bm.read()
            rec = ctx_b.records()
            im = ctx_b.images()
            assert same_bits(im["exit_weights"], rec[:, 17:]) and same_bits(im["images"][:, :15], rec[:, :15])
        assert rec.shape[0] == r["n_records"] > 1000
        pos = rec[:, 8:11]
        dirs = np.stack([rec[:, 11], rec[:, 12], np_exit_dz(rec[:, 11], rec[:, 12])], axis=1)
        W = rec[:, 17:]
        ze = float(prob_b.z[-1])
        bins, out = np_map(pos, dirs, W, np.arange(W.shape[1]), [ze + d for d in dist], window, 48, 40)
        assert res["n_entries"] == rec.shape[0]
        assert np.array_equal(res["bins"], bins) and np.array_equal(res["outside"], out)
        assert bins.sum() > 0
        lohi, outside, _ = exact_sums(pos, dirs, W, ze)
        assert np.array_equal(beam["sums"][0], lohi) and np.array_equal(beam["outside"][0], outside)
        assert int(beam["n_entries"][0]) == rec.shape[0]


def test_refusals_leave_both_contexts_usable(pa, oracle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    _, _, prob_a12, _, _, _ = problems(oracle, "ne12")
    en2 = (np.nextafter(10.0, 11.0),)
    _, _, prob_b_off, _ = make_custom(oracle, SHAPE_B, 200000, SRC, energies=(10.0,))
    prob_b_off2 = pa.Problem(prob_b_off.z, prob_b_off.cap, prob_b_off.ext, 0., 200000, 2.23, en2, [42.544635], [0.503696], *SRC)

    def refused(a, b, gap=1.0, off=(0., 0.), match=""):
        with pytest.raises(pa.HipError) as e:
            a.relay(b, gap, off)
        assert e.value.status == -2 and match in str(e.value), str(e.value)

    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        pin_a = ctx_a.transmission(SEED, 0, N, keep_images=True)
        pin_b = ctx_b.transmission(SEED, 0, N)
        pinned = (pin_a["sumw_fixed"].copy(), pin_a["counters"].copy(), pin_b["sumw_fixed"].copy(), pin_b["counters"].copy())
        refused(ctx_a, ctx_b, -0.5, match="gap")
        refused(ctx_a, ctx_b, float("nan"), match="gap")
        refused(ctx_a, ctx_b, 1.0, (float("inf"), 0.), match="finite")
        refused(ctx_a, ctx_a, match="context of its own")
        with pa.TraceContext(prob_a12) as ctx_12:
            refused(ctx_a, ctx_12, match="energy grid")
        with pa.TraceContext(prob_b_off2) as ctx_e:
            refused(ctx_a, ctx_e, match="energy grid")
        if pa.device_count() > 1:
            with pa.TraceContext(prob_b, 1) as ctx_d:
                refused(ctx_a, ctx_d, match="different devices")
        refused(ctx_b, ctx_a, match="kept no exit photons")               # B's last run kept no images
        with pytest.raises(pa.HipError):
            ctx_b.relay_totals()                                           # no relay into B yet
        # the refusals changed nothing: a relay still works, and source runs give their pinned totals
        ok = ctx_a.relay(ctx_b, 1.0)
        assert ok["counters"]["exit"] > 1000
        refused(ctx_b, ctx_a, match="result of a relay")                   # relays are not chained
        # what the relay was made with decides what its totals hold, whatever the option says later
        assert ctx_b.relay_totals()["sumw2_fixed"] is None
        ctx_b.set_option("weight_squares", 1)
        again = ctx_b.relay_totals()
        assert again["sumw2_fixed"] is None and np.array_equal(again["sumw_fixed"], ok["sumw_fixed"])
        ctx_b.set_option("weight_squares", 0)
        ctx_b.scan(SEED, pa.scan_points(x=(0., 0.01)), 1000)
        with pytest.raises(pa.HipError):
            ctx_b.relay_totals()                                           # the last call into B is a scan now
        ctx_a.transmission(SEED, 0, N, keep_images=True, leak_calc=True)
        refused(ctx_a, ctx_b, match="leak_calc")
        ctx_a.transmission(SEED, 0, N, keep_images=True)
        ctx_a.launch_photons([[0., 0., 0.]], [[0., 0., 1.]], [[1., 0., 0.]])
        refused(ctx_a, ctx_b, match="explicit-photon")
        ctx_a.transmission(SEED, 0, N, keep_images=True)
        ctx_a.scan(SEED, pa.scan_points(x=(0., 0.01)), 1000)
        refused(ctx_a, ctx_b, match="scan")
        ctx_a.transmission(SEED, 0, N, keep_images=False)
        refused(ctx_a, ctx_b, match="kept no exit photons")
        with pa.TraceContext(prob_a) as fresh:
            refused(fresh, ctx_b, match="no source run")
        after_a = ctx_a.transmission(SEED, 0, N, keep_images=True)
        after_b = ctx_b.transmission(SEED, 0, N)
        assert np.array_equal(after_a["sumw_fixed"], pinned[0]) and np.array_equal(after_a["counters"], pinned[1])
        assert np.array_equal(after_b["sumw_fixed"], pinned[2]) and np.array_equal(after_b["counters"], pinned[3])
        with pytest.raises(pa.HipError):
            ctx_b.relay_totals()                                           # a source run replaced the relay


def test_empty_relay(pa, oracle):
    """An offset of 0.1 cm puts A's focus outside B's acceptance: the oracle transmits nothing there (134 photons absorbed, 55 in
    the glass, 19808 outside the optic; a few still get through at 0.05 cm).  A valid result with zero records."""
    from tests.test_relay_cpu import np_fly
    optic_a, src, prob_a, optic_b, prob_b, (E, A, S) = problems(oracle, "pinned")
    o = oracle.transmission(optic_a, src, E, A, S, SEED, 0, N, images=True)
    im = o["images"]
    f = np_fly(im[:, 8], im[:, 9], im[:, 11], im[:, 12], im[:, 13], im[:, 14], 1.0, 0.1, 0.)
    assert int((oracle.launch_batch(optic_b, E, A, S, f[:, 0:3], f[:, 3:6], f[:, 6:9])["rc"] == 1).sum()) == 0
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        r = ctx_a.relay(ctx_b, 1.0, (0.1, 0.))
        c = r["counters"]
        assert c["exit"] == 0 and c["n_in"] == N and c["absorbed"] + c["glass"] + c["outside"] + c["error"] == N
        assert r["n_records"] == 0 and not r["sumw_fixed"].any() and not r["sumw2_fixed"].any()
        assert np.all(r["efficiencies"] == 0.) and np.all(r["efficiency_stderr"] == 0.)
        assert ctx_b.records().shape == (0, 18) and ctx_b.images()["images"].shape == (0, 17)
        with pa.SpotMap(ctx_b, [0.], (-1., 1., -1., 1.), (8, 8)) as m, pa.BeamMoments(ctx_b) as bm:
            m.add("exit")
            bm.add("exit")
            assert m.read()["n_entries"] == 0 and not m.read()["bins"].any() and not bm.read()["sums"].any()
        # and the next relay on the same pair is a full one
        assert ctx_a.relay(ctx_b, 1.0)["counters"]["exit"] > 1000

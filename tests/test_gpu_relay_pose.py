"""Posed relays on the GPU (pc_hip_pose_*, TraceContext.relay with a tilt and a selection): the pair of tests/test_gpu_relay.py -- the
ellipsoidal test optic A and the same optic reversed, B, looking at A's focus -- with B tilted and with a pinhole between the two.

What carries correctness is again the host round trip (test_same_photons_as_the_host_round_trip): A's records fetched, flown by the
host compile of pc_relay_fly_posed, the missed ones dropped, the rest traced by pc_hip_launch_photons of B and multiplied in numpy
must give the relay's records, exact sums and counters bit for bit.

The large pose (gap 0.01 cm, tilt_x 1.5 rad) turns B's entrance plane almost along A's axis, so that on A's exit photons both
`missed` causes occur and photons are still injected.  On the oracle's run of A (seed 20000, slots 0..19999, pinned 10 keV): 1051
photons run away from the plane (nd <= 0), 8692 have it behind them (np < 0), 10257 are injected.

The pinhole is r < 0.0009 cm in the focal plane 0.5 cm behind A: half of the exit weight of the oracle's run of A lies within
0.000916 cm there (6509 of its 20000 photons).

Floors of the comparison with the CPU oracle at the pose (3 mrad, 1 mrad), gap 1 cm (test_oracle_second_stage_posed), measured as
those of tests/test_gpu_relay.py are: python scripts/relay_floors.py --tilt 0.003 0.001 (CPU only; the oracle's launch_batch on B
against itself with one start coordinate moved by 1 ulp, the largest of four), tied to the constants below by
tests/test_relay_pose_cpu.py::test_posed_oracle_floors_are_the_ones_the_gpu_test_uses:
    config        rc 1    share of rc / i_refl flips    |delta| / sum * sqrt(n) of the transmitted weight (largest energy)
    pinned 10 keV 3323    0.0091                        0.0430
    12 energies   8723    0.03835                       0.1602
    rough B (5 A) 3209    0.0088                        0.0513
The margins are the project's: the flip cap is the oracle's own share, the weight bound four times the floor."""
import numpy as np
import pytest

from tests.test_gpu_relay import N, SEED, as_ints, fixed_sums, problems, same_bits
from tests.test_relay_cpu import np_valid
from tests.test_relay_pose_cpu import build_pose_host, host_fly_posed, np_fly_posed

pytestmark = pytest.mark.gpu

#        gap, (off_x, off_y), (tilt_x, tilt_y)
POSES = [(1.0, (0., 0.), (0.002, 0.)), (1.0, (0., 0.), (0., -0.005)), (1.0, (0.002, 0.), (0.003, 0.001))]
LARGE = (0.01, (0., 0.), (1.5, 0.))
TILTED = (1.0, (0., 0.), (0.003, 0.001))
PINHOLE = dict(axis="r", d=0.5, centre=(0., 0.), range=(0., 0.0009))
#               flip cap, weight floor at the pose TILTED (module docstring)
POSED_FLOORS = {"pinned": (0.0091, 0.0430), "ne12": (0.03835, 0.1602), "rough": (0.0088, 0.0513)}
COUNTER_KEYS = ("n_in", "exit", "absorbed", "glass", "outside", "error")


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_pose_host(tmp_path_factory.mktemp("relay_pose_host"))


def pose_run(pa, ctx_a, ctx_b, gap, off, tilt, select=None):
    """pc_hip_pose_run itself, whatever the tilt (TraceContext.relay sends a pose without tilt and selection to pc_hip_relay_run)"""
    import ctypes as C
    pose = np.array([gap, off[0], off[1], tilt[0], tilt[1]], dtype=np.float64)
    st = pa.lib().pc_hip_pose_run(ctx_a._h, ctx_b._h, pose.ctypes.data_as(C.POINTER(C.c_double)), None if select is None else select._h)
    if st != 0:
        raise pa.HipError("pc_hip_pose_run", st)
    ctx_b._relay_squares = getattr(ctx_b, "_weight_squares", False)
    r = ctx_b.relay_totals()
    ctx_b._last_n = r["n_records"]
    return r


def totals_key(r):
    return (r["counters_array"].tolist(), r["counters"]["missed"], r["counters"]["rejected"], as_ints(r["sumw_fixed"]),
            None if r["sumw2_fixed"] is None else as_ints(r["sumw2_fixed"]))


def round_trip(pa, host, rec_a, ctx_b, pose, passing=None):
    """the host round trip of a posed relay: records of A (those at the positions `passing`, if given) -> host compile of the
    contract -> the missed ones dropped -> pc_hip_launch_photons of B -> products.  Returns a dict: the records the relay must have
    left, rc of the injected photons, their entries in A's store, and the counts."""
    gap, off, tilt = pose
    ne = rec_a.shape[1] - 17
    valid = np_valid(rec_a[:, 10], rec_a[:, 17])
    sel = np.ones(len(valid), dtype=bool)
    if passing is not None:
        sel[:] = False
        sel[passing] = True
    idx = np.flatnonzero(valid & sel)
    basis = pa.relay_basis(gap, off, tilt)
    six = rec_a[idx][:, [8, 9, 11, 12, 13, 14]]
    f, hit = host_fly_posed(host, six, gap, off[0], off[1], basis)
    # which of the two causes (the contract's nd and np again, in numpy)
    dz = np.sqrt((1. - six[:, 2] * six[:, 2]) - six[:, 3] * six[:, 3])
    nd = (basis[6] * six[:, 2] + basis[7] * six[:, 3]) + basis[8] * dz
    away = ~(nd > 0.)
    assert not (away & hit).any()
    idx, f, ra = idx[hit], f[hit], rec_a[idx][hit]
    g = ctx_b.launch_photons(f[:, 0:3], f[:, 3:6], f[:, 6:9]) if len(idx) else None
    rc = g["rc"] if g is not None else np.zeros(0, dtype=np.int32)
    ok = rc == 1
    out = np.zeros((int(ok.sum()), 17 + ne))
    if g is not None:
        out[:, 0:2] = ra[ok, 0:2]
        out[:, 2:4], out[:, 4:6], out[:, 6:8] = f[ok, 0:2], f[ok, 3:5], f[ok, 6:8]
        out[:, 8:11], out[:, 11:13], out[:, 13:15] = g["exit_coords"][ok], g["exit_dir"][ok, 0:2], g["exit_elecv"][ok, 0:2]
        out[:, 15] = (ra[ok, 15].view(np.int64) + g["i_refl"][ok]).view(np.float64)
        out[:, 16] = (ra[ok, 16] + f[ok, 9]) + g["d_travel"][ok]
        out[:, 17:] = ra[ok, 17:] * g["weights"][ok]
    return dict(records=out, rc=rc, entries=idx, n_in=len(idx), skipped=int((~valid).sum()), rejected=int((valid & ~sel).sum()),
                missed=int((~hit).sum()), away=int(away.sum()), behind=int((~hit & ~away).sum()))


def check_against_round_trip(pa, host, ctx_a, ctx_b, pose, r, n_started, passing=None):
    rec = ctx_b.records()
    t_b = ctx_b.totals()
    mom = ctx_b.moments() if r["sumw2_fixed"] is not None else None
    rec_a = ctx_a.records()
    w = round_trip(pa, host, rec_a, ctx_b, pose, passing)              # (this launch replaces the relay on B)
    want, rc = w["records"], w["rc"]
    assert same_bits(rec, want), "relay records differ from the host round trip"
    c = r["counters"]
    assert (c["n_in"], c["skipped"], c["missed"], c["rejected"]) == (w["n_in"], w["skipped"], w["missed"], w["rejected"])
    assert c["n_in"] + c["skipped"] + c["missed"] + c["rejected"] == rec_a.shape[0] and c["n_started_a"] == n_started
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


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinned", "ne12"])
def test_zero_tilt_is_the_existing_relay(pa, oracle, name):
    _, _, prob_a, _, prob_b, _ = problems(oracle, name)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        for gap, off in ((1.0, (0., 0.)), (1.0, (0.002, 0.)), (0.8, (0., -0.001))):
            plain = ctx_a.relay(ctx_b, gap, off)
            rec_plain, t_plain = ctx_b.records(), ctx_b.totals()
            assert plain["counters"]["missed"] == 0 and plain["counters"]["rejected"] == 0
            for tilt in ((0., 0.), (-0., 0.)):
                posed = pose_run(pa, ctx_a, ctx_b, gap, off, tilt)
                assert totals_key(posed) == totals_key(plain), (gap, off)
                assert same_bits(ctx_b.records(), rec_plain)
                t = ctx_b.totals()
                assert np.array_equal(t["counters"], t_plain["counters"]) and np.array_equal(t["sumw_fixed"], t_plain["sumw_fixed"])
            again = ctx_a.relay(ctx_b, gap, off, tilt=(0., 0.), select=None)
            assert totals_key(again) == totals_key(plain)
        assert plain["counters"]["exit"] > 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinned", "ne12", "rough"])
def test_same_photons_as_the_host_round_trip(pa, oracle, host, name):
    """The large pose is a condition on the input: on the oracle's photons it gives 1051 away, 8692 behind, 10257 injected (module
    docstring); all three must occur on the GPU's photons."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, name)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        for pose in POSES + [LARGE]:
            r = ctx_a.relay(ctx_b, *pose)
            assert r["efficiency_stderr"] is not None and np.all(r["efficiency_stderr"] >= 0.)
            w = check_against_round_trip(pa, host, ctx_a, ctx_b, pose, r, ra["i_start"])
            print(name, pose, r["counters"], "away", w["away"], "behind", w["behind"], "eff", r["efficiencies"][:2], "stage 2 ms", r["kernel_ms"])
            if pose is LARGE:
                assert w["away"] > 0 and w["behind"] > 0 and w["n_in"] > 0
                assert r["counters"]["missed"] == w["away"] + w["behind"]
            else:
                assert r["counters"]["missed"] == 0
        assert ctx_a.relay(ctx_b, 1.0)["counters"]["exit"] > 1000          # and a plain relay afterwards is the one it was


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinned", "ne12"])
def test_aperture_and_its_complement(pa, oracle, host, name):
    _, _, prob_a, _, prob_b, _ = problems(oracle, name)
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ra = ctx_a.transmission(SEED, 0, N, keep_images=True)
        with pa.Selection(ctx_a, [PINHOLE]) as S, pa.Selection(ctx_a, [dict(PINHOLE, **{"not": True})]) as Sn:
            tot = S.apply("exit")
            Sn.apply("exit")
            share = tot["passed_w"][0] / (tot["passed_w"][0] + tot["rejected_w"][0])
            print(name, "pinhole passes", int(tot["n_pass"][0]), "photons,", share, "of the weight")
            # about half at 10 keV, where the radius was chosen; the focus shrinks with the energy, but both the pinhole and its
            # complement keep a share of every energy
            assert np.all((share > 0.1) & (share < 0.9)) and (name != "pinned" or 0.3 < share[0] < 0.7)
            whole = ctx_a.relay(ctx_b, *TILTED)
            rec_whole = ctx_b.records()
            through = ctx_a.relay(ctx_b, *TILTED, select=S)
            rec_through = ctx_b.records()
            around = ctx_a.relay(ctx_b, *TILTED, select=Sn)
            rec_around = ctx_b.records()
            _, pos = S.gather(positions=True)
            _, pos_n = Sn.gather(positions=True)
            # the two relays add up to the one without a selection, exactly
            for k in COUNTER_KEYS:
                assert through["counters"][k] + around["counters"][k] == whole["counters"][k], k
            ne = len(as_ints(whole["sumw_fixed"]))
            for key in ("sumw_fixed", "sumw2_fixed"):
                a, b, c = as_ints(through[key]), as_ints(around[key]), as_ints(whole[key])
                assert [a[e] + b[e] for e in range(ne)] == c, key
            assert through["counters"]["exit"] > 100 and around["counters"]["exit"] > 100
            assert whole["counters"]["rejected"] == 0
            assert through["counters"]["rejected"] == around["counters"]["n_in"] + around["counters"]["missed"]
            assert around["counters"]["rejected"] == through["counters"]["n_in"] + through["counters"]["missed"]
            for r in (whole, through, around):
                c = r["counters"]
                assert c["n_in"] + c["skipped"] + c["missed"] + c["rejected"] == N and c["skipped"] == whole["counters"]["skipped"]
            # the records through the selection are the rows of the whole relay whose entries pass the mask, in order
            w = round_trip(pa, host, ctx_a.records(), ctx_b, TILTED)
            assert same_bits(w["records"], rec_whole)
            origin = w["entries"][w["rc"] == 1]
            assert same_bits(rec_through, rec_whole[np.isin(origin, pos)])
            assert same_bits(rec_around, rec_whole[np.isin(origin, pos_n)])
            # and the relay through the selection is the host round trip of the passing entries
            again = ctx_a.relay(ctx_b, *TILTED, select=S)
            assert totals_key(again) == totals_key(through)
            check_against_round_trip(pa, host, ctx_a, ctx_b, TILTED, again, ra["i_start"], passing=pos)
            # no tilt, but an aperture: the general form with the identity basis
            flat = ctx_a.relay(ctx_b, 1.0, select=S)
            check_against_round_trip(pa, host, ctx_a, ctx_b, (1.0, (0., 0.), (0., 0.)), flat, ra["i_start"], passing=pos)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_launch_invariance(pa, oracle):
    """However A's run was stored and launched and whatever the block size, a tilted relay through a selection has bit-identical
    totals, `missed` and `rejected` included, and the same records in the same order -- after a compact run of A, whose positions
    are in the order of completion, as the same set."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    n = 4 * 65536 + 777                       # enough slots for run_parts 4
    pose = (1.0, (0.001, 0.), (0.002, -0.001))
    cut = dict(axis="r", d=0.5, centre=(0., 0.), range=(0., 0.002))
    base = None
    variants = [dict(), dict(plane_images=1), dict(plane_images=1, compact_images=1), dict(run_parts=4), dict(block_size=256),
                dict(block_size=512), dict(plane_images=1, compact_images=1, run_parts=4, block_size=256), dict(relay_acc_lds=0)]
    for opts in variants:
        with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
            ctx_b.set_option("weight_squares", 1)
            for k, v in opts.items():
                (ctx_b if k == "relay_acc_lds" else ctx_a).set_option(k, v)
            if "block_size" in opts:
                ctx_b.set_option("block_size", opts["block_size"])
            ctx_a.run(SEED, 0, n, keep_images=True)
            with pa.Selection(ctx_a, [cut]) as S:
                S.apply("exit")
                r = ctx_a.relay(ctx_b, *pose, select=S)
                rec = ctx_b.records()
        key = totals_key(r)
        if base is None:
            base = (key, rec)
            assert r["counters"]["exit"] > 5000 and r["counters"]["rejected"] > 5000
            continue
        assert key == base[0], opts
        if opts.get("compact_images"):
            assert same_bits(rec[np.lexsort(rec.T[::-1])], base[1][np.lexsort(base[1].T[::-1])]), opts
        else:
            assert same_bits(rec, base[1]), opts


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_contexts_usable(pa, oracle):
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")

    def refused(a, b, pose, select=None, match=""):
        with pytest.raises(pa.HipError) as e:
            a.relay(b, *pose, select=select)
        assert e.value.status == -2 and match in str(e.value), str(e.value)

    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b, pa.TraceGroup(prob_a, [0]) as grp:
        ctx_a.run(SEED, 0, N, keep_images=True)
        before = ctx_a.relay(ctx_b, 1.0)
        rec_before = ctx_b.records()

        def still_the_same():
            # B still holds the relay it held, and a plain relay gives the totals it gave
            assert totals_key(ctx_b.relay_totals()) == totals_key(before) and same_bits(ctx_b.records(), rec_before)
            assert totals_key(ctx_a.relay(ctx_b, 1.0)) == totals_key(before)

        for pose in ((1.0, (0., 0.), (np.pi / 2., 0.)), (1.0, (0., 0.), (0.001, float("nan"))), (-1.0, (0., 0.), (0.001, 0.)),
                     (1.0, (float("inf"), 0.), (0.001, 0.)), (1.0, (0., 0.), (0., -2.))):
            refused(ctx_a, ctx_b, pose, match="tilt")
            still_the_same()
        with pa.Selection(ctx_b, [PINHOLE]) as Sb, pa.Selection(grp, [PINHOLE]) as Sg, pa.Selection(ctx_a, [PINHOLE]) as S:
            Sb.apply("exit")                                           # the relay's records on B are its kind 0
            refused(ctx_a, ctx_b, TILTED, Sb, match="another owner")
            still_the_same()
            refused(ctx_a, ctx_b, TILTED, Sg, match="another owner")
            still_the_same()
            refused(ctx_a, ctx_b, TILTED, S, match="was not applied for kind 0")
            still_the_same()
            S.apply("exit")
            good = ctx_a.relay(ctx_b, *TILTED, select=S)
            assert good["counters"]["rejected"] > 0 and good["counters"]["exit"] > 0
            before, rec_before = ctx_a.relay(ctx_b, 1.0), ctx_b.records()
            ctx_a.run(SEED, 0, N, keep_images=True)                    # the entries of A are replaced: the mask is stale
            refused(ctx_a, ctx_b, TILTED, S, match="mask is stale: the entries of kind 0 were replaced after it was applied")
            still_the_same()
            with pytest.raises(pa.HipError) as e:
                S.gather()
            assert "mask is stale: the entries of kind 0 were replaced after it was applied" in str(e.value)      # the gather's wording
            S.apply("exit")
            assert totals_key(ctx_a.relay(ctx_b, *TILTED, select=S)) == totals_key(good)
            with pytest.raises(TypeError):
                ctx_a.relay(ctx_b, 1.0, select="pinhole")
        # what pc_hip_relay_run refuses, pc_hip_pose_run refuses
        refused(ctx_a, ctx_a, TILTED, match="context of its own")
        refused(ctx_b, ctx_a, TILTED, match="result of a relay")
        assert ctx_a.relay(ctx_b, 1.0)["counters"]["exit"] > 1000


# ---- 11 -----------------------------------------------------------------------------------------------------------------------
def test_rocking_curve(pa, oracle):
    """The aligned pair rocked about y: the response peaks at no tilt and is symmetric -- each pair of opposite tilts within three
    standard errors of its difference, taken from the curve's own (sqrt of the sum of the two squares: the two relays fly the same
    photons of A, which only makes their difference smaller than that of independent runs)."""
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    mrad = np.array([-10., -5., -2., 0., 2., 5., 10.])
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_b.set_option("weight_squares", 1)
        ctx_a.run(SEED, 0, N, keep_images=True)
        rc = pa.relay_rocking_curve(ctx_a, ctx_b, 1.0, [(1e-3 * m, 0.) for m in mrad])
        plain = ctx_a.relay(ctx_b, 1.0)
    eff, err = rc["efficiencies"][:, 0], rc["efficiency_stderr"][:, 0]
    print("tilt_x mrad", mrad, "eff", eff, "+-", err, "exit", [c["exit"] for c in rc["counters"]])
    assert rc["tilts"].shape == (7, 2) and rc["efficiencies"].shape == (7, 1) and len(rc["counters"]) == 7
    assert eff[3] == plain["efficiencies"][0] and err[3] == plain["efficiency_stderr"][0]
    assert int(np.argmax(eff)) == 3 and np.all(eff[3] > np.delete(eff, 3))
    assert eff[3] > 2. * eff[0] and eff[3] > 2. * eff[6]
    for k in range(3):
        assert abs(eff[k] - eff[6 - k]) <= 3. * np.hypot(err[k], err[6 - k]), (mrad[k], eff[k], eff[6 - k], err[k], err[6 - k])


# ---- 12 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pinned", "ne12", "rough"])
def test_oracle_second_stage_posed(pa, oracle, name):
    """The same photons (the GPU run of A, posed by the numpy restatement of the contract) through the oracle's B and through the
    relay: see the module docstring for the floors."""
    _, _, prob_a, optic_b, prob_b, (E, A, S) = problems(oracle, name)
    flip_cap, c_floor = POSED_FLOORS[name]
    gap, off, tilt = TILTED
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.transmission(SEED, 0, N, keep_images=True)
        ra = ctx_a.records()
        r = ctx_a.relay(ctx_b, gap, off, tilt)
        rec = ctx_b.records()
        f, hit = np_fly_posed(*(ra[:, k] for k in (8, 9, 11, 12, 13, 14)), gap, off[0], off[1], pa.relay_basis(gap, off, tilt))
        assert hit.all() and r["counters"]["missed"] == 0 and r["counters"]["n_in"] == N
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

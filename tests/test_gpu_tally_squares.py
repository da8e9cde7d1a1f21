"""The squared-weight sums of the tallies on the GPU (pc_hip_{spot,hist,joint,select}_track_squares / _read_squares, squares=True):
every cell's S2 equals the Python-integer sum of W*W over the run's own fetched records, binned by the numpy restatements of
tests/test_spot_cpu.py, test_hist_cpu.py and test_joint_cpu.py -- in both regimes, across the carry of lo into hi, across a tile
boundary, through selections, for the leak kinds and however the run was launched -- while the weight sums stay bit-identical to
those of an object that does not track squares."""
import numpy as np
import pytest

from tests.test_gpu_hist import DECK, KINDS, SEED, _prob, leak_entries, record_entries
from tests.test_gpu_select import D_SPOT, NX, NY, WINDOW, config, median_cut, real_selection
from tests.test_hist_cpu import np_bins, np_value
from tests.test_joint_cpu import QUANTITIES, axis, np_cells
from tests.test_select_cpu import np_pass
from tests.test_spot_cpu import np_q, np_spot_bin
from tests.test_tally_squares_cpu import to_ints, to_pairs

pytestmark = pytest.mark.gpu

N_SLOTS = 4000
REGIMES = (1, 2)


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


# ---- the restatement: Python-integer sums of W*W per cell --------------------------------------------------------------------------
def np_sq_sums(bins, Q, n_bins):
    """(object [S, n_bins], object [S]): the sums of Q*Q as Python integers per bin and over the entries with bin -1.  W*W <= 2^64 is cut
    into four 16-bit limbs of its low 64 bits and the 65th bit (Q = 2^32 only); each limb's float64 bincount is exact (< 2^16 * n)"""
    S = Q.shape[1]
    H, out = np.zeros((S, n_bins), dtype=object), np.zeros(S, dtype=object)
    inside = bins >= 0
    for s in range(S):
        q = Q[:, s]
        lo = q * q                                                              # uint64: mod 2^64
        limbs = [((lo >> np.uint64(16 * l)) & np.uint64(0xffff)).astype(np.float64) for l in range(4)] + [(q >> np.uint64(32)).astype(np.float64)]
        for l, part in enumerate(limbs):
            h = np.bincount(bins[inside], weights=part[inside], minlength=n_bins)
            H[s] += np.array([int(v) << (16 * l) for v in h], dtype=object)
            out[s] += int(part[~inside].sum()) << (16 * l)
    return H, out


def sq_total(Q):
    return [sum(int(v) * int(v) for v in Q[:, s]) for s in range(Q.shape[1])]


def sq_hists(axes, E, W, ze, leak=False):
    """object [S, total_bins], object [n_axes, S]"""
    Q = np_q(W)
    cells, outs = [], []
    for a in axes:
        v, ok = np_value(QUANTITIES.index(a["axis"]), E, leak, ze + a["d"], *a["centre"])
        H, out = np_sq_sums(np_bins(v, ok, a["range"][0], a["range"][1], a["bins"]), Q, a["bins"])
        cells.append(H)
        outs.append(out)
    return np.concatenate(cells, axis=1), np.stack(outs)


def sq_joint(pairs, E, W, ze, leak=False):
    Q = np_q(W)
    cells, outs = [], []
    for u, v in pairs:
        H, out = np_sq_sums(np_cells(u, v, E, leak, ze), Q, u["bins"] * v["bins"])
        cells.append(H)
        outs.append(out)
    return np.concatenate(cells, axis=1), np.stack(outs)


def sq_spot(E, W, zps, window, nx, ny):
    """object [P, S, ny, nx], object [P, S]"""
    Q = np_q(W)
    bins, outs = [], []
    for zp in zps:
        b = np_spot_bin(E[:, 0], E[:, 1], E[:, 2], E[:, 3], E[:, 4], E[:, 5], zp, window, nx, ny)
        H, out = np_sq_sums(b, Q, ny * nx)
        bins.append(H.reshape(-1, ny, nx))
        outs.append(out)
    return np.stack(bins), np.stack(outs)


def same_pairs(got, want_ints, what):
    assert np.array_equal(got, to_pairs(want_ints)), "%s differ from the Python-integer sums" % what


def add_pairs(a, b):
    return to_pairs(to_ints(a) + to_ints(b))


# ---- one run per energy count, every tally in both regimes with and without squares, read once ------------------------------------
_RUNS = {}


def the_run(pa, ne):
    """dict: E, W, ze, cfg, and per name ("spot1", "hist2", ...) the read() of the tracking object and of a plain one after the same add"""
    if ne in _RUNS:
        return _RUNS[ne]
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        ctx.wait()
        N = ctx.totals()["i_start"]
        E, W = record_entries(ctx.records())
        cfg = config(E, ze)
        reads = {}
        for regime in REGIMES:
            for sq in (True, False):
                with pa.SpotMap(ctx, [D_SPOT], WINDOW, (NX, NY), regime=regime, squares=sq) as m, \
                        pa.Histograms(ctx, cfg["axes"], regime=regime, squares=sq) as h, pa.JointHistograms(ctx, cfg["pairs"], regime=regime, squares=sq) as j:
                    for name, t in (("spot", m), ("hist", h), ("joint", j)):
                        t.add("exit")
                        reads[(name + str(regime), sq)] = t.read()
                        if sq:
                            reads[(name + str(regime), "stderr")] = t.stderr(N)
    _RUNS[ne] = dict(E=E, W=W, ze=ze, cfg=cfg, reads=reads, N=N)
    return _RUNS[ne]


CELLS = {"spot": "bins", "hist": "bins", "joint": "cells"}


# ---- 1, 4: the squares equal the restatement, and are conserved ----------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_squares_equal_the_restatement(pa, ne):
    r = the_run(pa, ne)
    E, W, ze, cfg = r["E"], r["W"], r["ze"], r["cfg"]
    assert len(E) == N_SLOTS
    want = {"spot": sq_spot(E, W, [ze + D_SPOT], WINDOW, NX, NY), "hist": sq_hists(cfg["axes"], E, W, ze), "joint": sq_joint(cfg["pairs"], E, W, ze)}
    total = sq_total(np_q(W))
    for regime in REGIMES:
        for name, (cells, outside) in want.items():
            got, plain = r["reads"][(name + str(regime), True)], r["reads"][(name + str(regime), False)]
            what = "%s, regime %d" % (name, regime)
            assert "squares" not in plain and "outside_squares" not in plain
            key = CELLS[name]
            assert got[key].any() and got["outside"].any(), what                          # weight inside and outside: both paths ran
            assert np.array_equal(got[key], plain[key]) and np.array_equal(got["outside"], plain["outside"]), "%s: the weight sums changed" % what
            assert np.array_equal(got["n_entries"], plain["n_entries"])
            sq, out = (got["squares"], got["outside_squares"]) if name == "spot" else (got["squares"][0], got["outside_squares"][0])
            same_pairs(sq, cells, what + ": squares")
            same_pairs(out, outside, what + ": outside_squares")
            if name != "spot":
                assert not got["squares"][1:].any() and not got["outside_squares"][1:].any()
            # 4: conservation per map, axis or pair and per energy, from the device's own numbers
            got_sq, got_out = to_ints(sq), to_ints(out)
            if name == "spot":
                for s in range(ne):
                    assert int(got_sq[0, s].sum()) + int(got_out[0, s]) == total[s], what
            else:
                off = np.cumsum([0] + ([a["bins"] for a in cfg["axes"]] if name == "hist" else [u["bins"] * v["bins"] for u, v in cfg["pairs"]]))
                for a in range(len(off) - 1):
                    for s in range(ne):
                        assert int(got_sq[s, off[a]:off[a + 1]].sum()) + int(got_out[a, s]) == total[s], (what, a, s)


@pytest.mark.parametrize("ne", [1, 12])
def test_stderr_and_marginals_follow_from_the_squares(pa, ne):
    """stderr(N) is pc_hip_tally_stderr of what read() returns; the marginal of S2 is the exact sum of the cells' S2"""
    r = the_run(pa, ne)
    for regime in REGIMES:
        for name in ("spot", "hist", "joint"):
            got = r["reads"][(name + str(regime), True)]
            err = r["reads"][(name + str(regime), "stderr")]
            key = CELLS[name]
            assert err.shape == got[key].shape and err.dtype == np.float64
            assert np.array_equal(err, pa.tally_stderr(got[key], got["squares"], r["N"]))
            assert ((err > 0.) == (got[key] > 0)).all()                                     # an error wherever there is weight, and only there
            # a cell of one entry of weight w: sqrt((w^2/N - w^2/N^2) / (N - 1)) = w / N * sqrt((N - 1) / (N - 1)) ... = w / N
            S, S2 = got[key].astype(object), to_ints(got["squares"])
            single = np.asarray((S * S == S2) & (S > 0), dtype=bool)
            assert single.any()
            N = r["N"]
            assert np.allclose(err[single], S[single].astype(np.float64) * 2.0 ** -32 / N, rtol=1e-12, atol=0.)
    prob = _prob(pa, ne)
    cfg = r["cfg"]
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        with pa.JointHistograms(ctx, cfg["pairs"], squares=True) as j, pa.JointHistograms(ctx, cfg["pairs"]) as jp:
            j.add("exit")
            jp.add("exit")
            sq = j.read()["pairs_squares"]
            for p, (u, v) in enumerate(cfg["pairs"]):
                mu, mv = j.marginal(p, "u", squares=True), j.marginal(p, "v", squares=True)
                assert mu.shape == (ne, u["bins"], 2) and mv.shape == (ne, v["bins"], 2)
                ints = to_ints(sq[p][0])
                assert to_ints(mu).tolist() == ints.sum(axis=1).tolist() and to_ints(mv).tolist() == ints.sum(axis=2).tolist()
                assert np.array_equal(j.marginal(p, "u"), jp.marginal(p, "u"))
            eff = np.linspace(0.1, 0.2, ne)
            dens, err = j.density(0, eff, n_started=r["N"])
            assert np.array_equal(dens, jp.density(0, eff)) and err.shape == dens.shape and ((err > 0.) == (dens > 0.)).all()
            with pytest.raises(ValueError):
                jp.marginal(0, "u", squares=True)
            with pytest.raises(ValueError):
                jp.density(0, eff, n_started=10)
            with pytest.raises(ValueError):
                jp.stderr(10)


# ---- 2: the carry -------------------------------------------------------------------------------------------------------------------
def test_carry_of_lo_into_hi(pa):
    """One N_REFL bin over [0, 1e9) holds every entry.  At 10 keV W*W is about 2^62: lo wraps after a handful of entries and hi counts
    the wraps."""
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        ctx.wait()
        _, W = record_entries(ctx.records())
        Q = np_q(W)
        want = sq_total(Q)[0]
        assert want >> 64 > N_SLOTS // 16 and np.median(Q[:, 0].astype(np.float64)) > 2.0 ** 30
        for regime in REGIMES:
            with pa.Histograms(ctx, [axis("nrefl", 0., 1e9, 1)], regime=regime, squares=True) as h:
                h.add("exit")
                r = h.read()
                assert r["squares"].shape == (3, 1, 1, 2) and r["outside_squares"].shape == (3, 1, 1, 2)
                assert int(r["bins"][0, 0, 0]) == sum(int(v) for v in Q[:, 0]) and not r["outside"].any() and not r["outside_squares"].any()
                lo, hi = (int(v) for v in r["squares"][0, 0, 0])
                assert (lo, hi) == (want & ((1 << 64) - 1), want >> 64), regime
                h.add("exit")                                                            # and again onto a pair that is already large
                assert to_ints(h.read()["squares"][0, 0, 0]) == 2 * want


# ---- 3: the tile seam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_tile_seam(pa, ne):
    """An X_AT axis sized from the split function so that the cells of a kind fit one tile of weight sums but cross the first tile
    boundary once each cell carries its pair: regime 1 makes one pass without squares and two with, and gives the same numbers"""
    tile = 8192
    per_tile = tile // 3                                                                     # pc_tally_tile_split, pinned by tests/test_tally_squares_cpu.py
    tiles = lambda total, squares: -(-total // (per_tile if squares else tile))
    r = the_run(pa, ne)
    E, W, ze = r["E"], r["W"], r["ze"]
    n_bins = (per_tile + per_tile // 4) // ne - 1                                            # ne * (n_bins + 1) cells: a quarter beyond one tile
    total = ne * (n_bins + 1)
    assert tiles(total, False) == 1 and tiles(total, True) == 2
    v, ok = np_value(QUANTITIES.index("x"), E, False, ze + 0.5)
    v = v[ok & np.isfinite(v)]
    axes = [axis("x", float(np.percentile(v, 10)), float(np.percentile(v, 90)), n_bins, d=0.5)]
    prob = _prob(pa, ne)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        with pa.Histograms(ctx, axes, squares=True) as h, pa.Histograms(ctx, axes) as plain, pa.Histograms(ctx, axes, regime=2, squares=True) as wide:
            assert h.regime == 1 and plain.regime == 1
            for t in (h, plain, wide):
                t.add("exit")
            got, ref, other = h.read(), plain.read(), wide.read()
    cells, outside = sq_hists(axes, E, W, ze)
    assert np.array_equal(got["bins"], ref["bins"]) and np.array_equal(got["outside"], ref["outside"])
    same_pairs(got["squares"][0], cells, "squares across the tile boundary")
    same_pairs(got["outside_squares"][0], outside, "outside_squares")
    assert np.array_equal(got["squares"], other["squares"]) and np.array_equal(got["outside_squares"], other["outside_squares"])
    # cells with weight on both sides of the boundary: cell = energy * (n_bins + 1) + bin
    flat = np.concatenate([got["squares"][0, :, :, 0], got["outside_squares"][0, 0, :, None, 0]], axis=1).ravel()
    hit = np.flatnonzero(flat)
    assert (hit < per_tile).sum() > 100 and (hit >= per_tile).sum() > 20


# ---- 5: gated adds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_gated_adds(pa, ne):
    r = the_run(pa, ne)
    E, W, ze, cfg = r["E"], r["W"], r["ze"], r["cfg"]
    c = median_cut("r", E, False, ze, d=0.5)
    cn = dict(c, **{"not": True})
    p = real_selection([c], E, False, ze)
    Q = np_q(W)
    total, passed, rejected = sq_total(Q), sq_total(Q[p]), sq_total(Q[~p])
    prob = _prob(pa, ne)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        with pa.Selection(ctx, [c], squares=True) as S, pa.Selection(ctx, [cn], squares=True) as Sn, pa.Selection(ctx, [c]) as Splain:
            res, resn, resp = S.apply("exit"), Sn.apply("exit"), Splain.apply("exit")
            assert "passed_w2" not in resp
            for k in ("n_pass", "n_seen", "passed_w", "rejected_w"):
                assert np.array_equal(res[k], resp[k]), k                                   # the totals without squares are unchanged
            assert res["passed_w2"].shape == (3, ne, 2) and not res["passed_w2"][1:].any() and not res["rejected_w2"][1:].any()
            assert to_ints(res["passed_w2"][0]).tolist() == passed and to_ints(res["rejected_w2"][0]).tolist() == rejected
            assert to_ints(resn["passed_w2"][0]).tolist() == rejected and to_ints(resn["rejected_w2"][0]).tolist() == passed
            assert [a + b for a, b in zip(passed, rejected)] == total                        # passed_w2 + rejected_w2 is the total
            T, T_err = S.transmission("exit")
            t2, e2 = pa.select_transmission(res["passed_w"][0], res["rejected_w"][0], res["passed_w2"][0], res["rejected_w2"][0])
            assert np.array_equal(T, t2) and np.array_equal(T_err, e2) and ((T > 0.) & (T < 1.)).all() and ((T_err > 0.) & (T_err < 0.1)).all()
            with pytest.raises(ValueError):
                Splain.transmission("exit")
            for regime in REGIMES:
                with pa.SpotMap(ctx, [D_SPOT], WINDOW, (NX, NY), regime=regime, squares=True) as m, \
                        pa.Histograms(ctx, cfg["axes"], regime=regime, squares=True) as h, pa.JointHistograms(ctx, cfg["pairs"], regime=regime, squares=True) as j:
                    want = {"spot": sq_spot(E[p], W[p], [ze + D_SPOT], WINDOW, NX, NY), "hist": sq_hists(cfg["axes"], E[p], W[p], ze),
                            "joint": sq_joint(cfg["pairs"], E[p], W[p], ze)}
                    for name, t in (("spot", m), ("hist", h), ("joint", j)):
                        what = "%s, regime %d" % (name, regime)
                        plain = r["reads"][(name + str(regime), True)]
                        t.add("exit", select=S)
                        gated = t.read()
                        sq, out = (gated["squares"], gated["outside_squares"]) if name == "spot" else (gated["squares"][0], gated["outside_squares"][0])
                        same_pairs(sq, want[name][0], what + ": gated squares")
                        same_pairs(out, want[name][1], what + ": gated outside_squares")
                        # gated sum + outside == passed_w2 per map, axis or pair and energy
                        gi, go = to_ints(sq), to_ints(out)
                        if name == "spot":
                            assert [int(gi[0, s].sum()) + int(go[0, s]) for s in range(ne)] == passed, what
                        else:
                            off = np.cumsum([0] + ([a["bins"] for a in cfg["axes"]] if name == "hist" else [u["bins"] * v["bins"] for u, v in cfg["pairs"]]))
                            for a in range(len(off) - 1):
                                assert [int(gi[s, off[a]:off[a + 1]].sum()) + int(go[a, s]) for s in range(ne)] == passed, (what, a)
                        # the selection's squares plus its complement's equal the plain add's, cell by cell
                        t.reset()
                        t.add("exit", select=Sn)
                        comp = t.read()
                        assert np.array_equal(add_pairs(gated["squares"], comp["squares"]), plain["squares"]), what
                        assert np.array_equal(add_pairs(gated["outside_squares"], comp["outside_squares"]), plain["outside_squares"]), what
                        t.add("exit", select=S)                                              # into one object: the plain add
                        both = t.read()
                        assert np.array_equal(both["squares"], plain["squares"]) and np.array_equal(both["outside_squares"], plain["outside_squares"]), what
                        assert np.array_equal(both[CELLS[name]], plain[CELLS[name]])


# ---- 6: launch invariance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_launch_invariance(pa, ne):
    prob = _prob(pa, ne)
    N = 196608                      # 3 launches with run_parts >= 3 (a run is cut into at most n / 65536 launches)
    r = the_run(pa, ne)
    cfg, ze = r["cfg"], r["ze"]
    c = median_cut("r", r["E"], False, ze, d=0.5)

    def make(owner):
        sel = pa.Selection(owner, [c], squares=True)
        ts = []
        for regime in REGIMES:
            ts += [pa.SpotMap(owner, [D_SPOT], WINDOW, (NX, NY), regime=regime, squares=True), pa.Histograms(owner, cfg["axes"], regime=regime, squares=True),
                   pa.JointHistograms(owner, cfg["pairs"], regime=regime, squares=True)]
        return sel, ts

    def sums_of(sel, ts, runs):
        """the plain adds' squares of every tally, and the selection's squares summed over the runs"""
        for t in ts:
            t.reset()
        tot = None
        for run in runs:
            run()
            res = sel.apply("exit")
            for t in ts:
                t.add("exit")
            part = to_ints(np.stack([res["passed_w2"][0], res["rejected_w2"][0]]))
            tot = part if tot is None else tot + part
        reads = [t.read() for t in ts]
        return [(r_["squares"], r_["outside_squares"]) for r_ in reads], tot

    def agree(got, ref, what):
        assert (got[1] == ref[1]).all(), what
        for k, ((a, b), (c_, d)) in enumerate(zip(got[0], ref[0])):
            assert np.array_equal(a, c_) and np.array_equal(b, d), "%s: tally %d" % (what, k)

    with pa.TraceContext(prob, 0) as ctx:
        sel, ts = make(ctx)
        ref = sums_of(sel, ts, [lambda: ctx.run(SEED, 0, N, keep_images=True)])
        assert all(sq.any() and out.any() for sq, out in ref[0])
        # the two regimes hold the same squares
        for k in range(3):
            assert np.array_equal(ref[0][k][0], ref[0][3 + k][0]) and np.array_equal(ref[0][k][1], ref[0][3 + k][1])
        ctx.set_option("run_parts", 4)
        agree(sums_of(sel, ts, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), ref, "(run_parts 4)")
        ctx.set_option("run_parts", 1)
        ctx.set_option("plane_images", 1)
        ctx.set_option("compact_images", 1)
        agree(sums_of(sel, ts, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), ref, "(compact planes)")
        ctx.set_option("compact_images", 0)
        agree(sums_of(sel, ts, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), ref, "(slot-order planes)")
        ctx.set_option("plane_images", 0)
        agree(sums_of(sel, ts, [lambda: ctx.run(SEED, 0, N // 2, keep_images=True), lambda: ctx.run(SEED, N // 2, N - N // 2, keep_images=True)]),
              ref, "(two half-runs into one object)")
        for t in ts + [sel]:
            t.close()
    with pa.TraceGroup(prob, [0, 0]) as g:
        sel, ts = make(g)
        agree(sums_of(sel, ts, [lambda: g.transmission(SEED, N, keep_images=True)]), ref, "(group [0, 0])")
        for t in ts + [sel]:
            t.close()


# ---- 7: the tie to the efficiencies' estimator --------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_tie_to_the_efficiency_estimator(pa, ne):
    """With "weight_squares" the run keeps B = sum of (uint64)((w*w) 2^62).  The one-bin cell keeps S2 = sum of W*W, W =
    round(w 2^32).  Per entry |W 2^-32 - w| <= 2^-33 and w <= 1 give |W*W 2^-64 - w*w| < 2^-32, the truncation of B adds 2^-62, and the
    bound n_entries * 2^-31 leaves a factor 2 over their sum.  The variance v = q - m*m then differs by at most (n / N) 2^-30 (2^-31
    from q, and 2 m dm <= 2^-31 from m with dm <= 2^-32 n / N), so the standard errors agree to the relative accuracy dv / v (first
    order: half of that), plus the rounding of the two long double evaluations."""
    prob = _prob(pa, ne)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("weight_squares", 1)
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        ctx.wait()
        tot = ctx.totals()
        B = to_ints(ctx.moments())
        for regime in REGIMES:
            with pa.Histograms(ctx, [axis("nrefl", 0., 1e9, 1)], regime=regime, squares=True) as h:
                h.add("exit")
                res = h.read()
                err = h.stderr(tot["i_start"])[0, :, 0]
            n = int(res["n_entries"][0])
            assert n == tot["i_exit"] == N_SLOTS
            S2 = to_ints(res["squares"][0, :, 0])
            want = pa.efficiency_stderr(tot["sumw_fixed"], ctx.moments(), tot["counters"])
            for e in range(ne):
                assert abs(int(S2[e]) - 4 * int(B[e])) <= n << 33, (regime, e)                # units of 2^-64
                v = want[e] ** 2 * (tot["i_start"] - 1)
                rel = (n / tot["i_start"]) * 2.0 ** -30 / v
                assert want[e] > 0. and abs(err[e] - want[e]) <= want[e] * (rel + 8 * 2.0 ** -53), (regime, e, err[e], want[e])


# ---- 8: the leak kinds ---------------------------------------------------------------------------------------------------------------
def test_leak_kinds(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True, leak_calc=True)
        ents = {"extleak": leak_entries(r["ext"]), "intleak": leak_entries(r["int"])}
        assert all(len(E) > 100 for E, _ in ents.values())
        cfg = config(ents["extleak"][0], ze, leak=True)
        got = {}
        for regime in REGIMES:
            with pa.Histograms(ctx, cfg["axes"], regime=regime, squares=True) as h, pa.JointHistograms(ctx, cfg["pairs"], regime=regime, squares=True) as j, \
                    pa.SpotMap(ctx, [D_SPOT], (-1., 1., -1., 1.), (16, 16), regime=regime, squares=True) as m:
                for kind in ("extleak", "intleak"):
                    h.add(kind)
                    j.add(kind)
                m.add("extleak")
                got[regime] = (h.read(), j.read(), m.read())
    for regime, (h, j, m) in got.items():
        for kind, (E, W) in ents.items():
            k = KINDS[kind]
            cells, outside = sq_hists(cfg["axes"], E, W, ze, leak=True)
            same_pairs(h["squares"][k], cells, "%s histograms, regime %d" % (kind, regime))
            same_pairs(h["outside_squares"][k], outside, "%s histograms outside, regime %d" % (kind, regime))
            assert h["squares"][k].any() and h["outside_squares"][k].any()
            cells, outside = sq_joint(cfg["pairs"], E, W, ze, leak=True)
            same_pairs(j["squares"][k], cells, "%s joint, regime %d" % (kind, regime))
            same_pairs(j["outside_squares"][k], outside, "%s joint outside, regime %d" % (kind, regime))
        assert not h["squares"][0].any() and not j["squares"][0].any()
        E, W = ents["extleak"]
        bins, out = sq_spot(E, W, [ze + D_SPOT], (-1., 1., -1., 1.), 16, 16)
        same_pairs(m["squares"], bins, "extleak spot map, regime %d" % regime)
        same_pairs(m["outside_squares"], out, "extleak spot map outside, regime %d" % regime)


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_objects_unchanged(pa):
    import ctypes as C
    from polycap_amd import _cabi
    L = _cabi.lib()
    u64p = C.POINTER(C.c_uint64)
    r = the_run(pa, 1)
    cfg, ze = r["cfg"], r["ze"]
    prob = _prob(pa, 1)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N_SLOTS, keep_images=True)
        tallies = [("spot", lambda **kw: pa.SpotMap(ctx, [D_SPOT], WINDOW, (NX, NY), **kw)), ("hist", lambda **kw: pa.Histograms(ctx, cfg["axes"], **kw)),
                   ("joint", lambda **kw: pa.JointHistograms(ctx, cfg["pairs"], **kw))]
        for stem, make in tallies:
            with make() as t:
                # read_squares without tracking
                buf = np.full(8, 77, dtype=np.uint64)
                assert getattr(L, "pc_hip_%s_read_squares" % stem)(t._h, buf.ctypes.data_as(u64p), buf.ctypes.data_as(u64p)) == -2
                assert b"does not track squares" in L.pc_hip_last_error() and (buf == 77).all()
                # track_squares after an add
                t.add("exit")
                before = t.read()
                assert getattr(L, "pc_hip_%s_track_squares" % stem)(t._h) == -2
                assert ("pc_hip_%s_track_squares" % stem).encode() in L.pc_hip_last_error() and b"holds no entries" in L.pc_hip_last_error()
                assert getattr(L, "pc_hip_%s_read_squares" % stem)(t._h, buf.ctypes.data_as(u64p), buf.ctypes.data_as(u64p)) == -2      # still not tracking
                t.add("exit")                                                               # and still adding as before
                after = t.read()
                key = CELLS[stem]
                assert np.array_equal(after[key], 2 * before[key]) and np.array_equal(after["outside"], 2 * before["outside"])
                assert "squares" not in after
                # allowed again after a reset; tracking twice is harmless
                t.reset()
                assert getattr(L, "pc_hip_%s_track_squares" % stem)(t._h) == 0 and getattr(L, "pc_hip_%s_track_squares" % stem)(t._h) == 0
                t.squares = True
                t.add("exit")
                got = t.read()
                want = r["reads"][(stem + ("2" if stem == "spot" else str(t.regime)), True)]
                assert np.array_equal(got[key], before[key]) and np.array_equal(got["squares"], want["squares"])
                assert np.array_equal(got["outside_squares"], want["outside_squares"])
                t.reset()                                                                   # a reset zeroes the pairs and keeps the tracking
                assert not t.read()["squares"].any()
                t.add("exit")
                assert np.array_equal(t.read()["squares"], want["squares"])
        c = median_cut("r", r["E"], False, ze, d=0.5)
        with pa.Selection(ctx, [c]) as S:
            buf = np.full(8, 77, dtype=np.uint64)
            assert L.pc_hip_select_read_squares(S._h, buf.ctypes.data_as(u64p), buf.ctypes.data_as(u64p)) == -2 and (buf == 77).all()
            before = S.apply("exit")
            assert L.pc_hip_select_track_squares(S._h) == -2 and b"before the selection is applied" in L.pc_hip_last_error()
            assert L.pc_hip_select_read_squares(S._h, buf.ctypes.data_as(u64p), buf.ctypes.data_as(u64p)) == -2
            after = S.apply("exit")
            assert all(np.array_equal(after[k], before[k]) for k in before) and "passed_w2" not in after
            assert np.array_equal(np_pass([c], r["E"], False, ze).sum(), after["n_pass"][0])


# ---- 10: the public call ------------------------------------------------------------------------------------------------------------
NEW_NAMES = {"/Spot/Exit_Squares", "/Spot/Exit_StdErr", "/Spot/Exit_Outside_Squares", "/Spot/Exit_Outside_StdErr",
             "/Hist/Exit/Bins_Squares", "/Hist/Exit/Bins_StdErr", "/Hist/Exit/Outside_Squares", "/Hist/Exit/Outside_StdErr",
             "/Joint/Exit/Cells_Squares", "/Joint/Exit/Cells_StdErr", "/Joint/Exit/Outside_Squares", "/Joint/Exit/Outside_StdErr",
             "/Select/Passed_Squares", "/Select/Rejected_Squares", "/Select/Transmission", "/Select/Transmission_StdErr"}


def test_public_call(pa, monkeypatch, tmp_path):
    from tests import test_gpu_select as G
    n = 12000
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        total = ctx.device_memory()[1]
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        N = ctx.totals()["i_start"]
        E, W = record_entries(ctx.records())
        cuts = [median_cut("r", E, False, ze, d=0.5)]
        real_selection(cuts, E, False, ze)
        with pa.Selection(ctx, cuts, squares=True) as S, pa.SpotMap(ctx, [0.5], WINDOW, (NX, NY), energies=G.PUB_SEL, squares=True) as m, \
                pa.Histograms(ctx, G.PUB_HIST_AXES, energies=G.PUB_SEL, squares=True) as h, \
                pa.JointHistograms(ctx, G.PUB_JOINT_PAIRS, energies=G.PUB_SEL, squares=True) as j:
            tot = S.apply("exit")
            T, T_err = S.transmission("exit")
            for t in (m, h, j):
                t.add("exit", select=S)
            spot, hist, joint = m.read(), h.read(), j.read()
            errs = m.stderr(N), h.stderr(N)[0], j.stderr(N)[0]
    assert hist["squares"][0].any() and joint["squares"][0].any() and spot["squares"].any() and tot["passed_w2"][0].any()
    text = G.select_text(cuts)

    def public(binding=None, **env):
        monkeypatch.delenv("POLYCAP_TALLY_STDERR", raising=False)
        return G._public(monkeypatch, n, binding=binding, **env)[1]

    def same(e, what):
        s1, h1, j1, sel = e.spot("exit"), e.hist("exit"), e.joint("exit"), e.select()
        assert np.array_equal(s1["squares"], spot["squares"]) and np.array_equal(s1["outside_squares"], spot["outside_squares"]), what
        assert np.array_equal(s1["bins"], spot["bins"]) and np.array_equal(s1["stderr"], errs[0]), what
        assert np.array_equal(h1["squares"], hist["squares"][0]) and np.array_equal(h1["outside_squares"], hist["outside_squares"][0]), what
        assert np.array_equal(h1["bins"], hist["bins"][0]) and np.array_equal(h1["stderr"], errs[1]) and h1["n_started"] == N, what
        assert np.array_equal(h1["outside_stderr"], pa.tally_stderr(hist["outside"][0], hist["outside_squares"][0], N)), what
        assert np.array_equal(j1["squares"], joint["squares"][0]) and np.array_equal(j1["outside_squares"], joint["outside_squares"][0]), what
        assert np.array_equal(j1["stderr"], errs[2]), what
        assert np.array_equal(sel["passed_w2"], tot["passed_w2"]) and np.array_equal(sel["rejected_w2"], tot["rejected_w2"]), what
        assert np.array_equal(sel["passed_w"], tot["passed_w"]), what
        assert np.array_equal(sel["transmission"][0], T) and np.array_equal(sel["transmission_stderr"][0], T_err), what
        assert np.isnan(sel["transmission"][1:]).all(), what                                # kinds the run has not: P + R == 0

    env = dict(POLYCAP_TALLY_STDERR="1", POLYCAP_SELECT=text, POLYCAP_SPOT=G.PUB_SPOT, POLYCAP_HIST=G.PUB_HIST, POLYCAP_JOINT=G.PUB_JOINT)
    eff = public(**env)
    same(eff, "one run, photons kept")
    share = (n / 4.0) * (17 + 291) * 8.0 / total
    same(public(POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share, **env), "POLYCAP_IMAGES=0 in four chunks")
    same(public(POLYCAP_HIP_DEVICES="0,0", **env), "POLYCAP_HIP_DEVICES=0,0")
    from polycap_amd.pyext import polycap as cy
    same(public(binding=cy, **env), "cython")
    # unset, and 0: the accessors of the parent
    off = dict(env)
    del off["POLYCAP_TALLY_STDERR"]
    for e0 in (public(**off), public(**dict(off, POLYCAP_TALLY_STDERR="0"))):
        for acc in (e0.spot("exit"), e0.hist("exit"), e0.joint("exit")):
            assert not {"squares", "outside_squares", "stderr", "outside_stderr", "n_started"} & set(acc)
        assert not {"passed_w2", "rejected_w2", "transmission", "transmission_stderr"} & set(e0.select())
        assert np.array_equal(e0.hist("exit")["bins"], hist["bins"][0]) and np.array_equal(e0.data[1], eff.data[1])
    eff_off = e0
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_TALLY_STDERR", "yes")
    with pytest.raises(ValueError, match="POLYCAP_TALLY_STDERR"):
        capi.Source.new_from_file(DECK).get_transmission_efficiencies(1, 1000)
    monkeypatch.delenv("POLYCAP_TALLY_STDERR")
    # the tally variables alone, without a selection
    e1 = public(POLYCAP_TALLY_STDERR="1", POLYCAP_HIST=G.PUB_HIST)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, n, keep_images=True)
        with pa.Histograms(ctx, G.PUB_HIST_AXES, energies=G.PUB_SEL, squares=True) as h:
            h.add("exit")
            want = h.read()
    assert np.array_equal(e1.hist("exit")["squares"], want["squares"][0]) and np.array_equal(e1.hist("exit")["bins"], want["bins"][0])
    # HDF5
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    import subprocess
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    on, offp = str(tmp_path / "on.h5"), str(tmp_path / "off.h5")
    eff.write_hdf5(on)
    eff_off.write_hdf5(offp)
    ls_on, ls_off = H._listing(on), H._listing(offp)
    assert set(ls_on) - set(ls_off) == NEW_NAMES and set(ls_off) <= set(ls_on)              # unset: the names the file had before
    assert not NEW_NAMES & set(ls_off)
    assert ls_on["/Hist/Exit/Bins_Squares"] == ls_on["/Hist/Exit/Bins"] + (2,) and ls_on["/Hist/Exit/Bins_StdErr"] == ls_on["/Hist/Exit/Bins"]
    assert ls_on["/Joint/Exit/Cells_Squares"] == ls_on["/Joint/Exit/Cells"] + (2,) and ls_on["/Spot/Exit_Squares"] == ls_on["/Spot/Exit"] + (2,)
    assert ls_on["/Select/Passed_Squares"] == (3, 291, 2) and ls_on["/Select/Transmission_StdErr"] == (3, 291)

    def read_u64(dset):
        out_ = str(tmp_path / "u.bin")
        subprocess.run([H.H5DUMP, "-d", dset, "-b", "LE", "-o", out_, on], check=True, capture_output=True)
        return np.fromfile(out_, dtype="<u8")

    assert np.array_equal(read_u64("/Hist/Exit/Bins_Squares").reshape(hist["squares"][0].shape), hist["squares"][0])
    assert np.array_equal(read_u64("/Select/Passed_Squares").reshape(3, 291, 2), tot["passed_w2"])
    assert np.array_equal(H._read(on, "/Hist/Exit/Bins_StdErr", str(tmp_path)).reshape(errs[1].shape), errs[1])


def test_public_leak_run(pa, monkeypatch):
    """leak_calc through the public call, on one device and on a group: every kind's squares equal the thin ABI's of the same run"""
    from tests import test_gpu_select as G
    n = 3000
    hist_text, axes = "axis=z,range=0:10,bins=50;axis=nrefl,range=0:256,bins=32", [axis("z", 0., 10., 50), axis("nrefl", 0., 256., 32)]
    prob = pa.problem_from_inp(DECK)
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=True)
        with pa.Histograms(ctx, axes, squares=True) as h:
            for kind in KINDS:
                h.add(kind)
            hist = h.read()
    assert all(hist["squares"][k].any() for k in range(3))
    monkeypatch.delenv("POLYCAP_TALLY_STDERR", raising=False)
    _, eff = G._public(monkeypatch, n, leak_calc=True, POLYCAP_TALLY_STDERR="1", POLYCAP_HIST=hist_text)
    _, effg = G._public(monkeypatch, n, leak_calc=True, POLYCAP_TALLY_STDERR="1", POLYCAP_HIST=hist_text, POLYCAP_HIP_DEVICES="0,0")
    for e in (eff, effg):
        for kind, k in KINDS.items():
            a = e.hist(kind)
            assert np.array_equal(a["bins"], hist["bins"][k]) and np.array_equal(a["squares"], hist["squares"][k]), kind
            assert np.array_equal(a["outside_squares"], hist["outside_squares"][k]) and a["n_started"] == r["i_start"], kind

"""Selections on the GPU (pc_hip_select_*, Selection, tally.add(kind, select=...)): the mask totals equal numpy on the run's own
fetched records, integer for integer; each of the four tallies filled through a selection equals the same tally computed in numpy
from the filtered records; a selection and its complement add up to the plain add cell by cell; refusals leave every object
unchanged; and nothing depends on how the run was launched.  Every cut's threshold is the median of its quantity over the fetched
records, and every test first asserts that between 10 % and 90 % of the entries pass: a selection that gates nothing or everything
proves nothing."""
import numpy as np
import pytest

from tests.test_beam_cpu import PAIRS, to_lohi
from tests.test_gpu_hist import DECK, KINDS, SEED, _prob, exit_entries, leak_entries, record_entries
from tests.test_hist_cpu import np_bins, np_hist, np_value
from tests.test_joint_cpu import QUANTITIES, axis, np_joint, np_value2
from tests.test_select_cpu import cut, np_pass
from tests.test_spot_cpu import np_q, np_spot_bin

pytestmark = pytest.mark.gpu

WINDOW, NX, NY, D_SPOT = (-0.004, 0.0055, -0.003, 0.0047), 37, 29, 0.5


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


# ---- the restatements of tests/test_gpu_spot.py, test_gpu_beam.py and test_gpu_hist.py, on entries [n, 10] ------------------------
def np_map(E, W, zps, window, nx, ny):
    """bins uint64 [P, S, ny, nx], outside [P, S]"""
    Q = np_q(W)
    P, S = len(zps), W.shape[1]
    bins = np.zeros((P, S, ny * nx), dtype=np.uint64)
    out = np.zeros((P, S), dtype=np.uint64)
    for p, zp in enumerate(zps):
        b = np_spot_bin(E[:, 0], E[:, 1], E[:, 2], E[:, 3], E[:, 4], E[:, 5], zp, window, nx, ny)
        ins = b >= 0
        for s in range(S):
            np.add.at(bins[p, s], b[ins], Q[ins, s])
            out[p, s] = Q[~ins, s].sum(dtype=np.uint64)
    return bins.reshape(P, S, ny, nx), out


def np_quantise(pos, dirs, ze):
    with np.errstate(all="ignore"):
        dz = dirs[:, 2]
        t = (ze - pos[:, 2]) / dz
        xe, ye = pos[:, 0] + dirs[:, 0] * t, pos[:, 1] + dirs[:, 1] * t
        sx, sy = dirs[:, 0] / dz, dirs[:, 1] / dz
        r = np.stack([np.rint(v * 16777216.0) for v in (xe, ye, sx, sy)], axis=1)
        ok = (dz > 0.) & np.all(np.abs(r) < 2.0 ** 31, axis=1)
    q = np.zeros(r.shape, dtype=np.int64)
    q[ok] = r[ok].astype(np.int64)
    return q, ok


def np_beam(E, W, ze):
    """(lo, hi) sums uint64 [nE, 15, 2] (signed 128-bit, two's complement) and outside uint64 [nE]"""
    q, ok = np_quantise(E[:, 0:3], E[:, 3:6], ze)
    Q = np_q(W)
    out = Q[~ok].sum(axis=0, dtype=np.uint64)
    Q, q = Q[ok].astype(np.int64), q[ok]
    P = np.empty((len(q), 15), dtype=np.int64)
    P[:, 0] = 1
    P[:, 1:5] = q
    for k, (a, b) in enumerate(PAIRS):
        P[:, 5 + k] = q[:, a] * q[:, b]
    wl = [(Q >> (11 * j)) & 0x7ff for j in range(3)]
    pl = [P & 0x1fffff, (P >> 21) & 0x1fffff, P >> 42]
    S = np.zeros((W.shape[1], 15), dtype=object)
    for j in range(3):
        for l in range(3):
            S += (wl[j].T @ pl[l]).astype(object) * (1 << (11 * j + 21 * l))
    return np.stack([to_lohi([int(v) for v in S[e]]) for e in range(W.shape[1])]), out


def np_hists(axes, E, W, ze, leak):
    Q = np_q(W)
    bins, outs = [], []
    for a in axes:
        v, ok = np_value(QUANTITIES.index(a["axis"]), E, leak, ze + a["d"], *a["centre"])
        H, out = np_hist(np_bins(v, ok, a["range"][0], a["range"][1], a["bins"]), Q, a["bins"])
        bins.append(H)
        outs.append(out)
    return np.concatenate(bins, axis=1), np.stack(outs)


# ---- the four tallies, in every regime, as one object -----------------------------------------------------------------------------
def values(name, E, leak, ze, d=0., centre=(0., 0.)):
    v, ok = np_value2(QUANTITIES.index(name), E, leak, ze + d, *centre)
    return v[ok & np.isfinite(v)]


def spread_axis(name, E, leak, ze, bins, d=0., centre=(0., 0.)):
    """an axis over the 15th to the 80th percentile of the entries' own values: weight inside and outside"""
    v = values(name, E, leak, ze, d, centre)
    lo, hi = (float(np.percentile(v, 15)), float(np.percentile(v, 80))) if len(v) else (0., 1.)
    if not lo < hi:
        lo, hi = lo - 1., lo + 1.
    return axis(name, lo, hi, bins, d=d, centre=centre)


def config(E, ze, leak=False):
    if leak:
        return dict(axes=[spread_axis("z", E, True, ze, 21), axis("nrefl", 0., 64., 64), axis("r_start", 0., 1., 4)],
                    pairs=[(spread_axis("z", E, True, ze, 12), axis("nrefl", 0., 256., 32)), (axis("start_x", -1., 1., 8), axis("nrefl", 0., 256., 8))])
    return dict(axes=[spread_axis("x", E, False, ze, 65, d=0.5), spread_axis("r", E, False, ze, 40, d=0.25, centre=(0.002, -0.001)),
                      axis("nrefl", 0., 256., 256), spread_axis("r_start", E, False, ze, 47)],
                pairs=[(spread_axis("x", E, False, ze, 33, d=0.5), spread_axis("slope_x", E, False, ze, 31)),
                       (spread_axis("start_x", E, False, ze, 24), spread_axis("start_y", E, False, ze, 20))])


class Tallies:
    """a spot map, histograms and joint histograms in both regimes, and beam moments, on one owner"""

    def __init__(self, pa, owner, cfg):
        self.cfg = cfg
        self.t = {"beam": pa.BeamMoments(owner)}
        for regime in (1, 2):
            self.t["spot%d" % regime] = pa.SpotMap(owner, [D_SPOT], WINDOW, (NX, NY), regime=regime)
            self.t["hist%d" % regime] = pa.Histograms(owner, cfg["axes"], regime=regime)
            self.t["joint%d" % regime] = pa.JointHistograms(owner, cfg["pairs"], regime=regime)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for t in self.t.values():
            t.close()

    def reset(self):
        for t in self.t.values():
            t.reset()

    def add(self, kind, select=None):
        for t in self.t.values():
            t.add(kind, select=select)

    def read(self, kind):
        """per tally (cells, outside, entries) of `kind`; a spot map keeps one map for all kinds"""
        k = KINDS[kind]
        out = {}
        for name, t in self.t.items():
            r = t.read()
            if name.startswith("spot"):
                out[name] = (r["bins"], r["outside"], int(r["n_entries"]))
            else:
                key = {"b": "sums", "h": "bins", "j": "cells"}[name[0]]
                out[name] = (r[key][k], r["outside"][k], int(r["n_entries"][k]))
        return out


def expect(cfg, E, W, ze, leak=False):
    """what Tallies.read gives after one add of the entries E, W, by numpy alone"""
    n = len(E)
    spot = np_map(E, W, [ze + D_SPOT], WINDOW, NX, NY) + (n,)
    hist = np_hists(cfg["axes"], E, W, ze, leak) + (n,)
    joint = np_joint(cfg["pairs"], E, W, ze, None, leak) + (n,)
    return {"beam": np_beam(E, W, ze) + (n,), "spot1": spot, "spot2": spot, "hist1": hist, "hist2": hist, "joint1": joint, "joint2": joint}


def same(got, want, what=""):
    assert set(got) == set(want)
    for name in want:
        for part, g, w in zip(("cells", "outside", "entries"), got[name], want[name]):
            assert np.array_equal(g, w), "%s: %s differ %s" % (name, part, what)


def add128(a, b):
    """(lo, hi) pairs uint64 [..., 2] added mod 2^128"""
    lo = a[..., 0] + b[..., 0]
    hi = a[..., 1] + b[..., 1] + (lo < a[..., 0]).astype(np.uint64)
    return np.stack([lo, hi], axis=-1)


def summed(a, b):
    """two reads added cell by cell: what the adds of both into one object give"""
    out = {}
    for name in a:
        cells = add128(a[name][0], b[name][0]) if name == "beam" else a[name][0] + b[name][0]
        out[name] = (cells, a[name][1] + b[name][1], a[name][2] + b[name][2])
    return out


# ---- cuts through the data -------------------------------------------------------------------------------------------------------
def median_cut(name, E, leak, ze, d=0., centre=(0., 0.), negate=False):
    """[lowest value, median) of the quantity over the entries; where so many entries sit on the median itself that fewer than 10 %
    are below it (whole numbers, events on one plane), the median's own value is taken in: [lowest value, the next double above it)"""
    v = values(name, E, leak, ze, d, centre)
    lo, hi = float(v.min()), float(np.median(v))
    if (v < hi).sum() < 0.1 * len(E):
        hi = float(np.nextafter(hi, np.inf))
    return cut(name, lo, hi, d=d, centre=centre, negate=negate)


def real_selection(cuts, E, leak, ze):
    """the numpy mask, after asserting that between 10 % and 90 % of the entries pass"""
    p = np_pass(cuts, E, leak, ze)
    assert 0.1 * len(E) <= p.sum() <= 0.9 * len(E), "the selection passes %d of %d entries" % (p.sum(), len(E))
    return p


def check_totals(res, kind, p, W):
    k = KINDS[kind]
    Q = np_q(W)
    assert res["n_pass"][k] == int(p.sum()) and res["n_seen"][k] == len(p)
    passed = [sum(int(v) for v in Q[p, e]) for e in range(W.shape[1])]
    rejected = [sum(int(v) for v in Q[~p, e]) for e in range(W.shape[1])]
    assert [int(v) for v in res["passed_w"][k]] == passed and [int(v) for v in res["rejected_w"][k]] == rejected
    assert [a + b for a, b in zip(passed, rejected)] == [sum(int(v) for v in Q[:, e]) for e in range(W.shape[1])]


EXIT_CUTS = (("r", dict(d=0.5)), ("nrefl", {}), ("tan_theta", {}), ("r_start", {}), ("start_x", {}), ("dtravel", {}))


# ---- 1, 2, 3: totals, gated tallies and the complement against numpy ---------------------------------------------------------------
@pytest.mark.parametrize("ne,n,opts", [(1, 60000, {}), (3, 20000, {}), (12, 12000, {}), (12, 12000, {"batch_reflections": 0})])
def test_exit_selection_equals_numpy(pa, ne, n, opts):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        E, W = record_entries(ctx.records())
        cfg = config(E, ze)
        with Tallies(pa, ctx, cfg) as T:
            T.add("exit")
            plain = T.read("exit")
            same(plain, expect(cfg, E, W, ze), "(plain add)")
            for name, kw in EXIT_CUTS:
                c = median_cut(name, E, False, ze, **kw)
                cn = dict(c, **{"not": True})
                p = real_selection([c], E, False, ze)
                with pa.Selection(ctx, [c]) as S, pa.Selection(ctx, [cn]) as Sn:
                    assert S.cuts == [c] and S.n_energies == ne
                    res, resn = S.apply("exit"), Sn.apply("exit")
                    check_totals(res, "exit", p, W)
                    check_totals(resn, "exit", ~p, W)
                    assert not res["n_seen"][1:].any() and not res["passed_w"][1:].any()
                    T.reset()
                    T.add("exit", select=S)
                    gated = T.read("exit")
                    same(gated, expect(cfg, E[p], W[p], ze), "(gated by %s)" % name)
                    # sum(bins) + outside == passed_w per axis, pair and energy
                    for key in ("hist1", "hist2", "joint1", "joint2"):
                        off = np.cumsum([0] + ([a["bins"] for a in cfg["axes"]] if key[0] == "h" else [u["bins"] * v["bins"] for u, v in cfg["pairs"]]))
                        for a in range(len(off) - 1):
                            tot = gated[key][0][:, off[a]:off[a + 1]].sum(axis=1, dtype=np.uint64) + gated[key][1][a]
                            assert np.array_equal(tot, res["passed_w"][0]), (key, a)
                    T.reset()
                    T.add("exit", select=Sn)
                    same(summed(gated, T.read("exit")), plain, "(%s and its complement)" % name)
                    # gated and plain adds mix in one object
                    T.add("exit", select=S)
                    same(T.read("exit"), plain, "(complement, then the selection, into one object)")


def test_eight_cuts_and_the_pinhole(pa):
    """8 cuts ANDed; and test 5: an R_AT cut [0, r) under a histogram of R_AT over [0, 2r) leaves its upper half and outside empty"""
    prob = _prob(pa, 3)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, 20000, keep_images=True)
        ctx.wait()
        E, W = record_entries(ctx.records())
        wide = lambda name, **kw: (lambda v: cut(name, float(np.percentile(v, 4)), float(np.percentile(v, 96)), **kw))(values(name, E, False, ze, kw.get("d", 0.)))
        cuts = [wide("x", d=0.5), wide("y", d=0.5), wide("slope_x"), wide("slope_y"), wide("start_x"), wide("start_y"), wide("dtravel"),
                cut("nrefl", 0., 1., negate=True)]
        p = real_selection(cuts, E, False, ze)
        cfg = config(E, ze)
        with pa.Selection(ctx, cuts) as S, Tallies(pa, ctx, cfg) as T:
            assert S.n_cuts == 8
            check_totals(S.apply("exit"), "exit", p, W)
            T.add("exit", select=S)
            same(T.read("exit"), expect(cfg, E[p], W[p], ze), "(8 cuts)")
        r = float(np.median(values("r", E, False, ze, 0.5)))
        c = cut("r", 0., r, d=0.5)
        p = real_selection([c], E, False, ze)
        for regime in (1, 2):
            with pa.Selection(ctx, [c]) as S, pa.Histograms(ctx, [axis("r", 0., 2. * r, 64, d=0.5)], regime=regime) as h:
                res = S.apply("exit")
                h.add("exit")
                plain = h.read()
                h.reset()
                h.add("exit", select=S)
                got = h.read()
                assert plain["bins"][0][:, 32:].any() and got["bins"][0][:, :32].any()
                assert not got["bins"][0][:, 32:].any() and not got["outside"][0].any()
                assert np.array_equal(got["bins"][0][:, :32], plain["bins"][0][:, :32])
                assert np.array_equal(got["bins"][0].sum(axis=1, dtype=np.uint64), res["passed_w"][0])
                assert got["n_entries"].tolist() == [int(p.sum()), 0, 0]


def test_all_holding_selection_is_the_plain_add(pa):
    prob = _prob(pa, 3)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, 20000, keep_images=True, max_attempts=1)          # failed slots: entries without an exit plane
        ctx.wait()
        assert ctx.totals(check=False)["failed_slots"] > 100
        E, W = record_entries(ctx.records())
        cfg = config(E, ze)
        with pa.Selection(ctx, [cut("z", -1e300, 1e300)]) as S, Tallies(pa, ctx, cfg) as T:
            res = S.apply("exit")
            assert res["n_pass"][0] == res["n_seen"][0] == 20000 and not res["rejected_w"].any()
            T.add("exit")
            plain = T.read("exit")
            same(plain, expect(cfg, E, W, ze), "(plain add)")
            T.reset()
            T.add("exit", select=S)
            same(T.read("exit"), plain, "(a selection that holds everything)")


# ---- leak kinds --------------------------------------------------------------------------------------------------------------------
def test_leak_kinds(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True, leak_calc=True)
        ents = {"extleak": leak_entries(r["ext"]), "intleak": leak_entries(r["int"]), "exit": exit_entries(r["images"], r["exit_weights"])}
        assert len(ents["extleak"][0]) > 100 and len(ents["intleak"][0]) > 100
        for kind in ("extleak", "intleak"):
            E, W = ents[kind]
            cfg = config(E, ze, leak=True)
            for name in ("nrefl", "x", "slope_x"):
                c = median_cut(name, E, True, ze)
                cn = dict(c, **{"not": True})
                p = real_selection([c], E, True, ze)
                with pa.Selection(ctx, [c]) as S, pa.Selection(ctx, [cn]) as Sn, Tallies(pa, ctx, cfg) as T:
                    check_totals(S.apply(kind), kind, p, W)
                    check_totals(Sn.apply(kind), kind, ~p, W)
                    T.add(kind)
                    plain = T.read(kind)
                    same(plain, expect(cfg, E, W, ze, leak=True), "(%s, plain)" % kind)
                    T.reset()
                    T.add(kind, select=S)
                    gated = T.read(kind)
                    same(gated, expect(cfg, E[p], W[p], ze, leak=True), "(%s gated by %s)" % (kind, name))
                    T.reset()
                    T.add(kind, select=Sn)
                    same(summed(gated, T.read(kind)), plain, "(%s: %s and its complement)" % (kind, name))
            # a quantity the kind does not have: nothing is inside, so the cut passes nothing and its negation everything
            with pa.Selection(ctx, [cut("r_start", 0., 1.)]) as S, pa.Selection(ctx, [cut("start_x", -1., 1., negate=True)]) as Sn, Tallies(pa, ctx, cfg) as T:
                k = KINDS[kind]
                a, b = S.apply(kind), Sn.apply(kind)
                assert a["n_pass"][k] == 0 and a["n_seen"][k] == len(E) and not a["passed_w"].any()
                assert b["n_pass"][k] == len(E) and not b["rejected_w"].any() and np.array_equal(b["passed_w"][k], a["rejected_w"][k])
                T.add(kind, select=S)
                got = T.read(kind)
                assert all(not v[0].any() and not v[1].any() and v[2] == 0 for v in got.values())
                T.add(kind, select=Sn)
                same(T.read(kind), expect(cfg, E, W, ze, leak=True), "(%s, the negated cut on a quantity it lacks)" % kind)
        # one selection applied for all three kinds
        E, W = ents["exit"]
        c = median_cut("nrefl", E, False, ze)
        with pa.Selection(ctx, [c]) as S:
            for kind in KINDS:
                res = S.apply(kind)
            for kind in KINDS:
                check_totals(res, kind, np_pass([c], ents[kind][0], kind != "exit", ze), ents[kind][1])


# ---- 6: seams ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 3])
def test_seams(pa, ne):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, 20000, keep_images=True)
        ctx.wait()
        E0, _ = record_entries(ctx.records())
        cfg = config(E0, ze)
        c = median_cut("r", E0, False, ze, d=0.5)
        with pa.Selection(ctx, [c]) as S, pa.Selection(ctx, [cut("z", 1e6, 2e6)]) as Snone, Tallies(pa, ctx, cfg) as T:
            for n in (1, 63, 64, 65, 257):                                      # too few to ask for 10 % to 90 %: the cut is that of the big run
                ctx.run(SEED + n, 0, n, keep_images=True, max_attempts=1)       # few of the slots transmit: the others have no exit plane
                ctx.wait()
                E, W = record_entries(ctx.records())
                assert len(E) == n
                p = np_pass([c], E, False, ze)
                check_totals(S.apply("exit"), "exit", p, W)
                T.reset()
                T.add("exit", select=S)
                same(T.read("exit"), expect(cfg, E[p], W[p], ze), "(%d entries, %d pass)" % (n, p.sum()))
                res = Snone.apply("exit")                                        # zero passing
                assert res["n_pass"][0] == 0 and res["n_seen"][0] == n and not res["passed_w"].any()
                before = T.read("exit")
                T.add("exit", select=Snone)
                same(T.read("exit"), before, "(a selection that passes nothing)")


def test_relay_and_a_relay_without_records(pa, oracle):
    from tests.test_gpu_relay import N as N_RELAY, SEED as SEED_RELAY, problems
    _, _, prob_a, _, prob_b, _ = problems(oracle, "pinned")
    ze = float(prob_b.z[-1])
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.run(SEED_RELAY, 0, N_RELAY, keep_images=True)
        r = ctx_a.relay(ctx_b, 1.0)
        E, W = record_entries(ctx_b.records())
        assert len(E) == r["n_records"] > 1000
        cfg = config(E, ze)
        c = median_cut("tan_theta", E, False, ze)
        p = real_selection([c], E, False, ze)
        with pa.Selection(ctx_b, [c]) as S, Tallies(pa, ctx_b, cfg) as T:
            check_totals(S.apply("exit"), "exit", p, W)
            T.add("exit", select=S)
            want = expect(cfg, E[p], W[p], ze)
            same(T.read("exit"), want, "(relay)")
            # a relay into the context replaces its entries: the mask is stale
            r0 = ctx_a.relay(ctx_b, 1.0, (0.1, 0.))
            assert r0["n_records"] == 0
            with pytest.raises(pa.HipError) as e:
                T.add("exit", select=S)
            assert e.value.status == -2 and "stale" in str(e.value)
            same(T.read("exit"), want, "(after the refusal)")
            res = S.apply("exit")                                                # zero records
            assert not res["n_pass"].any() and not res["n_seen"].any() and not res["passed_w"].any() and not res["rejected_w"].any()
            T.add("exit", select=S)
            same(T.read("exit"), want, "(a relay without records adds nothing)")


# ---- 7: launch invariance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 3])
def test_launch_invariance(pa, ne):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    N = 196608                      # 3 launches with run_parts >= 3 (a run is cut into at most n / 65536 launches)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, 20000, keep_images=True)
        ctx.wait()
        E, W = record_entries(ctx.records())
        cfg = config(E, ze)
        cuts = [median_cut("r", E, False, ze, d=0.5), cut("nrefl", 0., float(np.percentile(values("nrefl", E, False, ze), 80)))]
        real_selection(cuts, E, False, ze)
        with pa.Selection(ctx, cuts) as S, Tallies(pa, ctx, cfg) as T:
            def sums_of(runs):
                T.reset()
                tot = None
                for run in runs:
                    run()
                    res = S.apply("exit")
                    T.add("exit", select=S)
                    part = (int(res["n_pass"][0]), int(res["n_seen"][0]), res["passed_w"][0].copy(), res["rejected_w"][0].copy())
                    tot = part if tot is None else tuple(a + b for a, b in zip(tot, part))
                return tot, T.read("exit")

            ref_tot, ref = sums_of([lambda: ctx.run(SEED, 0, N, keep_images=True)])
            assert ref_tot[1] == N and 0.1 * N <= ref_tot[0] <= 0.9 * N
            assert all(v[2] == ref_tot[0] for v in ref.values())

            def agree(got, what):
                tot, res = got
                assert tot[:2] == ref_tot[:2] and np.array_equal(tot[2], ref_tot[2]) and np.array_equal(tot[3], ref_tot[3]), what
                same(res, ref, what)

            ctx.set_option("run_parts", 4)
            agree(sums_of([lambda: ctx.run(SEED, 0, N, keep_images=True)]), "(run_parts 4)")
            ctx.set_option("run_parts", 1)
            ctx.set_option("plane_images", 1)
            ctx.set_option("compact_images", 1)
            agree(sums_of([lambda: ctx.run(SEED, 0, N, keep_images=True)]), "(compact planes)")
            ctx.set_option("compact_images", 0)
            agree(sums_of([lambda: ctx.run(SEED, 0, N, keep_images=True)]), "(slot-order planes)")
            ctx.set_option("plane_images", 0)
            agree(sums_of([lambda: ctx.run(SEED, 0, N // 2, keep_images=True), lambda: ctx.run(SEED, N // 2, N - N // 2, keep_images=True)]),
                  "(two runs)")
    with pa.TraceGroup(prob, [0, 0]) as g:
        with pa.Selection(g, cuts) as S, Tallies(pa, g, cfg) as T:
            g.transmission(SEED, N, keep_images=True)
            res = S.apply("exit")
            T.add("exit", select=S)
            agree(((int(res["n_pass"][0]), int(res["n_seen"][0]), res["passed_w"][0], res["rejected_w"][0]), T.read("exit")), "(group [0, 0])")


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_objects_unchanged(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx, pa.TraceContext(prob, 0) as other, pa.TraceGroup(prob, [0, 0]) as g:
        ctx.run(SEED, 0, 5000, keep_images=True)
        ctx.wait()
        E, W = record_entries(ctx.records())
        cfg = config(E, ze)
        c = median_cut("r", E, False, ze, d=0.5)
        p = real_selection([c], E, False, ze)
        with pa.Selection(ctx, [c]) as S, Tallies(pa, ctx, cfg) as T:
            def refused(fn, words):
                before_t, before_s = T.read("exit"), S.read()
                with pytest.raises(pa.HipError) as e:
                    fn()
                assert e.value.status == -2 and all(w in str(e.value) for w in words), str(e.value)
                same(T.read("exit"), before_t, "(after the refusal)")
                after = S.read()
                assert all(np.array_equal(after[k], before_s[k]) for k in after)

            refused(lambda: T.t["hist1"].add("exit", select=S), ["pc_hip_hist_add_selected", "not applied for kind 0"])
            S.apply("exit")
            T.add("exit", select=S)
            want = expect(cfg, E[p], W[p], ze)
            same(T.read("exit"), want)
            for name, stem in (("spot2", "spot"), ("beam", "beam"), ("hist2", "hist"), ("joint1", "joint")):
                refused(lambda: T.t[name].add("extleak", select=S), ["pc_hip_%s_add_selected" % stem, "leak events need a leak_calc source run"])
                refused(lambda: T.t[name].add(3, select=S), ["pc_hip_%s_add_selected" % stem, "kind must be 0"])
            # wrong owner: another context's selection, a group's selection, a context's selection on a group's tally
            other.run(SEED, 0, 5000, keep_images=True)
            g.transmission(SEED, 5000, keep_images=True)
            with pa.Selection(other, [c]) as So, pa.Selection(g, [c]) as Sg, pa.Histograms(g, cfg["axes"]) as hg:
                So.apply("exit")
                Sg.apply("exit")
                for name in T.t:
                    refused(lambda: T.t[name].add("exit", select=So), ["different owners"])
                    refused(lambda: T.t[name].add("exit", select=Sg), ["different owners"])
                with pytest.raises(pa.HipError) as e:
                    hg.add("exit", select=S)
                assert e.value.status == -2 and "different owners" in str(e.value) and not hg.read()["bins"].any()
                hg.add("exit", select=Sg)                                         # the group's own selection: the same sums
                assert np.array_equal(hg.read()["bins"][0], want["hist1"][0]) and hg.read()["n_entries"][0] == int(p.sum())
            # a scan replaces nothing: the mask stays good
            ctx.scan(SEED, pa.scan_points(x=(0., 0.01)), 64)
            T.add("exit", select=S)
            same(T.read("exit"), summed(want, want), "(after a scan)")
            # stale: a new run of the same slots, an explicit launch
            ctx.run(SEED, 0, 5000, keep_images=True)
            for name in T.t:
                refused(lambda: T.t[name].add("exit", select=S), ["stale"])
            S.apply("exit")
            T.add("exit", select=S)
            same(T.read("exit"), summed(summed(want, want), want), "(applied anew)")
            # the last run kept no exit photons
            ctx.run(SEED, 0, 5000, keep_images=False)
            refused(lambda: T.t["joint2"].add("exit", select=S), ["kept no exit photons"])
            with pytest.raises(pa.HipError) as e:
                S.apply("exit")
            assert e.value.status == -2 and "pc_hip_select_apply: the last run kept no exit photons" in str(e.value)
        with pytest.raises(pa.HipError) as e:
            pa.Selection(ctx, [c, dict(c, range=(0.01, -0.01))])
        assert e.value.status == -2 and "cut 1: lo" in str(e.value)


def test_the_entry_cap_counts_n_pass(pa):
    """A tally takes 2^32 - 1 entries per kind.  Gated adds of a run of N entries of which P pass fit (2^32 - 1) // P times, about
    twice as often as adds that counted N would; the next one is refused with every object unchanged.  Reached as it can be reached:
    by adding one run's passing entries again and again (an add of a million entries to one small histogram is an enqueue)."""
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    ze = float(prob.z[-1])
    N, CAP = 1000000, (1 << 32) - 1
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, 20000, keep_images=True)
        ctx.wait()
        E, W = record_entries(ctx.records())
        c = median_cut("r", E, False, ze, d=0.5)
        real_selection([c], E, False, ze)
        ctx.run(SEED, 0, N, keep_images=True)
        with pa.Selection(ctx, [c]) as S, pa.Histograms(ctx, [axis("nrefl", 0., 256., 64)], regime=1) as h:
            res = S.apply("exit")
            P = int(res["n_pass"][0])
            assert res["n_seen"][0] == N and 0.1 * N <= P <= 0.9 * N
            K = CAP // P
            assert K > CAP // N + 1000                   # far more adds than a count of all entries would allow
            for _ in range(K):
                h.add("exit", select=S)
            before = h.read()
            assert before["n_entries"].tolist() == [K * P, 0, 0]
            assert [int(v) for v in before["bins"][0].sum(axis=1, dtype=np.uint64) + before["outside"][0, 0]] == [K * int(res["passed_w"][0, 0])]
            for add in (lambda: h.add("exit", select=S), lambda: h.add("exit")):
                with pytest.raises(pa.HipError) as e:
                    add()
                assert e.value.status == -2 and "2^32 - 1 entries" in str(e.value)
            after, tot = h.read(), S.read()
            assert after["n_entries"].tolist() == [K * P, 0, 0]
            assert np.array_equal(after["bins"], before["bins"]) and np.array_equal(after["outside"], before["outside"])
            assert all(np.array_equal(tot[k], res[k]) for k in res)


# ---- 9: the public call ----------------------------------------------------------------------------------------------------------
PUB_VARS = ("POLYCAP_SELECT", "POLYCAP_JOINT", "POLYCAP_HIST", "POLYCAP_BEAM", "POLYCAP_IMAGES", "POLYCAP_SPOT_SHARE", "POLYCAP_HIP_DEVICES",
            "POLYCAP_SPOT", "POLYCAP_STDERR")
PUB_SEL = [200, 0, 90]
PUB_SPOT = "dist=0.5;window=-0.004,0.0055,-0.003,0.0047;bins=37x29;energies=200,0,90"
PUB_HIST = "axis=x,d=0.5,range=-0.004:0.0055,bins=333;axis=nrefl,range=0:256,bins=256;energies=200,0,90"
PUB_HIST_AXES = [dict(axis="x", d=0.5, range=(-0.004, 0.0055), bins=333), dict(axis="nrefl", range=(0, 256), bins=256)]
PUB_JOINT = "axis=x,d=0.5,range=-0.004:0.0055,bins=33*axis=slope_x,range=-0.002:0.0015,bins=31;energies=200,0,90"
PUB_JOINT_PAIRS = [(axis("x", -0.004, 0.0055, 33, d=0.5), axis("slope_x", -0.002, 0.0015, 31))]


def _public(monkeypatch, n, binding=None, leak_calc=False, **env):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k in PUB_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = (binding or capi).Source.new_from_file(DECK)
    return src, src.get_transmission_efficiencies(1, n, leak_calc=leak_calc)


def select_text(cuts):
    """cuts as POLYCAP_SELECT takes them, every number with 17 digits: the same doubles"""
    return ";".join("axis=%s,d=%.17g,centre=%.17g:%.17g,range=%.17g:%.17g%s" % (c["axis"], c["d"], c["centre"][0], c["centre"][1], c["range"][0],
                                                                                 c["range"][1], ",not" if c["not"] else "")
                    if c["axis"] == "r" else "axis=%s,range=%.17g:%.17g%s" % (c["axis"], c["range"][0], c["range"][1], ",not" if c["not"] else "")
                    for c in cuts)


def test_public_api(pa, monkeypatch, tmp_path):
    n = 12000
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        total = ctx.device_memory()[1]
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        E, W = record_entries(ctx.records())
        nr = values("nrefl", E, False, ze)
        cuts = [median_cut("r", E, False, ze, d=0.5), cut("nrefl", 0., float(np.percentile(nr, 20)), negate=True)]
        p = real_selection(cuts, E, False, ze)
        with pa.Selection(ctx, cuts) as S, pa.SpotMap(ctx, [0.5], WINDOW, (NX, NY), energies=PUB_SEL) as m, pa.BeamMoments(ctx) as b, \
                pa.Histograms(ctx, PUB_HIST_AXES, energies=PUB_SEL) as h, pa.JointHistograms(ctx, PUB_JOINT_PAIRS, energies=PUB_SEL) as j:
            tot = S.apply("exit")
            check_totals(tot, "exit", p, W)
            for t in (m, b, h, j):
                t.add("exit", select=S)
            spot, beam, hist, joint = m.read(), b.read(), h.read(), j.read()
    text = select_text(cuts)
    assert pa.select_parse(text) == cuts

    def same_select(eff, what):
        s = eff.select()
        assert s["cuts"] == cuts, what
        for k in ("n_pass", "n_seen", "passed_w", "rejected_w"):
            assert np.array_equal(s[k], tot[k]) and s[k].dtype == tot[k].dtype, (what, k)
        return s

    # each of the four tally variables with POLYCAP_SELECT, histogram-only (chunked in four) and with the photons kept
    share = (n / 4.0) * (17 + 291) * 8.0 / total
    small = dict(POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    _, e_spot = _public(monkeypatch, n, POLYCAP_SELECT=text, POLYCAP_SPOT=PUB_SPOT, **small)
    _, F = e_spot.data
    same_select(e_spot, "spot")
    s1 = e_spot.spot_map("exit")
    bins = spot["bins"]
    tt = bins.reshape(1, 3, -1).sum(axis=2, dtype=np.uint64) + spot["outside"]
    assert np.array_equal(tt[0], tot["passed_w"][0][PUB_SEL])
    assert np.array_equal(s1["maps"], F[PUB_SEL][None, :, None, None] * bins.astype(np.float64) / tt.astype(np.float64)[:, :, None, None])
    _, e_beam = _public(monkeypatch, n, POLYCAP_SELECT=text, POLYCAP_BEAM="1", **small)
    same_select(e_beam, "beam")
    b1 = e_beam.beam("exit")
    assert np.array_equal(b1["sums"], beam["sums"][0]) and np.array_equal(b1["outside"], beam["outside"][0]) and b1["n_entries"] == int(p.sum())
    _, e_hist = _public(monkeypatch, n, POLYCAP_SELECT=text, POLYCAP_HIST=PUB_HIST, **small)
    same_select(e_hist, "hist")
    h1 = e_hist.hist("exit")
    assert np.array_equal(h1["bins"], hist["bins"][0]) and np.array_equal(h1["outside"], hist["outside"][0]) and h1["n_entries"] == int(p.sum())
    _, e_joint = _public(monkeypatch, n, POLYCAP_SELECT=text, POLYCAP_JOINT=PUB_JOINT, **small)
    same_select(e_joint, "joint")
    j1 = e_joint.joint("exit")
    assert np.array_equal(j1["cells"], joint["cells"][0]) and np.array_equal(j1["outside"], joint["outside"][0]) and j1["n_entries"] == int(p.sum())
    # all at once with the photons kept, on a group, and the selection alone
    both = dict(POLYCAP_SELECT=text, POLYCAP_HIST=PUB_HIST, POLYCAP_JOINT=PUB_JOINT, POLYCAP_BEAM="1", POLYCAP_SPOT=PUB_SPOT)
    for what, env in (("one run", both), ("POLYCAP_HIP_DEVICES=0,0", dict(both, POLYCAP_HIP_DEVICES="0,0"))):
        _, e2 = _public(monkeypatch, n, **env)
        same_select(e2, what)
        assert np.array_equal(e2.data[1], F), what
        assert np.array_equal(e2.hist("exit")["bins"], h1["bins"]) and np.array_equal(e2.joint("exit")["cells"], j1["cells"]), what
        assert np.array_equal(e2.beam("exit")["sums"], b1["sums"]) and np.array_equal(e2.spot_map("exit")["maps"], s1["maps"]), what
        if what == "one run":
            eff_all = e2
    _, e_only = _public(monkeypatch, n, POLYCAP_SELECT=text, POLYCAP_IMAGES="0")
    same_select(e_only, "the selection alone")
    # through Cython
    from polycap_amd.pyext import polycap as cy
    _, effy = _public(monkeypatch, n, binding=cy, POLYCAP_SELECT=text, POLYCAP_HIST=PUB_HIST, POLYCAP_IMAGES="0")
    same_select(effy, "cython")
    assert np.array_equal(effy.hist("exit")["bins"], h1["bins"])
    # unset: the same efficiencies, the plain tallies, and no selection
    _, effn = _public(monkeypatch, n, POLYCAP_HIST=PUB_HIST)
    assert np.array_equal(effn.data[1], F) and effn.hist("exit")["n_entries"] == n and not np.array_equal(effn.hist("exit")["bins"], h1["bins"])
    with pytest.raises(ValueError, match="POLYCAP_SELECT"):
        effn.select()
    # a malformed value fails with the reason
    from polycap_amd import capi
    for value, why in (("axis=r,range=0:1,bins=4", "item 0: unknown key"), (text + ";axis=nrefl,d=0.5,range=0:40", "cut 2: d "), ("", "at least one cut")):
        monkeypatch.setenv("POLYCAP_SELECT", value)
        with pytest.raises(ValueError, match="POLYCAP_SELECT") as e:
            capi.Source.new_from_file(DECK).get_transmission_efficiencies(1, 1000)
        assert why in str(e.value), str(e.value)
    # HDF5: the /Select group
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    import subprocess
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    path = str(tmp_path / "select.h5")
    eff_all.write_hdf5(path)
    ls = H._listing(path)
    assert ls["/Select/Cuts"] == (2, 7) and ls["/Select/Passed"] == (3, 291) and ls["/Select/Rejected"] == (3, 291) and ls["/Select/Entries"] == (3, 2)

    def read_u64(dset):
        out_ = str(tmp_path / "u.bin")
        subprocess.run([H.H5DUMP, "-d", dset, "-b", "LE", "-o", out_, path], check=True, capture_output=True)
        return np.fromfile(out_, dtype="<u8")

    assert np.array_equal(read_u64("/Select/Passed").reshape(3, 291), tot["passed_w"])
    assert np.array_equal(read_u64("/Select/Rejected").reshape(3, 291), tot["rejected_w"])
    assert read_u64("/Select/Entries").tolist() == [int(p.sum()), n, 0, 0, 0, 0]
    table = H._read(path, "/Select/Cuts", str(tmp_path)).reshape(2, 7)
    assert table[:, 0].tolist() == [2, 6] and table[:, 6].tolist() == [0, 1] and table[0, 1] == 0.5
    assert table[:, 4].tolist() == [c["range"][0] for c in cuts] and table[:, 5].tolist() == [c["range"][1] for c in cuts]
    pathn = str(tmp_path / "noselect.h5")
    effn.write_hdf5(pathn)
    assert not any(k.startswith("/Select") for k in H._listing(pathn))


def test_public_leak_run(pa, monkeypatch):
    """leak_calc through the public call, on one device and on a group: every kind equals the thin ABI's gated tallies of the same run"""
    n = 3000
    hist_text, axes = "axis=z,range=0:10,bins=50;axis=nrefl,range=0:256,bins=32", [axis("z", 0., 10., 50), axis("nrefl", 0., 256., 32)]
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=True)
        Ee, _ = leak_entries(r["ext"])
        cuts = [median_cut("nrefl", Ee, True, ze)]
        real_selection(cuts, Ee, True, ze)
        with pa.Selection(ctx, cuts) as S, pa.Histograms(ctx, axes) as h, pa.BeamMoments(ctx) as b:
            for kind in KINDS:
                tot = S.apply(kind)
                h.add(kind, select=S)
                b.add(kind, select=S)
            hist, beam = h.read(), b.read()
    assert tot["n_seen"].all() and 0 < tot["n_pass"][1] < tot["n_seen"][1]
    text = select_text(cuts)
    _, eff = _public(monkeypatch, n, leak_calc=True, POLYCAP_SELECT=text, POLYCAP_HIST=hist_text, POLYCAP_BEAM="1")
    _, effg = _public(monkeypatch, n, leak_calc=True, POLYCAP_SELECT=text, POLYCAP_HIST=hist_text, POLYCAP_BEAM="1", POLYCAP_HIP_DEVICES="0,0")
    for e in (eff, effg):
        s = e.select()
        assert s["cuts"] == cuts and all(np.array_equal(s[k], tot[k]) for k in ("n_pass", "n_seen", "passed_w", "rejected_w"))
        for kind, k in KINDS.items():
            a = e.hist(kind)
            assert a["n_entries"] == tot["n_pass"][k] and np.array_equal(a["bins"], hist["bins"][k]) and np.array_equal(a["outside"], hist["outside"][k])
            assert np.array_equal(e.beam(kind)["sums"], beam["sums"][k])

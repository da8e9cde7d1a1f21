"""Draws on the GPU (pc_hip_select_draw, Selection.draw, POLYCAP_DRAW): an unweighted sample of the entries a selection keeps.  Every
comparison takes the run's own fetched rows (records(), the planes, leaks()), quantises the weights of one energy with q(w), masks
them with the numpy form of the cuts and runs the Python-integer model of tests/draw/model.py on them: positions must be equal, rows
bit-identical (compared as uint64), and the total the model's T and passed_w of read().  For every tile and chunk size, windows, every
store of the exit photons, the leak event lists, a device group, and through the public call in both bindings."""
import ctypes as C

import numpy as np
import pytest

from tests.draw import model
from tests.test_gpu_gather import (DECK, KINDS, N_PUB, SEED, _bindings, _prob, _public, exit_entries, h5_read, leak_entries, median_cut, np_pass,
                                   real_selection, record_entries, result_records, rows_of_planes, same_rows, select_text, u64)
from tests.test_select_cpu import cut

pytestmark = pytest.mark.gpu

N1 = 5003           # 79 tiles of 64 entries, the last one of 11; 20 passes of a workgroup
FN = "pc_hip_select_draw"


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def values_of(R, p, nf, e):
    """V of the contract: q(w[e]) of the rows R where the mask p holds, 0 elsewhere"""
    V = model.quantise(R[:, nf + e])
    V[~np.asarray(p, dtype=bool)] = 0
    return V


def check(S, kind, R, p, e, N, phase, first=0, count=None, what=""):
    """one draw against the model on the rows R and the mask p; returns the drawn positions"""
    k = KINDS[kind]
    nf = 17 if k == 0 else 12
    want, T = model.draw(values_of(R, p, nf, e), N, phase, first, count)
    d = S.draw(kind, energy=e, n=N, phase=phase, first=first, count=count, positions=True)
    tag = "(%s, N %d, phase %d, window %d %s) %s" % (kind, N, phase, first, count, what)
    assert d["positions"].dtype == np.int64 and np.array_equal(d["positions"], want), tag
    same_rows(d["records"], R[want], tag)
    assert d["total"] == T == int(S.read()["passed_w"][k][e]), tag
    assert d["n"] == N and d["phase"] == phase and d["weight"] == T * 2.0 ** -32 / N
    return want


@pytest.fixture(scope="module")
def base(pa):
    """the records of one run of N1 slots in slot order, a cut on nrefl at its median, what passes it: computed once, read-only"""
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.run(SEED, 0, N1, keep_images=True)
        ctx.wait()
        R = ctx.records()
    E, _ = record_entries(R)
    c = median_cut("nrefl", E, False, ze)
    p = real_selection([c], E, False, ze)
    R.flags.writeable = False
    p.flags.writeable = False
    return dict(prob=prob, ze=ze, R=R, E=E, cut=c, p=p, n_pass=int(p.sum()))


# ---- 1: the whole sample ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 0])
def test_whole_sample(pa, base, tile):
    R, p, n_pass = base["R"], base["p"], base["n_pass"]
    rng = np.random.default_rng(1)
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.set_option("gather_tile", tile)
        ctx.run(SEED, 0, N1, keep_images=True)
        with pa.Selection(ctx, [base["cut"]]) as S:
            S.apply("exit")
            for N in (n_pass // 3, n_pass, 5 * n_pass):
                for phase in (0, 2 ** 32 - 1, int(rng.integers(1, 2 ** 32 - 1))):
                    pos = check(S, "exit", R, p, 0, N, phase, what="tile %d" % tile)
                    assert p[pos].all() and np.all(np.diff(pos) >= 0)
                    if N == 5 * n_pass:
                        assert np.bincount(pos).max() >= 5                  # duplicates: some entry is drawn five times at least
        with pa.Selection(ctx, pa.select_all()) as S:                       # every entry passes
            assert S.apply("exit")["n_pass"][0] == N1
            check(S, "exit", R, np.ones(N1, dtype=bool), 1, 3000, 12345, what="select_all, tile %d" % tile)
        d = ctx.draw(energy=1, n=3000, phase=12345, positions=True)          # the shorthand
        want, T = model.draw(values_of(R, np.ones(N1, dtype=bool), 17, 1), 3000, 12345)
        assert np.array_equal(d["positions"], want) and d["total"] == T
        same_rows(d["records"], R[want], "(TraceContext.draw)")
        a, b = ctx.draw(n=50, seed=7), ctx.draw(n=50, seed=7)               # phase None: from the seed, reproducibly
        assert a["phase"] == b["phase"] == int(np.random.default_rng(7).integers(0, 1 << 32, dtype=np.uint64))
        same_rows(a["records"], b["records"])


# ---- 2: windows and chunks -------------------------------------------------------------------------------------------------------
def test_windows_and_chunks(pa, base):
    R, p, n_pass = base["R"], base["p"], base["n_pass"]
    N, phase = 2 * n_pass + 1, 987654321
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.set_option("gather_tile", 64)
        ctx.set_option("gather_chunk_rows", 7)
        ctx.run(SEED, 0, N1, keep_images=True)
        with pa.Selection(ctx, [base["cut"]]) as S:
            S.apply("exit")
            whole = S.draw("exit", energy=0, n=N, phase=phase, positions=True)
            want, _ = model.draw(values_of(R, p, 17, 0), N, phase)
            assert np.array_equal(whole["positions"], want)
            tiles = want // 64
            seam = int(np.flatnonzero(np.diff(tiles) > 0)[10]) + 1          # the first draw of some tile: a window that begins on a tile seam
            inside = int(np.flatnonzero(np.diff(tiles) == 0)[40]) + 1       # a draw whose predecessor lies in the same tile
            assert tiles[seam] != tiles[seam - 1] and tiles[inside] == tiles[inside - 1] and seam != inside
            lo, hi = sorted((seam, inside))
            bounds = [0, 1, lo, hi, hi + 1, N - 1, N]                        # windows of length 1 at both ends and behind `hi`
            parts = [S.draw("exit", energy=0, n=N, phase=phase, first=a, count=b - a, positions=True) for a, b in zip(bounds[:-1], bounds[1:])]
            assert np.array_equal(np.concatenate([d["positions"] for d in parts]), whole["positions"])
            same_rows(np.concatenate([d["records"] for d in parts]), whole["records"], "(the windows one after the other)")
            for first, count in ((0, 0), (N, 0), (seam, 130)):
                check(S, "exit", R, p, 0, N, phase, first, count)
            ctx.set_option("gather_chunk_rows", 0)
            same_rows(S.draw("exit", energy=0, n=N, phase=phase)["records"], whole["records"], "(one chunk)")
            # the largest sample: its first and its last hundred draws
            big = 2 ** 31 - 1
            first = check(S, "exit", R, p, 0, big, phase, 0, 100)
            last = check(S, "exit", R, p, 0, big, phase, big - 100, 100)
            assert np.all(first == np.flatnonzero(values_of(R, p, 17, 0))[0]) and np.all(last == np.flatnonzero(values_of(R, p, 17, 0))[-1])


# ---- 3: edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_run_sizes(pa, base, n):
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        R = ctx.records()
        all_pass = np.ones(n, dtype=bool)
        assert np.array_equal(u64(R), u64(base["R"][:n]))                    # photons are keyed by (seed, slot)
        for tile in (64, 0):
            ctx.set_option("gather_tile", tile)
            with pa.Selection(ctx, pa.select_all()) as S:
                S.apply("exit")
                for N in (1, n, 3 * n + 1):
                    check(S, "exit", R, all_pass, 0, N, 2 ** 31, what="%d slots" % n)


def test_one_entry_no_entry_and_an_empty_tile(pa, base):
    R, E, ze = base["R"], base["E"], base["ze"]
    V = model.quantise(R[:, 17])
    x = R[:, 8]
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.set_option("gather_tile", 64)
        ctx.run(SEED, 0, N1, keep_images=True)
        # exactly one entry: the one of the largest exit x among those with weight
        i = int(np.argmax(np.where(V > 0, x, -np.inf)))
        one = cut("x", float(x[i]), float(np.nextafter(x[i], np.inf)))
        p = np_pass([one], E, False, ze)
        assert p.sum() == 1 and p[i] and V[i] > 0
        with pa.Selection(ctx, [one]) as S:
            S.apply("exit")
            pos = check(S, "exit", R, p, 0, 1000, 77)
            assert len(pos) == 1000 and np.all(pos == i)                     # a thousand copies of one row
        # no entry: the refusal, and the selection as it was
        none = cut("nrefl", 1e9, 2e9)
        assert np_pass([none], E, False, ze).sum() == 0
        with pa.Selection(ctx, [none]) as S:
            before = S.apply("exit")
            with pytest.raises(pa.HipError) as e:
                S.draw("exit", energy=0, n=10, phase=0)
            assert e.value.status == -2 and FN in str(e.value) and "no weight to draw from" in str(e.value)
            after = S.read()
            assert all(np.array_equal(after[k], before[k]) for k in after) and after["n_pass"][0] == 0
            assert S.gather().shape == (0, 19)
        # a sparse selection: whole tiles of 64 without a passing entry between tiles that have some
        lo = float(np.percentile(x, 49.5))
        hi = float(np.percentile(x, 50.5))
        sparse = cut("x", lo, hi)
        p = np_pass([sparse], E, False, ze)
        sums = np.add.reduceat(values_of(R, p, 17, 0), np.arange(0, N1, 64))
        empty = np.flatnonzero((sums[1:-1] == 0) & (sums[:-2] > 0) & (sums[2:] > 0))
        assert len(empty) >= 1 and p.sum() >= 10
        with pa.Selection(ctx, [sparse]) as S:
            S.apply("exit")
            pos = check(S, "exit", R, p, 0, 4 * int(p.sum()) + 1, 4242)
            assert not np.isin(pos // 64, empty + 1).any() and np.isin(empty, pos // 64).all() and np.isin(empty + 2, pos // 64).all()


# ---- 4: stores -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts,n", [({"plane_images": 1}, N1), ({"plane_images": 1, "compact_images": 1, "slot_ids": 1}, N1), ({"run_parts": 4}, 262149)])
def test_stores(pa, base, opts, n):
    prob, ze = base["prob"], base["ze"]
    N, phase = 4001, 31337
    with pa.TraceContext(prob, 0) as ctx:
        if n == N1:
            c, ref = base["cut"], base["R"]
        else:       # the slot-ordered store of the same seed and size, in one launch
            ctx.run(SEED, 0, n, keep_images=True)
            ctx.wait()
            ref = ctx.records()
            c = median_cut("nrefl", record_entries(ref)[0], False, ze)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_option("gather_chunk_rows", 1500)
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        store = rows_of_planes(ctx.image_planes())
        ids = ctx.slot_ids()
        p = real_selection([c], record_entries(store)[0], False, ze)
        with pa.Selection(ctx, [c]) as S:
            S.apply("exit")
            pos = check(S, "exit", store, p, 1, N, phase, what=repr(opts))    # through the store's own positions
    if "compact_images" in opts:
        assert not np.array_equal(ids, np.arange(n))                        # the order of completion is not the slot order
    else:       # slot order: the positions and rows of the records of the same run
        assert np.array_equal(ids, np.arange(n)) and np.array_equal(u64(store), u64(ref))
        pr = real_selection([c], record_entries(ref)[0], False, ze)
        want, _ = model.draw(values_of(ref, pr, 17, 1), N, phase)
        assert np.array_equal(pos, want)


# ---- 5: energies -----------------------------------------------------------------------------------------------------------------
def test_energies(pa):
    prob = _prob(pa, 12)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("gather_tile", 128)
        ctx.run(SEED, 0, 3001, keep_images=True)
        ctx.wait()
        R = ctx.records()
        E, _ = record_entries(R)
        c = median_cut("nrefl", E, False, ze)
        p = real_selection([c], E, False, ze)
        with pa.Selection(ctx, [c]) as S:
            S.apply("exit")
            got = {}
            for e in (0, 5, 11, 0, 5):                                      # the tile sums are those of one energy: back to 0 after 5
                pos = check(S, "exit", R, p, e, 2000, 5, what="energy %d" % e)
                assert e not in got or np.array_equal(got[e], pos)
                got[e] = pos
            assert not np.array_equal(got[0], got[5]) and not np.array_equal(got[5], got[11]) and not np.array_equal(got[0], got[11])
            for e in (-1, 12):
                with pytest.raises(pa.HipError) as err:
                    S.draw("exit", energy=e, n=10, phase=0)
                assert err.value.status == -2 and FN in str(err.value) and "energy" in str(err.value)


# ---- 6: leak kinds ---------------------------------------------------------------------------------------------------------------
def test_leak_kinds(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 30.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("gather_tile", 64)
        ctx.set_option("gather_chunk_rows", 100)
        r = ctx.transmission(SEED, 0, 2000, keep_images=True, leak_calc=True)
        Rx = ctx.records()
        rows = {"exit": Rx, "extleak": r["ext"], "intleak": r["int"]}
        ents = {"exit": record_entries(Rx)[0], "extleak": leak_entries(r["ext"])[0], "intleak": leak_entries(r["int"])[0]}
        for kind in KINDS:
            leak = kind != "exit"
            for name in ("nrefl", "x", "z"):                                 # the first quantity whose median splits this kind's entries
                c = median_cut(name, ents[kind], leak, ze)
                if 0.1 * len(ents[kind]) <= np_pass([c], ents[kind], leak, ze).sum() <= 0.9 * len(ents[kind]):
                    break
            p = real_selection([c], ents[kind], leak, ze)
            with pa.Selection(ctx, [c]) as S:
                S.apply(kind)
                for e in (0, 1):
                    pos = check(S, kind, rows[kind], p, e, 777, 99 + e)
                    assert S.draw(kind, energy=e, n=777, phase=99 + e)["records"].shape == (777, (12 if leak else 17) + 2)
                other = "exit" if leak else "extleak"
                with pytest.raises(pa.HipError) as err:                      # applied for this kind only
                    S.draw(other, energy=0, n=5, phase=0)
                assert err.value.status == -2 and "not applied for kind %d" % KINDS[other] in str(err.value)
        with pa.Selection(ctx, pa.select_all()) as S:                        # the all-pass cut holds for leak events too
            for kind in KINDS:
                assert S.apply(kind)["n_pass"][KINDS[kind]] == len(rows[kind])
                check(S, kind, rows[kind], np.ones(len(rows[kind]), dtype=bool), 0, 500, 1)


# ---- 7: a group ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_group(pa, base, devices):
    R, p, n_pass = base["R"], base["p"], base["n_pass"]
    with pa.TraceGroup(base["prob"], devices) as g:
        g.set_option("gather_tile", 128)
        g.set_option("gather_chunk_rows", 777)
        g.transmission(SEED, N1, keep_images=True)
        with pa.Selection(g, [base["cut"]]) as S:
            assert S.apply("exit")["n_pass"][0] == n_pass
            rows, pos = S.gather(positions=True)
            same_rows(rows, R[p], "(the group's entries are those of one device)")
            for N, phase in ((n_pass, 0), (3 * n_pass + 2, 2 ** 32 - 1)):
                want = check(S, "exit", R, p, 1, N, phase, what="group %r" % devices)      # global positions, the members one after the other
                k = int(np.searchsorted(want, N1 // len(devices)))                         # a window over the first boundary of the members
                assert 600 < k < N - 600
                check(S, "exit", R, p, 1, N, phase, k - 600, 1200, what="group %r, over a boundary" % devices)
        d = g.draw(energy=0, n=1000, phase=3, positions=True)                # the shorthand on a group
        want, T = model.draw(values_of(R, np.ones(N1, dtype=bool), 17, 0), 1000, 3)
        assert np.array_equal(d["positions"], want) and d["total"] == T
        same_rows(d["records"], R[want], "(TraceGroup.draw)")


# ---- 8: staleness and refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_selection_unchanged(pa, base):
    from polycap_amd import _cabi
    L = _cabi.lib()
    R, p, n_pass = base["R"], base["p"], base["n_pass"]
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.run(SEED, 0, N1, keep_images=True)
        with pa.Selection(ctx, [base["cut"]]) as S:
            def refused(fn, words):
                before = S.read()
                with pytest.raises(pa.HipError) as e:
                    fn()
                assert e.value.status == -2 and FN in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
                after = S.read()
                assert all(np.array_equal(after[k], before[k]) for k in after)

            refused(lambda: S.draw("exit", n=10, phase=0), ["not applied for kind 0"])
            S.apply("exit")
            rows = S.gather()
            same_rows(rows, R[p])
            check(S, "exit", R, p, 0, 100, 9)
            refused(lambda: S.draw("exit", n=0, phase=0), ["n_draw"])
            refused(lambda: S.draw("exit", n=2 ** 31, phase=0), ["n_draw"])
            refused(lambda: S.draw("exit", n=10, phase=0, first=0, count=11), ["first + count", "n_draw"])
            refused(lambda: S.draw("exit", n=10, phase=0, first=11, count=0), ["n_draw"])
            refused(lambda: S.draw("exit", n=10, phase=0, first=-1, count=1), ["first"])
            refused(lambda: S.draw("exit", n=10, phase=0, first=0, count=-1), ["count"])
            refused(lambda: S.draw("exit", energy=2, n=10, phase=0), ["energy"])
            refused(lambda: S.draw(3, n=10, phase=0), ["kind"])
            refused(lambda: S.draw("extleak", n=10, phase=0), ["not applied for kind 1"])

            def null_records():
                st = L.pc_hip_select_draw(S._h, 0, 0, 10, 0, 0, 1, None, None, None)
                if st != 0:
                    raise pa.HipError(FN, st)
            refused(null_records, ["records"])
            total = C.c_uint64(0)
            assert L.pc_hip_select_draw(S._h, 0, 0, 10, 0, 0, 0, None, None, C.byref(total)) == 0      # count 0 touches nothing but the total
            assert total.value == int(S.read()["passed_w"][0][0])
            # a gather and a draw of the same selection alternate without disturbing each other
            for _ in range(2):
                same_rows(S.gather(), rows, "(a gather after the refusals and a draw)")
                check(S, "exit", R, p, 1, 333, 21)
            # stale after the next run, of the same slots even: the wording of the gated adds
            ctx.run(SEED, 0, N1, keep_images=True)
            refused(lambda: S.draw("exit", n=10, phase=0), ["stale", "were replaced after it was applied"])
            refused(lambda: S.draw("exit", n=10, phase=0, count=0), ["stale"])
            S.apply("exit")
            check(S, "exit", R, p, 0, 100, 9, what="applied anew")
            same_rows(S.gather(), rows, "(applied anew)")
        # a new apply of another mask replaces the tile sums: the complement, at the same energy and tile
        with pa.Selection(ctx, [base["cut"]]) as S:
            S.apply("exit")
            check(S, "exit", R, p, 0, 500, 1)
        with pa.Selection(ctx, [dict(base["cut"], **{"not": True})]) as Sn:
            Sn.apply("exit")
            check(Sn, "exit", R, ~p, 0, 500, 1, what="the complement")


# ---- 9: the public call ----------------------------------------------------------------------------------------------------------
DRAW = dict(n=700, energy=3, phase=12345)
DRAW_TEXT = "n=700,energy=3,phase=12345"


def _pub(monkeypatch, binding, **env):
    monkeypatch.delenv("POLYCAP_DRAW", raising=False)
    return _public(monkeypatch, binding, **env)


@pytest.fixture(scope="module")
def pub(pa):
    """a first plain call in slot order: its own records, a cut on nrefl at their median, and the model's draws with and without it"""
    from polycap_amd import capi
    with pytest.MonkeyPatch.context() as mp:
        R = result_records(_pub(mp, capi, POLYCAP_COMPACT="0"), False)
    ze = float(pa.problem_from_inp(DECK).z[-1])
    E, _ = record_entries(R)
    c = median_cut("nrefl", E, False, ze)
    p = real_selection([c], E, False, ze)
    R.flags.writeable = False
    want = {}
    for name, mask in (("all", np.ones(len(R), dtype=bool)), ("cut", p)):
        pos, T = model.draw(values_of(R, mask, 17, DRAW["energy"]), DRAW["n"], DRAW["phase"])
        want[name] = dict(pos=pos, T=T)
    return dict(cut=c, text=select_text([c]), R=R, p=p, want=want)


def same_draw(got, R, want, what):
    assert got["n"] == DRAW["n"] and got["energy"] == DRAW["energy"] and got["phase"] == DRAW["phase"], what
    assert got["total"] == want["T"] and got["weight"] == want["T"] * 2.0 ** -32 / DRAW["n"], what
    assert got["positions"].dtype == np.int64 and np.array_equal(got["positions"], want["pos"]), what
    same_rows(got["records"], R[want["pos"]], what)


@pytest.mark.parametrize("name", ["ctypes", "cython"])
def test_public_call_draws_from_the_results_own_rows(pa, monkeypatch, pub, name):
    binding = dict(_bindings())[name]
    for which, sel in (("all", {}), ("cut", dict(POLYCAP_SELECT=pub["text"]))):
        eff = _pub(monkeypatch, binding, POLYCAP_DRAW=DRAW_TEXT, POLYCAP_COMPACT="0", **sel)
        R = result_records(eff, name == "cython")
        assert np.array_equal(u64(R), u64(pub["R"]))                        # the call's results do not depend on the variable
        same_draw(eff.draw(), R, pub["want"][which], "(%s, %s)" % (name, which))
        for kind in ("extleak", "intleak"):                                 # a plain call has exit photons only
            with pytest.raises(ValueError, match="pc_transmission_efficiencies_get_draw"):
                eff.draw(kind)
        if which == "all":                                                  # the all-pass selection is the draw's own: none is reported
            with pytest.raises(ValueError, match="POLYCAP_SELECT"):
                eff.select()
        else:
            assert eff.select()["n_pass"][0] == int(pub["p"].sum())
    plain = _pub(monkeypatch, binding, POLYCAP_COMPACT="0")
    with pytest.raises(ValueError, match="POLYCAP_DRAW"):
        plain.draw()
    eff = _pub(monkeypatch, binding, POLYCAP_DRAW="n=5", POLYCAP_COMPACT="0")      # energy and phase default to 0
    got = eff.draw()
    pos, T = model.draw(values_of(pub["R"], np.ones(N_PUB, dtype=bool), 17, 0), 5, 0)
    assert (got["n"], got["energy"], got["phase"], got["total"]) == (5, 0, 0, T) and np.array_equal(got["positions"], pos)


def test_public_call_equals_the_selections_draw(pa, monkeypatch, pub):
    """Selection.draw on a context run with the call's seed; POLYCAP_IMAGES=0, a device group, and a run too large for one slot range"""
    from polycap_amd import capi
    prob = pa.problem_from_inp(DECK)
    with pa.TraceContext(prob, 0) as ctx:
        total_b = ctx.device_memory()[1]
        ctx.run(SEED, 0, N_PUB, keep_images=True)
        for which, cuts in (("all", pa.select_all()), ("cut", [pub["cut"]])):
            with pa.Selection(ctx, cuts) as S:
                S.apply("exit")
                d = S.draw("exit", positions=True, **DRAW)
            assert np.array_equal(d["positions"], pub["want"][which]["pos"]) and d["total"] == pub["want"][which]["T"]
            same_rows(d["records"], pub["R"][d["positions"]], "(Selection.draw, %s)" % which)
    for what, env in (("POLYCAP_IMAGES=0", dict(POLYCAP_IMAGES="0")), ("POLYCAP_HIP_DEVICES=0,0", dict(POLYCAP_HIP_DEVICES="0,0")),
                      ("POLYCAP_IMAGES=0 on a group", dict(POLYCAP_IMAGES="0", POLYCAP_HIP_DEVICES="0,0"))):
        for which, sel in (("all", {}), ("cut", dict(POLYCAP_SELECT=pub["text"]))):
            eff = _pub(monkeypatch, capi, POLYCAP_DRAW=DRAW_TEXT, POLYCAP_COMPACT="0", **sel, **env)
            same_draw(eff.draw(), pub["R"], pub["want"][which], "(%s, %s)" % (what, which))
    share = (N_PUB / 4.0) * (17 + 291) * 8.0 / total_b                        # four slot ranges: no one beam to draw from
    with pytest.raises(ValueError, match="POLYCAP_DRAW") as e:
        _pub(monkeypatch, capi, POLYCAP_DRAW=DRAW_TEXT, POLYCAP_COMPACT="0", POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    assert "several slot ranges" in str(e.value)


def test_public_leak_call_carries_all_three_kinds(pa, monkeypatch):
    """at the deck's highest energy every kind has weight; at a low one a leak kind without any carries no rows and is no error"""
    from polycap_amd import capi
    n = 1000
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    specs = {"n=700,energy=290,phase=12345": dict(n=700, energy=290, phase=12345), DRAW_TEXT: DRAW}
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=True)
        ents = {"exit": exit_entries(r["images"], r["exit_weights"])[0], "extleak": leak_entries(r["ext"])[0], "intleak": leak_entries(r["int"])[0]}
        c = median_cut("nrefl", ents["extleak"], True, ze)
        real_selection([c], ents["extleak"], True, ze)
        want = {}
        for which, cuts in (("all", pa.select_all()), ("cut", [c])):
            with pa.Selection(ctx, cuts) as S:
                for kind in KINDS:
                    passed = S.apply(kind)["passed_w"][KINDS[kind]]
                    for text, d in specs.items():
                        want[text, which, kind] = (S.draw(kind, positions=True, **d) if int(passed[d["energy"]])
                                                   else dict(records=np.zeros((0, 0)), positions=np.zeros(0, dtype=np.int64), total=0))
    assert all(want["n=700,energy=290,phase=12345", "all", kind]["total"] > 0 for kind in KINDS)
    high, group, cut_text = "n=700,energy=290,phase=12345", {"POLYCAP_HIP_DEVICES": "0,0"}, dict(POLYCAP_SELECT=select_text([c]))
    for text, which, sel, env in ((high, "all", {}, {}), (high, "cut", cut_text, {}), (high, "cut", cut_text, group), (DRAW_TEXT, "all", {}, {})):
        eff = _pub(monkeypatch, capi, n=n, leak_calc=True, POLYCAP_DRAW=text, **sel, **env)
        for kind in KINDS:
            got, w = eff.draw(kind), want[text, which, kind]
            assert got["total"] == w["total"] and np.array_equal(got["positions"], w["positions"]), (text, kind, which, env)
            if w["total"]:
                same_rows(got["records"], w["records"], "(%s, %s, %s, %r)" % (text, kind, which, env))
            else:
                assert got["records"].shape == (0, 12 + 291)


def h5_attr(lib, path, group, name, ctype, mem):
    """a scalar attribute of a group read through the HDF5 library the writer bound, or None when there is none of that name"""
    h = C.CDLL(lib)
    hid = C.c_int64
    h.H5open()
    h.H5Fopen.restype, h.H5Fopen.argtypes = hid, [C.c_char_p, C.c_uint, hid]
    h.H5Aexists_by_name.restype, h.H5Aexists_by_name.argtypes = C.c_int, [hid, C.c_char_p, C.c_char_p, hid]
    h.H5Aopen_by_name.restype, h.H5Aopen_by_name.argtypes = hid, [hid, C.c_char_p, C.c_char_p, hid, hid]
    h.H5Aread.argtypes = [hid, hid, C.c_void_p]
    h.H5Aclose.argtypes = [hid]
    h.H5Fclose.argtypes = [hid]
    f = h.H5Fopen(path.encode(), 0, 0)
    assert f >= 0, path
    try:
        if h.H5Aexists_by_name(f, group.encode(), name.encode(), 0) <= 0:
            return None
        a = h.H5Aopen_by_name(f, group.encode(), name.encode(), 0, 0)
        assert a >= 0, name
        v = ctype(0)
        assert h.H5Aread(a, hid.in_dll(h, mem).value, C.byref(v)) >= 0, name
        h.H5Aclose(a)
        return v.value
    finally:
        h.H5Fclose(f)


def test_public_hdf5_group(pa, monkeypatch, pub, tmp_path):
    from polycap_amd import _cabi, capi
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    eff = _pub(monkeypatch, capi, POLYCAP_DRAW=DRAW_TEXT, POLYCAP_SELECT=pub["text"], POLYCAP_COMPACT="0")
    got = eff.draw()
    same_draw(got, pub["R"], pub["want"]["cut"], "(the call whose file is read)")
    lib = L.pc_hdf5_provider()
    if lib in (None, b"none"):
        return
    lib = lib.decode()
    path = str(tmp_path / "draw.h5")
    eff.write_hdf5(path)
    rec = h5_read(lib, path, "/Draw/Exit_Records", "float64")
    assert rec.shape == (DRAW["n"], 308) and np.array_equal(u64(rec), u64(got["records"]))
    pos = h5_read(lib, path, "/Draw/Exit_Positions", "int64")
    assert pos.shape == (DRAW["n"],) and np.array_equal(pos, got["positions"])
    for kind in ("ExtLeak", "IntLeak"):
        assert h5_read(lib, path, "/Draw/%s_Records" % kind, "float64") is None and h5_read(lib, path, "/Draw/%s_Positions" % kind, "int64") is None
        assert h5_attr(lib, path, "/Draw", kind + "_total", C.c_uint64, "H5T_NATIVE_ULLONG_g") is None
    energies = pa.problem_from_inp(DECK).energies
    assert h5_attr(lib, path, "/Draw", "n", C.c_int64, "H5T_NATIVE_LLONG_g") == DRAW["n"]
    assert h5_attr(lib, path, "/Draw", "energy_index", C.c_int64, "H5T_NATIVE_LLONG_g") == DRAW["energy"]
    assert h5_attr(lib, path, "/Draw", "energy_keV", C.c_double, "H5T_NATIVE_DOUBLE_g") == float(energies[DRAW["energy"]])
    assert h5_attr(lib, path, "/Draw", "phase", C.c_uint64, "H5T_NATIVE_ULLONG_g") == DRAW["phase"]
    assert h5_attr(lib, path, "/Draw", "Exit_total", C.c_uint64, "H5T_NATIVE_ULLONG_g") == got["total"]
    assert h5_attr(lib, path, "/Draw", "Exit_weight", C.c_double, "H5T_NATIVE_DOUBLE_g") == got["weight"]
    plain = _pub(monkeypatch, capi, POLYCAP_SELECT=pub["text"])
    pathn = str(tmp_path / "plain.h5")
    plain.write_hdf5(pathn)
    assert h5_read(lib, pathn, "/Select/Entries", "uint64") is not None
    assert h5_read(lib, pathn, "/Draw/Exit_Records", "float64") is None and h5_attr(lib, pathn, "/", "n", C.c_int64, "H5T_NATIVE_LLONG_g") is None

"""Gathers on the GPU (pc_hip_select_gather, Selection.gather, POLYCAP_SELECT_RECORDS): the rows of the entries a selection keeps,
compacted in order on the device, equal the run's own fetched rows filtered in numpy -- bit for bit, compared as uint64 -- with
their positions, for every store of the exit photons, for the leak event lists, for windows, chunks and tiles of every size, for a
device group, and through the public call in both bindings.  Every data-derived cut is the median of its quantity over the fetched
entries, and between 10 % and 90 % of the entries pass it (real_selection asserts that)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_hist import DECK, KINDS, SEED, _prob, exit_entries, leak_entries, record_entries
from tests.test_gpu_select import median_cut, real_selection, select_text
from tests.test_select_cpu import cut, np_pass

pytestmark = pytest.mark.gpu

N1 = 20037          # 314 tiles of 64 entries: more than the scan's one workgroup takes in a step; no multiple of 64


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_rows(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert np.array_equal(u64(got), u64(want)), "rows differ %s" % (what,)


def rows_of_planes(r):
    """records [n, 17 + nE] assembled from image_planes(): the planes in their order, the reflection count as int64 bits"""
    rec = np.concatenate([r["planes"].T, r["exit_weights"]], axis=1)
    rec[:, 15] = r["nrefl"].view(np.float64)
    return rec


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
    return dict(prob=prob, ze=ze, R=R, cut=c, p=p, rows=R[p], pos=np.flatnonzero(p))


# ---- 1: the whole selection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 0])
def test_whole_selection(pa, base, tile):
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.set_option("gather_tile", tile)
        ctx.run(SEED, 0, N1, keep_images=True)
        with pa.Selection(ctx, [base["cut"]]) as S:
            res = S.apply("exit")
            assert res["n_pass"][0] == len(base["pos"])
            rows, pos = S.gather(positions=True)
            same_rows(rows, base["rows"], "(tile %d)" % tile)
            assert pos.dtype == np.int64 and np.array_equal(pos, base["pos"])
            same_rows(S.gather("exit"), base["rows"], "(again, from the kept index list)")
            same_rows(rows, ctx.records()[pos], "(the context's own records at the positions)")


# ---- 2: windows and chunks -------------------------------------------------------------------------------------------------------
def test_windows_and_chunks(pa, base):
    n_pass = len(base["pos"])
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.set_option("gather_chunk_rows", 1000)
        ctx.run(SEED, 0, N1, keep_images=True)
        with pa.Selection(ctx, [base["cut"]]) as S:
            S.apply("exit")
            for first, count in ((0, 1), (n_pass - 1, 1), (63, 2), (1000, 4097), (0, 0)):
                rows, pos = S.gather("exit", first, count, positions=True)
                same_rows(rows, base["rows"][first:first + count], "(window %d, %d)" % (first, count))
                assert np.array_equal(pos, base["pos"][first:first + count])
            a, pa_ = S.gather("exit", 500, 1500, positions=True)          # ends inside a chunk; the next begins there
            b, pb = S.gather("exit", 2000, 2345, positions=True)
            same_rows(np.concatenate([a, b]), S.gather("exit", 500, 3845), "(two adjoining windows)")
            assert np.array_equal(np.concatenate([pa_, pb]), base["pos"][500:4345])
            same_rows(S.gather("exit", 1), base["rows"][1:], "(count None: everything from first on, in 11 chunks)")
            for rows_per_chunk in (1, 0):
                ctx.set_option("gather_chunk_rows", rows_per_chunk)
                same_rows(S.gather("exit", 70, 130), base["rows"][70:200], "(chunks of %d rows)" % rows_per_chunk)


# ---- 3: stores -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts,n", [({"plane_images": 1}, N1), ({"plane_images": 1, "compact_images": 1, "slot_ids": 1}, N1), ({"run_parts": 4}, 262149)])
def test_stores(pa, base, opts, n):
    prob, ze = base["prob"], base["ze"]
    with pa.TraceContext(prob, 0) as ctx:
        if n == N1:
            c, ref_rows, ref_pos = base["cut"], base["rows"], base["pos"]
        else:       # the slot-ordered store of the same seed and size, in one launch
            ctx.run(SEED, 0, n, keep_images=True)
            ctx.wait()
            R = ctx.records()
            E, _ = record_entries(R)
            c = median_cut("nrefl", E, False, ze)
            p = real_selection([c], E, False, ze)
            ref_rows, ref_pos = R[p], np.flatnonzero(p)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_option("gather_chunk_rows", 50000)
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        with pa.Selection(ctx, [c]) as S:
            S.apply("exit")
            rows, pos = S.gather(positions=True)
        store = rows_of_planes(ctx.image_planes())
        ids = ctx.slot_ids()
    E, _ = record_entries(store)
    p = real_selection([c], E, False, ze)
    assert np.array_equal(pos, np.flatnonzero(p)) and np.all(np.diff(pos) > 0)
    same_rows(rows, store[pos], "(the rows assembled from the planes at the positions, %r)" % (opts,))
    slots = ids[pos]
    if "compact_images" in opts:
        assert not np.array_equal(ids, np.arange(n))                        # the order of completion is not the slot order
    else:
        assert np.array_equal(ids, np.arange(n))
    order = np.argsort(slots, kind="stable")
    assert np.array_equal(slots[order], ref_pos)
    same_rows(rows[order], ref_rows, "(sorted by slot: the slot-ordered store's gather, %r)" % (opts,))


# ---- 4: edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, N1])
def test_edges(pa, base, n):
    with pa.TraceContext(base["prob"], 0) as ctx:
        ctx.run(SEED, 0, n, keep_images=True)
        ctx.wait()
        R = ctx.records()
        E, _ = record_entries(R)
        nr = E[:, 6]
        top = float(nr.max())
        cases = (("nothing passes", cut("nrefl", 1e9, 2e9)), ("everything passes", cut("nrefl", 0., 1e9)), ("the largest count", cut("nrefl", top, top + 1.)),
                 ("the median cut of the big run", base["cut"]))
        for what, c in cases:
            p = np_pass([c], E, False, base["ze"])
            with pa.Selection(ctx, [c]) as S:
                assert S.apply("exit")["n_pass"][0] == int(p.sum())
                rows, pos = S.gather(positions=True)
                same_rows(rows, R[p], "(%s, %d slots)" % (what, n))
                assert np.array_equal(pos, np.flatnonzero(p))
                if what == "nothing passes":
                    assert rows.shape == (0, 19) and S.gather("exit", 0, 0).shape == (0, 19)
                    with pytest.raises(pa.HipError) as e:
                        S.gather("exit", 0, 1)
                    assert e.value.status == -2 and "pc_hip_select_gather" in str(e.value) and "n_pass" in str(e.value)
                elif what == "everything passes":
                    assert len(rows) == n
                elif what == "the largest count":
                    assert 1 <= len(rows) and (n < 1000 or len(rows) < 0.1 * n)      # the few entries of the largest reflection count


# ---- 5: leak kinds ---------------------------------------------------------------------------------------------------------------
def test_leak_kinds(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("gather_tile", 64)
        r = ctx.transmission(SEED, 0, 2000, keep_images=True, leak_calc=True)
        for kind, ev in (("extleak", r["ext"]), ("intleak", r["int"])):
            E, _ = leak_entries(ev)
            c = median_cut("z", E, True, ze)
            p = real_selection([c], E, True, ze)
            with pa.Selection(ctx, [c]) as S:
                assert S.apply(kind)["n_pass"][KINDS[kind]] == int(p.sum())
                rows, pos = S.gather(kind, positions=True)
                assert rows.shape[1] == 13
                same_rows(rows, ev[p], "(%s)" % kind)
                assert np.array_equal(pos, np.flatnonzero(p))
                k = int(p.sum()) // 2
                same_rows(S.gather(kind, k), ev[p][k:], "(%s, the upper half)" % kind)
                with pytest.raises(pa.HipError) as e:                         # applied for this kind only
                    S.gather("exit", 0, 0)
                assert e.value.status == -2 and "not applied for kind 0" in str(e.value)


# ---- 6: wide rows ----------------------------------------------------------------------------------------------------------------
def test_wide_rows(pa):
    prob = _prob(pa, 70)                                                      # rows of 87 doubles: more than a wave's lanes
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("gather_chunk_rows", 999)
        ctx.run(SEED, 0, 5003, keep_images=True)
        ctx.wait()
        R = ctx.records()
        E, _ = record_entries(R)
        c = median_cut("nrefl", E, False, ze)
        p = real_selection([c], E, False, ze)
        with pa.Selection(ctx, [c]) as S:
            S.apply("exit")
            rows, pos = S.gather(positions=True)
            assert rows.shape[1] == 87
            same_rows(rows, R[p], "(70 energies)")
            assert np.array_equal(pos, np.flatnonzero(p))


# ---- 7: a group ------------------------------------------------------------------------------------------------------------------
def test_group(pa, base):
    n_pass = len(base["pos"])
    with pa.TraceGroup(base["prob"], [0, 0]) as g:
        g.set_option("gather_tile", 128)
        g.set_option("gather_chunk_rows", 777)
        g.transmission(SEED, N1, keep_images=True)
        with pa.Selection(g, [base["cut"]]) as S:
            assert S.apply("exit")["n_pass"][0] == n_pass
            rows, pos = S.gather(positions=True)
            same_rows(rows, base["rows"], "(group [0, 0])")
            assert np.array_equal(pos, base["pos"])                           # global positions
            mid = int(base["p"][:N1 // 2].sum())                              # the members' boundary is at the middle of the slots
            first, count = mid - 1500, 3000
            rows, pos = S.gather("exit", first, count, positions=True)
            assert pos[0] < N1 // 2 - 1000 and pos[-1] > N1 // 2 + 1000      # the window straddles the boundary wherever the split rounds to
            same_rows(rows, base["rows"][first:first + count], "(a window over the members' boundary)")
            assert np.array_equal(pos, base["pos"][first:first + count])
            same_rows(S.gather("exit", 0, 1), base["rows"][:1])
            same_rows(S.gather("exit", n_pass - 1, 1), base["rows"][-1:])


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_selection_unchanged(pa, base):
    from polycap_amd import _cabi
    L = _cabi.lib()
    n_pass = len(base["pos"])
    with pa.TraceContext(base["prob"], 0) as ctx:
        for name, value in (("gather_tile", 100), ("gather_tile", 32), ("gather_tile", 65536 + 64), ("gather_tile", -64), ("gather_chunk_rows", -1)):
            with pytest.raises(pa.HipError) as e:
                ctx.set_option(name, value)
            assert e.value.status == -2 and name in str(e.value), str(e.value)
        for name, value in (("gather_tile", 65536), ("gather_tile", 0), ("gather_chunk_rows", 1 << 30), ("gather_chunk_rows", 0)):
            ctx.set_option(name, value)
        ctx.run(SEED, 0, N1, keep_images=True)
        with pa.Selection(ctx, [base["cut"]]) as S:
            def refused(fn, words):
                before = S.read()
                with pytest.raises(pa.HipError) as e:
                    fn()
                assert e.value.status == -2 and "pc_hip_select_gather" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
                after = S.read()
                assert all(np.array_equal(after[k], before[k]) for k in after)

            refused(lambda: S.gather("exit", 0, 1), ["not applied for kind 0"])
            S.apply("exit")
            same_rows(S.gather(), base["rows"])
            refused(lambda: S.gather("exit", 0, n_pass + 1), ["first + count", "n_pass"])
            refused(lambda: S.gather("exit", n_pass, 1), ["first + count", "n_pass"])
            refused(lambda: S.gather("exit", n_pass + 1, 0), ["n_pass"])
            refused(lambda: S.gather("exit", -1, 1), ["first"])
            refused(lambda: S.gather("exit", 0, -1), ["count"])
            refused(lambda: S.gather(3, 0, 1), ["kind"])
            refused(lambda: S.gather(-1, 0, 1), ["kind"])
            refused(lambda: S.gather("extleak", 0, 1), ["not applied for kind 1"])

            def null_records():
                st = L.pc_hip_select_gather(S._h, 0, 0, 1, None, None)
                if st != 0:
                    raise pa.HipError("pc_hip_select_gather", st)
            refused(null_records, ["records"])
            assert L.pc_hip_select_gather(S._h, 0, 0, 0, None, None) == 0       # count 0 touches nothing
            same_rows(S.gather(), base["rows"], "(after the refusals)")
            # stale after the next run, of the same slots even
            ctx.run(SEED, 0, N1, keep_images=True)
            refused(lambda: S.gather("exit", 0, 1), ["stale"])
            refused(lambda: S.gather("exit", 0, 0), ["stale"])
            S.apply("exit")
            rows, pos = S.gather(positions=True)
            same_rows(rows, base["rows"], "(applied anew)")
            assert np.array_equal(pos, base["pos"])
            # a new apply replaces the index list: the complement
            with pa.Selection(ctx, [dict(base["cut"], **{"not": True})]) as Sn:
                Sn.apply("exit")
                same_rows(Sn.gather(), base["R"][~base["p"]], "(the complement)")


# ---- 9: the public call ----------------------------------------------------------------------------------------------------------
PUB_VARS = ("POLYCAP_SELECT", "POLYCAP_SELECT_RECORDS", "POLYCAP_JOINT", "POLYCAP_HIST", "POLYCAP_BEAM", "POLYCAP_IMAGES", "POLYCAP_SPOT_SHARE",
            "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT", "POLYCAP_STDERR", "POLYCAP_COMPACT", "POLYCAP_TALLY_STDERR")
N_PUB = 20000


def _public(monkeypatch, binding, n=N_PUB, leak_calc=False, **env):
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k in PUB_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return binding.Source.new_from_file(DECK).get_transmission_efficiencies(1, n, leak_calc=leak_calc)


def _bindings():
    from polycap_amd import capi
    from polycap_amd.pyext import polycap as cy
    return (("ctypes", capi), ("cython", cy))


def result_records(eff, cython):
    """the result's own start and exit arrays as records [n, 17 + nE], in array order"""
    if cython:
        s, x = eff._start(), eff._exit()
        start, sdir, sev, src = (np.asarray(s[k], dtype=np.float64).reshape(-1, 3) for k in (2, 3, 4, 5))
        xc, xd, xe = (np.asarray(x[k], dtype=np.float64).reshape(-1, 3) for k in (1, 2, 3))
        nr, dt, W = np.asarray(x[4], dtype=np.int64), np.asarray(x[5], dtype=np.float64), np.asarray(x[6], dtype=np.float64)
    else:
        _, _, (start, sdir, sev, src) = eff._start()
        _, (xc, xd, xe), nr, dt, W = eff._exit()
    n = len(nr)
    rec = np.empty((n, 17 + W.shape[1]))
    rec[:, 0:2], rec[:, 2:4], rec[:, 4:6], rec[:, 6:8] = src[:, :2], start[:, :2], sdir[:, :2], sev[:, :2]
    rec[:, 8:11], rec[:, 11:13], rec[:, 13:15] = xc, xd[:, :2], xe[:, :2]
    rec[:, 15] = np.ascontiguousarray(nr, dtype=np.int64).view(np.float64)
    rec[:, 16] = dt
    rec[:, 17:] = W.reshape(n, -1)
    return rec


@pytest.fixture(scope="module")
def pub_cut(pa):
    """a first plain call: the threshold of the cut on nrefl is the median of its own reflection counts"""
    from polycap_amd import capi
    with pytest.MonkeyPatch.context() as mp:
        R = result_records(_public(mp, capi, POLYCAP_COMPACT="0"), False)
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    E, _ = record_entries(R)
    c = median_cut("nrefl", E, False, ze)
    p = real_selection([c], E, False, ze)
    R.flags.writeable = False
    return dict(cut=c, text=select_text([c]), ze=ze, R=R, p=p)


@pytest.mark.parametrize("name", ["ctypes", "cython"])
def test_public_call_rows_are_the_results_own(pa, monkeypatch, pub_cut, name):
    binding = dict(_bindings())[name]
    c, ze = pub_cut["cut"], pub_cut["ze"]
    for compact in ("0", None):
        env = dict(POLYCAP_SELECT=pub_cut["text"], POLYCAP_SELECT_RECORDS="500")
        if compact is not None:
            env["POLYCAP_COMPACT"] = compact
        eff = _public(monkeypatch, binding, **env)
        R = result_records(eff, name == "cython")
        assert len(R) == N_PUB
        E, _ = record_entries(R)
        p = real_selection([c], E, False, ze)
        got = eff.select_records("exit")
        assert got["records"].shape == (500, 17 + 291) and got["positions"].dtype == np.int64
        assert np.array_equal(got["positions"], np.flatnonzero(p)[:500]), (name, compact)
        same_rows(got["records"], R[p][:500], "(%s, POLYCAP_COMPACT=%s)" % (name, compact))
        s = eff.select()
        assert s["n_pass"][0] == int(p.sum()) and s["n_seen"][0] == N_PUB
        if compact == "0":
            assert np.array_equal(u64(R), u64(pub_cut["R"]))                  # the slot order: the first call's arrays
        for kind in ("extleak", "intleak"):                                   # a plain call applies the selection to the exit photons only
            with pytest.raises(ValueError, match="pc_transmission_efficiencies_get_select_records"):
                eff.select_records(kind)
    plain = _public(monkeypatch, binding, POLYCAP_SELECT=pub_cut["text"], POLYCAP_COMPACT="0")
    with pytest.raises(ValueError, match="POLYCAP_SELECT_RECORDS"):
        plain.select_records()
    a, b = plain.select(), s
    assert all(np.array_equal(a[k], b[k]) for k in ("n_pass", "n_seen", "passed_w", "rejected_w"))      # the totals do not depend on the variable


def test_public_call_chunks_groups_and_limits(pa, monkeypatch, pub_cut):
    """POLYCAP_IMAGES=0 in at least three chunks, and a device group: rows and positions are those of the POLYCAP_COMPACT=0 call.  The
    chunks of such a run keep POLYCAP_COMPACT=0 too: positions inside a compact chunk are the order of completion, which no other call
    repeats."""
    from polycap_amd import capi
    R, p = pub_cut["R"], pub_cut["p"]
    n_pass = int(p.sum())
    with pa.TraceContext(pa.problem_from_inp(DECK, energies=[10.0]), 0) as ctx:
        total = ctx.device_memory()[1]
    share = (N_PUB / 4.0) * (17 + 291) * 8.0 / total                          # four chunks of 5000 slots
    sel = dict(POLYCAP_SELECT=pub_cut["text"], POLYCAP_COMPACT="0")
    ref = _public(monkeypatch, capi, POLYCAP_SELECT_RECORDS="500", **sel).select_records()
    same_rows(ref["records"], R[p][:500])
    several = (3 * n_pass) // 4
    assert 500 < int(p[:N_PUB // 4].sum()) < several                          # 500 rows come from the first chunk, `several` from three at least
    for limit, want in (("500", 500), (str(several), several), ("2000000000", n_pass)):
        for what, env in (("POLYCAP_IMAGES=0 in four chunks", dict(POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)),
                          ("POLYCAP_HIP_DEVICES=0,0", dict(POLYCAP_HIP_DEVICES="0,0"))):
            eff = _public(monkeypatch, capi, POLYCAP_SELECT_RECORDS=limit, **sel, **env)
            got = eff.select_records()
            assert np.array_equal(got["positions"], np.flatnonzero(p)[:want]), (what, limit)
            same_rows(got["records"], R[p][:want], "(%s, limit %s)" % (what, limit))
            s = eff.select()
            assert s["n_pass"][0] == n_pass and s["n_seen"][0] == N_PUB, (what, limit)
            if want == 500:
                assert np.array_equal(got["positions"], ref["positions"]) and np.array_equal(u64(got["records"]), u64(ref["records"]))


def test_public_leak_call_carries_all_three_kinds(pa, monkeypatch):
    from polycap_amd import capi
    n = 1000
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=True)
        ents = {"exit": exit_entries(r["images"], r["exit_weights"])[0], "extleak": leak_entries(r["ext"])[0], "intleak": leak_entries(r["int"])[0]}
        c = median_cut("nrefl", ents["extleak"], True, ze)
        real_selection([c], ents["extleak"], True, ze)
        want = {}
        with pa.Selection(ctx, [c]) as S:
            for kind in KINDS:
                S.apply(kind)
                want[kind] = S.gather(kind, positions=True)
    for env in ({}, {"POLYCAP_HIP_DEVICES": "0,0"}):
        eff = _public(monkeypatch, capi, n=n, leak_calc=True, POLYCAP_SELECT=select_text([c]), POLYCAP_SELECT_RECORDS="2000000000", **env)
        for kind in KINDS:
            got = eff.select_records(kind)
            rows, pos = want[kind]
            assert np.array_equal(np_pass([c], ents[kind], kind != "exit", ze).nonzero()[0], pos)
            same_rows(got["records"], rows, "(%s, %r)" % (kind, env))
            assert np.array_equal(got["positions"], pos), (kind, env)


def h5_read(lib, path, dset, dtype):
    """a dataset of a file as an array of its own shape through the HDF5 library the writer bound (dtype: float64, uint64 or int64, read
    without a conversion), or None when the file has no such dataset"""
    h = C.CDLL(lib)
    hid = C.c_int64
    h.H5open()
    h.H5Fopen.restype, h.H5Fopen.argtypes = hid, [C.c_char_p, C.c_uint, hid]
    h.H5Dopen2.restype, h.H5Dopen2.argtypes = hid, [hid, C.c_char_p, hid]
    h.H5Lexists.restype, h.H5Lexists.argtypes = C.c_int, [hid, C.c_char_p, hid]
    h.H5Dget_space.restype, h.H5Dget_space.argtypes = hid, [hid]
    h.H5Sget_simple_extent_ndims.argtypes = [hid]
    h.H5Sget_simple_extent_dims.argtypes = [hid, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    h.H5Dread.argtypes = [hid, hid, hid, hid, hid, C.c_void_p]
    for fn in (h.H5Sclose, h.H5Dclose, h.H5Fclose):
        fn.argtypes = [hid]
    mem = hid.in_dll(h, {"float64": "H5T_NATIVE_DOUBLE_g", "uint64": "H5T_NATIVE_ULLONG_g", "int64": "H5T_NATIVE_LLONG_g"}[dtype]).value
    f = h.H5Fopen(path.encode(), 0, 0)
    assert f >= 0, path
    try:
        if h.H5Lexists(f, dset.encode(), 0) <= 0:
            return None
        d = h.H5Dopen2(f, dset.encode(), 0)
        assert d >= 0, dset
        sp = h.H5Dget_space(d)
        rank = h.H5Sget_simple_extent_ndims(sp)
        dims = (C.c_uint64 * max(rank, 1))()
        h.H5Sget_simple_extent_dims(sp, dims, None)
        out = np.zeros(tuple(int(v) for v in dims[:rank]), dtype=dtype)
        assert h.H5Dread(d, mem, 0, 0, 0, out.ctypes.data_as(C.c_void_p)) >= 0, dset
        h.H5Sclose(sp)
        h.H5Dclose(d)
        return out
    finally:
        h.H5Fclose(f)


def test_public_hdf5_datasets(pa, monkeypatch, pub_cut, tmp_path):
    """the datasets of write_hdf5 read back equal the getter; read through the HDF5 library itself, so that the check does not depend on
    the h5dump and h5ls tools tests/test_hdf5_writer.py uses"""
    from polycap_amd import _cabi, capi
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    eff = _public(monkeypatch, capi, POLYCAP_SELECT=pub_cut["text"], POLYCAP_SELECT_RECORDS="500", POLYCAP_COMPACT="0")
    got = eff.select_records()
    same_rows(got["records"], pub_cut["R"][pub_cut["p"]][:500])
    lib = L.pc_hdf5_provider()
    if lib in (None, b"none"):
        return
    lib = lib.decode()
    path = str(tmp_path / "records.h5")
    eff.write_hdf5(path)
    rec = h5_read(lib, path, "/Select/Exit_Records", "float64")
    assert rec.shape == (500, 308) and np.array_equal(u64(rec), u64(got["records"]))
    pos = h5_read(lib, path, "/Select/Exit_Positions", "int64")
    assert pos.shape == (500,) and np.array_equal(pos, got["positions"])
    assert h5_read(lib, path, "/Select/Records_Limit", "uint64").tolist() == [500]
    assert h5_read(lib, path, "/Select/Entries", "uint64")[0].tolist() == [int(pub_cut["p"].sum()), N_PUB]
    for kind in ("ExtLeak", "IntLeak"):
        assert h5_read(lib, path, "/Select/%s_Records" % kind, "float64") is None and h5_read(lib, path, "/Select/%s_Positions" % kind, "int64") is None
    plain = _public(monkeypatch, capi, POLYCAP_SELECT=pub_cut["text"])
    pathn = str(tmp_path / "plain.h5")
    plain.write_hdf5(pathn)
    assert h5_read(lib, pathn, "/Select/Entries", "uint64") is not None
    for name in ("Exit_Records", "Exit_Positions", "Records_Limit"):
        assert h5_read(lib, pathn, "/Select/" + name, "float64") is None

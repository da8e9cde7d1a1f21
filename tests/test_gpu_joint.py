"""Joint histograms on the GPU (pc_hip_joint_*, JointHistograms, POLYCAP_JOINT): the device's uint64 sums equal numpy's exact sums
over the same run's own exit photons and leak events bit for bit, in every regime, whichever kernel traced the run and however it
was launched, split or sharded; the pair (X_AT, Y_AT) equals a spot map and a pair with an all-holding v axis a 1-D histogram.  Every
expectation is computed from the run's fetched records with the numpy restatement of the contract in tests/test_joint_cpu.py, never
from the code under test."""
import numpy as np
import pytest

from tests.test_gpu_hist import DECK, KINDS, REGIMES, SEED, _prob, exit_entries, leak_entries, record_entries
from tests.test_joint_cpu import QUANTITIES, axis, np_joint, np_value2
from tests.test_spot_cpu import np_q

pytestmark = pytest.mark.gpu

N_BINS = {"x": 33, "slope_x": 31, "start_x": 24, "start_y": 20, "r_start": 47, "nrefl": 256, "r": 19, "tan_theta": 21, "z": 12}
FOUR = (("x", "slope_x"), ("start_x", "start_y"), ("r_start", "nrefl"), ("r", "tan_theta"))


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def data_axis(name, E, W, ze, leak=False):
    """an axis whose range cuts through the run's own values (the 15th to the 80th percentile of the entries with weight, so that part
    of the weight falls outside); nrefl keeps 0:256"""
    d = {"x": 0.5, "r": 0.25}.get(name, 0.)
    centre = (0.002, -0.001) if name == "r" else (0., 0.)
    if name == "nrefl":
        return axis(name, 0., 256., N_BINS[name])
    v, ok = np_value2(QUANTITIES.index(name), E, leak, ze + d, *centre)
    v = v[ok & (W[:, 0] > 0.) & np.isfinite(v)]
    lo, hi = (float(np.percentile(v, 15)), float(np.percentile(v, 80))) if len(v) else (0., 1.)
    if not lo < hi:
        lo, hi = lo - 1., lo + 1.
    return axis(name, lo, hi, N_BINS[name], d=d, centre=centre)


def data_pairs(E, W, ze, names=FOUR, leak=False):
    return [(data_axis(u, E, W, ze, leak), data_axis(v, E, W, ze, leak)) for u, v in names]


def check(res, kind, pairs, E, W, ze, sel=None, leak=False, what=""):
    cells, out = np_joint(pairs, E, W, ze, sel, leak)
    k = KINDS[kind]
    assert res["n_entries"][k] == len(E), what
    assert np.array_equal(res["cells"][k], cells), "cells differ from numpy %s" % (what,)
    assert np.array_equal(res["outside"][k], out), "outside counters differ from numpy %s" % (what,)
    return cells, out


def real_case(pairs, cells, out):
    """by the numpy side alone: every pair has weight inside and outside, and ten or more distinct cells are occupied"""
    off = np.cumsum([0] + [u["bins"] * v["bins"] for u, v in pairs])
    for p in range(len(pairs)):
        assert cells[:, off[p]:off[p + 1]].any() and out[p].any(), "pair %d holds nothing or everything" % p
        assert (cells[:, off[p]:off[p + 1]] > 0).any(axis=0).sum() >= 10, "pair %d: fewer than ten cells are occupied" % p
    return off


# ---- exact against the records --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne,n,opts", [(1, 60000, {}), (3, 20000, {}), (12, 12000, {}), (12, 12000, {"batch_reflections": 0}),
                                      (65, 4000, {}), (291, 3000, {})])
def test_exit_joint_histograms_equal_numpy(pa, ne, n, opts):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        r = ctx.transmission(SEED, 0, n, keep_images=True)
        E, W = exit_entries(r["images"], r["exit_weights"])
        pairs = data_pairs(E, W, ze)
        total_cells = sum(u["bins"] * v["bins"] for u, v in pairs)
        got = {}
        for regime in REGIMES:
            with pa.JointHistograms(ctx, pairs, regime=regime) as h:
                assert h.regime == regime and h.total_cells == total_cells and h.n_selected == ne and h.n_pairs == 4
                h.add("exit")
                got[regime] = h.read()
        with pa.JointHistograms(ctx, pairs) as h:
            assert h.regime in REGIMES and h.pairs == pairs
            h.add("exit")
            got[0] = h.read()
            m_u, m_v = h.marginal(2, "u"), h.marginal(2, "v")
            dens = h.density(0, np.full(ne, 0.25))
    cells, out = None, None
    for regime, res in got.items():
        cells, out = check(res, "exit", pairs, E, W, ze, what="(%d energies, %s, regime %d)" % (ne, opts, regime))
        assert not res["cells"][1:].any() and not res["outside"][1:].any() and res["n_entries"].tolist() == [n, 0, 0]
    off = real_case(pairs, cells, out)
    # the identity, in Python integers
    total = [sum(int(v) for v in np_q(W[:, e])) for e in range(ne)]
    for p in range(len(pairs)):
        for e in range(0, ne, max(1, ne // 4)):
            assert sum(int(v) for v in got[0]["cells"][0, e, off[p]:off[p + 1]]) + int(got[0]["outside"][0, p, e]) == total[e]
    # the object's helpers on the same sums: marginals of (r_start, nrefl), density of (x, slope_x)
    c2 = cells[:, off[2]:off[3]].reshape(ne, 256, 47)
    assert np.array_equal(m_u, c2.sum(axis=1, dtype=np.uint64)) and np.array_equal(m_v, c2.sum(axis=2, dtype=np.uint64))
    c0 = cells[:, off[0]:off[1]].astype(np.float64)
    tot0 = np.array([float(sum(int(v) for v in cells[e, off[0]:off[1]]) + int(out[0, e])) for e in range(ne)])
    assert np.array_equal(dens.reshape(ne, -1), 0.25 * c0 / tot0[:, None])


# ---- against the spot maps and the histograms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_xy_pair_equals_a_spot_map(pa, ne):
    prob = _prob(pa, ne)
    x0, x1, y0, y1, nx, ny, d = -0.004, 0.0055, -0.003, 0.0047, 37, 29, 0.5
    with pa.TraceContext(prob, 0) as ctx:
        ctx.transmission(SEED, 0, 20000, keep_images=True)
        with pa.SpotMap(ctx, [d], (x0, x1, y0, y1), (nx, ny)) as m:
            m.add("exit")
            spot = m.read()
        assert (spot["bins"] > 0).sum() >= 10 and spot["outside"].any()
        for regime in REGIMES:
            with pa.JointHistograms(ctx, [(axis("x", x0, x1, nx, d=d), axis("y", y0, y1, ny, d=d))], regime=regime) as h:
                h.add("exit")
                res = h.read()
            assert np.array_equal(res["pairs"][0][0], spot["bins"][0]), regime
            assert np.array_equal(res["outside"][0, 0], spot["outside"][0]), regime
            assert res["n_entries"][0] == spot["n_entries"]


@pytest.mark.parametrize("ne", [1, 12])
def test_pair_with_an_all_holding_v_axis_equals_a_histogram(pa, ne):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True)
        E, W = exit_entries(r["images"], r["exit_weights"])
        for name in ("x", "r_start", "tan_theta"):
            u = data_axis(name, E, W, ze)
            with pa.Histograms(ctx, [u]) as h1:
                h1.add("exit")
                hist = h1.read()
            assert (hist["bins"][0] > 0).any(axis=0).sum() >= 10 and hist["outside"][0].any()
            for regime in REGIMES:
                with pa.JointHistograms(ctx, [(u, axis("nrefl", 0., 2.0 ** 40, 1))], regime=regime) as h:
                    h.add("exit")
                    res = h.read()
                assert np.array_equal(res["cells"], hist["bins"]) and np.array_equal(res["outside"], hist["outside"]), (name, regime)


# ---- seams ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 3])
def test_seams(pa, ne):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    sel = None if ne == 1 else [2, 0]                    # not ascending
    ext = float(prob.ext[0])
    # 1 x 1; a window that holds nothing; 16 x 256; 91 x 91 over the entrance face (8281 cells: one more tile than 8192 at a single
    # energy), placed so that the end of the first tile of 8192 cells falls into its middle rows (three outside counters precede it)
    pairs = [(axis("x", -0.05, 0.05, 1, d=0.5), axis("nrefl", 0., 256., 1)),
             (axis("x", 10., 11., 7, d=0.5), axis("slope_x", -1., 1., 5)),
             (axis("r_start", 0., ext, 16), axis("nrefl", 0., 256., 256)),
             (axis("start_x", -0.6 * ext, 0.6 * ext, 91), axis("start_y", -0.6 * ext, 0.6 * ext, 91))]
    seam = 8192 - (1 + 35 + 4096 + 3)
    with pa.TraceContext(prob, 0) as ctx:
        for regime in REGIMES:
            with pa.JointHistograms(ctx, pairs, energies=sel, regime=regime) as h:
                assert h.offsets == [0, 1, 36, 4132, 12413]
                for n in (1, 63, 64, 65, 257, 1000):
                    r = ctx.transmission(SEED + n, 0, n, keep_images=True)
                    E, W = exit_entries(r["images"], r["exit_weights"])
                    h.reset()
                    h.add("exit")
                    res = h.read()
                    cells, out = check(res, "exit", pairs, E, W, ze, sel=sel, what="(n %d, %d energies, regime %d)" % (n, ne, regime))
                    o = h.offsets
                    total = np_q(W[:, [0] if sel is None else sel]).sum(axis=0, dtype=np.uint64)
                    assert not cells[:, o[1]:o[2]].any() and np.array_equal(out[1], total)
                    assert cells[:, o[0]:o[1]].any() and cells[:, o[2]:o[3]].any()
                    if n >= 257:
                        hit = np.flatnonzero((cells[:, o[3]:o[4]] > 0).any(axis=0))      # on both sides of the first tile's end
                        assert len(hit) >= 10 and hit.min() < seam - 91 and hit.max() > seam + 91 and out[3].any()


def test_one_energy_more_than_a_chunk(pa):
    """the energies-across-lanes kernel cuts the selected energies into chunks of 512: 513 energies, and a selection that crosses it"""
    prob = _prob(pa, 513)
    ze = float(prob.z[-1])
    n = 600
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, n, keep_images=True)
        E, W = exit_entries(r["images"], r["exit_weights"])
        pairs = data_pairs(E, W, ze, (("x", "slope_x"), ("start_x", "start_y")))
        for sel in (None, list(range(512, -1, -1))):
            got = {}
            for regime in REGIMES:
                with pa.JointHistograms(ctx, pairs, energies=sel, regime=regime) as h:
                    h.add("exit")
                    got[regime] = h.read()
            for regime, res in got.items():
                cells, out = check(res, "exit", pairs, E, W, ze, sel=sel, what="(513 energies, regime %d)" % regime)
            assert cells[512].any() and cells[0].any() and out[:, 512].any() and out[:, 0].any()
            real_case(pairs, cells, out)


# ---- launch invariance ----------------------------------------------------------------------------------------------------------
def _sums_of(h, runs):
    h.reset()
    for run in runs:
        run()
        h.add("exit")
    return h.read()


@pytest.mark.parametrize("ne", [1, 3])
def test_launch_invariance(pa, ne):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    N = 196608                      # 3 launches with run_parts >= 3 (a run is cut into at most n / 65536 launches)
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True)
        pairs = data_pairs(*exit_entries(r["images"], r["exit_weights"]), ze)
        with pa.JointHistograms(ctx, pairs) as h:
            ref = _sums_of(h, [lambda: ctx.transmission(SEED, 0, N, keep_images=True)])
            assert ref["n_entries"][0] == N and ref["cells"][0].any() and ref["outside"][0].any()

            def same(res, what):
                assert res["n_entries"][0] == N, what
                assert np.array_equal(res["cells"], ref["cells"]) and np.array_equal(res["outside"], ref["outside"]), what

            ctx.set_option("run_parts", 4)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "run_parts 4")
            ctx.set_option("run_parts", 1)
            ctx.set_option("plane_images", 1)
            ctx.set_option("compact_images", 1)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "compact planes")
            ctx.set_option("compact_images", 0)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "slot-order planes")
            ctx.set_option("plane_images", 0)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N // 2, keep_images=True), lambda: ctx.run(SEED, N // 2, N - N // 2, keep_images=True)]),
                 "two runs")
        for regime in REGIMES:
            with pa.JointHistograms(ctx, pairs, regime=regime) as h2:
                same(_sums_of(h2, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "regime %d" % regime)
    with pa.TraceGroup(prob, [0, 0]) as g:
        with pa.JointHistograms(g, pairs) as h:
            g.transmission(SEED, N, keep_images=True)
            h.add("exit")
            same(h.read(), "group [0, 0]")


# ---- leak kinds -----------------------------------------------------------------------------------------------------------------
def _nrefl_axis(E, W):
    """reflection counts over the 15th to the 80th percentile of the events' own, one count per bin where the ends are whole"""
    n = E[W[:, 0] > 0., 6]
    lo, hi = float(np.percentile(n, 15)), float(np.percentile(n, 80))
    assert lo < hi
    return axis("nrefl", lo, hi, int(np.ceil(hi - lo)))


def test_leak_kinds_equal_numpy(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True, leak_calc=True)
        Ee, We = leak_entries(r["ext"])
        Ei, Wi = leak_entries(r["int"])
        Ex, Wx = exit_entries(r["images"], r["exit_weights"])
        assert len(Ee) > 100 and len(Ei) > 100
        # (z, nrefl) over the extleak events' own z and reflection counts, the same over the intleak events' own (most of those sit on
        # the exit face, far from the others, so that one range does not cut through both kinds' values; where their percentiles of z
        # coincide data_axis takes a range around them and the reflection counts alone put weight outside); a pair with start_x,
        # which no leak event has, over all of the entrance face
        ext = float(prob.ext[0])
        pairs = [(data_axis("z", Ee, We, ze, leak=True), _nrefl_axis(Ee, We)),
                 (data_axis("z", Ei, Wi, ze, leak=True), _nrefl_axis(Ei, Wi)),
                 (axis("start_x", -ext, ext, 16), axis("nrefl", 0., 256., 16))]
        got = {}
        for regime in REGIMES:
            with pa.JointHistograms(ctx, pairs, regime=regime) as h:
                for kind in ("extleak", "intleak", "exit"):
                    h.add(kind)
                got[regime] = h.read()
    off = np.cumsum([0] + [u["bins"] * v["bins"] for u, v in pairs])
    for regime, res in got.items():
        for kind, E, W, leak in (("extleak", Ee, We, True), ("intleak", Ei, Wi, True), ("exit", Ex, Wx, False)):
            cells, out = check(res, kind, pairs, E, W, ze, leak=leak, what="(%s, regime %d)" % (kind, regime))
            k = KINDS[kind]
            total = np_q(W).sum(axis=0, dtype=np.uint64)
            if leak:        # an exit-photon quantity: all the weight is outside; the kind's own pair is a real case
                assert not res["cells"][k][:, off[2]:].any() and np.array_equal(res["outside"][k][2], total)
                own = k - 1
                assert (cells[:, off[own]:off[own + 1]] > 0).any(axis=0).sum() >= 10 and out[own].all(), kind
            else:
                assert (cells[:, off[2]:off[3]] > 0).any(axis=0).sum() >= 10


# ---- relay ----------------------------------------------------------------------------------------------------------------------
def test_joint_histograms_of_a_relay(pa, oracle):
    from tests.test_gpu_relay import N as N_RELAY, SEED as SEED_RELAY, problems
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    ze = float(prob_b.z[-1])
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.run(SEED_RELAY, 0, N_RELAY, keep_images=True)
        r = ctx_a.relay(ctx_b, 1.0)
        rec = ctx_b.records()
        assert rec.shape[0] == r["n_records"] > 1000
        E, W = record_entries(rec)
        pairs = data_pairs(E, W, ze)
        for regime in REGIMES:
            with pa.JointHistograms(ctx_b, pairs, regime=regime) as h:
                h.add("exit")
                cells, out = check(h.read(), "exit", pairs, E, W, ze, what="(relay, regime %d)" % regime)
    real_case(pairs, cells, out)


# ---- misuse ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_object_unchanged(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    ze = float(prob.z[-1])
    pairs = [(axis("x", -0.01, 0.01, 16, d=0.5), axis("slope_x", -0.005, 0.005, 16))]
    with pa.TraceContext(prob, 0) as ctx:
        with pa.JointHistograms(ctx, pairs) as h:
            r = ctx.transmission(SEED, 0, 5000, keep_images=True)
            h.add("exit")
            before = h.read()
            for kind in ("extleak", "intleak"):                 # leak kinds after a plain run
                with pytest.raises(pa.HipError) as e:
                    h.add(kind)
                assert e.value.status == -2 and "pc_hip_joint_add: leak events need a leak_calc source run" in str(e.value)
            for kind in (3, -1):                                # kinds that do not exist
                with pytest.raises(pa.HipError) as e:
                    h.add(kind)
                assert e.value.status == -2 and "pc_hip_joint_add: kind must be 0 (exit photons), 1 (extleak) or 2 (intleak)" in str(e.value)
            ctx.transmission(SEED, 0, 5000, keep_images=False)
            with pytest.raises(pa.HipError) as e:
                h.add("exit")                                   # the last run kept no exit photons
            assert e.value.status == -2 and "pc_hip_joint_add: the last run kept no exit photons (run it with keep_images)" in str(e.value)
            after = h.read()
            assert after["n_entries"].tolist() == [5000, 0, 0]
            assert np.array_equal(after["cells"], before["cells"]) and np.array_equal(after["outside"], before["outside"])
            E, W = exit_entries(r["images"], r["exit_weights"])
            cells, out = check(after, "exit", pairs, E, W, ze)
            real_case(pairs, cells, out)
        with pytest.raises(pa.HipError) as e:
            pa.JointHistograms(ctx, [(pairs[0][0], axis("start_y", 0.01, -0.01, 4))])
        assert e.value.status == -2 and "pair 0: axis v: lo" in str(e.value)


# ---- the public call ------------------------------------------------------------------------------------------------------------
JOINT = "axis=x,d=0.5,range=-0.004:0.0055,bins=33*axis=slope_x,range=-0.002:0.0015,bins=31;" \
        "axis=start_x,range=-0.2:0.25,bins=24*axis=start_y,range=-0.3:0.2,bins=20;energies=200,0,90"
JOINT_PAIRS = [(axis("x", -0.004, 0.0055, 33, d=0.5), axis("slope_x", -0.002, 0.0015, 31)),
               (axis("start_x", -0.2, 0.25, 24), axis("start_y", -0.3, 0.2, 20))]
JOINT_SEL = [200, 0, 90]


def _public(monkeypatch, n, binding=None, leak_calc=False, **env):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k in ("POLYCAP_JOINT", "POLYCAP_HIST", "POLYCAP_BEAM", "POLYCAP_IMAGES", "POLYCAP_SPOT_SHARE", "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT",
              "POLYCAP_STDERR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = (binding or capi).Source.new_from_file(DECK)
    return src, src.get_transmission_efficiencies(1, n, leak_calc=leak_calc)


def test_public_api(pa, monkeypatch, tmp_path):
    n = 12000
    prob = pa.problem_from_inp(DECK)
    with pa.TraceContext(prob, 0) as ctx:
        total = ctx.device_memory()[1]
        with pa.JointHistograms(ctx, JOINT_PAIRS, energies=JOINT_SEL) as h:
            ctx.run(SEED, 0, n, keep_images=True)
            h.add("exit")
            res = h.read()
    off = real_case(JOINT_PAIRS, res["cells"][0], res["outside"][0])
    share = (n / 4.0) * (17 + 291) * 8.0 / total                    # four chunks
    _, eff = _public(monkeypatch, n, POLYCAP_JOINT=JOINT, POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    j1 = eff.joint("exit")
    E_keV, F = eff.data
    assert j1["cells"].shape == (3, 33 * 31 + 24 * 20) and j1["outside"].shape == (2, 3) and j1["n_entries"] == n
    assert j1["offsets"].tolist() == off.tolist() and np.array_equal(j1["energies"], E_keV[JOINT_SEL]) and j1["pairs"] == JOINT_PAIRS
    assert np.array_equal(j1["cells"], res["cells"][0]) and np.array_equal(j1["outside"], res["outside"][0])
    with pytest.raises(ValueError, match="kind"):
        eff.joint("extleak")

    def same(e2, what):
        j2 = e2.joint("exit")
        assert np.array_equal(j2["cells"], j1["cells"]) and np.array_equal(j2["outside"], j1["outside"]), what
        assert j2["n_entries"] == n and np.array_equal(j2["offsets"], j1["offsets"]) and j2["pairs"] == j1["pairs"], what
        assert np.array_equal(e2.data[1], F), what

    _, eff1 = _public(monkeypatch, n, POLYCAP_JOINT=JOINT)
    same(eff1, "with images, one run")
    _, effg = _public(monkeypatch, n, POLYCAP_JOINT=JOINT, POLYCAP_HIP_DEVICES="0,0")
    same(effg, "POLYCAP_HIP_DEVICES=0,0")
    # through Cython
    from polycap_amd.pyext import polycap as cy
    _, effy = _public(monkeypatch, n, binding=cy, POLYCAP_JOINT=JOINT, POLYCAP_IMAGES="0")
    jy = effy.joint("exit")
    for key in ("cells", "outside", "offsets", "energies"):
        assert np.array_equal(jy[key], j1[key]) and jy[key].dtype == j1[key].dtype, key
    assert jy["pairs"] == j1["pairs"] and jy["n_entries"] == n
    # unset: the same efficiencies, and no joint histograms
    _, effn = _public(monkeypatch, n)
    assert np.array_equal(effn.data[1], F)
    with pytest.raises(ValueError, match="POLYCAP_JOINT"):
        effn.joint("exit")
    # HDF5: the /Joint group
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    import subprocess
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    path = str(tmp_path / "joint.h5")
    eff1.write_hdf5(path)              # the run that kept its photons: a result without them has no /PC_Start and /PC_Exit to write
    ls = H._listing(path)
    tc = 33 * 31 + 24 * 20
    assert ls["/Joint/Exit/Cells"] == (3, tc) and ls["/Joint/Exit/Outside"] == (2, 3) and ls["/Joint/Exit/Pairs"] == (2, 15)
    assert ls["/Joint/Exit/Efficiency"] == (3, tc) and ls["/Joint/Exit/Efficiency_Outside"] == (2, 3) and ls["/Joint/Exit/Entries"] == (1,)
    assert not any(k.startswith("/Joint/ExtLeak") for k in ls)

    def read_u64(dset):
        out_ = str(tmp_path / "u.bin")
        subprocess.run([H.H5DUMP, "-d", dset, "-b", "LE", "-o", out_, path], check=True, capture_output=True)
        return np.fromfile(out_, dtype="<u8")

    assert np.array_equal(read_u64("/Joint/Exit/Cells").reshape(3, tc), j1["cells"])
    assert np.array_equal(read_u64("/Joint/Exit/Outside").reshape(2, 3), j1["outside"])
    assert read_u64("/Joint/Exit/Entries").tolist() == [n]
    table = H._read(path, "/Joint/Exit/Pairs", str(tmp_path)).reshape(2, 15)
    assert table[:, 0].tolist() == [0, 10] and table[:, 7].tolist() == [3, 11] and table[:, 14].tolist() == [0, 33 * 31]
    assert table[0, 1] == 0.5 and table[0, 4:7].tolist() == [-0.004, 0.0055, 33] and table[1, 11:14].tolist() == [-0.3, 0.2, 20]
    ef = H._read(path, "/Joint/Exit/Efficiency", str(tmp_path)).reshape(3, tc)
    eo = H._read(path, "/Joint/Exit/Efficiency_Outside", str(tmp_path)).reshape(2, 3)
    for p in range(2):
        for s in range(3):
            want = F[JOINT_SEL[s]]
            assert abs(ef[s, off[p]:off[p + 1]].sum() + eo[p, s] - want) <= 1e-12 * want, (p, s)
    pathn = str(tmp_path / "nojoint.h5")
    effn.write_hdf5(pathn)
    assert not any(k.startswith("/Joint") for k in H._listing(pathn))


def test_public_leak_run(pa, monkeypatch):
    """leak_calc through the public call, on one device and on a group: every kind equals a JointHistograms of the same run"""
    spec = "axis=z,range=0:10,bins=50*axis=nrefl,range=0:256,bins=32;axis=start_x,range=-0.3:0.3,bins=8*axis=nrefl,range=0:256,bins=8"
    pairs = [(axis("z", 0., 10., 50), axis("nrefl", 0., 256., 32)), (axis("start_x", -0.3, 0.3, 8), axis("nrefl", 0., 256., 8))]
    n = 3000
    _, eff = _public(monkeypatch, n, leak_calc=True, POLYCAP_JOINT=spec)
    _, effg = _public(monkeypatch, n, leak_calc=True, POLYCAP_JOINT=spec, POLYCAP_HIP_DEVICES="0,0")
    prob = pa.problem_from_inp(DECK)
    with pa.TraceContext(prob, 0) as ctx:
        ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=True)
        with pa.JointHistograms(ctx, pairs) as h:
            for kind in KINDS:
                h.add(kind)
            res = h.read()
    for kind, k in KINDS.items():
        a, g = eff.joint(kind), effg.joint(kind)
        assert a["n_entries"] > 0 and a["n_entries"] == res["n_entries"][k] == g["n_entries"], kind
        assert np.array_equal(a["cells"], res["cells"][k]) and np.array_equal(a["outside"], res["outside"][k]), kind
        assert np.array_equal(g["cells"], a["cells"]) and np.array_equal(g["outside"], a["outside"]), kind
        assert a["cells"][:, :1600].any()
        if k:
            assert not a["cells"][:, 1600:].any() and a["outside"][1].any()

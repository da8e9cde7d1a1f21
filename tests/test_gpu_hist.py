"""Histograms on the GPU (pc_hip_hist_*, Histograms, POLYCAP_HIST): the device's uint64 sums equal numpy's exact sums over the same
run's own exit photons and leak events bit for bit, in every regime, whichever kernel traced the run and however it was launched,
split or sharded.  Every expectation is computed from the run's fetched records with the numpy restatement of the contract in
tests/test_hist_cpu.py, never from the code under test."""
import os

import numpy as np
import pytest

from tests.conftest import EXAMPLE
from tests.test_hist_cpu import QUANTITIES, np_bins, np_hist, np_value, same_bits
from tests.test_spot_cpu import np_exit_dz, np_q

pytestmark = pytest.mark.gpu

DECK = os.path.join(EXAMPLE, "xos1.inp")
SEED = 5151
KINDS = {"exit": 0, "extleak": 1, "intleak": 2}
REGIMES = (1, 2)                 # workgroup-private LDS histograms, energies across lanes
N_BINS = {"x": 257, "y": 64, "r": 100, "slope_x": 33, "slope_y": 31, "tan_theta": 50, "nrefl": 256, "dtravel": 20, "r_start": 47, "z": 3}


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def _prob(pa, ne):
    return pa.problem_from_inp(DECK) if ne == 291 else pa.problem_from_inp(DECK, energies=list(np.linspace(5.0, 25.0, ne)))


# ---- entries as tests/test_hist_cpu.py lays them out: x, y, z, dx, dy, dz, n, dtravel, sx, sy -------------------------------------
def exit_entries(im, W):
    E = np.stack([im[:, 8], im[:, 9], im[:, 10], im[:, 11], im[:, 12], np_exit_dz(im[:, 11], im[:, 12]), im[:, 15], im[:, 16],
                  im[:, 2], im[:, 3]], axis=1)
    return E, W


def record_entries(rec):
    im = rec[:, :17].copy()
    im[:, 15] = rec[:, 15].copy().view(np.int64)
    return exit_entries(im, rec[:, 17:])


def leak_entries(ev):
    n = len(ev)
    E = np.stack([ev[:, 2], ev[:, 3], ev[:, 4], ev[:, 5], ev[:, 6], ev[:, 7], ev[:, 11], np.zeros(n), np.zeros(n), np.zeros(n)], axis=1)
    return E, ev[:, 12:]


def data_axes(E, W, ze, names=QUANTITIES, leak=False):
    """one axis per name whose range cuts through the run's own values (the 15th to the 80th percentile of the entries with weight,
    so that part of the weight falls outside); nrefl keeps 0:256"""
    axes = []
    live = W[:, 0] > 0.
    for name in names:
        q = QUANTITIES.index(name)
        d = {"x": 0.0, "y": 0.5, "r": 0.25}.get(name, 0.)
        centre = (0.002, -0.001) if name == "r" else (0., 0.)
        if name == "nrefl":
            lo, hi = 0., 256.
        else:
            v, ok = np_value(q, E, leak, ze + d, *centre)
            v = v[ok & live & np.isfinite(v)]
            lo, hi = (float(np.percentile(v, 15)), float(np.percentile(v, 80))) if len(v) else (0., 1.)
            if not lo < hi:
                lo, hi = lo - 1., lo + 1.
        axes.append(dict(axis=name, d=d, centre=centre, range=(lo, hi), bins=N_BINS[name]))
    return axes


def np_expect(axes, E, W, ze, sel=None, leak=False):
    """bins uint64 [S, total_bins], outside uint64 [n_axes, S]"""
    sel = np.arange(W.shape[1]) if sel is None else np.asarray(sel)
    Q = np_q(W[:, sel])
    bins, outs = [], []
    for a in axes:
        q = QUANTITIES.index(a["axis"])
        v, ok = np_value(q, E, leak, ze + a["d"], *a["centre"])
        b = np_bins(v, ok, a["range"][0], a["range"][1], a["bins"])
        H, out = np_hist(b, Q, a["bins"])
        bins.append(H)
        outs.append(out)
    return np.concatenate(bins, axis=1), np.stack(outs)


def check(res, kind, axes, E, W, ze, sel=None, leak=False, what=""):
    bins, out = np_expect(axes, E, W, ze, sel, leak)
    k = KINDS[kind]
    assert res["n_entries"][k] == len(E), what
    assert np.array_equal(res["bins"][k], bins), "bins differ from numpy %s" % (what,)
    assert np.array_equal(res["outside"][k], out), "outside counters differ from numpy %s" % (what,)
    return bins, out


# ---- exact against the records --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne,n,opts", [(1, 60000, {}), (3, 20000, {}), (12, 12000, {}), (12, 12000, {"batch_reflections": 0}),
                                      (65, 4000, {}), (291, 3000, {})])
def test_exit_histograms_equal_numpy(pa, ne, n, opts):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        r = ctx.transmission(SEED, 0, n, keep_images=True)
        E, W = exit_entries(r["images"], r["exit_weights"])
        axes = data_axes(E, W, ze)
        got = {}
        for regime in REGIMES:
            with pa.Histograms(ctx, axes, regime=regime) as h:
                assert h.regime == regime and h.total_bins == sum(N_BINS.values()) and h.n_selected == ne
                h.add("exit")
                got[regime] = h.read()
        with pa.Histograms(ctx, axes) as h:
            assert h.regime in REGIMES
            h.add("exit")
            got[0] = h.read()
    bins, out = None, None
    for regime, res in got.items():
        bins, out = check(res, "exit", axes, E, W, ze, what="(%d energies, %s, regime %d)" % (ne, opts, regime))
        assert not res["bins"][1:].any() and not res["outside"][1:].any() and res["n_entries"].tolist() == [n, 0, 0]
    # a real case, by the numpy side alone: a position axis with weight inside and outside, ten or more reflection counts
    off = np.cumsum([0] + [a["bins"] for a in axes])
    assert bins[:, off[0]:off[1]].any() and out[0].any(), "the x axis holds nothing or everything"
    assert (bins[0, off[6]:off[7]] > 0).sum() >= 10, "fewer than ten reflection counts occur"
    # the identity, in Python integers
    total = [sum(int(v) for v in np_q(W[:, e])) for e in range(ne)]
    for a in range(len(axes)):
        for e in range(0, ne, max(1, ne // 4)):
            assert sum(int(v) for v in got[0]["bins"][0, e, off[a]:off[a + 1]]) + int(got[0]["outside"][0, a, e]) == total[e]


@pytest.mark.parametrize("ne", [1, 3])
def test_seams(pa, ne):
    prob = _prob(pa, ne)
    ze = float(prob.z[-1])
    sel = None if ne == 1 else [2, 0]                    # not ascending
    # one bin; 9001 bins over the entrance radius (with the 3 others' cells more than the 8192 cells of a private tile, at one
    # energy already); a window that holds nothing; the reflection counts
    axes = [dict(axis="x", d=0.5, centre=(0., 0.), range=(-0.05, 0.05), bins=1),
            dict(axis="r_start", d=0., centre=(0., 0.), range=(0., float(prob.ext[0])), bins=9001),
            dict(axis="x", d=0.5, centre=(0., 0.), range=(10., 11.), bins=7),
            dict(axis="nrefl", d=0., centre=(0., 0.), range=(0., 256.), bins=256)]
    with pa.TraceContext(prob, 0) as ctx:
        for regime in REGIMES:
            with pa.Histograms(ctx, axes, energies=sel, regime=regime) as h:
                for n in (1, 63, 64, 65, 257, 1000):
                    r = ctx.transmission(SEED + n, 0, n, keep_images=True)
                    E, W = exit_entries(r["images"], r["exit_weights"])
                    h.reset()
                    h.add("exit")
                    res = h.read()
                    bins, out = check(res, "exit", axes, E, W, ze, sel=sel, what="(n %d, %d energies, regime %d)" % (n, ne, regime))
                    o = h.offsets
                    assert not bins[:, o[2]:o[3]].any() and np.array_equal(out[2], np_q(W[:, [0] if sel is None else sel]).sum(axis=0, dtype=np.uint64))
                    assert bins[:, o[1]:o[2]].any() and bins[:, o[3]:o[4]].any()
                    if n == 1000:
                        hit = np.flatnonzero((bins[:, o[1]:o[2]] > 0).any(axis=0))      # on both sides of the first tile's end
                        assert len(hit) > 500 and hit.min() < 4000 and hit.max() > 8400


def test_leak_kinds_equal_numpy(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    ze = float(prob.z[-1])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True, leak_calc=True)
        Ee, We = leak_entries(r["ext"])
        Ei, Wi = leak_entries(r["int"])
        Ex, Wx = exit_entries(r["images"], r["exit_weights"])
        assert len(Ee) > 100 and len(Ei) > 100
        names = ("z", "nrefl", "x", "tan_theta", "dtravel", "r_start")
        axes = data_axes(Ee, We, ze, names, leak=True)
        axes[4]["range"], axes[5]["range"] = (0., 2. * float(Ex[:, 7].max())), (0., 1.)      # every exit photon's path length and start radius
        got = {}
        for regime in REGIMES:
            with pa.Histograms(ctx, axes, regime=regime) as h:
                for kind in ("extleak", "intleak", "exit"):
                    h.add(kind)
                got[regime] = h.read()
    for regime, res in got.items():
        for kind, E, W, leak in (("extleak", Ee, We, True), ("intleak", Ei, Wi, True), ("exit", Ex, Wx, False)):
            bins, out = check(res, kind, axes, E, W, ze, leak=leak, what="(%s, regime %d)" % (kind, regime))
            off = np.cumsum([0] + [a["bins"] for a in axes])
            total = np_q(W).sum(axis=0, dtype=np.uint64)
            if leak:        # exit-photon quantities: all the weight is outside
                assert not res["bins"][KINDS[kind]][:, off[4]:].any()
                assert np.array_equal(res["outside"][KINDS[kind]][4], total) and np.array_equal(res["outside"][KINDS[kind]][5], total)
                assert bins[:, off[0]:off[1]].any() and bins[:, off[1]:off[2]].any()
            else:
                assert bins[:, off[4]:off[5]].any() and bins[:, off[5]:off[6]].any()


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
        axes = data_axes(*exit_entries(r["images"], r["exit_weights"]), ze)
        with pa.Histograms(ctx, axes) as h:
            ref = _sums_of(h, [lambda: ctx.transmission(SEED, 0, N, keep_images=True)])
            assert ref["n_entries"][0] == N and ref["bins"][0].any() and ref["outside"][0].any()

            def same(res, what):
                assert res["n_entries"][0] == N, what
                assert np.array_equal(res["bins"], ref["bins"]) and np.array_equal(res["outside"], ref["outside"]), what

            ctx.set_option("run_parts", 4)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "run_parts 4")
            ctx.set_option("run_parts", 1)
            ctx.set_option("plane_images", 1)
            ctx.set_option("compact_images", 1)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "compact planes")
            ctx.set_option("compact_images", 0)
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "slot-order planes")
            ctx.set_option("plane_images", 0)
            if ne == 1:
                for prod in (0, 1):
                    ctx.set_option("producer", prod)
                    same(_sums_of(h, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "producer %d" % prod)
                ctx.set_option("producer", -1)
            a, b = N // 3, N // 2
            same(_sums_of(h, [lambda: ctx.run(SEED, 0, a, keep_images=True), lambda: ctx.run(SEED, a, b - a, keep_images=True),
                              lambda: ctx.run(SEED, b, N - b, keep_images=True)]), "three runs")
        for regime in REGIMES:
            with pa.Histograms(ctx, axes, regime=regime) as h2:
                same(_sums_of(h2, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "regime %d" % regime)
    with pa.TraceGroup(prob, [0, 0]) as g:
        with pa.Histograms(g, axes) as h:
            g.transmission(SEED, N, keep_images=True)
            h.add("exit")
            same(h.read(), "group [0, 0]")


# ---- against the spot maps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", [1, 12])
def test_x_axis_equals_a_spot_map_of_one_row(pa, ne):
    prob = _prob(pa, ne)
    lo, hi, n, d = -0.004, 0.0055, 333, 0.5
    with pa.TraceContext(prob, 0) as ctx:
        ctx.transmission(SEED, 0, 20000, keep_images=True)
        with pa.SpotMap(ctx, [d], (lo, hi, -128., 128.), (n, 1)) as m:
            m.add("exit")
            spot = m.read()
        for regime in REGIMES:
            with pa.Histograms(ctx, [("x", (lo, hi), n, d)], regime=regime) as h:
                h.add("exit")
                res = h.read()
            assert spot["bins"].any() and spot["outside"].any()
            assert np.array_equal(res["bins"][0], spot["bins"][0, :, 0, :]), regime
            assert np.array_equal(res["outside"][0, 0], spot["outside"][0]), regime          # nothing misses +-128 cm in y


# ---- relay ----------------------------------------------------------------------------------------------------------------------
def test_histograms_of_a_relay(pa, oracle):
    from tests.test_gpu_relay import N as N_RELAY, SEED as SEED_RELAY, problems
    _, _, prob_a, _, prob_b, _ = problems(oracle, "ne12")
    ze = float(prob_b.z[-1])
    with pa.TraceContext(prob_a) as ctx_a, pa.TraceContext(prob_b) as ctx_b:
        ctx_a.run(SEED_RELAY, 0, N_RELAY, keep_images=True)
        r = ctx_a.relay(ctx_b, 1.0)
        rec = ctx_b.records()
        assert rec.shape[0] == r["n_records"] > 1000
        E, W = record_entries(rec)
        axes = data_axes(E, W, ze)
        for regime in REGIMES:
            with pa.Histograms(ctx_b, axes, regime=regime) as h:
                h.add("exit")
                bins, out = check(h.read(), "exit", axes, E, W, ze, what="(relay, regime %d)" % regime)
    assert bins.any() and out.any()


# ---- misuse ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_object_unchanged(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    ze = float(prob.z[-1])
    axes = [("x", (-0.01, 0.01), 64, 0.5), ("nrefl", (0, 256), 256)]
    with pa.TraceContext(prob, 0) as fresh:
        with pa.Histograms(fresh, axes) as h:
            with pytest.raises(pa.HipError) as e:
                h.add("exit")                           # no run yet
            assert e.value.status == -2 and "pc_hip_" in str(e.value)
            assert h.read()["n_entries"].tolist() == [0, 0, 0]
    with pa.TraceContext(prob, 0) as ctx:
        with pa.Histograms(ctx, axes) as h:
            r = ctx.transmission(SEED, 0, 5000, keep_images=True)
            h.add("exit")
            before = h.read()
            for kind in ("extleak", "intleak", 3, -1):          # leak kinds after a plain run, kinds that do not exist
                with pytest.raises(pa.HipError) as e:
                    h.add(kind)
                assert e.value.status == -2 and len(str(e.value)) > 30
            ctx.transmission(SEED, 0, 5000, keep_images=False)
            with pytest.raises(pa.HipError) as e:
                h.add("exit")                           # the last run kept no exit photons
            assert e.value.status == -2 and "keep_images" in str(e.value)
            after = h.read()
            assert after["n_entries"].tolist() == [5000, 0, 0]
            assert np.array_equal(after["bins"], before["bins"]) and np.array_equal(after["outside"], before["outside"])
            E, W = exit_entries(r["images"], r["exit_weights"])
            check(after, "exit", h.axes, E, W, ze)
        with pytest.raises(pa.HipError) as e:
            pa.Histograms(ctx, [("x", (0.01, -0.01), 64, 0.5)])
        assert e.value.status == -2 and "lo" in str(e.value)


def test_fwhm_and_quantile_of_the_focal_line(pa):
    """the object's helpers read the axis they are asked for and give what the host formulas give on the same bins"""
    prob = pa.problem_from_inp(DECK, energies=[10.0, 17.0])
    with pa.TraceContext(prob, 0) as ctx:
        ctx.transmission(SEED, 0, 60000, keep_images=True)
        with pa.Histograms(ctx, [("nrefl", (0, 256), 256), ("x", (-0.05, 0.05), 100, 0.5), dict(axis="r", d=0.5, range=(0, 0.05), bins=50)]) as h:
            h.add("exit")
            res = h.read()
            for e in (0, 1):
                assert same_bits(h.fwhm(1, e), pa.hist_fwhm(res["axes"][1][0, e], -0.05, 0.05))
                assert same_bits(h.quantile(2, e, 0.5), pa.hist_quantile(res["axes"][2][0, e], 0., 0.05, 0.5))
            assert res["axes"][2].shape == (3, 2, 50) and len(res["edges"][1]) == 101
            assert 0. < h.quantile(2, 0, 0.5) < h.quantile(2, 0, 0.9) <= 0.05


# ---- the public call ------------------------------------------------------------------------------------------------------------
HIST = "axis=x,d=0.5,range=-0.004:0.0055,bins=333;axis=r,d=0.5,centre=0.001:-0.001,range=0:0.01,bins=64;axis=nrefl,range=0:256,bins=256;" \
       "axis=dtravel,range=0:100,bins=10;energies=200,0,90"
HIST_AXES = [dict(axis="x", d=0.5, range=(-0.004, 0.0055), bins=333), dict(axis="r", d=0.5, centre=(0.001, -0.001), range=(0, 0.01), bins=64),
             dict(axis="nrefl", range=(0, 256), bins=256), dict(axis="dtravel", range=(0, 100), bins=10)]
HIST_SEL = [200, 0, 90]


def _public(monkeypatch, n, binding=None, leak_calc=False, **env):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k in ("POLYCAP_HIST", "POLYCAP_BEAM", "POLYCAP_IMAGES", "POLYCAP_SPOT_SHARE", "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT", "POLYCAP_STDERR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = (binding or capi).Source.new_from_file(DECK)
    return src, src.get_transmission_efficiencies(1, n, leak_calc=leak_calc)


def test_public_api(pa, monkeypatch, tmp_path):
    n = 12000
    src, eff = _public(monkeypatch, n, POLYCAP_HIST=HIST)
    h1 = eff.hist("exit")
    E_keV, F = eff.data
    assert h1["bins"].shape == (3, 663) and h1["outside"].shape == (4, 3) and h1["n_entries"] == n
    assert h1["offsets"].tolist() == [0, 333, 397, 653, 663] and np.array_equal(h1["energies"], E_keV[HIST_SEL])
    assert [a["axis"] for a in h1["axes"]] == ["x", "r", "nrefl", "dtravel"] and h1["axes"][1]["centre"] == (0.001, -0.001)
    assert h1["axes"][0]["range"] == (-0.004, 0.0055) and h1["axes"][0]["d"] == 0.5 and h1["axes"][2]["bins"] == 256
    # the sums are numpy's over the result's own exit data
    nx_, vecs, nr, dt, W = eff._exit()
    pos, d = vecs[0], vecs[1]
    prob = pa.problem_from_inp(DECK)
    ze = float(prob.z[-1])
    Ent = np.stack([pos[:, 0], pos[:, 1], pos[:, 2], d[:, 0], d[:, 1], np_exit_dz(d[:, 0], d[:, 1]), nr.astype(np.float64), dt,
                    np.zeros(len(dt)), np.zeros(len(dt))], axis=1)
    axes = [dict(a, d=a.get("d", 0.), centre=a.get("centre", (0., 0.))) for a in HIST_AXES]
    bins, out = np_expect(axes, Ent, W, ze, HIST_SEL)
    assert np.array_equal(h1["bins"], bins) and np.array_equal(h1["outside"], out)
    assert bins[:, :333].any() and out[0].any()
    with pytest.raises(ValueError, match="kind"):
        eff.hist("extleak")
    # a Histograms object on a context of the same problem: integer sums do not depend on launch or split
    with pa.TraceContext(prob, 0) as ctx:
        total = ctx.device_memory()[1]
        with pa.Histograms(ctx, HIST_AXES, energies=HIST_SEL) as h:
            ctx.run(SEED, 0, n // 2, keep_images=True)
            h.add("exit")
            ctx.run(SEED, n // 2, n - n // 2, keep_images=True)
            h.add("exit")
            res = h.read()
    assert np.array_equal(res["bins"][0], h1["bins"]) and np.array_equal(res["outside"][0], h1["outside"])

    def same(e2, what):
        h2 = e2.hist("exit")
        assert np.array_equal(h2["bins"], h1["bins"]) and np.array_equal(h2["outside"], h1["outside"]), what
        assert h2["n_entries"] == n and np.array_equal(h2["offsets"], h1["offsets"]) and h2["axes"] == h1["axes"], what
        assert np.array_equal(e2.data[1], F), what

    _, eff0 = _public(monkeypatch, n, POLYCAP_HIST=HIST, POLYCAP_IMAGES="0")
    same(eff0, "POLYCAP_IMAGES=0")
    share = (n / 4.0) * (17 + len(E_keV)) * 8.0 / total                    # four chunks
    _, effc = _public(monkeypatch, n, POLYCAP_HIST=HIST, POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    same(effc, "POLYCAP_IMAGES=0 in chunks")
    _, effg = _public(monkeypatch, n, POLYCAP_HIST=HIST, POLYCAP_HIP_DEVICES="0,0")
    same(effg, "POLYCAP_HIP_DEVICES=0,0")
    _, effb = _public(monkeypatch, n, POLYCAP_HIST=HIST, POLYCAP_BEAM="1", POLYCAP_STDERR="1")
    same(effb, "with POLYCAP_BEAM and POLYCAP_STDERR")
    assert effb.beam("exit")["n_entries"] == n
    # through Cython
    from polycap_amd.pyext import polycap as cy
    _, effy = _public(monkeypatch, n, binding=cy, POLYCAP_HIST=HIST)
    hy = effy.hist("exit")
    for key in ("bins", "outside", "offsets", "energies"):
        assert np.array_equal(hy[key], h1[key]) and hy[key].dtype == h1[key].dtype, key
    assert hy["axes"] == h1["axes"] and hy["n_entries"] == n
    # unset: the same efficiencies, and no histograms
    _, effn = _public(monkeypatch, n)
    assert np.array_equal(effn.data[1], F)
    with pytest.raises(ValueError, match="POLYCAP_HIST"):
        effn.hist("exit")
    # HDF5: the /Hist group
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    path = str(tmp_path / "hist.h5")
    eff.write_hdf5(path)
    ls = H._listing(path)
    assert ls["/Hist/Exit/Bins"] == (3, 663) and ls["/Hist/Exit/Outside"] == (4, 3) and ls["/Hist/Exit/Axes"] == (4, 8)
    assert ls["/Hist/Exit/Efficiency"] == (3, 663) and ls["/Hist/Exit/Efficiency_Outside"] == (4, 3) and ls["/Hist/Exit/Entries"] == (1,)
    assert not any(k.startswith("/Hist/ExtLeak") for k in ls)

    def read_u64(dset):
        out_ = str(tmp_path / "u.bin")
        import subprocess
        subprocess.run([H.H5DUMP, "-d", dset, "-b", "LE", "-o", out_, path], check=True, capture_output=True)
        return np.fromfile(out_, dtype="<u8")

    assert np.array_equal(read_u64("/Hist/Exit/Bins").reshape(3, 663), h1["bins"])
    assert np.array_equal(read_u64("/Hist/Exit/Outside").reshape(4, 3), h1["outside"])
    table = H._read(path, "/Hist/Exit/Axes", str(tmp_path)).reshape(4, 8)
    assert table[:, 0].tolist() == [0, 2, 6, 7] and table[:, 6].tolist() == [333, 64, 256, 10] and table[:, 7].tolist() == [0, 333, 397, 653]
    assert table[0, 1] == 0.5 and table[1, 2:4].tolist() == [0.001, -0.001] and table[0, 4:6].tolist() == [-0.004, 0.0055]
    ef = H._read(path, "/Hist/Exit/Efficiency", str(tmp_path)).reshape(3, 663)
    eo = H._read(path, "/Hist/Exit/Efficiency_Outside", str(tmp_path)).reshape(4, 3)
    o = h1["offsets"]
    for a in range(4):
        for s in range(3):
            want = F[HIST_SEL[s]]
            assert abs(ef[s, o[a]:o[a + 1]].sum() + eo[a, s] - want) <= 1e-12 * want, (a, s)
    pathn = str(tmp_path / "nohist.h5")
    effn.write_hdf5(pathn)
    assert not any(k.startswith("/Hist") for k in H._listing(pathn))


def test_public_leak_run(pa, monkeypatch):
    spec = "axis=z,range=0:10,bins=50;axis=nrefl,range=0:256,bins=256;axis=dtravel,range=0:100,bins=4"
    n = 3000
    _, eff = _public(monkeypatch, n, leak_calc=True, POLYCAP_HIST=spec)
    _, effg = _public(monkeypatch, n, leak_calc=True, POLYCAP_HIST=spec, POLYCAP_HIP_DEVICES="0,0")
    prob = pa.problem_from_inp(DECK)
    axes = [("z", (0, 10), 50), ("nrefl", (0, 256), 256), ("dtravel", (0, 100), 4)]
    with pa.TraceContext(prob, 0) as ctx:
        ctx.transmission(SEED, 0, n, keep_images=True, leak_calc=True)
        with pa.Histograms(ctx, axes) as h:
            for kind in KINDS:
                h.add(kind)
            res = h.read()
    for kind, k in KINDS.items():
        a, g = eff.hist(kind), effg.hist(kind)
        assert a["n_entries"] > 0 and a["n_entries"] == res["n_entries"][k] == g["n_entries"], kind
        assert np.array_equal(a["bins"], res["bins"][k]) and np.array_equal(a["outside"], res["outside"][k]), kind
        assert np.array_equal(g["bins"], a["bins"]) and np.array_equal(g["outside"], a["outside"]), kind
        assert a["bins"][:, :50].any()
        if k:
            total = a["bins"][:, :50].sum(axis=1, dtype=np.uint64) + a["outside"][0]          # all the weight of the kind
            assert not a["bins"][:, 306:].any() and a["outside"][2].any() and np.array_equal(a["outside"][2], total)

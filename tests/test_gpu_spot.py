"""Spot maps on the GPU (pc_hip_spot_*, SpotMap, POLYCAP_SPOT): the device's uint64 bins equal a numpy binning of the same entries
exactly, whichever accumulation regime made them and however the run was launched."""
import os

import numpy as np
import pytest

from tests.conftest import EXAMPLE
from tests.test_spot_cpu import np_exit_dz, np_q, np_spot_bin

pytestmark = pytest.mark.gpu

DECK = os.path.join(EXAMPLE, "xos1.inp")
SEED = 4242


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def np_map(pos, dirs, W, sel, zps, window, nx, ny):
    """numpy restatement: pos [n, 3], dirs [n, 3] (dz per entry), W [n, nE] -> bins [P, S, ny, nx], outside [P, S]"""
    Q = np_q(W[:, sel])
    P, S = len(zps), len(sel)
    bins = np.zeros((P, S, ny * nx), dtype=np.uint64)
    out = np.zeros((P, S), dtype=np.uint64)
    for p, zp in enumerate(zps):
        b = np_spot_bin(pos[:, 0], pos[:, 1], pos[:, 2], dirs[:, 0], dirs[:, 1], dirs[:, 2], zp, window, nx, ny)
        ins = b >= 0
        for s in range(S):
            np.add.at(bins[p, s], b[ins], Q[ins, s])
            out[p, s] = Q[~ins, s].sum(dtype=np.uint64)
    return bins.reshape(P, S, ny, nx), out


def exit_entries(r):
    """positions, directions (dz by the contract) and weights of the exit photons of TraceContext.transmission(keep_images)"""
    im = r["images"]
    dirs = np.stack([im[:, 11], im[:, 12], np_exit_dz(im[:, 11], im[:, 12])], axis=1)
    return im[:, 8:11], dirs, r["exit_weights"]


def cutting_window(pos, dirs, zp):
    """a window through the middle of the spot on plane zp: part of it falls outside"""
    t = (zp - pos[:, 2]) / dirs[:, 2]
    xd, yd = pos[:, 0] + dirs[:, 0] * t, pos[:, 1] + dirs[:, 1] * t
    ok = np.isfinite(xd) & np.isfinite(yd)
    return (float(np.percentile(xd[ok], 15)), float(np.percentile(xd[ok], 80)),
            float(np.percentile(yd[ok], 25)), float(np.percentile(yd[ok], 90)))


def check_map(m, res, pos, dirs, W, zps):
    sel = np.arange(W.shape[1]) if m.energies is None else m.energies
    bins, out = np_map(pos, dirs, W, sel, zps, m.window, m.nx, m.ny)
    assert np.array_equal(res["bins"], bins), "bins differ from numpy (wide=%s)" % m.wide
    assert np.array_equal(res["outside"], out), "outside counters differ from numpy (wide=%s)" % m.wide
    total = np_q(W[:, sel]).sum(axis=0, dtype=np.uint64)
    for p in range(len(zps)):
        assert np.array_equal(res["bins"][p].reshape(len(sel), -1).sum(axis=1, dtype=np.uint64) + res["outside"][p], total)


@pytest.fixture(scope="module")
def one_energy(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    ctx = pa.TraceContext(prob, 0)
    r = ctx.transmission(SEED, 0, 100000, keep_images=True)
    yield pa, prob, ctx, r
    ctx.close()


@pytest.mark.parametrize("regime", [0, 1, 2])
def test_exit_map_equals_numpy(one_energy, regime):
    pa, prob, ctx, r = one_energy
    pos, dirs, W = exit_entries(r)
    dist = np.array([0.0, 0.35, 1.2])
    zps = prob.z[-1] + dist
    win = cutting_window(pos, dirs, zps[1])
    with pa.SpotMap(ctx, dist, win, (48, 32), regime=regime) as m:
        m.add("exit")
        res = m.read()
        assert res["n_entries"] == 100000 and res["bins"].shape == (3, 1, 32, 48)
        assert (res["outside"] > 0).all() and (res["bins"] > 0).sum() > 100
        check_map(m, res, pos, dirs, W, zps)
        q_total = float(np_q(W).sum()) * 2.0 ** -32
        assert abs(q_total - r["sum_weights"][0]) <= r["i_exit"] * 2.0 ** -33
    # 512 x 512: 32 LDS tiles, i.e. 32 passes over the entries in the LDS regime
    with pa.SpotMap(ctx, dist[1:2], win, (512, 512), regime=regime) as m:
        m.add(0)
        res = m.read()
        assert m.wide == (regime != 1)
        check_map(m, res, pos, dirs, W, zps[1:2])


@pytest.mark.parametrize("sel", [[0, 11, 23], None])
@pytest.mark.parametrize("regime", [0, 1, 2])
def test_many_energies_both_regimes(pa, sel, regime):
    prob = pa.problem_from_inp(DECK, energies=np.linspace(5.0, 28.0, 24))
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 40000, keep_images=True)
        pos, dirs, W = exit_entries(r)
        dist = np.array([0.5, 2.0])
        zps = prob.z[-1] + dist
        win = cutting_window(pos, dirs, zps[0])
        with pa.SpotMap(ctx, dist, win, (20, 24), energies=sel, regime=regime) as m:
            assert m.wide == (regime != 1)
            m.add("exit")
            res = m.read()
            check_map(m, res, pos, dirs, W, zps)


def _map_of(m, runs):
    m.reset()
    for run in runs:
        run()
        m.add("exit")
    return m.read()


def test_launch_invariance(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    N = 196608                      # 3 launches with run_parts >= 3 (a run is cut into at most n / 65536 launches)
    dist, win = [0.3, 1.0], (-0.015, 0.01, -0.012, 0.013)
    with pa.TraceContext(prob, 0) as ctx:
        with pa.SpotMap(ctx, dist, win, (64, 40)) as m:
            ref = _map_of(m, [lambda: ctx.transmission(SEED, 0, N, keep_images=True)])
            assert ref["n_entries"] == N and (ref["bins"] > 0).sum() > 200 and (ref["outside"] > 0).all()

            def same(res, what):
                assert res["n_entries"] == N, what
                assert np.array_equal(res["bins"], ref["bins"]) and np.array_equal(res["outside"], ref["outside"]), what

            ctx.set_option("run_parts", 4)
            same(_map_of(m, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "run_parts")
            ctx.set_option("run_parts", 1)
            ctx.set_option("plane_images", 1)
            ctx.set_option("compact_images", 1)
            same(_map_of(m, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "compact planes")
            ctx.set_option("compact_images", 0)
            same(_map_of(m, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "slot-order planes")
            ctx.set_option("plane_images", 0)
            for prod in (0, 1):
                ctx.set_option("producer", prod)
                same(_map_of(m, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "producer %d" % prod)
            ctx.set_option("producer", -1)
            same(_map_of(m, [lambda: ctx.run(SEED, 0, N // 2, keep_images=True),
                             lambda: ctx.run(SEED, N // 2, N - N // 2, keep_images=True)]), "two runs")
    with pa.TraceGroup(prob, [0, 0]) as g:
        with pa.SpotMap(g, dist, win, (64, 40)) as m:
            g.transmission(SEED, N, keep_images=True)
            m.add("exit")
            same(m.read(), "group [0, 0]")


def test_leak_maps_equal_numpy(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True, leak_calc=True)
        dist = np.array([0.0, 1.0])
        zps = prob.z[-1] + dist
        for kind, ev in (("extleak", r["ext"]), ("intleak", r["int"])):
            assert len(ev) > 100, kind
            pos, dirs, W = ev[:, 2:5], ev[:, 5:8], ev[:, 12:]
            win = cutting_window(pos, dirs, zps[1])
            for regime in (1, 2):
                with pa.SpotMap(ctx, dist, win, (30, 30), regime=regime) as m:
                    m.add(kind)
                    res = m.read()
                    assert res["n_entries"] == len(ev)
                    check_map(m, res, pos, dirs, W, zps)


def test_errors(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    with pa.TraceContext(prob, 0) as ctx:
        with pa.SpotMap(ctx, [1.0], (-0.01, 0.01, -0.01, 0.01), (8, 8)) as m:
            ctx.transmission(SEED, 0, 5000, keep_images=False)
            with pytest.raises(pa.HipError) as e:
                m.add("exit")
            assert e.value.status == -2
            ctx.transmission(SEED, 0, 5000, keep_images=True)
            for kind in ("extleak", "intleak"):
                with pytest.raises(pa.HipError) as e:
                    m.add(kind)
                assert e.value.status == -2
            m.add("exit")
            assert m.read()["n_entries"] == 5000


def _public(monkeypatch, n, **env):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    src = capi.Source.new_from_file(DECK)
    return src, src.get_transmission_efficiencies(1, n)


def test_public_api(pa, monkeypatch, tmp_path):
    spec = "dist=0.2,1.5;window=-0.02,0.015,-0.018,0.02;bins=24x16;energies=0,90,200"
    n = 60000
    src, eff = _public(monkeypatch, n, POLYCAP_SPOT=spec, POLYCAP_IMAGES="1")
    s1 = eff.spot_map("exit")
    E, F = eff.data
    assert s1["maps"].shape == (2, 3, 16, 24) and np.array_equal(s1["distances"], [0.2, 1.5])
    assert np.array_equal(s1["energies"], E[[0, 90, 200]]) and s1["window"] == (-0.02, 0.015, -0.018, 0.02)
    # the map is numpy's binning of the result's own exit data, in efficiency units
    nx_, vecs, nr, dt, W = eff._exit()
    pos, d = vecs[0], vecs[1]
    dirs = np.stack([d[:, 0], d[:, 1], np_exit_dz(d[:, 0], d[:, 1])], axis=1)
    sel = np.array([0, 90, 200])
    zps = pa.problem_from_inp(DECK, energies=[10.0]).z[-1] + np.array([0.2, 1.5])
    bins, out = np_map(pos, dirs, W, sel, zps, (-0.02, 0.015, -0.018, 0.02), 24, 16)
    tot = bins.reshape(2, 3, -1).sum(axis=2, dtype=np.uint64) + out
    want = F[sel][None, :, None, None] * bins.astype(np.float64) / tot.astype(np.float64)[:, :, None, None]
    assert np.array_equal(s1["maps"], want)
    # maps plus outside sum to the efficiency
    sums = s1["maps"].sum(axis=(2, 3)) + s1["outside"]
    assert np.allclose(sums, F[sel][None, :], rtol=1e-12, atol=0)
    # POLYCAP_IMAGES=0: the same map, bit for bit, with nothing copied back
    _, eff0 = _public(monkeypatch, n, POLYCAP_SPOT=spec, POLYCAP_IMAGES="0")
    s0 = eff0.spot_map("exit")
    assert np.array_equal(s0["maps"], s1["maps"]) and np.array_equal(s0["outside"], s1["outside"])
    assert np.array_equal(eff0.data[1], F)
    # the chunked path (a small share of device memory): bit-equal to the unchunked run
    with pa.TraceContext(pa.problem_from_inp(DECK, energies=[10.0]), 0) as ctx:
        total = ctx.device_memory()[1]
    share = (n / 4.0) * (17 + len(E)) * 8.0 / total
    _, effc = _public(monkeypatch, n, POLYCAP_SPOT=spec, POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    sc = effc.spot_map("exit")
    assert np.array_equal(sc["maps"], s1["maps"]) and np.array_equal(sc["outside"], s1["outside"])
    assert np.array_equal(effc.data[1], F)
    # HDF5: the /Spot group
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    path = str(tmp_path / "spot.h5")
    eff.write_hdf5(path)
    ls = H._listing(path)
    assert ls["/Spot/Exit"] == (2, 3, 16, 24) and ls["/Spot/Exit_Outside"] == (2, 3)
    assert ls["/Spot/Distances"] == (2,) and ls["/Spot/Window"] == (4,) and ls["/Spot/Energies"] == (3,)
    units = H._units(path)
    assert units["/Spot/Exit"] == "a.u." and units["/Spot/Distances"] == "cm" and units["/Spot/Energies"] == "keV"
    got = H._read(path, "/Spot/Exit", str(tmp_path)).reshape(2, 3, 16, 24)
    assert np.array_equal(got, s1["maps"])

"""Exit-beam moments on the GPU (pc_hip_beam_*, BeamMoments, POLYCAP_BEAM): the device's 128-bit sums equal exact integer sums over
the same run's own exit photons and leak events bit for bit, whichever kernel traced the run and however it was launched, split or
sharded; and the derived parameters describe the beam the images show."""
import os

import numpy as np
import pytest

from tests.conftest import EXAMPLE
from tests.test_beam_cpu import PAIRS, py_params, same_bits, to_lohi
from tests.test_spot_cpu import np_exit_dz, np_q

pytestmark = pytest.mark.gpu

DECK = os.path.join(EXAMPLE, "xos1.inp")
SEED = 4343
KINDS = {"exit": 0, "extleak": 1, "intleak": 2}


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


# ---- exact sums in numpy: the contract on arrays, products split into limbs that int64 matrix products add exactly ------------
def np_quantise(pos, dirs, ze):
    """X, Y, U, V int64 [n, 4] and the in-range mask"""
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


def exact_sums(pos, dirs, W, ze, sel=None):
    """(lo, hi) sums uint64 [len(sel), 15, 2], outside uint64 [len(sel)] from entries and weights W [n, nE] (floats)"""
    sel = np.arange(W.shape[1]) if sel is None else np.asarray(sel)
    q, ok = np_quantise(pos, dirs, ze)
    Q = np_q(W[:, sel])                                             # uint64 [n, S]
    out = Q[~ok].sum(axis=0, dtype=np.uint64)
    Q, q = Q[ok].astype(np.int64), q[ok]
    P = np.empty((len(q), 15), dtype=np.int64)
    P[:, 0] = 1
    P[:, 1:5] = q
    for k, (a, b) in enumerate(PAIRS):
        P[:, 5 + k] = q[:, a] * q[:, b]
    # W = sum w_j 2^(11 j) (3 limbs < 2^11), P = sum p_l 2^(21 l) (p_0, p_1 in [0, 2^21), p_2 signed): partial products < 2^32
    wl = [(Q >> (11 * j)) & 0x7ff for j in range(3)]
    pl = [P & 0x1fffff, (P >> 21) & 0x1fffff, P >> 42]
    S = np.zeros((len(sel), 15), dtype=object)
    for j in range(3):
        for l in range(3):
            m = (wl[j].T @ pl[l]).astype(object)                      # [S, 15], exact in int64 (n < 2^30)
            S += m * (1 << (11 * j + 21 * l))
    lohi = np.stack([to_lohi([int(v) for v in S[e]]) for e in range(len(sel))])
    return lohi, out, [[int(v) for v in S[e]] for e in range(len(sel))]


def exit_entries(r):
    im = r["images"]
    dirs = np.stack([im[:, 11], im[:, 12], np_exit_dz(im[:, 11], im[:, 12])], axis=1)
    return im[:, 8:11], dirs, r["exit_weights"]


def _prob(pa, ne):
    return pa.problem_from_inp(DECK) if ne == 291 else pa.problem_from_inp(DECK, energies=list(np.linspace(5.0, 25.0, ne)))


# ---- exact against the images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne,n,opts", [(1, 60000, {}), (4, 20000, {}), (8, 20000, {}), (12, 12000, {}),
                                      (12, 12000, {"batch_reflections": 0}), (291, 3000, {})])
def test_exit_sums_equal_exact(pa, ne, n, opts):
    prob = _prob(pa, ne)
    with pa.TraceContext(prob, 0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        r = ctx.transmission(SEED, 0, n, keep_images=True)
        with pa.BeamMoments(ctx) as b:
            b.add("exit")
            res = b.read()
    assert res["n_entries"].tolist() == [n, 0, 0]
    pos, dirs, W = exit_entries(r)
    lohi, out, S = exact_sums(pos, dirs, W, prob.z[-1])
    assert np.array_equal(res["sums"][0], lohi), "sums differ from the exact ones (%d energies, %s)" % (ne, opts)
    assert np.array_equal(res["outside"][0], out)
    assert not res["sums"][1:].any() and not res["outside"][1:].any()
    rows = pa.beam_params(res["sums"][0])
    cols = pa.hip.beam_columns()
    for e in range(ne):
        assert same_bits([rows[c][e] for c in cols], py_params(S[e]))


def test_leak_sums_equal_exact(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0, 20.0])
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, 20000, keep_images=True, leak_calc=True)
        with pa.BeamMoments(ctx) as b:
            for kind in ("extleak", "intleak", "exit"):
                b.add(kind)
            res = b.read()
    for kind, ev in (("extleak", r["ext"]), ("intleak", r["int"])):
        assert len(ev) > 100, kind
        k = KINDS[kind]
        lohi, out, _ = exact_sums(ev[:, 2:5], ev[:, 5:8], ev[:, 12:], prob.z[-1])
        assert res["n_entries"][k] == len(ev)
        assert np.array_equal(res["sums"][k], lohi), kind
        assert np.array_equal(res["outside"][k], out), kind
    lohi, out, _ = exact_sums(*exit_entries(r), prob.z[-1])
    assert np.array_equal(res["sums"][0], lohi) and np.array_equal(res["outside"][0], out)


# ---- launch invariance ----------------------------------------------------------------------------------------------------------
def _sums_of(b, runs):
    b.reset()
    for run in runs:
        run()
        b.add("exit")
    return b.read()


@pytest.mark.parametrize("ne", [1, 4])
def test_launch_invariance(pa, ne):
    prob = _prob(pa, ne)
    N = 196608                      # 3 launches with run_parts >= 3 (a run is cut into at most n / 65536 launches)
    with pa.TraceContext(prob, 0) as ctx:
        with pa.BeamMoments(ctx) as b:
            ref = _sums_of(b, [lambda: ctx.transmission(SEED, 0, N, keep_images=True)])
            assert ref["n_entries"][0] == N and ref["sums"][0, :, 0].any()

            def same(res, what):
                assert res["n_entries"][0] == N, what
                assert np.array_equal(res["sums"], ref["sums"]) and np.array_equal(res["outside"], ref["outside"]), what

            ctx.set_option("run_parts", 4)
            same(_sums_of(b, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "run_parts 4")
            ctx.set_option("run_parts", 1)
            ctx.set_option("plane_images", 1)
            ctx.set_option("compact_images", 1)
            same(_sums_of(b, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "compact planes")
            ctx.set_option("compact_images", 0)
            same(_sums_of(b, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "slot-order planes")
            ctx.set_option("plane_images", 0)
            if ne == 1:
                for prod in (0, 1):
                    ctx.set_option("producer", prod)
                    same(_sums_of(b, [lambda: ctx.run(SEED, 0, N, keep_images=True)]), "producer %d" % prod)
                ctx.set_option("producer", -1)
            same(_sums_of(b, [lambda: ctx.run(SEED, 0, N // 3, keep_images=True),
                              lambda: ctx.run(SEED, N // 3, N - N // 3, keep_images=True)]), "two runs")
    with pa.TraceGroup(prob, [0, 0]) as g:
        with pa.BeamMoments(g) as b:
            g.transmission(SEED, N, keep_images=True)
            b.add("exit")
            same(b.read(), "group [0, 0]")


def test_errors(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    with pa.TraceContext(prob, 0) as ctx:
        with pa.BeamMoments(ctx) as b:
            ctx.transmission(SEED, 0, 5000, keep_images=False)
            with pytest.raises(pa.HipError) as e:
                b.add("exit")
            assert e.value.status == -2
            ctx.transmission(SEED, 0, 5000, keep_images=True)
            for kind in ("extleak", "intleak", 3, -1):
                with pytest.raises(pa.HipError) as e:
                    b.add(kind)
                assert e.value.status == -2
            b.add("exit")
            assert b.read()["n_entries"].tolist() == [5000, 0, 0]


# ---- physics sanity -------------------------------------------------------------------------------------------------------------
def test_centroid_size_and_waist_match_the_images(pa):
    """Centroid and RMS size at five distances from the parameters against numpy over the images, and the round waist against the
    argmin of a ladder of planes.  Positions and slopes are quantised to 2^-24 (cm, rad) and weights to 2^-32: the differences
    allowed here are a few quanta over the square root of the photon count."""
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    n = 100000
    with pa.TraceContext(prob, 0) as ctx:
        r = ctx.transmission(SEED, 0, n, keep_images=True)
        with pa.BeamMoments(ctx) as b:
            b.add("exit")
            p = b.params(distances=[0.0, 0.3, 1.0, 2.5, 5.0])
    pos, dirs, W = exit_entries(r)
    w = W[:, 0]
    ze = prob.z[-1]
    t = (ze - pos[:, 2]) / dirs[:, 2]
    x0, y0 = pos[:, 0] + dirs[:, 0] * t, pos[:, 1] + dirs[:, 1] * t
    ux, uy = dirs[:, 0] / dirs[:, 2], dirs[:, 1] / dirs[:, 2]
    assert abs(p["weight"][0] / w.sum() - 1) < 1e-9

    def at(d):
        x, y = x0 + d * ux, y0 + d * uy
        mx, my = np.average(x, weights=w), np.average(y, weights=w)
        sx, sy = np.sqrt(np.average((x - mx) ** 2, weights=w)), np.sqrt(np.average((y - my) ** 2, weights=w))
        return mx, my, sx, sy, np.hypot(sx, sy)

    for k, d in enumerate(p["distances"]):
        mx, my, sx, sy, sr = at(d)
        tol = 1e-6 * sr
        assert abs(p["at_x"][0, k] - mx) < tol and abs(p["at_y"][0, k] - my) < tol, d
        for name, v in (("size_x", sx), ("size_y", sy), ("size_r", sr)):
            assert abs(p["at_" + name][0, k] / v - 1) < 1e-6, (d, name)
    d_star = p["waist_r"][0]
    assert np.isfinite(d_star)
    step = 0.002
    ladder = np.arange(max(0.0, d_star - 1.0), d_star + 1.0, step)
    rr = np.array([at(d)[4] for d in ladder])
    assert abs(ladder[np.argmin(rr)] - d_star) <= step
    # the waist size is numpy's RMS radius on the plane at d*_r itself (the ladder's minimum lies up to half a step away)
    assert abs(at(d_star)[4] / p["size_waist_r"][0] - 1) < 1e-6


# ---- the public call ------------------------------------------------------------------------------------------------------------
def _public(monkeypatch, n, **env):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    for k in ("POLYCAP_BEAM", "POLYCAP_IMAGES", "POLYCAP_SPOT_SHARE", "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT", "POLYCAP_STDERR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = capi.Source.new_from_file(DECK)
    return src, src.get_transmission_efficiencies(1, n)


def test_public_api(pa, monkeypatch, tmp_path):
    n = 12000
    src, eff = _public(monkeypatch, n, POLYCAP_BEAM="1")
    b1 = eff.beam("exit")
    E, F = eff.data
    assert b1["sums"].shape == (len(E), 15, 2) and b1["n_entries"] == n
    # the sums are the exact sums of the result's own exit data (a few energies: the exact sums are slow in Python)
    nx_, vecs, nr, dt, W = eff._exit()
    pos, d = vecs[0], vecs[1]
    dirs = np.stack([d[:, 0], d[:, 1], np_exit_dz(d[:, 0], d[:, 1])], axis=1)
    sel = [0, 90, 200, len(E) - 1]
    ze = pa.problem_from_inp(DECK, energies=[10.0]).z[-1]
    lohi, out, S = exact_sums(pos, dirs, W, ze, sel)
    assert np.array_equal(b1["sums"][sel], lohi) and np.array_equal(b1["outside"][sel], out)
    for j, e in enumerate(sel):
        assert same_bits([b1[c][e] for c in pa.hip.beam_columns()], py_params(S[j]))
    with pytest.raises(ValueError, match="kind"):
        eff.beam("extleak")

    def same(e2, what):
        b2 = e2.beam("exit")
        assert np.array_equal(b2["sums"], b1["sums"]) and np.array_equal(b2["outside"], b1["outside"]), what
        assert b2["n_entries"] == n, what
        for c in pa.hip.beam_columns():
            assert same_bits(b2[c], b1[c]), (what, c)
        assert np.array_equal(e2.data[1], F), what

    _, eff0 = _public(monkeypatch, n, POLYCAP_BEAM="1", POLYCAP_IMAGES="0")
    same(eff0, "POLYCAP_IMAGES=0")
    with pa.TraceContext(pa.problem_from_inp(DECK, energies=[10.0]), 0) as ctx:
        total = ctx.device_memory()[1]
    share = (n / 4.0) * (17 + len(E)) * 8.0 / total
    _, effc = _public(monkeypatch, n, POLYCAP_BEAM="1", POLYCAP_IMAGES="0", POLYCAP_SPOT_SHARE="%.17g" % share)
    same(effc, "POLYCAP_IMAGES=0 in chunks")
    _, effg = _public(monkeypatch, n, POLYCAP_BEAM="1", POLYCAP_HIP_DEVICES="0,0")
    same(effg, "POLYCAP_HIP_DEVICES=0,0")
    # unset: the same efficiencies and images, and no beam
    _, effn = _public(monkeypatch, n)
    assert np.array_equal(effn.data[1], F)
    nx2, vecs2, nr2, dt2, W2 = effn._exit()
    # the same photons; the public call stores them in the order they leave the optic, which varies from run to run
    o1, o2 = np.lexsort((vecs[0][:, 1], vecs[0][:, 0])), np.lexsort((vecs2[0][:, 1], vecs2[0][:, 0]))
    assert np.array_equal(W2[o2], W[o1]) and all(np.array_equal(a[o2], b[o1], equal_nan=True) for a, b in zip(vecs2, vecs))
    with pytest.raises(ValueError, match="POLYCAP_BEAM"):
        effn.beam("exit")
    # HDF5: the /Beam group
    from tests import test_hdf5_writer as H
    from polycap_amd import _cabi
    import ctypes as C
    L = _cabi.lib()
    L.pc_hdf5_provider.restype = C.c_char_p
    if H.H5LS is None or L.pc_hdf5_provider() in (None, b"none"):
        return
    path = str(tmp_path / "beam.h5")
    eff.write_hdf5(path)
    ls = H._listing(path)
    ne = len(E)
    assert ls["/Beam/Exit_Sums"] == (ne, 15, 2) and ls["/Beam/Exit_Outside"] == (ne,) and ls["/Beam/Exit_Entries"] == (1,)
    assert ls["/Beam/Exit"] == (ne, 26)
    assert not any(k.startswith("/Beam/ExtLeak") for k in ls)
    got = H._read(path, "/Beam/Exit", str(tmp_path)).reshape(ne, 26)
    want = np.stack([b1[c] for c in pa.hip.beam_columns()], axis=1)
    assert np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    pathn = str(tmp_path / "nobeam.h5")
    effn.write_hdf5(pathn)
    assert not any(k.startswith("/Beam") for k in H._listing(pathn))


def test_public_leak_run(pa, monkeypatch):
    from polycap_amd import capi
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    monkeypatch.setenv("POLYCAP_BEAM", "1")
    for k in ("POLYCAP_IMAGES", "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT"):
        monkeypatch.delenv(k, raising=False)
    src = capi.Source.new_from_file(DECK)
    eff = src.get_transmission_efficiencies(1, 3000, leak_calc=True)
    for kind in ("exit", "extleak", "intleak"):
        b = eff.beam(kind)
        assert b["n_entries"] > 0 and b["sums"].shape[1:] == (15, 2), kind


def test_cython_binding_gives_the_same_beam(pa, monkeypatch):
    from polycap_amd import capi
    from polycap_amd.pyext import polycap as cy
    monkeypatch.setenv("POLYCAP_SEED", str(SEED))
    monkeypatch.setenv("POLYCAP_BEAM", "1")
    for k in ("POLYCAP_IMAGES", "POLYCAP_HIP_DEVICES", "POLYCAP_SPOT"):
        monkeypatch.delenv(k, raising=False)
    a = capi.Source.new_from_file(DECK).get_transmission_efficiencies(1, 5000).beam("exit")
    b = cy.Source.new_from_file(DECK).get_transmission_efficiencies(1, 5000).beam("exit")
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["outside"], b["outside"]) and a["n_entries"] == b["n_entries"]
    for c in pa.hip.beam_columns():
        assert same_bits(a[c], b[c]), c

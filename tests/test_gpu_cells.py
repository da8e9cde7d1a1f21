"""The two binned tallies at their maximum group count -- Histograms of 16 axes, JointHistograms of 8 pairs -- one energy past a chunk
of the energies-across-lanes kernel: 513 energies without squares, and with squares one past 2048 / groups (129 for the histograms, 257
for the joint histograms), where the outside counters and their (lo, hi) pairs fill the kernel's LDS array to its far corner.  Sums and
square sums equal, bit for bit, the numpy restatements of tests/test_gpu_hist.py, test_joint_cpu.py and test_gpu_tally_squares.py."""
import numpy as np
import pytest

from tests.test_gpu_hist import SEED, _prob, np_expect, record_entries
from tests.test_gpu_tally_squares import same_pairs, sq_hists, sq_joint
from tests.test_joint_cpu import QUANTITIES, axis, np_joint, np_value2

pytestmark = pytest.mark.gpu

N_SLOTS = 2000
ONE_PAST = {"hist": 129, "joint": 257}            # with squares a chunk is 2048 / 16 axes = 128 and 2048 / 8 pairs = 256 energies
AXES = (("x", 5), ("y", 4), ("r", 3), ("slope_x", 7), ("slope_y", 2), ("tan_theta", 6), ("nrefl", 8), ("dtravel", 3), ("r_start", 5),
        ("x", 1), ("y", 9), ("r", 4), ("slope_x", 2), ("slope_y", 3), ("tan_theta", 4), ("r_start", 6))
PAIRS = ((("x", 5), ("slope_x", 3)), (("start_x", 4), ("start_y", 4)), (("r_start", 3), ("nrefl", 5)), (("r", 2), ("tan_theta", 6)),
         (("slope_y", 3), ("start_x", 2)), (("dtravel", 1), ("y", 7)), (("tan_theta", 4), ("r_start", 2)), (("start_y", 5), ("r", 3)))


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def cut(name, bins, E, W, ze):
    """an axis from the 15th to the 80th percentile of the run's own values: weight inside, and weight in the outside counter"""
    d = {"x": 0.5, "y": 0.5, "r": 0.25}.get(name, 0.)
    centre = (0.002, -0.001) if name == "r" else (0., 0.)
    v, ok = np_value2(QUANTITIES.index(name), E, False, ze + d, *centre)
    v = v[ok & (W[:, 0] > 0.) & np.isfinite(v)]
    lo, hi = float(np.percentile(v, 15)), float(np.percentile(v, 80))
    assert lo < hi, name
    return axis(name, lo, hi, bins, d=d, centre=centre)


def groups_of(kind, E, W, ze):
    if kind == "hist":
        return [cut(n, b, E, W, ze) for n, b in AXES]
    return [(cut(nu, bu, E, W, ze), cut(nv, bv, E, W, ze)) for (nu, bu), (nv, bv) in PAIRS]


def restated(kind, groups, E, W, ze, sel, squares):
    """the sums [S, cells], [groups, S] and, with squares, the Python-integer square sums of the same shapes"""
    sums = (np_expect if kind == "hist" else np_joint)(groups, E, W, ze, sel)
    cols = np.arange(W.shape[1]) if sel is None else np.asarray(sel)
    sq = (sq_hists if kind == "hist" else sq_joint)(groups, E, W[:, cols], ze) if squares else None
    sizes = [g["bins"] for g in groups] if kind == "hist" else [u["bins"] * v["bins"] for u, v in groups]
    off = np.cumsum([0] + sizes)
    for g in range(len(groups)):                        # by the numpy side alone: every group has weight inside and outside
        assert sums[0][:, off[g]:off[g + 1]].any() and sums[1][g].any(), (kind, g)
    return sums, sq


def test_most_groups_one_energy_past_a_chunk(pa):
    made = {"hist": pa.Histograms, "joint": pa.JointHistograms}
    cells = {"hist": "bins", "joint": "cells"}
    # energies of the problem -> (kind, regime, squares, selection); the selections are not ascending and cross the chunk's end
    plan = {513: [(k, 2, False, None) for k in made]
                 + [("hist", r, True, list(range(400, 400 - 129, -1))) for r in (1, 2)]
                 + [("joint", r, True, list(range(400, 400 - 257, -1))) for r in (1, 2)],
            129: [("hist", 2, True, None), ("hist", 1, True, None)],
            257: [("joint", 2, True, None), ("joint", 1, True, None)]}
    for ne, cases in plan.items():
        prob = _prob(pa, ne)
        ze = float(prob.z[-1])
        want = {}
        with pa.TraceContext(prob, 0) as ctx:
            ctx.run(SEED, 0, N_SLOTS, keep_images=True)
            ctx.wait()
            E, W = record_entries(ctx.records())
            assert len(E) == N_SLOTS
            for kind, regime, squares, sel in cases:
                what = "%s, %d energies, regime %d, squares %s, selection %s" % (kind, ne, regime, squares, sel is not None)
                groups = groups_of(kind, E, W, ze)
                assert len(groups) == {"hist": 16, "joint": 8}[kind]
                ns = ne if sel is None else len(sel)
                assert ns == (ONE_PAST[kind] if squares else 513), what
                key = (kind, squares, sel is not None)
                if key not in want:
                    want[key] = restated(kind, groups, E, W, ze, sel, squares)
                (sums, out), sq = want[key]
                with made[kind](ctx, groups, energies=sel, regime=regime, squares=squares) as t:
                    assert t.regime == regime and t.n_selected == ns, what
                    t.add("exit")
                    got = t.read()
                assert got["n_entries"].tolist() == [N_SLOTS, 0, 0], what
                assert np.array_equal(got[cells[kind]][0], sums), "sums differ from numpy: " + what
                assert np.array_equal(got["outside"][0], out), "outside counters differ from numpy: " + what
                assert got["outside"][0, -1, -1] != 0, what              # the last group's counter at the last energy: the LDS array's far corner
                if squares:
                    same_pairs(got["squares"][0], sq[0], what + ": squares")
                    same_pairs(got["outside_squares"][0], sq[1], what + ": outside_squares")
                    assert got["outside_squares"][0, -1, -1].any(), what

"""The decisions about a leak_calc=true run without a GPU: the pure functions of polycap_amd/csrc/hip/pc_leak_plan.h, compiled for
the host (tests/plan/leak_host.cpp).  The expected values are written out from the formulas the planner documents:

    per_lane = max_depth*(PC_LF_HDR + ne)*8,  blocks = max(1, min(ceil(n/256), 2*n_cu, max(1, (stack_bytes/per_lane)/256)))
    first capacity = option if > 0 else max(floor, (16 + 8 ne) n);  grown = needed + needed/4 + 1024
    an automatic order is considered when enabled and 2*lanes <= n < 5*lanes and n < 2^32
    the slots are ordered when top*4*lanes > 0.8*13*total: descending, stable; n_heavy = min(n/400, 2*n_cu)"""
import numpy as np
import pytest

from tests.plan.pyleakplan import LeakPlanner

N_CU = 256
BIG = 8 << 30


@pytest.fixture(scope="module")
def lp(tmp_path_factory):
    return LeakPlanner(tmp_path_factory.mktemp("leak_host"))


def test_shapes(lp):
    assert lp.block == 256 and lp.frame_header == 24


@pytest.mark.parametrize("n_items, blocks", [(1, 1), (256, 1), (257, 2), (10**7, 512)])
def test_grid_by_items_and_compute_units(lp, n_items, blocks):
    assert lp.grid(n_items, 1, 40, BIG, N_CU) == (blocks, blocks * 256)


@pytest.mark.parametrize("ne", [1, 7])
def test_grid_by_stack_budget(lp, ne):
    per_lane = 40 * (24 + ne) * 8
    assert lp.grid(10**7, ne, 40, 3 * 256 * per_lane + 1, N_CU) == (3, 768)
    assert lp.grid(10**7, ne, 40, 3 * 256 * per_lane - 1, N_CU) == (2, 512)
    assert lp.grid(10**7, ne, 40, 256 * per_lane - 1, N_CU) == (1, 256)         # less than one block's stacks: the floor
    assert lp.grid(10**7, ne, 40, 1, N_CU) == (1, 256)
    assert lp.grid(300, ne, 40, 3 * 256 * per_lane + 1, N_CU) == (2, 512)       # fewer items than the budget allows


def test_first_capacity(lp):
    assert lp.capacity(5, 1, 10**6, 65536) == 5                                 # an option above 0 wins
    assert lp.capacity(0, 1, 1, 65536) == 65536
    assert lp.capacity(0, 7, 10000, 65536) == 720000
    assert lp.capacity(0, 1, 1, 4096) == 4096


def test_grown_capacity(lp):
    assert [lp.grown(n) for n in (0, 7, 10**9)] == [1024, 1032, 1250001024]


def test_window_in_which_an_order_is_considered(lp):
    assert [lp.considered(True, n, 256) for n in (511, 512, 1279, 1280)] == [False, True, True, False]
    assert not lp.considered(False, 600, 256)
    # the two sizes the project uses, on a device of 256 compute units (2*256*256 lanes)
    assert not lp.considered(True, 200000, 131072)
    assert lp.considered(True, 262144, 131072)
    assert not lp.considered(True, 2**32, 2**31)


def test_bound_by_the_longest_slot(lp):
    flat = lp.order(np.full(600, 10), 256, N_CU)
    assert not flat["ordered"] and (flat["top"], flat["total"], flat["n_heavy"]) == (10, 6000, 0)
    est = np.ones(600, dtype=np.uint32)
    est[123] = 1000
    one = lp.order(est, 256, N_CU)
    assert one["ordered"] and (one["top"], one["total"], one["n_heavy"]) == (1000, 1599, 1)
    assert one["order"][0] == 123 and np.array_equal(one["order"][1:], np.delete(np.arange(600), 123))


def _python_order(est):
    return np.array(sorted(range(len(est)), key=lambda k: -int(est[k])), dtype=np.uint32)


def test_order_is_descending_and_stable(lp):
    """5000 slots with values 0..50 (many ties); lanes = 2^20 makes the bound true (50*4*2^20 > 10.4*total).  One value at 2^22 - 1
    and at 2^22 crosses the switch between the counting sort and the comparison sort: both equal Python's stable sort exactly."""
    rng = np.random.default_rng(11)
    est = rng.integers(0, 51, 5000).astype(np.uint32)
    for big in (None, 2**22 - 1, 2**22):
        e = est.copy()
        if big is not None:
            e[777] = big
        got = lp.order(e, 2**20, N_CU)
        assert got["ordered"] and got["top"] == int(e.max()) and got["total"] == int(e.astype(np.uint64).sum())
        assert np.array_equal(got["order"], _python_order(e))
        assert got["n_heavy"] == 5000 // 400


def test_all_zero_estimate_keeps_the_slot_order(lp):
    """total = 0 makes the bound 0 > 0, which is false whatever the lanes: nothing to order by"""
    got = lp.order(np.zeros(5000, dtype=np.uint32), 2**20, N_CU)
    assert not got["ordered"] and (got["top"], got["total"]) == (0, 0)


@pytest.mark.parametrize("n, n_heavy", [(399, 0), (400, 1), (204800, 512), (10**6, 512)])
def test_heavy_tier(lp, n, n_heavy):
    est = np.ones(n, dtype=np.uint32)
    est[0] = 2**30                  # one slot that dwarfs the rest: ordered at any of these sizes
    got = lp.order(est, 256, N_CU)
    assert got["ordered"] and got["n_heavy"] == n_heavy
    assert got["order"][0] == 0 and np.array_equal(got["order"][1:], np.arange(1, n))

"""The launching-wave kernel's tracing loop against the one-photon-per-lane kernel, bit for bit, on the compact image store.

pc_trace_producer_kernel's tracing waves read their ring's tail at the head of a turn only when a lane waits for a photon
(PC3_POLL_WHEN_NEEDED, pc_producer_kernel.h) and decide a march step by one comparison against the margin of the stride taken
(PC_ONE_MARGIN_TEST, pc_device.h: that kernel alone, the lane kernel keeps the three-way test).  The build's other switches for
that loop (PC_FUSE_FIRST, PC_WALK_PIPE, PC3_BND_PER_BURST, PC3_DONE_AT_ADVANCE) are off and are not built by this file: a build
that turns one on is held to the same comparison by running it.  None of it may change a bit: a photon depends on (seed, slot,
attempt) only and the sums are exact integers, so the counters, the exact sums, and -- put in slot order by the slot-index
plane -- the compact planes, exit weights and reflection counts must equal those of pc_trace_kernel (options "producer" 0,
"pool" 0), whose loop polls nothing.

Shapes: xos1 at 1, 64, 65 slots (less than, exactly and one more than a wave), 960 and 961 (one more than the 15 x 64 tracing
lanes of a workgroup) and 20 000; cone.inp at 20 000 (photons hardly reflect: the rings run dry and lanes linger without a
slot, which is where the ring's tail is and is not read); a mono-capillary at 5 000 (every lane a boundary one: the hexagon
tests inside the march step and the visit); xos1 with 2 attempts per slot (slots fail)."""
import os

import numpy as np
import pytest

from tests.common import MONO_CASE, make_custom
from tests.conftest import EXAMPLE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problems(oracle):
    import polycap_amd as pa
    return {"xos1": pa.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"), energies=[10.0]),
            "cone": pa.problem_from_inp(os.path.join(EXAMPLE, "cone.inp"), energies=[10.0]),
            "mono": make_custom(oracle, **MONO_CASE)[2]}


def _run(ctx, n, max_attempts):
    ctx.run(20000, 0, n, max_attempts=max_attempts, keep_images=True)
    ctx.wait()
    t = ctx.totals(check=False)
    n_exit = int(t["counters"][0])             # the compact store holds the exit photons only: positions [0, n_exit)
    return ctx.image_planes(0, n_exit), ctx.slot_ids(0, n_exit), t


def _in_slot_order(planes, ids):
    """the compact store's planes (the exit photons, in order of completion), sorted by slot"""
    o = np.argsort(ids, kind="stable")
    return dict(ids=ids[o], planes=planes["planes"][:, o], exit_weights=planes["exit_weights"][o], nrefl=planes["nrefl"][o])


CASES = [("xos1", 1, 1 << 20), ("xos1", 64, 1 << 20), ("xos1", 65, 1 << 20), ("xos1", 960, 1 << 20), ("xos1", 961, 1 << 20),
         ("xos1", 20000, 1 << 20), ("cone", 20000, 1 << 20), ("mono", 5000, 1 << 20), ("xos1", 20000, 2)]


@pytest.mark.parametrize("name,n,max_attempts", CASES)
def test_producer_kernel_equals_lane_kernel_on_the_compact_store(problems, name, n, max_attempts):
    import polycap_amd as pa
    res = {}
    with pa.TraceContext(problems[name]) as ctx:
        for k, v in (("pool", 0), ("plane_images", 1), ("compact_images", 1), ("slot_ids", 1)):
            ctx.set_option(k, v)
        for kernel, producer in (("pc_trace_kernel", 0), ("pc_trace_producer_kernel", 1)):
            ctx.set_option("producer", producer)
            planes, ids, t = _run(ctx, n, max_attempts)
            assert ctx.last_kernel() == kernel
            res[kernel] = (t, _in_slot_order(planes, ids))
    (ta, a), (tb, b) = res["pc_trace_kernel"], res["pc_trace_producer_kernel"]
    assert np.array_equal(ta["counters"], tb["counters"]) and np.array_equal(ta["sumw_fixed"], tb["sumw_fixed"])
    n_exit = int(ta["counters"][0])
    assert n_exit > 0 and len(np.unique(a["ids"])) == n_exit            # photons left the optic, every slot at most once
    assert np.array_equal(a["ids"], b["ids"])
    assert np.array_equal(a["planes"], b["planes"], equal_nan=True)
    assert np.array_equal(a["exit_weights"], b["exit_weights"])
    assert np.array_equal(a["nrefl"], b["nrefl"])
    if max_attempts == 2:
        assert ta["failed_slots"] > 0 and n_exit < n
    else:
        assert n_exit == n and ta["failed_slots"] == 0

"""The launching-wave kernel's tracing loop against the one-photon-per-lane kernel, bit for bit.

The tracing waves of pc_trace_producer_kernel choose their phase as a wave-uniform number and run the phases as sibling
branches with one way round the loop (pc_producer_kernel.h); the lane kernel (options "producer" 0, "pool" 0) keeps the plain
loop.  A photon depends on (seed, slot, attempt) only and the sums are exact integers, so counters, the fixed-point weight
sum, exit weights and every image plane must be equal -- on problems that take every exit of the segment visit: a rough
surface, a profile of 9 nodes (reflection limit, end of profile inside a visit), a mono-capillary and boundary capillaries
(hexagon tests), and an elliptical source (src_x != src_y: the kernels' other source mode, an instantiation of its own),
with attempts unlimited and cut at 2 (failed slots)."""
import numpy as np
import pytest

from tests.common import GLASS, MONO_CASE, PIN_AMU, PIN_E, PIN_SCATF, SEVEN_CASE, load_xos1_tables, make_custom, make_pair

pytestmark = pytest.mark.gpu

SOURCE = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)


def _xos1_9_nodes(oracle):
    """xos1 cut to every 125th node, ends kept: nmax = 8."""
    from polycap_amd import Problem
    z, cap, ext = load_xos1_tables()
    idx = np.unique(np.append(np.arange(0, len(z), 125), len(z) - 1))
    assert len(idx) == 9
    optic = oracle.Optic(z[idx].copy(), cap[idx].copy(), ext[idx].copy(), 0.0, 200000, GLASS["density"])
    return Problem(optic.z, optic.cap, optic.ext, 0.0, 200000, GLASS["density"], np.array([PIN_E]), np.array([PIN_AMU]),
                   np.array([PIN_SCATF]), *SOURCE)


@pytest.fixture(scope="module")
def problems(oracle):
    return {"xos1": make_pair(oracle, "xos1")[2],
            "xos1_rough": make_pair(oracle, "xos1", sig_rough=5.0)[2],
            "xos1_9_nodes": _xos1_9_nodes(oracle),
            "xos1_elliptical": make_pair(oracle, "xos1", source=(2000., 0.2065, 0.15, 0., 0., 0., 0., 0.5))[2],
            "mono": make_custom(oracle, **MONO_CASE)[2],
            "seven": make_custom(oracle, **SEVEN_CASE)[2]}


CASES = [("xos1", 4096), ("xos1", 37), ("xos1_rough", 4096), ("xos1_9_nodes", 4096), ("mono", 4096), ("seven", 4096),
         ("xos1_elliptical", 4096)]


@pytest.mark.parametrize("max_attempts", [1 << 20, 2])
@pytest.mark.parametrize("name,n", CASES)
def test_producer_kernel_equals_lane_kernel(problems, name, n, max_attempts):
    import polycap_amd as pa
    res = {}
    with pa.TraceContext(problems[name]) as ctx:
        ctx.set_option("pool", 0)
        for kernel, producer in (("pc_trace_kernel", 0), ("pc_trace_producer_kernel", 1)):
            ctx.set_option("producer", producer)
            ctx.run(77, 1000, n, max_attempts=max_attempts, keep_images=True)
            ctx.wait()
            r = ctx.totals(check=False)
            r.update(ctx.images(0, n))
            assert ctx.last_kernel() == kernel
            res[kernel] = r
    a, b = res["pc_trace_kernel"], res["pc_trace_producer_kernel"]
    done = a["exit_weights"][:, 0] > 0            # a slot that ran out of attempts has weight 0 and no defined exit planes
    assert np.array_equal(a["counters"], b["counters"]) and np.array_equal(a["sumw_fixed"], b["sumw_fixed"])
    assert np.array_equal(a["exit_weights"], b["exit_weights"])
    assert np.array_equal(a["images"][done], b["images"][done], equal_nan=True)
    assert np.array_equal(a["images"][~done, :8], b["images"][~done, :8], equal_nan=True)
    assert a["counters"][0] > 0                   # photons did leave the optic
    if max_attempts == 2:
        assert a["failed_slots"] > 0 and not done.all()

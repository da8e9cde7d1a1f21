"""The launching-wave kernel with the packed margins and the select tail of its march step against the lane kernel, bit for bit.

pc_march_ok forms the margins of its two block strides as one pair of floats (packed multiply, add and fused multiply-add),
keeps the certificate value in single precision, and writes the outcome of a step as selects on the live values; the
launching-wave kernel sets the return code of a photon that reached the end of the optic once per burst of steps.  None of it
may change a bit: a photon depends on (seed, slot, attempt) only and the sums are exact integers, so counters, the
fixed-point weight sum, exit weights and every image plane of pc_trace_producer_kernel must equal those of pc_trace_kernel
(options "producer" 0, "pool" 0), which runs the same device functions in the plain one-photon-per-lane loop.

Problems: xos1 with the round source and with an elliptical one (the kernels' two source modes, an instantiation each), at 4096
slots (4 waves' worth per ring) and at 70000 (more than 2^16, every workgroup busy, rings refilled many times); xos1 cut to
30 nodes, where a block of PC_L2 = 25 segments fits from the first 5 nodes only and every other start node holds the infinite
margin of a stride that does not fit, and flights end inside blocks; and an optic of 37 capillaries in three rings whose
radius (0.24 of the optic's) reaches past the outer hexagon from the outer ring, so that its 18 capillaries (49 %) are boundary
ones by the launch's rule and take the hexagon tests inside the march step (the capillaries are drawn wider than their
spacing for that: every photon is traced in the one capillary it entered, so the overlap means nothing to either kernel)."""
import numpy as np
import pytest

from tests.common import GLASS, PIN_AMU, PIN_E, PIN_SCATF, load_xos1_tables, make_custom, make_pair

pytestmark = pytest.mark.gpu

SOURCE = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)
RINGS3_CASE = dict(shape=(0, 5., 0.05, 0.04, 0.012, 0.0096, 1000., 0.5), n_cap=37, source=(50., 0.05, 0.05, 0.002, 0.002, 0., 0., 0.3))


def _xos1_30_nodes(oracle):
    """xos1 cut to 30 nodes spread evenly over its length, ends kept: nmax = 29."""
    from polycap_amd import Problem
    z, cap, ext = load_xos1_tables()
    idx = np.unique(np.round(np.linspace(0, len(z) - 1, 30)).astype(int))
    assert len(idx) == 30
    optic = oracle.Optic(z[idx].copy(), cap[idx].copy(), ext[idx].copy(), 0.0, 200000, GLASS["density"])
    return Problem(optic.z, optic.cap, optic.ext, 0.0, 200000, GLASS["density"], np.array([PIN_E]), np.array([PIN_AMU]),
                   np.array([PIN_SCATF]), *SOURCE)


@pytest.fixture(scope="module")
def problems(oracle):
    return {"xos1": make_pair(oracle, "xos1")[2],
            "xos1_elliptical": make_pair(oracle, "xos1", source=(2000., 0.2065, 0.15, 0., 0., 0., 0., 0.5))[2],
            "xos1_30_nodes": _xos1_30_nodes(oracle),
            "rings3": make_custom(oracle, **RINGS3_CASE)[2]}


def test_problems_take_the_paths_they_are_here_for(problems):
    """The 30-node profile holds finite PC_L1 and PC_L2 margins at its first nodes only (strides are taken there and refused by
    an infinite margin everywhere else), and more than 10 % of the capillaries of the three-ring optic are boundary ones by
    the launch's own rule (pc_launch_init)."""
    from tests.emul import pyemul
    t = pyemul.march_tables(problems["xos1_30_nodes"])
    nmax = len(t["z"]) - 1
    assert (t["L1"], t["L2"], nmax) == (5, 25, 29)
    fits1, fits2 = np.arange(nmax + 1) + t["L1"] <= nmax, np.arange(nmax + 1) + t["L2"] <= nmax
    assert fits2.sum() == 5 and np.all(np.isfinite(t["mg_mb2"][fits2])) and np.all(np.isinf(t["mg_mb2"][~fits2]))
    assert fits1.sum() == 25 and np.all(np.isfinite(t["mg_mb1"][fits1])) and np.all(np.isinf(t["mg_mb1"][~fits1]))
    t = pyemul.march_tables(problems["rings3"])
    n = int(t["n_shells"])
    cos_pi_6 = 0.86602540378443864676
    qr = [(q, r) for q in range(-n, n + 1) for r in range(-n, n + 1) if max(abs(q), abs(r), abs(q + r)) <= n]
    assert len(qr) == 37
    bnd = 0
    for q, r in qr:
        ky, kx = r*1.5, (2.*q + r)*cos_pi_6
        m = max(abs(ky), abs(cos_pi_6*kx + 0.5*ky), abs(cos_pi_6*kx - 0.5*ky))
        bnd += not (cos_pi_6 - m/t["hexscale"] > t["bnd_thresh"])
    assert bnd/len(qr) > 0.10


CASES = [("xos1", 4096), ("xos1", 70000), ("xos1_elliptical", 4096), ("xos1_elliptical", 70000), ("xos1_30_nodes", 4096),
         ("rings3", 4096)]


@pytest.mark.parametrize("name,n", CASES)
def test_producer_kernel_equals_lane_kernel(problems, name, n):
    import polycap_amd as pa
    res = {}
    with pa.TraceContext(problems[name]) as ctx:
        ctx.set_option("pool", 0)
        for kernel, producer in (("pc_trace_kernel", 0), ("pc_trace_producer_kernel", 1)):
            ctx.set_option("producer", producer)
            ctx.run(20000, 0, n, max_attempts=1 << 20, keep_images=True)
            ctx.wait()
            r = ctx.totals(check=False)
            r.update(ctx.images(0, n))
            assert ctx.last_kernel() == kernel
            res[kernel] = r
    a, b = res["pc_trace_kernel"], res["pc_trace_producer_kernel"]
    assert np.array_equal(a["counters"], b["counters"]) and np.array_equal(a["sumw_fixed"], b["sumw_fixed"])
    assert np.array_equal(a["exit_weights"], b["exit_weights"])
    assert np.array_equal(a["images"], b["images"], equal_nan=True)
    assert a["counters"][0] == n and a["failed_slots"] == 0       # every slot ended with a photon that left the optic
    assert a["counters"][3] > 0                                   # and photons were reflected on the way

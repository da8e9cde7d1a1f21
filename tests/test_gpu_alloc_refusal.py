"""A device allocation the runtime refuses fails the run with PC_HIP_ERR_MEMORY (-4) and a message that names the buffer, and
leaves the context as usable as a fresh one: the next run gives the same results bit for bit.

The refused buffers are far larger than any device (about 9 TB), so the runtime turns them down at the call and no kernel ever
sees them.  A refusal must also leave no HIP error stored behind it: the next launch checks hipGetLastError, and a stale
out-of-memory there would fail a run that worked."""
import os

import numpy as np
import pytest

from tests.common import make_pair
from tests.conftest import EXAMPLE

pytestmark = pytest.mark.gpu

DECK = os.path.join(EXAMPLE, "xos1.inp")
SEED = 4242
HUGE = 1 << 36              # slots or records: 18 doubles each make about 9.9 TB


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def _records_context(pa, prob):
    ctx = pa.TraceContext(prob, 0)
    ctx.set_option("producer", 0)           # the lane kernel in both contexts, and no lifetime probe ahead of a big run
    ctx.set_option("plane_images", 0)       # the records store
    return ctx


def test_refused_image_records(pa):
    prob = pa.problem_from_inp(DECK, energies=[10.0])
    n = 65536
    with _records_context(pa, prob) as ctx:
        with pytest.raises(pa.HipError) as e:
            ctx.run(SEED, 0, HUGE, keep_images=True)
        assert e.value.status == -4
        assert "could not allocate the image planes" in str(e.value)
        got = ctx.transmission(SEED, 0, n, keep_images=True)
    with _records_context(pa, prob) as ctx:
        ref = ctx.transmission(SEED, 0, n, keep_images=True)
    assert got["i_exit"] == n
    assert np.array_equal(got["counters"], ref["counters"])
    assert np.array_equal(got["sumw_fixed"], ref["sumw_fixed"])


def test_refused_leak_records(pa, oracle):
    _, _, prob, _ = make_pair(oracle, "ellip")
    n = 300
    with pa.TraceContext(prob, 0) as ctx:
        ctx.set_option("leak_capacity", HUGE)
        with pytest.raises(pa.HipError) as e:
            ctx.run(SEED, 0, n, leak_calc=True)
        assert e.value.status == -4
        assert "could not allocate the leak record buffer" in str(e.value)
        ctx.set_option("leak_capacity", 0)
        got = ctx.transmission(SEED, 0, n, leak_calc=True)
    with pa.TraceContext(prob, 0) as ctx:
        ref = ctx.transmission(SEED, 0, n, leak_calc=True)
    assert len(ref["ext"]) + len(ref["int"]) > 0
    for k in ("counters", "sumw_fixed", "ext", "int"):
        assert np.array_equal(got[k], ref[k]), k

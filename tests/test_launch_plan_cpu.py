"""The launch plan without a GPU: pc_plan_launch of polycap_amd/csrc/hip/pc_plan.h, compiled for the host (tests/plan/plan_host.cpp),
must make for every recorded launch exactly the decisions that tests/golden/launch_plans.json holds.

The fixture was recorded on an MI355X from the commit BEFORE the planner existed: its launch code, patched to print what it was
about to launch (kernel, grid, block, dynamic LDS, the flags and thresholds it put into the kernel arguments, the scratch it
allocated), was driven over the cases below.  Each recorded launch also carries what the old code read to decide (problem sizes,
options, the call), which is what the planner is given here.  The shapes are also checked against DESIGN.md section 5."""
import json
import os

import pytest

from tests.conftest import GOLDEN
from tests.plan.pyplan import Planner

with open(os.path.join(GOLDEN, "launch_plans.json")) as _f:
    FIXTURE = json.load(_f)
CASES = FIXTURE["cases"]
N_CU = FIXTURE["n_cu"]
LANE, POOL, PRODUCER, WAVE, LOG = range(5)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return Planner(tmp_path_factory.mktemp("plan_host"))


def _replan(planner, launch):
    inputs = {k: launch["in"][k] for k in planner.input_names}
    return planner.plan(inputs, launch["opts"])


def test_fixture_covers_the_case_list():
    """what the fixture has to contain, so that a lost case is noticed"""
    names = set(CASES)
    assert N_CU == 256
    assert all(CASES[n] for n in names), "a case without a launch"
    for ne in (1, 3, 7, 9, 12, 40, 64, 291, 448, 449, 1000, 1400, 1700):
        assert {"src_ne%d_sq0" % ne, "src_ne%d_sq1" % ne, "exp_ne%d" % ne} <= names
    for ne in (1, 4, 8, 12, 597, 598):
        assert {"scan_ne%d_sq0" % ne, "scan_ne%d_sq1" % ne} <= names
    assert {"src_long_ne1_sq0", "src_long_ne4_sq0", "scan_long_ne1", "scan_long_ne4", "exp_long_ne4",
            "src_ne1_refl_unknown", "src_ne1_refl_0.5", "src_ne1_refl_20", "src_ne1_producer0_refl_20", "src_ne1_producer1",
            "src_ne1_pool1", "src_ne1_literal_producer1_pool1", "src_ne1_attempts_big_producer1", "src_ne12_batch0",
            "src_ne12_logcap8", "src_ne12_invalid", "src_ne1_keep", "src_ne12_keep", "src_ne1_1e3", "src_ne1_1e7", "src_ne12_1e7",
            "src_ne1_cu_share4", "src_ne12_cu_share4", "src_ne12_two_parts"} <= names
    modes = {(l["in"]["mode"], l["out"]["kernel"]) for c in CASES.values() for l in c}
    assert modes == {(0, LANE), (0, POOL), (0, PRODUCER), (0, LOG), (1, LANE), (2, LANE)}
    # both scratch halves of a run in parts, and the probe in front of a big first run
    assert {l["in"]["half"] for l in CASES["src_ne12_two_parts"]} == {0, 1}
    assert [l["in"]["force_lane"] for l in CASES["src_ne1_1e7"]] == [1, 0]
    assert [l["in"]["n_items"] for l in CASES["src_ne1_1e7"]] == [32768, 10000000]


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_recorded_launch(planner, name):
    for i, launch in enumerate(CASES[name]):
        got, want, site = _replan(planner, launch), launch["out"], launch["in"]
        for field in planner.field_names:
            assert got[field] == want[field], (name, i, field, got[field], want[field])
        # what the launcher derives from the plan and the launch site
        assert got["grid"] * got["block"] == want["total_threads"], (name, i)
        assert site["half"] * got["half_w"] == want["wscratch_off"], (name, i)
        assert site["half"] * got["half_l"] == want["rlog_off"], (name, i)


def test_fixture_agrees_with_the_design_document():
    """DESIGN.md section 5, Launch: lane kernels CUs x 2 x 512 threads, launching-wave kernel CUs x 1024, pool kernel CUs x 768, many-energy
    kernels one 512-thread workgroup per CU, the logging kernel from 9 energies on; a launch too small to fill the device gets as many
    workgroups as its items need"""
    def shape(launch):
        o = launch["out"]
        return o["kernel"], o["grid"], o["block"]
    # launches that fill the device
    assert shape(CASES["exp_ne1_sq1"][0]) == (LANE, 2 * N_CU, 512)                 # weights in registers
    assert shape(CASES["src_ne3_1e7"][0]) == (LANE, 2 * N_CU, 512)
    assert shape(CASES["src_ne1_1e7"][1]) == (PRODUCER, N_CU, 1024)
    assert shape(CASES["src_ne12_1e7"][0]) == (LOG, N_CU, 512)
    assert shape(CASES["src_ne12_batch0_two_parts"][0]) == (LANE, N_CU, 512)       # immediate sweeps
    # smaller ones: ceil(items / items per workgroup)
    assert shape(CASES["src_ne1_refl_unknown"][0]) == (LANE, -(-100000 // 512), 512)
    assert shape(CASES["src_ne7_sq0"][0]) == (LANE, -(-20000 // 512), 512)
    assert shape(CASES["src_ne9_sq0"][0]) == (LOG, -(-20000 // 512), 512)
    assert shape(CASES["src_ne291_sq0"][0]) == (LOG, -(-4000 // 512), 512)
    assert shape(CASES["src_ne1_refl_20"][0]) == (PRODUCER, -(-100000 // (15 * 64)), 1024)    # 15 tracing waves
    assert shape(CASES["src_ne1_pool1"][0]) == (POOL, -(-100000 // (12 * 128)), 768)          # 12 waves of 64 + 64 photons
    assert CASES["src_ne12_batch0"][0]["out"]["kne"] == 0


def test_option_defaults(planner):
    """the defaults of pc_launch_opts are those the recorded contexts ran with"""
    (l,) = CASES["src_ne1_refl_unknown"]
    assert planner.default_opts == l["opts"]


def test_experiment_kernel_is_planned_only_in_its_build(tmp_path_factory):
    """-DPC_EXPERIMENTS: option wave_per_photon sends single-energy histogram-only source runs to the wave-per-photon kernel, 4 workgroups of
    256 threads per CU of the whole device; without the define the option changes nothing"""
    (l,) = CASES["src_ne1_refl_unknown"]
    product = Planner(tmp_path_factory.mktemp("plan_product"))
    inputs = {k: l["in"][k] for k in product.input_names}
    assert product.plan(inputs, dict(l["opts"], wave_per_photon=1, cu_share=4))["kernel"] == LANE
    exp = Planner(tmp_path_factory.mktemp("plan_experiments"), flags=("-DPC_EXPERIMENTS",))
    p = exp.plan(inputs, dict(l["opts"], wave_per_photon=1, cu_share=4))
    assert (p["kernel"], p["grid"], p["block"], p["dyn_lds"]) == (WAVE, 4 * N_CU, 256, 0)
    assert exp.plan(dict(inputs, keep_images=1), dict(l["opts"], wave_per_photon=1))["kernel"] == LANE
    assert exp.plan(dict(inputs, n_items=10), dict(l["opts"], wave_per_photon=1))["grid"] == 3

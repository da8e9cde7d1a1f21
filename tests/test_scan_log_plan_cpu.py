"""The launch plan of scans with context option "scan_log", without a GPU: pc_plan_launch of polycap_amd/csrc/hip/pc_plan.h compiled
for the host with pc_plan_input::scan_log among the inputs (tests/plan/plan_scan_host.cpp).

scan_log = 0 plans every recorded scan of tests/golden/launch_plans.json as it was recorded.  scan_log = 1 sends the scans that a
source run of the same problem would log to the logging kernel in the shape of that source run (so that a point's log cuts are a
separate run's), leaves every other scan with its lane plan, and changes no source or explicit plan."""
import ctypes as C
import json
import os
import subprocess

import pytest

from tests.conftest import GOLDEN

HERE = os.path.dirname(os.path.abspath(__file__))
HIPD = os.path.join(os.path.dirname(HERE), "polycap_amd", "csrc", "hip")

with open(os.path.join(GOLDEN, "launch_plans.json")) as _f:
    CASES = json.load(_f)["cases"]
SCANS = sorted(n for n in CASES if n.startswith("scan"))
OTHERS = sorted(n for n in CASES if not n.startswith("scan"))
SOURCE, EXPLICIT, SCAN = range(3)
LANE, LOG = 0, 4


class ScanPlanner:
    """tests/plan/plan_scan_host.cpp built and called with dicts (the way tests/plan/pyplan.py calls plan_host.cpp)"""

    def __init__(self, directory):
        so = os.path.join(str(directory), "plan_scan_host.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-fPIC", "-shared", "-I", HIPD,
                               os.path.join(HERE, "plan", "plan_scan_host.cpp"), "-o", so])
        self.L = L = C.CDLL(so)
        for fn in (L.plan_opt_names, L.plan_input_names, L.plan_field_names):
            fn.restype = C.c_char_p
        self.opt_names = L.plan_opt_names().decode().split()
        self.input_names = L.plan_input_names().decode().split()
        self.field_names = L.plan_field_names().decode().split()

    def plan(self, launch, scan_log, inputs=None, opts=None):
        """the recorded launch replanned with scan_log and with the given inputs and options changed"""
        i = dict(launch["in"], scan_log=scan_log, **(inputs or {}))
        o = dict(launch["opts"], **(opts or {}))
        assert set(o) == set(self.opt_names) and set(self.input_names) <= set(i)
        co = (C.c_int32 * len(self.opt_names))(*[int(o[k]) for k in self.opt_names])
        ci = (C.c_double * len(self.input_names))(*[float(i[k]) for k in self.input_names])
        out = (C.c_int64 * len(self.field_names))()
        self.L.plan_launch(co, ci, out)
        return dict(zip(self.field_names, out))


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return ScanPlanner(tmp_path_factory.mktemp("plan_scan_host"))


def _recorded(planner, launch):
    return {f: launch["out"][f] for f in planner.field_names}


def test_the_shim_passes_the_field(planner):
    assert planner.input_names[-1] == "scan_log" and "scan_log" not in planner.opt_names
    assert {"scan_ne%d_sq%d" % (ne, sq) for ne in (1, 4, 8, 12, 597, 598) for sq in (0, 1)} <= set(SCANS)
    assert {"scan_long_ne1", "scan_long_ne4", "scan_long_ne12", "scan_ne12_lds_ec0"} <= set(SCANS)
    assert all(l["in"]["mode"] == SCAN for n in SCANS for l in CASES[n])
    assert all(l["in"]["mode"] != SCAN for n in OTHERS for l in CASES[n])


@pytest.mark.parametrize("name", SCANS)
def test_scan_log_0_plans_the_recorded_scan(planner, name):
    for launch in CASES[name]:
        assert planner.plan(launch, 0) == _recorded(planner, launch), name


@pytest.mark.parametrize("name", ["scan_ne%d_sq%d" % (ne, sq) for ne in (12, 597, 598) for sq in (0, 1)] + ["scan_ne12_cu_share4"])
def test_scan_log_1_logs_in_the_shape_of_a_source_run(planner, name):
    (launch,) = CASES[name]
    assert launch["out"]["kernel"] == LANE
    p = planner.plan(launch, 1)
    # a histogram-only source run of the same problem and item count
    s = planner.plan(launch, 0, inputs=dict(mode=SOURCE, keep_images=0))
    assert p["kernel"] == LOG and s["kernel"] == LOG, (name, p, s)
    for f in ("block", "log_cap", "stage_ps", "flush_min", "dyn_lds", "grid", "stage_doubles", "half_w", "half_l", "sweep_skip",
              "sweep_fuse", "sweep_exact_every", "sq", "sweep_rough"):
        assert p[f] == s[f], (name, f, p[f], s[f])
    ne = launch["in"]["ne"]
    assert p["block"] == 512 and p["grid"] == min(256 // launch["opts"]["cu_share"], -(-launch["in"]["n_items"] // 512))
    assert p["log_cap"] == (64 if ne >= 64 else 32) and p["stage_ps"] >= 1 and 1 <= p["flush_min"] <= p["stage_ps"]
    assert p["half_l"] == 3 * p["log_cap"] * p["grid"] * 512 and p["half_w"] == ne * p["grid"] * 512
    assert (p["sweep_skip"], p["sweep_fuse"]) == (1, 1)
    # the log stage fits beside the static tables: 160 KB of LDS per workgroup
    assert p["dyn_lds"] + 6 * 1024 * 8 + 1024 * 16 <= 163840


def test_scan_log_1_follows_the_log_options(planner):
    (launch,) = CASES["scan_ne12_sq1"]
    for opts in (dict(log_cap=8), dict(sweep_fuse=2, sweep_exact_every=3, sweep_skip=0), dict(flush_max=2), dict(log_min_energies=12)):
        p = planner.plan(launch, 1, opts=opts)
        s = planner.plan(launch, 0, inputs=dict(mode=SOURCE), opts=opts)
        assert p["kernel"] == LOG
        for f in ("block", "log_cap", "stage_ps", "flush_min", "dyn_lds", "sweep_skip", "sweep_fuse", "sweep_exact_every"):
            assert p[f] == s[f], (opts, f)
    assert planner.plan(launch, 1, opts=dict(log_cap=8))["log_cap"] == 8
    assert planner.plan(launch, 1, opts=dict(log_min_energies=13)) == _recorded(planner, launch)


@pytest.mark.parametrize("name", [n for n in SCANS if CASES[n][0]["in"]["ne"] <= 8 or "long" in n or "lds_ec0" in n])
def test_scan_log_1_keeps_the_lane_plan_of_scans_that_cannot_log(planner, name):
    for launch in CASES[name]:
        assert planner.plan(launch, 1) == _recorded(planner, launch), name


def test_scan_log_1_keeps_the_lane_plan_without_its_conditions(planner):
    (launch,) = CASES["scan_ne12_sq1"]
    assert planner.plan(launch, 1)["kernel"] == LOG
    for inputs, opts in ((dict(all_valid=0), {}), ({}, dict(batch_reflections=0)), ({}, dict(lds_ec=0))):
        p = planner.plan(launch, 1, inputs=inputs, opts=opts)
        assert p["kernel"] == LANE and p == planner.plan(launch, 0, inputs=inputs, opts=opts), (inputs, opts)
    (launch,) = CASES["scan_long_ne12"]
    assert launch["in"]["npts"] > 1024 and planner.plan(launch, 1)["kernel"] == LANE


@pytest.mark.parametrize("name", OTHERS)
def test_source_and_explicit_plans_ignore_the_field(planner, name):
    for launch in CASES[name]:
        assert planner.plan(launch, 1) == planner.plan(launch, 0) == _recorded(planner, launch), name

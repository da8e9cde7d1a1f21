"""Lanes per phase and modelled cost of the tracing waves of pc_trace_producer_kernel, on the host (phase_sim.cpp).

    python scripts/analysis/phase_sim.py                        # thresholds, strides and routing policies, 30000 slots
    python scripts/analysis/phase_sim.py --slots 5000 --quick   # the default knobs only

Needs no GPU and no libpolycap.so: phase_sim.cpp is a host compile of pc_device.h through tests/emul/pc_emul.cpp.  The problem
is xos1 at 10 keV from tests/golden/example/xos1.prf / .ext with the pinned constants (amu 42.544635, scatf 0.503696), seed
20000.  The GPU columns to compare with are the `scheduler` block of `python bench.py` (lanes per wave-phase).

The cost model weighs the counted phases with vector instructions per hot march step, first-segment block, EVENT visit and
NEW phase (--cost, default 40 90 700 150: the listing of the kernel before its march step was trimmed to 33; the ranking of
the knobs does not depend on it).  Strides other than the product's are builds of their own (-DPC_L1 / -DPC_L2)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from polycap_amd._cabi import Problem, ProblemS, dptr      # noqa: E402  (ctypes description of the problem only)

HERE = os.path.dirname(os.path.abspath(__file__))
POLICIES = ((0, "arrival order (product)"), (2, "batch sorted by kn"), (1, "kn bands"), (3, "reflection-count bands (oracle)"))


def build(tmp, strides=None):
    extra = [] if strides is None else ["-DPC_L1=%d" % strides[0], "-DPC_L2=%d" % strides[1]]
    so = os.path.join(tmp, "libphase_sim%s.so" % ("" if strides is None else "_%d_%d" % strides))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", "-mfma",
                           "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "polycap_amd", "csrc", "hip"),
                           "-o", so, os.path.join(HERE, "phase_sim.cpp")] + extra)
    L = C.CDLL(so)
    L.phase_sim_run.argtypes = [C.POINTER(ProblemS), C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.phase_sim_run.restype = C.c_int
    return L


def xos1():
    g = os.path.join(ROOT, "tests", "golden", "example")
    prf = np.loadtxt(os.path.join(g, "xos1.prf"), skiprows=1)
    ext = np.loadtxt(os.path.join(g, "xos1.ext"), skiprows=1)
    return Problem(prf[:, 0], prf[:, 1], ext[:, 1], 0.0, 200000, 2.23, [10.0], [42.544635], [0.503696], 2000.0, 0.2065, 0.2065,
                   0, 0, 0, 0, 0.0)


def run(L, prob, slots, waves, policy, et, ms, cost):
    out = np.zeros(16)
    c = np.asarray(cost, dtype=np.float64)
    r = L.phase_sim_run(C.byref(prob.s), 20000, slots, policy, waves, et, ms, dptr(c), dptr(out))
    if r:
        raise RuntimeError("phase_sim_run failed: %d" % r)
    return out


def line(name, o, base=None):
    rel = "" if base is None else "  %+5.1f %%" % (100.*(o[10] - base)/base)
    return ("%-34s MARCH %5.1f lanes x %.3e  first %5.1f  EVENT %5.1f x %.3e  NEW %4.1f x %.3e  MARCH steps/EVENT %4.1f  cost %.4e%s"
            % (name, o[2]/o[1], o[1], o[4]/max(o[3], 1), o[6]/o[5], o[5], o[8]/o[7], o[7], o[1]/o[5], o[10], rel))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=30000)
    ap.add_argument("--waves", type=int, default=15, help="tracing waves the photons are dealt to (one workgroup's)")
    ap.add_argument("--cost", type=float, nargs=4, default=[40., 90., 700., 150.])
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    prob = xos1()
    with tempfile.TemporaryDirectory(prefix="phase_sim_") as tmp:
        L = build(tmp)
        o = run(L, prob, a.slots, a.waves, 0, 48, 8, a.cost)
        base = o[10]
        print("xos1 10 keV, seed 20000, %d slots, %d entered photons, %d waves; corr(kn, reflections) %.2f" % (a.slots, o[0], a.waves, o[12]))
        print(line("defaults: event_threshold 48, march_stop 8", o))
        if a.quick:
            return
        print("thresholds:")
        for et in (32, 40, 48, 56, 60):
            for ms in (4, 8, 16):
                print(line("  event_threshold %d march_stop %d" % (et, ms), run(L, prob, a.slots, a.waves, 0, et, ms, a.cost), base))
        print("routing of entered photons to the tracing waves:")
        for pol, name in POLICIES:
            print(line("  " + name, run(L, prob, a.slots, a.waves, pol, 48, 8, a.cost), base))
        print("strides (PC_L1, PC_L2), a build each:")
        for st in ((5, 25), (4, 16), (4, 20), (3, 12), (6, 30), (5, 20), (8, 32)):
            print(line("  (%d, %d)" % st, run(build(tmp, st), prob, a.slots, a.waves, 0, 48, 8, a.cost), base))


if __name__ == "__main__":
    main()

"""Scans (pc_hip_scan_*): cost of a scan against the source runs it replaces.

    python scripts/bench_scan.py [single|grid]

single: xos1 at 10 keV, 1e6 slots, max_attempts 2^20: a one-point scan against pc_hip_transmission_run with the lane kernel
(producer=0, pool=0), alternating 5 times; kernel time of each (median, min, max) and the totals, which must be bit-identical.
grid: a 21 x 21 lateral grid (+-0.05 cm) on the uniform-illumination point source of the reference's leak tests (test ellipsoid,
source (5, 0.01, 0.01, -1, 0, 0, 0, 0)), 2e4 slots per point, max_attempts 1: one scan call against 441 one-point scan calls, each
waited for; wall time of each and started photons per second.  Run each mode as a process of its own under a time limit:
timeout -k 10 600 python scripts/bench_scan.py single"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def single(reps=5, n=1000000):
    prob = polycap_amd.problem_from_inp(INP, energies=[10.0])
    d, sx, sy = prob.source[0], prob.source[5], prob.source[6]
    t_run, t_scan = [], []
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.set_option("producer", 0)
        ctx.set_option("pool", 0)
        ctx.transmission(1, 0, 100000)                               # warm-up of both kernels
        ctx.scan(1, [[d, sx, sy]], 100000, max_attempts=1 << 20)
        for i in range(reps):
            ctx.run(7, 0, n, 1 << 20)
            t_run.append(ctx.wait())
            tot = ctx.totals(check=False)
            r = ctx.scan(7, [[d, sx, sy]], n, max_attempts=1 << 20)
            t_scan.append(r["kernel_ms"])
            assert np.array_equal(r["counters"][0], tot["counters"]) and np.array_equal(r["sumw_fixed"][0], tot["sumw_fixed"]), i
    out = dict(mode="single", slots=n, run_ms=spread(t_run), scan_ms=spread(t_scan),
               ratio_median=float(np.median(t_scan) / np.median(t_run)), bit_identical=True)
    print(json.dumps(out), flush=True)


def grid(npp=20000, side=21):
    from tests.common import make_pair
    from oracle import pyoracle
    pyoracle.build()
    _, _, prob, _ = make_pair(pyoracle, "ellip", source=(5., 0.01, 0.01, -1., 0., 0., 0., 0.))
    ax = np.linspace(-0.05, 0.05, side)
    pts = polycap_amd.scan_points(x=ax, y=ax)
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.scan(1, pts[:4], 2000)                                   # warm-up
        t0 = time.perf_counter()
        one = ctx.scan(3, pts, npp, max_attempts=1)
        t_one = time.perf_counter() - t0
        t0 = time.perf_counter()
        rows = [ctx.scan(3, pts[k:k + 1], npp, max_attempts=1) for k in range(len(pts))]
        t_many = time.perf_counter() - t0
    many = np.concatenate([r["counters"] for r in rows])
    assert np.array_equal(many, one["counters"])
    started = int(one["counters"][:, :3].sum())
    out = dict(mode="grid", points=len(pts), slots_per_point=npp, one_call_s=t_one, one_call_kernel_ms=one["kernel_ms"],
               calls_441_s=t_many, calls_441_kernel_ms_sum=float(sum(r["kernel_ms"] for r in rows)), speedup=t_many / t_one,
               started_photons_per_s_one_call=started / t_one, started_photons_per_s_441_calls=started / t_many)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "single"
    if mode == "single":
        single()
    elif mode == "grid":
        grid()
    else:
        raise SystemExit("mode must be single or grid")

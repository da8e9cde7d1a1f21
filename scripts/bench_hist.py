"""Histograms (pc_hip_hist_*, POLYCAP_HIST): cost of one add per regime against the run it reads and against the spot map that
holds the same X_AT axis.  Runs on a machine with an MI355X.

    python scripts/bench_hist.py [--photons 10000000] [--reps 7]

Cases: xos1 at 10 keV and on its 291-energy grid, 1e7 exit photons kept on the device (records, not fetched).  Axes: one N_REFL
axis of 256 bins (every entry of a wave goes to a few cells); one X_AT axis of 2048 bins over +-0.01 cm at 0.5 cm; eight mixed
axes.  Each energy count is a child process of its own under a time limit of its own, started only if the one before it ended
well.  For every (axes, regime): one warm-up add, then `reps` timed passes of reset + read (to drain the stream), add, read, as wall
time around calls that end in a stream synchronisation, minus the median time of a read alone; printed as median, minimum and
maximum.  The X_AT axis is also timed as a SpotMap of 2048 x 1 bins with a y window of +-128 cm under its default regime, on the
same data in the same process, and its bins must equal the histogram's.  Every pass must give the same sums bit for bit."""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")

X_AXIS = dict(axis="x", d=0.5, range=(-0.01, 0.01), bins=2048)
CASES = (("nrefl 256", [dict(axis="nrefl", range=(0, 256), bins=256)]),
         ("x 2048", [X_AXIS]),
         ("eight mixed", [X_AXIS, dict(axis="y", d=0.5, range=(-0.01, 0.01), bins=2048),
                          dict(axis="r", d=0.5, centre=(0., 0.), range=(0, 0.02), bins=1024),
                          dict(axis="slope_x", range=(-0.02, 0.02), bins=512), dict(axis="tan_theta", range=(0, 0.03), bins=512),
                          dict(axis="nrefl", range=(0, 256), bins=256), dict(axis="dtravel", range=(9.0, 9.001), bins=500),
                          dict(axis="r_start", range=(0, 0.25), bins=250)]))


def timed(obj, reps, keys):
    """(median, min, max) ms of one add, and the sums"""
    obj.reset()
    obj.add("exit")                     # warm-up
    ref = obj.read()
    t_read = []
    for _ in range(reps):
        t0 = time.perf_counter()
        obj.read()
        t_read.append((time.perf_counter() - t0) * 1e3)
    base = float(np.median(t_read))
    t = []
    for _ in range(reps):
        obj.reset()
        obj.read()
        t0 = time.perf_counter()
        obj.add("exit")
        r = obj.read()
        t.append((time.perf_counter() - t0) * 1e3 - base)
        assert all(np.array_equal(r[k], ref[k]) for k in keys), "sums differ between passes"
    return float(np.median(t)), min(t), max(t), ref


def child(ne, photons, reps):
    import polycap_amd
    prob = polycap_amd.problem_from_inp(INP, energies=[10.0] if ne == 1 else None)
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.run(31, 0, photons, keep_images=True)
        run_ms = ctx.wait()
        print("xos1, %d energies, %d exit photons: run kernel %.1f ms" % (prob.n_energies, photons, run_ms), flush=True)
        with polycap_amd.SpotMap(ctx, [0.5], (-0.01, 0.01, -128., 128.), (2048, 1)) as m:
            s_med, s_min, s_max, spot = timed(m, reps, ("bins", "outside"))
        print("  spot map 2048 x 1 (%s): add %.3f ms median (%.3f .. %.3f)" % ("energies across lanes" if m.wide else "LDS tiles", s_med, s_min, s_max), flush=True)
        for label, axes in CASES:
            for regime in (1, 2, 0):
                with polycap_amd.Histograms(ctx, axes, regime=regime) as h:
                    med, lo, hi, res = timed(h, reps, ("bins", "outside"))
                    used = h.regime
                print("  %-12s regime %d%s: add %.3f ms median (%.3f .. %.3f) = %.2f %% of the run" % (
                    label, used, " (default)" if regime == 0 else "", med, lo, hi, 100. * med / run_ms), flush=True)
                if label == "x 2048":
                    assert np.array_equal(res["bins"][0], spot["bins"][0, :, 0, :]) and np.array_equal(res["outside"][0, 0], spot["outside"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", type=int, default=0, help="run one energy count in this process (1 or 291)")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to each child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.photons, a.reps)
        return 0
    for ne in (1, 291):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(ne),
               "--photons", str(a.photons), "--reps", str(a.reps)]
        rc = subprocess.call(cmd)
        if rc != 0:          # a fault, an abort or a time limit: nothing more is started on the device
            print("bench_hist: the %d-energy case ended with status %d; stopping" % (ne, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

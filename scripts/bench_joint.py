"""Joint histograms (pc_hip_joint_*, POLYCAP_JOINT): cost of one add per regime, the pair (X_AT, Y_AT) next to the spot-map add of
the same shape in the same process.  Runs on a machine with an MI355X.

    python scripts/bench_joint.py [--photons 10000000] [--reps 11] [--out profiles/joint_ab.txt]

Cases: xos1 at 10 keV and on its 291-energy grid, 1e7 exit photons kept on the device (records, not fetched).  At 10 keV the pair
(x, y) at 0.5 cm over +-0.02 cm at 256^2 and at 1024^2 cells; at 291 energies the same pair at 64^2; at both the four pairs
(x, slope_x), (start_x, start_y), (r_start, nrefl), (r, tan_theta) of tests/test_gpu_joint.py.  Each energy count is a child process
of its own under a time limit of its own, started only if the one before it ended well.  For every (pairs, regime): one warm-up add,
then `reps` timed passes of reset + read (to drain the stream), add, read, as wall time around calls that end in a stream
synchronisation, minus the median time of a read alone; printed as median, minimum and maximum.  A regime whose warm-up add takes
longer than --skip-ms is timed once.  The spot-shaped pairs are also timed as a SpotMap in both of its regimes on the same data, and
their cells must equal the map's.  Every pass must give the same sums bit for bit.  The lines are also appended to --out."""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")
WINDOW = (-0.02, 0.02, -0.02, 0.02)


def xy(n):
    return [(dict(axis="x", d=0.5, range=WINDOW[:2], bins=n), dict(axis="y", d=0.5, range=WINDOW[2:], bins=n))]


FOUR = [(dict(axis="x", d=0.5, range=(-0.01, 0.01), bins=33), dict(axis="slope_x", range=(-0.005, 0.005), bins=31)),
        (dict(axis="start_x", range=(-0.3, 0.3), bins=24), dict(axis="start_y", range=(-0.3, 0.3), bins=20)),
        (dict(axis="r_start", range=(0., 0.3), bins=47), dict(axis="nrefl", range=(0, 256), bins=256)),
        (dict(axis="r", d=0.25, centre=(0.002, -0.001), range=(0., 0.02), bins=19), dict(axis="tan_theta", range=(0., 0.01), bins=21))]


def timed(obj, reps, keys, skip_ms):
    """(median, min, max) ms of one add, the number of timed passes, and the sums"""
    obj.reset()
    obj.read()
    t0 = time.perf_counter()
    obj.add("exit")                     # warm-up
    ref = obj.read()
    warm = (time.perf_counter() - t0) * 1e3
    t_read = []
    for _ in range(reps):
        t0 = time.perf_counter()
        obj.read()
        t_read.append((time.perf_counter() - t0) * 1e3)
    base = float(np.median(t_read))
    n = reps if warm < skip_ms else 1
    t = []
    for _ in range(n):
        obj.reset()
        obj.read()
        t0 = time.perf_counter()
        obj.add("exit")
        r = obj.read()
        t.append((time.perf_counter() - t0) * 1e3 - base)
        assert all(np.array_equal(r[k], ref[k]) for k in keys), "sums differ between passes"
    return float(np.median(t)), min(t), max(t), n, ref


def child(ne, photons, reps, skip_ms, out):
    import polycap_amd
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    prob = polycap_amd.problem_from_inp(INP, energies=[10.0] if ne == 1 else None)
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.run(31, 0, photons, keep_images=True)
        run_ms = ctx.wait()
        say("xos1, %d energies, %d exit photons: run kernel %.1f ms" % (prob.n_energies, photons, run_ms))
        for n in ((256, 1024) if ne == 1 else (64,)):
            spot_ms = {}
            for regime in (1, 2):
                with polycap_amd.SpotMap(ctx, [0.5], WINDOW, (n, n), regime=regime) as m:
                    med, lo, hi, k, spot = timed(m, reps, ("bins", "outside"), skip_ms)
                spot_ms[regime] = med
                say("  spot map %4d^2 regime %d: add %9.3f ms median of %2d (%.3f .. %.3f)" % (n, regime, med, k, lo, hi))
            for regime in (1, 2, 0):
                with polycap_amd.JointHistograms(ctx, xy(n), regime=regime) as h:
                    med, lo, hi, k, res = timed(h, reps, ("cells", "outside"), skip_ms)
                    used = h.regime
                assert np.array_equal(res["pairs"][0][0], spot["bins"][0]) and np.array_equal(res["outside"][0, 0], spot["outside"][0])
                say("  joint (x, y) %4d^2 regime %d%s: add %9.3f ms median of %2d (%.3f .. %.3f) = %.2f x the spot add of regime %d, %.2f x its faster one" % (
                    n, used, " (automatic)" if regime == 0 else "", med, k, lo, hi, med / spot_ms[used], used, med / min(spot_ms.values())))
        for regime in (1, 2, 0):
            with polycap_amd.JointHistograms(ctx, FOUR, regime=regime) as h:
                med, lo, hi, k, res = timed(h, reps, ("cells", "outside"), skip_ms)
                used = h.regime
            say("  joint four pairs   regime %d%s: add %9.3f ms median of %2d (%.3f .. %.3f) = %.2f %% of the run" % (
                used, " (automatic)" if regime == 0 else "", med, k, lo, hi, 100. * med / run_ms))
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--skip-ms", type=float, default=500., help="a regime whose warm-up add takes longer is timed once")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_ab.txt"))
    ap.add_argument("--child", type=int, default=0, help="run one energy count in this process (1 or 291)")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to each child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.photons, a.reps, a.skip_ms, a.out)
        return 0
    if a.out:
        with open(a.out, "w") as f:
            f.write("scripts/bench_joint.py --photons %d --reps %d: ms per add, median (minimum .. maximum) of the timed passes\n" % (a.photons, a.reps))
    for ne in (1, 291):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(ne),
               "--photons", str(a.photons), "--reps", str(a.reps), "--skip-ms", str(a.skip_ms), "--out", a.out]
        rc = subprocess.call(cmd)
        if rc != 0:          # a fault, an abort or a time limit: nothing more is started on the device
            print("bench_joint: the %d-energy case ended with status %d; stopping" % (ne, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Draws (pc_hip_select_draw): an unweighted sample of the exit beam made on the GPU, against the only way to one without it --
fetching every record and resampling in numpy.  Runs on a machine with an MI355X.

    python scripts/bench_draw.py [--photons 10000000] [--reps 5] [--out profiles/draw_ab.txt]

Workload: xos1 at 10 keV, 1e7 exit photons kept on the device as records.  Samples of 1e5 and of 1e6 photons through the selection
that every photon passes (polycap_amd.select_all()) and through the cut on r at d = 0.5 cm, [0, R), whose radius R is the 1 % weight
quantile of a histogram of r of the same run (the 0.65 % cut of profiles/gather_ab.txt: 1 % of the weight, 0.65 % of the entries).
For each, in one process and interleaved pass by pass after one warm-up of each:
  draw        Selection.apply + Selection.draw of the whole sample, into a fresh array: wall time
  full fetch  TraceContext.records() of the whole run into a fresh array, the mask of the cut in numpy, the weights quantised as the
              device quantises them, numpy's cumsum, searchsorted of the thresholds and the rows by fancy indexing: wall time.  The
              thresholds t_k need 128-bit products, which numpy does not have: they are computed once outside the timed part and
              handed to both passes, so the full fetch is not charged for them
Medians of `reps` passes with minimum and maximum; rows, bytes copied to the host.  Every pass of the draw must give the same rows bit
for bit, and the numpy path's rows must be the draw's wherever its mask is the device's.  The table goes to --out and to stdout.
The child runs under a time limit."""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")
D = 0.5
PHASE = 123456789
SIZES = (100_000, 1_000_000)


def stats(t):
    return float(np.median(t)), min(t), max(t)


def numpy_mask(rec, zp, radius):
    """the rows whose r at the plane zp is in [0, radius): exit photons carry the x and y components of their direction"""
    x, y, z, dx, dy = rec[:, 8], rec[:, 9], rec[:, 10], rec[:, 11], rec[:, 12]
    dz = np.sqrt((1. - dx * dx) - dy * dy)
    t = (zp - z) / dz
    r = np.hypot(x + dx * t, y + dy * t)
    return (dz > 0.) & (r / radius < 1.)


def numpy_draw(rec, mask, thresholds):
    """what a caller without the draw does: quantise, mask, cumulate, search, index"""
    v = rec[:, 17] * 4294967296.0
    V = np.where(v > 0., np.rint(v), 0.).astype(np.uint64)
    if mask is not None:
        V[~mask] = 0
    pos = np.searchsorted(np.cumsum(V, dtype=np.uint64), thresholds, side="right")
    return rec[pos]


def thresholds(T, N, phase):
    """t_k = floor((k 2^32 + r) T / (N 2^32)) in Python integers"""
    den = N << 32
    return np.array([((k << 32) + phase) * T // den for k in range(N)], dtype=np.uint64)


def child(photons, reps, out):
    import polycap_amd as pa
    prob = pa.problem_from_inp(INP, energies=[10.0])
    zp = float(prob.z[-1]) + D
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with pa.TraceContext(prob) as ctx:
        ctx.run(31, 0, photons, keep_images=True)
        run_ms = ctx.wait()
        say("xos1, 10 keV, %d exit photons kept as records on the device; trace kernel %.1f ms; rows of %d doubles"
            % (photons, run_ms, 17 + prob.n_energies))
        with pa.Histograms(ctx, [dict(axis="r", d=D, range=(0., 0.05), bins=16384)]) as h:
            h.add("exit")
            radius = float(h.quantile(0, 0, 0.01))
        say("%-10s %-8s %-11s %-34s %-10s %-12s" % ("selection", "sample", "path", "ms median (min .. max)", "entries", "bytes moved"))
        row_bytes = 8 * (17 + prob.n_energies)
        for name, cuts in (("all", pa.select_all()), ("r, 1 %", [dict(axis="r", d=D, range=(0., radius))])):
            with pa.Selection(ctx, cuts) as sel:
                res = sel.apply("exit")
                n_pass, T = int(res["n_pass"][0]), int(res["passed_w"][0][0])
                for N in SIZES:
                    tk = thresholds(T, N, PHASE)
                    ref = sel.draw("exit", energy=0, n=N, phase=PHASE)["records"]              # warm-up of the draw
                    rec = ctx.records()                                                          # and of the full fetch
                    full = numpy_draw(rec, None if name == "all" else numpy_mask(rec, zp, radius), tk)
                    del rec
                    t_d, t_f = [], []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        sel.apply("exit")
                        rows = sel.draw("exit", energy=0, n=N, phase=PHASE)["records"]
                        t_d.append((time.perf_counter() - t0) * 1e3)
                        assert np.array_equal(rows.view(np.uint64), ref.view(np.uint64)), "the drawn rows differ between passes"
                        t0 = time.perf_counter()
                        rec = ctx.records()
                        mask = None if name == "all" else numpy_mask(rec, zp, radius)
                        full = numpy_draw(rec, mask, tk)
                        t_f.append((time.perf_counter() - t0) * 1e3)
                        same_mask = mask is None or int(mask.sum()) == n_pass
                        del rec, mask
                    if same_mask:
                        assert np.array_equal(full.view(np.uint64), ref.view(np.uint64)), "numpy's rows differ from the drawn ones"
                    (dm, dlo, dhi), (fm, flo, fhi) = stats(t_d), stats(t_f)
                    say("%-10s %-8d %-11s %-34s %-10d %-12d" % (name, N, "draw", "%.2f (%.2f .. %.2f)" % (dm, dlo, dhi), n_pass, N * row_bytes))
                    say("%-10s %-8d %-11s %-34s %-10d %-12d" % (name, N, "full fetch", "%.2f (%.2f .. %.2f)" % (fm, flo, fhi), n_pass, photons * row_bytes))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_ab.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to the measuring process")
    a = ap.parse_args()
    if a.child:
        child(a.photons, a.reps, a.out)
        return 0
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--photons", str(a.photons),
           "--reps", str(a.reps), "--out", a.out]
    rc = subprocess.call(cmd)
    if rc != 0:
        print("bench_draw: the measuring process ended with status %d" % rc, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())

"""Gathers (pc_hip_select_gather): fetching only the photons a selection keeps, against fetching every record and filtering in numpy.
Runs on a machine with an MI355X.

    python scripts/bench_gather.py [--photons 10000000] [--reps 7] [--out profiles/gather_ab.txt]

Workload: xos1 at 10 keV, 1e7 exit photons kept on the device as records.  Cuts on r at d = 0.5 cm, [0, R), whose radii R are read
from a histogram of r of the same run (weighted, as every histogram here) at its 0.1 %, 1 %, 10 % and 50 % quantiles: that share of
the weight passes, and a somewhat smaller share of the entries, which the rows column states.
For each cut, in one process and interleaved pass by pass after one warm-up of each:
  gather      Selection.apply + Selection.gather of everything that passes, into a fresh array: wall time
  full fetch  TraceContext.records() of the whole run into a fresh array, and the filter in numpy (r from the record's fields,
              then the rows of the mask): wall time.  This is the only way to the selected photons without the gather
Medians of `reps` passes with minimum and maximum; rows, bytes copied to the host and the rate those bytes make in the median time.
Every pass of the gather must give the same rows bit for bit, and where numpy's r (not the device's operation order) passes the
same number of entries its rows must be the gather's.  The table goes to --out and to stdout.  The child runs under a time limit."""
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
QUANTILES = (0.001, 0.01, 0.1, 0.5)


def stats(t):
    return float(np.median(t)), min(t), max(t)


def numpy_filter(rec, zp, radius):
    """the rows whose r at the plane zp is in [0, radius): exit photons carry the x and y components of their direction"""
    x, y, z, dx, dy = rec[:, 8], rec[:, 9], rec[:, 10], rec[:, 11], rec[:, 12]
    dz = np.sqrt((1. - dx * dx) - dy * dy)
    t = (zp - z) / dz
    r = np.hypot(x + dx * t, y + dy * t)
    return rec[(dz > 0.) & (r / radius < 1.)]


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
            radii = [float(h.quantile(0, 0, q)) for q in QUANTILES]
        say("%-8s %-11s %-34s %-10s %-12s %-9s" % ("quantile", "path", "ms median (min .. max)", "rows", "bytes moved", "GB/s"))
        row_bytes = 8 * (17 + prob.n_energies)
        for q, radius in zip(QUANTILES, radii):
            with pa.Selection(ctx, [dict(axis="r", d=D, range=(0., radius))]) as sel:
                sel.apply("exit")
                ref = sel.gather("exit")                      # warm-up of the gather
                full = numpy_filter(ctx.records(), zp, radius)      # and of the full fetch
                t_g, t_f = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    sel.apply("exit")
                    rows = sel.gather("exit")
                    t_g.append((time.perf_counter() - t0) * 1e3)
                    assert np.array_equal(rows.view(np.uint64), ref.view(np.uint64)), "the gathered rows differ between passes"
                    t0 = time.perf_counter()
                    full = numpy_filter(ctx.records(), zp, radius)
                    t_f.append((time.perf_counter() - t0) * 1e3)
                if len(full) == len(ref):
                    assert np.array_equal(full.view(np.uint64), ref.view(np.uint64)), "numpy's rows differ from the gathered ones"
                (gm, glo, ghi), (fm, flo, fhi) = stats(t_g), stats(t_f)
                gb, fb = len(ref) * row_bytes, photons * row_bytes
                say("%-8g %-11s %-34s %-10d %-12d %-9.2f" % (q, "gather", "%.2f (%.2f .. %.2f)" % (gm, glo, ghi), len(ref), gb, gb / (gm * 1e6)))
                say("%-8g %-11s %-34s %-10d %-12d %-9.2f" % (q, "full fetch", "%.2f (%.2f .. %.2f)" % (fm, flo, fhi), len(full), fb, fb / (fm * 1e6)))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_ab.txt"))
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
        print("bench_gather: the measuring process ended with status %d" % rc, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())

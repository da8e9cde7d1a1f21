"""Selections (pc_hip_select_*): cost of one apply, and of a gated add next to the plain add of the same tally.  Runs on a machine with
an MI355X.

    python scripts/bench_select.py [--photons 10000000] [--reps 7]

Cases: xos1 at 10 keV and on its 291-energy grid, 1e7 exit photons kept on the device (records, not fetched).  The selection is the
pinhole of INTEGRATION.md section 11 (r at 0.5 cm within 50 um, and not fewer than 40 reflections).  Each energy count is a child
process of its own under a time limit of its own, started only if the one before it ended well.  Apply: one warm-up, then `reps`
timed passes as wall time around apply + read (which ends in a stream synchronisation), minus the median time of a read alone;
beside it the bytes the pass has to read (per entry the fields its cuts use and every weight, and the mask byte it writes) and the
time a bare read of them takes at --hbm-gbs (default 4000: a placeholder, not a measurement; give the rate a streaming read achieves
on the box, measured there).
Adds: for a spot map, beam moments, histograms and joint histograms, `reps` passes each of reset + read, add, read for the plain and
for the gated add, as median, minimum and maximum.  Every pass must give the same sums bit for bit, and the gated sums of the
selection and of its complement must add up to the plain ones."""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")
CUTS = [dict(axis="r", d=0.5, range=(0, 0.005)), {"axis": "nrefl", "range": (0, 40), "not": True}]
X_AXIS = dict(axis="x", d=0.5, range=(-0.01, 0.01), bins=2048)


def stats(t):
    return float(np.median(t)), min(t), max(t)


def timed_apply(sel, reps):
    ref = sel.apply("exit")
    t_read = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sel.read()
        t_read.append((time.perf_counter() - t0) * 1e3)
    base = float(np.median(t_read))
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = sel.apply("exit")
        t.append((time.perf_counter() - t0) * 1e3 - base)
        assert all(np.array_equal(r[k], ref[k]) for k in ref), "totals differ between passes"
    return stats(t), ref


def timed_add(obj, reps, keys, select=None):
    obj.reset()
    obj.add("exit", select=select)          # warm-up
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
        obj.add("exit", select=select)
        r = obj.read()
        t.append((time.perf_counter() - t0) * 1e3 - base)
        assert all(np.array_equal(r[k], ref[k]) for k in keys), "sums differ between passes"
    return stats(t), ref


def child(ne, photons, reps, hbm_gbs):
    import polycap_amd as pa
    prob = pa.problem_from_inp(INP, energies=[10.0] if ne == 1 else None)
    with pa.TraceContext(prob) as ctx:
        ctx.run(31, 0, photons, keep_images=True)
        run_ms = ctx.wait()
        print("xos1, %d energies, %d exit photons: run kernel %.1f ms" % (prob.n_energies, photons, run_ms), flush=True)
        comp = [CUTS[0], dict(CUTS[1], **{"not": False})]          # the complement in the second cut, given the first
        with pa.Selection(ctx, CUTS) as sel, pa.Selection(ctx, comp) as sel_c:
            (med, lo, hi), tot = timed_apply(sel, reps)
            sel_c.apply("exit")
            # x, y, z, dx, dy (r at a distance), the reflection count, every weight; one mask byte written
            nbytes = photons * (8 * (6 + prob.n_energies) + 1)
            print("  apply: %.3f ms median (%.3f .. %.3f); %d of %d pass; %.1f MB to touch = %.3f ms at %.0f GB/s" % (
                med, lo, hi, tot["n_pass"][0], tot["n_seen"][0], nbytes / 1e6, nbytes / (hbm_gbs * 1e6), hbm_gbs), flush=True)
            makers = (("spot map 256^2", lambda: pa.SpotMap(ctx, [0.5], (-0.01, 0.01, -0.01, 0.01), (256, 256)), ("bins", "outside")),
                      ("beam moments", lambda: pa.BeamMoments(ctx), ("sums", "outside")),
                      ("hist x 2048", lambda: pa.Histograms(ctx, [X_AXIS]), ("bins", "outside")),
                      ("joint x*slope_x 256^2", lambda: pa.JointHistograms(ctx, [(dict(X_AXIS, bins=256), dict(axis="slope_x", range=(-0.005, 0.005), bins=256))]),
                       ("cells", "outside")))
            for label, make, keys in makers:
                with make() as obj:
                    plain_t, plain = timed_add(obj, reps, keys)
                    gated_t, gated = timed_add(obj, reps, keys, select=sel)
                    if label != "beam moments":          # 128-bit sums: the tests add those
                        obj.add("exit", select=sel_c)
                        both = obj.read()
                        first = dict(axis="r", d=0.5, range=(0, 0.005))
                        with pa.Selection(ctx, [first]) as s1:
                            s1.apply("exit")
                            obj.reset()
                            obj.add("exit", select=s1)
                            want = obj.read()
                        assert all(np.array_equal(both[k], want[k]) for k in keys), "the selection and its complement do not add up"
                print("  %-22s plain add %.3f ms median (%.3f .. %.3f); gated add %.3f ms median (%.3f .. %.3f)" % ((label,) + plain_t + gated_t), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=4000.)
    ap.add_argument("--child", type=int, default=0, help="run one energy count in this process (1 or 291)")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed to each child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.photons, a.reps, a.hbm_gbs)
        return 0
    for ne in (1, 291):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(ne),
               "--photons", str(a.photons), "--reps", str(a.reps), "--hbm-gbs", str(a.hbm_gbs)]
        rc = subprocess.call(cmd)
        if rc != 0:          # a fault, an abort or a time limit: nothing more is started on the device
            print("bench_select: the %d-energy case ended with status %d; stopping" % (ne, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

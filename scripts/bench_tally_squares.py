"""Squared-weight sums of the tallies (pc_hip_*_track_squares): what the plain add costs now against the parent commit, and what the
add that tracks squares costs against the plain one.  Runs on a machine with an MI355X.

    python scripts/bench_tally_squares.py [--parent DIR] [--photons 10000000] [--reps 7] [--rounds 2]

Sizes: those of scripts/bench_hist.py (one N_REFL axis of 256 bins, one X_AT axis of 2048 bins, eight mixed axes), scripts/bench_joint.py
((X_AT, Y_AT) at 256^2 at one energy, 64^2 at 291) and scripts/bench_select.py (the pinhole's apply, a spot map of 256^2); xos1 at
10 keV and on its 291-energy grid, 1e7 exit photons kept on the device.  --parent is a built checkout of the parent commit: its
polycap_amd is imported instead of this tree's and only the plain adds are timed.  The trees alternate, `rounds` times, each (tree,
energy count) a child process of its own under a time limit of its own, started only if the one before it ended well; the spread of
the parent's medians between rounds is the yardstick for the plain add of this tree.  Timing as in bench_hist.py: one warm-up add,
then `reps` passes of reset + read, add, read as wall time around calls that end in a stream synchronisation, minus the median time
of a read alone.  Every pass must give the same sums bit for bit, and the tracking object's weight sums must equal the plain one's."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_AXIS = dict(axis="x", d=0.5, range=(-0.01, 0.01), bins=2048)
EIGHT = [X_AXIS, dict(axis="y", d=0.5, range=(-0.01, 0.01), bins=2048), dict(axis="r", d=0.5, centre=(0., 0.), range=(0, 0.02), bins=1024),
         dict(axis="slope_x", range=(-0.02, 0.02), bins=512), dict(axis="tan_theta", range=(0, 0.03), bins=512),
         dict(axis="nrefl", range=(0, 256), bins=256), dict(axis="dtravel", range=(9.0, 9.001), bins=500), dict(axis="r_start", range=(0, 0.25), bins=250)]
CUTS = [dict(axis="r", d=0.5, range=(0, 0.005)), {"axis": "nrefl", "range": (0, 40), "not": True}]


def timed(np, obj, reps, keys, fn):
    """(median, min, max) ms of fn(), and what read() gives after it"""
    if hasattr(obj, "reset"):
        obj.reset()
    fn()                                # warm-up
    ref = obj.read()
    t_read = []
    for _ in range(reps):
        t0 = time.perf_counter()
        obj.read()
        t_read.append((time.perf_counter() - t0) * 1e3)
    base = float(np.median(t_read))
    t = []
    for _ in range(reps):
        if hasattr(obj, "reset"):
            obj.reset()
        obj.read()
        t0 = time.perf_counter()
        fn()
        r = obj.read()
        t.append((time.perf_counter() - t0) * 1e3 - base)
        assert all(np.array_equal(r[k], ref[k]) for k in keys), "sums differ between passes"
    return (float(np.median(t)), min(t), max(t)), ref


def child(tree, ne, photons, reps):
    sys.path.insert(0, tree)
    import numpy as np
    import polycap_amd as pa
    assert os.path.abspath(os.path.dirname(os.path.dirname(pa.__file__))) == os.path.abspath(tree)
    squares = hasattr(pa, "tally_stderr")
    prob = pa.problem_from_inp(os.path.join(tree, "tests", "golden", "example", "xos1.inp"), energies=[10.0] if ne == 1 else None)
    n2 = 256 if ne == 1 else 64
    pair = [(dict(X_AXIS, bins=n2), dict(axis="y", d=0.5, range=(-0.01, 0.01), bins=n2))]
    regimes = (1, 2) if ne == 1 else (2,)          # regime 1 at 291 energies is one pass over the entries per tile: not a size anyone runs
    makers = [("hist nrefl 256 r%d" % r, lambda r=r, **kw: pa.Histograms(ctx, [dict(axis="nrefl", range=(0, 256), bins=256)], regime=r, **kw), "bins") for r in regimes]
    makers += [("hist x 2048 r%d" % r, lambda r=r, **kw: pa.Histograms(ctx, [X_AXIS], regime=r, **kw), "bins") for r in regimes]
    makers += [("hist eight mixed r2", lambda **kw: pa.Histograms(ctx, EIGHT, regime=2, **kw), "bins")]
    makers += [("joint %d^2 r2" % n2, lambda **kw: pa.JointHistograms(ctx, pair, regime=2, **kw), "cells")]
    makers += [("spot %d^2" % n2, lambda **kw: pa.SpotMap(ctx, [0.5], (-0.01, 0.01, -0.01, 0.01), (n2, n2), **kw), "bins")]
    with pa.TraceContext(prob) as ctx:
        ctx.run(31, 0, photons, keep_images=True)
        run_ms = ctx.wait()
        print("tree %s (%s), %d energies, %d exit photons: run kernel %.1f ms" % (tree, "this commit" if squares else "parent", prob.n_energies, photons, run_ms), flush=True)
        for label, make, key in makers:
            with make() as obj:
                plain_t, plain = timed(np, obj, reps, (key, "outside"), lambda: obj.add("exit"))
            line = "  %-20s plain add %8.3f ms median (%8.3f .. %8.3f)" % ((label,) + plain_t)
            if squares:
                with make(squares=True) as obj:
                    sq_t, sq = timed(np, obj, reps, (key, "outside", "squares", "outside_squares"), lambda: obj.add("exit"))
                assert np.array_equal(sq[key], plain[key]) and np.array_equal(sq["outside"], plain["outside"]), "tracking changed the weight sums"
                line += "; squares add %8.3f ms median (%8.3f .. %8.3f) = %.2f x" % (sq_t + (sq_t[0] / plain_t[0],))
            print(line, flush=True)
        with pa.Selection(ctx, CUTS) as sel:
            plain_t, plain = timed(np, sel, reps, ("passed_w", "rejected_w"), lambda: sel.apply("exit"))
        line = "  %-20s plain     %8.3f ms median (%8.3f .. %8.3f)" % (("select apply",) + plain_t)
        if squares:
            with pa.Selection(ctx, CUTS, squares=True) as sel:
                sq_t, sq = timed(np, sel, reps, ("passed_w", "rejected_w", "passed_w2", "rejected_w2"), lambda: sel.apply("exit"))
            assert np.array_equal(sq["passed_w"], plain["passed_w"]) and np.array_equal(sq["rejected_w"], plain["rejected_w"])
            line += "; squares     %8.3f ms median (%8.3f .. %8.3f) = %.2f x" % (sq_t + (sq_t[0] / plain_t[0],))
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; without it only this tree is timed")
    ap.add_argument("--photons", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--energies", default="1,291")
    ap.add_argument("--child", default=None, help="run one (tree, energy count) in this process: TREE:NE")
    ap.add_argument("--limit", type=int, default=300, help="seconds allowed to each child")
    a = ap.parse_args()
    if a.child:
        tree, ne = a.child.rsplit(":", 1)
        child(tree, int(ne), a.photons, a.reps)
        return 0
    trees = ([os.path.abspath(a.parent)] if a.parent else []) + [ROOT]
    for rnd in range(a.rounds):
        for ne in (int(v) for v in a.energies.split(",")):
            for tree in trees:
                print("round %d" % rnd, flush=True)
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "%s:%d" % (tree, ne),
                       "--photons", str(a.photons), "--reps", str(a.reps)]
                rc = subprocess.call(cmd, cwd=tree)
                if rc != 0:          # a fault, an abort or a time limit: nothing more is started on the device
                    print("bench_tally_squares: %s at %d energies ended with status %d; stopping" % (tree, ne, rc), flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

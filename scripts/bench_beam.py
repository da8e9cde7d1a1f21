"""Exit-beam moments (pc_hip_beam_*, POLYCAP_BEAM): cost of the beam pass against the run it reads.

    timeout -k 10 600 python scripts/bench_beam.py

Cases: xos1 at 10 keV with 1e7 exit photons kept on the device (images, not fetched); xos1 on its 291-energy grid with 1e6 slots;
a leak_calc run of 262144 slots at 10 and 20 keV (exit photons, extleak and intleak added).  For each case: the run's kernel time
(ctx.wait), then 5 timed passes of reset + add + read after one warm-up, as wall time around calls that end in a stream
synchronisation, minus the median time of a read alone (the copy of the sums and the synchronisation), as median (min .. max).
For the kernel time alone run the script under rocprofv3 --kernel-trace --stats (pc_beam_kernel).  Every pass must give the same
sums bit for bit."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")


def timed(b, kinds, reps=5):
    b.reset()
    for k in kinds:
        b.add(k)
    ref = b.read()
    t_read = []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.read()
        t_read.append((time.perf_counter() - t0) * 1e3)
    t_pass = []
    for _ in range(reps):
        b.reset()
        b.read()
        t0 = time.perf_counter()
        for k in kinds:
            b.add(k)
        r = b.read()
        t_pass.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(r["sums"], ref["sums"]) and np.array_equal(r["outside"], ref["outside"]), "sums differ between passes"
        assert np.array_equal(r["n_entries"], ref["n_entries"])
    base = np.median(t_read)
    return np.median(t_pass) - base, min(t_pass) - base, max(t_pass) - base, ref


def main():
    cases = (("xos1 10 keV, 1e7 exit photons", [10.0], 10_000_000, False, ("exit",)),
             ("xos1 291 energies, 1e6 slots", None, 1_000_000, False, ("exit",)),
             ("leak run, 262144 slots, 2 energies", [10.0, 20.0], 262_144, True, ("exit", "extleak", "intleak")))
    for label, energies, n, leak, kinds in cases:
        prob = polycap_amd.problem_from_inp(INP, energies=energies)
        with polycap_amd.TraceContext(prob) as ctx:
            ctx.run(31, 0, n, keep_images=True, leak_calc=leak)
            run_ms = ctx.wait()
            kern = ctx.last_kernel()
            with polycap_amd.BeamMoments(ctx) as b:
                med, best, worst, ref = timed(b, kinds)
            p = polycap_amd.beam_params(ref["sums"][0])
        share = 100.0 * med / run_ms
        print("%s: run kernel %.2f ms (%s), beam pass %.3f ms median (%.3f .. %.3f) = %.2f %% of the run; entries %s; bit-identical "
              "over 6 passes" % (label, run_ms, kern, med, best, worst, share,
                                 ref["n_entries"].tolist()), flush=True)
        e = 0 if energies is not None else int(np.argmin(np.abs(np.asarray(prob.energies) - 10.0)))
        print("    at %.2f keV: waist_r %.4f cm, size_waist_r %.3e cm, size_exit_r %.3e cm, div_x %.3e rad" % (
            prob.energies[e], p["waist_r"][e], p["size_waist_r"][e], p["size_exit_r"][e], p["div_x"][e]), flush=True)


if __name__ == "__main__":
    main()

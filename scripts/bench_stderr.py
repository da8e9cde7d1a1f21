"""Standard errors (option "weight_squares", POLYCAP_STDERR): cost of summing the squared exit weights, off against on.

    python scripts/bench_stderr.py [kernel|api]

kernel: the headline run (xos1 at 10 keV, 1e7 slots, histogram only) and sweep_291 (xos1 on its 291-energy grid, 1e6 slots, histogram
only): kernel time of 5 runs with the option off and 5 with it on, interleaved, after one warm-up run of each.  api: the public call at
10 keV with 1e7 photons and POLYCAP_IMAGES=0, POLYCAP_STDERR unset against POLYCAP_STDERR=1.  Run each mode as a process of its own
under a time limit: timeout -k 10 600 python scripts/bench_stderr.py kernel"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")


def kernel():
    for label, energies, n in (("headline, 10 keV", [10.0], 10_000_000), ("sweep_291", None, 1_000_000)):
        prob = polycap_amd.problem_from_inp(INP, energies=energies)
        with polycap_amd.TraceContext(prob) as ctx:
            ms = {0: [], 1: []}
            for rep in range(6):
                for on in (0, 1):
                    ctx.set_option("weight_squares", on)
                    ctx.run(20000 + rep, 0, n, keep_images=False)
                    t = ctx.wait()
                    if rep > 0:
                        ms[on].append(t)
            kern = ctx.last_kernel()
            print("%s (%s), %d slots: off %s ms (best %.2f), on %s ms (best %.2f), on/off of the medians %.4f" % (
                label, kern, n, " ".join("%.2f" % t for t in ms[0]), min(ms[0]), " ".join("%.2f" % t for t in ms[1]), min(ms[1]),
                np.median(ms[1]) / np.median(ms[0])), flush=True)


def api():
    from polycap_amd import capi
    src0 = capi.Source.new_from_file(INP)
    desc = capi.Description(None, 0, 0, None, 0, _handle=capi._lib().polycap_source_get_description(src0._h), _owner=src0)
    src = capi.Source(desc, 2000., 0.2065, 0.2065, 0., 0., 0., 0., 0., np.array([10.0]))
    os.environ["POLYCAP_SEED"] = "11"
    os.environ["POLYCAP_IMAGES"] = "0"
    n = 10_000_000
    src.get_transmission_efficiencies(-1, 100000)
    ts = {"unset": [], "1": []}
    for _ in range(5):
        for v in ("unset", "1"):
            if v == "unset":
                os.environ.pop("POLYCAP_STDERR", None)
            else:
                os.environ["POLYCAP_STDERR"] = v
            t0 = time.perf_counter()
            eff = src.get_transmission_efficiencies(-1, n)
            ts[v].append((time.perf_counter() - t0) * 1e3)
            if v == "1":
                se = eff.efficiency_stderr()
            del eff
    for v in ("unset", "1"):
        print("public call, %d photons, POLYCAP_IMAGES=0, POLYCAP_STDERR %s: %s ms (best %.1f)" % (
            n, v, " ".join("%.1f" % t for t in ts[v]), min(ts[v])), flush=True)
    print("standard error at 10 keV: %.3e" % se[0], flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    (kernel if mode == "kernel" else api)()

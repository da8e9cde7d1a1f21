"""Spot maps (pc_hip_spot_*): cost of the map kernel alone and of the public call that makes one.

    python scripts/bench_spot.py [kernel|api] [slots]

kernel: xos1 at 10 keV, 1e7 exit photons kept on the device, maps of 128^2 and 1024^2 in both accumulation regimes (LDS tiles,
energies across lanes); then 291 energies x 64^2 (all energies of the deck) in both regimes.  api: the public call at 10 keV with
POLYCAP_IMAGES=0 POLYCAP_SPOT=... against POLYCAP_IMAGES=1 without maps (every plane copied back).  Run each mode as a process of
its own under a time limit: timeout -k 10 600 python scripts/bench_spot.py kernel"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")
WIN = (-0.02, 0.02, -0.02, 0.02)


def time_add(ctx, m, reps=5):
    """one add, enqueue to the end of its kernel, `reps` times after a warm-up: "median (min .. max)" in ms"""
    m.add("exit")
    m.reset()
    ctx.device_synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.add("exit")
        ctx.device_synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return "%.3f ms per add median (%.3f .. %.3f)" % (float(np.median(t)), min(t), max(t))


def kernel(n):
    prob = polycap_amd.problem_from_inp(INP, energies=[10.0])
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.transmission(1, 0, n, keep_images=False)
        ctx.run(7, 0, n, keep_images=True)
        ms = ctx.wait()
        print("10 keV, %d exit photons: trace %.2f ms" % (n, ms), flush=True)
        for bins in (128, 1024):
            for regime in (1, 2):
                with polycap_amd.SpotMap(ctx, [1.0], WIN, (bins, bins), regime=regime) as m:
                    print("  map %4d^2, %s: %s" % (bins, "energies across lanes" if m.wide else "LDS tiles",
                                                              time_add(ctx, m)), flush=True)
    prob = polycap_amd.problem_from_inp(INP)
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.run(7, 0, n, keep_images=True)
        ms = ctx.wait()
        print("%d energies, %d exit photons: trace %.2f ms" % (prob.n_energies, n, ms), flush=True)
        for regime in (1, 2):
            for sel in ([0, 100, 200], list(range(0, prob.n_energies, 36)), None):
                with polycap_amd.SpotMap(ctx, [1.0], WIN, (64, 64), energies=sel, regime=regime) as m:
                    print("  map 64^2 x %3d energies, %s: %s" % (m.shape[1], "energies across lanes" if m.wide else "LDS tiles",
                                                                            time_add(ctx, m, reps=3)), flush=True)


def api(n):
    from polycap_amd import capi
    src0 = capi.Source.new_from_file(INP)
    desc = capi.Description(None, 0, 0, None, 0, _handle=capi._lib().polycap_source_get_description(src0._h), _owner=src0)
    src = capi.Source(desc, 2000., 0.2065, 0.2065, 0., 0., 0., 0., 0., np.array([10.0]))
    os.environ["POLYCAP_SEED"] = "11"
    src.get_transmission_efficiencies(-1, 100000)
    for label, env in (("POLYCAP_IMAGES=1, no maps", {"POLYCAP_IMAGES": "1"}),
                       ("POLYCAP_IMAGES=0 POLYCAP_SPOT (128^2)", {"POLYCAP_IMAGES": "0", "POLYCAP_SPOT": "dist=1;window=-0.02,0.02,-0.02,0.02;bins=128x128"}),
                       ("POLYCAP_IMAGES=0 POLYCAP_SPOT (3 planes, 256^2)", {"POLYCAP_IMAGES": "0", "POLYCAP_SPOT": "dist=0.5,1,2;window=-0.02,0.02,-0.02,0.02;bins=256x256"})):
        os.environ.pop("POLYCAP_SPOT", None)
        os.environ.update(env)
        ts = []
        for _ in range(4):
            t0 = time.perf_counter()
            eff = src.get_transmission_efficiencies(-1, n)
            ts.append((time.perf_counter() - t0) * 1e3)
            del eff
        print("public call, %d photons, %s: %s ms (best %.1f)" % (n, label, " ".join("%.1f" % t for t in ts), min(ts)), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10000000
    (kernel if mode == "kernel" else api)(n)

"""Emit relays (pc_hip_emit_*): a thin sample between two optics, on the device against through the host.

    python scripts/bench_emit.py [1 12 ...]    # numbers of energies (default: 1 and 12)

The ellipsoidal test optic A (tests/common.py) and the same optic reversed, B, at 90 degrees, 0.5 cm from A's focus, with a sample
sheet at 45 degrees in the focus (the confocal geometry of tests/test_gpu_emit.py); 1e6 exit photons of A, traced once and kept on
the device.  Timed from there, in 5 interleaved passes after a warm-up pass (host, emit, host scan, emit scan, and again), medians:
  host       the round trip the emit replaces: fetch A's records, the contract of include/polycap-hip.h in numpy (Philox4x32-10
             in numpy on the slots, so that both sides emit the same photons), pc_hip_launch_photons on B, the weights multiplied on
             the host (its parts are reported too);
  emit       TraceContext.emit: count, scan and inject kernels, the same trace kernel, the finish kernel; nothing per-photon crosses PCIe;
  host scan  21 host round trips, one per depth of -50 .. 50 um (the records are fetched once per trip, as a loop of round trips does);
  emit scan  emit_depth_scan over the same 21 depths.
Both sides give the same photons, which is checked on the number of transmitted photons and on the transmitted weight.  The numpy
part of the host figure is plain numpy, so the ratio is partly a numpy figure; the parts are reported for that reason.  Every energy
count is measured by a child process of its own under a time limit (STEP_TIMEOUT seconds); the first one that fails or runs out of
time ends the script, and nothing more is started on the GPU."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

SHAPE_B = (2, 9., 0.0585, 0.2065, 9.9153e-5, 0.00035, 0.5, 1000.)          # tests/common.py:TEST_SHAPE reversed
SRC = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)
GEOM = dict(focus=0.5, sample_angle=math.pi / 4., det_angle=math.pi / 2., wd=0.5)
DEPTHS = [5e-4 * k for k in range(-10, 11)]
EMIT_SEED = 4242
PI = float.fromhex("0x1.921fb54442d18p+1")


def problems(energies):
    """the two optics, built like the tests build them (the profile generator of the CPU oracle)"""
    from tests.common import make_custom, make_pair
    from oracle import pyoracle
    pyoracle.build()
    _, _, pa, _ = make_pair(pyoracle, "ellip", energies=energies)
    _, _, pb, _ = make_custom(pyoracle, SHAPE_B, 200000, SRC, energies=energies)
    return pa, pb


def philox_uniforms(seed, slots):
    """uniforms 0 and 1 of the streams (seed, slot, attempt 0): Philox4x32-10 on counter (slot lo, slot hi, 0, 0), in numpy"""
    u64, m32 = np.uint64, np.uint64(0xFFFFFFFF)
    s = slots.astype(u64)
    c0, c1, c2, c3 = s & m32, s >> u64(32), np.zeros_like(s), np.zeros_like(s)
    k0, k1 = u64(seed & 0xFFFFFFFF), u64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> u64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + u64(0x9E3779B9)) & m32, (k1 + u64(0xBB67AE85)) & m32
    w0, w1 = (c1 << u64(32)) | c0, (c3 << u64(32)) | c2
    return (w0 >> u64(11)).astype(np.float64) * 2.0 ** -53, (w1 >> u64(11)).astype(np.float64) * 2.0 ** -53


def emit_numpy(rec, slots, fr, R, seed):
    """the emission of the contract in numpy: (start, direction, electric vector, t, r, g, kept)"""
    ns, hs, u, v, n, c = fr[0:3], fr[3], fr[4:7], fr[7:10], fr[10:13], fr[13:16]
    x, y, dx, dy = (rec[:, k] for k in (8, 9, 11, 12))
    with np.errstate(all="ignore"):
        dz = np.sqrt((1. - dx * dx) - dy * dy)
        sd = (ns[0] * dx + ns[1] * dy) + ns[2] * dz
        sp = hs - (ns[0] * x + ns[1] * y)
        t = sp / sd
        u1, u2 = philox_uniforms(seed, slots)
        a, b = (2. * u1 - 1.) * R, (2. * u2 - 1.) * R
        q0, q1, q2 = c[0] - (x + dx * t), c[1] - (y + dy * t), c[2] - dz * t
        f0 = a + ((u[0] * q0 + u[1] * q1) + u[2] * q2)
        f1 = b + ((v[0] * q0 + v[1] * q1) + v[2] * q2)
        f2 = (n[0] * q0 + n[1] * q1) + n[2] * q2
        k = (rec[:, 10] > 0.) & (rec[:, 17] > 0.) & (sd > 0.) & (sp >= 0.) & (f2 > 0.)
        r2 = (f0 * f0 + f1 * f1) + f2 * f2
        r = np.sqrt(r2)
        d0, d1, d2 = f0 / r, f1 / r, f2 / r
        g = ((R * R) * d2) / (PI * r2)
        h = np.sqrt(d2 * d2 + d0 * d0)
        even = (slots & 1) == 0
        zero = np.zeros_like(x)
        ev = np.stack([np.where(even, d2 / h, 0. - (d0 * d1) / h), np.where(even, zero, h), np.where(even, 0. - d0 / h, 0. - (d1 * d2) / h)], axis=1)
    return np.stack([a, b, zero], axis=1)[k], np.stack([d0, d1, d2], axis=1)[k], ev[k], g[k], k


def host_trip(a, b, depth, R, times=None):
    """one host round trip: the transmitted weight per energy and the number of transmitted photons"""
    t0 = time.perf_counter()
    rec = a.records()
    t1 = time.perf_counter()
    fr = polycap_amd.emit_frame(GEOM["focus"], GEOM["sample_angle"], depth, GEOM["det_angle"], GEOM["wd"], (0., 0.), R)["frame"]
    st, di, ev, g, k = emit_numpy(rec, np.arange(rec.shape[0], dtype=np.int64), fr, R, EMIT_SEED)
    t2 = time.perf_counter()
    o = b.launch_photons(st, di, ev)
    t3 = time.perf_counter()
    ok = o["rc"] == 1
    sums = ((rec[k][ok, 17:] * g[ok][:, None]) * o["weights"][ok]).sum(axis=0)
    t4 = time.perf_counter()
    if times is not None:
        times["host"].append((t4 - t0) * 1e3); times["fetch"].append((t1 - t0) * 1e3)
        times["numpy"].append((t2 - t1 + t4 - t3) * 1e3); times["launch"].append((t3 - t2) * 1e3)
    return sums, int(ok.sum())


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def main(ne, n=1000000, passes=5):
    pa, pb = problems((10.0,) if ne == 1 else tuple(np.linspace(5., 27., ne)))
    R = float(pb.ext[0])
    tm = dict(host=[], fetch=[], numpy=[], launch=[], emit=[], stage2=[], host_scan=[], emit_scan=[])
    with polycap_amd.TraceContext(pa) as a, polycap_amd.TraceContext(pb) as b:
        a.run(20000, 0, n, keep_images=True)
        a_ms = a.wait()
        for i in range(passes + 1):
            warm = i == 0                                                 # warm-up: buffers allocated, kernels loaded
            sums, n_ok = host_trip(a, b, 0., R, None if warm else tm)
            t0 = time.perf_counter()
            r = a.emit(b, GEOM["focus"], GEOM["sample_angle"], 0., GEOM["det_angle"], GEOM["wd"], seed=EMIT_SEED)
            t1 = time.perf_counter()
            assert r["counters"]["exit"] == n_ok and np.allclose(r["sum_weights"], sums, rtol=1e-9)
            exits = [host_trip(a, b, d, R)[1] for d in DEPTHS]
            t2 = time.perf_counter()
            sc = polycap_amd.emit_depth_scan(a, b, DEPTHS, GEOM["focus"], GEOM["sample_angle"], GEOM["det_angle"], GEOM["wd"], seed=EMIT_SEED)
            t3 = time.perf_counter()
            assert exits == [c["exit"] for c in sc["counters"]]
            if not warm:
                tm["emit"].append((t1 - t0) * 1e3); tm["stage2"].append(r["kernel_ms"])
                tm["host_scan"].append((t2 - t1) * 1e3); tm["emit_scan"].append((t3 - t2) * 1e3)
        out = dict(n_energies=ne, exit_photons_a=n, a_kernel_ms=a_ms, injected=r["counters"]["n_in"], transmitted=r["counters"]["exit"],
                   efficiency=float(r["efficiencies"][0]), host_ms=spread(tm["host"]), host_fetch_ms=spread(tm["fetch"]),
                   host_numpy_ms=spread(tm["numpy"]), host_launch_photons_ms=spread(tm["launch"]), emit_ms=spread(tm["emit"]),
                   emit_stage2_kernel_ms=spread(tm["stage2"]), speedup_median=float(np.median(tm["host"]) / np.median(tm["emit"])),
                   scan_depths=len(DEPTHS), scan_exit=exits, scan_host_ms=spread(tm["host_scan"]), scan_emit_ms=spread(tm["emit_scan"]),
                   scan_speedup_median=float(np.median(tm["host_scan"]) / np.median(tm["emit_scan"])))
        print(json.dumps(out), flush=True)


STEP_TIMEOUT = 420


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--one":
        main(int(args[1]))
    else:
        import subprocess
        for ne in ([int(v) for v in args] or [1, 12]):
            # a fresh process per measurement, under its own time limit; a failure ends the script
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(ne)], timeout=STEP_TIMEOUT, check=True)

"""Slab emits (pc_hip_slab_*): an emit relay through a thick sample, against the thin emit and against the round trip through the host.

    python scripts/bench_emit_slab.py [1 12 ...]    # numbers of energies (default: 1 and 12)

The pair of scripts/bench_emit.py (the ellipsoidal test optic A, the same optic reversed, B, at 90 degrees, 0.5 cm from A's focus, the
sample at 45 degrees in the focus) with a slab of 20 um behind the sheet and one attenuation coefficient per energy; 1e6 exit photons of
A, traced once and kept on the device.  Timed from there, in 5 interleaved passes after a warm-up pass (slab, thin, host, and again),
medians:
  slab   TraceContext.emit with thickness, mu_in, mu_out: count, scan and inject kernels (a third uniform, the path in the slab), the
         same trace kernel, the finish kernel (one exponential per photon and energy);
  thin   TraceContext.emit on the same contexts: the cost of the slab is reported as the ratio slab / thin of one run;
  host   the round trip the slab emit replaces: fetch A's records, the contract of include/polycap-hip.h in numpy (Philox4x32-10 in
         numpy on the slots, so that both sides emit the same photons), pc_hip_launch_photons on B, the weights and the exponential
         on the host (its parts are reported too).
Both sides give the same photons, which is checked on the number of transmitted photons and on the transmitted weight.  The numpy part
of the host figure is plain numpy, so that ratio is partly a numpy figure.  Every energy count is measured by a child process of its
own under a time limit (STEP_TIMEOUT seconds); the first one that fails or runs out of time ends the script, and nothing more is
started on the GPU."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import polycap_amd
from bench_emit import EMIT_SEED, GEOM, PI, problems, spread

THICKNESS = 0.002
LOG2E, LN2_HI, LN2_LO = 1.4426950408889634074, 6.93147180369123816490e-01, 1.90821492927058770002e-10
EXP_C = (2.50521083854417187751e-08, 2.75573192239858906526e-07, 2.75573192239858906526e-06, 2.48015873015873015873e-05,
         1.98412698412698412698e-04, 1.38888888888888888889e-03, 8.33333333333333333333e-03, 4.16666666666666666667e-02,
         1.66666666666666666667e-01, 0.5, 1.0, 1.0)


def mu_of(energies, scale):
    return scale * (10. / np.asarray(energies, dtype=np.float64)) ** 2.7 + 3.


def philox_block(seed, slots, block):
    """the two uniforms of block `block` of the streams (seed, slot, attempt 0): Philox4x32-10 on counter (slot lo, slot hi, 0, block)"""
    u64, m32 = np.uint64, np.uint64(0xFFFFFFFF)
    s = slots.astype(u64)
    c0, c1, c2, c3 = s & m32, s >> u64(32), np.zeros_like(s), np.full_like(s, block)
    k0, k1 = u64(seed & 0xFFFFFFFF), u64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> u64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + u64(0x9E3779B9)) & m32, (k1 + u64(0xBB67AE85)) & m32
    w0, w1 = (c1 << u64(32)) | c0, (c3 << u64(32)) | c2
    return (w0 >> u64(11)).astype(np.float64) * 2.0 ** -53, (w1 >> u64(11)).astype(np.float64) * 2.0 ** -53


def exp_neg(x):
    """E(x) of the contract for -700 <= x <= 0"""
    k = np.rint(x * LOG2E)
    r = x - k * LN2_HI
    r = r - k * LN2_LO
    p = np.full_like(x, EXP_C[0])
    for c in EXP_C[1:]:
        p = p * r + c
    return np.where(x < -700., 0., np.ldexp(p, k.astype(np.int32)))


def slab_numpy(rec, slots, fr, R, seed):
    """the slab's emission of the contract in numpy: (start, direction, electric vector, gl, s, s_out, kept)"""
    ns, hs, u, v, n, c, kk, T = fr[0:3], fr[3], fr[4:7], fr[7:10], fr[10:13], fr[13:16], fr[16:19], fr[19]
    x, y, dx, dy = (rec[:, k] for k in (8, 9, 11, 12))
    with np.errstate(all="ignore"):
        dz = np.sqrt((1. - dx * dx) - dy * dy)
        sd = (ns[0] * dx + ns[1] * dy) + ns[2] * dz
        sp = hs - (ns[0] * x + ns[1] * y)
        t = sp / sd
        L = T / sd
        u1, u2 = philox_block(seed, slots, 0)
        u3, _ = philox_block(seed, slots, 1)
        s = u3 * L
        zn = s * sd
        a, b = (2. * u1 - 1.) * R, (2. * u2 - 1.) * R
        q0, q1, q2 = c[0] - ((x + dx * t) + dx * s), c[1] - ((y + dy * t) + dy * s), c[2] - (dz * t + dz * s)
        f0 = a + ((u[0] * q0 + u[1] * q1) + u[2] * q2)
        f1 = b + ((v[0] * q0 + v[1] * q1) + v[2] * q2)
        f2 = (n[0] * q0 + n[1] * q1) + n[2] * q2
        r2 = (f0 * f0 + f1 * f1) + f2 * f2
        r = np.sqrt(r2)
        d0, d1, d2 = f0 / r, f1 / r, f2 / r
        g = ((R * R) * d2) / (PI * r2)
        h = np.sqrt(d2 * d2 + d0 * d0)
        cn = ((kk[0] * f0 + kk[1] * f1) + kk[2] * f2) / r
        s_out = np.where(cn > 0., np.maximum(T - zn, 0.) / cn, zn / (0. - cn))
        gl = g * L
        k = (rec[:, 10] > 0.) & (rec[:, 17] > 0.) & (sd > 0.) & (sp >= 0.) & (f2 > 0.) & ((cn > 0.) | (cn < 0.)) & (gl < 1.)
        even = (slots & 1) == 0
        zero = np.zeros_like(x)
        ev = np.stack([np.where(even, d2 / h, 0. - (d0 * d1) / h), np.where(even, zero, h), np.where(even, 0. - d0 / h, 0. - (d1 * d2) / h)], axis=1)
    return np.stack([a, b, zero], axis=1)[k], np.stack([d0, d1, d2], axis=1)[k], ev[k], gl[k], s[k], s_out[k], k


def host_trip(a, b, R, mu_in, mu_out, times=None):
    """one host round trip: the transmitted weight per energy and the number of transmitted photons"""
    t0 = time.perf_counter()
    rec = a.records()
    t1 = time.perf_counter()
    fr = polycap_amd.emit_slab_frame(GEOM["focus"], GEOM["sample_angle"], 0., GEOM["det_angle"], GEOM["wd"], (0., 0.), R, thickness=THICKNESS)["frame"]
    st, di, ev, gl, s, s_out, k = slab_numpy(rec, np.arange(rec.shape[0], dtype=np.int64), fr, R, EMIT_SEED)
    t2 = time.perf_counter()
    o = b.launch_photons(st, di, ev)
    t3 = time.perf_counter()
    ok = o["rc"] == 1
    att = exp_neg(0. - (mu_in[None, :] * s[ok][:, None] + mu_out[None, :] * s_out[ok][:, None]))
    sums = (((rec[k][ok, 17:] * gl[ok][:, None]) * att) * o["weights"][ok]).sum(axis=0)
    t4 = time.perf_counter()
    if times is not None:
        times["host"].append((t4 - t0) * 1e3); times["fetch"].append((t1 - t0) * 1e3)
        times["numpy"].append((t2 - t1 + t4 - t3) * 1e3); times["launch"].append((t3 - t2) * 1e3)
    return sums, int(ok.sum())


def main(ne, n=1000000, passes=5):
    energies = (10.0,) if ne == 1 else tuple(np.linspace(5., 27., ne))
    pa, pb = problems(energies)
    mu_in, mu_out = mu_of(energies, 400.), mu_of(energies, 900.)
    R = float(pb.ext[0])
    tm = dict(host=[], fetch=[], numpy=[], launch=[], slab=[], slab_stage2=[], thin=[], thin_stage2=[])
    geom = (GEOM["focus"], GEOM["sample_angle"], 0., GEOM["det_angle"], GEOM["wd"])
    with polycap_amd.TraceContext(pa) as a, polycap_amd.TraceContext(pb) as b:
        a.run(20000, 0, n, keep_images=True)
        a_ms = a.wait()
        for i in range(passes + 1):
            warm = i == 0                                                 # warm-up: buffers allocated, kernels loaded
            t0 = time.perf_counter()
            r = a.emit(b, *geom, seed=EMIT_SEED, thickness=THICKNESS, mu_in=mu_in, mu_out=mu_out)
            t1 = time.perf_counter()
            thin = a.emit(b, *geom, seed=EMIT_SEED)
            t2 = time.perf_counter()
            sums, n_ok = host_trip(a, b, R, mu_in, mu_out, None if warm else tm)
            assert r["counters"]["exit"] == n_ok and np.allclose(r["sum_weights"], sums, rtol=1e-9)
            if not warm:
                tm["slab"].append((t1 - t0) * 1e3); tm["slab_stage2"].append(r["kernel_ms"])
                tm["thin"].append((t2 - t1) * 1e3); tm["thin_stage2"].append(thin["kernel_ms"])
        out = dict(n_energies=ne, exit_photons_a=n, a_kernel_ms=a_ms, thickness_cm=THICKNESS, injected=r["counters"]["n_in"],
                   transmitted=r["counters"]["exit"], transmitted_thin=thin["counters"]["exit"], efficiency=float(r["efficiencies"][0]),
                   efficiency_thin=float(thin["efficiencies"][0]), slab_ms=spread(tm["slab"]), slab_stage2_kernel_ms=spread(tm["slab_stage2"]),
                   thin_ms=spread(tm["thin"]), thin_stage2_kernel_ms=spread(tm["thin_stage2"]),
                   slab_over_thin_median=float(np.median(tm["slab"]) / np.median(tm["thin"])),
                   slab_minus_thin_ms_median=float(np.median(tm["slab"]) - np.median(tm["thin"])),
                   host_ms=spread(tm["host"]), host_fetch_ms=spread(tm["fetch"]), host_numpy_ms=spread(tm["numpy"]),
                   host_launch_photons_ms=spread(tm["launch"]), host_over_slab_median=float(np.median(tm["host"]) / np.median(tm["slab"])))
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

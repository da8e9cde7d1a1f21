"""Layered emits (pc_hip_layers_*): an emit relay through a stack of sample layers, against the slab emit of the same total thickness
and against the round trip through the host.

    python scripts/bench_emit_layers.py [1 12 ...]    # numbers of energies (default: 1 and 12)

The pair of scripts/bench_emit_slab.py (the ellipsoidal test optic A, the same optic reversed, B, at 90 degrees, 0.5 cm from A's focus,
the sample at 45 degrees in the focus) with a stack of 5, 10 and 5 um behind the sheet, three attenuation tables and three production
rows; 1e6 exit photons of A, traced once and kept on the device.  Timed from there, in 5 interleaved passes after a warm-up pass
(layers, slab, host, and again), medians:
  layers TraceContext.emit with layers=: the prefix tables on the host and one copy, count, scan and inject kernels (the slab's
         geometry and the search for the layer), the same trace kernel, the finish kernel (two quotients, five table loads and one
         exponential per photon and energy);
  slab   TraceContext.emit with thickness = 20 um, mu_in, mu_out on the same contexts: the yardstick, the code as it was.  Both trace the
         same photons through B (one geometry); the cost of the layers is reported as the ratio layers / slab of one run;
  host   the round trip the layered emit replaces: fetch A's records, the contract of include/polycap-hip.h in numpy (Philox4x32-10 in
         numpy on the slots, so that both sides emit the same photons), pc_hip_launch_photons on B, the optical depths, the
         exponential and the weights on the host (its parts are reported too).
The layered emit and the host round trip give the same photons, which is checked on the number of transmitted photons and on the
transmitted weight.  The numpy part of the host figure is plain numpy, so that ratio is partly a numpy figure.  Every energy count is
measured by a child process of its own under a time limit (STEP_TIMEOUT seconds); the first one that fails or runs out of time ends
the script, and nothing more is started on the GPU."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import polycap_amd
from bench_emit import EMIT_SEED, GEOM, PI, problems, spread
from bench_emit_slab import exp_neg, mu_of, philox_block

THICKNESSES = (0.0005, 0.001, 0.0005)
SCALES_IN, SCALES_OUT = (400., 90., 1500.), (900., 200., 2500.)


def stack(energies):
    ne = len(energies)
    prod = (np.linspace(0.5, 2., ne), np.linspace(7., 3., ne), np.full(ne, 0.25))
    return [dict(thickness=t, mu_in=mu_of(energies, si), mu_out=mu_of(energies, so), production=q)
            for t, si, so, q in zip(THICKNESSES, SCALES_IN, SCALES_OUT, prod)]


def tables(layers):
    """(thickness [n], mu_in, pin, mu_out, sout, pout, production [n, ne]) in the contract's order of operations"""
    th = np.array([l["thickness"] for l in layers])
    mu_in, mu_out, prod = (np.array([l[k] for l in layers]) for k in ("mu_in", "mu_out", "production"))
    n = len(th)
    pin, pout, sout = np.zeros_like(mu_in), np.zeros_like(mu_out), np.zeros_like(mu_out)
    for j in range(1, n):
        pin[j] = pin[j - 1] + mu_in[j - 1] * th[j - 1]
        pout[j] = pout[j - 1] + mu_out[j - 1] * th[j - 1]
    for j in range(n - 2, -1, -1):
        sout[j] = sout[j + 1] + mu_out[j + 1] * th[j + 1]
    return th, mu_in, pin, mu_out, sout, pout, prod


def layers_numpy(rec, slots, fr, Z, R, seed):
    """the stack's emission of the contract in numpy: (start, direction, electric vector, gl, sd, cn, za, zb, j, kept)"""
    ns, hs, u, v, n, c, kk, T, qmax = fr[0:3], fr[3], fr[4:7], fr[7:10], fr[10:13], fr[13:16], fr[16:19], fr[19], fr[20]
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
        gl = g * L
        j = np.zeros(len(zn), dtype=np.int64)
        for i in range(1, len(Z) - 1):
            j += zn >= Z[i]
        za, zb = zn - Z[j], np.maximum(Z[j + 1] - zn, 0.)
        k = (rec[:, 10] > 0.) & (rec[:, 17] > 0.) & (sd > 0.) & (sp >= 0.) & (f2 > 0.) & ((cn > 0.) | (cn < 0.)) & (gl * qmax < 1.)
        even = (slots & 1) == 0
        zero = np.zeros_like(x)
        ev = np.stack([np.where(even, d2 / h, 0. - (d0 * d1) / h), np.where(even, zero, h), np.where(even, 0. - d0 / h, 0. - (d1 * d2) / h)], axis=1)
    return np.stack([a, b, zero], axis=1)[k], np.stack([d0, d1, d2], axis=1)[k], ev[k], gl[k], sd[k], cn[k], za[k], zb[k], j[k], k


def host_trip(a, b, R, layers, tab, times=None):
    """one host round trip: the transmitted weight per energy and the number of transmitted photons"""
    th, mu_in, pin, mu_out, sout, pout, prod = tab
    t0 = time.perf_counter()
    rec = a.records()
    t1 = time.perf_counter()
    fl = polycap_amd.emit_layers_frame(GEOM["focus"], GEOM["sample_angle"], 0., GEOM["det_angle"], GEOM["wd"], (0., 0.), R, layers=layers)
    st, di, ev, gl, sd, cn, za, zb, j, k = layers_numpy(rec, np.arange(rec.shape[0], dtype=np.int64), fl["frame"], fl["bounds"], R, EMIT_SEED)
    t2 = time.perf_counter()
    o = b.launch_photons(st, di, ev)
    t3 = time.perf_counter()
    ok = o["rc"] == 1
    j, sd, cn, za, zb = j[ok], sd[ok][:, None], cn[ok][:, None], za[ok][:, None], zb[ok][:, None]
    tau_in = (pin[j] + mu_in[j] * za) / sd
    tau_out = np.where(cn > 0., (sout[j] + mu_out[j] * zb) / cn, (pout[j] + mu_out[j] * za) / (0. - cn))
    att = exp_neg(0. - (tau_in + tau_out))
    sums = (((rec[k][ok, 17:] * gl[ok][:, None]) * (prod[j] * att)) * o["weights"][ok]).sum(axis=0)
    t4 = time.perf_counter()
    if times is not None:
        times["host"].append((t4 - t0) * 1e3); times["fetch"].append((t1 - t0) * 1e3)
        times["numpy"].append((t2 - t1 + t4 - t3) * 1e3); times["launch"].append((t3 - t2) * 1e3)
    return sums, int(ok.sum())


def main(ne, n=1000000, passes=5):
    energies = (10.0,) if ne == 1 else tuple(np.linspace(5., 27., ne))
    pa, pb = problems(energies)
    layers = stack(energies)
    tab = tables(layers)
    total = float(sum(THICKNESSES))
    mu_in, mu_out = mu_of(energies, 400.), mu_of(energies, 900.)
    R = float(pb.ext[0])
    tm = dict(host=[], fetch=[], numpy=[], launch=[], layers=[], layers_stage2=[], slab=[], slab_stage2=[])
    geom = (GEOM["focus"], GEOM["sample_angle"], 0., GEOM["det_angle"], GEOM["wd"])
    with polycap_amd.TraceContext(pa) as a, polycap_amd.TraceContext(pb) as b:
        a.run(20000, 0, n, keep_images=True)
        a_ms = a.wait()
        for i in range(passes + 1):
            warm = i == 0                                                 # warm-up: buffers allocated, kernels loaded
            t0 = time.perf_counter()
            r = a.emit(b, *geom, seed=EMIT_SEED, layers=layers)
            t1 = time.perf_counter()
            slab = a.emit(b, *geom, seed=EMIT_SEED, thickness=total, mu_in=mu_in, mu_out=mu_out)
            t2 = time.perf_counter()
            sums, n_ok = host_trip(a, b, R, layers, tab, None if warm else tm)
            assert r["counters"]["exit"] == n_ok and np.allclose(r["sum_weights"], sums, rtol=1e-9)
            if not warm:
                tm["layers"].append((t1 - t0) * 1e3); tm["layers_stage2"].append(r["kernel_ms"])
                tm["slab"].append((t2 - t1) * 1e3); tm["slab_stage2"].append(slab["kernel_ms"])
        out = dict(n_energies=ne, exit_photons_a=n, a_kernel_ms=a_ms, thicknesses_cm=THICKNESSES, injected=r["counters"]["n_in"],
                   transmitted=r["counters"]["exit"], transmitted_slab=slab["counters"]["exit"], efficiency=float(r["efficiencies"][0]),
                   efficiency_slab=float(slab["efficiencies"][0]), layers_ms=spread(tm["layers"]), layers_stage2_kernel_ms=spread(tm["layers_stage2"]),
                   slab_ms=spread(tm["slab"]), slab_stage2_kernel_ms=spread(tm["slab_stage2"]),
                   layers_over_slab_median=float(np.median(tm["layers"]) / np.median(tm["slab"])),
                   layers_minus_slab_ms_median=float(np.median(tm["layers"]) - np.median(tm["slab"])),
                   host_ms=spread(tm["host"]), host_fetch_ms=spread(tm["fetch"]), host_numpy_ms=spread(tm["numpy"]),
                   host_launch_photons_ms=spread(tm["launch"]), host_over_layers_median=float(np.median(tm["host"]) / np.median(tm["layers"])))
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

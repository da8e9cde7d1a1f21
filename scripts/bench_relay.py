"""Relays (pc_hip_relay_*): the exit beam of one optic through a second one, on the device against through the host.

    python scripts/bench_relay.py [1 12 ...]    # numbers of energies (default: 1 and 12)

The ellipsoidal test optic A (tests/common.py) and the same optic reversed, B, 1 cm behind A's exit and aligned (a confocal pair);
1e6 exit photons of A, traced once and kept on the device.  Timed from there, each as the median of 5 repeats after a warm-up:
  host   the round trip the relay replaces: fetch A's records, transform them in numpy, pc_hip_launch_photons on B, multiply the
         weights on the host (its parts are reported too);
  relay  TraceContext.relay: inject kernel, the same trace kernel, finish kernel; nothing per-photon crosses PCIe.
Both give the same photons, which is checked on the transmitted weight.  The numpy part of the host figure is plain numpy (stacked
copies, fancy indexing), so the ratio is partly a numpy figure; the parts are reported for that reason.  Every energy count is
measured by a child process of its own under a time limit (STEP_TIMEOUT seconds); the first one that fails or runs out of time ends
the script, and nothing more is started on the GPU."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import polycap_amd

SHAPE_B = (2, 9., 0.0585, 0.2065, 9.9153e-5, 0.00035, 0.5, 1000.)          # tests/common.py:TEST_SHAPE reversed
SRC = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)


def problems(energies):
    """the two optics, built like the tests build them (the profile generator of the CPU oracle)"""
    from tests.common import make_custom, make_pair
    from oracle import pyoracle
    pyoracle.build()
    _, _, pa, _ = make_pair(pyoracle, "ellip", energies=energies)
    _, _, pb, _ = make_custom(pyoracle, SHAPE_B, 200000, SRC, energies=energies)
    return pa, pb


def fly(rec, gap):
    x, y, dx, dy, ex, ey = (rec[:, k] for k in (8, 9, 11, 12, 13, 14))
    dz = np.sqrt((1. - dx * dx) - dy * dy)
    ez = -(ex * dx + ey * dy) / dz
    t = gap / dz
    zero = np.zeros_like(x)
    return np.stack([x + dx * t, y + dy * t, zero], axis=1), np.stack([dx, dy, dz], axis=1), np.stack([ex, ey, ez], axis=1)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def main(ne, n=1000000, reps=5, gap=1.0):
    pa, pb = problems((10.0,) if ne == 1 else tuple(np.linspace(5., 27., ne)))
    t_host, t_fetch, t_numpy, t_launch, t_relay, t_stage2 = [], [], [], [], [], []
    with polycap_amd.TraceContext(pa) as a, polycap_amd.TraceContext(pb) as b:
        a.run(20000, 0, n, keep_images=True)
        a_ms = a.wait()
        for i in range(reps + 1):
            t0 = time.perf_counter()
            rec = a.records()
            t1 = time.perf_counter()
            st, di, ev = fly(rec, gap)
            t2 = time.perf_counter()
            g = b.launch_photons(st, di, ev)
            t3 = time.perf_counter()
            ok = g["rc"] == 1
            sum_host = (rec[ok, 17:] * g["weights"][ok]).sum(axis=0)
            t4 = time.perf_counter()
            r = a.relay(b, gap)
            t5 = time.perf_counter()
            assert r["counters"]["exit"] == int(ok.sum()) and np.allclose(r["sum_weights"], sum_host, rtol=1e-9)
            if i == 0:
                continue                                              # warm-up: buffers allocated, kernels loaded
            t_host.append((t4 - t0) * 1e3); t_fetch.append((t1 - t0) * 1e3); t_numpy.append((t2 - t1 + t4 - t3) * 1e3)
            t_launch.append((t3 - t2) * 1e3); t_relay.append((t5 - t4) * 1e3); t_stage2.append(r["kernel_ms"])
    out = dict(n_energies=ne, exit_photons_a=n, a_kernel_ms=a_ms, transmitted=r["counters"]["exit"], host_ms=spread(t_host),
               host_fetch_ms=spread(t_fetch), host_numpy_ms=spread(t_numpy), host_launch_photons_ms=spread(t_launch),
               relay_ms=spread(t_relay), relay_stage2_kernel_ms=spread(t_stage2),
               speedup_median=float(np.median(t_host) / np.median(t_relay)))
    print(json.dumps(out), flush=True)


STEP_TIMEOUT = 300


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        main(int(sys.argv[2]))
    else:
        import subprocess
        for ne in ([int(v) for v in sys.argv[1:]] or [1, 12]):
            # a fresh process per measurement, under its own time limit; a failure ends the script
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(ne)], timeout=STEP_TIMEOUT, check=True)

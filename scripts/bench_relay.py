"""Relays (pc_hip_relay_*): the exit beam of one optic through a second one, on the device against through the host.

    python scripts/bench_relay.py [--tilt] [--select] [1 12 ...]    # numbers of energies (default: 1 and 12)

The ellipsoidal test optic A (tests/common.py) and the same optic reversed, B, 1 cm behind A's exit and aligned (a confocal pair);
1e6 exit photons of A, traced once and kept on the device.  Timed from there, each as the median of 5 repeats after a warm-up:
  host   the round trip the relay replaces: fetch A's records, transform them in numpy, pc_hip_launch_photons on B, multiply the
         weights on the host (its parts are reported too);
  relay  TraceContext.relay: inject kernel, the same trace kernel, finish kernel; nothing per-photon crosses PCIe.
With --tilt a second line per energy count: the relay with B tilted by (3 mrad, 1 mrad) (pc_hip_pose_run), wall time and stage-2
kernel time beside the untilted ones, and a 21-point rocking curve (tilt_x -10 .. 10 mrad, relay_rocking_curve) against 21 host
round trips with the tilt done in numpy.  With --select a line for the untilted relay through a pinhole in A's focal plane that
passes about half of the 10 keV weight (a Selection of A, r < 0.0009 cm 0.5 cm behind its exit).  Without the two options the
output is what it was.
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


def fly_posed(rec, gap, basis):
    """the posed relay's contract in numpy (no offset); the photons that miss B's entrance plane are dropped: (start, direction,
    electric vector, kept)"""
    x, y, dx, dy, ex, ey = (rec[:, k] for k in (8, 9, 11, 12, 13, 14))
    u0, u1, u2, v0, v1, v2, n0, n1, n2 = basis
    dz = np.sqrt((1. - dx * dx) - dy * dy)
    ez = -(ex * dx + ey * dy) / dz
    nd = (n0 * dx + n1 * dy) + n2 * dz
    npl = (n0 * (0. - x) + n1 * (0. - y)) + n2 * gap
    k = (nd > 0.) & (npl >= 0.)
    t = npl / nd
    r0, r1, r2 = x + dx * t, y + dy * t, dz * t - gap
    zero = np.zeros_like(x)
    st = np.stack([(u0 * r0 + u1 * r1) + u2 * r2, (v0 * r0 + v1 * r1) + v2 * r2, zero], axis=1)
    di = np.stack([(u0 * dx + u1 * dy) + u2 * dz, (v0 * dx + v1 * dy) + v2 * dz, nd], axis=1)
    ev = np.stack([(u0 * ex + u1 * ey) + u2 * ez, (v0 * ex + v1 * ey) + v2 * ez, (n0 * ex + n1 * ey) + n2 * ez], axis=1)
    return st[k], di[k], ev[k], k


TILT = (0.003, 0.001)
ROCKING = [(1e-3 * m, 0.) for m in range(-10, 11)]
PINHOLE = dict(axis="r", d=0.5, centre=(0., 0.), range=(0., 0.0009))


def host_posed(a, b, gap, tilt):
    """one host round trip with a tilted B: the transmitted weight per energy and the number of transmitted photons"""
    rec = a.records()
    st, di, ev, k = fly_posed(rec, gap, polycap_amd.relay_basis(gap, (0., 0.), tilt))
    g = b.launch_photons(st, di, ev)
    ok = g["rc"] == 1
    return (rec[k][ok, 17:] * g["weights"][ok]).sum(axis=0), int(ok.sum())


def tilt_leg(a, b, ne, n, reps, gap):
    t_relay, t_stage2, t_rock, t_host = [], [], [], []
    sum_host, n_host = host_posed(a, b, gap, TILT)
    for i in range(reps + 1):
        t0 = time.perf_counter()
        r = a.relay(b, gap, tilt=TILT)
        t1 = time.perf_counter()
        if i:
            t_relay.append((t1 - t0) * 1e3); t_stage2.append(r["kernel_ms"])
    assert r["counters"]["exit"] == n_host and np.allclose(r["sum_weights"], sum_host, rtol=1e-9)
    for i in range(3 + 1):
        t0 = time.perf_counter()
        rc = polycap_amd.relay_rocking_curve(a, b, gap, ROCKING)
        t1 = time.perf_counter()
        exits = [host_posed(a, b, gap, tl)[1] for tl in ROCKING]
        t2 = time.perf_counter()
        assert exits == [c["exit"] for c in rc["counters"]]
        if i:
            t_rock.append((t1 - t0) * 1e3); t_host.append((t2 - t1) * 1e3)
    print(json.dumps(dict(leg="tilt", n_energies=ne, exit_photons_a=n, tilt=list(TILT), transmitted=r["counters"]["exit"], missed=r["counters"]["missed"],
                          relay_ms=spread(t_relay), relay_stage2_kernel_ms=spread(t_stage2), rocking_points=len(ROCKING),
                          rocking_relay_ms=spread(t_rock), rocking_host_ms=spread(t_host),
                          rocking_speedup_median=float(np.median(t_host) / np.median(t_rock)))), flush=True)


def select_leg(a, b, ne, n, reps, gap):
    t_relay, t_stage2 = [], []
    with polycap_amd.Selection(a, [PINHOLE]) as sel:
        tot = sel.apply("exit")
        for i in range(reps + 1):
            t0 = time.perf_counter()
            r = a.relay(b, gap, select=sel)
            t1 = time.perf_counter()
            if i:
                t_relay.append((t1 - t0) * 1e3); t_stage2.append(r["kernel_ms"])
    share = tot["passed_w"][0] / (tot["passed_w"][0] + tot["rejected_w"][0])
    print(json.dumps(dict(leg="select", n_energies=ne, exit_photons_a=n, pinhole_r_cm=PINHOLE["range"][1], weight_share_passed=[float(v) for v in share],
                          injected=r["counters"]["n_in"], rejected=r["counters"]["rejected"], transmitted=r["counters"]["exit"],
                          relay_ms=spread(t_relay), relay_stage2_kernel_ms=spread(t_stage2))), flush=True)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def main(ne, n=1000000, reps=5, gap=1.0, legs=()):
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
        if "--tilt" in legs:
            tilt_leg(a, b, ne, n, reps, gap)
        if "--select" in legs:
            select_leg(a, b, ne, n, reps, gap)


STEP_TIMEOUT = 300


if __name__ == "__main__":
    legs = [v for v in sys.argv[1:] if v in ("--tilt", "--select")]
    args = [v for v in sys.argv[1:] if v not in legs]
    if len(args) == 2 and args[0] == "--one":
        main(int(args[1]), legs=legs)
    else:
        import subprocess
        for ne in ([int(v) for v in args] or [1, 12]):
            # a fresh process per measurement, under its own time limit; a failure ends the script
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(ne)] + legs, timeout=STEP_TIMEOUT, check=True)

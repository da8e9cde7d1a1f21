#!/usr/bin/env python3
"""bench.py -- headline benchmark of the photon trace path (BASELINE.json: xos1.inp, 10 keV).

One "step" = one pass of the hot path over one batch: polycap_source_get_transmission_efficiencies for
--photons exit-photon slots per GPU (default 1e7 = BASELINE config C2) on the xos1 optic at 10 keV, image planes
kept in HBM, followed by the one RCCL all-reduce of the per-energy histogram.  Inputs (profile tables, optical
constants, source parameters) are resident in HBM before the timed region; outputs (totals and the 18 image planes of
struct _polycap_images, written by the kernel itself in coalesced runs: the photons a wave finalises together take the next
free positions of the planes) stay in HBM.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run does what its headline figure needs: set up, warm up, time the K steps, dump (with --dump-outputs) and print
the result line.  Everything else it can measure runs with --full only (below).

--dump-outputs DIR writes what the last timed step handed its caller as DIR/<name>.npy (float64, under 64 MB in all):
efficiencies, sum_weights and photon_counts (exit, not entered, not transmitted, reflections) of the whole job, and with
image planes a fixed sample of rank 0's exit photons, exit_images [k, 17] (the planes of struct _polycap_images, the
reflection count as a float) and exit_weights [k, n_energies].  The compact store keeps exit photons in the order of
completion, which varies from run to run, so the sample is chosen by a fixed hash of each photon's source start
coordinates and sorted by them: with the same arguments two runs, or two builds, dump the same photons in the same order.

With N > 1 and no torch.distributed environment the command starts the N ranks itself (a child
`python -m torch.distributed.run --nproc-per-node N ... bench.py ...`, before anything touches the GPU) and relays
rank 0's JSON line; under torch.distributed.run it is one rank of the job.

value = started photons per second (i_start / wall; the unit of simulation work and the denominator of the
efficiency), whole job, max-over-ranks wall time; exit photons/s is printed next to it.
Weak scaling: every rank traces --photons slots.

--full adds, after the timed region: `scheduler` and `roofline.valu_fp64` from one instrumented launch of the last step's
slots, the `rccl` block (every rank's mean kernel time, one extra gather) under torch.distributed.run, and these legs,
rank 0 at N = 1 only (each bounded to seconds; --no-extras leaves out all but cpu_baseline, --no-cpu-baseline that one):
  wall_incl_copyback  the same workload through the public C API with all 18 image planes copied back into host arrays
                      (SURVEY 8d's wall = kernel + reduce + result copy-back; never `value`)
  sweep_291           BASELINE C3's kernel: xos1 on the deck's 291-energy grid, histogram only, launches of 1e6 and 4e6 slots
  sweep_300           the same on BASELINE's literal "300-bin" grid, np.linspace(1, 30, 300)
  ellip_l9_rough      BASELINE C5's deck: ellip_l9.inp with sig_rough = 5 Angstrom, 1 and 291 energies
  leak_262144         leak_calc=true: the reference's test optic, 10 keV, 262144 exit photons
  parity_fixture      the metric's parity half at the north-star N: the 128 committed oracle runs (tests/golden/
                      oracle_totals_xos1_10keV.json, 2.4e8 started photons) retraced on the device on identical seeds
  cpu_baseline        the CPU oracle (reference algorithm, OpenMP) on a bounded sample of the headline workload
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
VALU_ISSUE_PEAK = 256 * 4 * 2.4e9 / 4.0   # CUs x SIMDs x one wave64 VALU instruction per 4 cycles at 2.4 GHz
# rocprofv3 --pmc passes of this same command, condensed by scripts/summarize_profile.py (profiles/README)
PMC_SUMMARY = os.path.join(ROOT, "profiles", "r04", "headline_pmc_summary.json")
BYTES_PER_EXIT_PHOTON = 17 * 8   # 17 image planes of 8 B; + 8 B per energy for exit_coord_weights


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--photons", type=int, default=10_000_000, help="exit-photon slots per GPU per step")
    ap.add_argument("--seed", type=int, default=20000)
    ap.add_argument("--no-images", action="store_true", help="histogram-only mode (no per-photon planes)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: scheduler statistics, the rccl block, the extra "
                         "legs and the CPU baseline (see the module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the legs other than the CPU baseline (profiling runs)")
    ap.add_argument("--cpu-sample", type=int, default=0,
                    help="with --full: exit-photon slots of the CPU baseline sample (0 = sized from a short probe to about 15 s "
                         "of CPU work)")
    ap.add_argument("--opt", action="append", default=[], help="kernel option name=value (event_threshold, blocks_per_cu, ...)")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="collective backend for --gpus > 1 (nccl = RCCL over xGMI; gloo only to rehearse the multi-process "
                         "path on a box with fewer GPUs than ranks: ranks then share devices)")
    ap.add_argument("--master-port", type=int, default=0, help="rendezvous port when bench.py starts the ranks itself")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (see the module docstring)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` typed as is: start the N-rank job as a fresh child before this process has imported
    torch or touched the GPU, relay its output (rank 0 prints the one JSON line) and return its exit status."""
    import socket
    port = args.master_port
    if not port:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    args.gpus = world

    import numpy as np
    import polycap_amd
    from polycap_amd import distributed as pcd

    if polycap_amd.device_count() < 1:
        sys.exit("bench.py: no HIP device (the trace path has no CPU fallback)")
    dev_index = local_rank if args.backend == "nccl" else local_rank % polycap_amd.device_count()
    torch = dist = None
    red_dev = None
    under_launcher = "RANK" in os.environ and "MASTER_PORT" in os.environ      # torch.distributed.run, any world size
    if world > 1 or under_launcher:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            torch.cuda.set_device(dev_index)
            red_dev = torch.device("cuda", dev_index)
            dist.init_process_group(backend="nccl", device_id=red_dev)
        else:
            dist.init_process_group(backend="gloo")

    deck = os.path.join(ROOT, "tests", "golden", "example", "xos1.inp")
    prob = polycap_amd.problem_from_inp(deck, energies=[10.0])
    ne = prob.n_energies
    keep_images = not args.no_images
    ctx = polycap_amd.TraceContext(prob, dev_index)
    ctx.set_option("plane_images", 1)     # the image layout polycap_source_get_transmission_efficiencies runs with (planes, not records)
    ctx.set_option("compact_images", 1)   # ... and its store: exit photons in the order of completion, coalesced runs per plane
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    n_local = args.photons
    slot0 = rank * n_local           # weak scaling: rank r owns slots [r*n, (r+1)*n)

    def barrier():
        # with ranks (any job under torch.distributed.run) the process-group barrier lines them up; then the whole device
        # is synchronised: torch's streams through torch.cuda.synchronize, the library's own through hipDeviceSynchronize
        if dist is not None:
            dist.barrier()
            if red_dev is not None:
                torch.cuda.synchronize()
        ctx.device_synchronize()

    def step(k):
        ctx.run(args.seed + k, slot0, n_local, keep_images=keep_images)
        ms = ctx.wait()                                   # HIP events on the kernel's own stream
        t = ctx.totals()
        vec = pcd.pack_totals(t["counters"], t["sumw_fixed"])
        vec = pcd.allreduce_totals(vec, red_dev)
        return ms, vec

    for k in range(args.warmup):
        step(-1 - k)
    barrier()
    t0 = time.perf_counter()
    kernel_ms, started, exited = [], 0, 0
    last = None
    for k in range(args.steps):
        ms, vec = step(k)
        kernel_ms.append(ms)
        counters, sums, _ = pcd.unpack_totals(vec)
        started += int(counters[0] + counters[1] + counters[2])
        exited += int(counters[0])
        last = (counters, sums)
    barrier()
    wall = time.perf_counter() - t0
    rccl = None
    if dist is not None:
        tt = torch.tensor([wall], dtype=torch.float64, device=red_dev if red_dev is not None else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        wall = float(tt.item())
        if args.full:
            # one extra gather, outside the timed region: every rank's mean kernel time, so that the scaling record shows that
            # the collective saw all the ranks and where the tail of a step is
            rccl = pcd.ranks_report(float(np.mean(kernel_ms)), red_dev)

    if rank == 0:
        counters, sums = last
        eff = pcd.efficiencies_from_totals(counters, sums)
        dumped = None
        if args.dump_outputs:
            # before anything else runs on the context: the instrumented launch of --full overwrites the last step's planes
            dumped = dump_outputs(args.dump_outputs, ctx, counters, sums, eff, n_local if keep_images else 0)
        avg_ms = float(np.mean(kernel_ms))
        alg_bytes = n_local * (BYTES_PER_EXIT_PHOTON + 8 * ne) if keep_images else 8.0 * (ne + 6)
        achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
        kernel = ctx.last_kernel() or "pc_trace_kernel"        # what traced the timed steps (the context picks it, hip.py)
        pmc = pmc_summary(n_local, keep_images, kernel)
        out = {
            "metric": "photons/s (started photons, whole job), xos1 10 keV",
            "value": started / wall,
            "unit": "photons/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": wall / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (Philox-sampled parallel beam on the xos1 profile tables; O/Si glass constants pinned at 10 keV by the reference's own test)",
            "config": {"workload": "example/xos1.inp, 10 keV single energy, %d exit photons per GPU per step%s" %
                                   (n_local, "" if keep_images else ", histogram only"),
                       "exit_photons_per_gpu": n_local, "n_energies": ne, "images": keep_images,
                       "parallelism": "slots sharded over %d GPU(s), one RCCL all-reduce of the histogram per step" % world},
            "exit_photons_per_s": exited / wall,
            "rccl": rccl,
            "efficiency_10keV": float(eff[0]),
            "avg_reflections": float(counters[3]) / max(1, int(counters[0])),
            "started_per_exit": started / max(1, exited),
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS,
                         "traffic": (pmc["FETCH_SIZE"] + pmc["WRITE_SIZE"]) * 1024.0 if pmc else None,
                         "kernel": {"pc_trace_kernel": "pc_trace_kernel<1,0,1024>"}.get(kernel, kernel + "<0>"), "kernel_ms": avg_ms,
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "note": "fp64-VALU/divergence-bound by construction (SURVEY 8d): 144 B per exit photon, written once in coalesced "
                                 "runs (compact store); traffic and the VALU counters come from the committed rocprofv3 --pmc summary "
                                 "of this command (FETCH_SIZE + WRITE_SIZE in KB, raw: the guide's gfx950 x2 correction applies to "
                                 "16-B-per-lane streaming reads, this kernel's traffic is 8-B-per-lane stores), kernel_ms is measured live",
                         "valu_issue": valu_issue(pmc, avg_ms)},
        }
        if args.full:
            # scheduler statistics: the production instantiation of the launching-wave kernel does not count march steps (the
            # ballot sat in its hot loop); one instrumented launch of the last step's slots outside the timed region fills them in
            ctx.set_option("march_stats", 1)
            ctx.run(args.seed + args.steps - 1, slot0, n_local, keep_images=keep_images)
            ctx.wait()
            sched = ctx.phase_stats()
            ctx.set_option("march_stats", 0)
            # useful fp64 work of the kernel as executed (after certified skipping), from its own counters: a march lane-step is
            # 6 FMA = 12 flop; a segment visit ~150 flop-equivalents (quadratic, 7 div, 1-2 sqrt, hexagon tests) and a reflection
            # ~120 + 100 per energy; against the 78.6 TFLOP/s vector-fp64 peak of the MI355X
            useful_flop = 12.0 * sched["march"]["lanes"] + 150.0 * sched["event"]["lanes"] \
                + (120.0 + 100.0 * ne) * float(counters[3]) / max(1, int(counters[0])) * n_local
            ref_flop_eq = 9.0e4 * (started / args.steps / world)   # the reference's literal march: ~9e4 flop-eq per started photon (8d)
            out["scheduler"] = sched
            out["roofline"]["valu_fp64"] = {
                "peak_tflops": 78.6, "useful_tflops": useful_flop / (avg_ms * 1e-3) / 1e12,
                "frac": useful_flop / (avg_ms * 1e-3) / 1e12 / 78.6,
                "reference_algorithm_equivalent_tflops": ref_flop_eq / (avg_ms * 1e-3) / 1e12,
                "note": "useful = arithmetic the certified march still needs, from the kernel's own lane-step counters; the same "
                        "photons cost the reference's literal march ~9e4 flop-equivalents each"}
        if args.full and world == 1 and not args.no_extras:
            if keep_images:
                out["wall_incl_copyback"] = wall_incl_copyback(deck, n_local, started / float(args.steps * n_local))
            out["sweep_291"] = side_workload("xos1", None, None, 1_000_000, dev_index, "profiles/r04/ne291_pmc_summary.json")
            out["sweep_291"]["launch_of_4e6_slots"] = side_workload("xos1", None, None, 4_000_000, dev_index)
            out["sweep_300"] = side_workload("xos1", np.linspace(1.0, 30.0, 300), None, 1_000_000, dev_index)
            out["ellip_l9_rough"] = {"n_energies_1": side_workload("ellip_l9", [10.0], 5.0, 4_000_000, dev_index),
                                     "n_energies_291": side_workload("ellip_l9", None, 5.0, 500_000, dev_index,
                                                                     "profiles/r04/ellip291_pmc_summary.json")}
            out["leak_262144"] = leak_workload(262_144, dev_index)
            out["parity_fixture"] = parity_fixture(prob, dev_index)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(prob, args, ctx)
        if dumped is not None:
            out["dump_outputs"] = dumped
        print(json.dumps(out), flush=True)
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()


DUMP_SAMPLE_BYTES = 48 << 20     # --dump-outputs: bound of the exit photon sample (the totals add a few bytes)
DUMP_CHUNK = 1 << 20             # exit photons fetched from the device at a time


def photon_keys(planes):
    """A fixed 64-bit hash per exit photon of its source start coordinates (planes 0 and 1, drawn from the photon's own
    Philox stream): the same photon gets the same key in every run, wherever the compact store put it."""
    import numpy as np
    x = np.ascontiguousarray(planes[0]).view(np.uint64) ^ (np.ascontiguousarray(planes[1]).view(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    x ^= x >> np.uint64(31)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(29)
    return x


def sample_exit_photons(fetch, n_exit, n_energies):
    """Rows [k, 17 + n_energies] (the 17 image planes, then the exit weights) of a fixed sample of the n_exit photons that
    fetch(first, count) -> (planes [17, count], exit_weights [count, n_energies]) hands out in any order: every photon
    whose key falls in the sample, sorted by its columns (source start coordinates first), at most DUMP_SAMPLE_BYTES."""
    import numpy as np
    cap = max(1, DUMP_SAMPLE_BYTES // (8 * (17 + n_energies)))
    period = np.uint64(max(1, -(-8 * n_exit // (7 * cap))))     # expected sample: 7/8 of the bound, or every photon
    rows = [np.zeros((0, 17 + n_energies))]
    for first in range(0, n_exit, DUMP_CHUNK):
        planes, weights = fetch(first, min(DUMP_CHUNK, n_exit - first))
        keep = photon_keys(planes) % period == 0
        rows.append(np.concatenate([planes[:, keep].T, weights[keep]], axis=1))
    rows = np.concatenate(rows)
    return rows[np.lexsort(rows.T[::-1])][:cap]


def dump_outputs(out_dir, ctx, counters, sums, eff, n_images):
    """--dump-outputs: the last timed step's results as out_dir/<name>.npy (float64); n_images = exit photons the context
    holds image planes of (0: none)."""
    import numpy as np
    arrays = {"efficiencies": np.asarray(eff, dtype=np.float64),
              "sum_weights": np.asarray(sums, dtype=np.float64),
              "photon_counts": np.asarray(counters[:4], dtype=np.float64)}     # the launch count (counters[5]) is scheduling
    if n_images:
        def fetch(first, count):
            p = ctx.image_planes(first, count)
            return p["planes"], p["exit_weights"]
        rows = sample_exit_photons(fetch, n_images, ctx.problem.n_energies)
        arrays["exit_images"] = np.ascontiguousarray(rows[:, :17])
        arrays["exit_weights"] = np.ascontiguousarray(rows[:, 17:])
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "files": sorted(name + ".npy" for name in arrays), "exit_photons_with_images": n_images,
            "exit_photons_sampled": len(arrays["exit_images"]) if n_images else 0,
            "bytes": int(sum(a.nbytes for a in arrays.values()))}


def pmc_summary(n_local, keep_images, kernel):
    """The committed counter summary applies to the default command only (same workload, same kernel)."""
    if n_local != 10_000_000 or not keep_images:
        return None
    try:
        with open(PMC_SUMMARY) as f:
            summary = json.load(f)
    except Exception:
        return None
    if (kernel + "<") not in summary.get("meta", {}).get("kernel", ""):
        return None                       # the counters belong to another kernel
    return summary


def simd_valu_busy(pmc):
    """Share of the kernel's cycles in which a SIMD's vector ALU is executing an instruction, from the counters alone:
    SQ_ACTIVE_INST_VALU counts 4-cycle steps summed over waves, SQ_BUSY_CYCLES the kernel's cycles summed over the 32 shader
    engines (checked against the kernel time of four profiled kernels: SQ_BUSY_CYCLES / 32 = duration x 2.0-2.2 GHz), the chip
    has 1024 SIMDs: 4 A / (1024 B / 32) = A / (8 B).  No clock frequency enters."""
    if not pmc or "SQ_ACTIVE_INST_VALU" not in pmc or not pmc.get("SQ_BUSY_CYCLES"):
        return None
    return pmc["SQ_ACTIVE_INST_VALU"] / (8.0 * pmc["SQ_BUSY_CYCLES"])


def valu_issue(pmc, kernel_ms):
    """VALU issue rate of the trace kernel: wave-instructions per launch (SQ_INSTS_VALU of the committed PMC summary) over
    the live kernel time, against the chip's issue peak.  This, not HBM, is the resource the kernel saturates."""
    if not pmc:
        return None
    rate = pmc["SQ_INSTS_VALU"] / (kernel_ms * 1e-3)
    return {"wave_instructions_per_launch": pmc["SQ_INSTS_VALU"], "achieved_per_s": rate, "peak_per_s": VALU_ISSUE_PEAK,
            "frac": rate / VALU_ISSUE_PEAK,
            "simd_valu_busy": simd_valu_busy(pmc),
            "lane_utilisation": pmc["SQ_THREAD_CYCLES_VALU"] / (64.0 * pmc["SQ_ACTIVE_INST_VALU"]),
            "source": os.path.relpath(PMC_SUMMARY, ROOT) + " (rocprofv3 --pmc) / HIP-event kernel time of this run"}


def pmc_block(pmc_file, kernel, kernel_ms):
    """VALU issue rate, lane utilisation, wait share and HBM traffic of a leg from the committed rocprofv3 --pmc summary of exactly
    its workload (scripts/profile_r04.sh + scripts/summarize_profile.py --kernel ...) over the kernel time measured here.  The
    summary must name the kernel that ran here (tests/test_bench_contract.py checks the committed ones): else no block."""
    try:
        with open(os.path.join(ROOT, pmc_file)) as f:
            pmc = json.load(f)
    except Exception:
        return {"missing": pmc_file}
    named = pmc.get("meta", {}).get("kernel", "")
    if not kernel or (kernel + "<") not in named:
        return {"mismatch": "summary %s is of %r, this leg ran %r" % (pmc_file, named, kernel)}
    rate = pmc["SQ_INSTS_VALU"] / (kernel_ms * 1e-3)
    return {"kernel": named, "wave_instructions_per_launch": pmc["SQ_INSTS_VALU"], "achieved_per_s": rate,
            "peak_per_s": VALU_ISSUE_PEAK, "frac": rate / VALU_ISSUE_PEAK, "simd_valu_busy": simd_valu_busy(pmc),
            "lane_utilisation": pmc["SQ_THREAD_CYCLES_VALU"] / (64.0 * pmc["SQ_ACTIVE_INST_VALU"]),
            "wait_share": pmc["SQ_WAIT_ANY"] / pmc["SQ_WAVE_CYCLES"] if "SQ_WAIT_ANY" in pmc else None,
            "hbm_traffic_bytes_per_launch": (2.0 * pmc["FETCH_SIZE"] + pmc["WRITE_SIZE"]) * 1024.0 if "FETCH_SIZE" in pmc and "WRITE_SIZE" in pmc else None,
            "hbm_traffic_note": "2 x FETCH_SIZE + WRITE_SIZE (gfx950 tallies 128-B read requests at 64 B: MI355X_MICROARCH.md)",
            "source": pmc_file + " (rocprofv3 --pmc of this workload) / HIP-event kernel time of this run"}


def side_workload(deck_name, energies, sig_rough, n_slots, dev_index, pmc_file=None):
    """started photons/s of another BASELINE configuration's kernel (histogram only, one warm-up launch + one timed launch of the same size).
    pmc_file: committed rocprofv3 --pmc summary of exactly this workload."""
    import polycap_amd
    path = os.path.join(ROOT, "tests", "golden", "example", deck_name + ".inp")
    prob = polycap_amd.problem_from_inp(path, energies=energies, sig_rough=sig_rough)
    with polycap_amd.TraceContext(prob, dev_index) as c:
        c.transmission(1, 0, n_slots)              # one untimed warm-up launch of the same size (buffers, clocks), like the headline's warm-up steps
        t0 = time.perf_counter()
        r = c.transmission(2, 0, n_slots)
        dt = time.perf_counter() - t0
        kernel = c.last_kernel()
        sweeps = c.sweep_stats() if kernel == "pc_trace_log_kernel" else None
    eff = r["efficiencies"]
    out = {"workload": "example/%s.inp, %d energies%s, %d exit photons, histogram only" %
                       (deck_name, prob.n_energies, "" if sig_rough is None else ", sig_rough %g A" % sig_rough, n_slots),
           "started_photons_per_s": r["i_start"] / (r["kernel_ms"] * 1e-3), "kernel": kernel, "kernel_ms": r["kernel_ms"], "wall_ms": dt * 1e3,
           "n_started": r["i_start"], "n_exit": r["i_exit"], "n_energies": prob.n_energies,
           "efficiency_first_last": [float(eff[0]), float(eff[-1])],
           "constants": "synthetic away from 10 keV" if getattr(prob, "synthetic_constants", False) else "pinned"}
    if sweeps:
        out["sweeps"] = {"passes": sweeps["passes"], "pass_reflection_steps": sweeps["iterations"],
                         "waves_finish_at": sweeps["wave_life_sum"] / max(1.0, float(sweeps["wave_life_max"])) / (r_waves(kernel) or 1.0)}
    if pmc_file is not None:
        out["valu_issue"] = pmc_block(pmc_file, kernel, r["kernel_ms"])
    return out


def r_waves(kernel):
    """waves of a full launch of the logging kernel: one 512-thread workgroup per CU"""
    return 256 * 8.0 if kernel == "pc_trace_log_kernel" else None


def leak_workload(n_slots, dev_index):
    """SURVEY 8(f) rank 1, leak_calc=true: the reference's ellipsoidal test optic (tests/leaks.c), uniform illumination, 10 keV,
    one warm-up run + one timed run; kernel time by HIP events, wall = with the events in the reference's list order on the host.
    Beside it the CPU oracle's leak driver (the reference's literal algorithm) on a bounded sample of the same slots."""
    import polycap_amd
    from polycap_amd import capi
    from polycap_amd.decks import optical_constants
    prof = capi.Profile(capi.Profile.ELLIPSOIDAL, 9., 0.2065, 0.0585, 0.00035, 9.9153e-5, 1000., 0.5)
    a, s, _ = optical_constants([8, 14], [0.53, 0.47], 2.23, [10.0])
    source = (2000.0, 0.2065, 0.2065, -1.0, 0.0, 0.0, 0.0, 0.5)
    prob = polycap_amd.Problem(prof.get_z(), prof.get_cap(), prof.get_ext(), 0.0, 200000, 2.23, [10.0], a, s, *source)
    with polycap_amd.TraceContext(prob, dev_index) as c:
        c.transmission(1, 0, 4096, leak_calc=True)
        c.transmission(20000, 0, n_slots, leak_calc=True, leak_views=True)       # sizes the context's buffers like a second call of a session
        t0 = time.perf_counter()
        r = c.transmission(20000, 0, n_slots, leak_calc=True, leak_views=True)
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        ext_copy, int_copy = c.leaks(copy=True)
        dt_copy = time.perf_counter() - t0
        kernel = c.last_kernel()
    out = {"workload": "leak_calc=true, ellipsoidal test optic of the reference's tests/leaks.c, 10 keV, %d exit photons" % n_slots,
           "started_photons_per_s": r["i_start"] / (r["kernel_ms"] * 1e-3), "kernel_ms": r["kernel_ms"], "wall_ms": dt * 1e3,
           "wall_what": "run + wait + totals + both event lists in host memory in the reference's list order (ordered on the device, one "
                        "copy into the context's pinned lists, handed out as views)",
           "wall_over_kernel": dt * 1e3 / r["kernel_ms"], "own_copies_of_the_lists_ms": dt_copy * 1e3,
           "n_started": r["i_start"], "n_exit": r["i_exit"], "extleak_events": len(r["ext"]), "intleak_events": len(r["int"]),
           "kernel": kernel, "valu_issue": pmc_block("profiles/r04/leak_pmc_summary.json", kernel, r["kernel_ms"])}
    try:
        from oracle import pyoracle as O
        affinity, quota, model = host_cpus()
        threads = affinity if quota is None else max(1, min(affinity, int(round(quota))))
        optic = O.Optic(prob.z, prob.cap, prob.ext, prob.sig_rough, prob.n_cap, prob.density)
        n_cpu = 125 * threads           # ~55 started photons/s per thread: about 6 s of CPU work per thread
        t0 = time.perf_counter()
        o = O.transmission(optic, O.make_source(*source), [10.0], a, s, 20000, 0, n_cpu, leak_calc=True, n_threads=threads)
        dtc = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": o["i_start"] / dtc, "unit": "photons/s", "cores": threads, "kind": "port", "cpu_model": model,
                               "sample": "oracle leak driver (oracle/polycap_oracle_leak.c, the reference's literal wall search) on slots "
                                         "[0,%d) of the same workload, %.1f s on %d threads" % (n_cpu, dtc, threads),
                               "extleak_events": int(len(o["ext"])), "intleak_events": int(len(o["int"]))}
    except Exception as e:      # the checker is not part of the product: a leg without it still reports the device side
        out["cpu_baseline"] = {"error": repr(e)}
    return out


def wall_incl_copyback(deck, n_photons, started_per_exit):
    """One polycap_source_get_transmission_efficiencies(n_photons) call through the public C API: kernel + totals + all 18
    image planes in host arrays (PCIe).  Started photons = exit photons x the ratio measured in the timed steps."""
    import numpy as np
    from polycap_amd import capi
    src0 = capi.Source.new_from_file(deck)
    desc = capi.Description(None, 0, 0, None, 0, _handle=capi._lib().polycap_source_get_description(src0._h), _owner=src0)
    src = capi.Source(desc, 2000., 0.2065, 0.2065, 0., 0., 0., 0., 0., np.array([10.0]))
    # the library prints the reference's summary lines on C stdout: keep this process's stdout to the one JSON line
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        warm = src.get_transmission_efficiencies(-1, int(n_photons))      # warm-up like the timed steps: context, device and staging buffers
        del warm
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            eff = src.get_transmission_efficiencies(-1, int(n_photons))
            dt = time.perf_counter() - t0
            del eff
            best = dt if best is None else min(best, dt)
    finally:
        import ctypes
        ctypes.CDLL(None).fflush(None)      # the C library's buffered summary lines go where fd 1 points now
        os.dup2(saved, 1)
        os.close(saved)
    return {"ms": best * 1e3, "started_photons_per_s": started_per_exit * n_photons / best, "exit_photons_per_s": n_photons / best,
            "what": "polycap_source_get_transmission_efficiencies(%d) through the public C API, 17 planes + weights copied to host "
                    "arrays (%.2f GB over PCIe), best of 2 after a warm-up call" % (n_photons, n_photons * 144 / 1e9)}


def parity_fixture(prob, dev_index):
    """BASELINE's metric is photons/s AND the efficiency delta against the CPU reference.  The CPU side of that comparison at
    the north-star N (>= 1.2e8 started photons for 1e-4) costs 40 CPU-minutes, so it is a committed fixture: the
    oracle's counters and exact weight sums for 128 seeds x 1e6 exit-photon slots of this workload (scripts/
    make_oracle_totals.py; four of the seeds are re-run live by tests/test_parity_fixture.py).  Here the device retraces the
    same (seed, slot) Philox streams (0.8 s) and the line carries the pooled delta, its per-seed mean +- s.e. and the noise
    constant c = std(delta) sqrt(N_seed).  Only data is read: nothing under oracle/ runs in this leg."""
    import numpy as np
    import polycap_amd
    with open(os.path.join(ROOT, "tests", "golden", "oracle_totals_xos1_10keV.json")) as f:
        doc = json.load(f)
    # the fixture's problem: the xos1 tables with the pinned pair of the reference's test (tests/photon.c:75-76) to the bit
    p = polycap_amd.Problem(prob.z, prob.cap, prob.ext, 0.0, prob.n_cap, prob.density, np.array([10.0]), np.array([42.544635]),
                            np.array([0.503696]), *prob.source)
    n = int(doc["n_slots"])
    d, Sg, So, Ng, No = [], 0, 0, 0, 0
    t0 = time.perf_counter()
    with polycap_amd.TraceContext(p, dev_index) as c:
        for r in doc["runs"]:
            g = c.transmission(int(r["seed"]), 0, n)
            sg = int(g["sumw_fixed"][0, 0]) + (int(g["sumw_fixed"][0, 1]) << 64)
            so, no, ng = int(r["sumw_exact"]), sum(r["counters"][:3]), int(g["i_start"])
            d.append((sg / ng) / (so / no) - 1.0)
            Sg += sg; So += so; Ng += ng; No += no
    dt = time.perf_counter() - t0
    d = np.array(d)
    K = len(d)
    pooled = (Sg / Ng) / (So / No) - 1.0
    se = float(d.std(ddof=1) / np.sqrt(K))
    # efficiency = (sum w / (exit + not transmitted)) * open area = sum w / started
    return {"n_seeds": K, "exit_slots_per_seed": n, "n_started_oracle": No, "n_started_device": Ng,
            "efficiency_oracle": So / 2.0**62 / No, "efficiency_device": Sg / 2.0**62 / Ng,
            "eff_rel_delta_pooled": abs(pooled), "eff_rel_delta_pooled_signed": pooled, "tolerance": 1e-4, "within_tolerance": bool(abs(pooled) <= 1e-4),
            "i_start_rel_delta": Ng / No - 1.0,
            "per_seed_delta_mean": float(d.mean()), "per_seed_delta_se": se, "z": float(d.mean() / se),
            "noise_constant_c": float(d.std(ddof=1) * np.sqrt(No / K)), "seeds_positive": int((d > 0).sum()),
            "device_s": dt,
            "what": "identical (seed, slot) streams: oracle totals from tests/golden/oracle_totals_xos1_10keV.json (oracle/polycap_oracle.c, "
                    "the reference's literal algorithm) against the device's exact fixed-point sums"}


def host_cpus():
    """(usable hardware threads, model name): the affinity mask capped by the cgroup CPU quota of this box"""
    n = os.cpu_count() or 1
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        pass
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                tok = f.read().split()
            if path.endswith("cpu.max"):
                if tok[0] != "max":
                    quota = float(tok[0]) / float(tok[1])
            else:
                q = float(tok[0])
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    per = float(f.read().split()[0])
                if q > 0:
                    quota = q / per
            break
        except Exception:
            continue
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except Exception:
        pass
    return n, quota, model


def cpu_baseline(prob, args, ctx):
    """The CPU oracle (plain-C restatement of the reference algorithm, OpenMP over slots, dynamic schedule) timed on this
    host on a bounded sample of the same workload, one thread and all usable threads, plus the efficiency delta GPU vs
    CPU on exactly those slots."""
    from oracle import pyoracle as O
    affinity, quota, model = host_cpus()
    threads = affinity if quota is None else max(1, min(affinity, int(round(quota))))
    optic = O.Optic(prob.z, prob.cap, prob.ext, prob.sig_rough, prob.n_cap, prob.density)
    src = O.make_source(*prob.source)
    O.transmission(optic, src, prob.energies, prob.amu, prob.scatf, args.seed, 0, 2000, n_threads=threads)  # warm up
    # one thread: ~4 s
    t0 = time.perf_counter()
    o1 = O.transmission(optic, src, prob.energies, prob.amu, prob.scatf, args.seed, 0, 30_000, n_threads=1)
    dt1 = time.perf_counter() - t0
    one_thread = o1["i_start"] / dt1
    n = args.cpu_sample
    if n <= 0:
        # bounded sample: sized so that the timed run is about 15 s on this host
        probe = 4000 * threads
        t0 = time.perf_counter()
        O.transmission(optic, src, prob.energies, prob.amu, prob.scatf, args.seed, 0, probe, n_threads=threads)
        rate = probe / max(time.perf_counter() - t0, 1e-3)
        n = int(min(max(15.0 * rate, 50_000), 8_000_000))
    t0 = time.perf_counter()
    o = O.transmission(optic, src, prob.energies, prob.amu, prob.scatf, args.seed, 0, n, n_threads=threads)
    dt = time.perf_counter() - t0
    g = ctx.transmission(args.seed, 0, n, keep_images=False)
    return {"value": o["i_start"] / dt, "unit": "photons/s", "cores": threads, "kind": "port",
            "sample": "oracle (C restatement of the reference, literal segment march, OpenMP schedule(dynamic,64)) on slots [0,%d) of the "
                      "same xos1 10 keV workload, %.1f s on %d threads" % (n, dt, threads),
            "cpu_model": model, "threads": threads, "affinity_cpus": affinity, "cgroup_cpu_quota": quota,
            "one_thread_value": one_thread, "one_thread_sample": "slots [0,30000), %.1f s" % dt1,
            "parallel_efficiency": (o["i_start"] / dt) / (one_thread * threads),
            "exit_photons_per_s": o["i_exit"] / dt,
            "efficiency_cpu": float(o["efficiencies"][0]), "efficiency_gpu_same_slots": float(g["efficiencies"][0]),
            "eff_rel_delta": abs(float(g["efficiencies"][0]) - float(o["efficiencies"][0])) / float(o["efficiencies"][0]),
            "eff_rel_delta_one_sigma_at_this_n": 0.48 / float(o["i_start"]) ** 0.5,      # measured noise constant of identical-seed runs (parity_fixture)
            "eff_delta_note": "identical seeds on a %.1e-photon sample; the trace is chaotic, so the delta falls as ~0.6/sqrt(N): "
                              "at N = 2.4e8 it is below 1e-4 (profiles/r02/parity_1e8.json, tests/test_parity_fixture.py)" % o["i_start"]}


if __name__ == "__main__":
    main()

"""bench.py on a box without a GPU: it must refuse loudly (the trace has no CPU fallback), and the helpers that read the
committed rocprofv3 summary must find it.  The timed path itself needs an MI355X (driver runs it at round end)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refuses_without_a_device():
    import polycap_amd
    if polycap_amd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "no HIP device" in (r.stderr + r.stdout)
    assert r.stdout.strip() == ""            # no JSON line that could be mistaken for a measurement


def test_multi_gpu_flag_starts_its_own_ranks():
    """`python bench.py --gpus 2` typed as is starts the two ranks itself (a fresh torch.distributed.run child, before
    anything touches the GPU) and returns their status: on a box without a GPU both ranks refuse loudly."""
    import polycap_amd
    if polycap_amd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=900, env=env)
    out = r.stderr + r.stdout
    assert r.returncode != 0 and "no HIP device" in out
    assert not any(line.startswith("{") for line in r.stdout.splitlines())   # no JSON line that could pass for a measurement


def test_committed_counters_are_readable():
    sys.path.insert(0, ROOT)
    import bench
    assert os.path.exists(bench.PMC_SUMMARY)
    with open(bench.PMC_SUMMARY) as f:
        kernel = json.load(f)["meta"]["kernel"].split("void ")[-1].split("<")[0]
    s = bench.pmc_summary(10_000_000, True, kernel)
    for k in ("SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_THREAD_CYCLES_VALU", "FETCH_SIZE", "WRITE_SIZE"):
        assert s[k] > 0
    t = (s["FETCH_SIZE"] + s["WRITE_SIZE"]) * 1024.0
    assert 1.4e9 < t < 2.9e9                 # algorithmic 1.44 GB per launch; measured 1.68 GB with the compact store (round 2: 7.95 GB)
    # the summary belongs to the default command only: other sizes, histogram-only runs and the lane kernel get none
    assert bench.pmc_summary(1000, True, kernel) is None and bench.pmc_summary(10_000_000, False, kernel) is None
    assert bench.pmc_summary(10_000_000, True, "pc_trace_pool_kernel") is None and bench.valu_issue(None, 27.0) is None
    v = bench.valu_issue(s, 27.0)
    assert 0.5 < v["frac"] < 1.0 and 0.3 < v["lane_utilisation"] < 0.8
    # the vector pipes' busy share from the counters alone (no clock frequency): the headline kernel saturates them
    assert 0.85 < v["simd_valu_busy"] < 1.0
    for name, lo, hi in (("ne291", 0.7, 0.9), ("ellip291", 0.65, 0.9), ("leak", 0.2, 0.5)):
        with open(os.path.join(ROOT, "profiles", "r04", name + "_pmc_summary.json")) as f:
            assert lo < bench.simd_valu_busy(json.load(f)) < hi, name


def test_dump_sample_does_not_depend_on_the_store_order(monkeypatch):
    """--dump-outputs samples the compact image store, whose order of completion varies from run to run: the same photons
    handed out in another order give the same rows, within the byte bound; a small run is dumped whole."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 1000 * 8 * 19)      # 1000 rows of 17 planes + 2 energies
    monkeypatch.setattr(bench, "DUMP_CHUNK", 4096)
    rng = np.random.default_rng(3)
    n, ne = 20_000, 2
    planes, weights = rng.uniform(-1, 1, size=(17, n)), rng.uniform(0, 1, size=(n, ne))
    perm = rng.permutation(n)

    def fetcher(p, w):
        return lambda first, count: (p[:, first:first + count], w[first:first + count])
    a = bench.sample_exit_photons(fetcher(planes, weights), n, ne)
    b = bench.sample_exit_photons(fetcher(planes[:, perm], weights[perm]), n, ne)
    assert np.array_equal(a, b) and 500 < len(a) <= 1000 and a.shape[1] == 17 + ne
    assert np.all(np.diff(a[:, 0]) >= 0)                                  # sorted by the source start x coordinate
    rows = np.concatenate([planes.T, weights], axis=1)
    sorted_rows = rows[np.argsort(rows[:, 0])]
    assert np.array_equal(sorted_rows[np.searchsorted(sorted_rows[:, 0], a[:, 0])], a)      # whole photons, as they were
    small = bench.sample_exit_photons(fetcher(planes[:, :700], weights[:700]), 700, ne)
    assert np.array_equal(small, rows[:700][np.lexsort(rows[:700].T[::-1])])


FULL_ONLY = ("scheduler", "wall_incl_copyback", "sweep_291", "sweep_300", "ellip_l9_rough", "leak_262144", "parity_fixture",
             "cpu_baseline")     # what a bench line carries with --full only


@pytest.mark.gpu
def test_dump_outputs_repeat_from_run_to_run(tmp_path):
    """bench.py --dump-outputs: the same arguments give the same inputs, hence the same outputs, file for file, and --full
    (which runs its instrumented launch on the same context after the dump) dumps the same files again; the result line
    still carries the step time of exactly --steps timed steps.  A plain run measures nothing but its steps: none of what
    --full adds, and at most 30 s of its whole time outside them."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--photons", "300000"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    import time
    import numpy as np
    dumps = []
    for k, extra in enumerate(([], [], ["--full", "--no-extras", "--no-cpu-baseline"])):
        d = tmp_path / ("run%d" % k)
        t0 = time.perf_counter()
        r = subprocess.run(cmd + extra + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=env)
        wall = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        if extra:
            assert "scheduler" in line and "valu_fp64" in line["roofline"]
        else:
            assert not [key for key in FULL_ONLY if key in line] and "valu_fp64" not in line["roofline"]
            assert wall - 3 * line["ms_per_step"] * 1e-3 < 30.0
        files = sorted(p.name for p in d.iterdir())
        assert files == ["efficiencies.npy", "exit_images.npy", "exit_weights.npy", "photon_counts.npy", "sum_weights.npy"]
        assert sum((d / f).stat().st_size for f in files) <= 64 << 20
        dumps.append({f[:-len(".npy")]: np.load(d / f) for f in files})
    a = dumps[0]
    assert a["photon_counts"][0] == 300000 and a["exit_images"].shape == (300000, 17) and a["exit_weights"].shape == (300000, 1)
    for b in dumps[1:]:
        for f in a:
            assert a[f].dtype == np.float64 and np.array_equal(a[f], b[f], equal_nan=True), f
    assert a["efficiencies"][0] == line["efficiency_10keV"]


def test_host_cpu_description():
    sys.path.insert(0, ROOT)
    import bench
    n, quota, model = bench.host_cpus()
    assert n >= 1 and (quota is None or quota > 0) and isinstance(model, str) and model


def test_every_committed_summary_names_the_kernel_its_leg_claims():
    """Round 3's leak summary described the 4.8 ms pre-pass kernel (the summariser picked the kernel by dispatch count).  The
    summaries bench.py reads are produced with `scripts/summarize_profile.py --kernel <name>` now, and each must be of the kernel
    that runs the leg; bench.pmc_block refuses a summary of another kernel instead of quoting it."""
    sys.path.insert(0, ROOT)
    import bench
    want = {"headline": "pc_trace_producer_kernel<0, false>", "ne291": "pc_trace_log_kernel<", "ellip291": "pc_trace_log_kernel<",
            "leak": "pc_leak_kernel<"}
    for tag, name in want.items():
        path = os.path.join(ROOT, "profiles", "r04", tag + "_pmc_summary.json")
        with open(path) as f:
            d = json.load(f)
        assert name in d["meta"]["kernel"], (tag, d["meta"]["kernel"])
        for k in ("SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_THREAD_CYCLES_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY"):
            assert d[k] > 0, (tag, k)
    b = bench.pmc_block("profiles/r04/leak_pmc_summary.json", "pc_leak_kernel", 180.0)
    assert b["kernel"].startswith("void pc_leak_kernel<") and 0.05 < b["frac"] < 1.0 and 0.1 < b["lane_utilisation"] <= 1.0
    assert "mismatch" in bench.pmc_block("profiles/r04/leak_pmc_summary.json", "pc_trace_kernel", 180.0)
    assert "missing" in bench.pmc_block("profiles/r04/no_such_summary.json", "pc_leak_kernel", 180.0)
    # the many-energy kernel: rows no longer stream through HBM (round 3: 47 GB per 1e6-slot launch)
    b = bench.pmc_block("profiles/r04/ne291_pmc_summary.json", "pc_trace_log_kernel", 28.0)
    assert b["hbm_traffic_bytes_per_launch"] < 8e9 and b["wait_share"] < 0.35


def test_summariser_fails_on_a_missing_kernel(tmp_path):
    """scripts/summarize_profile.py wants the kernel by name and exits non-zero when no dispatch of it was profiled."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "summarize_profile.py"), "no_such_tag", "r04"], capture_output=True, text=True)
    assert r.returncode != 0 and "--kernel" in (r.stderr + r.stdout)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "summarize_profile.py"), "no_such_tag", "r04", "--kernel", "pc_leak_kernel"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "no counter passes" in (r.stderr + r.stdout)


def test_committed_bench_line_has_the_contract_keys():
    """profiles/r04/headline_bench.json is the line `python bench.py` printed on the MI355X box of the round's final evidence run
    (the legs are `--full`'s now): the keys the driver reads, the two objects the tier asks for, and the extra legs DESIGN
    section 7 quotes."""
    with open(os.path.join(ROOT, "profiles", "r04", "headline_bench.json")) as f:
        d = json.load(f)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f64" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["traffic"] > 0
    assert r["kernel_ms"] <= d["ms_per_step"]          # a step is the kernel + totals + reduce
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0
    for leg in ("wall_incl_copyback", "sweep_291", "sweep_300", "ellip_l9_rough", "leak_262144", "parity_fixture"):
        assert leg in d, leg
    assert d["parity_fixture"]["within_tolerance"] and d["parity_fixture"]["eff_rel_delta_pooled"] <= 1e-4
    assert d["leak_262144"]["n_exit"] == 262144 and d["leak_262144"]["started_photons_per_s"] > 2e6
    assert d["leak_262144"]["kernel"] == "pc_leak_kernel" and "pc_leak_kernel<" in d["leak_262144"]["valu_issue"]["kernel"]
    assert d["leak_262144"]["cpu_baseline"]["value"] > 0
    for leg in (d["sweep_291"], d["sweep_300"], d["ellip_l9_rough"]["n_energies_291"]):
        assert leg["kernel"] == "pc_trace_log_kernel"
    assert d["sweep_291"]["valu_issue"]["kernel"].startswith("void pc_trace_log_kernel<") and d["sweep_300"]["n_energies"] == 300

"""A run's result does not depend on how it is launched.

A photon depends only on (seed, slot, attempt) and the sums are exact fixed-point sums, so the counters, sumw_fixed, every
exit weight and every image plane are the same bit for bit however a run is cut into launches (option run_parts, option
compact_parts), however its photons share the many-energy kernel's sweep passes (options flush_max, log_cap, sweep_fuse) and
wherever the slot range is split.  The many-energy kernels keep per-lane state in device memory (weight rows, reflection logs,
the start fields of the compact store), which two launches in flight on two streams must not share; and a photon's sweep
result must depend on its own log only, not on which photons share its pass.  Every comparison below is bit-equality against
the single-launch run of the same slots; that run is tied to the oracle (oracle/, a CPU fp64 restatement of the reference's
code) by one efficiency check per problem.
"""
import os

import numpy as np
import pytest

from tests.common import make_pair
from tests.conftest import EXAMPLE

pytestmark = pytest.mark.gpu

MIN_PART_SLOTS = 65536      # pc_hip_transmission_run traces at most n_slots / 65536 launches
FIX = 4611686018427387904.0  # 2^62: the scale of the exact sums


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible: the GPU tests need an MI355X"
    return polycap_amd


def _launches(n, parts):
    """a parts case must really be traced as that many launches: the run caps the part count at n_slots / 65536"""
    assert n >= parts * MIN_PART_SLOTS, "%d slots would be traced in fewer than %d launches" % (n, parts)


def _opts(ctx, **opts):
    for k, v in opts.items():
        ctx.set_option(k, v)


def _records(ctx, seed, slot0, n, parts=1):
    """record store, run cut into `parts` launches"""
    if parts > 1:
        _launches(n, parts)
    _opts(ctx, plane_images=0, run_parts=parts)
    r = ctx.transmission(seed, slot0, n, keep_images=True)
    _opts(ctx, run_parts=1)
    return r


def _planes(ctx, seed, slot0, n, parts, before_wait):
    """plane store (option plane_images, what the C API uses), fetched behind the kernel or after wait()"""
    _launches(n, parts)
    _opts(ctx, plane_images=1, run_parts=parts)
    ctx.run(seed, slot0, n, keep_images=True)
    if before_wait:
        p = ctx.image_planes(0, n)
        ctx.wait()
    else:
        ctx.wait()
        p = ctx.image_planes(0, n)
    t = ctx.totals()
    _opts(ctx, plane_images=0, run_parts=1)
    return t, p


def _same_totals(a, b, what):
    assert np.array_equal(a["counters"][:6], b["counters"][:6]), what
    assert np.array_equal(a["sumw_fixed"], b["sumw_fixed"]), what


def _same_records(a, b, what):
    _same_totals(a, b, what)
    assert np.array_equal(a["exit_weights"], b["exit_weights"]), what
    assert np.array_equal(a["images"], b["images"], equal_nan=True), what


def _same_planes(ref, t, p, what):
    _same_totals(ref, t, what)
    assert np.array_equal(p["exit_weights"], ref["exit_weights"]), what
    assert np.array_equal(p["planes"], ref["images"].T, equal_nan=True), what
    assert np.array_equal(p["nrefl"], ref["nrefl"]), what


def _fixed_sums(w):
    """per energy: sum over photons of floor(w 2^62), as Python ints (the device's exact sums)"""
    f = np.floor(w * FIX).astype(np.uint64)
    hi = (f >> np.uint64(32)).sum(axis=0, dtype=np.uint64)
    lo = (f & np.uint64(0xffffffff)).sum(axis=0, dtype=np.uint64)
    return [(int(h) << 32) + int(l) for h, l in zip(hi, lo)]


def _device_sums(t):
    return [int(lo) + (int(hi) << 64) for lo, hi in t["sumw_fixed"]]


def _deck(pa, name, **kw):
    return pa.problem_from_inp(os.path.join(EXAMPLE, name + ".inp"), **kw)


def _vs_oracle(pa, oracle, ctx, prob, seed, ref, n_o, tol_c, lo=None, energies=None, amu=None, scatf=None):
    """the first n_o slots of the single-launch run against the oracle on the same streams: a run of those slots alone gives
    the same photons bit for bit, and its efficiencies agree with the oracle's within tol_c / sqrt(i_start)"""
    g = ctx.transmission(seed, 0, n_o, keep_images=True)
    assert np.array_equal(g["exit_weights"], ref["exit_weights"][:n_o]) and np.array_equal(g["images"], ref["images"][:n_o], equal_nan=True)
    optic = oracle.Optic(prob.z, prob.cap, prob.ext, prob.sig_rough, prob.n_cap, prob.density)
    E = prob.energies if energies is None else energies
    o = oracle.transmission(optic, oracle.make_source(*prob.source), E, prob.amu if amu is None else amu,
                            prob.scatf if scatf is None else scatf, seed, 0, n_o)
    assert g["i_exit"] == n_o == o["i_exit"]
    tol = tol_c / np.sqrt(o["i_start"])
    assert abs(g["i_start"] - o["i_start"]) / o["i_start"] < tol
    d = np.abs(g["efficiencies"] / o["efficiencies"] - 1.0)
    if lo is None:
        assert np.all(d < tol), d.max() * np.sqrt(o["i_start"])
    else:
        assert np.all(d[lo] < tol) and np.all(d < 0.05), (d[lo].max() * np.sqrt(o["i_start"]), d.max())


# ---------------------------------------------------------------------------------------------------------------- run parts
PARTS_CASES = {
    # name: (energies, n_slots, part counts, kernel options, kernel)
    "xos1_12_lane": (12, 460_001, (2, 4, 7), dict(batch_reflections=0), "pc_trace_kernel"),
    "xos1_12_log": (12, 460_001, (2, 4, 7), dict(batch_reflections=1), "pc_trace_log_kernel"),
    "xos1_291": (291, 460_001, (2, 4, 7), {}, "pc_trace_log_kernel"),
    "ellip_l9_rough_291": (291, 460_001, (2, 4, 7), {}, "pc_trace_log_kernel"),
    "xos1_1000": (1000, 140_001, (2,), {}, "pc_trace_log_kernel"),
}


@pytest.mark.parametrize("case", list(PARTS_CASES))
def test_run_parts_at_many_energies(pa, oracle, case):
    """run_parts 2, 4, 7 (consecutive launches alternating between two streams, the tail of one overlapping the head of the next)
    against one launch, with images kept, in the record store and in the plane store: counters, exact sums, every exit weight
    and every image plane bit for bit."""
    n_energies, n, parts_list, opts, kernel = PARTS_CASES[case]
    seed = 13
    ora = {}
    if case.startswith("xos1_12"):
        _, _, prob, (E, A, S) = make_pair(oracle, "xos1", energies=np.linspace(3.0, 30.0, 12))
        ora = dict(energies=E, amu=A, scatf=S)
    elif case == "xos1_291":
        prob = _deck(pa, "xos1")
    elif case == "ellip_l9_rough_291":
        prob = _deck(pa, "ellip_l9", sig_rough=5.0)
    else:
        prob = _deck(pa, "xos1", energies=np.linspace(2.0, 40.0, 1000))
    assert prob.n_energies == n_energies
    with pa.TraceContext(prob) as ctx:
        _opts(ctx, **opts)
        ref = _records(ctx, seed, 0, n)
        assert ctx.last_kernel() == kernel
        assert ref["i_exit"] == n and ref["failed_slots"] == 0
        for parts in parts_list:
            r = _records(ctx, seed, 0, n, parts)
            assert ctx.last_kernel() == kernel
            _same_records(ref, r, (case, "records", parts))
            del r
        for k, parts in enumerate(parts_list):
            t, p = _planes(ctx, seed, 0, n, parts, before_wait=(k % 2 == 0) or len(parts_list) == 1)
            _same_planes(ref, t, p, (case, "planes", parts))
            del t, p
        if case == "xos1_12_log":
            _vs_oracle(pa, oracle, ctx, prob, seed, ref, 20000, 1.5, **ora)
        elif case == "xos1_291":
            _vs_oracle(pa, oracle, ctx, prob, seed, ref, 10000, 1.5, lo=np.asarray(prob.energies) <= 15.0)


# ------------------------------------------------------------------------------------------------------------ compact parts
def _compact(ctx, seed, n, parts):
    _opts(ctx, plane_images=1, compact_images=1, slot_ids=1, compact_parts=parts)
    ctx.run(seed, 0, n, keep_images=True)
    p = ctx.image_planes(0, n)            # before wait(): a compact run is fetched block by block behind the kernel
    ctx.wait()
    t = ctx.totals()
    ids = ctx.slot_ids(0, n)
    _opts(ctx, compact_images=0, slot_ids=0, compact_parts=1)
    return t, p, ids


def _check_permutation(ref, cmp, ids, n):
    assert np.array_equal(np.sort(ids), np.arange(n)), "every slot exactly once"
    assert np.array_equal(cmp["planes"], ref["planes"][:, ids], equal_nan=True)
    assert np.array_equal(cmp["exit_weights"], ref["exit_weights"][ids])
    assert np.array_equal(cmp["nrefl"], ref["nrefl"][ids])


@pytest.mark.parametrize("n_energies", [1, 12])
def test_compact_parts(pa, n_energies):
    """compact_parts 2 and 3 (a compact run of >= 4e6 slots as that many launches on two streams): the lanes' start fields (the
    lane kernel, one energy) and with 12 energies the logging kernel's start fields, reflection logs and weight rows together.
    The planes are a permutation of the slot-ordered run's, and the compact run of one launch gives the same set of photons."""
    n = 4_000_001
    prob = _deck(pa, "xos1", energies=[10.0] if n_energies == 1 else np.linspace(3.0, 30.0, 12))
    kernel = "pc_trace_kernel" if n_energies == 1 else "pc_trace_log_kernel"
    with pa.TraceContext(prob) as ctx:
        if n_energies == 1:
            _opts(ctx, producer=0)
        _opts(ctx, plane_images=1)
        ctx.run(21, 0, n, keep_images=True)
        ctx.wait()
        ref = ctx.image_planes(0, n)
        t0 = ctx.totals()
        assert ctx.last_kernel() == kernel and t0["i_exit"] == n
        for parts in (1, 2, 3):
            _launches(n, parts)
            t, cmp, ids = _compact(ctx, 21, n, parts)
            assert ctx.last_kernel() == kernel
            _same_totals(t0, t, ("compact", n_energies, parts))
            _check_permutation(ref, cmp, ids, n)
            del cmp, ids


# -------------------------------------------------------------------------------------------------------- public C API
def test_c_api_automatic_run_parts(pa, monkeypatch, tmp_path):
    """polycap_source_get_transmission_efficiencies traces 2e6 photons with images as run_parts = 4 launches: with the slot-ordered
    store (POLYCAP_COMPACT=0) on a 19-energy grid of xos1.inp the result equals POLYCAP_RUN_PARTS=1 bit for bit."""
    from polycap_amd import capi
    lines = open(os.path.join(EXAMPLE, "xos1.inp")).read().splitlines()
    assert lines[10].split() == ["1.0", "30.0", "0.1"] and lines[13] == "xos1.prf"
    lines[10] = "3.0 30.0 1.5"
    for k in (13, 14, 15):
        lines[k] = os.path.join(EXAMPLE, lines[k])
    deck = tmp_path / "xos1_19.inp"
    deck.write_text("\n".join(lines) + "\n")
    src = capi.Source.new_from_file(str(deck))
    monkeypatch.setenv("POLYCAP_SEED", "77")
    for k in ("POLYCAP_HIP_DEVICES", "POLYCAP_IMAGES", "POLYCAP_RCCL", "POLYCAP_RUN_PARTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("POLYCAP_COMPACT", "0")
    n = 2_000_000
    _launches(n, 4)
    a = src.get_transmission_efficiencies(-1, n)
    monkeypatch.setenv("POLYCAP_RUN_PARTS", "1")
    b = src.get_transmission_efficiencies(-1, n)
    assert len(a.data[0]) == 19
    assert np.array_equal(a.data[0], b.data[0]) and np.array_equal(a.data[1], b.data[1])
    wa, wb = a.exit_weights, b.exit_weights
    assert wa.shape == (n, 19) and np.array_equal(wa, wb)
    assert np.array_equal(a.d_travel, b.d_travel) and np.array_equal(a.n_refl, b.n_refl)


# ------------------------------------------------------------------------------------------------------ sweep pass mates
@pytest.mark.parametrize("exact_every", [0, 5])
def test_sweep_passes_do_not_leak_between_photons(pa, oracle, exact_every):
    """C5 (ellip_l9.inp, 291 energies, 5 A roughness).  A sweep pass takes the items of several photons; with roughness the FAST
    loop applies a log's roughness factors as one exponential and the EXACT loop one per reflection, so a photon must be swept
    the way its own log asks whoever shares its pass.  Option sweep_exact_every (test hook) sends every 5th slot's logs through
    the EXACT loop, which makes mixed passes common.  Exit weights and exact sums are the same bit for bit under every schedule:
    flush_max, a split of the slot range, run_parts (log_cap moves the cuts between logs: weights to rounding); histogram-only runs (sweep_fuse 0, 1, 2 -- 2 forces the pass that
    takes a fused photon's sums back) give the images run's sums, which are the sums of its exit weights."""
    prob = _deck(pa, "ellip_l9", sig_rough=5.0)
    assert prob.n_energies == 291
    seed, n, cut = 41, 270_001, 100_003
    assert cut % 128 != 0
    with pa.TraceContext(prob) as ctx:
        _opts(ctx, sweep_exact_every=exact_every)
        ref = _records(ctx, seed, 0, n)
        assert ctx.last_kernel() == "pc_trace_log_kernel" and ref["i_exit"] == n
        assert _device_sums(ref) == _fixed_sums(ref["exit_weights"])
        for opts in (dict(flush_max=1), dict(flush_max=16)):
            _opts(ctx, **opts)
            r = _records(ctx, seed, 0, n)
            _opts(ctx, flush_max=8)
            _same_records(ref, r, (exact_every, opts))
            del r
        # the log capacity decides where a photon's logs are cut, and with roughness each log's roughness factors are one
        # exponential: other bits, so the same photons with weights to rounding, and sums that are still those of the weights
        _opts(ctx, log_cap=5)
        r = _records(ctx, seed, 0, n)
        _opts(ctx, log_cap=0)
        assert np.array_equal(ref["counters"][:6], r["counters"][:6]) and np.array_equal(ref["images"], r["images"], equal_nan=True)
        assert np.nanmax(np.abs(r["exit_weights"] - ref["exit_weights"]) / ref["exit_weights"]) < 1e-13
        assert _device_sums(r) == _fixed_sums(r["exit_weights"])
        del r
        r = _records(ctx, seed, 0, n, parts=4)
        _same_records(ref, r, (exact_every, "run_parts 4"))
        del r
        lo = _records(ctx, seed, 0, cut)
        assert np.array_equal(lo["exit_weights"], ref["exit_weights"][:cut])
        assert np.array_equal(lo["images"], ref["images"][:cut], equal_nan=True)
        hi = _records(ctx, seed, cut, n - cut)
        assert np.array_equal(hi["exit_weights"], ref["exit_weights"][cut:])
        assert np.array_equal(hi["images"], ref["images"][cut:], equal_nan=True)
        assert [x + y for x, y in zip(_device_sums(lo), _device_sums(hi))] == _device_sums(ref)
        assert np.array_equal(lo["counters"][:6] + hi["counters"][:6], ref["counters"][:6])
        del lo, hi
        for fuse in (0, 1, 2):
            _opts(ctx, sweep_fuse=fuse)
            h = ctx.transmission(seed, 0, n)
            _same_totals(ref, h, (exact_every, "sweep_fuse", fuse))
        _opts(ctx, sweep_fuse=1)
        if exact_every:
            _vs_oracle(pa, oracle, ctx, prob, seed, ref, 20000, 1.5, lo=np.asarray(prob.energies) <= 15.0)


def test_sweep_exact_every_is_transparent_without_roughness(pa):
    """On the smooth xos1 deck (291 energies) both sweep loops perform the same products: sweep_exact_every = 5 gives the same
    counters, sums, exit weights and image planes as 0, with images kept and histogram only; the option's range is checked."""
    prob = _deck(pa, "xos1")
    n = 150_001
    with pa.TraceContext(prob) as ctx:
        a = _records(ctx, 3, 0, n)
        ah = ctx.transmission(3, 0, n)
        _opts(ctx, sweep_exact_every=5)
        b = _records(ctx, 3, 0, n)
        bh = ctx.transmission(3, 0, n)
        assert ctx.last_kernel() == "pc_trace_log_kernel"
        for bad in (-1, 1 << 31):
            with pytest.raises(pa.HipError):
                ctx.set_option("sweep_exact_every", bad)
    _same_records(a, b, "sweep_exact_every 5")
    _same_totals(a, ah, "histogram only")
    _same_totals(a, bh, "histogram only, sweep_exact_every 5")

"""GPU parity tests: every call goes through the C-ABI of libpolycap.so (include/polycap-hip.h) to the HIP
kernels and is compared with the CPU oracle on identical inputs.

Tolerances.  The reference's trace is chaotic: a 1-ulp change of a start coordinate grows by ~5-8x per
reflection (tests/test_chaos_floor.py measures it on the oracle itself, profiles/r02/parity_1e8.json shows the
device's differences growing at the same rate from a ten times smaller start), so two correct fp64 implementations
agree per photon only while few reflections have happened, and agree statistically afterwards.  Hence:
  * single-event / short trajectories: tight absolute tolerances that grow with the reflection count;
  * discrete outcomes and efficiencies on identical seeds: equal within c/sqrt(N); measured c = 0.48 for the
    efficiency at 10 keV (128 seeds x 1e6 slots, no bias), the tests allow 1.0 (more where many energies or
    rarely-hit high energies widen the spread, stated in each test); at N = 2.4e8 started photons the delta is
    1.4e-5, inside the north-star 1e-4 (tests/test_parity_fixture.py);
  * GPU vs the host compile of the same device header: bit-identical (both are the same IEEE operation sequence).
"""
import numpy as np
import pytest

from tests.common import make_pair, rel, PIN_AMU, PIN_SCATF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import polycap_amd
    assert polycap_amd.device_count() >= 1, "no HIP device visible"
    return polycap_amd


def _photons(oracle, optic, src, n, seed=20000):
    return oracle.sample_photons(optic, src, seed, np.arange(n))


def test_known_answers_launch(pa, oracle, known):
    """reference tests/photon.c:194-360 through pc_hip_launch_photons"""
    optic, src, prob, _ = make_pair(oracle, "ellip")
    l = known["launch"]
    starts = np.array([c["start"] for c in l["cases"]], dtype=np.float64)
    dirs = np.array([c["dir"] for c in l["cases"]], dtype=np.float64)
    ev = np.tile(np.array(l["start_elecv"], dtype=np.float64), (len(starts), 1))
    with pa.TraceContext(prob) as ctx:
        for literal in (0, 1):
            ctx.set_option("literal_march", literal)
            r = ctx.launch_photons(starts, dirs, ev)
            assert r["rc"].tolist() == [c["rc"] for c in l["cases"]]
            k = 2  # straight through: exit coords unchanged, no reflection, no travel
            assert np.allclose(r["exit_coords"][k], 0, atol=1e-5) and r["i_refl"][k] == 0 and abs(r["d_travel"][k]) < 1e-6
        # reference tests/capil.c:341-499 second case seen through launch: one reflection near z = 4.9758
        r = ctx.launch_photons([[0, 0, 0]], [[3e-5, 3e-5, 0.999]], [[0.5, 0.5, 0.]])
        o = oracle.launch_one(optic, [10.0], [PIN_AMU], [PIN_SCATF], (0, 0, 0), (3e-5, 3e-5, 0.999), (0.5, 0.5, 0.))
        assert r["rc"][0] == o["rc"] and r["i_refl"][0] == o["i_refl"]


def test_single_reflection_weights(pa, oracle, known):
    """reference tests/capil.c:302-334: reflectivity 0.984522 / 0.496310 / 0.000035 at 2 / 3.1 / 20 mrad and 10 keV,
    reproduced with photons that reflect exactly once in a straight capillary"""
    from polycap_amd import Problem
    E, A, S = [10.0], [PIN_AMU], [PIN_SCATF]
    z = np.linspace(0, 0.6, 201)
    prob = Problem(z, np.full(201, 1e-3), np.full(201, 0.05), 0.0, 7, 2.23, E, A, S)
    opt = oracle.Optic(z, np.full(201, 1e-3), np.full(201, 0.05), 0.0, 7, 2.23)
    with pa.TraceContext(prob) as ctx:
        for alfa, expect, rc in ((2e-3, 0.984522, 1), (3.1e-3, 0.496310, 1), (2e-2, 0.000035, 0)):
            d = (np.sin(alfa), 0.0, np.cos(alfa))
            o = oracle.launch_one(opt, E, A, S, (0, 0, 0.0), d, (0, 1, 0))
            r = ctx.launch_photons([[0, 0, 0.0]], [d], [[0, 1, 0]])
            assert r["rc"][0] == rc and r["i_refl"][0] == rc and abs(r["weights"][0, 0] - expect) < 1e-5
            assert rel(r["weights"][0], o["weights"]).max() < 1e-9
            assert np.abs(r["exit_coords"][0] - o["exit_coords"]).max() < 1e-12


def test_sampler_matches_oracle(pa, oracle):
    """polycap_source_get_photon on the device vs the oracle on the same Philox streams"""
    for which, source in (("xos1", (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0)),
                          ("ellip", (0.05, 0.1, 0.1, 0.2, 0.2, 0., 0., 0.5)),        # tests/source.c:58 divergent beam
                          ("ellip", (2000., 0.2065, 0.1, 0., 0., 0.01, -0.02, 0.9)),  # elliptical source: libm path
                          ("ellip", (5., 0.01, 0.01, -1., 0., 0., 0., 0.0))):         # uniform illumination (tests/leaks.c:1264)
        optic, src, prob, _ = make_pair(oracle, which, source=source)
        slots = np.arange(4000)
        ref = oracle.sample_photons(optic, src, 424242, slots, attempt=3)
        with pa.TraceContext(prob) as ctx:
            got = ctx.sample_photons(424242, slots, np.full(slots.shape, 3))
        assert np.abs(got - ref).max() < 1e-13, (which, source)


def test_certified_march_is_bit_identical_to_literal_march(pa, oracle):
    """Skipping certified-miss segments must not change a single bit of any photon."""
    for which in ("xos1", "ellip"):
        optic, src, prob, _ = make_pair(oracle, which)
        ph = _photons(oracle, optic, src, 60000)
        with pa.TraceContext(prob) as ctx:
            fast = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
            ctx.set_option("literal_march", 1)
            lit = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        for k in fast:
            assert np.array_equal(fast[k], lit[k], equal_nan=True), (which, k)


def test_gpu_bit_identical_to_host_compile_of_device_header(pa, oracle):
    """The kernels and tests/emul (g++ compile of pc_device.h) execute the same IEEE operation sequence."""
    from tests.emul import pyemul
    for which, energies in (("xos1", (10.0,)), ("ellip", (10.0,)), ("xos1", (8.0, 10.0, 12.5))):
        optic, src, prob, _ = make_pair(oracle, which, energies=energies)
        ph = _photons(oracle, optic, src, 30000, seed=7)
        with pa.TraceContext(prob) as ctx:
            g = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        e = pyemul.launch_batch(prob, ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        for k in g:
            assert np.array_equal(g[k], e[k], equal_nan=True), (which, energies, k)


def test_explicit_photons_vs_oracle(pa, oracle):
    """Identical photons through the oracle and the kernel: discrete outcomes agree except for the chaotic tail,
    short trajectories agree tightly, the summed weight agrees within the reference's own self-noise."""
    for which in ("xos1", "ellip"):
        optic, src, prob, (E, A, S) = make_pair(oracle, which)
        n = 200000
        ph = _photons(oracle, optic, src, n)
        o = oracle.launch_batch(optic, E, A, S, ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        with pa.TraceContext(prob) as ctx:
            g = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        # entrance decisions (rc 2 / -2) involve no chaos: identical
        ent_o = np.isin(o["rc"], (2, -2))
        assert np.array_equal(ent_o, np.isin(g["rc"], (2, -2)))
        assert np.array_equal(o["rc"][ent_o], g["rc"][ent_o])
        # measured on the oracle itself: a 1-ulp input change flips rc or i_refl for 13-15 % of photons; the kernel
        # differs from the oracle by rounding only, so it must stay well below that
        flips = ((o["rc"] != g["rc"]) | (o["i_refl"] != g["i_refl"])).mean()
        # observed: xos1 3.9 % (profiles/r02/parity_1e8.json), the ellipsoidal test optic 6.8 % (its photons reflect more often)
        assert flips < (0.06 if which == "xos1" else 0.08), (which, flips)
        # short trajectories (<= 3 reflections): amplification is still small
        short = (o["rc"] == g["rc"]) & (o["i_refl"] == g["i_refl"]) & (o["i_refl"] <= 3) & np.isin(o["rc"], (0, 1))
        assert short.sum() >= 5
        assert np.abs(g["exit_coords"][short] - o["exit_coords"][short]).max() < 1e-6
        assert rel(g["weights"][short], o["weights"][short]).max() < 1e-6
        # transmitted weight on identical photons: |delta|/sum <= c/sqrt(n) with c = 1.0 (1-ulp self-noise of the
        # oracle is c ~ 0.25, see tests/test_chaos_floor.py)
        so, sg = o["weights"][o["rc"] == 1, 0].sum(), g["weights"][g["rc"] == 1, 0].sum()
        assert abs(sg - so) / so < 1.0 / np.sqrt(n), (which, so, sg)


def test_transmission_driver_vs_oracle(pa, oracle, known):
    """polycap_source_get_transmission_efficiencies on the device vs the oracle driver, same seed, same slots."""
    t = known["transmission_curve"]
    optic, src, prob, (E, A, S) = make_pair(oracle, "ellip")
    n = 30000
    o = oracle.transmission(optic, src, E, A, S, 20000, 0, n, images=True)
    with pa.TraceContext(prob) as ctx:
        g = ctx.transmission(20000, 0, n, keep_images=True)
    assert g["i_exit"] == n and g["failed_slots"] == 0
    # the reference's published known answer (tests/source.c:218): 0.135 +- 0.0075 at 10 keV
    assert abs(g["efficiencies"][0] - 0.135) <= 0.0075
    # same seed, same slots.  Photons whose trajectories decorrelate (chaos) also change the retry sequence of their
    # slot, so i_start and the efficiency differ by c/sqrt(i_start) with c = 0.48 measured over 128 seeds x 1e6 slots
    # (profiles/r02/parity_1e8.json: no bias, mean delta -1.4e-5 +- 3.1e-5); tolerance 2 x that spread (the run is
    # reproducible bit for bit, so the assertion is deterministic)
    tol = 1.0 / np.sqrt(g["i_start"])
    assert abs(g["i_start"] - o["i_start"]) / o["i_start"] < tol
    assert abs(g["efficiencies"][0] - o["efficiencies"][0]) / o["efficiencies"][0] < tol
    assert abs(g["sum_irefl"] - o["sum_irefl"]) / o["sum_irefl"] < tol
    # totals are consistent with the per-slot planes
    assert np.isclose(g["exit_weights"].sum(), g["sum_weights"][0], rtol=1e-12)
    assert g["nrefl"].sum() == g["sum_irefl"]
    img = g["images"]
    names = list(pa.IMG_FIELDS)
    col = lambda k: img[:, names.index(k)]
    assert np.all(col("pc_exit_z") == 9.0) and np.all(col("dtravel") >= 9.0)
    assert np.all(np.abs(col("pc_start_x")) <= 0.2065) and np.all(col("pc_start_dir_x") == 0.)
    assert set(np.unique(col("pc_start_elecv_x"))) <= {0., 1.} and np.all(col("pc_start_elecv_x") + col("pc_start_elecv_y") == 1.)
    assert np.all((g["exit_weights"] >= 1e-4) & (g["exit_weights"] <= 1.0))
    # slots whose first attempt is transmitted with few reflections follow the oracle photon by photon
    oi = o["images"]
    same_start = (oi[:, 2] == img[:, 2]) & (oi[:, 3] == img[:, 3])
    few = same_start & (oi[:, 15] <= 3) & (img[:, 15] == oi[:, 15])
    assert few.sum() >= 1
    assert np.abs(img[few][:, 8:10] - oi[few][:, 8:10]).max() < 1e-6
    assert rel(g["exit_weights"][few], o["exit_weights"][few]).max() < 1e-6
    # pc_exit_dtravel: the device adds the path to a hit as (hz - Pz)/dz instead of the reference's sqrt(dx^2+dy^2+dz^2)
    # (src/polycap-capil.c:1315-1318): the same length of a unit direction up to rounding -- not bit-pinned, so pinned here
    # against the oracle on the photons that follow it
    assert rel(img[few][:, 16], oi[few][:, 16]).max() < 1e-12, rel(img[few][:, 16], oi[few][:, 16]).max()
    # ... and on every photon with the oracle's start and reflection count (their trajectories may have drifted apart by then:
    # observed 4.5e-6 of the ~9 cm)
    same = same_start & (img[:, 15] == oi[:, 15])
    assert same.sum() > n // 10 and rel(img[same][:, 16], oi[same][:, 16]).max() < 1e-4


def test_partition_invariance_and_reproducibility(pa, oracle):
    """Slot-keyed Philox + exact fixed-point sums: any split of the slot range gives bit-identical results."""
    optic, src, prob, _ = make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))
    n = 50000
    with pa.TraceContext(prob) as ctx:
        a = ctx.transmission(99, 0, n, keep_images=True)
        a2 = ctx.transmission(99, 0, n, keep_images=False)
        ctx.set_option("event_threshold", 17)      # the scheduler's switches shape the phases, never a photon
        ctx.set_option("march_stop", 3)
        ctx.set_option("new_threshold", 9)
        ctx.set_option("blocks_per_cu", 2)
        b0 = ctx.transmission(99, 0, 20000, keep_images=True)
        b1 = ctx.transmission(99, 20000, n - 20000, keep_images=True)
        # one run traced as several launches on two streams (what the public API does to overlap the image fetch)
        big = 400000
        c1 = ctx.transmission(7, 5, big, keep_images=True)
        ctx.set_option("run_parts", 5)
        c5 = ctx.transmission(7, 5, big, keep_images=True)
        planes = ctx.image_planes(1000, big - 3000)      # the SoA fetch of the C host layer against the record fetch
        ctx.set_option("run_parts", 1)
    assert np.array_equal(planes["planes"].T, c5["images"][1000:big - 2000], equal_nan=True)
    assert np.array_equal(planes["exit_weights"], c5["exit_weights"][1000:big - 2000])
    assert np.array_equal(c1["counters"][:4], c5["counters"][:4]) and np.array_equal(c1["sumw_fixed"], c5["sumw_fixed"])
    assert np.array_equal(c1["images"], c5["images"], equal_nan=True) and np.array_equal(c1["exit_weights"], c5["exit_weights"])
    assert np.array_equal(a["counters"][:4], a2["counters"][:4]) and np.array_equal(a["sumw_fixed"], a2["sumw_fixed"])
    assert np.array_equal(a["counters"][:4], b0["counters"][:4] + b1["counters"][:4])
    assert np.array_equal(a["images"], np.vstack([b0["images"], b1["images"]]), equal_nan=True)
    assert np.array_equal(a["exit_weights"], np.vstack([b0["exit_weights"], b1["exit_weights"]]))
    lo = int(b0["sumw_fixed"][0, 0]) + int(b1["sumw_fixed"][0, 0])
    hi = int(b0["sumw_fixed"][0, 1]) + int(b1["sumw_fixed"][0, 1]) + (lo >> 64)
    assert (lo & (2**64 - 1), hi) == (int(a["sumw_fixed"][0, 0]), int(a["sumw_fixed"][0, 1]))


def test_run_sharded_single_rank_uses_the_kernel(pa, oracle):
    from polycap_amd import distributed as pcd
    optic, src, prob, _ = make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))
    r = pcd.run_sharded(prob, 5, 30000)
    with pa.TraceContext(prob) as ctx:
        t = ctx.transmission(5, 0, 30000)
    assert r["counters"][:4].tolist() == t["counters"][:4].tolist()
    assert r["sumw_exact"][0] == int(t["sumw_fixed"][0, 0]) + (int(t["sumw_fixed"][0, 1]) << 64)
    assert np.array_equal(r["efficiencies"], t["efficiencies"])


def test_multi_energy_and_roughness(pa, oracle):
    """n_energies > 1 (weights in memory) and sig_rough > 0 (exp path): kernel vs oracle on identical photons."""
    energies = np.linspace(5.0, 20.0, 7)
    optic, src, prob, (E, A, S) = make_pair(oracle, "ellip", energies=energies, sig_rough=5.0)
    n = 40000
    ph = _photons(oracle, optic, src, n, seed=5)
    o = oracle.launch_batch(optic, E, A, S, ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
    with pa.TraceContext(prob) as ctx:
        g = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        t = ctx.transmission(5, 0, 5000, keep_images=True)
    flips = ((o["rc"] != g["rc"]) | (o["i_refl"] != g["i_refl"])).mean()
    assert flips < 0.09, flips      # observed 8.0 % on this optic (more reflections per photon than xos1: 3.9 %); a 1-ulp change of the input flips 14 %
    so, sg = o["weights"][o["rc"] == 1].sum(axis=0), g["weights"][g["rc"] == 1].sum(axis=0)
    assert np.all(np.abs(sg - so) / so < 1.0 / np.sqrt(n)), (np.abs(sg - so) / so * np.sqrt(n)).max()
    short = (o["rc"] == g["rc"]) & (o["i_refl"] == g["i_refl"]) & (o["i_refl"] <= 3) & np.isin(o["rc"], (0, 1))
    assert rel(g["weights"][short], o["weights"][short]).max() < 1e-6
    assert np.all(np.diff(t["efficiencies"]) < 0)      # transmission falls with energy
    assert np.allclose(t["exit_weights"].sum(axis=0), t["sum_weights"], rtol=1e-12)


def test_mono_capillary_and_boundary_capillaries(pa, oracle):
    """mono-capillary (n_shells == 0) under uniform illumination and a 7-capillary optic (all boundary capillaries)"""
    from tests.common import make_custom, MONO_CASE, SEVEN_CASE
    for case in (MONO_CASE, SEVEN_CASE):
        optic, src, prob, (E, A, S) = make_custom(oracle, **case)
        n = 20000
        ph = oracle.sample_photons(optic, src, 5, np.arange(n))
        o = oracle.launch_batch(optic, E, A, S, ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        with pa.TraceContext(prob) as ctx:
            assert np.abs(ctx.sample_photons(5, np.arange(n)) - ph).max() < 1e-13
            g = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
            t = ctx.transmission(5, 0, 3000, keep_images=True)
        assert np.array_equal(o["rc"], g["rc"]) and np.array_equal(o["i_refl"], g["i_refl"])
        m = np.isin(o["rc"], (0, 1))
        assert rel(g["weights"][m], o["weights"][m]).max() < 1e-8
        ot = oracle.transmission(optic, src, E, A, S, 5, 0, 3000, images=True)
        assert t["i_exit"] == 3000 and np.array_equal(t["counters"][:4], ot["counters"])
        assert np.allclose(t["exit_weights"], ot["exit_weights"], rtol=1e-8, atol=0)
        assert np.allclose(t["images"][:, :15], ot["images"][:, :15], rtol=0, atol=1e-9)


def test_degenerate_source_nan_photons(pa, oracle):
    """cone.inp-style source (src_y = 0): half the photons are NaN and must be absorbed, as in the reference."""
    optic, src, prob, (E, A, S) = make_pair(oracle, "ellip", source=(100., 0.2065, 0., 0., 0., 0., 0., 0.))
    slots = np.arange(2000)
    ref = oracle.sample_photons(optic, src, 1, slots)
    with pa.TraceContext(prob) as ctx:
        got = ctx.sample_photons(1, slots)
        g = ctx.launch_photons(got[:, 0:3], got[:, 3:6], got[:, 6:9])
    assert np.array_equal(np.isnan(ref[:, 0]), np.isnan(got[:, 0]))
    o = oracle.launch_batch(optic, E, A, S, ref[:, 0:3], ref[:, 3:6], ref[:, 6:9])
    nan = np.isnan(ref[:, 0])
    assert nan.sum() > 100 and np.array_equal(o["rc"][nan], g["rc"][nan])


@pytest.mark.parametrize("binding", ["ctypes", "cython"])
def test_public_c_api_on_gpu(pa, oracle, known, binding):
    """polycap_photon_launch / polycap_source_get_transmission_efficiencies through the reference-shaped C API,
    via the ctypes classes and via the compiled Cython module `polycap`."""
    if binding == "ctypes":
        from polycap_amd import capi
    else:
        import os
        import sys
        from tests.conftest import ROOT
        sys.path.insert(0, os.path.join(ROOT, "polycap_amd", "pyext"))
        import polycap as capi
    prof = capi.Profile(capi.Profile.ELLIPSOIDAL, 9., 0.2065, 0.0585, 0.00035, 9.9153e-5, 1000., 0.5)
    desc = capi.Description(prof, 0.0, 200000, {"O": 53.0, "Si": 47.0}, 2.23)
    l = known["launch"]
    for c in l["cases"]:
        photon = capi.Photon(desc, c["start"], c["dir"], l["start_elecv"])
        if c["rc"] == -2:
            with pytest.raises(ValueError):
                photon.launch([10.0])
            continue
        w = photon.launch([10.0])
        if c["rc"] == 2:
            assert w is None
        else:
            assert w is not None and w.shape == (1,)
    # reference tests/source.c:165-278: seven energies, 30000 photons, published curve and per-photon sanity checks
    t = known["transmission_curve"]
    src = capi.Source(desc, t["d_source"], t["src_x"], t["src_y"], t["src_sigx"], t["src_sigy"], t["src_shiftx"],
                      t["src_shifty"], t["hor_pol"], np.array(t["energies"], dtype=np.float64))
    eff = src.get_transmission_efficiencies(-1, t["n_photons"])
    energies, effs = eff.data
    assert eff.data is eff.data and not effs.flags.writeable          # tests/python.py:230-235, 262-277
    assert np.all(np.abs(effs - np.array(t["efficiencies"])) <= np.array(t["tolerances"]))
    assert len(list(eff.start_coords)) == t["n_photons"]
    w = eff.exit_weights
    assert w.shape == (t["n_photons"], 7) and w[0, 0] >= 3.5e-4 and np.all((w >= 0) & (w <= 1))
    assert 0 < eff.n_refl[0] < 200 and eff.d_travel[0] >= 9. and next(iter(eff.exit_coords)).z == 9.
    assert next(iter(eff.start_direction)) == (0., 0., 1.)
    with pytest.raises(ValueError):
        eff.write_hdf5(None)
    # reference tests/source.c:280-290: the result of a real run goes to an HDF5 file; read back with h5dump where present
    import os
    import tempfile
    from tests import test_hdf5_writer as H
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "run.h5")
        eff.write_hdf5(path)
        assert os.path.getsize(path) > 30000 * 17 * 8
        if H.H5DUMP is not None:
            assert np.array_equal(H._read(path, "/Transmission_Efficiencies", tmp), effs)
            assert np.array_equal(H._read(path, "/PC_Exit/Weights", tmp).reshape(w.shape), w)
            assert np.array_equal(H._read(path, "/PC_Exit/N_Reflections", tmp), eff.n_refl.astype(np.float64))
    photon = src.get_photon(capi.Rng(20000))
    assert abs(photon.start_coords[0]) <= 0.2065


def test_full_size_properties_xos1_1e7(pa):
    """BASELINE config C2 at full size (xos1.inp, 10 keV, 1e7 exit photons): size-independent properties instead of
    an oracle run -- exact bookkeeping identities, exact partition invariance of the totals, physical sanity, and
    agreement with the efficiency of an independent 2e5-slot sample within its statistical error."""
    import os
    from tests.conftest import EXAMPLE
    prob = pa.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"), energies=[10.0])
    n = 10_000_000
    with pa.TraceContext(prob) as ctx:
        full = ctx.transmission(20000, 0, n, keep_images=True)
        parts = [ctx.transmission(20000, s0, c) for s0, c in ((0, 3_000_001), (3_000_001, 6_999_999))]
        small = ctx.transmission(4242, 0, 200_000)
    assert full["i_exit"] == n and full["failed_slots"] == 0
    assert full["launches"] >= full["i_start"]                       # launches also count photons that missed the optic / errored
    # checksum of checksums: per-slot weights and reflection counts add up to the exact fixed-point totals
    w = full["exit_weights"][:, 0]
    tot = int(full["sumw_fixed"][0, 0]) + (int(full["sumw_fixed"][0, 1]) << 64)
    assert sum(int(x) for x in np.floor(w * 4611686018427387904.0).astype(np.uint64)) == tot
    assert int(full["nrefl"].sum()) == full["sum_irefl"]
    # exact partition invariance at full size
    assert np.array_equal(full["counters"][:4], parts[0]["counters"][:4] + parts[1]["counters"][:4])
    lo = sum(int(p["sumw_fixed"][0, 0]) for p in parts)
    hi = sum(int(p["sumw_fixed"][0, 1]) for p in parts) + (lo >> 64)
    assert (lo & (2**64 - 1), hi) == (int(full["sumw_fixed"][0, 0]), int(full["sumw_fixed"][0, 1]))
    # physics: every exit photon sits in the exit window at z = 9 cm with 1e-4 <= weight <= 1, travelled >= 9 cm
    img = full["images"]
    names = list(pa.IMG_FIELDS)
    col = lambda k: img[:, names.index(k)]
    assert np.all(col("pc_exit_z") == prob.z[-1]) and np.all(col("dtravel") >= prob.z[-1])
    assert np.all(np.hypot(col("pc_exit_x"), col("pc_exit_y")) <= prob.ext[-1] + 1e-12)
    assert np.all((w >= 1e-4) & (w <= 1.0))
    assert np.all(np.hypot(col("src_start_x"), col("src_start_y")) <= 0.2065 * (1 + 1e-12))
    # simulated open area (iexit+not_trans)/i_start equals the fraction of the entrance covered by capillaries
    # (reference prints both, src/polycap-source.c:1062): calculated 0.6586 for xos1; statistical error ~1e-4
    n_sh = round(np.sqrt(12. * prob.n_cap - 3.) / 6. - 0.5)
    calc = ((n_sh + 0.5) * 6.) ** 2 / 12. * (prob.cap[0] ** 2 * np.pi) / (3. * np.sin(np.pi / 3) * prob.ext[0] ** 2)
    sim = (full["i_exit"] + full["not_transmitted"]) / full["i_start"]
    assert abs(sim - calc) < 2e-3
    # independent seed: efficiencies agree within 5 sigma of the small sample (sigma_rel ~ 1.08/sqrt(N_started))
    sig = 1.08 / np.sqrt(small["i_start"])
    assert abs(small["efficiencies"][0] - full["efficiencies"][0]) / full["efficiencies"][0] < 5 * sig
    assert 35.0 < full["sum_irefl"] / n < 42.0     # reflections per exit photon (SURVEY: 38.3-38.6)


def test_command_line_program(pa, tmp_path):
    """reference src/main.c: deck in, HDF5 result file out; fourth argument 1 switches the leak calculation on"""
    import os
    import subprocess
    from tests.conftest import EXAMPLE, ROOT
    from tests import test_hdf5_writer as H
    exe = os.path.join(ROOT, "polycap_amd", "bin", "polycap")
    out = str(tmp_path / "ellip.h5")
    env = dict(os.environ, POLYCAP_SEED="7")
    r = subprocess.run([exe, os.path.join(EXAMPLE, "ellip_l9.inp"), out, "4", "1", "2000"], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert "Starting calculations" in r.stdout and "iexit: 2000" in r.stdout
    assert os.path.getsize(out) > 2000 * 17 * 8
    if H.H5LS is not None:
        shapes = H._listing(out)
        assert shapes["/PC_Exit/Coordinates"] == (3, 2000) and "/Input/PC_Shape" in shapes
        eff = H._read(out, "/Transmission_Efficiencies", str(tmp_path))
        assert np.all((eff >= 0) & (eff <= 1)) and eff.max() > 0


def _same_photons_weights_to_rounding(g, e, rtol=1e-11):
    """Kernels whose weights live in memory (more than 8 energies, or several on a long profile) evaluate the Fresnel factor
    in FORM 3 of pc_device.h with the hardware reciprocal square root / reciprocal + one Newton step (a few 1e-15 per factor, tests/test_gpu_devmath.py); the
    host compile evaluates the same expressions with IEEE sqrt and division.  The trajectory does not depend on the weights
    (only the "no weight above 1e-4 left" decision does): everything but the weights is identical bit for bit, the weights to
    accumulated rounding."""
    for k in g:
        if k == "weights":
            assert np.all(np.abs(g[k] - e[k]) <= rtol * np.abs(e[k])), (k, np.max(np.abs(g[k] / e[k] - 1.0)))
        else:
            assert np.array_equal(g[k], e[k], equal_nan=True), k


def test_long_profile_uses_the_wide_lds_tables(pa, oracle):
    """Profiles with more than 1024 points (up to 2048) run on the kernels built for the wide LDS pitch: identical to
    the host compile of the device code, for one energy (register weights) and for three (weights in memory), and
    in agreement with the oracle."""
    from tests.emul import pyemul
    from tests.common import TEST_SHAPE, GLASS, synthetic_constants
    from polycap_amd import Problem
    optic = oracle.Optic.from_shape(*TEST_SHAPE, 0.0, 200000, GLASS["density"], nmax=1599)
    source = (2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.5)
    ph = oracle.sample_photons(optic, oracle.make_source(*source), 11, np.arange(20000))
    for energies in ((10.0,), (8.0, 10.0, 12.5)):
        E = np.array(energies)
        amu, scatf = (np.array([PIN_AMU]), np.array([PIN_SCATF])) if len(E) == 1 else synthetic_constants(E)
        prob = Problem(optic.z, optic.cap, optic.ext, 0.0, 200000, GLASS["density"], E, amu, scatf, *source)
        with pa.TraceContext(prob) as ctx:
            g = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
            t = ctx.transmission(5, 0, 50000, keep_images=True)
        e = pyemul.launch_batch(prob, ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        if len(E) == 1:
            for k in g:
                assert np.array_equal(g[k], e[k], equal_nan=True), (energies, k)
        else:
            _same_photons_weights_to_rounding(g, e)
        o = oracle.transmission(optic, oracle.make_source(*source), E, amu, scatf, 5, 0, 50000)
        assert t["i_exit"] == 50000
        assert np.all(np.abs(t["efficiencies"] - o["efficiencies"]) <= 2. / np.sqrt(o["i_start"]) * o["efficiencies"] + 1e-12)


@pytest.mark.parametrize("n_energies", [12, 24, 40, 291])
def test_many_energies_match_the_host_compile(pa, oracle, n_energies):
    """The any-n_energies kernel (weights in memory, cooperative sweeps: 4 photons per pass up to 16 energies, 2 up to 32,
    one beyond; FORM 3 of the Fresnel factor) against the host compile of the device code -- every photon the same, bit for
    bit, except the weights, which agree to rounding -- and the driver against the oracle."""
    from tests.emul import pyemul
    energies = np.linspace(3.0, 30.0, n_energies)
    optic, src, prob, (E, A, S) = make_pair(oracle, "xos1", energies=energies)
    ph = _photons(oracle, optic, src, 6000, seed=3)
    with pa.TraceContext(prob) as ctx:
        g = ctx.launch_photons(ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
        t = ctx.transmission(9, 0, 20000, keep_images=True)
    e = pyemul.launch_batch(prob, ph[:, 0:3], ph[:, 3:6], ph[:, 6:9])
    _same_photons_weights_to_rounding(g, e)
    o = oracle.transmission(optic, src, E, A, S, 9, 0, 20000)
    assert t["i_exit"] == 20000
    assert np.all(np.abs(t["efficiencies"] - o["efficiencies"]) <= 1.5 / np.sqrt(o["i_start"]) * o["efficiencies"] + 1e-12), \
        (np.abs(t["efficiencies"] / o["efficiencies"] - 1.0) * np.sqrt(o["i_start"])).max()
    w = t["exit_weights"]
    assert w.shape == (20000, n_energies) and np.all((w >= 0) & (w <= 1)) and np.all(w.max(axis=1) >= 1e-4)
    # checksum of checksums: the per-slot weights add up to the exact fixed-point totals, energy by energy
    for k in (0, n_energies // 2, n_energies - 1):
        tot = int(t["sumw_fixed"][k, 0]) + (int(t["sumw_fixed"][k, 1]) << 64)
        assert sum(int(x) for x in np.floor(w[:, k] * 4611686018427387904.0).astype(np.uint64)) == tot


def test_pool_and_producer_kernels_are_bit_identical(pa, oracle):
    """Options "pool" (photons parked in LDS are exchanged between lanes, pc_pool_kernel.h: the default for single-energy
    source runs up to v14) and "producer" (a launching wave per workgroup hands launched photons to the tracing waves
    through LDS rings, pc_producer_kernel.h: chosen automatically for long-lived photons).  A photon depends on
    (seed, slot, attempt) only and the sums are exact, so totals and every image plane equal those of the
    one-photon-per-lane kernel."""
    from tests.common import make_custom, MONO_CASE, SEVEN_CASE
    probs = [make_pair(oracle, "xos1")[2], make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))[2],
             make_custom(oracle, **MONO_CASE)[2], make_custom(oracle, **SEVEN_CASE)[2]]
    for k, prob in enumerate(probs):
        for n, max_attempts in ((60000, 1 << 20), (37, 1 << 20), (3000, 2)):
            with pa.TraceContext(prob) as ctx:
                res = {}
                for name, pool, producer in (("lane", 0, 0), ("pool", 1, 0), ("producer", 0, 1)):
                    ctx.set_option("pool", pool)
                    ctx.set_option("producer", producer)
                    ctx.run(31 + k, 1000, n, max_attempts=max_attempts, keep_images=True)
                    ctx.wait()
                    r = ctx.totals(check=False)
                    r.update(ctx.images(0, n))
                    assert ctx.last_kernel() == {"lane": "pc_trace_kernel", "pool": "pc_trace_pool_kernel", "producer": "pc_trace_producer_kernel"}[name]
                    st = ctx.phase_stats()
                    # (the production instantiation of the launching-wave kernel leaves the march counters alone: option march_stats)
                    assert st["event"]["phases"] > 0 and (name == "producer" or st["march"]["phases"] > 0)
                    res[name] = r
            a = res["lane"]
            done = a["exit_weights"][:, 0] > 0        # a slot that ran out of attempts has weight 0 and no defined exit planes
            for name in ("pool", "producer"):
                b = res[name]
                assert np.array_equal(a["counters"], b["counters"]) and np.array_equal(a["sumw_fixed"], b["sumw_fixed"]), (name, k, n)
                assert np.array_equal(a["exit_weights"], b["exit_weights"]), (name, k, n)
                assert np.array_equal(a["images"][done], b["images"][done], equal_nan=True), (name, k, n)
                assert np.array_equal(a["images"][~done, :8], b["images"][~done, :8], equal_nan=True), (name, k, n)
            if max_attempts == 2:
                assert a["failed_slots"] > 0 and not done.all()


def test_logged_reflections_equal_the_immediate_sweep(pa):
    """Beyond 8 energies a source run logs its reflections (24 B each) and sweeps a photon's weights once per log, the photon
    flying on meanwhile (pc_trace_log_kernel, option batch_reflections, default on).  On the C3 deck counters, exact sums, every
    exit weight and every image plane equal those of the immediate sweep bit for bit, with images kept and -- where weights below
    2^-64 are no longer multiplied -- in histogram-only runs, for several log capacities.  On the C5 deck with roughness the
    logging kernel applies a log's roughness factors as one exponential: photons and planes identical, weights to 1e-13."""
    import os
    from tests.conftest import EXAMPLE
    for deck, sig, n in (("xos1", None, 40000), ("ellip_l9", 5.0, 30000)):
        prob = pa.problem_from_inp(os.path.join(EXAMPLE, deck + ".inp"), sig_rough=sig)
        assert prob.n_energies == 291
        with pa.TraceContext(prob) as ctx:
            ctx.set_option("batch_reflections", 0)
            a = ctx.transmission(77, 0, n, keep_images=True)
            assert ctx.last_kernel() == "pc_trace_kernel"
            ctx.set_option("batch_reflections", 1)
            for cap, keep in ((64, True), (64, False), (5, True), (200, False)):
                ctx.set_option("log_cap", cap)
                b = ctx.transmission(77, 0, n, keep_images=keep)
                assert ctx.last_kernel() == "pc_trace_log_kernel"
                st = ctx.sweep_stats()
                assert st["passes"] > 0 and st["iterations"] > 0 and 0. < st["ct_tame"] < 1e-9
                assert np.array_equal(a["counters"][:6], b["counters"][:6]), (deck, cap, keep)
                if sig is None:
                    assert np.array_equal(a["sumw_fixed"], b["sumw_fixed"]), (deck, cap, keep)
                else:
                    assert np.abs(b["sum_weights"] / a["sum_weights"] - 1.0).max() < 1e-14, (deck, cap, keep)
                if keep:
                    assert np.array_equal(a["images"], b["images"], equal_nan=True), (deck, cap)
                    if sig is None:
                        assert np.array_equal(a["exit_weights"], b["exit_weights"]), (deck, cap)
                    else:
                        assert np.nanmax(np.abs(b["exit_weights"] - a["exit_weights"]) / a["exit_weights"]) < 1e-13, (deck, cap)


def test_logged_reflections_over_the_range_of_energy_counts(pa):
    """The logging kernel serves every energy count above 8 whose sums and constants leave room in LDS for one log per wave: 9
    and 20 (a sweep round gathers several photons to fill a pass of 64 lanes), 33, 449 (the immediate kernel's constants no longer
    fit in LDS there, it reads them from memory), 1000 (the log capacity is halved to fit beside 56 KB of sums and constants).
    Counters and exact sums equal the immediate sweep's; images kept at 9, 20 and 1000; option log_min_energies restores the
    immediate sweep below a count."""
    import os
    from tests.conftest import EXAMPLE
    for ne in (9, 20, 33, 449, 1000):
        prob = pa.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"), energies=np.linspace(2.0, 40.0, ne))
        with pa.TraceContext(prob) as ctx:
            keep = ne in (9, 20, 1000)
            ctx.set_option("batch_reflections", 0)
            a = ctx.transmission(5, 3, 12000, keep_images=keep)
            assert ctx.last_kernel() == "pc_trace_kernel"
            ctx.set_option("batch_reflections", 1)
            b = ctx.transmission(5, 3, 12000, keep_images=keep)
            assert ctx.last_kernel() == "pc_trace_log_kernel", ne
            assert np.array_equal(a["counters"][:6], b["counters"][:6]), ne
            assert np.array_equal(a["sumw_fixed"], b["sumw_fixed"]), ne
            if keep:
                assert np.array_equal(a["exit_weights"], b["exit_weights"])
                assert np.array_equal(a["images"], b["images"], equal_nan=True)
            if ne == 20:
                ctx.set_option("log_min_energies", 21)
                c = ctx.transmission(5, 3, 12000, keep_images=keep)
                assert ctx.last_kernel() == "pc_trace_kernel"
                assert np.array_equal(a["sumw_fixed"], c["sumw_fixed"]) and np.array_equal(a["images"], c["images"], equal_nan=True)


def test_logged_reflections_with_photons_that_die(pa, oracle):
    """The logging kernel on grids whose photons are absorbed (10-30 keV: every energy falls below 1e-4 within a few steep
    reflections): the lane's proxy energy triggers the sweep that ends the photon where the immediate sweep ends it -- counters
    (not_transmitted included), sums and planes identical; and a run against the oracle."""
    energies = np.linspace(10.0, 30.0, 40)
    optic, src, prob, (E, A, S) = make_pair(oracle, "xos1", energies=energies)
    with pa.TraceContext(prob) as ctx:
        ctx.set_option("batch_reflections", 0)
        a = ctx.transmission(5, 0, 60000, keep_images=True)
        ctx.set_option("batch_reflections", 1)
        b = ctx.transmission(5, 0, 60000, keep_images=True)
        assert ctx.last_kernel() == "pc_trace_log_kernel"
        c = ctx.transmission(5, 0, 60000)
    assert a["not_transmitted"] > 1000
    for r in (b, c):
        assert np.array_equal(a["counters"][:6], r["counters"][:6]) and np.array_equal(a["sumw_fixed"], r["sumw_fixed"])
    assert np.array_equal(a["exit_weights"], b["exit_weights"]) and np.array_equal(a["images"], b["images"], equal_nan=True)
    # an elliptical, divergent, shifted source (the generic sampling path: pc_trace_log_kernel<PC_MODE_SRC_GENERIC>) and uniform illumination
    for source in ((2000., 0.2065, 0.1, 0., 0., 0.01, -0.02, 0.9), (5., 0.01, 0.01, -1., 0., 0., 0., 0.0)):
        _, _, p2, _ = make_pair(oracle, "ellip", energies=np.linspace(6.0, 30.0, 48), source=source)
        with pa.TraceContext(p2) as ctx:
            ctx.set_option("batch_reflections", 0)
            a2 = ctx.transmission(3, 7, 20000, keep_images=True)
            ctx.set_option("batch_reflections", 1)
            b2 = ctx.transmission(3, 7, 20000, keep_images=True)
            assert ctx.last_kernel() == "pc_trace_log_kernel"
            c2 = ctx.transmission(3, 7, 20000)
        for r in (b2, c2):
            assert np.array_equal(a2["counters"][:6], r["counters"][:6]) and np.array_equal(a2["sumw_fixed"], r["sumw_fixed"]), source
        assert np.array_equal(a2["exit_weights"], b2["exit_weights"]) and np.array_equal(a2["images"], b2["images"], equal_nan=True), source
    o = oracle.transmission(optic, src, E, A, S, 5, 0, 20000)
    with pa.TraceContext(prob) as ctx:
        t = ctx.transmission(5, 0, 20000)
        # slots that use up their attempts (two per slot here): the same failed slots, counters and sums from both kernels, with the
        # slot-ordered image store and with the compact one (whose positions behind the cursor are zeroed)
        res = {}
        for b in (0, 1):
            ctx.set_option("batch_reflections", b)
            ctx.run(9, 100, 30000, max_attempts=2, keep_images=True)
            ctx.wait()
            res[b] = (ctx.totals(check=False), ctx.images(0, 30000))
        assert res[0][0]["failed_slots"] > 1000
        assert np.array_equal(res[0][0]["counters"], res[1][0]["counters"]) and np.array_equal(res[0][0]["sumw_fixed"], res[1][0]["sumw_fixed"])
        done = res[0][1]["exit_weights"].max(axis=1) > 0
        assert np.array_equal(done, res[1][1]["exit_weights"].max(axis=1) > 0)
        assert np.array_equal(res[0][1]["exit_weights"], res[1][1]["exit_weights"])
        assert np.array_equal(res[0][1]["images"][done], res[1][1]["images"][done], equal_nan=True)
        ctx.set_option("plane_images", 1)
        ctx.set_option("compact_images", 1)
        ctx.run(9, 100, 30000, max_attempts=2, keep_images=True)
        ctx.wait()
        tc = ctx.totals(check=False)
        pl = ctx.image_planes(0, 30000)
        assert np.array_equal(tc["counters"], res[1][0]["counters"]) and np.array_equal(tc["sumw_fixed"], res[1][0]["sumw_fixed"])
        n_ok = int(tc["i_exit"])
        assert n_ok == int(done.sum()) and np.all(pl["exit_weights"][n_ok:] == 0.) and np.all(pl["planes"][:, n_ok:] == 0.)
        assert np.all(pl["exit_weights"][:n_ok].max(axis=1) >= 1e-4)
    assert np.all(np.abs(t["efficiencies"] - o["efficiencies"]) <= 1.5 / np.sqrt(o["i_start"]) * o["efficiencies"] + 1e-12)
    assert abs(t["not_transmitted"] - o["not_transmitted"]) <= 4 * np.sqrt(o["not_transmitted"])


def test_kernel_choice_by_photon_lifetime(pa, oracle, monkeypatch):
    """Option "producer" = -1 (default): a context's first big run is preceded by a small probe with the default kernel; the
    launching-wave kernel then traces optics whose photons reflect often (xos1) and the default kernel the others."""
    monkeypatch.delenv("POLYCAP_PRODUCER", raising=False)      # the suite may run with the kernel forced: this test is about the choice
    _, _, prob, _ = make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))
    with pa.TraceContext(prob) as ctx:
        small = ctx.transmission(5, 0, 100_000)
        assert ctx.last_kernel() == "pc_trace_producer_kernel" or ctx.last_kernel() == "pc_trace_kernel"
        first = ctx.last_kernel()
        big = ctx.transmission(5, 0, 2_100_000)
        assert ctx.last_kernel() == "pc_trace_producer_kernel"
        ctx.set_option("producer", 0)
        ref = ctx.transmission(5, 0, 2_100_000)
        assert ctx.last_kernel() == "pc_trace_kernel"
    assert first == "pc_trace_kernel"                  # nothing known yet, and too small for a probe
    assert np.array_equal(big["counters"], ref["counters"]) and np.array_equal(big["sumw_fixed"], ref["sumw_fixed"])


def test_image_fetch_paths_agree_on_a_multi_energy_run(pa, oracle):
    """Records (pc_hip_transmission_records) and SoA planes (pc_hip_transmission_images, fetched before wait() from a run
    cut into parts) carry the same data, weights of 7 energies included; sizes above the threaded-pipeline threshold."""
    optic, src, prob, _ = make_pair(oracle, "ellip", energies=(5.0, 8.0, 11.0, 14.0, 17.0, 20.0, 25.0))
    n = 200000
    with pa.TraceContext(prob) as ctx:
        a = ctx.transmission(3, 11, n, keep_images=True)
        ctx.set_option("run_parts", 3)
        ctx.set_option("fetch_threads", 5)
        ctx.run(3, 11, n, keep_images=True)
        p = ctx.image_planes(0, n)
        ctx.wait()
        b = ctx.totals()
        r = ctx.images(100, n - 300)
    assert np.array_equal(a["images"], p["planes"].T, equal_nan=True) and np.array_equal(a["exit_weights"], p["exit_weights"])
    assert np.array_equal(a["images"][100:n - 200], r["images"], equal_nan=True)
    assert np.array_equal(a["exit_weights"][100:n - 200], r["exit_weights"])
    assert np.array_equal(a["counters"][:4], b["counters"][:4]) and np.array_equal(a["sumw_fixed"], b["sumw_fixed"])


@pytest.mark.parametrize("deck, sig_rough, n", [("xos1", None, 100_000_000), ("ellip_l9", 5.0, 20_000_000)])
def test_energy_sweep_properties_at_scale(pa, deck, sig_rough, n):
    """BASELINE configs C3 (xos1, 1e8 exit photons: full size) and C5 (ellip_l9 with 5 A roughness; 2e7 of its 1.25e8 per GPU) on
    the decks' own 291-energy grid 1-30 keV, histogram only as at
    those sizes (the weight plane alone would be 233 GB at 1e8 photons): exact additivity of the per-energy sums over a
    partition of the slot range, the same photons as a single-energy run (geometry does not depend on the energy grid),
    a transmission curve that falls with energy above 10 keV, and agreement with an independent sample."""
    import os
    from tests.conftest import EXAMPLE
    path = os.path.join(EXAMPLE, deck + ".inp")
    prob = pa.problem_from_inp(path, sig_rough=sig_rough)
    ne = prob.n_energies
    assert ne == 291
    cut = n // 3 + 1
    with pa.TraceContext(prob) as ctx:
        full = ctx.transmission(77, 0, n)
        parts = [ctx.transmission(77, 0, cut), ctx.transmission(77, cut, n - cut)]
        other = ctx.transmission(78, 0, 300_000)
    assert full["i_exit"] == n and full["failed_slots"] == 0
    assert np.array_equal(full["counters"][:4], parts[0]["counters"][:4] + parts[1]["counters"][:4])
    for e in range(ne):
        lo = sum(int(p["sumw_fixed"][e, 0]) for p in parts)
        hi = sum(int(p["sumw_fixed"][e, 1]) for p in parts) + (lo >> 64)
        assert (lo & (2**64 - 1), hi) == (int(full["sumw_fixed"][e, 0]), int(full["sumw_fixed"][e, 1])), e
    eff = full["efficiencies"]
    E = np.asarray(prob.energies)
    assert np.all((eff > 0) & (eff < 1))
    hiE = E >= 10.0
    assert np.all(np.diff(eff[hiE]) < 0)                     # harder photons reflect worse: strictly falling curve
    assert eff[E == 1.0][0] > 3 * eff[-1]
    # independent seed: the curves agree within the statistical error of the smaller sample (sigma_rel ~ 1.1/sqrt(N_started)
    # at 10 keV = 0.2 %; the spread of the weights, hence the error, grows with energy: 1 % observed at 30 keV)
    assert np.all(np.abs(other["efficiencies"] / eff - 1.0) < 0.03)
    assert np.all(np.abs(other["efficiencies"] / eff - 1.0)[E <= 10.0] < 5 * 1.1 / np.sqrt(other["i_start"]))
    # the photons of a sweep are the photons of a single-energy run at the lowest energy as long as that weight decides
    # survival: started / entered counts depend on geometry only, so they equal those of any other energy grid
    one = pa.problem_from_inp(path, energies=[float(E[0])], sig_rough=sig_rough)
    with pa.TraceContext(one) as ctx:
        single = ctx.transmission(77, 0, 200_000)
    with pa.TraceContext(prob) as ctx:
        sweep = ctx.transmission(77, 0, 200_000)
    assert sweep["not_entered"] == single["not_entered"]


def test_c5_deck_roughness_vs_oracle(pa, oracle):
    """BASELINE config C5 on the deck itself: example/ellip_l9.inp, its 291-point grid, sig_rough = 5 (Angstrom, the unit
    of the reference: include/polycap-description.h:45, example/dub_foc.inp:1; used raw at src/polycap-capil.c:626).
    The driver against the oracle on identical seeds, and the roughness must cost transmission -- a unit slip
    (5e-8 "cm") makes exp(-(1.01358 E alpha sigma)^2) == 1 and fails here."""
    import os
    from tests.conftest import EXAMPLE
    path = os.path.join(EXAMPLE, "ellip_l9.inp")
    rough = pa.problem_from_inp(path, sig_rough=5.0)
    smooth = pa.problem_from_inp(path)
    assert rough.n_energies == 291 and smooth.sig_rough == 0.0 and rough.sig_rough == 5.0
    n = 20000
    with pa.TraceContext(rough) as ctx:
        g = ctx.transmission(77, 0, n)
        g10 = ctx.transmission(78, 0, 400_000)
    with pa.TraceContext(smooth) as ctx:
        s10 = ctx.transmission(78, 0, 400_000)
    E = np.asarray(rough.energies)
    k10 = int(np.argmin(np.abs(E - 10.0)))
    # survey probe of the compiled reference: 0.1256 with 5 A against 0.1345 without at 10 keV, -6.6 %
    ratio = g10["efficiencies"] / s10["efficiencies"]
    assert 0.90 < ratio[k10] < 0.96, ratio[k10]
    assert np.all(ratio[E >= 3.0] < 0.995) and np.all(np.diff(ratio[(E >= 5.0) & (E <= 20.0)]) < 2e-3)
    assert abs(g10["efficiencies"][k10] - 0.1256) < 0.004 and abs(s10["efficiencies"][k10] - 0.1345) < 0.004
    optic = oracle.Optic(rough.z, rough.cap, rough.ext, 5.0, rough.n_cap, rough.density)
    o = oracle.transmission(optic, oracle.make_source(*rough.source), rough.energies, rough.amu, rough.scatf, 77, 0, n)
    assert g["i_exit"] == n == o["i_exit"]
    tol = 1.5 / np.sqrt(o["i_start"])
    assert abs(g["i_start"] - o["i_start"]) / o["i_start"] < tol
    lo = E <= 15.0          # beyond, a handful of photons carry the sum and the relative error grows (1 % at 30 keV)
    assert np.all(np.abs(g["efficiencies"] / o["efficiencies"] - 1.0)[lo] < tol)
    assert np.all(np.abs(g["efficiencies"] / o["efficiencies"] - 1.0) < 0.05)


def test_device_group_is_bit_identical_to_one_device(pa, oracle):
    """pc_hip_group_*: the slot range sharded over several device contexts of one process (the same GPU listed more than
    once on a one-GPU box) gives the totals and every image plane of the single-context run, bit for bit; the totals of
    a one-device group summed through RCCL (ncclCommInitAll + ncclAllReduce of the 32-bit limbs) equal the host sum."""
    optic, src, prob, _ = make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))
    n = 300_001
    with pa.TraceContext(prob) as ctx:
        one = ctx.transmission(41, 0, n, keep_images=True)
    for devices in ([0, 0], [0, 0, 0]):
        with pa.TraceGroup(prob, devices) as grp:
            g = grp.transmission(41, n, keep_images=True)
        assert not g["reduced_by_rccl"]                 # a device twice: host limb sum
        assert np.array_equal(g["counters"][:4], one["counters"][:4]) and np.array_equal(g["sumw_fixed"], one["sumw_fixed"])
        assert np.array_equal(g["images"], one["images"], equal_nan=True) and np.array_equal(g["exit_weights"], one["exit_weights"])
        assert np.array_equal(g["efficiencies"], one["efficiencies"])
    with pa.TraceGroup(prob, [0]) as grp:
        r = grp.transmission(41, n, reduce=1)           # RCCL or fail: a communicator of one rank
        h = grp.transmission(41, n, reduce=0)
    assert r["reduced_by_rccl"] and not h["reduced_by_rccl"]
    assert np.array_equal(r["counters"], h["counters"]) and np.array_equal(r["sumw_fixed"], h["sumw_fixed"])
    assert np.array_equal(r["sumw_fixed"], one["sumw_fixed"])
    # seven energies: the limb vector has 6 + 4 x 7 entries
    optic, src, prob7, _ = make_pair(oracle, "ellip", energies=(5.0, 8.0, 11.0, 14.0, 17.0, 20.0, 25.0))
    with pa.TraceContext(prob7) as ctx:
        one7 = ctx.transmission(3, 0, 50_000)
    with pa.TraceGroup(prob7, [0]) as grp:
        r7 = grp.transmission(3, 50_000, reduce=1)
    with pa.TraceGroup(prob7, [0, 0]) as grp:
        h7 = grp.transmission(3, 50_000)
    assert np.array_equal(r7["sumw_fixed"], one7["sumw_fixed"]) and np.array_equal(h7["sumw_fixed"], one7["sumw_fixed"])
    assert np.array_equal(r7["counters"][:4], one7["counters"][:4]) and np.array_equal(h7["counters"][:4], one7["counters"][:4])


def test_device_group_members_share_one_probe_and_enqueue_concurrently(pa):
    """BASELINE C2 over a device list as the 8-GPU node would run it (here [0, 0, 0, 0] on the one GPU: 4 x 1.25e6 slots, each
    below the size from which a context probes by itself): one probe decides the kernel for every member -- the launching-wave
    kernel on xos1 --, the members are enqueued from host threads without a blocking call between them (the enqueue returns in
    under a millisecond), and the whole run costs what one context needs for the same slots plus the start and the drain of
    three more launches (the members' kernels follow each other on the one GPU, ~1.2 ms each; on distinct GPUs they run side by
    side: measured 11.5 ms for one context, 15.1 ms for four members)."""
    import os
    import time
    from tests.conftest import EXAMPLE
    prob = pa.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"), energies=[10.0])
    n = 5_000_000
    with pa.TraceContext(prob) as ctx:
        ctx.transmission(1, 0, n)                      # warm-up: probe + kernel choice
        t0 = time.perf_counter()
        one = ctx.transmission(7, 0, n)
        t_one = time.perf_counter() - t0
        assert ctx.last_kernel() == "pc_trace_producer_kernel"
    with pa.TraceGroup(prob, [0, 0, 0, 0]) as grp:
        grp.transmission(1, n)                         # warm-up: the group's one probe
        assert grp.last_kernels() == ["pc_trace_producer_kernel"] * 4
        t0 = time.perf_counter()
        g = grp.transmission(7, n)
        t_grp = time.perf_counter() - t0
        assert grp.last_kernels() == ["pc_trace_producer_kernel"] * 4
    assert np.array_equal(g["counters"][:4], one["counters"][:4]) and np.array_equal(g["sumw_fixed"], one["sumw_fixed"])
    print("one context %.2f ms, four members %.2f ms, enqueue of the four members %.3f ms" % (t_one * 1e3, t_grp * 1e3, grp.enqueue_s * 1e3))
    assert grp.enqueue_s < 1e-3, grp.enqueue_s
    assert t_grp <= 1.15 * t_one + 3 * 1.5e-3, (t_grp, t_one)


def test_c_api_multi_device_and_histogram_only(pa, monkeypatch):
    """polycap_source_get_transmission_efficiencies with POLYCAP_HIP_DEVICES (the photon loop sharded over a device list,
    reference src/polycap-source.c:697-745, totals summed as :973-980) and POLYCAP_IMAGES=0 (histogram-only result):
    two "devices" equal one bit for bit through the public C API, and BASELINE C3 at its full size (xos1.inp, 291
    energies, 1e8 exit photons: 233 GB of weights with images) runs through the drop-in call."""
    import os
    from polycap_amd import capi
    from tests.conftest import EXAMPLE
    monkeypatch.setenv("POLYCAP_SEED", "77")
    src = capi.Source.new_from_file(os.path.join(EXAMPLE, "xos1.inp"))

    def run(n, **env):
        for k in ("POLYCAP_HIP_DEVICES", "POLYCAP_IMAGES", "POLYCAP_RCCL", "POLYCAP_COMPACT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return src.get_transmission_efficiencies(-1, n)

    a = run(200_000)
    b = run(200_000, POLYCAP_HIP_DEVICES="0,0")
    c = run(200_000, POLYCAP_HIP_DEVICES="0", POLYCAP_RCCL="1")
    assert np.array_equal(a.data[1], b.data[1]) and np.array_equal(a.data[1], c.data[1])
    # the public call stores exit photons in the order of completion (compact store): the same photons, bit for bit, in another
    # order -- put both in the order of the path length (distinct doubles) before comparing
    ia, ib = np.argsort(a.d_travel, kind="stable"), np.argsort(b.d_travel, kind="stable")
    assert np.array_equal(a.exit_weights[ia], b.exit_weights[ib]) and np.array_equal(a.n_refl[ia], b.n_refl[ib])
    assert np.array_equal(a.d_travel[ia], b.d_travel[ib])
    # POLYCAP_COMPACT=0: every photon at the position of its slot, so even the order is the same
    a0, b0 = run(200_000, POLYCAP_COMPACT="0"), run(200_000, POLYCAP_HIP_DEVICES="0,0", POLYCAP_COMPACT="0")
    assert np.array_equal(a0.exit_weights, b0.exit_weights) and np.array_equal(a0.d_travel, b0.d_travel)
    i0 = np.argsort(a0.d_travel, kind="stable")
    assert np.array_equal(a0.exit_weights[i0], a.exit_weights[ia]) and np.array_equal(a0.n_refl[i0], a.n_refl[ia])
    del a0, b0
    h = run(200_000, POLYCAP_HIP_DEVICES="0,0", POLYCAP_IMAGES="0")
    assert np.array_equal(a.data[1], h.data[1])
    with pytest.raises(ValueError):
        h.exit_weights                                    # no per-photon planes in a histogram-only result
    del a, b, c, h
    # C3 at full size through the drop-in call, against the thin-ABI run of the same streams
    full = run(100_000_000, POLYCAP_HIP_DEVICES="0,0", POLYCAP_IMAGES="0")
    E, eff = full.data
    assert len(E) == 291 and np.all((eff > 0) & (eff < 1)) and np.all(np.diff(eff[E >= 10.0]) < 0)
    prob = pa.problem_from_inp(os.path.join(EXAMPLE, "xos1.inp"))
    with pa.TraceContext(prob) as ctx:
        t = ctx.transmission(77, 0, 100_000_000)
    assert np.array_equal(eff, t["efficiencies"])


def test_reference_loop_check_get_photon_launch_vs_driver(pa, known):
    """The reference's own consistency check of the path (tests/source.c:306-340, tests/python.py:279-301): a hand-rolled
    loop of polycap_source_get_photon(rng seeded 20000) + polycap_photon_launch through the public API until 30000
    photons are transmitted, against the curve of polycap_source_get_transmission_efficiencies, within 0.0075 at all
    seven energies.  Every iteration is two C-API calls = two kernel launches on one photon (that is what the API is):
    the loop is bounded to a minute, the measured per-photon latency is printed."""
    import time
    from polycap_amd import capi
    t = known["transmission_curve"]
    prof = capi.Profile(capi.Profile.ELLIPSOIDAL, 9., 0.2065, 0.0585, 0.00035, 9.9153e-5, 1000., 0.5)
    desc = capi.Description(prof, 0.0, 200000, {"O": 53.0, "Si": 47.0}, 2.23)
    energies = np.array(t["energies"], dtype=np.float64)
    src = capi.Source(desc, t["d_source"], t["src_x"], t["src_y"], t["src_sigx"], t["src_sigy"], t["src_shiftx"],
                      t["src_shifty"], t["hor_pol"], energies)
    eff = src.get_transmission_efficiencies(-1, 30000)
    curve = eff.data[1]
    rng = capi.Rng(20000)
    w_tot = np.zeros(7)
    phot_ini = phot_transm = 0
    t0 = time.perf_counter()
    while phot_transm < 30000:
        photon = src.get_photon(rng)
        try:
            w = photon.launch(energies)
        except ValueError:          # return code -2: not in the entrance window (tests/source.c:329)
            continue
        phot_ini += 1
        if w is not None:
            assert np.all((w >= 0.) & (w <= 1.))
            w_tot += w
            phot_transm += 1
        assert time.perf_counter() - t0 < 120., "the per-photon API loop is too slow"
    dt = time.perf_counter() - t0
    w_tot /= phot_ini
    print("loop check: %d launched, %d transmitted in %.1f s (%.0f us per get_photon + launch); loop %s driver %s"
          % (phot_ini, phot_transm, dt, 1e6 * dt / phot_ini, np.round(w_tot, 4), np.round(curve, 4)))
    assert np.all(np.abs(curve - w_tot) <= 0.0075)


def test_c_client_of_the_drop_in_api(pa, tmp_path):
    """tests/c/dropin_client.c -- a C program against include/polycap.h as a user of the reference would write it -- linked
    to libpolycap.so: the reference's seven-energy curve, getter sanity checks, launch return codes, the get_photon+launch
    loop against the driver and the error convention (reference tests/source.c, tests/photon.c)."""
    import os
    import subprocess
    from tests.test_abi_symbols import build_dropin_client
    exe = build_dropin_client(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, POLYCAP_OPTCONST="builtin", POLYCAP_SEED="20000"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "all checks passed" in r.stdout


def test_plane_images_equal_records(pa, oracle):
    """Option "plane_images" (what polycap_source_get_transmission_efficiencies uses): the kernels store the planes of
    struct _polycap_images themselves and the fetch is a copy of planes into the caller's pinned arrays.  Same bits as the
    record store, for one energy (pool kernel), seven (register weights) and twelve (weights in memory), whole and in
    parts, full and partial fetches; the record fetch refuses a plane run.  Every run of 3 parts is big enough to be traced as
    three launches (a run is cut into at most n_slots / 65536)."""
    cases = [make_pair(oracle, "xos1", source=(2000., 0.2065, 0.2065, 0., 0., 0., 0., 0.0))[2],
             make_pair(oracle, "ellip", energies=(5.0, 8.0, 11.0, 14.0, 17.0, 20.0, 25.0))[2],
             make_pair(oracle, "xos1", energies=np.linspace(3.0, 30.0, 12))[2]]
    for prob in cases:
        n = 300_000 if prob.n_energies == 1 else 200_000
        assert n >= 3 * 65536
        with pa.TraceContext(prob) as ctx:
            ctx.run(13, 7, n, keep_images=True)
            ref = ctx.image_planes(0, n)
            rt = ctx.totals()
            for parts in (1, 3):
                ctx.set_option("plane_images", 1)
                ctx.set_option("run_parts", parts)
                ctx.run(13, 7, n, keep_images=True)
                p = ctx.image_planes(0, n)
                q = ctx.image_planes(1001, n - 5000)
                t = ctx.totals()
                with pytest.raises(pa.HipError):
                    ctx.images(0, 10)
                ctx.set_option("plane_images", 0)
                ctx.set_option("run_parts", 1)
                assert np.array_equal(p["planes"], ref["planes"], equal_nan=True) and np.array_equal(p["exit_weights"], ref["exit_weights"])
                assert np.array_equal(p["nrefl"], ref["nrefl"])
                assert np.array_equal(q["planes"], ref["planes"][:, 1001:n - 3999], equal_nan=True)
                assert np.array_equal(q["exit_weights"], ref["exit_weights"][1001:n - 3999])
                assert np.array_equal(t["counters"][:4], rt["counters"][:4]) and np.array_equal(t["sumw_fixed"], rt["sumw_fixed"])

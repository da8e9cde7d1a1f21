"""The device's fast arithmetic (pc_device.h, PC_FAST_MATH_DEVICE: v_rsq_f64 / v_rcp_f64 + one Newton step, the exp polynomial)
and the Fresnel forms built on it, element by element on the MI355X (tests/devmath/probe.hip) against exact values (mpmath,
tests/devmath/exact.py) and against the host compile of the same calls.  Every measured maximum is printed (run with -s)."""
import os
import re

import numpy as np
import pytest

from tests.devmath import exact, grid, pyprobe
from tests.test_devmath_cpu import EPS, K_HOST, exact_form, form_errors, form_inputs

pytestmark = pytest.mark.gpu

SQRT_DIV_TOL = 8e-15     # pc_sqrt_fast, pc_div_fast: relative
EXP_TOL = 1e-14          # pc_exp_neg_fast where exp(x) is normal: relative
# where exp(x) is subnormal the result carries the polynomial's relative error (EXP_TOL) plus the final rounding to a multiple of
# 2^-1074: an absolute 2^-1074 alone cannot hold near 2^-1022, where 1e-14 relative is 45 units of 2^-1074 (measured: 55)
SUBNORMAL_ULP = 2.0 ** -1074
# the device forms: the host's K (test_devmath_cpu.K_HOST) plus the two roots and the reciprocal after their Newton steps, which
# enter R like roundings of its inputs (measured: K up to 19.4 for FORMs 3/3s; FORMs 0/1 use IEEE operations on the device too)
K_DEVICE = {op: k + 20.0 for op, k in K_HOST.items()}
# device against the host compile of the same form: within both forms' bounds everywhere, and within DEV_HOST_REL where R >= 1e-6
# and the form is well conditioned (R + cond <= WELL R).  Near the critical angle the roots' 2^-48 is amplified like any input
# rounding: there the two differ by up to 2.1e-12 relative (measured)
DEV_HOST_REL = 2e-14
WELL = 6.0
CODE_MARGIN = 1e-12      # return codes are compared where the exact value is this far from 0, 1 and the 1e-4 threshold


def _run(p, op, e, x):
    return pyprobe.run(p, op, e, x, device=True)


def test_sqrt_and_div_fast():
    """pc_sqrt_fast and pc_div_fast over normal inputs 2^-200 ... 2^64 and over the values FORM 3 feeds them (|z|^2, Q, Ds Dp)."""
    p = grid.problem("synthetic")
    rng = np.random.default_rng(11)
    x = np.ldexp(1.0 + rng.random(20000), rng.integers(-200, 64, 20000))
    x = np.concatenate([x, [2.0 ** -200, 2.0 ** 64, 1.0, 2.0, 0.5, np.nextafter(1.0, 0.), np.nextafter(1.0, 2.)]])
    # what the forms take roots of: |z|^2 = (c^2 - d2)^2 + zi2 and Q = |z| + |c^2 - d2|, over the grid's energies and cosines
    ec = pyprobe.energy_consts(p)
    c = grid.log_grid(-16, 0, 16)
    zr = (c[None, :] ** 2 - ec["d2"][:, None]).ravel()
    m2 = zr * zr + np.repeat(ec["zi2"], c.size)
    x = np.concatenate([x, m2, np.sqrt(m2) + np.abs(zr)])
    y, _ = _run(p, "sqrt", 0, pyprobe.rows(x.size, c=x))
    err = np.array([exact.sqrt_rel_err(a, b) for a, b in zip(x, y[:, 0])])
    print("pc_sqrt_fast: max rel err %.2e over %d inputs (at %r)" % (err.max(), x.size, x[np.argmax(err)]))
    assert err.max() <= SQRT_DIV_TOL

    a = np.ldexp(1.0 + rng.random(20000), rng.integers(-100, 32, 20000))
    b = np.ldexp(1.0 + rng.random(20000), rng.integers(-100, 32, 20000))
    # denominators of FORM 3: Ds Dp from 1e-60 to 1e2
    b = np.concatenate([b, 10.0 ** rng.uniform(-60, 2, 5000)])
    a = np.concatenate([a, rng.random(5000) * b[-5000:]])
    y, _ = _run(p, "div", 0, pyprobe.rows(a.size, c=a, st2=b))
    err = np.array([exact.div_rel_err(u, v, w) for u, v, w in zip(a, b, y[:, 0])])
    print("pc_div_fast: max rel err %.2e over %d inputs (at %r / %r)" % (err.max(), a.size, a[np.argmax(err)], b[np.argmax(err)]))
    assert err.max() <= SQRT_DIV_TOL


def _exp_inputs():
    k = np.arange(0, 1076)
    bnd = -(k + 0.5) * np.log(2.0)
    near = np.concatenate([bnd, np.nextafter(bnd, -np.inf), np.nextafter(bnd, np.inf)])
    rng = np.random.default_rng(3)
    normal = np.concatenate([-rng.random(20000) * 708.0, -10.0 ** rng.uniform(-16, 0, 2000), np.linspace(-2.0, 0.0, 4001)])
    sub = np.linspace(-745.2, -708.0, 4001)
    # rough_c = 1.01358 E sig_rough at 100 keV and 1e4 A, a log of up to 255 reflections at cos theta = 1 (pc_trace_log_kernel)
    deep = -(1.01358 * 100.0 * 1e4) ** 2 * 255.0
    far = np.concatenate([-np.logspace(np.log10(746.0), 12, 400), [-746.0, -1e13, deep, -1e20, -1e44, -1e100, -1e300, -np.inf]])
    return np.concatenate([[-0.0, 0.0], near, normal, sub, far])


def test_exp_neg_fast():
    """pc_exp_neg_fast at -0.0 and 0.0, on the reduction boundaries -(k + 1/2) ln 2 and their neighbours, over [-708, 0] (normal
    results: relative error <= EXP_TOL), over [-745.2, -708] (subnormal results: EXP_TOL relative plus one 2^-1074), and below:
    0 at and below -746, down to the most negative argument a valid input can produce (-inf: sig_rough has no upper bound, so
    rough_c^2 c^2 overflows).  Never inf or NaN."""
    p = grid.problem("synthetic")
    x = _exp_inputs()
    y = _run(p, "exp", 0, pyprobe.rows(x.size, c=x))[0][:, 0]
    assert np.all(np.isfinite(y)), x[~np.isfinite(y)][:10]
    assert y[0] == 1.0 and y[1] == 1.0
    assert np.all(y[x <= -746.0] == 0.0)
    normal = x >= -708.0
    ref = [exact.exp_mp(v) for v in x[normal]]
    rel = np.array([exact.rel_err(g, r) for g, r in zip(y[normal], ref)])
    print("pc_exp_neg_fast: max rel err %.2e over [-708, 0] (%d inputs, at x = %r)" % (rel.max(), rel.size, x[normal][np.argmax(rel)]))
    assert rel.max() <= EXP_TOL
    sub = (x < -708.0) & (x > -746.0)
    ref = [exact.exp_mp(v) for v in x[sub]]
    ab = np.array([float(abs(exact._m(g) - r)) for g, r in zip(y[sub], ref)])
    lim = np.array([float(r) for r in ref]) * EXP_TOL + SUBNORMAL_ULP
    print("pc_exp_neg_fast: max abs err %.2e = %.2f x 2^-1074 over [-746, -708]" % (ab.max(), ab.max() / SUBNORMAL_ULP))
    assert np.all(ab <= lim)


@pytest.mark.parametrize("glass", ["deck", "synthetic"])
@pytest.mark.parametrize("op", ["f3", "f3s", "ff0", "ff1"])
def test_device_forms_within_their_conditioning(glass, op):
    """FORM 3, FORM 3s and FORMs 0/1 on the device against the exact value at their own double inputs (within K_DEVICE eps of the
    condition sum) and against the host compile of the same form (DEV_HOST_REL where R >= 1e-6 and well conditioned)."""
    p, ec, e, x, f3, f01, ph = form_inputs(glass)
    y, R, K, rel = form_errors(op, p, e, x, f3, f01, device=True)
    yh, _, Kh, relh = form_errors(op, p, e, x, f3, f01, device=False)
    _, cond = exact_form(op, x, f3, f01)
    big = R >= 1e-6
    well = big & (cond <= WELL * R)
    dh = np.abs(y - yh) / np.maximum(np.abs(yh), 1e-300)
    for k in range(p.n_energies):
        m = e == k
        b = m & big
        print("DEVMATH %-4s %-9s E %6.1f amu %-9.3g | K dev %6.2f host %5.2f | rel(R>=1e-6) dev %.2e host %.2e | dev/host %.2e" % (
            op, glass, p.energies[k], p.amu[k], K[m].max(), Kh[m].max(), rel[b].max() if b.any() else 0.,
            relh[b].max() if b.any() else 0., dh[b].max() if b.any() else 0.))
    assert np.all(np.isfinite(y))
    print("DEVMATH %-4s %-9s dev/host where well conditioned (%d points): %.2e" % (op, glass, well.sum(), dh[well].max()))
    assert K.max() <= K_DEVICE[op], (op, glass, K.max(), x[np.argmax(K)])
    assert np.all(np.abs(y - yh) <= (K_DEVICE[op] + K_HOST[op]) * EPS * cond)
    assert well.sum() > 1000 and dh[well].max() <= DEV_HOST_REL, (op, glass, dh[well].max(), x[well][np.argmax(dh[well])])


def test_fresnel3xN_is_bit_identical_to_fresnel3():
    """pc_fresnel3xN at PCS_CHAINS (the FAST loop of pc_trace_log_kernel) and at 1 gives on the device exactly what as many calls of
    pc_fresnel3 give."""
    src = open(os.path.join(grid.ROOT, "polycap_amd", "csrc", "hip", "pc_sweep_kernel.h")).read()
    assert int(re.search(r"#define PCS_CHAINS (\d+)", src).group(1)) == 2, "the probe evaluates pc_fresnel3xN<2>"
    for glass in ("deck", "synthetic"):
        p, ec, e, x, f3, f01, ph = form_inputs(glass)
        keep = np.concatenate([np.flatnonzero(e == k)[: 2 * ((e == k).sum() // 2)] for k in range(p.n_energies)])
        e, x = e[keep], x[keep]
        one, _ = _run(p, "f3", e, x)
        for op in ("f3x1", "f3x2"):
            y, _ = _run(p, op, e, x)
            assert np.array_equal(y[:, 0].view(np.uint64), one[:, 0].view(np.uint64)), (op, glass)


@pytest.mark.parametrize("sig_rough", grid.SIG_ROUGH)
@pytest.mark.parametrize("glass", ["deck", "synthetic"])
def test_return_codes_match_the_host(glass, sig_rough):
    """pc_reflect_energy_fast, pc_reflect_energy3 and pc_reflect_energy_f<0/1> return on the device what the host compile returns
    wherever the exact factor is more than CODE_MARGIN from 0 and 1 and the exact new weight that far from the 1e-4 threshold.
    The points inside the margin are reported, not asserted on."""
    p0, ec0, e, x, f3, f01, ph = form_inputs(glass)
    p = grid.problem(glass, sig_rough)
    ec = pyprobe.energy_consts(p)
    rng = np.random.default_rng(17)
    x = x.copy()
    x[:, pyprobe.COLS.index("w")] = 10.0 ** rng.uniform(-4.5, 0, x.shape[0])
    c = x[:, 0]
    rough = np.array([exact.exp(-(ec["rough_c"][k] * ci) ** 2) for k, ci in zip(e, c)])
    for op, form in (("re_fast", "f3s"), ("re3", "f3"), ("re0", "ff0"), ("re1", "ff1")):
        R, _ = exact_form(form, x, f3, f01)
        wx = x[:, pyprobe.COLS.index("w")] * R * rough
        clear = (np.abs(R) > CODE_MARGIN) & (np.abs(R - 1.0) > CODE_MARGIN) & (np.abs(wx - 1e-4) > CODE_MARGIN)
        _, cd = _run(p, op, e, x)
        _, ch = pyprobe.run(p, op, e, x, device=False)
        near = ~clear
        print("codes %-7s %-9s sig_rough %g: %d points, codes %s; %d inside the margin, %d of them differ%s" % (
            op, glass, sig_rough, cd.size, dict(zip(*np.unique(cd, return_counts=True))), near.sum(), (cd != ch)[near].sum(),
            "" if not (cd != ch)[near].any() else " (e.g. c = %r at E %g: device %d host %d)" % (
                c[near & (cd != ch)][0], p.energies[e[near & (cd != ch)][0]], cd[near & (cd != ch)][0], ch[near & (cd != ch)][0])))
        assert np.array_equal(cd[clear], ch[clear]), (op, glass, sig_rough, np.flatnonzero(clear & (cd != ch))[:5])


@pytest.mark.parametrize("deck,sig_rough", [("xos1", None), ("ellip_l9", 5.0)])
def test_tame_reflections_cannot_fail_the_range_test(deck, sig_rough):
    """pc_trace_log_kernel skips the reference's range test rtot in [0, 1] (src/polycap-capil.c:633-637) for reflections with cos
    theta >= ct_tame (pc_sweep_certify).  For every energy of the 291-energy decks the device's FORM 3 factor at 64 points per
    decade over [ct_tame, 1], with fractions 1/0, 0/1, 1/2 and random, lies in [0, 1 - 1e-12]: the skipped test cannot fire."""
    import polycap_amd
    from tests.conftest import EXAMPLE
    prob = polycap_amd.problem_from_inp(os.path.join(EXAMPLE, deck + ".inp"), sig_rough=sig_rough)
    assert prob.n_energies == 291
    with polycap_amd.TraceContext(prob) as ctx:
        ctx.transmission(5, 0, 2000)
        assert ctx.last_kernel() == "pc_trace_log_kernel"
        ct = ctx.sweep_stats()["ct_tame"]
    assert 0.0 < ct < 1.0
    c = ct * 10.0 ** (np.arange(int(np.ceil(-np.log10(ct) * 64)) + 1) / 64.0)
    c = np.concatenate([[ct], c[c < 1.0], [1.0]])
    ne = prob.n_energies
    e = np.repeat(np.arange(ne, dtype=np.int32), c.size * 4)
    cc = np.tile(np.repeat(c, 4), ne)
    fs, _ = grid.fractions(cc.size)
    es2, sd2 = fs, np.ones_like(fs)
    fp = (sd2 - es2) / sd2          # as pc_refl_geom3 forms the fractions of a logged reflection
    y, _ = _run(prob, "f3", e, pyprobe.rows(cc.size, c=cc, fs=es2 / sd2, fp=fp))
    f = y[:, 0]
    print("%s: ct_tame %.3e, %d factors over %d energies: min %.3e, max 1 - %.3e" % (deck, ct, f.size, ne, f.min(), 1.0 - f.max()))
    assert np.all(f >= 0.0) and np.all(f <= 1.0 - 1e-12), (deck, f.min(), f.max(), cc[np.argmax(f)], e[np.argmax(f)])


@pytest.mark.parametrize("case", ["grid12", "deck291"])
def test_sweep_certificate_is_the_host_functions(case):
    """A context makes its sweep certificate with pc_sweep_certify (pc_sweep_cert.h) on the first launch of the logging kernel.  The
    function is pure, so the host compile of it (tests/emul) returns the same ct_tame and proxies bit for bit;
    tests/test_sweep_cert_cpu.py checks those against mpmath."""
    import polycap_amd
    from tests.emul import pyemul
    from tests.test_sweep_cert_cpu import PROBLEMS
    prob = PROBLEMS[case]()
    want = pyemul.sweep_cert(prob)
    with polycap_amd.TraceContext(prob) as ctx:
        before = ctx.sweep_stats()
        assert before["ct_tame"] == -1.0 and before["proxies"] == [-1, -1]      # unknown until a logging launch
        ctx.transmission(5, 0, 2000)
        assert ctx.last_kernel() == "pc_trace_log_kernel"
        got = ctx.sweep_stats()
    print("%s: ct_tame %r proxies %s" % (case, got["ct_tame"], got["proxies"]))
    assert np.float64(got["ct_tame"]).tobytes() == np.float64(want["ct_tame"]).tobytes(), (got["ct_tame"], want["ct_tame"])
    assert got["proxies"] == want["proxies"]

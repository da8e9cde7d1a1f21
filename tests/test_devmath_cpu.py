"""The Fresnel forms of pc_device.h in the host compile (IEEE sqrt, division and exp) against their exact values (mpmath,
tests/devmath/exact.py), and the device probe's cross-compile.  The device's own arithmetic (v_rsq_f64 / v_rcp_f64 + Newton,
the exp polynomial) is tested against the same references in tests/test_gpu_devmath.py."""
import os

import numpy as np
import pytest

from tests.devmath import exact, grid, pyprobe

EPS = exact.EPS
# |x - R| <= K eps (R + cond), cond = sum |dR/dx_i x_i| over the form's own double inputs (exact.py).  One K per form, from the
# host build over the whole grid (measured: FORM 3 3.5, FORM 3s 2.3, FORMs 0/1 2.3 and 2.0)
K_HOST = dict(f3=4.0, f3s=3.0, ff0=3.0, ff1=3.0)
# FORM 3 against the physical reflectivity is never worse than the better of FORMs 0/1 by more than this, absolutely (measured
# 6.7e-16: at steep angles, where R < 1e-6 and FORM 3's own c - g cancels); near the critical angle, where FORMs 0/1 lose up to
# 2e-5 relative to the reference's 1 - sin^2/n^2, it is far closer
PHYS_SLACK = 1.0e-15


def form_inputs(glass):
    p, ec, e, c, st2, f3, f01, ph = grid.fresnel_points(glass)
    n = c.size
    fs, fp = grid.fractions(n)
    es2, ep2, sd2 = grid.geometry(n)
    x = pyprobe.rows(n, c=c, st2=st2, es2=es2, ep2=ep2, sd2=sd2, fs=fs, fp=fp)
    return p, ec, e, x, f3, f01, ph


def exact_form(op, x, f3, f01):
    """(R, cond) of op at the rows x"""
    fs, fp, es2, ep2, sd2 = (x[:, pyprobe.COLS.index(k)] for k in ("fs", "fp", "es2", "ep2", "sd2"))
    if op in ("f3", "f3x1", "f3x2"):
        Rs, Rp, cs, cp = f3
        R = fs * Rs + fp * Rp
        return R, R + fs * (Rs + cs) + fp * (Rp + cp)
    Rs, Rp, cs, cp = f3 if op == "f3s" else f01
    R = (es2 * Rs + ep2 * Rp) / sd2
    return R, 2 * R + (es2 * (Rs + cs) + ep2 * (Rp + cp)) / sd2


def form_errors(op, p, e, x, f3, f01, device):
    """(value, exact R, K = |x - R| / (eps (R + cond)), relative error) of op over the rows"""
    y, _ = pyprobe.run(p, op, e, x, device=device)
    R, cond = exact_form(op, x, f3, f01)
    return y[:, 0], R, np.abs(y[:, 0] - R) / (EPS * cond), np.abs(y[:, 0] - R) / np.maximum(R, 1e-300)


@pytest.mark.parametrize("glass", ["deck", "synthetic"])
@pytest.mark.parametrize("op", ["f3", "f3s", "ff0", "ff1"])
def test_host_forms_within_their_conditioning(glass, op):
    """The host compile of FORM 3, FORM 3s and FORMs 0/1 at 1 ... 100 keV, cos theta 1e-16 ... 1 and around every critical angle:
    within K eps of the exact value at its own double inputs, K as measured (K_HOST)."""
    p, ec, e, x, f3, f01, ph = form_inputs(glass)
    y, R, K, rel = form_errors(op, p, e, x, f3, f01, device=False)
    for k in range(p.n_energies):
        m = e == k
        big = m & (R >= 1e-6)
        print("host %-4s %-9s E %6.1f keV amu %-9.3g K %.2f  rel(R >= 1e-6) %.2e" % (
            op, glass, p.energies[k], p.amu[k], K[m].max(), rel[big].max() if big.any() else 0.))
    assert np.all(np.isfinite(y))
    assert K.max() <= K_HOST[op], (op, glass, K.max(), x[np.argmax(K)])


@pytest.mark.parametrize("glass", ["deck", "synthetic"])
def test_form3_not_worse_than_forms01_against_the_physical_reflectivity(glass):
    """pc_device.h: FORM 3 does not reproduce the reference's cancellation in 1 - sin^2/n^2.  Against R at the exact (delta,
    beta) its error is never larger than the better of FORMs 0/1 by more than PHYS_SLACK, and near every critical angle, where
    FORMs 0/1 lose digits, it is far closer."""
    p, ec, e, x, f3, f01, ph = form_inputs(glass)
    es2, ep2, sd2 = (x[:, pyprobe.COLS.index(k)] for k in ("es2", "ep2", "sd2"))
    R = (es2 * ph[0] + ep2 * ph[1]) / sd2
    y3, _ = pyprobe.run(p, "f3s", e, x, device=False)
    y0, _ = pyprobe.run(p, "ff0", e, x, device=False)
    y1, _ = pyprobe.run(p, "ff1", e, x, device=False)
    e3 = np.abs(y3[:, 0] - R)
    e01 = np.minimum(np.abs(y0[:, 0] - R), np.abs(y1[:, 0] - R))
    big = R >= 1e-6
    print("%s: FORM 3 rel err (R >= 1e-6) max %.2e, FORMs 0/1 %.2e; FORM 3 worse by at most %.2e absolute" % (
        glass, (e3 / R)[big].max(), (e01 / R)[big].max(), (e3 - e01).max()))
    assert (e3 - e01).max() <= PHYS_SLACK
    # where FORMs 0/1 lose more than 1e-10 relative (there are such points at every energy but the lowest), FORM 3 is 100 times closer
    lost = big & (e01 > 1e-10 * R)
    print("  %d points where FORMs 0/1 lose > 1e-10: FORM 3 closer by a factor of at least %.0f" % (lost.sum(), (e01 / np.maximum(e3, 1e-300))[lost].min()))
    assert lost.sum() >= 50 and np.all(e3[lost] * 100.0 <= e01[lost])


def test_probe_cross_compiles_for_gfx950(tmp_path):
    """tests/devmath/probe.hip builds with the library's own flags (-O3 -ffp-contract=off, gfx950) and exports probe_run."""
    import subprocess
    so = str(tmp_path / "libpc_probe.so")
    subprocess.check_call(pyprobe.compile_cmd(so))
    assert os.path.getsize(so) > 0
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert " T probe_run" in syms

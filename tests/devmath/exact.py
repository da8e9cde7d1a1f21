"""TEST-ONLY: the reflectivity and the primitives of pc_device.h in high precision (mpmath), with the condition terms the
tolerances are built from.

Every form is compared with the exact value of the function it evaluates *at its own double inputs*:
  FORM 3 / 3s  R(d2, n2_re, n2_im, cr2, c2; fs, fp)   g = sqrt(c2 - d2 + i n2_im), n^2 = n2_re + i n2_im, c = cr2/sqrt 2
  FORMs 0 / 1  R(n, ninv2, st2, c; es2, ep2, sd2)   csq = sqrt(1 - ninv2 st2)
with R_s = |(c - g)/(c + g)|^2, R_p = |(g - n^2 c)/(g + n^2 c)|^2 (FORM 3, polycap_refl_polar multiplied through by n) and
R_s = |(c - n csq)/(c + n csq)|^2, R_p = |(csq - n c)/(csq + n c)|^2 (FORMs 0/1, src/polycap-capil.c:503-515).  For each the
condition sum  cond = sum_i |dR/dx_i x_i|  over its inputs is formed from the analytic derivatives, so that a form is right
when |x - R| <= K eps (R + cond) for one K per form.  `physical` is R at the exact (delta, beta) of (E, density, scatf, amu).
"""
import math

import mpmath as mp
import numpy as np

EPS = 2.0 ** -53
DPS = 40
# constants of pc_problem.h:24-26 (the physical reference uses them exactly as decimal numbers)
HC, N_AVOG, R0 = "1.23984193E-7", "6.022098e+23", "2.8179403227e-13"


def _m(x):
    return mp.mpf(float(x))


def _abs2(z):
    return z.real * z.real + z.imag * z.imag


def _dR(r, dr):
    """d|r|^2 = 2 Re(conj(r) dr)"""
    return 2 * (r.real * dr.real + r.imag * dr.imag)


SQRT2 = 1.41421356237309504880    # PC_SQRT2 as the double pc_refl_cr2 multiplies with


def f3_inputs(c):
    """what FORM 3 receives for cos theta = c: cr2 = pc_refl_cr2(c), c2 = c*c (two roundings, two inputs of their own)"""
    c = np.asarray(c, dtype=np.float64)
    return c * SQRT2, c * c


def fresnel3(d2, n2r, n2i, cr2, c2):
    """FORM 3 at its own inputs: (Rs, Rp, cond_s, cond_p) as floats.  The form takes cos theta twice, as cr2 = c sqrt(2) and as
    c2 = c^2, each rounded: the exact function is that of c = cr2/sqrt(2) (exact root) and of c2, g = sqrt(c2 - d2 + i n2_im);
    cond runs over (d2, n2_re, n2_im, cr2, c2).  At steep angles r_s = (c - g)/(c + g) with c - g ~ d2/(2c): the rounding of
    c2 is amplified by c^2/d2, and so is the condition term of c2."""
    with mp.workdps(DPS):
        d2, n2r, n2i, cr2, c2 = _m(d2), _m(n2r), _m(n2i), _m(cr2), _m(c2)
        c = cr2 / mp.sqrt(2)
        z = mp.mpc(c2 - d2, n2i)
        g = mp.sqrt(z)
        m = mp.mpc(n2r, n2i)
        mc = m * c
        rs = (c - g) / (c + g)
        rp = (g - mc) / (g + mc)
        Rs, Rp = _abs2(rs), _abs2(rp)
        if g == 0:
            return float(Rs), float(Rp), math.inf, math.inf
        drs_dg = -2 * c / (c + g) ** 2
        drs_dc = 2 * g / (c + g) ** 2
        drp_dg = 2 * mc / (g + mc) ** 2
        drp_dm = -2 * g * c / (g + mc) ** 2
        drp_dc = -2 * g * m / (g + mc) ** 2
        i = mp.mpc(0, 1)
        # derivatives along each input, times the input (the factor of cr2 = c sqrt 2 is c d/dc)
        dg = {"c": 0, "c2": 1 / (2 * g), "d2": -1 / (2 * g), "n2r": 0, "n2i": i / (2 * g)}
        dm = {"c": 0, "c2": 0, "d2": 0, "n2r": 1, "n2i": i}
        own = {"c": drs_dc, "c2": 0, "d2": 0, "n2r": 0, "n2i": 0}
        ownp = {"c": drp_dc, "c2": 0, "d2": 0, "n2r": 0, "n2i": 0}
        val = {"c": c, "c2": c2, "d2": d2, "n2r": n2r, "n2i": n2i}
        cs = cp = mp.mpf(0)
        for k in val:
            cs += abs(_dR(rs, own[k] + drs_dg * dg[k]) * val[k])
            cp += abs(_dR(rp, ownp[k] + drp_dg * dg[k] + drp_dm * dm[k]) * val[k])
        return float(Rs), float(Rp), float(cs), float(cp)


def fresnel01(n_re, n_im, ninv2_re, ninv2_im, st2, c):
    """FORMs 0/1 at their own inputs: (Rs, Rp, cond_s, cond_p), cond over (n_re, n_im, ninv2_re, ninv2_im, st2, c)."""
    with mp.workdps(DPS):
        n_re, n_im, a, b, st2, c = (_m(v) for v in (n_re, n_im, ninv2_re, ninv2_im, st2, c))
        n = mp.mpc(n_re, n_im)
        ninv2 = mp.mpc(a, b)
        w = 1 - ninv2 * st2
        csq = mp.sqrt(w)
        h = n * csq
        u = n * c
        rs = (c - h) / (c + h)
        rp = (csq - u) / (csq + u)
        Rs, Rp = _abs2(rs), _abs2(rp)
        if csq == 0:
            return float(Rs), float(Rp), math.inf, math.inf
        i = mp.mpc(0, 1)
        drs_dh = -2 * c / (c + h) ** 2
        drs_dc = 2 * h / (c + h) ** 2
        drp_dcsq = 2 * u / (csq + u) ** 2
        drp_du = -2 * csq / (csq + u) ** 2
        dcsq = {"n_re": 0, "n_im": 0, "a": -st2 / (2 * csq), "b": -i * st2 / (2 * csq), "st2": -ninv2 / (2 * csq), "c": 0}
        dn = {"n_re": 1, "n_im": i, "a": 0, "b": 0, "st2": 0, "c": 0}
        val = {"n_re": n_re, "n_im": n_im, "a": a, "b": b, "st2": st2, "c": c}
        cs = cp = mp.mpf(0)
        for k in val:
            dh = dn[k] * csq + n * dcsq[k]
            du = dn[k] * c + (n if k == "c" else 0)
            drs = drs_dh * dh + (drs_dc if k == "c" else 0)
            drp = drp_dcsq * dcsq[k] + drp_du * du
            cs += abs(_dR(rs, drs) * val[k])
            cp += abs(_dR(rp, drp) * val[k])
        return float(Rs), float(Rp), float(cs), float(cp)


def delta_beta(E, density, scatf, amu):
    """Exact (delta, beta) of n = 1 - delta + i beta (pc_problem.h:161-162 in exact arithmetic) as mpf."""
    with mp.workdps(DPS):
        hc, na, r0 = mp.mpf(HC), mp.mpf(N_AVOG), mp.mpf(R0)
        E, density, scatf, amu = _m(E), _m(density), _m(scatf), _m(amu)
        delta = (hc / E) ** 2 * (na * r0 * density / (2 * mp.pi)) * scatf
        beta = hc / (4 * mp.pi) * (amu / E)
        return +delta, +beta


def physical(delta, beta, c):
    """(Rs, Rp) of the exact refractive index and the exact sin^2 = 1 - c^2 at cos theta = c (a double)."""
    with mp.workdps(DPS):
        c = _m(c)
        n = mp.mpc(1 - delta, beta)
        csq = mp.sqrt(1 - (1 - c * c) / (n * n))
        h, u = n * csq, n * c
        return float(_abs2((c - h) / (c + h))), float(_abs2((csq - u) / (csq + u)))


def exp(x):
    with mp.workdps(DPS):
        return float(mp.exp(_m(x)))


def exp_mp(x):
    """exp(x) as an mpf (for errors of results that round to subnormals)"""
    with mp.workdps(DPS):
        return mp.exp(_m(x))


def rel_err(got, exact_mpf):
    """|got - exact| / exact, in high precision, as a float"""
    with mp.workdps(DPS):
        return float(abs(_m(got) - exact_mpf) / exact_mpf)


def sqrt_rel_err(x, y):
    with mp.workdps(DPS):
        s = mp.sqrt(_m(x))
        return float(abs(_m(y) - s) / s)


def div_rel_err(a, b, y):
    with mp.workdps(DPS):
        q = _m(a) / _m(b)
        return float(abs(_m(y) - q) / abs(q))


def fresnel3_table(ec, e, c):
    """fresnel3 at energies e (indices into the pc_energy_const dict ec) and cosines c: arrays (Rs, Rp, cs, cp)."""
    cr2, c2 = f3_inputs(c)
    out = np.array([fresnel3(ec["d2"][k], ec["n2_re"][k], ec["n2_im"][k], a, b) for k, a, b in zip(e, cr2, c2)])
    return out.T


def fresnel01_table(ec, e, c, st2):
    out = np.array([fresnel01(ec["n_re"][k], ec["n_im"][k], ec["ninv2_re"][k], ec["ninv2_im"][k], s, ci)
                    for k, ci, s in zip(e, c, st2)])
    return out.T


def fma_neg_sq_one(c):
    """fma(-c, c, 1.0): 1 - c^2 rounded once, as pc_reflect_geom forms sin^2"""
    with mp.workdps(DPS):
        return float(1 - _m(c) * _m(c))

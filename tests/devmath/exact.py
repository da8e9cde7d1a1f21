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


# ---------------------------------------------------------------------------------------------------------------------------
# The geometric half of a reflection: the reference's definitions (src/polycap-capil.c:52-255 segment, :444-563 refl_polar,
# :565-655 reflect) evaluated from the double inputs as stored, at GDPS digits.  Results stay mpf (errors of 1e-16 on
# coordinates of order 1 are differences of nearly equal numbers); the *_err functions turn them into floats.
GDPS = 70
U = EPS                       # unit roundoff of one correctly rounded operation
GUARD_LAST = 1.e-5            # the doubles the reference compares with (:134-171, :178)
GUARD_PROJ = 1.e-10


def _v(x):
    return [mp.mpf(float(t)) for t in x]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def segment(row):
    """polycap_capil_segment in exact arithmetic on one probe row (z0, z1, cap0, cap1, zh0, zh1, kx, ky, P, d), every input finite.

    Returns a dict: status (the reference's, or None where it divides by zero: dz = 0, a = 0 with the root asked for); hz, h
    (3), n (3) as mpf when status is 1; roots; cond = the sensitivity of the selected root to relative changes of a, b, c (its
    relative error per relative 2^-53 of each, summed); guards = [(name, value, err)]: every quantity the reference compares,
    its exact distance from the threshold and the first-order running error bound of the reference's own evaluation of it (one
    2^-53 per operation).  A guard decides the status safely when |value| is a multiple of err."""
    with mp.workdps(GDPS):
        z0, z1, R0, R1, zh0, zh1, kx, ky, Px, Py, Pz, dx, dy, dz = _v(row)
        out = dict(status=None, guards=[], cond=None, roots=None, a=None, discr=None)
        if dz < 0 or z1 <= z0 or R0 < 0 or R1 < 0 or z0 < 0:
            out["status"] = -1
            return out
        if dz == 0:
            return out
        u = mp.mpf(U)
        dn = mp.sqrt(dx * dx + dy * dy + dz * dz)
        c0x, c0y, c1x, c1y = kx * zh0, ky * zh0, kx * zh1, ky * zh1
        cdx, cdy, cdz = c1x - c0x, c1y - c0y, z1 - z0
        sx, sy = dx / dz, dy / dz
        t0 = z0 - Pz
        p0x, p0y = Px + sx * t0, Py + sy * t0
        ddx, ddy = sx - cdx / cdz, sy - cdy / cdz
        rr = (R1 - R0) / cdz
        qx, qy = p0x - c0x, p0y - c0y
        a = ddx * ddx + ddy * ddy - rr * rr
        b = 2 * (qx * ddx + qy * ddy - R0 * rr)
        c = qx * qx + qy * qy - R0 * R0
        D = b * b - 4 * a * c
        # running error of the reference's evaluation, first order
        e_ddx = u * (abs(sx) + (abs(c1x) + abs(c0x)) / cdz + 3 * abs(cdx / cdz) + abs(ddx))
        e_ddy = u * (abs(sy) + (abs(c1y) + abs(c0y)) / cdz + 3 * abs(cdy / cdz) + abs(ddy))
        e_rr = 3 * u * abs(rr)
        e_qx = u * (abs(p0x) + 3 * abs(sx * t0) + abs(c0x) + abs(qx))
        e_qy = u * (abs(p0y) + 3 * abs(sy * t0) + abs(c0y) + abs(qy))
        e_a = 2 * (abs(ddx) * e_ddx + abs(ddy) * e_ddy + abs(rr) * e_rr) + 3 * u * (ddx * ddx + ddy * ddy + rr * rr)
        e_b = 2 * (abs(ddx) * e_qx + abs(qx) * e_ddx + abs(ddy) * e_qy + abs(qy) * e_ddy + R0 * e_rr) \
            + 6 * u * (abs(qx * ddx) + abs(qy * ddy) + abs(R0 * rr))
        e_c = 2 * (abs(qx) * e_qx + abs(qy) * e_qy) + 3 * u * (qx * qx + qy * qy + R0 * R0)
        e_D = 2 * abs(b) * e_b + 4 * (abs(a) * e_c + abs(c) * e_a) + 3 * u * (b * b + 4 * abs(a * c))
        out["a"], out["discr"], out["b2"], out["rr2"] = a, D, b * b, rr * rr
        out["guards"].append(("discr", D, e_D))
        if D < 0:
            out["status"] = -2
            return out
        if a == 0:
            return out
        s = mp.sqrt(D)
        last = Pz
        g_last, g_proj = mp.mpf(GUARD_LAST), mp.mpf(GUARD_PROJ)

        def root(sign):
            t = (-b + sign * s) / (2 * a)
            # the errors of a, b, c move the root by (t^2 da + t db + dc) / sqrt(D) (they move -b and sqrt(D) together: no
            # cancellation between them; sqrt(D) is floored at its own error for tangent rays); the roundings of -b +- sqrt(D)
            # themselves do cancel against 2a
            e_t = (t * t * e_a + abs(t) * e_b + e_c) / max(s, mp.sqrt(e_D)) + 3 * u * (abs(b) + s) / (2 * abs(a)) + 3 * u * abs(t)
            zr = z0 + t
            e_z = e_t + u * abs(zr)
            return t, zr, e_t, e_z

        def bad(zr):
            return zr < z0 or zr - last < g_last or zr > z1

        roots = [root(1), root(-1)] if D != 0 else [root(0)]
        out["roots"] = [r[1] for r in roots]
        reach = max(z1 - z0, abs(last + g_last - z0))
        for k, (t, zr, e_t, e_z) in enumerate(roots):
            if abs(t) > 4 * reach:
                # a root far outside the segment (a ray nearly parallel to the wall: a -> 0) is rejected whatever its sign; its
                # own error grows like t^2, that of 1/t does not: it stays rejected while 1/|t| stays below 1/reach
                out["guards"].append(("far%d" % k, 1 / reach - 1 / abs(t), e_t / (t * t)))
                continue
            out["guards"] += [("zr%d-z0" % k, zr - z0, e_t + u * abs(z0)), ("z1-zr%d" % k, z1 - zr, e_z + u * abs(z1)),
                              ("zr%d-last-1e-5" % k, zr - last - g_last, e_z + u * abs(zr - last))]
        if D == 0:
            sel = roots[0]
        else:
            b1, b2 = bad(roots[0][1]), bad(roots[1][1])
            if b1 and b2:
                out["status"] = -3
                return out
            if b1:
                sel = roots[1]
            elif b2:
                sel = roots[0]
            else:
                sel = roots[1] if roots[1][1] - last < roots[0][1] - last else roots[0]
                out["guards"].append(("zr1-zr0", roots[1][1] - roots[0][1], roots[0][3] + roots[1][3]))
        t, hz, e_t, e_z = sel
        out["cond"] = (abs(t * t * a) + abs(t * b) + abs(c)) / (s * abs(t)) if s != 0 and t != 0 else mp.inf
        out["e_hz"] = e_z
        if hz > z1:
            out["status"] = -4
            return out
        if hz < z0 or hz - last < g_last:
            out["status"] = -5
            return out
        ndz = dz / dn
        d_proj = (hz - z0) / ndz
        out["guards"].append(("d_proj-1e-10", d_proj - g_proj, e_t / ndz + 2 * u * abs(d_proj)))
        if d_proj < g_proj:
            out["status"] = -6
            return out
        hx, hy = p0x + d_proj * dx / dn, p0y + d_proj * dy / dn
        # :225-246: the axis point opposite the hit, the radial unit vector, tilted by the wall angle
        cap_dir = [cdx, cdy, cdz]
        rel = [qx, qy, mp.mpf(0)]
        pd = [dx / dn, dy / dn, dz / dn]
        s2 = _dot(pd, cap_dir)
        tpar = (d_proj + _dot(rel, cap_dir) / s2) / (_dot(cap_dir, cap_dir) / s2)
        inn = [hx - (c0x + tpar * cdx), hy - (c0y + tpar * cdy), hz - (z0 + tpar * cdz)]
        li, lc = mp.sqrt(_dot(inn, inn)), mp.sqrt(_dot(cap_dir, cap_dir))
        gam = mp.atan((R0 - R1) / lc)
        n = [mp.cos(gam) * inn[k] / li + mp.sin(gam) * cap_dir[k] / lc for k in range(3)]
        ln = mp.sqrt(_dot(n, n))
        out.update(status=1, hz=hz, h=[hx, hy, hz], n=[v / ln for v in n], p0=[p0x, p0y], d_proj=d_proj)
        return out


def segment_errors(ex, out_row):
    """(|hz - hz*|, |h - h*|, angle(n, n*), | |n| - 1 |) of a probe or oracle result (hx, hy, hz, nx, ny, nz, ...) against
    segment()'s result ex (status 1), as floats."""
    with mp.workdps(GDPS):
        h, n = _v(out_row[0:3]), _v(out_row[3:6])
        dh = [h[k] - ex["h"][k] for k in range(3)]
        cr = _cross(n, ex["n"])
        ln = mp.sqrt(_dot(n, n))
        ang = mp.atan2(mp.sqrt(_dot(cr, cr)), _dot(n, ex["n"]))
        return float(abs(dh[2])), float(mp.sqrt(_dot(dh, dh))), float(ang), float(abs(ln - 1))


def geom(row):
    """The geometry of a reflection from (d, E, n) as stored.  'own': what pc_reflect_geom / pc_refl_geom3 evaluate, exactly
    (no normalisation: the product relies on unit vectors); 'ref': the reference's definitions, which normalise d, n and E
    (cos theta, sin^2 theta, (E.s)^2, 1 - (E.s)^2); 'bound': the first-order running error of the product's evaluation of each
    own quantity (one 2^-53 per operation), the conditioning bound the measured errors are held against.  mpf throughout."""
    with mp.workdps(GDPS):
        d, E, n = _v(row[0:3]), _v(row[3:6]), _v(row[6:9])
        u = mp.mpf(U)
        alfa = _dot(d, n)
        absdn = sum(abs(d[k] * n[k]) for k in range(3))
        s = _cross(n, d)
        sd2 = _dot(s, s)
        es = _dot(E, s)
        es2, st2 = es * es, 1 - alfa * alfa
        ep2 = sd2 - es2
        own = dict(alfa=alfa, st2=st2, es2=es2, ep2=ep2, sd2=sd2, c2=alfa * alfa)
        b_alfa = 3 * u * absdn
        b_s = [2 * u * (abs(n[(k + 1) % 3] * d[(k + 2) % 3]) + abs(d[(k + 1) % 3] * n[(k + 2) % 3])) for k in range(3)]
        b_sd2 = 3 * u * sd2 + 2 * sum(abs(s[k]) * b_s[k] for k in range(3))
        b_es = 3 * u * sum(abs(E[k] * s[k]) for k in range(3)) + sum(abs(E[k]) * b_s[k] for k in range(3))
        b_es2 = 2 * abs(es) * b_es + u * es2 + b_es * b_es
        b_ep2 = b_es2 + b_sd2 + u * abs(ep2)
        bound = dict(alfa=b_alfa, st2=u * abs(st2) + 2 * abs(alfa) * b_alfa, es2=b_es2, ep2=b_ep2, sd2=b_sd2,
                     c2=u * alfa * alfa + 2 * abs(alfa) * b_alfa)
        ref = dict()
        ld, ln, lE = (mp.sqrt(_dot(v, v)) for v in (d, n, E))
        ref["cos"] = alfa / (ld * ln) if ld * ln != 0 else mp.nan
        ref["sin2"] = 1 - ref["cos"] ** 2
        if sd2 > 0:
            own["fs"], own["fp"] = es2 / sd2, ep2 / sd2
            bound["fs"] = (b_es2 + own["fs"] * b_sd2) / sd2 + u * own["fs"]
            bound["fp"] = (b_ep2 + abs(own["fp"]) * b_sd2) / sd2 + u * abs(own["fp"])
            ref["fs"] = es2 / (sd2 * lE * lE)
            ref["fp"] = 1 - ref["fs"]
        # the mirror image of d about the plane with normal n: as the product forms it (d - 2 (d.n) n) and exactly
        own["mirror"] = [d[k] - 2 * alfa * n[k] for k in range(3)]
        ref["mirror"] = [d[k] - 2 * alfa * n[k] / (ln * ln) for k in range(3)] if ln != 0 else None
        bound["mirror"] = [u * abs(own["mirror"][k]) + 2 * abs(n[k]) * (b_alfa + u * abs(alfa)) for k in range(3)]
        own["len_d"], own["len_n"] = ld, ln
        return dict(own=own, ref=ref, bound=bound)


def absdiff(got, exact_mpf):
    """|got - exact| as a float, formed at GDPS digits"""
    with mp.workdps(GDPS):
        return float(abs(mp.mpf(float(got)) - exact_mpf))


def vec_len_minus_one(v):
    with mp.workdps(GDPS):
        w = _v(v)
        return float(mp.sqrt(_dot(w, w)) - 1)


def unit(v):
    """v / |v| rounded to doubles, from high precision"""
    with mp.workdps(GDPS):
        l = mp.sqrt(_dot(v, v))
        return [float(t / l) for t in v]


# ---------------------------------------------------------------------------------------------------------------------------
# The certified march in rational arithmetic (tests/test_devmath_march_cpu.py).  Every double is an exact rational and
# g_j(z) = |p(z) - (kx, ky) zh(z)|^2 - R(z)^2 is a polynomial in them, so nothing below has a tolerance.  The ray is the photon's
# own: the line through the row's start P along the normalised direction d the probe reports -- not the rounded ox, oy, sx, sy
# the certificates evaluate (the margin m exists to cover that difference).  zh and R are piecewise linear in the table doubles.
# To keep every number dyadic (no division before the very end) g is carried as G = dz^2 g, which has g's sign.
from fractions import Fraction

TEN_MU = Fraction(1.0e-5)          # the double the code adds to P.z and the reference compares with (src/polycap-capil.c:134-171)


def fr(x):
    return Fraction(float(x))


def march_profile(t):
    """exact rationals of the tables of pyemul.march_tables"""
    return {k: [fr(v) for v in t[k]] for k in ("z", "cap", "ext", "zh")}


def admissible_from(Pz):
    """Where the admissible range of the first segment of a flight begins, as a rational.  The reference admits a root zr (a
    double) when fl(zr - P.z) >= 1e-5, which zr - P.z >= 1e-5 (1 - 2^-53) already allows; pc_march_first_ok starts its range at
    the double fl(P.z + 1e-5), which may lie below P.z + 1e-5.  The smaller of P.z + 1e-5 (1 - 2^-52) and fl(P.z + 1e-5) is taken:
    the range tested is then at least as wide as the reference's and as the code's own, so the maximum of g over it is at least
    theirs -- the strict side for a test that asserts max g < 0."""
    Pz = float(Pz)
    return min(fr(Pz) + TEN_MU * (1 - Fraction(1, 2 ** 52)), fr(Pz + 1.0e-5))


def _dy(x):
    """a double as (integer, e) with x = integer / 2^e"""
    n, d = float(x).as_integer_ratio()
    return n, d.bit_length() - 1


def _scaled(vals):
    """doubles as integers over one common power of two: ([v 2^e], e)"""
    pairs = [_dy(v) for v in vals]
    e = max(q for _, q in pairs)
    return [n << (e - q) for n, q in pairs], e


class MarchRay:
    """The exact ray of one MARCH row on one profile and the exact maximum of g per segment.  Doubles are dyadic, so all of it is
    integer arithmetic over common powers of two (lengths over 2^E, the direction over 2^Ed, k over 2^Ek); a Fraction is formed
    of the result only."""

    def __init__(self, prof, P, d, k):
        self.prof = prof
        n = len(prof["z"])
        ints, self.E = _scaled([float(v) for key in ("z", "zh", "cap") for v in prof[key]] + [float(v) for v in P])
        self.z, self.zh, self.R, self.P = ints[:n], ints[n:2 * n], ints[2 * n:3 * n], ints[3 * n:]
        self.d, self.Ed = _scaled(d)
        self.k, self.Ek = _scaled(k)
        # G = dz^2 g over 2^(2 (E + Ed + Ek)); g = G_int / den
        self.den = self.d[2] * self.d[2] << (2 * (self.E + self.Ek))
        self._Q = {}

    def Q(self, j):
        """dz (P_xy - k zh_j) + d_xy (z_j - P_z), over 2^(E + Ed + Ek): dz times the ray's offset from the capillary axis at node j"""
        if j not in self._Q:
            zh, dzj = self.zh[j], (self.z[j] - self.P[2]) << self.Ek
            self._Q[j] = (self.d[2] * ((self.P[0] << self.Ek) - self.k[0] * zh) + self.d[0] * dzj,
                          self.d[2] * ((self.P[1] << self.Ek) - self.k[1] * zh) + self.d[1] * dzj)
        return self._Q[j]

    def _quad(self, j):
        """(A, B, C) of G(u) = A u^2 + B u + C on segment j, u = (z - z_j)/(z_j+1 - z_j): G = den g, integers"""
        (ax, ay), (bx, by) = self.Q(j), self.Q(j + 1)
        ex, ey = bx - ax, by - ay
        s = self.d[2] << self.Ek                     # dz R over 2^(E + Ed + Ek) is s R_int
        R0, dR = s * self.R[j], s * (self.R[j + 1] - self.R[j])
        return ex * ex + ey * ey - dR * dR, 2 * (ax * ex + ay * ey - R0 * dR), ax * ax + ay * ay - R0 * R0

    def max_g(self, j, z_from=None):
        """(max of g over segment j from z_from (a rational; None: the segment's first node) to its last node, u of the maximum),
        None when that range is empty.  g(u) = A u^2 + B u + C on u = (z - z_j)/(z_j+1 - z_j): the ends, and the vertex when
        A < 0 puts it inside."""
        A, B, Cc = self._quad(j)
        lo = 0
        if z_from is not None:
            zf = z_from * (1 << self.E)
            if zf > self.z[j]:
                lo = (zf - self.z[j]) / (self.z[j + 1] - self.z[j])
                if lo >= 1:
                    return None
        best, at = (A * lo + B) * lo + Cc, lo
        g1 = A + B + Cc
        if g1 > best:
            best, at = g1, 1
        if A < 0 and B > 0:
            u = Fraction(-B, 2 * A)
            if lo < u < 1:
                gv = Cc - Fraction(B * B, 4 * A)
                if gv > best:
                    best, at = gv, u
        return Fraction(best) / self.den, Fraction(at)

    def g_at(self, z):
        """g at the rational z, on the segment that holds it (the last one for z at or beyond the last node, the first below the
        first): the ray's own g, extended linearly in zh and R where z lies outside the profile"""
        zf = z * (1 << self.E)
        n = len(self.z)
        j = 0
        while j < n - 2 and self.z[j + 1] <= zf:
            j += 1
        A, B, Cc = self._quad(j)
        u = (zf - self.z[j]) / (self.z[j + 1] - self.z[j])
        return Fraction((A * u + B) * u + Cc) / self.den

    def g_node(self, j):
        """g at node j"""
        ax, ay = self.Q(j)
        s = (self.d[2] << self.Ek) * self.R[j]
        return Fraction(ax * ax + ay * ay - s * s, self.den)


def mirrored(d, n, cosalfa):
    """The direction pc_event_post leaves: per component fma(-2 cosalfa, n, d), i.e. the exact d - 2 cosalfa n rounded once
    (-2 cosalfa is exact in doubles; a Fraction converts to the nearest double)."""
    c2 = Fraction(-2.0 * float(cosalfa))
    return [float(fr(d[c]) + c2 * fr(n[c])) for c in range(3)]


def march_table_bounds(t):
    """What the certificate tables of pyemul.march_tables must be at least, exactly: m = max(1e-6 capmin^2, 1e-10 capmax extmax)
    with the two constants as the doubles the setup multiplies with; adj = dR^2max/4 + m; and per stride L (PC_L1, PC_L2) and
    start node i whose block fits: the chord deviation Dzh of zh (a piecewise linear table deviates most from a chord at a node),
    the base dR^2/4 + 2 R_blk DR + m with DR the chord deviation of cap and R_blk the largest radius of the block, and 2 R_blk;
    r2 also covers the clipped PC_L2 block of a start node near the end."""
    p = march_profile(t)
    z, cap, ext, zh = p["z"], p["cap"], p["ext"], p["zh"]
    n = len(z)
    m = max(fr(1e-6) * min(cap) ** 2, fr(1e-10) * max(cap) * max(abs(e) for e in ext))
    dr2max = max((cap[i + 1] - cap[i]) ** 2 for i in range(n - 1))
    out = dict(m=m, adj=dr2max / 4 + m, L={}, r2=[2 * max(cap[i:min(n, i + t["L2"] + 1)]) for i in range(n)])
    for L in (t["L1"], t["L2"]):
        rows = []
        for i in range(n):
            if i + L >= n:
                rows.append(None)
                continue
            span = z[i + L] - z[i]
            dzh = dr = Fraction(0)
            for j in range(i + 1, i + L):
                u = (z[j] - z[i]) / span
                dzh = max(dzh, abs(zh[j] - (zh[i] + (zh[i + L] - zh[i]) * u)))
                dr = max(dr, abs(cap[j] - (cap[i] + (cap[i + L] - cap[i]) * u)))
            rblk = max(cap[i:i + L + 1])
            dR = cap[i + L] - cap[i]
            rows.append(dict(md=dzh, mb=dR * dR / 4 + 2 * rblk * dr + m, r2=2 * rblk))
        out["L"][L] = rows
    return out


def circle_inside_hexagon(cx, cy, cap, ext):
    """Exactly: the circle of radius cap about (cx, cy) lies strictly inside the hexagon of circum-radius ext > 0 with corners on
    the x axis (polycap_photon_within_pc_boundary): for the three edge normals (0, 1), (sqrt 3/2, +-1/2) and both signs,
    sqrt3/2 ext - sigma n.c - cap > 0.  The root is removed by comparing squares: sqrt3 alpha > beta."""
    def s3_gt(alpha, beta):            # sqrt(3) * alpha > beta
        if alpha > 0:
            return beta < 0 or 3 * alpha * alpha > beta * beta
        return beta < 0 and 3 * alpha * alpha < beta * beta
    if not ext > 0:
        return False
    for sg in (1, -1):
        if not s3_gt(ext, 2 * (cap + sg * cy)):                       # sqrt3/2 ext > cap + sg cy
            return False
        for t in (1, -1):                                             # sqrt3/2 (ext - sg cx) > cap + sg t cy / 2
            if not s3_gt(ext - sg * cx, 2 * cap + sg * t * cy):
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------
# The leak path's wall search in rational arithmetic (tests/test_devmath_leak_cpu.py).  The ray is the photon's own, through the
# row's P along the row's d.  ext(z), cap(z), zh(z) (the table's doubles) and zz(z) = ext(z)/hexscale are piecewise linear between
# the nodes; 2/3, 3/2, cos(pi/6) and hexscale are the doubles the code uses.
#
# Cell (q, r) of the cube rounding of pc_hex_index is where, with (dq, dr) the fractional axial coordinates minus (q, r),
# |dq - dr| <= 1, |2 dq + dr| <= 1 and |dq + 2 dr| <= 1.  Multiplied by zz > 0 each bound is linear in z on a profile segment, so
# membership over a stretch is decided at its ends and at the nodes inside it.
import bisect

COSPI_6 = Fraction(0.86602540378443864676)
TWO_THIRDS = Fraction(2.0 / 3)
U53 = Fraction(1, 2 ** 53)


def hex_forms(x, y, zz, q, r):
    """(a1, a2, a3) = zz (dq - dr, 2 dq + dr, dq + 2 dr) of the point (x, y) against cell (q, r): inside means |a_k| <= zz"""
    Q = x / (2 * COSPI_6) - y / 3 - q * zz
    R = y * TWO_THIRDS - r * zz
    return Q - R, 2 * Q + R, Q + 2 * R


def hex_cells(x, y, zz):
    """exactly: the cells (q, r) whose closed hexagon holds (x, y) -- one, two on an edge, three at a corner -- and for each the
    smallest of 1 - |a_k| / zz (0 on an edge).  A Fraction passed in is taken as it is (entrance: zz between two nodes)."""
    x, y, zz = (v if isinstance(v, Fraction) else fr(v) for v in (x, y, zz))
    qf, rf = (x / (2 * COSPI_6) - y / 3) / zz, y * TWO_THIRDS / zz
    out = {}
    for q in range(math_floor(qf) - 1, math_floor(qf) + 3):
        for r in range(math_floor(rf) - 1, math_floor(rf) + 3):
            a = hex_forms(x, y, zz, q, r)
            m = min(zz - abs(v) for v in a)
            if m >= 0:
                out[(q, r)] = m / zz
    return out, qf, rf


def math_floor(v):
    return v.numerator // v.denominator


def hex_error_bound(x, y, zz, qf, rf):
    """first-order running error bound (one 2^-53 per operation) of the fractional coordinates pc_hex_index forms and of the three
    differences its cube rounding compares, as one number in cell units"""
    x, y, zz = (abs(v if isinstance(v, Fraction) else fr(v)) for v in (x, y, zz))
    eq = U53 * ((x / (2 * COSPI_6) + y / 3 + abs(x / (2 * COSPI_6) - y / 3)) / zz + abs(qf))
    er = 2 * U53 * abs(rf)
    es = eq + er + 2 * U53 * (abs(qf) + abs(rf))
    return 2 * (eq + er + es)


class WallRay:
    """One WALL row on one profile, exactly.  t: dict of the tables' doubles z, cap, ext, zh and hexscale."""

    def __init__(self, t, P, d):
        self.zf = [float(v) for v in t["z"]]
        self.z = [fr(v) for v in t["z"]]
        self.cap = [fr(v) for v in t["cap"]]
        self.ext = [fr(v) for v in t["ext"]]
        self.zh = [fr(v) for v in t["zh"]]
        hs = fr(t["hexscale"])
        self.zz = [e / hs for e in self.ext]
        self.P = [fr(v) for v in P]
        self.d = [fr(v) for v in d]
        self.nmax = len(self.z) - 1

    def xy(self, z):
        s = (z - self.P[2]) / self.d[2]
        return self.P[0] + self.d[0] * s, self.P[1] + self.d[1] * s

    def seg(self, z):
        return min(self.nmax - 1, max(0, bisect.bisect_right(self.z, z) - 1))

    def at(self, tab, z, j=None):
        j = self.seg(z) if j is None else j
        return tab[j] + (tab[j + 1] - tab[j]) * (z - self.z[j]) / (self.z[j + 1] - self.z[j])

    def pieces(self, za, zb):
        """[za, zb] (za <= zb) cut at the nodes inside it: list of (z0, z1, segment)"""
        pts = [za] + [z for z in self.z[bisect.bisect_right(self.z, za):bisect.bisect_left(self.z, zb)]] + [zb]
        return [(a, b, self.seg((a + b) / 2)) for a, b in zip(pts[:-1], pts[1:])] if zb > za else [(za, zb, self.seg(za))]

    def cell_slack(self, z, q, r, j=None):
        """zz(z) - max |a_k| at z for cell (q, r), and zz(z): > 0 strictly inside"""
        x, y = self.xy(z)
        zz = self.at(self.zz, z, j)
        return zz - max(abs(v) for v in hex_forms(x, y, zz, q, r)), zz

    def min_cell_slack(self, za, zb, q, r):
        """smallest (zz - max |a_k|) / zz over [za, zb]: the forms are linear on every piece, so the ends of the pieces decide the
        sign; the value is the smallest of the end values"""
        best = None
        for a, b, j in self.pieces(za, zb):
            for z in (a, b):
                s, zz = self.cell_slack(z, q, r, j)
                v = s / zz
                best = v if best is None or v < best else best
        return best

    def min_gap2(self, za, zb, K, zt):
        """exact minimum over [za, zb] of |p(z) - K zt(z)|^2 - cap(z)^2 for the axis table zt (self.zz or self.zh), with the z of
        the minimum: a quadratic on every piece -- its ends, and the vertex where it opens upwards and lies inside"""
        best, at = None, None
        Kx, Ky = K
        for a, b, j in self.pieces(za, zb):
            xa, ya = self.xy(a)
            xb, yb = self.xy(b)
            ta, tb = self.at(zt, a, j), self.at(zt, b, j)
            ca, cb = self.at(self.cap, a, j), self.at(self.cap, b, j)
            ux, uy = xa - Kx * ta, ya - Ky * ta
            ex, ey = xb - Kx * tb - ux, yb - Ky * tb - uy
            dc = cb - ca
            A = ex * ex + ey * ey - dc * dc
            B = 2 * (ux * ex + uy * ey - ca * dc)
            C0 = ux * ux + uy * uy - ca * ca
            cands = [(C0, a), (A + B + C0, b)]
            if A > 0 and 0 < -B < 2 * A:
                s = -B / (2 * A)
                cands.append((C0 - B * B / (4 * A), a + (b - a) * s))
            for v, z in cands:
                if best is None or v < best:
                    best, at = v, z
        return best, at

    def first_exit(self, za, q, r):
        """first z >= za at which the ray leaves the closed cell (q, r) going up in z, with the slacks zz - |a_k| of the three
        forms there (the crossed one is 0); None when it stays inside up to the last node"""
        zb = self.z[self.nmax]
        if za >= zb:
            return None
        for a, b, j in self.pieces(za, zb):
            xa, ya = self.xy(a)
            xb, yb = self.xy(b)
            zza, zzb = self.at(self.zz, a, j), self.at(self.zz, b, j)
            fa, fb = hex_forms(xa, ya, zza, q, r), hex_forms(xb, yb, zzb, q, r)
            s_best = None
            for k in range(3):
                for sg in (1, -1):
                    ga, gb = zza - sg * fa[k], zzb - sg * fb[k]          # >= 0 inside, linear on the piece
                    if gb < 0 and ga >= 0:
                        s = ga / (ga - gb)
                        s_best = s if s_best is None or s < s_best else s_best
                    elif ga < 0:
                        s_best = Fraction(0)
            if s_best is not None:
                z = a + (b - a) * s_best
                x, y = self.xy(z)
                zz = self.at(self.zz, z, j)
                return z, sorted((zz - abs(v)) / zz for v in hex_forms(x, y, zz, q, r)), j
        return None


def cell_K(q, r):
    """the doubles the wall search multiplies zz (or zh) with for the axis of capillary (q, r)"""
    return fr((2.0 * q + r) * 0.86602540378443864676), fr(r * 1.5)


def leak_table_bounds(t):
    """per stride L (PC_L1, PC_L2) and start node i: the exact chord deviation of cap over the block, None where it does not fit"""
    z, cap = [fr(v) for v in t["z"]], [fr(v) for v in t["cap"]]
    n = len(z)
    out = {}
    for L in (t["L1"], t["L2"]):
        rows = []
        for i in range(n):
            if i + L >= n:
                rows.append(None)
                continue
            span = z[i + L] - z[i]
            rows.append(max([abs(cap[j] - (cap[i] + (cap[i + L] - cap[i]) * (z[j] - z[i]) / span)) for j in range(i + 1, i + L)] + [Fraction(0)]))
        out[L] = rows
    return out


def outer_scan(t, c, d):
    """The backward scan of pc_outer_intersect, exactly, for a ray that ended at c on or beyond the last node flying along d
    (dz > 0): the first node j = nmax - 1, nmax - 2, ... 0 at which the ray is not outside the outer hexagon (largest of |y|,
    |C x + y/2|, |C x - y/2| <= sqrt(3)/2 ext, compared in squares) or ext <= 0; None when there is none.  Also the smallest, over
    the nodes scanned, of |largest form - hexd| / bound, bound the first-order running error of the code's evaluation."""
    z, ext, hexd = [fr(v) for v in t["z"]], [fr(v) for v in t["ext"]], [fr(v) for v in t["hexd"]]
    c, d = [fr(v) for v in c], [fr(v) for v in d]
    found, clear = None, None
    # the end point itself comes first: inside the hexagon there (or ext <= 0) the search returns 0 at once
    m = max(abs(c[1]), abs(COSPI_6 * c[0] + c[1] / 2), abs(COSPI_6 * c[0] - c[1] / 2))
    clear = abs(m - hexd[-1]) / (U53 * (3 * (abs(c[0]) + abs(c[1])) + 3 * hexd[-1]))
    if ext[-1] <= 0 or 4 * m * m <= 3 * ext[-1] * ext[-1]:
        return None, clear
    for j in range(len(z) - 2, -1, -1):
        s = (z[j] - c[2]) / d[2]
        dx_, dy_ = d[0] * s, d[1] * s
        x, y = c[0] + dx_, c[1] + dy_
        m = max(abs(y), abs(COSPI_6 * x + y / 2), abs(COSPI_6 * x - y / 2))
        inside = ext[j] <= 0 or 4 * m * m <= 3 * ext[j] * ext[j]
        bound = U53 * (abs(c[0]) + abs(c[1]) + 8 * (abs(dx_) + abs(dy_)) + 3 * (abs(x) + abs(y)) + 3 * hexd[j])
        cl = abs(m - hexd[j]) / bound
        clear = cl if clear is None or cl < clear else clear
        if inside:
            found = j
            break
    return found, clear


# ---------------------------------------------------------------------------------------------------------------------------
# The two ends of a photon's life (tests/test_devmath_ends_cpu.py): the random stream, the quadrant sine / cosine, the source
# sampler (src/polycap-source.c:54-137), the entrance tests of polycap_photon_launch (src/polycap-photon.c:507-645) and the exit
# window (src/polycap-source.c:762-777), from the reference's text: Python integers for the stream, Fractions where the quantities
# are rational, mpmath at EDPS digits for roots and libm.  cos(pi/6) is the double the reference's macro holds wherever the
# reference multiplies with it; its exact value sqrt(3)/2 only where the product's kx is judged.
EDPS = 60
M32 = 0xffffffff


def philox(ctr, key):
    """Philox4x32-10 (Random123) in Python integers: counter (4 words), key (2 words) -> 4 words"""
    c0, c1, c2, c3 = (int(v) & M32 for v in ctr)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(seed, slot, attempt, d):
    """uniform #d of the stream (seed, slot, attempt) as a Fraction k / 2^53: counter (slot_lo, slot_hi, attempt, d >> 1), key
    (seed_lo, seed_hi); even d takes words (0, 1) of the block, odd d words (2, 3); the 64-bit word's upper 53 bits"""
    o = philox((slot & M32, (slot >> 32) & M32, attempt, d >> 1), (seed & M32, (seed >> 32) & M32))
    w = (o[3] << 32 | o[2]) if d & 1 else (o[1] << 32 | o[0])
    return Fraction(w >> 11, 1 << 53)


def _mpq(q):
    """a Fraction (or a double) as an mpf at the working precision"""
    if isinstance(q, Fraction):
        return mp.mpf(q.numerator) / q.denominator
    return mp.mpf(float(q))


def ulp_of(v):
    """spacing of the doubles at |v| (v an mpf or a float; the smallest subnormal at 0)"""
    a = abs(float(v))
    if a < 2.0 ** -1022:
        return 2.0 ** -1074
    return 2.0 ** (math.frexp(a)[1] - 53)


def ulp_err(got, exact_mpf):
    """|got - exact| in units of the spacing of the doubles at the exact value, as a float"""
    with mp.workdps(EDPS):
        return float(abs(mp.mpf(float(got)) - exact_mpf) / mp.mpf(ulp_of(exact_mpf)))


def sincos(x):
    """(sin x, cos x) of the double x as mpf"""
    with mp.workdps(EDPS):
        v = mp.mpf(float(x))
        return mp.sin(v), mp.cos(v)


def hex_distance(radius, x, y):
    """polycap_photon_within_pc_boundary as a signed distance (mpf; working precision of the caller): centre-to-edge distance
    sqrt(radius^2 - (radius/2)^2) minus the largest of |y|, |C x + y/2|, |C x - y/2|, C the reference's double: > 0 inside.
    radius, x, y Fractions."""
    m = max(abs(y), abs(COSPI_6 * x + y / 2), abs(COSPI_6 * x - y / 2))
    return mp.sqrt(_mpq(radius * radius - radius * radius / 4)) - _mpq(m)


def sample_photon(source, cap0, ext0, mono, seed, slot, attempt):
    """polycap_source_get_photon (src/polycap-source.c:54-137) on the stream (seed, slot, attempt).  source = (d_source, src_x,
    src_y, src_sigx, src_sigy, src_shiftx, src_shifty, hor_pol), doubles.  Returns dict(out = the 12 outputs (start, direction,
    electric vector, source point with z = 0) as mpf, hexdist = the smallest |hex_distance| of any tried (x, y) pair in units of
    ext0 (None where no pair is tried), signs = (sign of cos phi, sign of sin phi) from the quadrant rules, e0 = 0 / 1 (horizontal /
    vertical), tries = pairs tried, quadrant = 0..3)."""
    with mp.workdps(EDPS):
        d_source, src_x, src_y, sigx, sigy, shx, shy, hor_pol = (fr(v) for v in source)
        d = 0

        def draw():
            nonlocal d
            u = uniform(seed, slot, attempt, d)
            d += 1
            return u

        r = draw()
        phi = mp.atan(_mpq(src_y / src_x) * mp.tan(2 * mp.pi * _mpq(r) / 4))
        r = draw()
        quadrant = 0
        if Fraction(1, 4) <= r < Fraction(1, 2):
            phi, quadrant = mp.pi - phi, 1
        if Fraction(1, 2) <= r < Fraction(3, 4):
            phi, quadrant = mp.pi + phi, 2
        if r >= Fraction(3, 4):
            phi, quadrant = -phi, 3
        c, s = mp.cos(phi), mp.sin(phi)
        sx_, sy_ = _mpq(src_x), _mpq(src_y)
        max_rad = sx_ * sy_ / mp.sqrt((sy_ * c) ** 2 + (sx_ * s) ** 2)
        r = draw()
        sr = mp.sqrt(_mpq(r))
        srcx, srcy = sr * max_rad * c + _mpq(shx), sr * max_rad * s + _mpq(shy)
        hexdist, tries = None, 0
        if sigx < 0 or sigy < 0:
            if mono:
                x = (2 * draw() - 1) * fr(cap0)
                y = (2 * draw() - 1) * fr(cap0)
            else:
                e0_ = fr(ext0)
                while True:
                    x = (2 * draw() - 1) * e0_
                    y = (2 * draw() - 1) * e0_
                    tries += 1
                    hd = hex_distance(e0_, x, y)
                    rel = abs(hd) / _mpq(e0_)
                    hexdist = rel if hexdist is None or rel < hexdist else hexdist
                    if hd >= 0:
                        break
            x, y = _mpq(x), _mpq(y)
            dx, dy, dz = x - srcx, y - srcy, _mpq(d_source)
        else:
            dx = _mpq(sigx * (1 - 2 * abs(draw())))
            dy = _mpq(sigy * (1 - 2 * abs(draw())))
            dz = mp.mpf(1)
            x, y = srcx + dx * _mpq(d_source) / dz, srcy + dy * _mpq(d_source) / dz
        n = mp.sqrt(dx * dx + dy * dy + dz * dz)
        dx, dy, dz = dx / n, dy / n, dz / n
        frac_hor_pol = (1 + hor_pol) / 2
        r = draw()
        e0 = 0 if abs(r) <= frac_hor_pol else 1
        ex, ey, ez = (mp.mpf(1), mp.mpf(0), mp.mpf(0)) if e0 == 0 else (mp.mpf(0), mp.mpf(1), mp.mpf(0))
        cosalpha = ex * dx + ey * dy + ez * dz
        c_ae = 1 / mp.sin(mp.acos(cosalpha))
        c_be = -c_ae * cosalpha
        ex, ey, ez = ex * c_ae + dx * c_be, ey * c_ae + dy * c_be, ez * c_ae + dz * c_be
        n = mp.sqrt(ex * ex + ey * ey + ez * ez)
        ex, ey, ez = ex / n, ey / n, ez / n
        sign = lambda v: (v > 0) - (v < 0)
        return dict(out=[x, y, mp.mpf(0), dx, dy, dz, ex, ey, ez, srcx, srcy, mp.mpf(0)], hexdist=hexdist, signs=(sign(c), sign(s)),
                    e0=e0, tries=tries, quadrant=quadrant)


def _cube_round(qf, rf):
    """cube rounding of fractional axial coordinates in doubles: a first guess only, never a decision"""
    sf = -qf - rf
    rq, rr, rs = round(qf), round(rf), round(sf)
    dq, dr, ds = abs(qf - rq), abs(rf - rr), abs(sf - rs)
    if dq > dr and dq > ds:
        rq = -rr - rs
    elif dr > ds:
        rr = -rq - rs
    return int(rq), int(rr)


def entrance_profile(z, cap, ext):
    """the profile's doubles as Fractions, once per profile"""
    return dict(z=[fr(v) for v in z], cap=[fr(v) for v in cap], ext=[fr(v) for v in ext], zf=[float(v) for v in z])


def entrance(prof, n_shells, x, y, z):
    """The entrance tests of polycap_photon_launch (src/polycap-photon.c:507-645) for a start point (x, y, z), exactly.
    prof = entrance_profile(...).  Returns dict:
      z_id     last node <= z among 0 .. nmax - 1 (0 for z <= 0): the segment the reference interpolates in
      ix       last node <= z among 0 .. nmax (0 for z <= 0): the segment the photon starts in
      cur_ext  the interpolated exterior radius (Fraction)
      outer    signed distance to the outer boundary, > 0 inside: the hexagon of circum-radius cur_ext, the circle for n_shells = 0
      cells    {(q, r): dict(slack, rad, cx, cy, wall)} for every cell whose closed hexagon holds the point or misses it by no
               more than hex_error_bound (cell units): slack as hex_cells gives it (negative: missed by that much), the interpolated
               radius and centre of the cell's capillary (Fractions) and the signed distance to its wall (float, > 0 inside)
      cell_eb  hex_error_bound at the point
    The mono-capillary has the one cell (0, 0)."""
    with mp.workdps(EDPS):
        Z, CAP, EXT = prof["z"], prof["cap"], prof["ext"]
        nmax = len(Z) - 1
        zf = float(z)
        x, y, zq = fr(x), fr(y), fr(z)
        z_id = ix = 0
        if zf > 0:
            ix = max(0, bisect.bisect_right(prof["zf"], zf) - 1)
            z_id = min(ix, nmax - 1)
        t = (zq - Z[z_id]) / (Z[z_id + 1] - Z[z_id])
        cur_ext = EXT[z_id] + (EXT[z_id + 1] - EXT[z_id]) * t
        out = dict(z_id=z_id, ix=ix, cur_ext=cur_ext, cell_eb=Fraction(0))
        if n_shells == 0:
            out["outer"] = float(_mpq(cur_ext) - mp.sqrt(_mpq(x * x + y * y)))
            cands = {(0, 0): Fraction(1)}
        else:
            out["outer"] = float(hex_distance(cur_ext, x, y))
            zz = cur_ext / (2 * COSPI_6 * (n_shells + 1))
            qf, rf = (x / (2 * COSPI_6) - y / 3) / zz, y * TWO_THIRDS / zz
            eb = hex_error_bound(x, y, zz, qf, rf)
            out["cell_eb"] = eb
            cands = {}
            # The closed hexagons tile the plane: a point inside one cell by the relative slack m misses every other cell by at
            # least m.  The cell that rounding in doubles suggests is tried first, and the neighbourhood only where it does not
            # hold the point by 1e-6.
            q0, r0 = _cube_round(float(qf), float(rf))
            m = min(zz - abs(v) for v in hex_forms(x, y, zz, q0, r0)) / zz
            if m > Fraction(1, 10 ** 6) and m > eb:
                cands[(q0, r0)] = m
            else:
                for q in range(math_floor(qf) - 1, math_floor(qf) + 3):
                    for r in range(math_floor(rf) - 1, math_floor(rf) + 3):
                        m = min(zz - abs(v) for v in hex_forms(x, y, zz, q, r)) / zz
                        if m >= -eb:
                            cands[(q, r)] = m
        cells = {}
        for (q, r), m in cands.items():
            # cap_x[i] = (2 q + r) C ext[i] / (2 C (n_shells + 1)), cap_y[i] = r (3/2) ext[i] / (2 C (n_shells + 1)): :622-627
            hs = 2 * COSPI_6 * (n_shells + 1)
            if zf > 0:
                rad = CAP[z_id] + (CAP[z_id + 1] - CAP[z_id]) * t
                e = cur_ext
            else:
                rad, e = CAP[0], EXT[0]
            cx, cy = (2 * q + r) * COSPI_6 * e / hs, r * Fraction(3, 2) * e / hs
            wall = float(_mpq(rad) - mp.sqrt(_mpq((x - cx) ** 2 + (y - cy) ** 2)))
            cells[(q, r)] = dict(slack=m, rad=rad, cx=cx, cy=cy, wall=wall)
        out["cells"] = cells
        return out


def unit3(v):
    """v / |v| of three doubles as mpf"""
    with mp.workdps(EDPS):
        w = [mp.mpf(float(t)) for t in v]
        n = mp.sqrt(_dot(w, w))
        return [t / n for t in w]


def ray_constants(P, d):
    """(1 / dz, dx / dz, dy / dz, Px - dx/dz Pz, Py - dy/dz Pz) of the unit vector along d (doubles; the norm cancels in all but
    the first), mpf: src/polycap-capil.c:1236-1243"""
    with mp.workdps(EDPS):
        w = [mp.mpf(float(t)) for t in d]
        p = [mp.mpf(float(t)) for t in P]
        n = mp.sqrt(_dot(w, w))
        sx, sy = w[0] / w[2], w[1] / w[2]
        return n / w[2], sx, sy, p[0] - sx * p[2], p[1] - sy * p[2]


def axis_factors(q, r):
    """(kx, ky, |k|) of capillary (q, r) with the exact cos(pi/6): (2 q + r) sqrt(3)/2, 3 r / 2, mpf (src/polycap-photon.c:624-627)"""
    with mp.workdps(EDPS):
        kx, ky = (2 * q + r) * mp.sqrt(3) / 2, mp.mpf(3 * r) / 2
        return kx, ky, mp.sqrt(kx * kx + ky * ky)


def exit_window(z_end, ext_end, mono, P, d):
    """src/polycap-source.c:762-777 exactly: the photon at P flying along d (doubles) extrapolated to z_end; returns (tx, ty)
    (Fractions), the signed distance to the exit hexagon of circum-radius ext_end (the circle for mono), > 0 inside (float), and the
    scale max(|Px|, |Py|, |dx t|, |dy t|, ext_end) (float)"""
    with mp.workdps(EDPS):
        Px, Py, Pz, dx, dy, dz = (fr(v) for v in tuple(P) + tuple(d))
        t = (fr(z_end) - Pz) / dz
        tx, ty = Px + dx * t, Py + dy * t
        e = fr(ext_end)
        dist = float(_mpq(e) - mp.sqrt(_mpq(tx * tx + ty * ty))) if mono else float(hex_distance(e, tx, ty))
        return (tx, ty), dist, float(max(abs(Px), abs(Py), abs(dx * t), abs(dy * t), e))

/*
 * probe_ops.h -- TEST-ONLY: one element of every arithmetic primitive and Fresnel form of pc_device.h, evaluated the way the
 * kernels call it.  Included by tests/devmath/probe.hip (device: the PC_FAST_MATH_DEVICE branch) and by tests/emul/pc_emul.cpp
 * (host: IEEE sqrt, division and exp), so both sides run the same call on the same inputs.
 *
 * Inputs per element, in[PC_PROBE_IN]: c (cos theta), st2, es2, ep2, sd2, fs, fp, w.  The primitives read in[0] (and in[1]
 * for the quotient in[0]/in[1]).  Outputs out[2] and a return code; see the table at PC_PROBE_*.
 *
 * The geometry ops (PC_PROBE_SEGMENT, PC_PROBE_GEOM, PC_PROBE_BOUNCE: the other half of a reflection) have input and output rows
 * of their own widths (pc_probe_in_width, pc_probe_out_width) and an entry point of their own; see pc_probe_geom_eval.
 */
#ifndef PC_PROBE_OPS_H
#define PC_PROBE_OPS_H

#include "pc_problem.h"
#include "pc_device.h"

#define PC_PROBE_IN 8

enum {
	PC_PROBE_SQRT = 0,     /* out0 = pc_sqrt_fast(in0) */
	PC_PROBE_DIV = 1,      /* out0 = pc_div_fast(in0, in1) */
	PC_PROBE_EXP = 2,      /* out0 = pc_exp_neg_fast(in0) */
	PC_PROBE_F3 = 3,       /* out0 = pc_fresnel3(.., pc_refl_cr2(c), c*c, fs, fp) */
	PC_PROBE_F3S = 4,      /* out0 = pc_fresnel3s(.., pc_refl_cr2(c), c*c, es2, ep2, sd2) */
	PC_PROBE_F3X1 = 5,     /* out0 = pc_fresnel3xN<1> */
	PC_PROBE_F3X2 = 6,     /* out0 = pc_fresnel3xN<2> over elements 2t, 2t+1 (one energy per pair) */
	PC_PROBE_FF0 = 7,      /* out0 = rtot, out1 = r_rough, code = pc_fresnel_f<0> */
	PC_PROBE_FF1 = 8,      /* the same for pc_fresnel_f<1> */
	PC_PROBE_RE_FAST = 9,  /* out0 = w, code = pc_reflect_energy_fast */
	PC_PROBE_RE3 = 10,     /* out0 = w, code = pc_reflect_energy3(.., c, c*c, fs, fp) */
	PC_PROBE_RE0 = 11,     /* out0 = w, code = pc_reflect_energy_f<0> */
	PC_PROBE_RE1 = 12,     /* out0 = w, code = pc_reflect_energy_f<1> */
	PC_PROBE_NOPS = 13
};

/* elements one thread evaluates */
static inline int pc_probe_group(int op) { return (op == PC_PROBE_F3X2) ? 2 : 1; }

template <int N>
PC_HD void pc_probe_xN(const pc_energy_const &k, const double *in, double *out)
{
	double q[N][4], rt[N];
	for (int j = 0; j < N; j++) {
		const double c = in[j*PC_PROBE_IN];
		q[j][0] = pc_refl_cr2(c); q[j][1] = c*c; q[j][2] = in[j*PC_PROBE_IN + 5]; q[j][3] = in[j*PC_PROBE_IN + 6];
	}
	pc_fresnel3xN<N>(k.d2, k.n2_re, k.n2_im, k.zi2, q, rt);
	for (int j = 0; j < N; j++) { out[2*j] = rt[j]; out[2*j + 1] = 0.; }
}

/* elements [i, i + pc_probe_group(OP)) of in[], out[] and code[]; k is the energy of element i */
template <int OP>
PC_HD void pc_probe_eval(const pc_energy_const &k, const double *in, double *out, int *code)
{
	const double c = in[0];
	pc_refl_geom g;
	g.alfa = c; g.st2 = in[1]; g.es2 = in[2]; g.ep2 = in[3]; g.sd2 = in[4];
	double w = in[7];
	out[0] = out[1] = 0.;
	code[0] = 0;
	if constexpr (OP == PC_PROBE_SQRT) out[0] = pc_sqrt_fast(in[0]);
	else if constexpr (OP == PC_PROBE_DIV) out[0] = pc_div_fast(in[0], in[1]);
	else if constexpr (OP == PC_PROBE_EXP) out[0] = pc_exp_neg_fast(in[0]);
	else if constexpr (OP == PC_PROBE_F3) out[0] = pc_fresnel3(k.d2, k.n2_re, k.n2_im, k.zi2, pc_refl_cr2(c), c*c, in[5], in[6]);
	else if constexpr (OP == PC_PROBE_F3S) out[0] = pc_fresnel3s(k.d2, k.n2_re, k.n2_im, k.zi2, pc_refl_cr2(c), c*c, in[2], in[3], in[4]);
	else if constexpr (OP == PC_PROBE_F3X1) pc_probe_xN<1>(k, in, out);
	else if constexpr (OP == PC_PROBE_F3X2) { pc_probe_xN<2>(k, in, out); code[1] = 0; }
	else if constexpr (OP == PC_PROBE_FF0 || OP == PC_PROBE_FF1) {
		double rtot = 0., rr = 0.;
		code[0] = (OP == PC_PROBE_FF0) ? pc_fresnel_f<0>(k, g, rtot, rr) : pc_fresnel_f<1>(k, g, rtot, rr);
		out[0] = rtot; out[1] = rr;
	} else if constexpr (OP == PC_PROBE_RE_FAST) { code[0] = pc_reflect_energy_fast(k, g, w); out[0] = w; }
	else if constexpr (OP == PC_PROBE_RE3) { code[0] = pc_reflect_energy3(k, c, c*c, in[5], in[6], w); out[0] = w; }
	else if constexpr (OP == PC_PROBE_RE0) { code[0] = pc_reflect_energy_f<0>(k, g, w); out[0] = w; }
	else if constexpr (OP == PC_PROBE_RE1) { code[0] = pc_reflect_energy_f<1>(k, g, w); out[0] = w; }
}

/* host-side checks shared by both builds: op known, n a whole number of groups, every energy index in range and the same
 * within a group.  Returns 0 or a negative error. */
static inline int pc_probe_check(int op, long long n, const int *e, int ne)
{
	if (op < 0 || op >= PC_PROBE_NOPS || n < 0) return -2;
	const int G = pc_probe_group(op);
	if (n % G) return -2;
	for (long long i = 0; i < n; i++) {
		if (e[i] < 0 || e[i] >= ne) return -2;
		if (i % G && e[i] != e[i - i % G]) return -2;
	}
	return 0;
}

/* ------------------------------------------------------------------ geometry ops
 * Numbered after the arithmetic ops (whose numbers and 8-double rows stay as they are); rows of their own widths.
 *   SEGMENT  in[14] = z0, z1, cap0, cap1, zh0, zh1, kx, ky, Px, Py, Pz, dx, dy, dz    (d a unit vector, P the last interaction point)
 *            out[8] = hx, hy, hz, nx, ny, nz, p0x, p0y; code = pc_segment<1> on the two-node table of the element
 *   GEOM     in[9]  = d, E, n
 *            out[8] = alfa, st2, es2, ep2, sd2, c2, fs, fp; code = pc_reflect_geom (then pc_refl_geom3 when it accepts)
 *   BOUNCE   in[9]  = d, E, n
 *            out[8] = d', E', |d'| - 1, 0: E' as pc_reflect<1> leaves it (FORM 0 at the element's energy), d' as pc_event_post
 *            leaves it for a kept reflection; code = what pc_reflect returned (1 keep, 0 absorbed, -1 error; -1 leaves d, E as given)
 * The two-node table of a SEGMENT element is tab[PC_PROBE_SEG_TAB] = z[2], cap[2], zh[2], idz[2], cap2[2]: z, cap, idz and cap2
 * as pc_build_tables makes them from the element's (z0, z1, cap0, cap1) (pc_probe_seg_table), zh as given.  A profile that
 * pc_build_tables rejects (NaN, cap < 0, z1 <= z0) never reaches a kernel: its element gets PC_PROBE_SETUP_REJECT and is not
 * evaluated. */
enum { PC_PROBE_SEGMENT = 13, PC_PROBE_GEOM = 14, PC_PROBE_BOUNCE = 15, PC_PROBE_GEOM_END = 16 };
#define PC_PROBE_SEG_IN 14
#define PC_PROBE_VEC_IN 9
#define PC_PROBE_GEOM_OUT 8
#define PC_PROBE_SEG_TAB 10
#define PC_PROBE_SETUP_REJECT (-100)

static inline int pc_probe_is_geom(int op) { return op >= PC_PROBE_SEGMENT && op < PC_PROBE_GEOM_END; }
static inline int pc_probe_in_width(int op) { return (op == PC_PROBE_SEGMENT) ? PC_PROBE_SEG_IN : (pc_probe_is_geom(op) ? PC_PROBE_VEC_IN : PC_PROBE_IN); }
static inline int pc_probe_out_width(int op) { return pc_probe_is_geom(op) ? PC_PROBE_GEOM_OUT : 2; }

/* the product's setup (pc_build_tables) of the two-node profile (z0, z1), (cap0, cap1) of a SEGMENT row, glass and energies
 * of p; returns 0, or -1 when the setup rejects the profile */
static inline int pc_probe_seg_table(const pc_hip_problem *p, const double *in, double *tab)
{
	const double z[2] = {in[0], in[1]}, cap[2] = {in[2], in[3]}, ext[2] = {1., 1.};
	pc_hip_problem q = *p;
	q.nmax = 1; q.z = z; q.cap = cap; q.ext = ext;
	pc_host_tables t;
	std::string err;
	for (int j = 0; j < PC_PROBE_SEG_TAB; j++) tab[j] = 0.;
	if (pc_build_tables(&q, t, err)) return -1;
	for (int j = 0; j < 2; j++) { tab[j] = t.z[j]; tab[2 + j] = t.cap[j]; tab[4 + j] = in[4 + j]; tab[6 + j] = t.idz[j]; tab[8 + j] = t.cap2[j]; }
	return 0;
}

/* a photon with every field the geometry reads or pc_event_post touches set: direction and electric vector from v[0..5] */
PC_HD void pc_probe_photon(pc_photon<1> &ph, const double *v)
{
	ph.Px = ph.Py = ph.Pz = 0.;
	ph.dx = v[0]; ph.dy = v[1]; ph.dz = v[2];
	ph.ex = v[3]; ph.ey = v[4]; ph.ez = v[5];
	ph.kx = ph.ky = ph.kn = 0.;
	ph.sx = ph.sy = ph.ox = ph.oy = ph.idzd = ph.C0 = ph.dtravel = 0.;
	ph.w[0] = 1.;
	ph.wmem = nullptr; ph.wstride = 0;
	ph.i = ph.irefl = ph.first = ph.bnd = ph.wset = ph.lv = ph.rc = ph.qr = 0;
}

/* one element of a geometry op: k its energy, in its row, tab its two-node table (SEGMENT only) */
template <int OP>
PC_HD void pc_probe_geom_eval(const pc_energy_const &k, const double *in, const double *tab, double *out, int *code)
{
	for (int j = 0; j < PC_PROBE_GEOM_OUT; j++) out[j] = 0.;
	pc_photon<1> ph;
	if constexpr (OP == PC_PROBE_SEGMENT) {
		const double v[6] = {in[11], in[12], in[13], 0., 0., 0.};
		pc_probe_photon(ph, v);
		pc_tables T;
		T.z = tab; T.cap = tab + 2; T.zh = tab + 4; T.idz = tab + 6; T.cap2 = tab + 8;
		ph.kx = in[6]; ph.ky = in[7];
		ph.Px = in[8]; ph.Py = in[9]; ph.Pz = in[10];
		pc_ray_setup(ph);
		code[0] = pc_segment(T, ph, 0, out[6], out[7], out[0], out[1], out[2], out[3], out[4], out[5]);
	} else {
		pc_probe_photon(ph, in);
		const double nx = in[6], ny = in[7], nz = in[8];
		pc_refl_geom g;
		g.alfa = g.st2 = g.es2 = g.ep2 = g.sd2 = 0.;
		const int rg = pc_reflect_geom(ph, nx, ny, nz, g);
		if constexpr (OP == PC_PROBE_GEOM) {
			code[0] = rg;
			out[0] = g.alfa;
			if (rg == 1) {
				out[1] = g.st2; out[2] = g.es2; out[3] = g.ep2; out[4] = g.sd2;
				pc_refl_geom3(g, out[5], out[6], out[7]);
			}
		} else {
			int r = -1;
			if (rg == 1) {
				pc_params Pm = pc_params();
				Pm.nmax = 1 << 30; Pm.n_energies = 1;
				r = pc_reflect<1>(Pm, &k, ph, nx, ny, nz);
				if (r >= 0) {
					/* pc_event_pre hands pc_event_post the same cosine pc_reflect_geom forms (the same products, summed in
					 * the same order) */
					pc_hit h;
					h.nx = nx; h.ny = ny; h.nz = nz; h.cosalfa = g.alfa; h.ix = 0;
					pc_event_post(Pm, ph, h, 1);
				}
			}
			code[0] = r;
			out[0] = ph.dx; out[1] = ph.dy; out[2] = ph.dz;
			out[3] = ph.ex; out[4] = ph.ey; out[5] = ph.ez;
			out[6] = sqrt(ph.dx*ph.dx + ph.dy*ph.dy + ph.dz*ph.dz) - 1.0;
		}
	}
}

/* host-side checks of a geometry call: op, size, row widths as the caller states them, energy indices */
static inline int pc_probe_geom_check(int op, long long n, int in_w, int out_w, const int *e, int ne)
{
	if (!pc_probe_is_geom(op) || n < 0 || in_w != pc_probe_in_width(op) || out_w != pc_probe_out_width(op)) return -2;
	for (long long i = 0; i < n; i++)
		if (e[i] < 0 || e[i] >= ne) return -2;
	return 0;
}

#endif

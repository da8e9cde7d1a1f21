/*
 * probe_ops.h -- TEST-ONLY: one element of every arithmetic primitive and Fresnel form of pc_device.h, evaluated the way the
 * kernels call it.  Included by tests/devmath/probe.hip (device: the PC_FAST_MATH_DEVICE branch) and by tests/emul/pc_emul.cpp
 * (host: IEEE sqrt, division and exp), so both sides run the same call on the same inputs.
 *
 * Inputs per element, in[PC_PROBE_IN]: c (cos theta), st2, es2, ep2, sd2, fs, fp, w.  The primitives read in[0] (and in[1]
 * for the quotient in[0]/in[1]).  Outputs out[2] and a return code; see the table at PC_PROBE_*.
 */
#ifndef PC_PROBE_OPS_H
#define PC_PROBE_OPS_H

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

#endif

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
 *
 * Op MARCH (PC_PROBE_MARCH) walks one photon per row through the certified march of a whole profile -- pc_launch_init, pc_march_step,
 * pc_event_pre -- and reports every step; see pc_probe_march_eval.
 *
 * The leak ops (PC_PROBE_WALL, PC_PROBE_OUTER, PC_PROBE_HEX) call the wall search of pc_leak.h -- pc_wall_begin, pc_wall_step,
 * pc_wall_probe as pc_leak_launch sequences them; pc_outer_intersect; pc_hex_index -- on the whole profile; see pc_probe_wall_eval.
 *
 * Op FLIGHTS (PC_PROBE_FLIGHTS) is op MARCH carried on through the reflections: after a hit pc_event_post mirrors the direction and
 * the next flight is marched, up to NB flights; see pc_probe_flights_eval.
 *
 * The ops of a photon's two ends (PC_PROBE_SINCOS, PC_PROBE_UNIFORM, PC_PROBE_ENTER, PC_PROBE_EXIT): the quadrant sine / cosine and
 * the random stream of the sampler, everything pc_launch_init leaves, and pc_in_exit_window; see pc_probe_ends_eval.
 */
#ifndef PC_PROBE_OPS_H
#define PC_PROBE_OPS_H

#include "pc_problem.h"
#include "pc_device.h"
#include "pc_leak.h"

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
/* row widths per op (PC_PROBE_MARCH = 16, PC_PROBE_WALL = 17, PC_PROBE_OUTER = 18, PC_PROBE_HEX = 19, PC_PROBE_FLIGHTS = 20,
 * PC_PROBE_SINCOS = 21, PC_PROBE_UNIFORM = 22, PC_PROBE_ENTER = 23, PC_PROBE_EXIT = 24 and their widths are defined with the ops,
 * further down) */
static inline int pc_probe_in_width(int op) { return (op == 21) ? 1 : (op == 22) ? 6 : (op == 23) ? 9 : (op == 24) ? 6 : (op == 20) ? 12 : (op == 17) ? 9 : (op == 18) ? 7 : (op == 19) ? 3 : (op == 16) ? 11 : (op == PC_PROBE_SEGMENT) ? PC_PROBE_SEG_IN : (pc_probe_is_geom(op) ? PC_PROBE_VEC_IN : PC_PROBE_IN); }
static inline int pc_probe_out_width(int op) { return (op == 21) ? 2 : (op == 22) ? 1 : (op == 23) ? 31 : (op == 24) ? 1 : (op == 20) ? 22 + 24*12 + 5*128 : (op == 17) ? 20 + 17*96 : (op == 18) ? 4 : (op == 19) ? 2 : (op == 16) ? 22 + 4*64 : pc_probe_is_geom(op) ? PC_PROBE_GEOM_OUT : 2; }

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

/* ------------------------------------------------------------------ op MARCH
 * One photon per row through the certified march of the WHOLE profile of the problem passed to the call, tables and parameters
 * as pc_build_tables makes them (mg, adj / adjf, bnd_thresh, hexd: what a kernel gets).  Product code only, in this order:
 * pc_launch_init with the row's start; then at most K times pc_march_step and, when that returns EVENT, pc_event_pre: a miss goes
 * on, REFLECT or DONE ends the row.  No reflection is evaluated (no energy enters).  Numbered after the geometry ops; rows of its
 * own widths and an entry point of its own (probe_run_march / emul_probe_run_march).
 *   in[11]   = x, y, z, dx, dy, dz, ex, ey, ez, literal (0 / 1: Pm.literal of this row), K (0 .. PC_PROBE_MARCH_K)
 *   out[278] = entrance [0..9]: state pc_launch_init returned, rc, qr, kx, ky, bnd, i, and the normalised direction d it left
 *              end      [10..21]: how (PC_PROBE_END_*), i, rc, C0, Px, Py, Pz, nx, ny, nz, cosalfa (normal and cosine on REFLECT,
 *                                 else 0), number of trail entries
 *              trail    [22 + 4 t ..]: i before, i after, kind (PC_PROBE_STEP_*), segments the creep loop of pc_event_pre walked
 *                                 in front of its literal visit (literal kinds only), one entry per pass of the loop
 * code = ph.rc at the end. */
enum { PC_PROBE_MARCH = 16 };
#define PC_PROBE_MARCH_IN 11
#define PC_PROBE_MARCH_K 64
#define PC_PROBE_MARCH_HEAD 22
#define PC_PROBE_MARCH_OUT (PC_PROBE_MARCH_HEAD + 4*PC_PROBE_MARCH_K)
#define PC_PROBE_MARCH_NODES 64
enum {
	PC_PROBE_END_STEPS = 0,     /* K passes made, still marching */
	PC_PROBE_END_REFLECT = 1,   /* pc_event_pre found a hit: P is the hit point */
	PC_PROBE_END_EXIT = 2,      /* pc_march_step reached the end of the profile (rc 1) */
	PC_PROBE_END_EVENT = 3,     /* pc_event_pre ended the photon (rc -1) */
	PC_PROBE_END_ENTRANCE = 4   /* pc_launch_init did not let it in (rc 2 / -2) */
};
enum {
	PC_PROBE_STEP_FIRST = 0,    /* first-segment certificate (pc_march_first_ok) */
	PC_PROBE_STEP_SINGLE = 1,   /* pc_march_ok, one segment */
	PC_PROBE_STEP_L1 = 2,       /* pc_march_ok, PC_L1 segments */
	PC_PROBE_STEP_L2 = 3,       /* pc_march_ok, PC_L2 segments */
	PC_PROBE_STEP_LOWER = 4,    /* failed probe that lowered lv; nothing skipped */
	PC_PROBE_STEP_MISS = 5,     /* literal visit without a hit (after `creep` certified single segments) */
	PC_PROBE_STEP_HIT = 6,      /* literal visit with a hit (REFLECT) */
	PC_PROBE_STEP_DONE = 7      /* pc_event_pre ended the photon */
};

/* the device-side view of the profile tables of a MARCH call: n = nmax + 1 entries each, in this order in one buffer of
 * PC_PROBE_MARCH_TAB*n doubles (z, cap, zh, cap2, hexd, idz, ext) plus n pc_marg4 */
#define PC_PROBE_MARCH_TAB 7
PC_HD void pc_probe_march_tables(pc_tables &T, const double *tab, const pc_marg4 *mg, int n)
{
	T.z = tab; T.cap = tab + n; T.zh = tab + 2*n; T.cap2 = tab + 3*n; T.hexd = tab + 4*n; T.idz = tab + 5*n; T.ext = tab + 6*n;
	T.mg = mg;
}

PC_HD void pc_probe_march_eval(const pc_tables &T, const pc_params &Pm0, const double *in, double *out, int *code)
{
	for (int j = 0; j < PC_PROBE_MARCH_OUT; j++) out[j] = 0.;
	pc_params Pm = Pm0;
	Pm.literal = (in[9] != 0.) ? 1 : 0;
	int K = (int)in[10];
	if (K < 0) K = 0;
	if (K > PC_PROBE_MARCH_K) K = PC_PROBE_MARCH_K;
	pc_photon<1> ph;
	const double zero[6] = {0., 0., 0., 0., 0., 0.};
	pc_probe_photon(ph, zero);
	int st = pc_launch_init(T, Pm, ph, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8]);
	out[0] = st; out[1] = ph.rc; out[2] = ph.qr; out[3] = ph.kx; out[4] = ph.ky; out[5] = ph.bnd; out[6] = ph.i;
	out[7] = ph.dx; out[8] = ph.dy; out[9] = ph.dz;
	int how = PC_PROBE_END_STEPS, nt = 0;
	pc_hit h;
	h.nx = h.ny = h.nz = h.cosalfa = 0.; h.ix = 0;
	if (st != PC_ST_MARCH) how = PC_PROBE_END_ENTRANCE;
	for (int t = 0; t < K && how == PC_PROBE_END_STEPS; t++) {
		const int i0 = ph.i, first = ph.first;
		double *tr = out + PC_PROBE_MARCH_HEAD + 4*nt;
		st = pc_march_step(T, Pm, ph);
		if (st == PC_ST_DONE) { how = PC_PROBE_END_EXIT; break; }
		int kind, creep = 0;
		if (st == PC_ST_MARCH) {
			const int adv = ph.i - i0;
			kind = first ? PC_PROBE_STEP_FIRST : (adv == 0) ? PC_PROBE_STEP_LOWER : (adv == 1) ? PC_PROBE_STEP_SINGLE
			     : (adv == PC_L1) ? PC_PROBE_STEP_L1 : PC_PROBE_STEP_L2;
		} else {
			const int crept = (ph.lv == 3);
			st = pc_event_pre(T, Pm, ph, h);
			if (st == PC_ST_MARCH) { kind = PC_PROBE_STEP_MISS; creep = ph.i - 1 - i0; }
			else {
				kind = (st == PC_ST_REFLECT) ? PC_PROBE_STEP_HIT : PC_PROBE_STEP_DONE;
				/* rc 1 from pc_event_pre: its creep loop walked to the end of the profile, the exit pc_march_step reports otherwise */
				how = (st == PC_ST_REFLECT) ? PC_PROBE_END_REFLECT : (ph.rc == 1) ? PC_PROBE_END_EXIT : PC_PROBE_END_EVENT;
				creep = ph.i - i0;
			}
			if (!crept) creep = 0;
		}
		tr[0] = i0; tr[1] = ph.i; tr[2] = kind; tr[3] = creep;
		nt++;
	}
	out[10] = how; out[11] = ph.i; out[12] = ph.rc; out[13] = ph.C0;
	out[14] = ph.Px; out[15] = ph.Py; out[16] = ph.Pz;
	if (how == PC_PROBE_END_REFLECT) { out[17] = h.nx; out[18] = h.ny; out[19] = h.nz; out[20] = h.cosalfa; }
	out[21] = nt;
	code[0] = ph.rc;
}

/* host-side checks of a MARCH call: widths, profile size, K and the literal flag of every row */
static_assert(PC_PROBE_MARCH == 16 && PC_PROBE_MARCH_IN == 11 && PC_PROBE_MARCH_OUT == 22 + 4*64, "widths of op MARCH as pc_probe_in_width / pc_probe_out_width state them");
static inline int pc_probe_march_check(const pc_hip_problem *p, long long n, int in_w, int out_w, const double *in)
{
	if (n < 0 || in_w != pc_probe_in_width(PC_PROBE_MARCH) || out_w != pc_probe_out_width(PC_PROBE_MARCH)) return -2;
	if (p->nmax < 1 || p->nmax + 1 > PC_PROBE_MARCH_NODES) return -2;
	for (long long i = 0; i < n; i++) {
		const double lit = in[i*in_w + 9], K = in[i*in_w + 10];
		if (!(lit == 0. || lit == 1.) || !(K >= 0. && K <= PC_PROBE_MARCH_K) || K != (double)(int)K) return -2;
	}
	return 0;
}

/* ------------------------------------------------------------------ the leak ops
 * Numbered after MARCH; rows of their own widths and an entry point each (probe_run_wall / _outer / _hex and their emul_ twins).
 * Product code only (pc_leak.h), on the tables pc_build_tables makes of the whole profile: z, cap, zh, cap2, hexd, idz, ext, stp,
 * istp, mg, dr.
 *
 * WALL   one photon in the glass per row.  A pc_leak_lane is filled with P, the direction d AS GIVEN (the caller passes a unit
 *        vector; nothing is normalised here, so the row's doubles are the ray), kx = ky = 0 and pc_trace_begin; then
 *        pc_wall_begin(T, Pm, L, PC_LS_INWALL_END, hint) and pc_wall_step / pc_wall_probe as pc_leak_launch sequences them, until the
 *        state returned is PC_LS_INWALL_END or max_units units are spent.
 *   in[9]     = Px, Py, Pz, dx, dy, dz, literal (0 / 1), hint (-1 or a node index), max_units
 *   out[1652] = begin [0..3]: state pc_wall_begin returned, q_i, r_i, z_id (0 when it returned at once)
 *               end   [4..19]: wt, d_travel, q_out, r_out, hx, hy, hz, px, py, pz, nst, dist, z_id, iesc, units used,
 *                              how (PC_PROBE_WALL_FINISHED / _CAPPED)
 *               trail [20 + 17 t ..], one entry for each of the first PC_PROBE_WALL_K units: state called, z_id before, z_id after,
 *                              pz before, pz after, nst before, nst after, q_i, r_i, q_new, r_new, iesc (all after), then five
 *                              columns only a build with PC_LEAK_STATS fills (-1 otherwise: the device has no counters), from the
 *                              counters that moved during the unit: kind (0 certified stretch, 1 literal step, 2 probe unit), blocks
 *                              skipped at level 0, 1, 2, and the visit (0 none, 6 miss, 7 hit).  Units beyond run without a trail.
 *   code = W.wt at the end.
 * OUTER  in[7] = cx, cy, cz, dx, dy, dz, literal;  out[4] = return value of pc_outer_intersect, ox, oy, oz (0 when it returned 0)
 * HEX    in[3] = x, y, zz;  out[2] = q, r of pc_hex_index */
enum { PC_PROBE_WALL = 17, PC_PROBE_OUTER = 18, PC_PROBE_HEX = 19 };
#define PC_PROBE_WALL_IN 9
#define PC_PROBE_WALL_K 96
#define PC_PROBE_WALL_HEAD 20
#define PC_PROBE_WALL_ENTRY 17
#define PC_PROBE_WALL_SHARED 12       /* columns of a trail entry both builds fill */
#define PC_PROBE_WALL_OUT (PC_PROBE_WALL_HEAD + PC_PROBE_WALL_ENTRY*PC_PROBE_WALL_K)
#define PC_PROBE_OUTER_IN 7
#define PC_PROBE_OUTER_OUT 4
#define PC_PROBE_HEX_IN 3
#define PC_PROBE_HEX_OUT 2
#define PC_PROBE_WALL_UNITS_DEVICE 200000LL      /* a lane of the device build is never asked for more units than this */
#define PC_PROBE_WALL_UNITS_HOST 50000000LL
enum { PC_PROBE_WALL_FINISHED = 0, PC_PROBE_WALL_CAPPED = 1 };

/* the device-side view of the tables of a leak op: n = nmax + 1 entries each, in this order in one buffer of PC_PROBE_LEAK_TAB*n
 * doubles (z, cap, zh, cap2, hexd, idz, ext, stp, istp) plus n pc_marg4 and n pc_drdev */
#define PC_PROBE_LEAK_TAB 9
PC_HD void pc_probe_leak_tables(pc_tables &T, const double *tab, const pc_marg4 *mg, const pc_drdev *dr, int n)
{
	pc_probe_march_tables(T, tab, mg, n);
	T.stp = tab + 7*n; T.istp = tab + 8*n;
	T.dr = dr;
}

PC_HD void pc_probe_wall_eval(const pc_tables &T, const pc_params &Pm0, const double *in, double *out, int *code)
{
	for (int j = 0; j < PC_PROBE_WALL_HEAD; j++) out[j] = 0.;       /* the trail is zeroed by the caller */
	pc_params Pm = Pm0;
	Pm.literal = (in[6] != 0.) ? 1 : 0;
	const long long max_units = (long long)in[8];
	pc_leak_lane L;
	L.w = pc_wall();
	pc_photon<0> &ph = L.ph;
	ph.Px = in[0]; ph.Py = in[1]; ph.Pz = in[2];
	ph.dx = in[3]; ph.dy = in[4]; ph.dz = in[5];
	ph.ex = ph.ey = ph.ez = 0.;
	ph.kx = ph.ky = ph.kn = 0.;
	ph.C0 = 0.f; ph.dtravel = 0.;
	ph.w[0] = 1.;
	ph.wmem = nullptr; ph.wstride = 0;
	ph.i = ph.irefl = ph.first = ph.bnd = ph.wset = ph.lv = ph.rc = ph.qr = 0;
	pc_trace_begin(ph);
	pc_wall &W = L.w;
	int st = pc_wall_begin(T, Pm, L, PC_LS_INWALL_END, (int)in[7]);
	out[0] = st;
	if (st != PC_LS_INWALL_END) { out[1] = W.q_i; out[2] = W.r_i; out[3] = W.z_id; }
	long long units = 0;
	int how = PC_PROBE_WALL_FINISHED;
	while (st != PC_LS_INWALL_END) {
		if (units >= max_units) { how = PC_PROBE_WALL_CAPPED; break; }
		const int called = st, z0 = W.z_id;
		const double pz0 = W.pz, nst0 = (double)W.nst;
#ifdef PC_LEAK_STATS
		long long c0[8];
		for (int j = 0; j < 8; j++) c0[j] = pc_leak_stats[j];
#endif
		st = (called == PC_LS_WALL_STEP) ? pc_wall_step(T, Pm, L, L.after_wall) : pc_wall_probe(T, Pm, L, L.after_wall);
		if (units < PC_PROBE_WALL_K) {
			double *tr = out + PC_PROBE_WALL_HEAD + PC_PROBE_WALL_ENTRY*units;
			tr[0] = called; tr[1] = z0; tr[2] = W.z_id; tr[3] = pz0; tr[4] = W.pz; tr[5] = nst0; tr[6] = (double)W.nst;
			tr[7] = W.q_i; tr[8] = W.r_i; tr[9] = W.q_new; tr[10] = W.r_new; tr[11] = W.iesc;
			for (int j = PC_PROBE_WALL_SHARED; j < PC_PROBE_WALL_ENTRY; j++) tr[j] = -1.;
#ifdef PC_LEAK_STATS
			long long c[8];
			for (int j = 0; j < 8; j++) c[j] = pc_leak_stats[j] - c0[j];
			tr[12] = (called == PC_LS_WALL_PROBE) ? 2. : (c[0] ? 0. : 1.);
			tr[13] = (double)c[3]; tr[14] = (double)c[4]; tr[15] = (double)c[5];
			tr[16] = c[7] ? 7. : (c[6] ? 6. : 0.);
#endif
		}
		units++;
	}
	out[4] = W.wt; out[5] = W.d_travel; out[6] = W.q_out; out[7] = W.r_out;
	out[8] = W.hx; out[9] = W.hy; out[10] = W.hz; out[11] = W.px; out[12] = W.py; out[13] = W.pz;
	out[14] = (double)W.nst; out[15] = W.dist; out[16] = W.z_id; out[17] = W.iesc; out[18] = (double)units; out[19] = how;
	code[0] = W.wt;
}

PC_HD void pc_probe_outer_eval(const pc_tables &T, const pc_params &Pm0, const double *in, double *out, int *code)
{
	pc_params Pm = Pm0;
	Pm.literal = (in[6] != 0.) ? 1 : 0;
	double ox = 0., oy = 0., oz = 0.;
	const int r = pc_outer_intersect(T, Pm, in[0], in[1], in[2], in[3], in[4], in[5], ox, oy, oz);
	out[0] = r; out[1] = r ? ox : 0.; out[2] = r ? oy : 0.; out[3] = r ? oz : 0.;
	code[0] = r;
}

PC_HD void pc_probe_hex_eval(const double *in, double *out, int *code)
{
	pc_hex_index(in[0], in[1], in[2], out[0], out[1]);
	code[0] = 0;
}

/* host-side checks of a leak op, in both builds, before anything runs: widths; every value finite; WALL: dz != 0 (pc_wall_step
 * then runs 2^28 units by design -- a hang on a GPU), literal 0 / 1, hint -1 or a node index, max_units a whole number of at most
 * `unit_cap`; OUTER: literal 0 / 1; HEX: zz > 0 */
static_assert(PC_PROBE_WALL_OUT == 20 + 17*96, "widths of op WALL as pc_probe_out_width states them");
static inline int pc_probe_leak_check(const pc_hip_problem *p, int op, long long n, int in_w, int out_w, const double *in, long long unit_cap)
{
	if (op < PC_PROBE_WALL || op > PC_PROBE_HEX || n < 0 || in_w != pc_probe_in_width(op) || out_w != pc_probe_out_width(op)) return -2;
	if (p->nmax < 1) return -2;
	for (long long i = 0; i < n; i++) {
		const double *r = in + i*in_w;
		for (int j = 0; j < in_w; j++)
			if (!std::isfinite(r[j])) return -2;
		if (op == PC_PROBE_WALL) {
			if (r[5] == 0.) return -2;
			if (!(r[6] == 0. || r[6] == 1.)) return -2;
			if (!(r[7] >= -1. && r[7] <= (double)p->nmax) || r[7] != (double)(int)r[7]) return -2;
			if (!(r[8] >= 0. && r[8] <= (double)unit_cap) || r[8] != (double)(long long)r[8]) return -2;
		} else if (op == PC_PROBE_OUTER) {
			if (!(r[6] == 0. || r[6] == 1.)) return -2;
		} else {
			if (!(r[2] > 0.)) return -2;
		}
	}
	return 0;
}

/* ------------------------------------------------------------------ op FLIGHTS
 * Op MARCH carried on through the reflections: one photon per row through the WHOLE profile, flight after flight, tables and
 * parameters as pc_build_tables makes them.  Product code only, in the order the kernels call it: pc_launch_init; then passes of
 * pc_march_step and, when that returns EVENT, pc_event_pre; on REFLECT pc_event_post(Pm, ph, h, 1) -- the geometric reflection -- and
 * the loop goes on with the next flight.  No energy enters and pc_reflect is not called: it writes the weights, wset and the
 * electric vector (its component-wise absolute value) and nothing else of the photon -- neither P, d, the ray nor i, first, lv,
 * C0, irefl -- so the chain of flights is the one a kept reflection (r = 1) leaves at every energy.  Numbered after HEX; rows of
 * its own widths and an entry point of its own (probe_run_flights / emul_probe_run_flights).
 *   in[12]   = x, y, z, dx, dy, dz, ex, ey, ez, literal (0 / 1), K (passes, 0 .. PC_PROBE_FLIGHTS_K), NB (flights, 1 .. PC_PROBE_FLIGHTS_NB)
 *   out[950] = entrance [0..9]: as op MARCH
 *              chain    [10..21]: how it ended (PC_PROBE_CHAIN_*), rc, irefl, flights begun, trail entries, i, P, d at the end
 *              flight f [22 + 24 f ..]: at its start, as pc_trace_begin left the photon: irefl, i, lv, bnd, first, P[3], d[3];
 *                                 at its end: how (PC_PROBE_END_*), i, normal[3] and cosalfa (on a hit, else 0), ix (on a hit),
 *                                 P[3] (the hit point on a hit), C0; two spare columns (0)
 *              trail    [310 + 5 t ..]: flight, i before, i after, kind (PC_PROBE_STEP_*), creep -- one entry per pass, as op MARCH
 * code = ph.rc at the end. */
enum { PC_PROBE_FLIGHTS = 20 };
#define PC_PROBE_FLIGHTS_IN 12
#define PC_PROBE_FLIGHTS_K 128
#define PC_PROBE_FLIGHTS_NB 12
#define PC_PROBE_FLIGHTS_HEAD 22
#define PC_PROBE_FLIGHTS_FL 24
#define PC_PROBE_FLIGHTS_ENTRY 5
#define PC_PROBE_FLIGHTS_TRAIL (PC_PROBE_FLIGHTS_HEAD + PC_PROBE_FLIGHTS_FL*PC_PROBE_FLIGHTS_NB)
#define PC_PROBE_FLIGHTS_OUT (PC_PROBE_FLIGHTS_TRAIL + PC_PROBE_FLIGHTS_ENTRY*PC_PROBE_FLIGHTS_K)
enum {
	PC_PROBE_CHAIN_EXIT = 0,      /* the end of the profile (rc 1), from pc_march_step or the creep loop of pc_event_pre */
	PC_PROBE_CHAIN_EVENT = 1,     /* pc_event_pre ended the photon (rc -1) */
	PC_PROBE_CHAIN_LIMIT = 2,     /* irefl > nmax in pc_event_post (rc 1) */
	PC_PROBE_CHAIN_FLIGHTS = 3,   /* NB flights marched, each ended in a hit; the photon stands at the start of the next */
	PC_PROBE_CHAIN_PASSES = 4,    /* K passes made, still marching */
	PC_PROBE_CHAIN_ENTRANCE = 5   /* pc_launch_init did not let it in (rc 2 / -2) */
};

PC_HD void pc_probe_flights_eval(const pc_tables &T, const pc_params &Pm0, const double *in, double *out, int *code)
{
	for (int j = 0; j < PC_PROBE_FLIGHTS_OUT; j++) out[j] = 0.;
	pc_params Pm = Pm0;
	Pm.literal = (in[9] != 0.) ? 1 : 0;
	int K = (int)in[10], NB = (int)in[11];
	if (K < 0) K = 0;
	if (K > PC_PROBE_FLIGHTS_K) K = PC_PROBE_FLIGHTS_K;
	if (NB < 1) NB = 1;
	if (NB > PC_PROBE_FLIGHTS_NB) NB = PC_PROBE_FLIGHTS_NB;
	pc_photon<1> ph;
	const double zero[6] = {0., 0., 0., 0., 0., 0.};
	pc_probe_photon(ph, zero);
	int st = pc_launch_init(T, Pm, ph, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8]);
	out[0] = st; out[1] = ph.rc; out[2] = ph.qr; out[3] = ph.kx; out[4] = ph.ky; out[5] = ph.bnd; out[6] = ph.i;
	out[7] = ph.dx; out[8] = ph.dy; out[9] = ph.dz;
	int how = (st == PC_ST_MARCH) ? -1 : PC_PROBE_CHAIN_ENTRANCE, nt = 0, nf = 0;
	pc_hit h;
	h.nx = h.ny = h.nz = h.cosalfa = 0.; h.ix = 0;
	double *fl = nullptr;             /* the flight being marched */
	while (how < 0) {
		if (!fl) {
			if (nf == NB) { how = PC_PROBE_CHAIN_FLIGHTS; break; }
			fl = out + PC_PROBE_FLIGHTS_HEAD + PC_PROBE_FLIGHTS_FL*nf;
			fl[0] = ph.irefl; fl[1] = ph.i; fl[2] = ph.lv; fl[3] = ph.bnd; fl[4] = ph.first;
			fl[5] = ph.Px; fl[6] = ph.Py; fl[7] = ph.Pz; fl[8] = ph.dx; fl[9] = ph.dy; fl[10] = ph.dz;
			nf++;
		}
		int end = -1;                 /* how this flight ended, once it has */
		if (nt == K) { how = PC_PROBE_CHAIN_PASSES; end = PC_PROBE_END_STEPS; }
		else {
			const int i0 = ph.i, first = ph.first;
			st = pc_march_step(T, Pm, ph);
			if (st == PC_ST_DONE) { how = PC_PROBE_CHAIN_EXIT; end = PC_PROBE_END_EXIT; }
			else {
				int kind, creep = 0;
				if (st == PC_ST_MARCH) {
					const int adv = ph.i - i0;
					kind = first ? PC_PROBE_STEP_FIRST : (adv == 0) ? PC_PROBE_STEP_LOWER : (adv == 1) ? PC_PROBE_STEP_SINGLE
					     : (adv == PC_L1) ? PC_PROBE_STEP_L1 : PC_PROBE_STEP_L2;
				} else {
					const int crept = (ph.lv == 3);
					st = pc_event_pre(T, Pm, ph, h);
					if (st == PC_ST_MARCH) { kind = PC_PROBE_STEP_MISS; creep = ph.i - 1 - i0; }
					else {
						kind = (st == PC_ST_REFLECT) ? PC_PROBE_STEP_HIT : PC_PROBE_STEP_DONE;
						end = (st == PC_ST_REFLECT) ? PC_PROBE_END_REFLECT : (ph.rc == 1) ? PC_PROBE_END_EXIT : PC_PROBE_END_EVENT;
						if (st != PC_ST_REFLECT) how = (ph.rc == 1) ? PC_PROBE_CHAIN_EXIT : PC_PROBE_CHAIN_EVENT;
						creep = ph.i - i0;
					}
					if (!crept) creep = 0;
				}
				double *tr = out + PC_PROBE_FLIGHTS_TRAIL + PC_PROBE_FLIGHTS_ENTRY*nt;
				tr[0] = nf - 1; tr[1] = i0; tr[2] = ph.i; tr[3] = kind; tr[4] = creep;
				nt++;
			}
		}
		if (end < 0) continue;
		fl[11] = end; fl[12] = ph.i;
		if (end == PC_PROBE_END_REFLECT) { fl[13] = h.nx; fl[14] = h.ny; fl[15] = h.nz; fl[16] = h.cosalfa; fl[17] = h.ix; }
		fl[18] = ph.Px; fl[19] = ph.Py; fl[20] = ph.Pz; fl[21] = ph.C0;
		fl = nullptr;
		if (end == PC_PROBE_END_REFLECT && pc_event_post(Pm, ph, h, 1) == PC_ST_DONE) how = PC_PROBE_CHAIN_LIMIT;
	}
	out[10] = how; out[11] = ph.rc; out[12] = ph.irefl; out[13] = nf; out[14] = nt; out[15] = ph.i;
	out[16] = ph.Px; out[17] = ph.Py; out[18] = ph.Pz; out[19] = ph.dx; out[20] = ph.dy; out[21] = ph.dz;
	code[0] = ph.rc;
}

/* host-side checks of a FLIGHTS call: widths, profile size, every value finite, the literal flag, K and NB of every row */
static_assert(PC_PROBE_FLIGHTS == 20 && PC_PROBE_FLIGHTS_IN == 12 && PC_PROBE_FLIGHTS_OUT == 22 + 24*12 + 5*128, "widths of op FLIGHTS as pc_probe_in_width / pc_probe_out_width state them");
static inline int pc_probe_flights_check(const pc_hip_problem *p, long long n, int in_w, int out_w, const double *in)
{
	if (n < 0 || in_w != pc_probe_in_width(PC_PROBE_FLIGHTS) || out_w != pc_probe_out_width(PC_PROBE_FLIGHTS)) return -2;
	if (p->nmax < 1 || p->nmax + 1 > PC_PROBE_MARCH_NODES) return -2;
	for (long long i = 0; i < n; i++) {
		const double *r = in + i*in_w;
		for (int j = 0; j < in_w; j++)
			if (!std::isfinite(r[j])) return -2;
		if (!(r[9] == 0. || r[9] == 1.)) return -2;
		if (!(r[10] >= 0. && r[10] <= PC_PROBE_FLIGHTS_K) || r[10] != (double)(int)r[10]) return -2;
		if (!(r[11] >= 1. && r[11] <= PC_PROBE_FLIGHTS_NB) || r[11] != (double)(int)r[11]) return -2;
	}
	return 0;
}

/* ------------------------------------------------------------------ the ops of a photon's two ends
 * Numbered after FLIGHTS; rows of their own widths and an entry point each (probe_run_sincos / _uniform / _enter / _exit and their
 * emul_ twins).  Product code only, called as the kernels call it.
 *   SINCOS   in[1]  = x (0 <= x <= 2: the sampler passes [0, pi/2));  out[2] = sn, cs of pc_sincos_quadrant(x)
 *   UNIFORM  in[6]  = seed_lo, seed_hi, slot_lo, slot_hi, attempt, d: 32-bit values carried in doubles, d <= PC_PROBE_UNIFORM_D
 *            out[1] = uniform #d of the stream (seed, slot, attempt): pc_rng_init, then pc_rng_uniform d + 1 times, so that an odd
 *                     d takes the second half of the block its predecessor drew
 *   ENTER    in[9]  = x, y, z, dx, dy, dz, ex, ey, ez, as the first nine columns of op MARCH
 *            out[31] = what pc_launch_init leaves (PC_PROBE_ENTER_OUT): the state it returned, rc, q, r (decoded from qr; 0 where it
 *                     returned before qr was set: rc -2), qr, kx, ky, kn, bnd, i, P[3], d[3], E[3], first, lv, idzd, sx, sy, ox, oy,
 *                     irefl, dtravel, C0, w[0], wset.  The photon is zeroed before the call (pc_probe_photon), so a field the call
 *                     does not reach reads 0.  Tables and parameters as pc_build_tables makes them of the whole profile.
 *   EXIT     in[6]  = Px, Py, Pz, dx, dy, dz;  out[1] = pc_in_exit_window on the problem's Pm (z_end, ext_end, mono)
 * code = rc (ENTER), the answer (EXIT), 0 otherwise. */
enum { PC_PROBE_SINCOS = 21, PC_PROBE_UNIFORM = 22, PC_PROBE_ENTER = 23, PC_PROBE_EXIT = 24 };
#define PC_PROBE_SINCOS_IN 1
#define PC_PROBE_SINCOS_OUT 2
#define PC_PROBE_UNIFORM_IN 6
#define PC_PROBE_UNIFORM_OUT 1
#define PC_PROBE_UNIFORM_D 4095
#define PC_PROBE_ENTER_IN 9
#define PC_PROBE_ENTER_OUT 31
#define PC_PROBE_EXIT_IN 6
#define PC_PROBE_EXIT_OUT 1

template <int OP>
PC_HD void pc_probe_ends_eval(const pc_tables &T, const pc_params &Pm, const double *in, double *out, int *code)
{
	code[0] = 0;
	if constexpr (OP == PC_PROBE_SINCOS) {
		pc_sincos_quadrant(in[0], out[0], out[1]);
	} else if constexpr (OP == PC_PROBE_UNIFORM) {
		const uint64_t seed = ((uint64_t)(uint32_t)in[1] << 32) | (uint32_t)in[0], slot = ((uint64_t)(uint32_t)in[3] << 32) | (uint32_t)in[2];
		const uint32_t d = (uint32_t)in[5];
		pc_rng g;
		pc_rng_init(g, seed, slot, (uint32_t)in[4]);
		double u = 0.;
		for (uint32_t j = 0; j <= d; j++) u = pc_rng_uniform(g);
		out[0] = u;
	} else if constexpr (OP == PC_PROBE_ENTER) {
		pc_photon<1> ph;
		const double zero[6] = {0., 0., 0., 0., 0., 0.};
		pc_probe_photon(ph, zero);
		const int st = pc_launch_init(T, Pm, ph, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8]);
		const int has_qr = (st == PC_ST_MARCH || ph.rc == 2);
		out[0] = st; out[1] = ph.rc;
		out[2] = has_qr ? (double)((int)((unsigned)ph.qr >> 16) - 32768) : 0.;
		out[3] = has_qr ? (double)((ph.qr & 0xffff) - 32768) : 0.;
		out[4] = ph.qr; out[5] = ph.kx; out[6] = ph.ky; out[7] = ph.kn; out[8] = ph.bnd; out[9] = ph.i;
		out[10] = ph.Px; out[11] = ph.Py; out[12] = ph.Pz; out[13] = ph.dx; out[14] = ph.dy; out[15] = ph.dz;
		out[16] = ph.ex; out[17] = ph.ey; out[18] = ph.ez; out[19] = ph.first; out[20] = ph.lv;
		out[21] = ph.idzd; out[22] = ph.sx; out[23] = ph.sy; out[24] = ph.ox; out[25] = ph.oy;
		out[26] = ph.irefl; out[27] = ph.dtravel; out[28] = ph.C0; out[29] = ph.w[0]; out[30] = ph.wset;
		code[0] = ph.rc;
	} else {
		pc_photon<1> ph;
		const double v[6] = {in[3], in[4], in[5], 0., 0., 0.};
		pc_probe_photon(ph, v);
		ph.Px = in[0]; ph.Py = in[1]; ph.Pz = in[2];
		const int ok = pc_in_exit_window(Pm, ph);
		out[0] = ok;
		code[0] = ok;
	}
}

/* host-side checks of an ends op, in both builds, before anything runs: op, widths, every value finite; SINCOS: 0 <= x <= 2;
 * UNIFORM: whole numbers below 2^32, d <= PC_PROBE_UNIFORM_D (a lane draws d + 1 uniforms) */
static_assert(PC_PROBE_ENTER == 23 && PC_PROBE_ENTER_OUT == 31, "widths of the ends ops as pc_probe_in_width / pc_probe_out_width state them");
static inline int pc_probe_ends_check(const pc_hip_problem *p, int op, long long n, int in_w, int out_w, const double *in)
{
	if (op < PC_PROBE_SINCOS || op > PC_PROBE_EXIT || n < 0 || in_w != pc_probe_in_width(op) || out_w != pc_probe_out_width(op)) return -2;
	if (p->nmax < 1) return -2;
	for (long long i = 0; i < n; i++) {
		const double *r = in + i*in_w;
		for (int j = 0; j < in_w; j++)
			if (!std::isfinite(r[j])) return -2;
		if (op == PC_PROBE_SINCOS && !(r[0] >= 0. && r[0] <= 2.)) return -2;
		if (op == PC_PROBE_UNIFORM) {
			for (int j = 0; j < in_w; j++)
				if (!(r[j] >= 0. && r[j] <= 4294967295.) || r[j] != (double)(uint32_t)r[j]) return -2;
			if (r[5] > (double)PC_PROBE_UNIFORM_D) return -2;
		}
	}
	return 0;
}

#endif

/*
 * pc_emit_layers.h -- layered emits: an emit relay through a stack of sample layers (include/polycap-hip.h, pc_hip_layers_*).  The
 * geometry is the slab emit's with the stack's total thickness, restated here so that pc_emit.h stays as it is; on top of it every
 * photon finds the layer its interaction lies in, once, and every energy takes that layer's production coefficient and the optical
 * depths of the two rays through the layers in front of and behind the interaction, from prefix tables that the host sums once per
 * call.  One more injection rule of the relay's kernels, pc_rule_layers, beside pc_rule_emit and pc_rule_slab.
 *
 * As in pc_emit.h, the first part compiles for the host as well: -DPC_EMIT_HOST_ONLY stops the header after it.
 */
#ifndef PC_EMIT_LAYERS_H
#define PC_EMIT_LAYERS_H

#include "pc_emit.h"

#define PC_EMIT_MAX_LAYERS 16      /* PC_HIP_MAX_LAYERS of include/polycap-hip.h */

/* the twenty-one numbers of a layered frame: the slab's twenty with T = the stack's total thickness, then qmax */
enum { PC_EMIT_LAYERS_QMAX = PC_EMIT_SLAB_N_FRAME, PC_EMIT_LAYERS_N_FRAME = PC_EMIT_SLAB_N_FRAME + 1 };
/* the eighteen numbers of a layered state: the emit's nine, then */
enum { PC_LAYERS_T = 9, PC_LAYERS_R, PC_LAYERS_GL, PC_LAYERS_S, PC_LAYERS_SD, PC_LAYERS_CN, PC_LAYERS_A, PC_LAYERS_B, PC_LAYERS_J, PC_LAYERS_N_STATE };

/* what pc_emit_layers_bad found */
enum { PC_LAYERS_BAD_N = 1, PC_LAYERS_BAD_THICKNESS, PC_LAYERS_BAD_TOTAL, PC_LAYERS_BAD_MU_IN, PC_LAYERS_BAD_MU_OUT, PC_LAYERS_BAD_PRODUCTION };

/* the boundaries of a stack: Z[0] = 0, Z[j + 1] = Z[j] + thickness[j], summed left to right; Z[n] is the total thickness T */
static inline void pc_emit_layers_bounds(int n, const double *thickness, double *Z)
{
	Z[0] = 0.;
	for (int j = 0; j < n; j++) Z[j + 1] = Z[j] + thickness[j];
}

/* What a stack's spec adds to the emit's: 0 when it is valid, else the first of PC_LAYERS_BAD_N (n outside 1 .. 16),
 * _THICKNESS (thickness[*layer] not finite or not in (0, 1]), _TOTAL (the boundaries' last above 1), _MU_IN, _MU_OUT, _PRODUCTION
 * (entry *at of row *layer not finite or negative).  The tables are row-major by layer: mu_in [n][n_in], mu_out and production
 * [n][n_out]. */
static inline int pc_emit_layers_bad(int n, const double *thickness, int n_in, const double *mu_in, int n_out, const double *mu_out,
	const double *production, int *layer, int *at)
{
	*layer = -1; *at = -1;
	if (n < 1 || n > PC_EMIT_MAX_LAYERS) return PC_LAYERS_BAD_N;
	for (int j = 0; j < n; j++)
		if (!(thickness[j] > 0. && thickness[j] <= 1.)) { *layer = j; return PC_LAYERS_BAD_THICKNESS; }
	double Z[PC_EMIT_MAX_LAYERS + 1];
	pc_emit_layers_bounds(n, thickness, Z);
	if (!(Z[n] <= 1.)) return PC_LAYERS_BAD_TOTAL;
	const double *const tab[3] = { mu_in, mu_out, production };
	const int len[3] = { n_in, n_out, n_out };
	for (int k = 0; k < 3; k++)
		for (int j = 0; j < n; j++)
			for (int e = 0; e < len[k]; e++) {
				const double v = tab[k][(long long)j*len[k] + e];
				if (!(v >= 0. && v <= 1.7976931348623157e308)) { *layer = j; *at = e; return PC_LAYERS_BAD_MU_IN + k; }
			}
	return 0;
}

/* the largest entry of a valid production table [n][n_out]: the frame's qmax */
static inline double pc_emit_layers_qmax(int n, int n_out, const double *production)
{
	double q = 0.;
	for (long long k = 0; k < (long long)n*n_out; k++)
		if (production[k] > q) q = production[k];
	return q;
}

/* The frame of a valid layered spec: the slab's with the total thickness T = Z[n], then qmax.  Host only. */
static inline void pc_emit_layers_frame(const double *f, double T, double qmax, double *fr)
{
	pc_emit_slab_frame(f, T, fr);
	fr[PC_EMIT_LAYERS_QMAX] = qmax;
}

/* The prefix tables of a stack, in plain doubles, each product formed before its add:
 *   pin [j][e] = sum_{k<j} mu_in [k][e]*thickness[k]     added left to right      [n][n_in]
 *   pout[j][e] = sum_{k<j} mu_out[k][e]*thickness[k]     added left to right      [n][n_out]
 *   sout[j][e] = sum_{k>j} mu_out[k][e]*thickness[k]     added right to left      [n][n_out]
 * Host only. */
static inline void pc_emit_layers_tables(int n, const double *thickness, int n_in, const double *mu_in, int n_out, const double *mu_out,
	double *pin, double *pout, double *sout)
{
	for (int e = 0; e < n_in; e++) {
		double acc = 0.;
		for (int j = 0; j < n; j++) {
			pin[(long long)j*n_in + e] = acc;
			const double m = mu_in[(long long)j*n_in + e]*thickness[j];
			acc = acc + m;
		}
	}
	for (int e = 0; e < n_out; e++) {
		double acc = 0.;
		for (int j = 0; j < n; j++) {
			pout[(long long)j*n_out + e] = acc;
			const double m = mu_out[(long long)j*n_out + e]*thickness[j];
			acc = acc + m;
		}
		acc = 0.;
		for (int j = n - 1; j >= 0; j--) {
			sout[(long long)j*n_out + e] = acc;
			const double m = mu_out[(long long)j*n_out + e]*thickness[j];
			acc = acc + m;
		}
	}
}

/* pc_emit_slab_at for a stack of n layers with the boundaries Z [n + 1] (fr's T is Z[n]): the contract of include/polycap-hip.h,
 * operation by operation.  The slab's geometry, then the layer of the interaction, j = the number of inner boundaries Z[1 .. n - 1]
 * at or below zn, so that a point on a boundary belongs to the layer behind it and a zn that rounding carried past T stays in the
 * last one; its offsets a = zn - Z[j] and b = Z[j + 1] - zn, set to 0 when negative; and the guard !(gl*qmax < 1).  Returns
 * PC_EMIT_INJECT and out = {the emit's nine, t, r, gl, s, sd, cn, a, b, j}, or PC_EMIT_MISS_SAMPLE / PC_EMIT_MISS_DETECTOR: out is
 * then not written. */
static inline __host__ __device__ int pc_emit_layers_at(double x, double y, double dx, double dy, int odd, const double *fr, double R,
	int n, const double *Z, double u1, double u2, double u3, double *out)
{
	const double *ns = fr + PC_EMIT_NS, *u = fr + PC_EMIT_U, *v = fr + PC_EMIT_V, *nn = fr + PC_EMIT_N, *c = fr + PC_EMIT_CB, *k = fr + PC_EMIT_SLAB_K;
	const double T = fr[PC_EMIT_SLAB_T];
	const double dz = sqrt((1. - dx*dx) - dy*dy);
	const double sd = (ns[0]*dx + ns[1]*dy) + ns[2]*dz;
	const double sp = fr[PC_EMIT_HS] - (ns[0]*x + ns[1]*y);
	if (!(sd > 0.) || !(sp >= 0.)) return PC_EMIT_MISS_SAMPLE;
	const double t = sp / sd;
	const double p0 = x + dx*t, p1 = y + dy*t, p2 = dz*t;
	const double L = T / sd;
	const double s = u3*L, zn = s*sd;
	const double pp0 = p0 + dx*s, pp1 = p1 + dy*s, pp2 = p2 + dz*s;
	const double a = (2.*u1 - 1.)*R, b = (2.*u2 - 1.)*R;
	const double q0 = c[0] - pp0, q1 = c[1] - pp1, q2 = c[2] - pp2;
	const double f0 = a + ((u[0]*q0 + u[1]*q1) + u[2]*q2);
	const double f1 = b + ((v[0]*q0 + v[1]*q1) + v[2]*q2);
	const double f2 = (nn[0]*q0 + nn[1]*q1) + nn[2]*q2;
	if (!(f2 > 0.)) return PC_EMIT_MISS_DETECTOR;
	const double r2 = (f0*f0 + f1*f1) + f2*f2;
	const double r = sqrt(r2);
	const double d0 = f0/r, d1 = f1/r, d2 = f2/r;
	const double g = ((R*R)*d2) / (PC_EMIT_PI*r2);
	const double h = sqrt(d2*d2 + d0*d0);
	const double cn = ((k[0]*f0 + k[1]*f1) + k[2]*f2) / r;
	if (!(cn > 0.) && !(cn < 0.)) return PC_EMIT_MISS_DETECTOR;
	const double gl = g*L;
	if (!(gl*fr[PC_EMIT_LAYERS_QMAX] < 1.)) return PC_EMIT_MISS_SAMPLE;
	int j = 0;
	for (int i = 1; i < n; i++) j += (zn >= Z[i]) ? 1 : 0;
	const double za = zn - Z[j];
	double zb = Z[j + 1] - zn;
	if (zb < 0.) zb = 0.;
	out[0] = a; out[1] = b; out[2] = 0.;
	out[3] = d0; out[4] = d1; out[5] = d2;
	if (!odd) {
		out[6] = d2/h; out[7] = 0.; out[8] = 0. - d0/h;
	} else {
		out[6] = 0. - (d0*d1)/h; out[7] = h; out[8] = 0. - (d1*d2)/h;
	}
	out[PC_LAYERS_T] = t; out[PC_LAYERS_R] = r; out[PC_LAYERS_GL] = gl; out[PC_LAYERS_S] = s;
	out[PC_LAYERS_SD] = sd; out[PC_LAYERS_CN] = cn; out[PC_LAYERS_A] = za; out[PC_LAYERS_B] = zb; out[PC_LAYERS_J] = (double)j;
	return PC_EMIT_INJECT;
}

/* one exit photon of the first optic at the stack and on to the target: pc_emit_layers_at with draws 0, 1 and 2 of the stream of its
 * slot, the slab's three */
static inline __host__ __device__ int pc_emit_layers_state(double x, double y, double dx, double dy, uint64_t slot, const double *fr, double R,
	int n, const double *Z, uint64_t seed, double *out)
{
	pc_rng rng;
	pc_rng_init(rng, seed, slot, 0u);
	const double u1 = pc_rng_uniform(rng), u2 = pc_rng_uniform(rng), u3 = pc_rng_uniform(rng);
	return pc_emit_layers_at(x, y, dx, dy, (int)(slot & 1ull), fr, R, n, Z, u1, u2, u3, out);
}

/* the optical depth of one ray between the interaction and a face: (acc + mu*x) / c, with
 *   the way in                   acc = pin [j][ea],  mu = mu_in [j][ea],  x = a,  c = sd
 *   out through the back         acc = sout[j][e],   mu = mu_out[j][e],   x = b,  c = cn         (cn > 0)
 *   out through the front        acc = pout[j][e],   mu = mu_out[j][e],   x = a,  c = 0 - cn     (cn < 0) */
static inline __host__ __device__ double pc_emit_layers_tau(double acc, double mu, double x, double c)
{
	return (acc + mu*x) / c;
}

/* weight of a photon behind both optics and the stack between them: w = ((wA * gl) * (q * E(0 - (tau_in + tau_out)))) * wB, q the
 * production coefficient of the layer of interaction */
static inline __host__ __device__ double pc_emit_layers_weight(double w_a, double gl, double q, double tau_in, double tau_out, double w_b)
{
	const double att = pc_emit_exp_neg(0. - (tau_in + tau_out));
	return ((w_a*gl)*(q*att))*w_b;
}

/* The weight of the photon with the state o at one energy of the second optic: the two optical depths from the tables' entries ki (row
 * j of the tables over the first optic's energies) and ko (row j of those over the second optic's), the way out by the sign of cn. */
static inline __host__ __device__ double pc_emit_layers_weight_at(const double *o, double w_a, const double *pin, const double *mu_in, long long ki,
	const double *sout, const double *pout, const double *mu_out, const double *prod, long long ko, double w_b)
{
	const double cn = o[PC_LAYERS_CN];
	const double tau_in = pc_emit_layers_tau(pin[ki], mu_in[ki], o[PC_LAYERS_A], o[PC_LAYERS_SD]);
	const double tau_out = cn > 0. ? pc_emit_layers_tau(sout[ko], mu_out[ko], o[PC_LAYERS_B], cn)
	                               : pc_emit_layers_tau(pout[ko], mu_out[ko], o[PC_LAYERS_A], 0. - cn);
	return pc_emit_layers_weight(w_a, o[PC_LAYERS_GL], prod[ko], tau_in, tau_out, w_b);
}

/* path of a photon behind both optics: the slab's */
static inline __host__ __device__ double pc_emit_layers_dtravel(double d_a, double t, double s, double r, double d_b)
{
	return (((d_a + t) + s) + r) + d_b;
}

#ifndef PC_EMIT_HOST_ONLY

static_assert(PC_EMIT_MAX_LAYERS == PC_HIP_MAX_LAYERS, "the header's limit is the contract's");

struct pc_emit_layers_place {
	double fr[PC_EMIT_LAYERS_N_FRAME], R;
	unsigned long long seed;
	long long slot0;            /* as pc_emit_place's */
	const long long *ids;
	const int *emap;
	int n, n_in, n_out;         /* layers; energies of the first and of the second optic: the tables' row lengths */
	/* in the second context's relay table buffer: the boundaries [n + 1]; mu_in and pin [n][n_in]; mu_out, sout, pout and the
	 * production coefficients [n][n_out] */
	const double *Z, *mu_in, *pin, *mu_out, *sout, *pout, *prod;
};

/* The stack as an injection rule: pc_emit_layers_state on the stream of the entry's slot, the emit rule's order of questions; the
 * weight, the only place that reads the tables; the slab's path. */
struct pc_rule_layers {
	typedef pc_emit_layers_place place;
	enum { N_STATE = PC_LAYERS_N_STATE, KIND = PC_RELAY_KIND_EMIT };
	static __device__ __forceinline__ int fly(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		const double *e = s.p + i*s.ss;
		const double x = e[(long long)PC_F_EXITX*s.fs], y = e[(long long)PC_F_EXITY*s.fs], dx = e[(long long)PC_F_EDIRX*s.fs], dy = e[(long long)PC_F_EDIRY*s.fs];
		const long long slot = pl.slot0 + (pl.ids ? pl.ids[i] : i);
		return pc_emit_layers_state(x, y, dx, dy, (uint64_t)slot, pl.fr, pl.R, pl.n, pl.Z, pl.seed, o);
	}
	static __device__ __forceinline__ void state(const pc_spot_src &s, const place &pl, long long ia, double *o) { (void)fly(s, pl, ia, o); }
	static __device__ __forceinline__ int entry(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		if (!pc_relay_src_valid(s, i)) return PC_RELAY_SKIP;
		if (s.mask && !s.mask[i]) return PC_RELAY_REJECT;
		return fly(s, pl, i, o);
	}
	static __device__ __forceinline__ double weight(const pc_spot_src &s, const place &pl, long long ia, int en, const double *o, double w_b)
	{
		const int ea = pl.emap[en];
		const long long ki = (long long)o[PC_LAYERS_J]*pl.n_in + ea, ko = (long long)o[PC_LAYERS_J]*pl.n_out + en;
		return pc_emit_layers_weight_at(o, s.w[ia*s.ws + ea], pl.pin, pl.mu_in, ki, pl.sout, pl.pout, pl.mu_out, pl.prod, ko, w_b);
	}
	static __device__ __forceinline__ double dtravel(double d_a, const double *o, double d_b)
	{
		return pc_emit_layers_dtravel(d_a, o[PC_LAYERS_T], o[PC_LAYERS_S], o[PC_LAYERS_R], d_b);
	}
};

/* the stack's spec alone: its emit, the layers, and three tables that are lists of coefficients, a row per layer */
static int pc_emit_layers_check_spec(const pc_hip_layers *sp, const std::string &w)
{
	if (!sp) return pc_fail(PC_HIP_ERR_INVALID, w + ": spec must not be NULL");
	const int st = pc_emit_check_spec(&sp->emit, w);
	if (st) return st;
	const std::string bad_n = w + ": n_layers is " + std::to_string(sp->n_layers) + ", outside 1 .. " + std::to_string(PC_HIP_MAX_LAYERS);
	if (sp->n_layers < 1 || sp->n_layers > PC_HIP_MAX_LAYERS) return pc_fail(PC_HIP_ERR_INVALID, bad_n);
	if (!sp->thickness) return pc_fail(PC_HIP_ERR_INVALID, w + ": thickness must hold n_layers entries");
	if (!sp->mu_in || sp->n_mu_in < 1) return pc_fail(PC_HIP_ERR_INVALID, w + ": n_mu_in must be the length of mu_in's rows, at least 1");
	if (!sp->mu_out || sp->n_mu_out < 1) return pc_fail(PC_HIP_ERR_INVALID, w + ": n_mu_out must be the length of mu_out's rows, at least 1");
	if (!sp->production) return pc_fail(PC_HIP_ERR_INVALID, w + ": production must hold n_layers rows of n_mu_out entries");
	int layer = -1, at = -1;
	const int bad = pc_emit_layers_bad(sp->n_layers, sp->thickness, sp->n_mu_in, sp->mu_in, sp->n_mu_out, sp->mu_out, sp->production, &layer, &at);
	static const char *const table[3] = { "mu_in", "mu_out", "production" };
	switch (bad) {
	case 0: return PC_HIP_OK;
	case PC_LAYERS_BAD_N: return pc_fail(PC_HIP_ERR_INVALID, bad_n);
	case PC_LAYERS_BAD_THICKNESS:
		return pc_fail(PC_HIP_ERR_INVALID, w + ": thickness[" + std::to_string(layer) + "] is not valid (finite, above 0 and at most 1 cm)");
	case PC_LAYERS_BAD_TOTAL: return pc_fail(PC_HIP_ERR_INVALID, w + ": the total thickness of the layers is above 1 cm");
	default:
		return pc_fail(PC_HIP_ERR_INVALID, w + ": " + table[bad - PC_LAYERS_BAD_MU_IN] + "[" + std::to_string(layer) + "][" + std::to_string(at)
		               + "] is not valid (finite and >= 0)");
	}
}

static void pc_emit_layers_spec_frame(const pc_hip_layers *sp, double *fr)
{
	const pc_hip_emit *e = &sp->emit;
	const double f[PC_EMIT_N_FIELDS] = { e->focus, e->sample_angle, e->depth, e->det_angle, e->wd, e->off_u, e->off_v, e->target_half };
	double Z[PC_HIP_MAX_LAYERS + 1];
	pc_emit_layers_bounds(sp->n_layers, sp->thickness, Z);
	pc_emit_layers_frame(f, Z[sp->n_layers], pc_emit_layers_qmax(sp->n_layers, sp->n_mu_out, sp->production), fr);
}

/* what the pair of contexts can refuse of a valid layered spec: what it refuses of the emit, then a table whose rows are not as
 * long as its context's grid */
static int pc_emit_layers_check_pair(const pc_hip_ctx *a, const pc_hip_ctx *b, const pc_hip_layers *sp, const std::string &w, std::vector<int> &emap)
{
	const int st = pc_emit_check_pair(a, b, &sp->emit, w, emap);
	if (st) return st;
	if ((size_t)sp->n_mu_in != a->energies.size())
		return pc_fail(PC_HIP_ERR_INVALID, w + ": n_mu_in is " + std::to_string(sp->n_mu_in) + ", but the first context has " + std::to_string(a->energies.size()) + " energies");
	if ((size_t)sp->n_mu_out != b->energies.size())
		return pc_fail(PC_HIP_ERR_INVALID, w + ": n_mu_out is " + std::to_string(sp->n_mu_out) + ", but the second context has " + std::to_string(b->energies.size()) + " energies");
	return PC_HIP_OK;
}

extern "C" {

int pc_hip_layers_validate(const pc_hip_layers *spec)
{
	return pc_emit_layers_check_spec(spec, "pc_hip_layers_validate");
}

int pc_hip_layers_frame(const pc_hip_layers *spec, double frame[21])
{
	if (!frame) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_layers_frame: frame must not be NULL");
	const int st = pc_emit_layers_check_spec(spec, "pc_hip_layers_frame");
	if (st) return st;
	pc_emit_layers_spec_frame(spec, frame);
	return PC_HIP_OK;
}

int pc_hip_layers_run(pc_hip_ctx *a, pc_hip_ctx *b, const pc_hip_layers *spec, pc_hip_select *select)
{
	const char *who = "pc_hip_layers_run";
	const std::string w(who);
	int st = pc_relay_check_pair(a, b, w);
	if (!st) st = pc_emit_layers_check_spec(spec, w);
	if (st) return st;
	std::vector<int> emap;
	pc_spot_src s;
	int64_t cnt_a[6];
	st = pc_relay_open(a, b, who, select, spec->emit.map == nullptr, [&] { return pc_emit_layers_check_pair(a, b, spec, w, emap); }, s, cnt_a);
	if (st) return st;
	pc_emit_layers_place pl;
	pc_emit_layers_spec_frame(spec, pl.fr);
	pl.R = spec->emit.target_half;
	pl.seed = spec->emit.seed;
	pl.slot0 = a->run_slot0;
	pl.ids = a->img.device_view().ids;
	pl.n = spec->n_layers; pl.n_in = spec->n_mu_in; pl.n_out = spec->n_mu_out;
	/* the tables in the order of the place's pointers, one host block and one copy */
	const size_t n = (size_t)pl.n, t_in = n*(size_t)pl.n_in, t_out = n*(size_t)pl.n_out;
	std::vector<double> tab(n + 1 + 2*t_in + 4*t_out);
	double *h_Z = tab.data(), *h_mu_in = h_Z + n + 1, *h_pin = h_mu_in + t_in, *h_mu_out = h_pin + t_in, *h_sout = h_mu_out + t_out,
	       *h_pout = h_sout + t_out, *h_prod = h_pout + t_out;
	pc_emit_layers_bounds(pl.n, spec->thickness, h_Z);
	std::copy(spec->mu_in, spec->mu_in + t_in, h_mu_in);
	std::copy(spec->mu_out, spec->mu_out + t_out, h_mu_out);
	std::copy(spec->production, spec->production + t_out, h_prod);
	pc_emit_layers_tables(pl.n, spec->thickness, pl.n_in, spec->mu_in, pl.n_out, spec->mu_out, h_pin, h_pout, h_sout);
	/* the last refusals: the second context still holds what it held */
	st = b->relay.d_emap.grow(emap.size(), (w + ": could not allocate the energy map").c_str());
	if (!st) st = b->relay.d_mu.grow(tab.size(), (w + ": could not allocate the layers' tables").c_str());
	if (st) return st;
	PC_HIP_CHECK(hipMemcpy(b->relay.d_emap, emap.data(), emap.size()*sizeof(int), hipMemcpyHostToDevice));
	PC_HIP_CHECK(hipMemcpy(b->relay.d_mu, tab.data(), tab.size()*sizeof(double), hipMemcpyHostToDevice));
	const double *d = b->relay.d_mu;
	pl.emap = b->relay.d_emap;
	pl.Z = d; pl.mu_in = d + (h_mu_in - h_Z); pl.pin = d + (h_pin - h_Z); pl.mu_out = d + (h_mu_out - h_Z); pl.sout = d + (h_sout - h_Z);
	pl.pout = d + (h_pout - h_Z); pl.prod = d + (h_prod - h_Z);
	return pc_relay_drive<pc_rule_layers>(b, who, s, cnt_a, pl);
}

} /* extern "C" */

#endif /* PC_EMIT_HOST_ONLY */
#endif /* PC_EMIT_LAYERS_H */

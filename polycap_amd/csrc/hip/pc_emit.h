/*
 * pc_emit.h -- emit relays: a thin sample between two optics (the confocal geometry).  The exit photons that the last source run of
 * the first context left on the device are flown to a thin sheet, re-emitted there isotropically towards a square target on the
 * second optic's entrance plane, one sampled direction per photon with the target's solid-angle weight, traced through the second
 * optic and left on the second context as a relay leaves them (include/polycap-hip.h, pc_hip_emit_*).  Everything around the
 * injection is the relay's (pc_relay.h): the compaction, the explicit-photon trace, the exact sums, the records.  The injection
 * rule is one function, pc_emit_state, which the count, the inject and the finish kernel all evaluate from the first store's
 * entry: the same operations give the same bits.  A slab emit (pc_hip_slab_*) gives the sample a thickness behind the sheet and
 * attenuates both ways: a second rule, pc_rule_slab over pc_emit_slab_state, beside the thin one, which stays as it is.
 *
 * The first part (the frame, the spec check and the per-entry arithmetic) compiles for the host as well: -DPC_EMIT_HOST_ONLY stops
 * the header after it.
 */
#ifndef PC_EMIT_H
#define PC_EMIT_H

#include <math.h>
#include <stdint.h>

#include "pc_device.h"      /* pc_rng */

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define PC_EMIT_PI 3.141592653589793      /* the double nearest pi, 0x1.921fb54442d18p+1 */

/* the eight doubles of pc_hip_emit, in its order */
enum { PC_EMIT_FOCUS = 0, PC_EMIT_SAMPLE_ANGLE, PC_EMIT_DEPTH, PC_EMIT_DET_ANGLE, PC_EMIT_WD, PC_EMIT_OFF_U, PC_EMIT_OFF_V, PC_EMIT_TARGET_HALF,
       PC_EMIT_N_FIELDS };
/* the sixteen numbers of a frame: n_s (3), h_s, u (3), v (3), n (3), c_B (3) */
enum { PC_EMIT_NS = 0, PC_EMIT_HS = 3, PC_EMIT_U = 4, PC_EMIT_V = 7, PC_EMIT_N = 10, PC_EMIT_CB = 13, PC_EMIT_N_FRAME = 16 };

static inline const char *pc_emit_field_name(int k)
{
	static const char *const names[PC_EMIT_N_FIELDS] = { "focus", "sample_angle", "depth", "det_angle", "wd", "off_u", "off_v", "target_half" };
	return (k >= 0 && k < PC_EMIT_N_FIELDS) ? names[k] : "?";
}

/* The eight doubles of a spec: 0 when they are valid, else 1 + the index of the first field that is not.  Every field finite;
 * focus >= 0; |sample_angle| < pi/2 strictly (the double below is the nearest to pi/2); |det_angle| <= pi; wd > 0; target_half > 0. */
static inline int pc_emit_spec_bad(const double *f)
{
	for (int k = 0; k < PC_EMIT_N_FIELDS; k++)
		if (!(fabs(f[k]) <= 1.7976931348623157e308)) return 1 + k;
	if (!(f[PC_EMIT_FOCUS] >= 0.)) return 1 + PC_EMIT_FOCUS;
	if (!(fabs(f[PC_EMIT_SAMPLE_ANGLE]) < 1.5707963267948966)) return 1 + PC_EMIT_SAMPLE_ANGLE;
	if (!(fabs(f[PC_EMIT_DET_ANGLE]) <= PC_EMIT_PI)) return 1 + PC_EMIT_DET_ANGLE;
	if (!(f[PC_EMIT_WD] > 0.)) return 1 + PC_EMIT_WD;
	if (!(f[PC_EMIT_TARGET_HALF] > 0.)) return 1 + PC_EMIT_TARGET_HALF;
	return 0;
}

/* The frame of a valid spec in the first optic's exit frame: the contract of include/polycap-hip.h, operation by operation.  Host
 * only: the kernels get the sixteen numbers.  "0. - a" where a sign is turned, as in pc_relay_pose_basis: angles (0, 0) give the
 * identity with plus-signed zeros. */
static inline void pc_emit_frame(const double *f, double *fr)
{
	const double sb = sin(f[PC_EMIT_SAMPLE_ANGLE]), cb = cos(f[PC_EMIT_SAMPLE_ANGLE]);
	const double sa = sin(f[PC_EMIT_DET_ANGLE]), ca = cos(f[PC_EMIT_DET_ANGLE]);
	const double focus = f[PC_EMIT_FOCUS], depth = f[PC_EMIT_DEPTH], wd = f[PC_EMIT_WD], ou = f[PC_EMIT_OFF_U], ov = f[PC_EMIT_OFF_V];
	double *ns = fr + PC_EMIT_NS, *u = fr + PC_EMIT_U, *v = fr + PC_EMIT_V, *n = fr + PC_EMIT_N, *c = fr + PC_EMIT_CB;
	ns[0] = sb; ns[1] = 0.; ns[2] = cb;
	fr[PC_EMIT_HS] = (ns[0]*(depth*ns[0]) + ns[1]*(depth*ns[1])) + ns[2]*(focus + depth*ns[2]);
	u[0] = ca; u[1] = 0.; u[2] = 0. - sa;
	v[0] = 0.; v[1] = 1.; v[2] = 0.;
	n[0] = sa; n[1] = 0.; n[2] = ca;
	const double c0[3] = { 0., 0., focus };
	for (int k = 0; k < 3; k++) c[k] = ((c0[k] + wd*n[k]) + ou*u[k]) + ov*v[k];
}

/* What becomes of an exit photon at the sample (the values of PC_RELAY_SKIP .. PC_RELAY_REJECT of pc_relay.h, and two more) */
enum { PC_EMIT_SKIP = 0, PC_EMIT_INJECT = 1, PC_EMIT_REJECT = 2, PC_EMIT_MISS_SAMPLE = 3, PC_EMIT_MISS_DETECTOR = 4 };

/* One exit photon of the first optic -- position (x, y), direction (dx, dy), slot of the first run -- at the sample and on to the
 * target: the contract of include/polycap-hip.h, operation by operation (the library is built with -ffp-contract=off).  fr = the
 * frame, R = target_half.  Returns PC_EMIT_INJECT and out = {x, y, z, dx, dy, dz, ex, ey, ez of the photon in the second optic's
 * frame, t (flight to the sheet), r (flight from the sheet to the target point), g (the target's solid angle over 4 pi)}, or
 * PC_EMIT_MISS_SAMPLE / PC_EMIT_MISS_DETECTOR: out is then not written. */
static inline __host__ __device__ int pc_emit_state(double x, double y, double dx, double dy, uint64_t slot, const double *fr, double R,
	uint64_t seed, double *out)
{
	const double *ns = fr + PC_EMIT_NS, *u = fr + PC_EMIT_U, *v = fr + PC_EMIT_V, *n = fr + PC_EMIT_N, *c = fr + PC_EMIT_CB;
	const double dz = sqrt((1. - dx*dx) - dy*dy);
	const double sd = (ns[0]*dx + ns[1]*dy) + ns[2]*dz;
	const double sp = fr[PC_EMIT_HS] - (ns[0]*x + ns[1]*y);
	if (!(sd > 0.) || !(sp >= 0.)) return PC_EMIT_MISS_SAMPLE;
	const double t = sp / sd;
	const double p0 = x + dx*t, p1 = y + dy*t, p2 = dz*t;
	pc_rng rng;
	pc_rng_init(rng, seed, slot, 0u);
	const double u1 = pc_rng_uniform(rng), u2 = pc_rng_uniform(rng);
	const double a = (2.*u1 - 1.)*R, b = (2.*u2 - 1.)*R;
	const double q0 = c[0] - p0, q1 = c[1] - p1, q2 = c[2] - p2;
	const double f0 = a + ((u[0]*q0 + u[1]*q1) + u[2]*q2);
	const double f1 = b + ((v[0]*q0 + v[1]*q1) + v[2]*q2);
	const double f2 = (n[0]*q0 + n[1]*q1) + n[2]*q2;
	if (!(f2 > 0.)) return PC_EMIT_MISS_DETECTOR;
	const double r2 = (f0*f0 + f1*f1) + f2*f2;
	const double r = sqrt(r2);
	const double d0 = f0/r, d1 = f1/r, d2 = f2/r;
	const double g = ((R*R)*d2) / (PC_EMIT_PI*r2);
	const double h = sqrt(d2*d2 + d0*d0);
	out[0] = a; out[1] = b; out[2] = 0.;
	out[3] = d0; out[4] = d1; out[5] = d2;
	if ((slot & 1ull) == 0ull) {
		out[6] = d2/h; out[7] = 0.; out[8] = 0. - d0/h;
	} else {
		out[6] = 0. - (d0*d1)/h; out[7] = h; out[8] = 0. - (d1*d2)/h;
	}
	out[9] = t; out[10] = r; out[11] = g;
	return PC_EMIT_INJECT;
}

/* weight of a photon behind both optics: w = (wA * g) * wB */
static inline __host__ __device__ double pc_emit_weight(double w_a, double g, double w_b)
{
	return (w_a*g)*w_b;
}

/* path of a photon behind both optics: first optic, flight to the sheet, flight to the target, second optic, added in this order */
static inline __host__ __device__ double pc_emit_dtravel(double d_a, double t, double r, double d_b)
{
	return ((d_a + t) + r) + d_b;
}

/* ---- slab emits: the sample is a slab of thickness T behind the sheet, with attenuation on the way in and on the way out
 * (include/polycap-hip.h, pc_hip_slab_*).  The thin emission above stays as it is; the slab restates its steps around the point of
 * interaction, which lies a sampled path s behind the sheet. */

/* the twenty numbers of a slab's frame: the emit's sixteen, k = (n_s.u, n_s.v, n_s.n), T */
enum { PC_EMIT_SLAB_K = PC_EMIT_N_FRAME, PC_EMIT_SLAB_T = PC_EMIT_N_FRAME + 3, PC_EMIT_SLAB_N_FRAME = PC_EMIT_N_FRAME + 4 };
/* the fourteen numbers of a slab's state: the emit's nine, then */
enum { PC_SLAB_T = 9, PC_SLAB_R, PC_SLAB_GL, PC_SLAB_S, PC_SLAB_SOUT, PC_SLAB_N_STATE };

/* exp(x) for x <= 0, the shape of pc_exp_neg_fast (pc_device.h) in plain multiplies and adds: the same bits on the host, on the
 * device and in numpy, whatever PC_FAST_MATH_DEVICE is.  x < -700: +0, so that no subnormal arises; exp(0) = 1 exactly (k = 0,
 * r = 0); a NaN comes back.  k*ln2_hi is exact (ln2_hi has 32 significant bits, |k| <= 1010); < 1e-14 relative
 * (tests/test_emit_slab_cpu.py). */
static inline __host__ __device__ double pc_emit_exp_neg(double x)
{
	if (x < -700.) return 0.;
	if (x != x) return x;
	const double k = rint(x*1.4426950408889634074);
	double r = x - k*6.93147180369123816490e-01;
	r = r - k*1.90821492927058770002e-10;
	double p = 2.50521083854417187751e-08;                 /* 1/11! */
	p = p*r + 2.75573192239858906526e-07;
	p = p*r + 2.75573192239858906526e-06;
	p = p*r + 2.48015873015873015873e-05;
	p = p*r + 1.98412698412698412698e-04;
	p = p*r + 1.38888888888888888889e-03;
	p = p*r + 8.33333333333333333333e-03;
	p = p*r + 4.16666666666666666667e-02;
	p = p*r + 1.66666666666666666667e-01;
	p = p*r + 0.5;
	p = p*r + 1.0;
	p = p*r + 1.0;
	return ldexp(p, (int)k);
}

/* what a slab's spec adds to the emit's: 0 when it is valid, else 1 thickness (finite, in (0, 1]), 2 mu_in, 3 mu_out (every entry
 * finite and >= 0; *at = the first one that is not) */
static inline int pc_emit_slab_bad(double thickness, int n_in, const double *mu_in, int n_out, const double *mu_out, int *at)
{
	*at = -1;
	if (!(thickness > 0. && thickness <= 1.)) return 1;
	for (int e = 0; e < n_in; e++)
		if (!(mu_in[e] >= 0. && mu_in[e] <= 1.7976931348623157e308)) { *at = e; return 2; }
	for (int e = 0; e < n_out; e++)
		if (!(mu_out[e] >= 0. && mu_out[e] <= 1.7976931348623157e308)) { *at = e; return 3; }
	return 0;
}

/* The frame of a valid slab spec: pc_emit_frame, then the sheet's normal in B's axes and the thickness.  Host only. */
static inline void pc_emit_slab_frame(const double *f, double thickness, double *fr)
{
	pc_emit_frame(f, fr);
	const double *ns = fr + PC_EMIT_NS, *u = fr + PC_EMIT_U, *v = fr + PC_EMIT_V, *n = fr + PC_EMIT_N;
	double *k = fr + PC_EMIT_SLAB_K;
	k[0] = (ns[0]*u[0] + ns[1]*u[1]) + ns[2]*u[2];
	k[1] = (ns[0]*v[0] + ns[1]*v[1]) + ns[2]*v[2];
	k[2] = (ns[0]*n[0] + ns[1]*n[1]) + ns[2]*n[2];
	fr[PC_EMIT_SLAB_T] = thickness;
}

/* pc_emit_state for a slab, with the three uniforms of the entry's stream given: the contract of include/polycap-hip.h, operation by
 * operation.  odd = the slot's lowest bit.  Returns PC_EMIT_INJECT and out = {the emit's nine, t, r, gl (the target's solid angle
 * over 4 pi times the path through the slab), s (the path to the interaction), s_out (the emitted ray's path out of the slab)}, or
 * PC_EMIT_MISS_SAMPLE / PC_EMIT_MISS_DETECTOR: out is then not written.  With u3 < 1, as the stream gives it, s < L and zn <= T: the
 * clamp of tz stands guard over the roundings of L and zn. */
static inline __host__ __device__ int pc_emit_slab_at(double x, double y, double dx, double dy, int odd, const double *fr, double R,
	double u1, double u2, double u3, double *out)
{
	const double *ns = fr + PC_EMIT_NS, *u = fr + PC_EMIT_U, *v = fr + PC_EMIT_V, *n = fr + PC_EMIT_N, *c = fr + PC_EMIT_CB, *k = fr + PC_EMIT_SLAB_K;
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
	const double f2 = (n[0]*q0 + n[1]*q1) + n[2]*q2;
	if (!(f2 > 0.)) return PC_EMIT_MISS_DETECTOR;
	const double r2 = (f0*f0 + f1*f1) + f2*f2;
	const double r = sqrt(r2);
	const double d0 = f0/r, d1 = f1/r, d2 = f2/r;
	const double g = ((R*R)*d2) / (PC_EMIT_PI*r2);
	const double h = sqrt(d2*d2 + d0*d0);
	const double cn = ((k[0]*f0 + k[1]*f1) + k[2]*f2) / r;
	double s_out;
	if (cn > 0.) {
		double tz = T - zn;
		if (tz < 0.) tz = 0.;
		s_out = tz/cn;
	} else if (cn < 0.) {
		s_out = zn/(0. - cn);
	} else {
		return PC_EMIT_MISS_DETECTOR;
	}
	const double gl = g*L;
	if (!(gl < 1.)) return PC_EMIT_MISS_SAMPLE;
	out[0] = a; out[1] = b; out[2] = 0.;
	out[3] = d0; out[4] = d1; out[5] = d2;
	if (!odd) {
		out[6] = d2/h; out[7] = 0.; out[8] = 0. - d0/h;
	} else {
		out[6] = 0. - (d0*d1)/h; out[7] = h; out[8] = 0. - (d1*d2)/h;
	}
	out[PC_SLAB_T] = t; out[PC_SLAB_R] = r; out[PC_SLAB_GL] = gl; out[PC_SLAB_S] = s; out[PC_SLAB_SOUT] = s_out;
	return PC_EMIT_INJECT;
}

/* one exit photon of the first optic at the slab and on to the target: pc_emit_slab_at with draws 0, 1 and 2 of the stream of its
 * slot (draws 0 and 1 are the thin emission's) */
static inline __host__ __device__ int pc_emit_slab_state(double x, double y, double dx, double dy, uint64_t slot, const double *fr, double R,
	uint64_t seed, double *out)
{
	pc_rng rng;
	pc_rng_init(rng, seed, slot, 0u);
	const double u1 = pc_rng_uniform(rng), u2 = pc_rng_uniform(rng), u3 = pc_rng_uniform(rng);
	return pc_emit_slab_at(x, y, dx, dy, (int)(slot & 1ull), fr, R, u1, u2, u3, out);
}

/* weight of a photon behind both optics and the slab between them: w = ((wA * gl) * att) * wB, att = E(0 - (mu_in*s + mu_out*s_out)) */
static inline __host__ __device__ double pc_emit_slab_weight(double w_a, double gl, double mu_in, double s, double mu_out, double s_out, double w_b)
{
	const double a = mu_in*s + mu_out*s_out;
	const double att = pc_emit_exp_neg(0. - a);
	return ((w_a*gl)*att)*w_b;
}

/* path of a photon behind both optics: first optic, flight to the slab, path to the interaction, flight to the target, second optic */
static inline __host__ __device__ double pc_emit_slab_dtravel(double d_a, double t, double s, double r, double d_b)
{
	return (((d_a + t) + s) + r) + d_b;
}

#ifndef PC_EMIT_HOST_ONLY

struct pc_emit_place {
	double fr[PC_EMIT_N_FRAME], R;
	unsigned long long seed;
	long long slot0;            /* first slot of the first context's run */
	const long long *ids;       /* compact store: slot - slot0 of the entry at every position; NULL: the position itself */
	const int *emap;            /* energy e of the second optic takes the first one's weight emap[e] */
};

static_assert(PC_EMIT_SKIP == PC_RELAY_SKIP && PC_EMIT_INJECT == PC_RELAY_INJECT && PC_EMIT_REJECT == PC_RELAY_REJECT && PC_EMIT_MISS_SAMPLE == PC_RELAY_MISS
              && PC_EMIT_MISS_DETECTOR == PC_RELAY_MISS_DETECTOR, "the emission's outcomes are the relay's");

/* The emission as an injection rule of the relay's kernels (pc_relay.h): pc_emit_state on the stream of the entry's slot; the
 * weight (wA[emap[e]] * g) * wB[e], the only place that reads the energy map; the path with the two flights. */
struct pc_rule_emit {
	typedef pc_emit_place place;
	enum { N_STATE = 12, KIND = PC_RELAY_KIND_EMIT };
	static __device__ __forceinline__ int fly(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		const double *e = s.p + i*s.ss;
		const double x = e[(long long)PC_F_EXITX*s.fs], y = e[(long long)PC_F_EXITY*s.fs], dx = e[(long long)PC_F_EDIRX*s.fs], dy = e[(long long)PC_F_EDIRY*s.fs];
		const long long slot = pl.slot0 + (pl.ids ? pl.ids[i] : i);
		return pc_emit_state(x, y, dx, dy, (uint64_t)slot, pl.fr, pl.R, pl.seed, o);
	}
	static __device__ __forceinline__ void state(const pc_spot_src &s, const place &pl, long long ia, double *o) { (void)fly(s, pl, ia, o); }
	/* pc_rule_posed's order: a failed slot is skipped, the selection is asked before the flight */
	static __device__ __forceinline__ int entry(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		if (!pc_relay_src_valid(s, i)) return PC_RELAY_SKIP;
		if (s.mask && !s.mask[i]) return PC_RELAY_REJECT;
		return fly(s, pl, i, o);
	}
	static __device__ __forceinline__ double weight(const pc_spot_src &s, const place &pl, long long ia, int en, const double *o, double w_b)
	{
		return pc_emit_weight(s.w[ia*s.ws + pl.emap[en]], o[11], w_b);
	}
	static __device__ __forceinline__ double dtravel(double d_a, const double *o, double d_b) { return pc_emit_dtravel(d_a, o[9], o[10], d_b); }
};

/* the spec alone: its eight doubles, and a map that is either absent or a list of indices */
static int pc_emit_check_spec(const pc_hip_emit *sp, const std::string &w)
{
	if (!sp) return pc_fail(PC_HIP_ERR_INVALID, w + ": spec must not be NULL");
	const double f[PC_EMIT_N_FIELDS] = { sp->focus, sp->sample_angle, sp->depth, sp->det_angle, sp->wd, sp->off_u, sp->off_v, sp->target_half };
	const int bad = pc_emit_spec_bad(f);
	if (bad)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": " + pc_emit_field_name(bad - 1) + " is not valid (every field finite, focus >= 0, |sample_angle| below pi/2, "
		               "|det_angle| <= pi, wd > 0, target_half > 0)");
	if (!sp->map && sp->n_map != 0) return pc_fail(PC_HIP_ERR_INVALID, w + ": n_map must be 0 without a map");
	if (sp->map && sp->n_map < 1) return pc_fail(PC_HIP_ERR_INVALID, w + ": n_map must be the number of the map's entries, at least 1");
	for (int32_t e = 0; sp->map && e < sp->n_map; e++)
		if (sp->map[e] < 0) return pc_fail(PC_HIP_ERR_INVALID, w + ": map[" + std::to_string(e) + "] is negative");
	return PC_HIP_OK;
}

static void pc_emit_spec_frame(const pc_hip_emit *sp, double *fr)
{
	const double f[PC_EMIT_N_FIELDS] = { sp->focus, sp->sample_angle, sp->depth, sp->det_angle, sp->wd, sp->off_u, sp->off_v, sp->target_half };
	pc_emit_frame(f, fr);
}

/* what the pair of contexts can refuse of a valid spec: the map against the two grids (emap = the map, or the identity), then a
 * first store without the slots of its entries */
static int pc_emit_check_pair(const pc_hip_ctx *a, const pc_hip_ctx *b, const pc_hip_emit *sp, const std::string &w, std::vector<int> &emap)
{
	const int ne = b->host.pm.n_energies;
	emap.resize((size_t)ne);
	if (sp->map) {
		if ((size_t)sp->n_map != b->energies.size())
			return pc_fail(PC_HIP_ERR_INVALID, w + ": n_map is " + std::to_string(sp->n_map) + ", but the second context has " + std::to_string(b->energies.size()) + " energies");
		for (int e = 0; e < ne; e++) {
			if (sp->map[e] < 0 || (size_t)sp->map[e] >= a->energies.size())
				return pc_fail(PC_HIP_ERR_INVALID, w + ": map[" + std::to_string(e) + "] = " + std::to_string(sp->map[e]) + " is no index into the first context's "
				               + std::to_string(a->energies.size()) + " energies");
			emap[(size_t)e] = sp->map[e];
		}
	} else {
		for (int e = 0; e < ne; e++) emap[(size_t)e] = e;
	}
	/* every entry needs the slot it came from: a compact store holds its entries in the order of completion */
	if (a->img.plan.layout == PC_IMG_COMPACT && !a->img.device_view().ids)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context's run was stored compact without its slots, which the emission's random numbers are keyed by: "
		               "run it with option \"slot_ids\" 1, or without option \"compact_images\"");
	return PC_HIP_OK;
}

struct pc_emit_slab_place {
	double fr[PC_EMIT_SLAB_N_FRAME], R;
	unsigned long long seed;
	long long slot0;            /* as pc_emit_place's */
	const long long *ids;
	const int *emap;
	const double *mu_in, *mu_out;      /* the sample's attenuation coefficients at the first and at the second optic's energies */
};

/* The slab as an injection rule: pc_emit_slab_state on the stream of the entry's slot, the emit rule's order of questions; the
 * weight ((wA[emap[e]] * gl) * att) * wB[e], the only place that reads the two tables; the path with the stretch inside the slab. */
struct pc_rule_slab {
	typedef pc_emit_slab_place place;
	enum { N_STATE = PC_SLAB_N_STATE, KIND = PC_RELAY_KIND_EMIT };
	static __device__ __forceinline__ int fly(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		const double *e = s.p + i*s.ss;
		const double x = e[(long long)PC_F_EXITX*s.fs], y = e[(long long)PC_F_EXITY*s.fs], dx = e[(long long)PC_F_EDIRX*s.fs], dy = e[(long long)PC_F_EDIRY*s.fs];
		const long long slot = pl.slot0 + (pl.ids ? pl.ids[i] : i);
		return pc_emit_slab_state(x, y, dx, dy, (uint64_t)slot, pl.fr, pl.R, pl.seed, o);
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
		return pc_emit_slab_weight(s.w[ia*s.ws + ea], o[PC_SLAB_GL], pl.mu_in[ea], o[PC_SLAB_S], pl.mu_out[en], o[PC_SLAB_SOUT], w_b);
	}
	static __device__ __forceinline__ double dtravel(double d_a, const double *o, double d_b)
	{
		return pc_emit_slab_dtravel(d_a, o[PC_SLAB_T], o[PC_SLAB_S], o[PC_SLAB_R], d_b);
	}
};

/* the slab's spec alone: its emit, the thickness, and two tables that are lists of coefficients */
static int pc_emit_slab_check_spec(const pc_hip_slab *sp, const std::string &w)
{
	if (!sp) return pc_fail(PC_HIP_ERR_INVALID, w + ": spec must not be NULL");
	const int st = pc_emit_check_spec(&sp->emit, w);
	if (st) return st;
	if (!sp->mu_in || sp->n_mu_in < 1) return pc_fail(PC_HIP_ERR_INVALID, w + ": n_mu_in must be the number of mu_in's entries, at least 1");
	if (!sp->mu_out || sp->n_mu_out < 1) return pc_fail(PC_HIP_ERR_INVALID, w + ": n_mu_out must be the number of mu_out's entries, at least 1");
	int at = -1;
	switch (pc_emit_slab_bad(sp->thickness, sp->n_mu_in, sp->mu_in, sp->n_mu_out, sp->mu_out, &at)) {
	case 0: return PC_HIP_OK;
	case 1: return pc_fail(PC_HIP_ERR_INVALID, w + ": thickness is not valid (finite, above 0 and at most 1 cm)");
	case 2: return pc_fail(PC_HIP_ERR_INVALID, w + ": mu_in[" + std::to_string(at) + "] is not valid (finite and >= 0)");
	default: return pc_fail(PC_HIP_ERR_INVALID, w + ": mu_out[" + std::to_string(at) + "] is not valid (finite and >= 0)");
	}
}

static void pc_emit_slab_spec_frame(const pc_hip_slab *sp, double *fr)
{
	const pc_hip_emit *e = &sp->emit;
	const double f[PC_EMIT_N_FIELDS] = { e->focus, e->sample_angle, e->depth, e->det_angle, e->wd, e->off_u, e->off_v, e->target_half };
	pc_emit_slab_frame(f, sp->thickness, fr);
}

/* what the pair of contexts can refuse of a valid slab spec: what it refuses of the emit, then a table that is not as long as its
 * context's grid */
static int pc_emit_slab_check_pair(const pc_hip_ctx *a, const pc_hip_ctx *b, const pc_hip_slab *sp, const std::string &w, std::vector<int> &emap)
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

int pc_hip_emit_validate(const pc_hip_emit *spec)
{
	return pc_emit_check_spec(spec, "pc_hip_emit_validate");
}

int pc_hip_emit_frame(const pc_hip_emit *spec, double frame[16])
{
	if (!frame) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_emit_frame: frame must not be NULL");
	const int st = pc_emit_check_spec(spec, "pc_hip_emit_frame");
	if (st) return st;
	pc_emit_spec_frame(spec, frame);
	return PC_HIP_OK;
}

int pc_hip_emit_run(pc_hip_ctx *a, pc_hip_ctx *b, const pc_hip_emit *spec, pc_hip_select *select)
{
	const char *who = "pc_hip_emit_run";
	const std::string w(who);
	int st = pc_relay_check_pair(a, b, w);
	if (!st) st = pc_emit_check_spec(spec, w);
	if (st) return st;
	std::vector<int> emap;
	pc_spot_src s;
	int64_t cnt_a[6];
	st = pc_relay_open(a, b, who, select, spec->map == nullptr, [&] { return pc_emit_check_pair(a, b, spec, w, emap); }, s, cnt_a);
	if (st) return st;
	pc_emit_place pl;
	pc_emit_spec_frame(spec, pl.fr);
	pl.R = spec->target_half;
	pl.seed = spec->seed;
	pl.slot0 = a->run_slot0;
	pl.ids = a->img.device_view().ids;
	/* the last refusal: the second context still holds what it held (a map of an earlier emit relay served that relay's kernels only) */
	st = b->relay.d_emap.grow(emap.size(), (w + ": could not allocate the energy map").c_str());
	if (st) return st;
	PC_HIP_CHECK(hipMemcpy(b->relay.d_emap, emap.data(), emap.size()*sizeof(int), hipMemcpyHostToDevice));
	pl.emap = b->relay.d_emap;
	return pc_relay_drive<pc_rule_emit>(b, who, s, cnt_a, pl);
}

int pc_hip_emit_counts(pc_hip_ctx *ctx, int64_t counts[3])
{
	if (!ctx || !counts) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_emit_counts: ctx and counts must not be NULL");
	if (ctx->last_call != PC_CALL_RELAY || ctx->relay.kind != PC_RELAY_KIND_EMIT)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_emit_counts: the context's last call was not an emit relay into it");
	const int64_t *lost = ctx->relay.lost;
	counts[0] = lost[PC_RELAY_MISS - PC_RELAY_REJECT]; counts[1] = lost[PC_RELAY_MISS_DETECTOR - PC_RELAY_REJECT]; counts[2] = lost[0];
	return PC_HIP_OK;
}

int pc_hip_slab_validate(const pc_hip_slab *spec)
{
	return pc_emit_slab_check_spec(spec, "pc_hip_slab_validate");
}

int pc_hip_slab_frame(const pc_hip_slab *spec, double frame[20])
{
	if (!frame) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_slab_frame: frame must not be NULL");
	const int st = pc_emit_slab_check_spec(spec, "pc_hip_slab_frame");
	if (st) return st;
	pc_emit_slab_spec_frame(spec, frame);
	return PC_HIP_OK;
}

int pc_hip_slab_run(pc_hip_ctx *a, pc_hip_ctx *b, const pc_hip_slab *spec, pc_hip_select *select)
{
	const char *who = "pc_hip_slab_run";
	const std::string w(who);
	int st = pc_relay_check_pair(a, b, w);
	if (!st) st = pc_emit_slab_check_spec(spec, w);
	if (st) return st;
	std::vector<int> emap;
	pc_spot_src s;
	int64_t cnt_a[6];
	st = pc_relay_open(a, b, who, select, spec->emit.map == nullptr, [&] { return pc_emit_slab_check_pair(a, b, spec, w, emap); }, s, cnt_a);
	if (st) return st;
	pc_emit_slab_place pl;
	pc_emit_slab_spec_frame(spec, pl.fr);
	pl.R = spec->emit.target_half;
	pl.seed = spec->emit.seed;
	pl.slot0 = a->run_slot0;
	pl.ids = a->img.device_view().ids;
	/* the last refusals: the second context still holds what it held.  The tables lie in one buffer, mu_in before mu_out */
	const size_t n_in = (size_t)spec->n_mu_in, n_out = (size_t)spec->n_mu_out;
	st = b->relay.d_emap.grow(emap.size(), (w + ": could not allocate the energy map").c_str());
	if (!st) st = b->relay.d_mu.grow(n_in + n_out, (w + ": could not allocate the attenuation tables").c_str());
	if (st) return st;
	PC_HIP_CHECK(hipMemcpy(b->relay.d_emap, emap.data(), emap.size()*sizeof(int), hipMemcpyHostToDevice));
	PC_HIP_CHECK(hipMemcpy(b->relay.d_mu, spec->mu_in, n_in*sizeof(double), hipMemcpyHostToDevice));
	PC_HIP_CHECK(hipMemcpy(b->relay.d_mu + n_in, spec->mu_out, n_out*sizeof(double), hipMemcpyHostToDevice));
	pl.emap = b->relay.d_emap;
	pl.mu_in = b->relay.d_mu;
	pl.mu_out = b->relay.d_mu + n_in;
	return pc_relay_drive<pc_rule_slab>(b, who, s, cnt_a, pl);
}

} /* extern "C" */

#endif /* PC_EMIT_HOST_ONLY */
#endif /* PC_EMIT_H */

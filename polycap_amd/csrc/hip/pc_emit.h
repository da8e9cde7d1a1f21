/*
 * pc_emit.h -- emit relays: a thin sample between two optics (the confocal geometry).  The exit photons that the last source run of
 * the first context left on the device are flown to a thin sheet, re-emitted there isotropically towards a square target on the
 * second optic's entrance plane, one sampled direction per photon with the target's solid-angle weight, traced through the second
 * optic and left on the second context as a relay leaves them (include/polycap-hip.h, pc_hip_emit_*).  Everything around the
 * injection is the relay's (pc_relay.h): the compaction, the explicit-photon trace, the exact sums, the records.  The injection
 * rule is one function, pc_emit_state, which the count, the inject and the finish kernel all evaluate from the first store's
 * entry: the same operations give the same bits.
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

} /* extern "C" */

#endif /* PC_EMIT_HOST_ONLY */
#endif /* PC_EMIT_H */

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

/* pc_emit_state of entry i, which is an exit photon, on the stream of its slot */
static __device__ __forceinline__ int pc_emit_src_state(const pc_spot_src &s, const pc_emit_place &pl, long long i, double *o)
{
	const double *e = s.p + i*s.ss;
	const double x = e[(long long)PC_F_EXITX*s.fs], y = e[(long long)PC_F_EXITY*s.fs], dx = e[(long long)PC_F_EDIRX*s.fs], dy = e[(long long)PC_F_EDIRY*s.fs];
	const long long slot = pl.slot0 + (pl.ids ? pl.ids[i] : i);
	return pc_emit_state(x, y, dx, dy, (uint64_t)slot, pl.fr, pl.R, pl.seed, o);
}

/* What becomes of entry i of the first store: the one predicate of the count and the inject kernels (pc_relay_entry's order: a
 * failed slot is skipped, the selection is asked before the flight) */
static __device__ __forceinline__ int pc_emit_entry(const pc_spot_src &s, const pc_emit_place &pl, long long i, double *o)
{
	if (!pc_relay_src_valid(s, i)) return PC_EMIT_SKIP;
	if (s.mask && !s.mask[i]) return PC_EMIT_REJECT;
	return pc_emit_src_state(s, pl, i, o);
}

/* Stable compaction, step 1 (pc_relay_count_posed_kernel with three ways to be lost): counts[i / 64] = the entries of wave i / 64
 * that are injected; lost[0] += those that miss the sample, lost[1] += those that miss the detector, lost[2] += those the selection
 * rejects, one atomic per wave that has any. */
__global__ void __launch_bounds__(256) pc_emit_count_kernel(pc_spot_src s, pc_emit_place pl, long long n, unsigned long long *counts,
	unsigned long long *lost)
{
	const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
	double o[12];
	const int what = (i < n) ? pc_emit_entry(s, pl, i, o) : PC_EMIT_SKIP;
	const unsigned long long m = __ballot(what == PC_EMIT_INJECT), ms = __ballot(what == PC_EMIT_MISS_SAMPLE);
	const unsigned long long md = __ballot(what == PC_EMIT_MISS_DETECTOR), mr = __ballot(what == PC_EMIT_REJECT);
	if ((threadIdx.x & 63) == 0 && i < n) {
		counts[i >> 6] = (unsigned long long)__popcll(m);
		if (ms) atomicAdd(&lost[0], (unsigned long long)__popcll(ms));
		if (md) atomicAdd(&lost[1], (unsigned long long)__popcll(md));
		if (mr) atomicAdd(&lost[2], (unsigned long long)__popcll(mr));
	}
}

/* Inject (pc_relay_inject_kernel with pc_emit_entry): every entry that is injected becomes one explicit photon of the second
 * context at the position the prefix sums give it; map[position] = its entry. */
__global__ void __launch_bounds__(256) pc_emit_inject_kernel(pc_spot_src s, pc_emit_place pl, const unsigned long long *offs, long long n,
	double *in_start, double *in_dir, double *in_elecv, long long *map)
{
	const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
	double o[12];
	const int keep = (i < n) ? (pc_emit_entry(s, pl, i, o) == PC_EMIT_INJECT) : 0;
	const unsigned long long m = __ballot(keep);
	if (!keep) return;
	const int lane = threadIdx.x & 63;
	const long long pos = (long long)offs[i >> 6] + __popcll(m & ((1ull << lane) - 1ull));
	in_start[3*pos] = o[0]; in_start[3*pos + 1] = o[1]; in_start[3*pos + 2] = o[2];
	in_dir[3*pos] = o[3]; in_dir[3*pos + 1] = o[4]; in_dir[3*pos + 2] = o[5];
	in_elecv[3*pos] = o[6]; in_elecv[3*pos + 1] = o[7]; in_elecv[3*pos + 2] = o[8];
	map[pos] = i;
}

/* Finish (pc_relay_finish_kernel with the emission's state, weight and path): counters of the second stage's outcomes; for every
 * transmitted photon the weights (wA[emap[e]] * g) * wB[e], their exact sums (and the squares' when sumw2 is given) and its image
 * record at the position the prefix sums give it.  Integer sums only. */
__global__ void __launch_bounds__(256) pc_emit_finish_kernel(pc_spot_src s, pc_emit_place pl, pc_relay_stage2 b, const long long *map,
	const unsigned long long *offs, long long n_in, int ne, int acc_lds, double *rec_out, pc_totals *totals, unsigned long long *sumw,
	unsigned long long *sumw2, unsigned long long *relay_cnt)
{
	extern __shared__ unsigned long long l_acc[];
	const int tid = threadIdx.x, lane = tid & 63;
	const int words = sumw2 ? 4 : 2;
	if (acc_lds) {
		for (int k = tid; k < words*ne; k += blockDim.x) l_acc[k] = 0ull;
		__syncthreads();
	}
	unsigned long long *acc = acc_lds ? l_acc : sumw, *acc2 = acc_lds ? l_acc + 2*ne : sumw2;
	const long long recd = PC_N_FIELDS + ne;
	unsigned long long c_in = 0, c_exit = 0, c_abs = 0, c_glass = 0, c_out = 0, c_err = 0, c_irefl = 0;
	for (long long i0 = (long long)blockIdx.x*blockDim.x + (tid - lane); i0 < n_in; i0 += (long long)gridDim.x*blockDim.x) {
		const long long i = i0 + lane;
		const bool act = i < n_in;
		const int rc = act ? b.rc[i] : -99;
		const bool ok = rc == 1;
		const unsigned long long m = __ballot(ok);
		c_in += (unsigned long long)__popcll(__ballot(act));
		c_exit += (unsigned long long)__popcll(m);
		c_abs += (unsigned long long)__popcll(__ballot(rc == 0));
		c_glass += (unsigned long long)__popcll(__ballot(rc == 2));
		c_out += (unsigned long long)__popcll(__ballot(rc == -2));
		c_err += (unsigned long long)__popcll(__ballot(act && rc != 1 && rc != 0 && rc != 2 && rc != -2));
		if (!m) continue;
		long long ia = 0;
		double *r = nullptr;
		double g = 0.;
		unsigned long long f_irefl = 0ull;
		if (ok) {
			ia = map[i];
			const double *e = s.p + ia*s.ss;
			/* the injected state again, from A's entry and its slot's stream: the same bits as the inject kernel wrote, and t, r and
			 * g, which the batch buffer does not hold, come with them */
			double o[12];
			(void)pc_emit_src_state(s, pl, ia, o);
			g = o[11];
			const long long pos = (long long)offs[i >> 6] + __popcll(m & ((1ull << lane) - 1ull));
			r = rec_out + pos*recd;
			const long long n_a = ((const long long *)e)[(long long)PC_F_NREFL*s.fs], n_b = b.irefl[i];
			r[PC_F_SRCX] = e[(long long)PC_F_SRCX*s.fs]; r[PC_F_SRCY] = e[(long long)PC_F_SRCY*s.fs];
			r[PC_F_STARTX] = o[0]; r[PC_F_STARTY] = o[1];
			r[PC_F_SDIRX] = o[3]; r[PC_F_SDIRY] = o[4];
			r[PC_F_SEVX] = o[6]; r[PC_F_SEVY] = o[7];
			r[PC_F_EXITX] = b.exit_coords[3*i]; r[PC_F_EXITY] = b.exit_coords[3*i + 1]; r[PC_F_EXITZ] = b.exit_coords[3*i + 2];
			r[PC_F_EDIRX] = b.exit_dir[3*i]; r[PC_F_EDIRY] = b.exit_dir[3*i + 1];
			/* a photon that met no wall keeps the electric vector it was given (as pc_hip_launch_photons reports it) */
			r[PC_F_EEVX] = n_b ? b.exit_elecv[3*i] : o[6]; r[PC_F_EEVY] = n_b ? b.exit_elecv[3*i + 1] : o[7];
			((long long *)r)[PC_F_NREFL] = n_a + n_b;
			r[PC_F_DTRAVEL] = pc_emit_dtravel(e[(long long)PC_F_DTRAVEL*s.fs], o[9], o[10], b.dtravel[i]);
			f_irefl = (unsigned long long)(n_a + n_b);
		}
		c_irefl += pc_wave_sum_u64(f_irefl);
		for (int en = 0; en < ne; en++) {
			double w = 0.;
			if (ok) {
				w = pc_emit_weight(s.w[ia*s.ws + pl.emap[en]], g, b.w[i*ne + en]);
				r[PC_F_WEIGHTS + en] = w;
			}
			unsigned long long lo = 0ull, hi = 0ull;
			pc_wave_acc128(ok ? pc_relay_fix(w) : 0ull, lo, hi);
			if (lane == 0 && (lo | hi)) pc_atomic_add128(acc + 2*en, lo, hi);
			if (sumw2) {
				lo = hi = 0ull;
				pc_wave_acc128(ok ? pc_fix_sq(w) : 0ull, lo, hi);
				if (lane == 0 && (lo | hi)) pc_atomic_add128(acc2 + 2*en, lo, hi);
			}
		}
	}
	if (acc_lds) {
		__syncthreads();
		for (int en = tid; en < ne; en += blockDim.x) {
			if (l_acc[2*en] | l_acc[2*en + 1]) pc_atomic_add128(sumw + 2*en, l_acc[2*en], l_acc[2*en + 1]);
			if (sumw2 && (l_acc[2*ne + 2*en] | l_acc[2*ne + 2*en + 1])) pc_atomic_add128(sumw2 + 2*en, l_acc[2*ne + 2*en], l_acc[2*ne + 2*en + 1]);
		}
	}
	if (lane == 0 && c_in) {
		/* the second context's totals and the relay's counters, as pc_relay_finish_kernel counts them */
		atomicAdd(&totals->counters[PC_CNT_EXIT], c_exit);
		atomicAdd(&totals->counters[PC_CNT_NOT_ENTERED], c_in - c_exit - c_abs);
		atomicAdd(&totals->counters[PC_CNT_NOT_TRANSMITTED], c_abs);
		atomicAdd(&totals->counters[PC_CNT_IREFL], c_irefl);
		atomicAdd(&totals->counters[PC_CNT_LAUNCHES], c_in);
		atomicAdd(&relay_cnt[0], c_in); atomicAdd(&relay_cnt[1], c_exit); atomicAdd(&relay_cnt[2], c_abs);
		atomicAdd(&relay_cnt[3], c_glass); atomicAdd(&relay_cnt[4], c_out); atomicAdd(&relay_cnt[5], c_err);
	}
}

/* the counts and prefix sums over the first store (pc_emit_count_kernel, pc_relay_scan_kernel); lost = {missed the sample, missed
 * the detector, rejected} (waits for the stream) */
static int pc_emit_offsets(pc_hip_ctx *b, const pc_spot_src &s, const pc_emit_place &pl, long long n, unsigned long long *d_lost,
	long long *total, long long lost[3])
{
	const long long nw = (n + 63)/64;
	PC_HIP_CHECK(hipMemsetAsync(d_lost, 0, 3*sizeof(unsigned long long), b->stream));
	hipLaunchKernelGGL(pc_emit_count_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, b->stream, s, pl, n, (unsigned long long *)b->d_relay_scan, d_lost);
	PC_HIP_CHECK(hipGetLastError());
	hipLaunchKernelGGL(pc_relay_scan_kernel, dim3(1), dim3(1024), 0, b->stream, (unsigned long long *)b->d_relay_scan, nw);
	PC_HIP_CHECK(hipGetLastError());
	unsigned long long t = 0, l[3] = {0, 0, 0};
	PC_HIP_CHECK(hipMemcpyAsync(&t, b->d_relay_scan + nw, sizeof(t), hipMemcpyDeviceToHost, b->stream));
	PC_HIP_CHECK(hipMemcpyAsync(l, d_lost, sizeof(l), hipMemcpyDeviceToHost, b->stream));
	PC_HIP_CHECK(hipStreamSynchronize(b->stream));
	*total = (long long)t;
	for (int k = 0; k < 3; k++) lost[k] = (long long)l[k];
	return PC_HIP_OK;
}

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

/* An emit relay behind its spec check: pc_relay_run's steps with the emission as the injection rule. */
static int pc_emit_run(pc_hip_ctx *a, pc_hip_ctx *b, const pc_hip_emit *sp, pc_hip_select *sel)
{
	const char *who = "pc_hip_emit_run";
	const std::string w(who);
	int st = pc_relay_check(a, b, w, sp->map == nullptr);
	if (st) return st;
	const int ne = b->host.pm.n_energies;
	std::vector<int> emap((size_t)ne);
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
	PC_HIP_CHECK(hipSetDevice(a->device));
	/* the first run is complete (and the apply of the selection behind it), and nothing of the second context is in flight */
	st = pc_hip_transmission_wait(a, nullptr);
	if (!st) st = pc_hip_transmission_wait(b, nullptr);
	if (st) return st;
	int64_t cnt_a[6];
	st = pc_hip_transmission_totals(a, nullptr, cnt_a, nullptr);
	if (st && st != PC_HIP_ERR_ATTEMPTS) return st;         /* failed slots of the first run are skipped and counted below */
	pc_spot_src s;
	st = pc_spot_source(a, 0, s, who);
	if (st) return st;
	if (sel) {
		st = pc_relay_check_select(a, sel, s, w);
		if (st) return st;
		s.mask = sel->m[0].d_mask[0];
	}
	const long long n_a = s.n;
	pc_emit_place pl;
	pc_emit_spec_frame(sp, pl.fr);
	pl.R = sp->target_half;
	pl.seed = sp->seed;
	pl.slot0 = a->run_slot0;
	pl.ids = a->img.device_view().ids;
	st = b->d_emit_map.grow((size_t)ne, (w + ": could not allocate the energy map").c_str());
	if (st) return st;
	pl.emap = b->d_emit_map;

	/* from here on the second context holds the relay, or nothing */
	b->img.reset(); b->leak.events_of_run = 0; b->last_run_plain = 0;
	b->entries_epoch++;
	b->last_call = PC_CALL_NONE;
	b->run_pending = 0; b->run_slots = 0;
	b->run_squares = b->opts.weight_squares;
	b->last_ms = 0.f;
	const size_t nw_a = (size_t)((n_a + 63)/64);
	/* counts and offsets [nw_a + 1], the finish kernel's counters [8] behind the second compaction's, the count kernel's three last */
	st = b->d_relay_scan.grow(nw_a + 1 + 8 + 3, (w + ": could not allocate the compaction counters").c_str());
	if (!st) st = b->d_relay_map.grow((size_t)n_a, (w + ": could not allocate the photon map").c_str());
	if (st) return st;
	PC_HIP_CHECK(hipMemcpy(b->d_emit_map, emap.data(), (size_t)ne*sizeof(int), hipMemcpyHostToDevice));

	long long n_in = 0, n_out = 0, lost[3] = {0, 0, 0};
	st = pc_emit_offsets(b, s, pl, n_a, b->d_relay_scan + nw_a + 1 + 8, &n_in, lost);
	if (st) return st;
	const long long skipped = n_a - n_in - lost[0] - lost[1] - lost[2];
	/* as in a relay: every entry the predicate skips must be a failed slot of A's run */
	if (skipped != cnt_a[4])
		return pc_fail(PC_HIP_ERR_INVALID, w + ": " + std::to_string(skipped) + " entries of the first run have no exit plane or a zero first weight, but "
		               + std::to_string(cnt_a[4]) + " of its slots failed: exit photons with a zero first weight cannot be relayed");
	unsigned long long h_cnt[8] = {0};
	if (n_in > 0) {
		pc_batch bt;
		st = pc_batch_layout(b, n_in, false, bt);
		if (st) return st;
		hipLaunchKernelGGL(pc_emit_inject_kernel, dim3((unsigned)((n_a + 255)/256)), dim3(256), 0, b->stream, s, pl,
		                   (const unsigned long long *)b->d_relay_scan, n_a, bt.d_start, bt.d_dir, bt.d_ev, (long long *)b->d_relay_map);
		PC_HIP_CHECK(hipGetLastError());
		/* stage 2: the explicit-photon trace kernel over the injected photons (many energies: the immediate sweep) */
		st = pc_batch_trace(b, bt, 0);
		if (st) return st;
		b->run_squares = b->opts.weight_squares;      /* the finish kernel keeps the sums an explicit launch does not */
		st = pc_relay_compact_offsets(b, s, bt.d_rc, n_in, &n_out);
		if (st) return st;
		st = b->img.keep_records(n_out, (w + ": could not allocate the image records").c_str());
		if (st) return st;
		unsigned long long *d_cnt = b->d_relay_scan + (size_t)((n_in + 63)/64) + 1;
		PC_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 8*sizeof(unsigned long long), b->stream));
		unsigned long long *sumw = PC_TOTALS_SUMW(b->d_totals.p);
		unsigned long long *sumw2 = b->opts.weight_squares ? PC_TOTALS_SUMW2(b->d_totals.p, ne) : nullptr;
		const size_t lds = (size_t)(sumw2 ? 4 : 2)*(size_t)ne*sizeof(unsigned long long);
		const int acc_lds = (b->relay_acc_lds && lds <= 32768) ? 1 : 0;
		long long grid = (n_in + 255)/256;
		if (grid > 8ll*pc_plan_cus(b->opts, b->n_cu)) grid = 8ll*pc_plan_cus(b->opts, b->n_cu);
		const pc_relay_stage2 s2 = { bt.d_rc, bt.d_w, bt.d_ec, bt.d_ed, bt.d_ee, bt.d_dt, bt.d_ir };
		hipLaunchKernelGGL(pc_emit_finish_kernel, dim3((unsigned)grid), dim3(256), acc_lds ? lds : 0, b->stream, s, pl, s2,
		                   (const long long *)b->d_relay_map, (const unsigned long long *)b->d_relay_scan, n_in, ne, acc_lds, (double *)b->img.d_img,
		                   (pc_totals *)b->d_totals, sumw, sumw2, d_cnt);
		PC_HIP_CHECK(hipGetLastError());
		PC_HIP_CHECK(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, b->stream));
		PC_HIP_CHECK(hipStreamSynchronize(b->stream));
		float ms = 0.f;
		PC_HIP_CHECK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
		b->last_ms = ms;
	} else {
		/* nothing to trace (pc_batch_trace clears the totals otherwise) */
		PC_HIP_CHECK(hipMemsetAsync(b->d_totals, 0, b->totals_bytes, b->stream));
		PC_HIP_CHECK(hipStreamSynchronize(b->stream));
	}
	for (int k = 0; k < 6; k++) b->relay_counters[k] = (int64_t)h_cnt[k];
	b->relay_counters[6] = skipped;
	b->relay_counters[7] = cnt_a[0] + cnt_a[1] + cnt_a[2];
	/* pc_hip_pose_counts goes on telling what it tells: missed = a photon that reached no entrance plane, for either reason */
	b->relay_lost[0] = lost[0] + lost[1]; b->relay_lost[1] = lost[2];
	for (int k = 0; k < 3; k++) b->emit_lost[k] = lost[k];
	b->relay_emit = 1;
	b->run_slots = n_out;
	b->img.valid = 1;
	b->last_call = PC_CALL_RELAY;
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
	int st = pc_relay_check_pair(a, b, "pc_hip_emit_run");
	if (!st) st = pc_emit_check_spec(spec, "pc_hip_emit_run");
	if (st) return st;
	return pc_emit_run(a, b, spec, select);
}

int pc_hip_emit_counts(pc_hip_ctx *ctx, int64_t counts[3])
{
	if (!ctx || !counts) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_emit_counts: ctx and counts must not be NULL");
	if (ctx->last_call != PC_CALL_RELAY || !ctx->relay_emit)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_emit_counts: the context's last call was not an emit relay into it");
	for (int k = 0; k < 3; k++) counts[k] = ctx->emit_lost[k];
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_EMIT_HOST_ONLY */
#endif /* PC_EMIT_H */

/*
 * pc_relay.h -- relays: the exit photons that the last source run of one context left on the device are flown through free space
 * to the entrance plane of a second optic (another context on the same device), traced through it with their weights carried on,
 * and left on the second context as a source run leaves its own: exact weight sums, counters and image records
 * (include/polycap-hip.h, pc_hip_relay_*).  Nothing per-photon crosses PCIe: an inject kernel writes the second context's
 * explicit-launch inputs from the first one's store, the explicit-photon trace kernel runs over them as it does for
 * pc_hip_launch_photons, and a finish kernel multiplies the weights, adds the exact sums and compacts the transmitted photons, in
 * the order of their positions in the first store, into the second context's image records.  A posed relay (pc_hip_pose_*) tilts
 * the second optic and takes a selection of the first context as an aperture between the two: the same kernels with one more
 * predicate -- selected, and not missing the tilted entrance plane -- evaluated alike where the photons are counted and injected.
 *
 * The first part (the per-photon arithmetic) compiles for the host as well: -DPC_RELAY_HOST_ONLY stops the header after it.
 */
#ifndef PC_RELAY_H
#define PC_RELAY_H

#include <math.h>
#include <stdint.h>

#include "pc_exact.h"

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

/* An entry of the first store is an exit photon unless its slot failed: a failed slot has zero weights (slot-ordered store) or
 * every plane zero (compact store), and the exit plane of an optic lies at z > 0. */
static inline __host__ __device__ int pc_relay_entry_valid(double exit_z, double w0)
{
	return (exit_z > 0. && w0 > 0.) ? 1 : 0;
}

/* From an exit record's position (x, y), direction (dx, dy) and electric vector (ex, ey) to the start of the photon in the second
 * optic's frame: out = {x, y, z, dx, dy, dz, ex, ey, ez, t}.  The contract of include/polycap-hip.h, operation by operation (the
 * library is built with -ffp-contract=off). */
static inline __host__ __device__ void pc_relay_fly(double x, double y, double dx, double dy, double ex, double ey,
	double gap, double off_x, double off_y, double *out)
{
	const double dz = sqrt((1. - dx*dx) - dy*dy);
	const double ez = -(ex*dx + ey*dy) / dz;
	const double t = gap / dz;
	out[0] = (x + dx*t) - off_x;
	out[1] = (y + dy*t) - off_y;
	out[2] = 0.;
	out[3] = dx; out[4] = dy; out[5] = dz;
	out[6] = ex; out[7] = ey; out[8] = ez;
	out[9] = t;
}

/* The axes u, v, n of a tilted second optic in the first one's exit frame: the columns of Ry(tilt_x) * Rx(-tilt_y), written out as
 * products of the four sines and cosines (basis = u0 u1 u2 v0 v1 v2 n0 n1 n2).  Host only: the kernels get the nine numbers.
 * "0. - a" where a sign is turned, so that a zero keeps its plus sign and the basis of tilt (0, 0) is the identity bit for bit. */
static inline void pc_relay_pose_basis(double tilt_x, double tilt_y, double *basis)
{
	const double sx = sin(tilt_x), cx = cos(tilt_x), sy = sin(tilt_y), cy = cos(tilt_y);
	basis[0] = cx;            basis[1] = 0.; basis[2] = 0. - sx;
	basis[3] = 0. - sx*sy;    basis[4] = cy; basis[5] = 0. - cx*sy;
	basis[6] = sx*cy;         basis[7] = sy; basis[8] = cx*cy;
}

/* pc_relay_fly for a second optic with the axes `basis` (u, v, n) whose entrance centre is at (off_x, off_y, gap): the contract of
 * include/polycap-hip.h, operation by operation.  Returns 1 and out = {x, y, z, dx, dy, dz, ex, ey, ez, t} in the second optic's
 * frame, or 0 for a photon that misses the entrance plane (it runs parallel to the plane or away from it, or the plane lies
 * behind it): out is then not written. */
static inline __host__ __device__ int pc_relay_fly_posed(double x, double y, double dx, double dy, double ex, double ey,
	double gap, double off_x, double off_y, const double *basis, double *out)
{
	const double *u = basis, *v = basis + 3, *n = basis + 6;
	const double dz = sqrt((1. - dx*dx) - dy*dy);
	const double ez = -(ex*dx + ey*dy) / dz;
	const double nd = (n[0]*dx + n[1]*dy) + n[2]*dz;
	const double np = (n[0]*(off_x - x) + n[1]*(off_y - y)) + n[2]*gap;
	if (!(nd > 0.) || !(np >= 0.)) return 0;
	const double t = np / nd;
	const double r0 = (x + dx*t) - off_x, r1 = (y + dy*t) - off_y, r2 = dz*t - gap;
	out[0] = (u[0]*r0 + u[1]*r1) + u[2]*r2;
	out[1] = (v[0]*r0 + v[1]*r1) + v[2]*r2;
	out[2] = 0.;
	out[3] = (u[0]*dx + u[1]*dy) + u[2]*dz;
	out[4] = (v[0]*dx + v[1]*dy) + v[2]*dz;
	out[5] = nd;
	out[6] = (u[0]*ex + u[1]*ey) + u[2]*ez;
	out[7] = (v[0]*ex + v[1]*ey) + v[2]*ez;
	out[8] = (n[0]*ex + n[1]*ey) + n[2]*ez;
	out[9] = t;
	return 1;
}

/* weight of a photon behind both optics: one fp64 product */
static inline __host__ __device__ double pc_relay_weight(double w_a, double w_b)
{
	return w_a * w_b;
}

/* (uint64)(w * 2^62), truncated: what the weight adds to the exact sum */
static inline __host__ __device__ unsigned long long pc_relay_fix(double w)
{
	return (unsigned long long)(w * 4611686018427387904.0);
}

/* path of a photon behind both optics: first optic, free flight, second optic, added in this order */
static inline __host__ __device__ double pc_relay_dtravel(double d_a, double t, double d_b)
{
	return (d_a + t) + d_b;
}

/* the placement of the second optic: finite, gap >= 0 */
static inline __host__ __device__ int pc_relay_placement_ok(double gap, double off_x, double off_y)
{
	return (gap >= 0. && gap <= 1.7976931348623157e308 && fabs(off_x) <= 1.7976931348623157e308 && fabs(off_y) <= 1.7976931348623157e308) ? 1 : 0;
}

/* the pose of the second optic: a placement and two finite tilts strictly inside (-pi/2, pi/2) (the double below is the nearest to
 * pi/2) */
static inline __host__ __device__ int pc_relay_pose_ok(double gap, double off_x, double off_y, double tilt_x, double tilt_y)
{
	return (pc_relay_placement_ok(gap, off_x, off_y) && fabs(tilt_x) < 1.5707963267948966 && fabs(tilt_y) < 1.5707963267948966) ? 1 : 0;
}

/* A pose without a tilt (either zero) and without a selection is a plain relay: it runs pc_relay_fly, not pc_relay_fly_posed with
 * the identity, whose sums of products may turn the sign of a zero. */
static inline __host__ __device__ int pc_relay_pose_plain(double tilt_x, double tilt_y, int selected)
{
	return (tilt_x == 0. && tilt_y == 0. && !selected) ? 1 : 0;
}

/* efficiency of the train of optics from the exact sum (lo, hi) and the photons started into the first optic: sum / (N 2^62) in
 * long double, 0 when nothing was started */
static inline double pc_relay_efficiency(uint64_t lo, uint64_t hi, int64_t n_started)
{
	if (n_started <= 0) return 0.;
	return (double)(pc_exact_value(lo, hi) / ((long double)n_started * PC_EXACT_2P62));
}

#ifndef PC_RELAY_HOST_ONLY

struct pc_relay_place { double gap, off_x, off_y, basis[9]; };      /* basis: u, v, n of a posed relay (pc_relay_pose_basis) */

static __device__ __forceinline__ int pc_relay_src_valid(const pc_spot_src &s, long long i)
{
	return pc_relay_entry_valid(s.p[i*s.ss + (long long)PC_F_EXITZ*s.fs], s.w[i*s.ws]);
}

/* What becomes of entry i of the first store.  PC_RELAY_SKIP: no exit photon (a failed slot); PC_RELAY_INJECT: it starts into the
 * second optic; the rest are the ways to be lost between the optics, counted at lost[code - PC_RELAY_REJECT]: the selection's mask
 * byte (s.mask, NULL = none) is clear; it misses the entrance plane (of an emit relay: the sample); emit relays only: it misses the
 * detector. */
enum { PC_RELAY_SKIP = 0, PC_RELAY_INJECT = 1, PC_RELAY_REJECT = 2, PC_RELAY_MISS = 3, PC_RELAY_MISS_DETECTOR = 4, PC_RELAY_N_LOST = 3 };
/* what a context holds of a relay (pc_relay_state::kind) */
enum { PC_RELAY_KIND_NONE = 0, PC_RELAY_KIND_RELAY, PC_RELAY_KIND_EMIT };

/* An injection rule: how an exit photon of the first store becomes a photon of the second optic.  The kernels below are written
 * once over a rule, a struct of
 *   place      what the rule needs to know of the geometry, passed to the kernels by value
 *   N_STATE    the numbers of an injected state: {x, y, z, dx, dy, dz, ex, ey, ez} at the second optic, then what the weight and
 *              the path need
 *   KIND       what the second context then holds
 *   entry()    the outcome code of entry i, and its state when it is PC_RELAY_INJECT: the one predicate of the count and the inject
 *              kernels, which recompute it from the entry -- the same operations give the same bits
 *   state()    the state of an entry known to be injected (the finish kernel)
 *   weight()   the weight behind both optics at energy en of the second one
 *   dtravel()  the path behind both optics
 * The plain rule flies every exit photon with pc_relay_fly; the posed rule asks the selection, then pc_relay_fly_posed; the emit
 * rule is pc_emit.h's. */
struct pc_rule_plain {
	typedef pc_relay_place place;
	enum { N_STATE = 10, KIND = PC_RELAY_KIND_RELAY };
	static __device__ __forceinline__ void state(const pc_spot_src &s, const place &pl, long long ia, double *o)
	{
		const double *e = s.p + ia*s.ss;
		pc_relay_fly(e[(long long)PC_F_EXITX*s.fs], e[(long long)PC_F_EXITY*s.fs], e[(long long)PC_F_EDIRX*s.fs], e[(long long)PC_F_EDIRY*s.fs],
		             e[(long long)PC_F_EEVX*s.fs], e[(long long)PC_F_EEVY*s.fs], pl.gap, pl.off_x, pl.off_y, o);
	}
	static __device__ __forceinline__ int entry(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		if (!pc_relay_src_valid(s, i)) return PC_RELAY_SKIP;
		state(s, pl, i, o);
		return PC_RELAY_INJECT;
	}
	static __device__ __forceinline__ double weight(const pc_spot_src &s, const place &, long long ia, int en, const double *, double w_b)
	{
		return pc_relay_weight(s.w[ia*s.ws + en], w_b);
	}
	static __device__ __forceinline__ double dtravel(double d_a, const double *o, double d_b) { return pc_relay_dtravel(d_a, o[9], d_b); }
};

struct pc_rule_posed : pc_rule_plain {      /* the plain rule's weight and path */
	static __device__ __forceinline__ int fly(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		const double *e = s.p + i*s.ss;
		return pc_relay_fly_posed(e[(long long)PC_F_EXITX*s.fs], e[(long long)PC_F_EXITY*s.fs], e[(long long)PC_F_EDIRX*s.fs], e[(long long)PC_F_EDIRY*s.fs],
		                          e[(long long)PC_F_EEVX*s.fs], e[(long long)PC_F_EEVY*s.fs], pl.gap, pl.off_x, pl.off_y, pl.basis, o);
	}
	static __device__ __forceinline__ void state(const pc_spot_src &s, const place &pl, long long ia, double *o) { (void)fly(s, pl, ia, o); }
	static __device__ __forceinline__ int entry(const pc_spot_src &s, const place &pl, long long i, double *o)
	{
		if (!pc_relay_src_valid(s, i)) return PC_RELAY_SKIP;
		if (s.mask && !s.mask[i]) return PC_RELAY_REJECT;
		return fly(s, pl, i, o) ? PC_RELAY_INJECT : PC_RELAY_MISS;
	}
};

/* Stable compaction, step 1: how many of the 64 items of every wave are kept.  Item i is photon i of the second stage, kept when
 * it was transmitted (rc 1).  One thread per item; counts[i / 64] for every wave that holds an item. */
__global__ void __launch_bounds__(256) pc_relay_count_kernel(const int *rc, long long n, unsigned long long *counts)
{
	const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
	const int keep = (i < n) ? (rc[i] == 1) : 0;
	const unsigned long long m = __ballot(keep);
	if ((threadIdx.x & 63) == 0 && i < n) counts[i >> 6] = (unsigned long long)__popcll(m);
}

/* Step 1 over the first store under a rule: an entry is kept when the rule injects it; lost[code - PC_RELAY_REJECT] += the entries
 * of every other outcome but a skip, one atomic per wave that has any. */
template <class RULE>
__global__ void __launch_bounds__(256) pc_relay_count_rule_kernel(pc_spot_src s, typename RULE::place pl, long long n, unsigned long long *counts,
	unsigned long long *lost)
{
	const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
	double o[RULE::N_STATE];
	const int what = (i < n) ? RULE::entry(s, pl, i, o) : PC_RELAY_SKIP;
	const unsigned long long m = __ballot(what == PC_RELAY_INJECT);
	unsigned long long ml[PC_RELAY_N_LOST];
#pragma unroll
	for (int k = 0; k < PC_RELAY_N_LOST; k++) ml[k] = __ballot(what == PC_RELAY_REJECT + k);
	if ((threadIdx.x & 63) == 0 && i < n) {
		counts[i >> 6] = (unsigned long long)__popcll(m);
#pragma unroll
		for (int k = 0; k < PC_RELAY_N_LOST; k++)
			if (ml[k]) atomicAdd(&lost[k], (unsigned long long)__popcll(ml[k]));
	}
}

/* Step 2, one workgroup: counts[0 .. nw) -> their exclusive prefix sums in place, counts[nw] = the total */
__global__ void __launch_bounds__(1024) pc_relay_scan_kernel(unsigned long long *counts, long long nw)
{
	__shared__ unsigned long long wsum[16];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	unsigned long long carry = 0ull;
	for (long long base = 0; base < nw; base += 1024) {
		const long long k = base + tid;
		const unsigned long long v = (k < nw) ? counts[k] : 0ull;
		unsigned long long x = v;
#pragma unroll
		for (int off = 1; off < 64; off <<= 1) {
			const unsigned long long y = __shfl_up(x, off, 64);
			if (lane >= off) x += y;
		}
		if (lane == 63) wsum[wave] = x;
		__syncthreads();
		unsigned long long before = 0ull, all = 0ull;
		for (int j = 0; j < 16; j++) {
			const unsigned long long t = wsum[j];
			if (j < wave) before += t;
			all += t;
		}
		if (k < nw) counts[k] = carry + before + (x - v);
		carry += all;
		__syncthreads();
	}
	if (tid == 0) counts[nw] = carry;
}

/* Inject: every entry of the first store that the rule injects becomes one explicit photon of the second context, at the
 * position the prefix sums give it (the order of the store); map[position] = its entry.  Reads are coalesced when the store is
 * planes and strided by the record when it is records. */
template <class RULE>
__global__ void __launch_bounds__(256) pc_relay_inject_kernel(pc_spot_src s, typename RULE::place pl, const unsigned long long *offs, long long n,
	double *in_start, double *in_dir, double *in_elecv, long long *map)
{
	const long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x;
	double o[RULE::N_STATE];
	const int keep = (i < n) ? (RULE::entry(s, pl, i, o) == PC_RELAY_INJECT) : 0;
	const unsigned long long m = __ballot(keep);
	if (!keep) return;
	const int lane = threadIdx.x & 63;
	const long long pos = (long long)offs[i >> 6] + __popcll(m & ((1ull << lane) - 1ull));
	in_start[3*pos] = o[0]; in_start[3*pos + 1] = o[1]; in_start[3*pos + 2] = o[2];
	in_dir[3*pos] = o[3]; in_dir[3*pos + 1] = o[4]; in_dir[3*pos + 2] = o[5];
	in_elecv[3*pos] = o[6]; in_elecv[3*pos + 1] = o[7]; in_elecv[3*pos + 2] = o[8];
	map[pos] = i;
}

struct pc_relay_stage2 {          /* what the explicit-photon trace left in the batch buffer */
	const int *rc;
	const double *w, *exit_coords, *exit_dir, *exit_elecv, *dtravel;
	const long long *irefl;
};

/* Finish: counters of the second stage's outcomes; for every transmitted photon the rule's weights, their exact sums (and the
 * squares' when sumw2 is given) and its image record at the position the prefix sums give it.  A wave takes 64 consecutive
 * photons at a time; the sums of a workgroup are gathered in LDS (acc_lds) when they fit, else go to the global pairs at once.
 * Integer sums only: the totals depend on the set of photons, not on the launch shape. */
template <class RULE>
__global__ void __launch_bounds__(256) pc_relay_finish_kernel(pc_spot_src s, typename RULE::place pl, pc_relay_stage2 b, const long long *map,
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
		double o[RULE::N_STATE];
		unsigned long long f_irefl = 0ull;
		if (ok) {
			ia = map[i];
			const double *e = s.p + ia*s.ss;
			/* the injected state again, from A's entry: the same operations give the same bits as the inject kernel wrote, and what
			 * the batch buffer does not hold of it (the flight; of an emission its solid angle too) comes with them */
			RULE::state(s, pl, ia, o);
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
			r[PC_F_DTRAVEL] = RULE::dtravel(e[(long long)PC_F_DTRAVEL*s.fs], o, b.dtravel[i]);
			f_irefl = (unsigned long long)(n_a + n_b);
		}
		c_irefl += pc_wave_sum_u64(f_irefl);
		for (int en = 0; en < ne; en++) {
			double w = 0.;
			if (ok) {
				w = RULE::weight(s, pl, ia, en, o, b.w[i*ne + en]);
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
		/* the second context's totals as a source run of the injected photons would count them: exit, not entered (everything
		 * that neither left nor was absorbed), not transmitted, reflections of the exit photons (both optics), launches */
		atomicAdd(&totals->counters[PC_CNT_EXIT], c_exit);
		atomicAdd(&totals->counters[PC_CNT_NOT_ENTERED], c_in - c_exit - c_abs);
		atomicAdd(&totals->counters[PC_CNT_NOT_TRANSMITTED], c_abs);
		atomicAdd(&totals->counters[PC_CNT_IREFL], c_irefl);
		atomicAdd(&totals->counters[PC_CNT_LAUNCHES], c_in);
		atomicAdd(&relay_cnt[0], c_in); atomicAdd(&relay_cnt[1], c_exit); atomicAdd(&relay_cnt[2], c_abs);
		atomicAdd(&relay_cnt[3], c_glass); atomicAdd(&relay_cnt[4], c_out); atomicAdd(&relay_cnt[5], c_err);
	}
}

/* The scratch of a compaction of n items in pc_relay_state::d_scan: the per-wave counts [(n + 63)/64], which become their offsets,
 * the total, the loss counters.  The finish kernel's counters follow the second compaction's. */
#define PC_RELAY_SCAN_WORDS(n) ((size_t)(((n) + 63)/64) + 1 + PC_RELAY_N_LOST)

/* counts + prefix sums of n items on the context's stream.  rc == NULL: the entries of the first store under the rule, lost = how
 * many were lost in each way; else the photons of the second stage that were transmitted.  *total = how many are kept (waits for
 * the stream) */
template <class RULE>
static int pc_relay_offsets(pc_hip_ctx *b, const pc_spot_src &s, const typename RULE::place &pl, const int *rc, long long n, long long *total,
	long long *lost)
{
	const long long nw = (n + 63)/64;
	unsigned long long *d = b->relay.d_scan;
	const dim3 grid((unsigned)((n + 255)/256));
	if (rc) {
		hipLaunchKernelGGL(pc_relay_count_kernel, grid, dim3(256), 0, b->stream, rc, n, d);
	} else {
		PC_HIP_CHECK(hipMemsetAsync(d + nw + 1, 0, PC_RELAY_N_LOST*sizeof(unsigned long long), b->stream));
		hipLaunchKernelGGL(pc_relay_count_rule_kernel<RULE>, grid, dim3(256), 0, b->stream, s, pl, n, d, d + nw + 1);
	}
	PC_HIP_CHECK(hipGetLastError());
	hipLaunchKernelGGL(pc_relay_scan_kernel, dim3(1), dim3(1024), 0, b->stream, d, nw);
	PC_HIP_CHECK(hipGetLastError());
	unsigned long long t[1 + PC_RELAY_N_LOST] = {0};
	PC_HIP_CHECK(hipMemcpyAsync(t, d + nw, (rc ? 1 : 1 + PC_RELAY_N_LOST)*sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
	PC_HIP_CHECK(hipStreamSynchronize(b->stream));
	*total = (long long)t[0];
	for (int k = 0; !rc && k < PC_RELAY_N_LOST; k++) lost[k] = (long long)t[1 + k];
	return PC_HIP_OK;
}

/* the contexts of a relay */
static int pc_relay_check_pair(pc_hip_ctx *a, pc_hip_ctx *b, const std::string &w)
{
	if (!a || !b) return pc_fail(PC_HIP_ERR_INVALID, w + ": the contexts must not be NULL");
	if (a == b) return pc_fail(PC_HIP_ERR_INVALID, w + ": the second optic needs a context of its own");
	return PC_HIP_OK;
}

/* everything else that can refuse a relay, before anything is launched (same_grid false: an emit relay with an energy map, whose
 * contexts have a grid each) */
static int pc_relay_check(pc_hip_ctx *a, pc_hip_ctx *b, const std::string &w, bool same_grid = true)
{
	if (a->device != b->device)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the contexts are on different devices (" + std::to_string(a->device) + " and " + std::to_string(b->device) + ")");
	if (same_grid && (a->energies.size() != b->energies.size() || memcmp(a->energies.data(), b->energies.data(), a->energies.size()*sizeof(double)) != 0))
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the contexts need the same energy grid, bit for bit");
	switch (a->last_call) {
	case PC_CALL_RUN: break;
	case PC_CALL_RUN_LEAK: return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context's last run was a leak_calc run");
	case PC_CALL_EXPLICIT: return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context's last call was an explicit-photon launch, not a source run");
	case PC_CALL_SCAN: return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context's last call was a scan, not a source run");
	case PC_CALL_RELAY: return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context holds the result of a relay, not of a source run");
	default: return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context has made no source run");
	}
	if (!a->img.valid)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the first context's last run kept no exit photons (run it with keep_images)");
	return PC_HIP_OK;
}

/* the selection of a posed relay: the first context's own, applied for kind 0 to the entries s that the relay reads (the rule and
 * the wording of pc_hip_select_gather) */
static int pc_relay_check_select(const pc_hip_ctx *a, const pc_hip_select *sel, const pc_spot_src &s, const std::string &w)
{
	if (sel->group || sel->m.size() != 1 || sel->m[0].ctx != a)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the selection belongs to another owner than the first context (make it on that context, not on a group or on the second context)");
	if (!sel->applied[0])
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the selection was not applied for kind 0 (pc_hip_select_apply)");
	if (sel->m[0].epoch[0] != a->entries_epoch || sel->m[0].n[0] != s.n)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the selection's mask is stale: the entries of kind 0 were replaced after it was applied");
	return PC_HIP_OK;
}

/* The opening of every relay: all that can refuse it, while the second context still holds what it held.  more (optional): what the
 * kind of relay checks of the pair before anything waits.  s = the entries the relay reads, under the selection's mask if there is
 * one; cnt_a = the first run's counters. */
static int pc_relay_open(pc_hip_ctx *a, pc_hip_ctx *b, const char *who, pc_hip_select *sel, bool same_grid, const std::function<int()> &more,
	pc_spot_src &s, int64_t cnt_a[6])
{
	const std::string w(who);
	int st = pc_relay_check(a, b, w, same_grid);
	if (!st && more) st = more();
	if (st) return st;
	PC_HIP_CHECK(hipSetDevice(a->device));
	/* the first run is complete (and the apply of the selection behind it), and nothing of the second context is in flight */
	st = pc_hip_transmission_wait(a, nullptr);
	if (!st) st = pc_hip_transmission_wait(b, nullptr);
	if (st) return st;
	st = pc_hip_transmission_totals(a, nullptr, cnt_a, nullptr);
	if (st && st != PC_HIP_ERR_ATTEMPTS) return st;         /* failed slots of the first run are skipped and counted by the pipeline */
	st = pc_spot_source(a, 0, s, who);
	if (st) return st;
	if (sel) {
		st = pc_relay_check_select(a, sel, s, w);
		if (st) return st;
		s.mask = sel->m[0].d_mask[0];
	}
	return PC_HIP_OK;
}

/* The pipeline of every relay behind its opening: the entries s of the first store into the second context b under RULE at pl. */
template <class RULE>
static int pc_relay_drive(pc_hip_ctx *b, const char *who, const pc_spot_src &s, const int64_t cnt_a[6], const typename RULE::place &pl)
{
	const std::string w(who);
	pc_relay_state &rs = b->relay;
	const long long n_a = s.n;
	const int ne = b->host.pm.n_energies;

	/* from here on the second context holds the relay, or nothing */
	b->img.reset(); b->leak.events_of_run = 0; b->last_run_plain = 0;
	b->entries_epoch++;
	b->last_call = PC_CALL_NONE;
	b->run_pending = 0; b->run_slots = 0;
	b->run_squares = b->opts.weight_squares;
	b->last_ms = 0.f;
	/* the first compaction's scratch holds the second one's, which is over fewer items, and the finish kernel's counters [8] behind it */
	int st = rs.d_scan.grow(PC_RELAY_SCAN_WORDS(n_a) + 8, (w + ": could not allocate the compaction counters").c_str());
	if (!st) st = rs.d_map.grow((size_t)n_a, (w + ": could not allocate the photon map").c_str());
	if (st) return st;

	long long n_in = 0, n_out = 0, lost[PC_RELAY_N_LOST] = {0, 0, 0};
	st = pc_relay_offsets<RULE>(b, s, pl, nullptr, n_a, &n_in, lost);
	if (st) return st;
	const long long skipped = n_a - n_in - lost[0] - lost[1] - lost[2];
	/* The predicate reads the first weight only.  Every entry it skips must be a failed slot of A's run: a grid whose first
	 * energy has no valid constants, or a first weight that underflowed to 0, would otherwise vanish without a word */
	if (skipped != cnt_a[4])
		return pc_fail(PC_HIP_ERR_INVALID, w + ": " + std::to_string(skipped) + " entries of the first run have no exit plane or a zero first weight, but "
		               + std::to_string(cnt_a[4]) + " of its slots failed: exit photons with a zero first weight cannot be relayed");
	unsigned long long h_cnt[8] = {0};
	if (n_in > 0) {
		pc_batch bt;
		st = b->batch.layout((size_t)ne, n_in, false, bt);
		if (st) return st;
		hipLaunchKernelGGL(pc_relay_inject_kernel<RULE>, dim3((unsigned)((n_a + 255)/256)), dim3(256), 0, b->stream, s, pl,
		                   (const unsigned long long *)rs.d_scan, n_a, bt.d_start, bt.d_dir, bt.d_ev, (long long *)rs.d_map);
		PC_HIP_CHECK(hipGetLastError());
		/* stage 2: the explicit-photon trace kernel over the injected photons (many energies: the immediate sweep) */
		st = pc_batch_trace(b, bt, 0);
		if (st) return st;
		b->run_squares = b->opts.weight_squares;      /* the finish kernel keeps the sums an explicit launch does not */
		st = pc_relay_offsets<RULE>(b, s, pl, bt.d_rc, n_in, &n_out, nullptr);
		if (st) return st;
		st = b->img.keep_records(n_out, (w + ": could not allocate the image records").c_str());
		if (st) return st;
		unsigned long long *d_cnt = rs.d_scan + PC_RELAY_SCAN_WORDS(n_in);
		PC_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 8*sizeof(unsigned long long), b->stream));
		unsigned long long *sumw = PC_TOTALS_SUMW(b->d_totals.p);
		unsigned long long *sumw2 = b->opts.weight_squares ? PC_TOTALS_SUMW2(b->d_totals.p, ne) : nullptr;
		const size_t lds = (size_t)(sumw2 ? 4 : 2)*(size_t)ne*sizeof(unsigned long long);
		const int acc_lds = (rs.acc_lds && lds <= 32768) ? 1 : 0;
		long long grid = (n_in + 255)/256;
		if (grid > 8ll*pc_plan_cus(b->opts, b->n_cu)) grid = 8ll*pc_plan_cus(b->opts, b->n_cu);
		const pc_relay_stage2 s2 = { bt.d_rc, bt.d_w, bt.d_ec, bt.d_ed, bt.d_ee, bt.d_dt, bt.d_ir };
		hipLaunchKernelGGL(pc_relay_finish_kernel<RULE>, dim3((unsigned)grid), dim3(256), acc_lds ? lds : 0, b->stream, s, pl, s2,
		                   (const long long *)rs.d_map, (const unsigned long long *)rs.d_scan, n_in, ne, acc_lds, (double *)b->img.d_img,
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
	for (int k = 0; k < 6; k++) rs.counters[k] = (int64_t)h_cnt[k];
	rs.counters[6] = skipped;
	rs.counters[7] = cnt_a[0] + cnt_a[1] + cnt_a[2];
	for (int k = 0; k < PC_RELAY_N_LOST; k++) rs.lost[k] = lost[k];
	rs.kind = RULE::KIND;
	b->run_slots = n_out;
	b->img.valid = 1;
	b->last_call = PC_CALL_RELAY;
	return PC_HIP_OK;
}

/* a relay behind the check of its placement: posed (basis, and sel, optional, between the optics) or plain (basis == NULL) */
static int pc_relay_at(pc_hip_ctx *a, pc_hip_ctx *b, const char *who, double gap, double off_x, double off_y, const double *basis, pc_hip_select *sel)
{
	pc_spot_src s;
	int64_t cnt_a[6];
	const int st = pc_relay_open(a, b, who, sel, true, nullptr, s, cnt_a);
	if (st) return st;
	pc_relay_place pl = { gap, off_x, off_y, { 1., 0., 0., 0., 1., 0., 0., 0., 1. } };
	if (!basis) return pc_relay_drive<pc_rule_plain>(b, who, s, cnt_a, pl);
	memcpy(pl.basis, basis, sizeof(pl.basis));
	return pc_relay_drive<pc_rule_posed>(b, who, s, cnt_a, pl);
}

extern "C" {

int pc_hip_relay_validate(const pc_hip_relay_placement *pl)
{
	if (!pl) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_relay_validate: placement must not be NULL");
	if (!pc_relay_placement_ok(pl->gap, pl->off_x, pl->off_y))
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_relay_validate: gap must be finite and >= 0, off_x and off_y finite");
	return PC_HIP_OK;
}

int pc_hip_relay_run(pc_hip_ctx *a, pc_hip_ctx *b, const pc_hip_relay_placement *placement)
{
	int st = pc_relay_check_pair(a, b, "pc_hip_relay_run");
	if (!st) st = pc_hip_relay_validate(placement);
	if (st) return st;
	return pc_relay_at(a, b, "pc_hip_relay_run", placement->gap, placement->off_x, placement->off_y, nullptr, nullptr);
}

int pc_hip_pose_validate(const pc_hip_pose *pose)
{
	if (!pose) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_pose_validate: pose must not be NULL");
	if (!pc_relay_pose_ok(pose->gap, pose->off_x, pose->off_y, pose->tilt_x, pose->tilt_y))
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_pose_validate: gap must be finite and >= 0, off_x and off_y finite, |tilt_x| and |tilt_y| below pi/2");
	return PC_HIP_OK;
}

int pc_hip_pose_basis(const pc_hip_pose *pose, double basis[9])
{
	if (!basis) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_pose_basis: basis must not be NULL");
	const int st = pc_hip_pose_validate(pose);
	if (st) return st;
	pc_relay_pose_basis(pose->tilt_x, pose->tilt_y, basis);
	return PC_HIP_OK;
}

int pc_hip_pose_run(pc_hip_ctx *a, pc_hip_ctx *b, const pc_hip_pose *pose, pc_hip_select *select)
{
	int st = pc_relay_check_pair(a, b, "pc_hip_pose_run");
	if (!st) st = pc_hip_pose_validate(pose);
	if (st) return st;
	if (pc_relay_pose_plain(pose->tilt_x, pose->tilt_y, select != nullptr))
		return pc_relay_at(a, b, "pc_hip_pose_run", pose->gap, pose->off_x, pose->off_y, nullptr, nullptr);
	double basis[9];
	pc_relay_pose_basis(pose->tilt_x, pose->tilt_y, basis);
	return pc_relay_at(a, b, "pc_hip_pose_run", pose->gap, pose->off_x, pose->off_y, basis, select);
}

int pc_hip_pose_counts(pc_hip_ctx *ctx, int64_t counts[2])
{
	if (!ctx || !counts) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_pose_counts: ctx and counts must not be NULL");
	if (ctx->last_call != PC_CALL_RELAY) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_pose_counts: the context's last call was not a relay into it");
	const int64_t *lost = ctx->relay.lost;      /* missed: a photon that reached no entrance plane, for either reason */
	counts[0] = lost[PC_RELAY_MISS - PC_RELAY_REJECT] + lost[PC_RELAY_MISS_DETECTOR - PC_RELAY_REJECT]; counts[1] = lost[0];
	return PC_HIP_OK;
}

int pc_hip_relay_totals(pc_hip_ctx *ctx, int64_t counters[8], uint64_t *sumw_fixed, uint64_t *sumw2_fixed)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_relay_totals: ctx must not be NULL");
	if (ctx->last_call != PC_CALL_RELAY) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_relay_totals: the context's last call was not a relay into it");
	if (sumw2_fixed && !ctx->run_squares)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_relay_totals: the relay was made without option weight_squares");
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	const size_t ne = (size_t)ctx->host.pm.n_energies;
	if (counters) memcpy(counters, ctx->relay.counters, sizeof(ctx->relay.counters));
	if (sumw_fixed) PC_HIP_CHECK(hipMemcpy(sumw_fixed, PC_TOTALS_SUMW(ctx->d_totals.p), 2*ne*sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (sumw2_fixed) PC_HIP_CHECK(hipMemcpy(sumw2_fixed, PC_TOTALS_SUMW2(ctx->d_totals.p, ne), 2*ne*sizeof(uint64_t), hipMemcpyDeviceToHost));
	return PC_HIP_OK;
}

void pc_hip_relay_efficiencies(size_t n_energies, const uint64_t *sumw_fixed, const uint64_t *sumw2_fixed, const int64_t counters[8],
                               double *efficiencies, double *stderr_)
{
	const int64_t n = counters[7];
	for (size_t e = 0; e < n_energies; e++)
		efficiencies[e] = pc_relay_efficiency(sumw_fixed[2*e], sumw_fixed[2*e + 1], n);
	if (sumw2_fixed && stderr_) {
		const int64_t c6[6] = { n, 0, 0, 0, 0, 0 };      /* N = every photon started into the first optic */
		pc_hip_efficiency_stderr(n_energies, sumw_fixed, sumw2_fixed, c6, stderr_);
	}
}

} /* extern "C" */

#endif /* PC_RELAY_HOST_ONLY */
#endif /* PC_RELAY_H */

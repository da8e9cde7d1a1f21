/*
 * pc_kernels.hip -- gfx950 kernels of the photon trace path + the thin C-ABI of include/polycap-hip.h.
 *
 * Kernel shape (CDNA4, wave64):
 *   - persistent waves: grid = CUs x resident blocks; every wave pulls chunks of exit-photon slots from one
 *     global counter, every lane owns one slot at a time and retries it until a photon is transmitted
 *     (reference driver loop src/polycap-source.c:744-884);
 *   - profile tables (z, cap, zh, cap^2, hexd: 5 x (nmax+1) fp64 = 40 KB for nmax=999) are staged once per
 *     workgroup into LDS; per-energy constants are wave-uniform scalar loads;
 *   - the photon life cycle is scheduled wave-wide by phase (MARCH / EVENT / NEW) with ballots so that the
 *     expensive, rare code (segment quadratic + Fresnel, source sampling) runs with many active lanes;
 *   - totals are accumulated in exact 128-bit fixed point, so they do not depend on scheduling or on how
 *     slots are split over devices.
 * No MFMA: there is no dense contraction in this path.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "polycap-hip.h"
#include "pc_device.h"
#include "pc_leak.h"
#include "pc_problem.h"
#include "pc_moments.h"
#include "pc_plan.h"
#include "pc_images.h"
#include "pc_exact.h"
#include "pc_totals.h"      /* struct pc_totals: the block the kernels add to */

#ifndef PC_MARCH_UNROLL
#define PC_MARCH_UNROLL 4      /* march steps between two ballots of the burst loop.  With march_stop = 8 (a burst goes on while 8 lanes march):
                                * 3: 23.6 ms, 4: 23.4, 5: 23.9, 8: 24.1 (scripts/ab_build.sh, xos1 10 keV, 1e7 slots) */
#endif
#define PC_KE 5                /* energies per lane whose weights are in flight together in a cooperative sweep */
#ifndef PC_CHUNK
#define PC_CHUNK 128           /* slots a wave takes from the global counter at a time */
#endif
#define PC_FIX_SCALE 4611686018427387904.0 /* 2^62 */
#ifndef PC_MIN_WAVES_NE0
#define PC_MIN_WAVES_NE0 2     /* the any-n_energies kernel: 256 VGPRs (it spills 470 B per lane at 128), 8 waves per CU */
#endif
#ifndef PC_MIN_WAVES
#define PC_MIN_WAVES 4         /* __launch_bounds__ waves per SIMD the register allocator must leave room for */
#endif

/* --------------------------------------------------------------------------- kernel arguments */

struct pc_kargs {
	const double *g_z, *g_cap, *g_zh, *g_cap2, *g_hexd, *g_idz, *g_ext, *g_stp, *g_istp;
	const pc_marg4 *g_mg;         /* block-certificate record per start node (pc_problem.h) */
	const pc_drdev *g_dr;         /* leak path: chord deviations of cap per start node */
	unsigned int *work_est;       /* [n_slots] or null: reflections + 1 of every attempt, summed per slot (lane kernels, source runs) */
	const pc_energy_const *ec;
	const double *ec_soa;         /* the sweeps' constants field-major [7][n_energies] (FORM 3: d2, n2_re, n2_im, zi2, rough_c, valid, rough_k2) */
	pc_params pm;
	unsigned long long seed;
	long long slot0, n_slots;
	unsigned int max_attempts;
	int keep_images;
	int event_threshold;
	int march_burst;
	int march_stop;               /* a burst goes on while at least this many lanes march (<= event_threshold, which starts it) */
	pc_totals *totals;
	unsigned long long *work;     /* the launch's work counter (relative slot index handed out next) */
	unsigned long long *sumw;     /* 2*n_energies */
	double *img;                  /* image store of the launch's slots, or NULL: field f of slot j at img[j*img_ss + f*img_fs], weight e at
	                               * img_w[j*img_ws + e].  Records (one per slot): img_ss = 17 + n_energies, img_fs = 1, img_w = img + 17,
	                               * img_ws = img_ss.  Planes (struct _polycap_images): img_ss = 1, img_fs = slots of the run, img_w = weights
	                               * [slot][n_energies], img_ws = n_energies */
	double *img_w;
	long long img_ss, img_fs, img_ws;
	/* Compact image store (option "compact_images", planes only): an exit photon takes the next free position of the run's
	 * planes instead of the position of its slot -- the photons a wave finalises together are written as one coalesced run per
	 * plane -- and the blocks of 2^blk_shift positions are published as they fill (the copy engine fetches behind the kernel).
	 * The order of the photons in the planes is then the order of completion; img_ids, when asked for, says which slot sits
	 * where. */
	unsigned long long *img_cursor;   /* next free position, or NULL: a photon is stored at its slot */
	long long *img_ids;               /* slot of position p (option "slot_ids"), or NULL */
	long long img_id0;                /* what img_ids adds to a launch's slot numbers: the launch's first slot in the run (compact_parts) */
	unsigned int *blk_done;           /* per block: positions written so far */
	unsigned int *blk_flag;           /* per block, host-visible: complete */
	int blk_shift;
	long long img_n;                  /* positions of the launch: its slots */
	double *lane_start;               /* compact store in the kernels that launch in the tracing lane: the 8 start fields of the
	                                   * lane's photon wait here, one 64-byte line per lane, until the photon has left the optic.
	                                   * Per-lane state: two launches in flight (parts on two streams) get disjoint halves */
	int new_threshold;
	int lds_acc;                  /* NE == 0: accumulate weight sums in LDS (2*n_energies u64 of dynamic LDS, 4* with sumw2) */
	int lds_ec;                   /* NE == 0: per-energy constants staged in LDS behind the sums (6*n_energies doubles) */
	int sweep_rough;              /* NE == 0: some energy has a roughness factor (sig_rough != 0): the sweeps evaluate exp(-(c alfa)^2) */
	int pool_event_min;           /* pool kernel: photons waiting for an EVENT phase that make it run before anything else */
	int event_march;              /* pool kernel: march steps taken right after an EVENT phase, while the wave is still full of fresh flights */
	int pool_refill;              /* pool kernel: lanes that must be free before a march burst tops itself up from the pool */
	double *wscratch;             /* NE==0: n_energies * total_threads (per-lane state: two launches in flight get disjoint halves) */
	long long total_threads;
	/* pc_trace_log_kernel (pc_sweep_kernel.h): many-energy source runs whose reflections are logged */
	double *rlog;                 /* [total_threads][log_cap][3]: cos theta, fs, fp (pc_refl_geom3) of the lane's logged reflections (per-lane
	                               * state, as wscratch) */
	int log_cap;                  /* reflections per log */
	int stage_ps;                 /* photons of a wave swept per round: their logs are staged in LDS (stage_ps*log_cap*PCS_ENT doubles per wave) */
	int n_proxy, proxy_e[2];      /* energies whose weights every lane carries itself (pc_sweep_certificate) */
	int flush_min;                /* photons of a wave that wait for a sweep before one is run for them alone */
	int sweep_skip;               /* histogram-only runs: a weight below 2^-64 is not multiplied any further */
	int sweep_fuse;               /* histogram-only runs: the sweep of a finished photon adds its weights to the sums itself (2: whatever its proxies say -- tests) */
	int sweep_exact_every;        /* tests: > 0 = the logs of the photons whose slot is a multiple of this are swept as untame (EXACT loop) */
	double ct_tame;               /* a reflection with cos theta >= ct_tame has 0 <= rtot < 1 - 1e-11 at every energy of the run */
	/* explicit-photon mode */
	const double *in_start, *in_dir, *in_elecv;
	int *out_rc;
	double *out_weights, *out_exit_coords, *out_exit_dir, *out_exit_elecv, *out_dtravel;
	long long *out_irefl;
	/* option "weight_squares": 2*n_energies (lo, hi) sums of the squared weights (include/polycap-hip.h) right behind sumw, or NULL.
	 * The kernels that add to it are instantiated with SQ = true; where the sums are kept in LDS, the squares take another
	 * 2*n_energies u64 behind the weights'.  (Last in the struct: the default kernels' argument offsets stay as they were.) */
	unsigned long long *sumw2;
	/* Scans (MODE PC_MODE_SCAN_*, pc_hip_scan_run) keep no images and launch no explicit photons; they take their arguments in
	 * fields of those (PC_SCAN_* below), so that the struct -- and with it every other kernel -- stays exactly as it was: relative slot
	 * s of the launch is flat index img_id0 + s = point k, slot j (pc_scan_map with img_n slots per point), sampled at point k of
	 * the table in in_start on the stream (seed, slot0 + j, attempt).  Per point, 6 + 4 n_energies u64 of exact totals at sumw +
	 * k (6 + 4 n_energies): the 6 counters, 2 n_energies (lo, hi) weight sums, 2 n_energies of the squares (SQ). */
};

/* the scan's view of pc_kargs (see there) */
#define PC_SCAN_PTS(a) ((const pc_scan_point *)(a).in_start)
#define PC_SCAN_FIRST(a) ((a).img_id0)
#define PC_SCAN_NPP(a) ((a).img_n)

/* Stores of the compact image store: written through to memory (system-coherent), so that a block can be handed to the copy
 * engine while the kernel runs without a write-back of the whole L2 (an agent-scope release on gfx950) per batch of photons */
__device__ __forceinline__ void pc_store_wt(double *p, double v)
{
	__hip_atomic_store((unsigned long long *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void pc_store_wt(long long *p, long long v)
{
	__hip_atomic_store((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* positions [base, base + k) have been written by this wave (k <= 64 < block size): count them into their blocks and
 * publish a block that is complete.  Called by one lane after the wave's stores have been acknowledged. */
__device__ __forceinline__ void pc_blocks_written(const pc_kargs &a, unsigned long long base, int k)
{
	if (!a.blk_done || k <= 0) return;
	const unsigned long long B = 1ull << a.blk_shift;
	unsigned long long b = base >> a.blk_shift;
	unsigned long long left = (unsigned long long)k, at = base;
	while (left) {
		const unsigned long long end = (b + 1ull) << a.blk_shift;
		const unsigned long long c = (end - at < left) ? end - at : left;
		const unsigned long long size = ((unsigned long long)a.img_n - (b << a.blk_shift) < B) ? (unsigned long long)a.img_n - (b << a.blk_shift) : B;
		const unsigned int old = __hip_atomic_fetch_add(&a.blk_done[b], (unsigned int)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if ((unsigned long long)old + c == size)
			__hip_atomic_store(&a.blk_flag[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		left -= c; at += c; b++;
	}
}

/* the 18 fields of one exit photon at position `pos` of the image store: src/polycap-source.c:779-798 (start images, from
 * the sampled photon `s`) and :900-923 (exit images).  WT: stores written through (compact store). */
template <bool WT>
__device__ __forceinline__ void pc_store_field(double *p, double v)
{
	if (WT) pc_store_wt(p, v); else *p = v;
}

template <bool WT>
__device__ __forceinline__ void pc_write_start_fields(const pc_kargs &a, long long pos, double srcx, double srcy, double x, double y,
                                                      double dx, double dy, double evx, double evy)
{
	const long long fs = a.img_fs;
	double *r = a.img + pos*a.img_ss;
	pc_store_field<WT>(r + PC_F_SRCX*fs, srcx); pc_store_field<WT>(r + PC_F_SRCY*fs, srcy);
	pc_store_field<WT>(r + PC_F_STARTX*fs, x); pc_store_field<WT>(r + PC_F_STARTY*fs, y);
	pc_store_field<WT>(r + PC_F_SDIRX*fs, dx); pc_store_field<WT>(r + PC_F_SDIRY*fs, dy);
	pc_store_field<WT>(r + PC_F_SEVX*fs, evx); pc_store_field<WT>(r + PC_F_SEVY*fs, evy);
}

/* start_electric_vector projected on the plane perpendicular to the direction, components rounded (:789-796) */
__device__ __forceinline__ void pc_start_elecv_image(const pc_start &s, double cosalpha0, double &evx, double &evy)
{
	const double c_ae = 1.0 / sqrt(1.0 - cosalpha0*cosalpha0), c_be = -1.*c_ae*cosalpha0;
	double tx = s.ex*c_ae + s.dx*c_be, ty = s.ey*c_ae + s.dy*c_be, tz = s.ez*c_ae + s.dz*c_be;
	pc_norm3(tx, ty, tz);
	evx = round(tx); evy = round(ty);
}

template <bool WT>
__device__ __forceinline__ void pc_write_exit_fields(const pc_kargs &a, const pc_params &Pm, long long pos, double Px, double Py, double Pz,
                                                     double dx, double dy, double dz, double ex, double ey, double ez,
                                                     double cosalpha0, long long irefl, double dtravel)
{
	const long long fs = a.img_fs;
	double *r = a.img + pos*a.img_ss;
	const double t = (Pm.z_end - Pz) / dz;
	const double xx = Px + dx*t, xy = Py + dy*t, xz = Pz + dz*t;
	pc_store_field<WT>(r + PC_F_EXITX*fs, xx); pc_store_field<WT>(r + PC_F_EXITY*fs, xy); pc_store_field<WT>(r + PC_F_EXITZ*fs, xz);
	pc_store_field<WT>(r + PC_F_EDIRX*fs, dx); pc_store_field<WT>(r + PC_F_EDIRY*fs, dy);
	const double c_ae = 1.0 / sqrt(1.0 - cosalpha0*cosalpha0), c_be = -1.*c_ae*cosalpha0;
	double tx = ex*c_ae + dx*c_be, ty = ey*c_ae + dy*c_be, tz = ez*c_ae + dz*c_be;
	pc_norm3(tx, ty, tz);
	pc_store_field<WT>(r + PC_F_EEVX*fs, round(tx)); pc_store_field<WT>(r + PC_F_EEVY*fs, round(ty));
	if (WT) pc_store_wt((long long *)r + PC_F_NREFL*fs, irefl); else ((long long *)r)[PC_F_NREFL*fs] = irefl;
	const double lx = xx - Px, ly = xy - Py, lz = Pm.z_end - Pz;
	pc_store_field<WT>(r + PC_F_DTRAVEL*fs, dtravel + sqrt(lx*lx + ly*ly + lz*lz));
}

/* lane states on top of pc_device.h's: what the NEW phase has to do for the lane */
enum { LS_IDLE = 0, LS_NEED_SLOT = 1, LS_START = 5, LS_MARCH = PC_ST_MARCH, LS_EVENT = PC_ST_EVENT, LS_DONE = PC_ST_DONE };

__device__ __forceinline__ unsigned long long pc_wave_sum_u64(unsigned long long v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1)
		v += __shfl_xor(v, off, PC_WAVE);
	return v;
}

/* exact 128-bit accumulation of the wave's 64-bit fixed-point values into a wave-uniform (hi:lo) through two 32-bit partial sums */
__device__ __forceinline__ void pc_wave_acc128(unsigned long long f, unsigned long long &acc_lo, unsigned long long &acc_hi)
{
	const unsigned long long s_low = pc_wave_sum_u64(f & 0xffffffffull), s_high = pc_wave_sum_u64(f >> 32);
	const unsigned long long lo = s_low + (s_high << 32);
	const unsigned long long hi = (s_high >> 32) + ((lo < s_low) ? 1ull : 0ull);
	const unsigned long long old = acc_lo;
	acc_lo = old + lo;
	acc_hi += hi + ((acc_lo < old) ? 1ull : 0ull);
}

/* exact add of a value below 2^64 to an LDS (lo, hi) pair */
__device__ __forceinline__ void pc_lds_add128(unsigned long long *lohi, unsigned long long f)
{
	const unsigned long long old = atomicAdd(&lohi[0], f);
	if (old + f < old) atomicAdd(&lohi[1], 1ull);
}

/* exact add of a 128-bit (hi:lo) value to a global (lo,hi) pair; carries are derived from each add's old value */
__device__ __forceinline__ void pc_atomic_add128(unsigned long long *lohi, unsigned long long lo, unsigned long long hi)
{
	unsigned long long old = atomicAdd(&lohi[0], lo);
	unsigned long long carry = (old + lo < old) ? 1ull : 0ull;
	if (hi + carry) atomicAdd(&lohi[1], hi + carry);
}

/* the six per-energy constants of the immediate sweeps, field-major in ec_soa / its LDS copy: d2, n2_re, n2_im, zi2, rough_c,
 * valid (FORM 3, pc_device.h); the seventh field of ec_soa, rough_k2, is what pc_trace_log_kernel reads instead of rough_c */
__device__ __forceinline__ pc_energy_const pc_ec_from_soa(const double *ecs, int ne, int e)
{
	pc_energy_const ec;
	ec.n_re = ec.n_im = ec.ninv2_re = ec.ninv2_im = ec.rough_k2 = 0.;
	ec.d2 = ecs[e]; ec.n2_re = ecs[ne + e]; ec.n2_im = ecs[2*ne + e]; ec.zi2 = ecs[3*ne + e];
	ec.rough_c = ecs[4*ne + e]; ec.valid = ecs[5*ne + e];
	return ec;
}

/* one energy of one reflection in the immediate sweeps of the any-n_energies kernel: FORM 3 of pc_device.h.  Same return
 * values as pc_reflect_energy_f. */
__device__ __forceinline__ int pc_reflect_energy_sweep(const pc_energy_const &ec, double c, double c2, double fs, double fp, double &w)
{
	if (ec.valid == 0.) return -1;
	return pc_reflect_energy3(ec, c, c2, fs, fp, w);
}

/* --------------------------------------------------------------------------- the trace kernel
 * NE > 0: up to NE energies, weights in registers (NE = 1, 4, 8 are instantiated; a run with fewer energies than NE
 * pads with copies of the last one whose weights are pinned to 0).  NE == 0: any n_energies, weights in wscratch.
 * MODE: PC_MODE_EXPLICIT: photons come from in_start/in_dir/in_elecv (polycap_photon_launch), no retry, no
 * source; PC_MODE_SRC_CIRCULAR / _GENERIC: photons are sampled from the source (circular / elliptical). */
enum { PC_MODE_SRC_CIRCULAR = 0, PC_MODE_SRC_GENERIC = 1, PC_MODE_EXPLICIT = 2 };
/* scans (pc_hip_scan_run): source runs whose slots belong to points with a source position each, totals kept per point.  The
 * finishing lanes' contributions are gathered into the wave-uniform totals as in a source run; those are tagged with the point they
 * belong to and flushed to it when a phase's lanes belong to another one (slots are handed out in contiguous PC_CHUNK ranges, so a
 * wave holds one or two consecutive points at a time).  Sums that a source run keeps in LDS go to the point's global sums. */
enum { PC_MODE_SCAN_CIRCULAR = 3, PC_MODE_SCAN_GENERIC = 4 };

/* Source runs with more than 8 energies have a kernel of their own: pc_trace_log_kernel (pc_sweep_kernel.h). */
template <int NE, int MODE, int PITCH, bool SQ = false>
__global__ void __launch_bounds__(PC_BLOCK, NE == 0 ? PC_MIN_WAVES_NE0 : PC_MIN_WAVES)
pc_trace_kernel(pc_kargs a)
{
	constexpr bool EXPLICIT = (MODE == PC_MODE_EXPLICIT);
	constexpr bool SCAN = (MODE == PC_MODE_SCAN_CIRCULAR || MODE == PC_MODE_SCAN_GENERIC);
	constexpr bool GENERIC = (MODE == PC_MODE_SRC_GENERIC || MODE == PC_MODE_SCAN_GENERIC);
	static_assert(!(SQ && EXPLICIT), "explicit launches keep no sums");
	/* static LDS with a compile-time pitch: table reads become ds_read with immediate offsets */
	__shared__ double lds[6*PITCH];
	__shared__ pc_marg4 ldsg[PITCH];
	/* NE == 0: per-workgroup exact weight sums, (lo, hi) per energy, when they fit (a.lds_acc); else global atomics */
	extern __shared__ unsigned long long l_acc[];
	const int npts = a.pm.nmax + 1;
	double *l_z = lds, *l_cap = lds + PITCH, *l_zh = lds + 2*PITCH, *l_cap2 = lds + 3*PITCH;
	double *l_hexd = lds + 4*PITCH, *l_idz = lds + 5*PITCH;
	for (int k = threadIdx.x; k < npts; k += blockDim.x) {
		l_z[k] = a.g_z[k];
		l_cap[k] = a.g_cap[k];
		l_zh[k] = a.g_zh[k];
		l_cap2[k] = a.g_cap2[k];
		l_hexd[k] = a.g_hexd[k];
		l_idz[k] = a.g_idz[k];
		ldsg[k] = a.g_mg[k];
	}
	/* u64 of the LDS sums: 2 per energy, 4 with the squared weights (A at [0, 2 ne), B at [2 ne, 4 ne)) */
	if (NE != 1 && a.lds_acc)
		for (int k = threadIdx.x; k < (SQ ? 4 : 2)*a.pm.n_energies; k += blockDim.x) l_acc[k] = 0ull;
	/* NE == 0: the per-energy constants of the cooperative sweeps, staged behind the sums when they fit (a.lds_ec):
	 * every reflection of every photon reads all 6*n_energies of them */
	if (NE == 0 && a.lds_ec) {
		double *l_ec = (double *)(l_acc + (SCAN ? 0 : (SQ ? 4 : 2)*a.pm.n_energies));
		for (int k = threadIdx.x; k < 6*a.pm.n_energies; k += blockDim.x) l_ec[k] = a.ec_soa[k];
	}
	__syncthreads();
	pc_tables T;
	T.z = l_z; T.cap = l_cap; T.zh = l_zh; T.cap2 = l_cap2; T.ext = a.g_ext;
	T.hexd = l_hexd; T.idz = l_idz;
	T.mg = ldsg;
	const long long fs = a.img_fs, ss = a.img_ss, ws = a.img_ws;      /* strides of the image store: records or planes (pc_kargs) */
	const pc_params &Pm = a.pm;
	const int ne = (NE > 0) ? NE : Pm.n_energies;
	const int ner = Pm.n_energies;   /* NE > 1 serves any n_energies <= NE: the surplus weights start at 0 and stay there */
	const int lane = threadIdx.x & (PC_WAVE - 1);
	const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;

	pc_photon<NE> ph;
	/* NE == 0: the lane's n_energies weights are contiguous, so the wave can sweep one photon's weights with 64
	 * lanes over energies (coalesced) in the cooperative loops below */
	ph.wmem = (NE > 0) ? nullptr : (a.wscratch + gtid*(long long)a.pm.n_energies);
	ph.wstride = 1;
	ph.wset = 0;
	ph.rc = 0;

	int state = LS_NEED_SLOT;
	long long slot = -1;          /* relative slot index in [0, n_slots) */
	long long sk = 0;             /* scans: the slot's point */
	unsigned int attempt = 0;
	double cosalpha0 = 0.;         /* start_electric_vector . start_direction: projection constants of src/polycap-source.c:789-796 */
	/* wave-uniform chunk of slots */
	long long chunk_next = 0, chunk_end = 0;

	/* per-lane totals */
	/* 32 bits per lane are plenty (a lane handles n_slots / total_threads slots); the wave sums are 64-bit */
	/* wave-uniform totals (scalar registers): the lanes' contributions are gathered with ballots / wave sums at the end
	 * of every NEW phase, so no per-lane counter stays live across the march and event loops */
	unsigned long long u_exit = 0, u_not_entered = 0, u_not_trans = 0, u_irefl = 0, u_failed = 0, u_launch = 0;
	unsigned long long u_acc_lo = 0, u_acc_hi = 0;   /* NE == 1: exact 128-bit weight sum; NE > 1 and NE == 0 sum in LDS */
	unsigned long long u_sq_lo = 0, u_sq_hi = 0;     /* NE == 1: the same of the squared weights (a.sumw2) */
	long long u_pt = -1;                             /* scans: the point the wave-uniform totals belong to (-1: none yet) */
	/* scans: adds the wave-uniform totals to point u_pt and clears them (a macro: a lambda that captures the totals by reference
	 * would change how the source runs' instantiations are compiled) */
#define PC_SCAN_FLUSH() do { \
		if (u_pt >= 0 && lane == 0) { \
			unsigned long long *t_ = a.sumw + u_pt*PC_SCAN_STRIDE((long long)a.pm.n_energies); \
			if (u_exit) atomicAdd(&t_[PC_CNT_EXIT], u_exit); \
			if (u_not_entered) atomicAdd(&t_[PC_CNT_NOT_ENTERED], u_not_entered); \
			if (u_not_trans) atomicAdd(&t_[PC_CNT_NOT_TRANSMITTED], u_not_trans); \
			if (u_irefl) atomicAdd(&t_[PC_CNT_IREFL], u_irefl); \
			if (u_failed) atomicAdd(&t_[PC_CNT_FAILED], u_failed); \
			if (u_launch) atomicAdd(&t_[PC_CNT_LAUNCHES], u_launch); \
			if (NE == 1 && (u_acc_lo | u_acc_hi)) pc_atomic_add128(t_ + PC_SCAN_SUMS, u_acc_lo, u_acc_hi); \
			if (NE == 1 && SQ && (u_sq_lo | u_sq_hi)) pc_atomic_add128(t_ + PC_SCAN_SQUARES(1), u_sq_lo, u_sq_hi); \
		} \
		u_exit = u_not_entered = u_not_trans = u_irefl = u_failed = u_launch = 0; \
		u_acc_lo = u_acc_hi = u_sq_lo = u_sq_hi = 0; \
	} while (0)

	/* wave-uniform scheduler statistics (diagnostics: lane utilisation per phase type) */
	unsigned long long st_march = 0, st_march_l = 0, st_event = 0, st_event_l = 0, st_new = 0, st_new_l = 0;

	for (;;) {
		const unsigned long long mM = __ballot(state == LS_MARCH);
		const unsigned long long mE = __ballot(state == LS_EVENT);
		const unsigned long long mN = __ballot(state == LS_DONE || state == LS_NEED_SLOT || state == LS_START);
		if ((mM | mE | mN) == 0ull) break;
		const int nM = __popcll(mM), nE = __popcll(mE), nN = __popcll(mN);

		/* NEW is worth a phase once enough lanes wait for it, or when nothing else can run */
		const bool do_new = (nN >= a.new_threshold) || (nM == 0 && nE == 0);
		if (nM > 0 && (nM >= a.event_threshold || (nE == 0 && !do_new))) {
			/* ---------------- MARCH burst: certified node skipping, 6 FMA + 3 LDS reads per node */
			if (Pm.literal) {
				if (state == LS_MARCH)
					state = pc_march_step(T, Pm, ph);
			} else {
				/* lanes fresh from an event or a launch first clear the segment that holds their last interaction point */
				if (state == LS_MARCH && ph.first)
					state = pc_march_step(T, Pm, ph);
				for (int b = 0; b < a.march_burst; b++) {
					unsigned int lanes_in_burst = 0;     /* lanes that take each of these steps (scheduler statistics) */
#pragma unroll
					for (int u = 0; u < PC_MARCH_UNROLL; u++) {
						lanes_in_burst += (unsigned)__popcll(__ballot(state == LS_MARCH));
						if (state == LS_MARCH)
							state = pc_march_step_hot(T, Pm, ph);
					}
					const int cM = __popcll(__ballot(state == LS_MARCH));
					st_march += PC_MARCH_UNROLL; st_march_l += lanes_in_burst;
					if (cM == 0) break;
					if (cM < a.march_stop && (cM != nM || do_new || nE > 0)) break;
				}
			}
		} else if (nE > 0 && !(do_new && nN > nE)) {
			/* ---------------- EVENT: full quadratic of one segment (+ wall hit, Fresnel reflection) */
			st_event += 1; st_event_l += (unsigned)nE;
			if (NE > 0) {
				if (state == LS_EVENT)
					state = pc_event<NE, !EXPLICIT>(T, Pm, a.ec, ph);      /* source runs: pc_fresnel3s (pc_device.h) */
			} else {
				/* many energies: geometry per lane, then the wave sweeps each pending photon's weights with all 64
				 * lanes over energies (coalesced, full lane utilisation whatever the number of pending photons) */
				pc_hit h;
				pc_refl_geom g;
				int pend = 0, res = 0;
				h.nx = h.ny = h.nz = h.cosalfa = 0.; h.ix = 0;
				g.alfa = g.st2 = g.es2 = g.ep2 = g.sd2 = 0.;
				double g_c2 = 0., g_fs = 0., g_fp = 0.;      /* what FORM 3 takes from the geometry (pc_refl_geom3) */
				if (state == LS_EVENT) {
					int st = pc_event_pre(T, Pm, ph, h);
					if (st == PC_ST_REFLECT) {
						if (pc_reflect_geom(ph, h.nx, h.ny, h.nz, g) < 0) { pend = 2; res = -1; }
						else { pend = 1; pc_refl_geom3(g, g_c2, g_fs, g_fp); }
					} else {
						state = st;
					}
				}
				/* the sweep is instantiated once per address space of the per-energy constants (LDS copy or global table): with one
				 * merged pointer the compiler has to use flat loads, which are several times slower than ds_read for LDS data */
				auto sweep = [&](const double *ecs) {
					unsigned long long mP = __ballot(pend == 1);
					const long long wave_gtid0 = gtid - lane;
					if (ne <= 32) {
						/* up to 32 energies: the wave is split into 64/G groups of G = 16 or 32 lanes and sweeps that many
						 * pending photons per pass (lane = photon group x energy); four passes are in flight together so that
						 * the latency of their weight loads (the weights live in HBM/L2) is paid once per batch, not per pass */
						const int G = (ne <= 16) ? 16 : 32, PP = PC_WAVE / G;
						const int sub = lane / G, e = lane - sub*G;
						const unsigned long long gm = (G == 32) ? 0xffffffffull : 0xffffull;
						const pc_energy_const ec = pc_ec_from_soa(ecs, ne, (e < ne) ? e : 0);
						while (mP) {
							int srcv[4], myslot = -1;
	#pragma unroll
							for (int j = 0; j < 4; j++) {
								srcv[j] = -1;
								for (int k = 0; k < PP && mP; k++) {
									const int p = __ffsll((long long)mP) - 1;
									mP &= mP - 1ull;
									if (sub == k) srcv[j] = p;
									if (lane == p) myslot = 4*j + k;
								}
							}
							double wv[4];
	#pragma unroll
							for (int j = 0; j < 4; j++) {
								const int from = (srcv[j] < 0) ? 0 : srcv[j];
								const int wset_p = __shfl(ph.wset, from, PC_WAVE);
								wv[j] = (srcv[j] >= 0 && e < ne && wset_p) ? a.wscratch[(wave_gtid0 + srcv[j])*(long long)ne + e] : 1.0;
							}
							unsigned long long mBv[4], mKv[4];
	#pragma unroll
							for (int j = 0; j < 4; j++) {
								const int from = (srcv[j] < 0) ? 0 : srcv[j];
								const double p_c = __shfl(g.alfa, from, PC_WAVE), p_c2 = __shfl(g_c2, from, PC_WAVE);
								const double p_fs = __shfl(g_fs, from, PC_WAVE), p_fp = __shfl(g_fp, from, PC_WAVE);
								int bad = 0, keep = 0;
								if (srcv[j] >= 0 && e < ne) {
									int r = pc_reflect_energy_sweep(ec, p_c, p_c2, p_fs, p_fp, wv[j]);
									a.wscratch[(wave_gtid0 + srcv[j])*(long long)ne + e] = wv[j];
									bad = (r < 0);
									keep = (r > 0);
								}
								mBv[j] = __ballot(bad);
								mKv[j] = __ballot(keep);
							}
							if (myslot >= 0) {
								const int j = myslot >> 2, k = myslot & 3;
								const unsigned long long m = gm << (k*G);
								const unsigned long long B = (j == 0) ? mBv[0] : ((j == 1) ? mBv[1] : ((j == 2) ? mBv[2] : mBv[3]));
								const unsigned long long K = (j == 0) ? mKv[0] : ((j == 1) ? mKv[1] : ((j == 2) ? mKv[2] : mKv[3]));
								res = (B & m) ? -1 : ((K & m) ? 1 : 0);
							}
						}
					} else
					while (mP) {
						const int p = __ffsll((long long)mP) - 1;
						mP &= mP - 1ull;
						const double p_c = __shfl(g.alfa, p, PC_WAVE), p_c2 = __shfl(g_c2, p, PC_WAVE);
						const double p_fs = __shfl(g_fs, p, PC_WAVE), p_fp = __shfl(g_fp, p, PC_WAVE);
						const int wset_p = __shfl(ph.wset, p, PC_WAVE);
						double *wp = a.wscratch + (wave_gtid0 + p)*(long long)ne;
						int bad = 0, keep = 0;
						for (int e0 = 0; e0 < ne; e0 += PC_WAVE*PC_KE) {
							/* all loads of this sweep are issued before the first Fresnel evaluation */
							double wv[PC_KE];
	#pragma unroll
							for (int k = 0; k < PC_KE; k++) {
								const int e = e0 + k*PC_WAVE + lane;
								wv[k] = (wset_p && e < ne) ? wp[e] : 1.0;
							}
	#pragma unroll
							for (int k = 0; k < PC_KE; k++) {
								const int e = e0 + k*PC_WAVE + lane;
								if (e < ne) {
									const pc_energy_const ec = pc_ec_from_soa(ecs, ne, e);
									int r = pc_reflect_energy_sweep(ec, p_c, p_c2, p_fs, p_fp, wv[k]);
									wp[e] = wv[k];
									bad |= (r < 0);
									keep |= (r > 0);
								}
							}
						}
						const int anybad = __any(bad), anykeep = __any(keep);
						if (lane == p) res = anybad ? -1 : (anykeep ? 1 : 0);
					}
				};
				if (NE == 0 && a.lds_ec) sweep((const double *)(l_acc + (SCAN ? 0 : (SQ ? 4 : 2)*a.pm.n_energies)));
				else sweep(a.ec_soa);
				if (pend) {
					if (pend == 1) { ph.wset = 1; ph.ex = fabs(ph.ex); ph.ey = fabs(ph.ey); ph.ez = fabs(ph.ez); }
					state = pc_event_post(Pm, ph, h, res);
				}
			}
		} else if (nN > 0 && do_new) {
			st_new += 1; st_new_l += (unsigned)nN;
			/* ---------------- NEW: finalise finished photons, hand out slots, sample + entrance tests */
			int coop = 0;                 /* NE == 0: what the cooperative weight sweep has to do for this lane's photon */
			int f_exit = 0, f_not_entered = 0, f_not_trans = 0, f_failed = 0, f_launch = 0;   /* this lane's contributions */
			unsigned int f_irefl = 0;
			unsigned long long f_w = 0, f_w2 = 0;
			long long done_slot = slot;   /* where the finished photon's images go: its slot, or (compact store) the next free position */
			int ok = 0;                   /* the photon left through the exit window: src/polycap-source.c:758-777 */
			if (state == LS_DONE) {
				const int rc = ph.rc;
				if (EXPLICIT) {
					const long long j = slot;
					a.out_rc[j] = rc;
					if (NE > 0) {
#pragma unroll
						for (int e = 0; e < (NE > 0 ? NE : 1); e++)
							if (e < ner) a.out_weights[j*ner + e] = ph.w[NE > 0 ? e : 0];
					} else
						coop = 1;    /* weights are copied by the cooperative sweep below */
					a.out_exit_coords[3*j] = ph.Px; a.out_exit_coords[3*j+1] = ph.Py; a.out_exit_coords[3*j+2] = ph.Pz;
					a.out_exit_dir[3*j] = ph.dx; a.out_exit_dir[3*j+1] = ph.dy; a.out_exit_dir[3*j+2] = ph.dz;
					a.out_exit_elecv[3*j] = ph.ex; a.out_exit_elecv[3*j+1] = ph.ey; a.out_exit_elecv[3*j+2] = ph.ez;
					a.out_irefl[j] = ph.irefl;
					a.out_dtravel[j] = ph.dtravel;
					state = LS_NEED_SLOT;
				} else {
					if (rc == 0) f_not_trans = 1;
					else if (rc == 2) f_not_entered = 1;
					else if (rc == 1) ok = pc_in_exit_window(Pm, ph);
					/* what a leak run of the same slots is ordered by (pc_leak_run::auto_order) */
					if (a.work_est) atomicAdd(&a.work_est[slot], (unsigned int)ph.irefl + 1u);
				}
			}
			/* compact store: the exit photons of this phase take the next positions of the planes, one coalesced run per plane */
			const bool compact = !EXPLICIT && a.keep_images && a.img_cursor != nullptr;
			unsigned long long c_base = 0ull;
			int c_k = 0;
			if (compact) {
				const unsigned long long mOK = __ballot(ok);
				if (mOK) {
					c_k = __popcll(mOK);
					if (lane == 0) c_base = atomicAdd(a.img_cursor, (unsigned long long)c_k);
					c_base = __shfl(c_base, 0, PC_WAVE);
					if (ok) done_slot = (long long)(c_base + (unsigned long long)__popcll(mOK & ((1ull << lane) - 1ull)));
				}
			}
			if (!EXPLICIT && state == LS_DONE) {
				if (ok) {
					f_exit = 1;
					f_irefl = (unsigned int)ph.irefl;
					if (NE == 1) {
						double w = ph.w[0];
						f_w = (unsigned long long)(w * PC_FIX_SCALE);
						if (SQ) f_w2 = pc_fix_sq(w);
						if (a.keep_images) { if (compact) pc_store_wt(a.img_w + done_slot*ws, w); else a.img_w[done_slot*ws] = w; }
					} else if (NE > 1) {
						/* a few energies: exact sums in LDS (2 x u64 per energy), flushed once per workgroup (scans: per point, below) */
#pragma unroll
						for (int e = 0; e < (NE > 0 ? NE : 1); e++) {
							if (!SCAN && e < ner) {
								double w = ph.w[NE > 0 ? e : 0];
								unsigned long long f = (unsigned long long)(w * PC_FIX_SCALE);
								unsigned long long old = atomicAdd(&l_acc[2*e], f);
								if (old + f < old) atomicAdd(&l_acc[2*e + 1], 1ull);
								if (SQ) pc_lds_add128(&l_acc[2*ner + 2*e], pc_fix_sq(w));
								if (a.keep_images) { if (compact) pc_store_wt(a.img_w + done_slot*ws + e, w); else a.img_w[done_slot*ws + e] = w; }
							}
						}
					} else {
						coop = 1;    /* sums and image weights are handled by the cooperative sweep below */
					}
					if (a.keep_images) {
						/* src/polycap-source.c:900-923 */
						if (compact) {
							/* the start images waited in the lane's own line (written at the launch, below) */
							const double *ls = a.lane_start + gtid*8;
							pc_write_start_fields<true>(a, done_slot, ls[0], ls[1], ls[2], ls[3], ls[4], ls[5], ls[6], ls[7]);
							pc_write_exit_fields<true>(a, Pm, done_slot, ph.Px, ph.Py, ph.Pz, ph.dx, ph.dy, ph.dz, ph.ex, ph.ey, ph.ez, cosalpha0, (long long)ph.irefl, ph.dtravel);
							if (a.img_ids) pc_store_wt(a.img_ids + done_slot, a.img_id0 + slot);
						} else {
							pc_write_exit_fields<false>(a, Pm, done_slot, ph.Px, ph.Py, ph.Pz, ph.dx, ph.dy, ph.dz, ph.ex, ph.ey, ph.ez, cosalpha0, (long long)ph.irefl, ph.dtravel);
						}
					}
					state = LS_NEED_SLOT;
				} else {
					attempt++;
					if (attempt >= a.max_attempts) {
						f_failed = 1;
						if (a.keep_images && !compact) {
							if (NE > 0) for (int e = 0; e < ner; e++) a.img_w[slot*ws + e] = 0.;
							else coop = 2;   /* zero weights */
						}
						state = LS_NEED_SLOT;
					} else {
						state = LS_START;
					}
				}
			}
			if (NE == 0) {
				/* cooperative sweep over the weights of the photons finalised above: 64 lanes over energies */
				unsigned long long mC = __ballot(coop != 0);
				const long long wave_gtid0 = gtid - lane;
				while (mC) {
					const int p = __ffsll((long long)mC) - 1;
					mC &= mC - 1ull;
					const int what = __shfl(coop, p, PC_WAVE);
					const int wset_p = __shfl(ph.wset, p, PC_WAVE);
					const long long slot_p = __shfl(done_slot, p, PC_WAVE);
					long long k_p = 0;        /* scans: the photon's point */
					if constexpr (SCAN) k_p = __shfl(sk, p, PC_WAVE);
					const double *wp = a.wscratch + (wave_gtid0 + p)*(long long)ne;
					for (int e = lane; e < ne; e += PC_WAVE) {
						double w = (what == 2) ? 0. : (wset_p ? wp[e] : 1.0);
						if (EXPLICIT) {
							a.out_weights[slot_p*ne + e] = w;
						} else {
							if (what == 1) {
								unsigned long long f = (unsigned long long)(w * PC_FIX_SCALE);
								if constexpr (SCAN) {
									unsigned long long *t = a.sumw + k_p*PC_SCAN_STRIDE((long long)a.pm.n_energies) + PC_SCAN_SUMS;
									pc_atomic_add128(t + 2*e, f, 0ull);
									if (SQ) pc_atomic_add128(t + 2*ne + 2*e, pc_fix_sq(w), 0ull);
								} else if (a.lds_acc) {
									unsigned long long old = atomicAdd(&l_acc[2*e], f);
									if (old + f < old) atomicAdd(&l_acc[2*e + 1], 1ull);
									if (SQ) pc_lds_add128(&l_acc[2*ne + 2*e], pc_fix_sq(w));
								} else {
									pc_atomic_add128(a.sumw + 2*e, f, 0ull);
									if (SQ) pc_atomic_add128(a.sumw2 + 2*e, pc_fix_sq(w), 0ull);
								}
							}
							if (a.keep_images) { if (compact) pc_store_wt(a.img_w + slot_p*ws + e, w); else a.img_w[slot_p*ws + e] = w; }
						}
					}
				}
			}
			if constexpr (SCAN) {
				/* the finished photons' contributions, point by point over the lanes that share one (sk is still the finished slot's) */
				const bool has = (f_exit | f_not_entered | f_not_trans | f_failed) != 0;
				unsigned long long pend = __ballot(has);
				while (pend) {
					const long long k = __shfl(sk, __ffsll((long long)pend) - 1, PC_WAVE);
					const bool mine = has && sk == k;
					pend &= ~__ballot(mine);
					if (k != u_pt) { PC_SCAN_FLUSH(); u_pt = k; }
					u_not_trans += (unsigned long long)__popcll(__ballot(mine && f_not_trans));
					u_not_entered += (unsigned long long)__popcll(__ballot(mine && f_not_entered));
					u_failed += (unsigned long long)__popcll(__ballot(mine && f_failed));
					const bool mx = mine && f_exit;
					const unsigned long long mX = __ballot(mx);
					if (mX) {
						u_exit += (unsigned long long)__popcll(mX);
						u_irefl += pc_wave_sum_u64(mx ? (unsigned long long)f_irefl : 0ull);
						if (NE == 1) {
							pc_wave_acc128(mx ? f_w : 0ull, u_acc_lo, u_acc_hi);
							if (SQ) pc_wave_acc128(mx ? f_w2 : 0ull, u_sq_lo, u_sq_hi);
						} else if (NE > 1) {
							/* a few energies: the group's exact sums go to the point at once (the weights are the lanes' until the launch below) */
							unsigned long long *t = a.sumw + k*PC_SCAN_STRIDE((long long)a.pm.n_energies) + PC_SCAN_SUMS;
#pragma unroll
							for (int e = 0; e < (NE > 0 ? NE : 1); e++) {
								if (e < ner) {
									const double w = ph.w[NE > 0 ? e : 0];
									unsigned long long lo = 0, hi = 0;
									pc_wave_acc128(mx ? (unsigned long long)(w * PC_FIX_SCALE) : 0ull, lo, hi);
									if (lane == 0 && (lo | hi)) pc_atomic_add128(t + 2*e, lo, hi);
									if (SQ) {
										unsigned long long lo2 = 0, hi2 = 0;
										pc_wave_acc128(mx ? pc_fix_sq(w) : 0ull, lo2, hi2);
										if (lane == 0 && (lo2 | hi2)) pc_atomic_add128(t + 2*ner + 2*e, lo2, hi2);
									}
								}
							}
						}
					}
				}
			}
			/* compact store: the positions [c_base, c_base + c_k) are complete (fields above, weights by the lanes or the cooperative
			 * sweep): count them into their blocks once the stores have reached memory, so that the fetch can copy a finished block
			 * while the kernel runs (the launching-wave kernel does the same, pc_producer_kernel.h) */
			if (compact && c_k > 0 && a.blk_done) {
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				if (lane == 0) pc_blocks_written(a, c_base, c_k);
			}
			/* hand out slots: wave-uniform chunk, refilled from the global counter by one lane */
			{
				const unsigned long long need = __ballot(state == LS_NEED_SLOT);
				if (need) {
					const int k = __popcll(need);
					if (chunk_end - chunk_next < k) {
						/* top up: take what is left of the old chunk first, then a fresh chunk */
						long long have = chunk_end - chunk_next;
						long long base_new = 0;
						if (lane == 0) base_new = (long long)atomicAdd(a.work, (unsigned long long)PC_CHUNK);
						base_new = __shfl(base_new, 0, PC_WAVE);
						const int rank = __popcll(need & ((1ull << lane) - 1ull));
						if (state == LS_NEED_SLOT) {
							slot = (rank < have) ? (chunk_next + rank) : (base_new + (rank - have));
						}
						chunk_next = base_new + (k - have);
						chunk_end = base_new + PC_CHUNK;
					} else {
						const int rank = __popcll(need & ((1ull << lane) - 1ull));
						if (state == LS_NEED_SLOT) slot = chunk_next + rank;
						chunk_next += k;
					}
					if (state == LS_NEED_SLOT) {
						if (slot >= a.n_slots) { state = LS_IDLE; }
						else {
							attempt = 0; state = LS_START;
							if constexpr (SCAN) {
								long long j;
								pc_scan_map(PC_SCAN_FIRST(a) + slot, PC_SCAN_NPP(a), sk, j);
							}
						}
					}
				}
			}
			/* start an attempt */
			if (state == LS_START) {
				f_launch = 1;
				if (EXPLICIT) {
					const long long j = slot;
					state = pc_launch_init(T, Pm, ph, a.in_start[3*j], a.in_start[3*j+1], a.in_start[3*j+2],
					                       a.in_dir[3*j], a.in_dir[3*j+1], a.in_dir[3*j+2],
					                       a.in_elecv[3*j], a.in_elecv[3*j+1], a.in_elecv[3*j+2]);
					if (NE > 1) {
#pragma unroll
						for (int e = 0; e < (NE > 0 ? NE : 1); e++) if (e >= ner) ph.w[NE > 0 ? e : 0] = 0.;
					}
				} else {
					pc_start s;
					if constexpr (SCAN) {
						const pc_scan_point pt = PC_SCAN_PTS(a)[sk];       /* the point's source position, once per attempt */
						const long long j = PC_SCAN_FIRST(a) + slot - sk*PC_SCAN_NPP(a);   /* slot j of point sk (pc_scan_map) */
						pc_sample_photon_at<GENERIC>(Pm, pt.d_source, pt.src_shiftx, pt.src_shifty, a.seed, (unsigned long long)(a.slot0 + j), attempt, s);
					} else
						pc_sample_photon<MODE == PC_MODE_SRC_GENERIC>(Pm, a.seed, (unsigned long long)(a.slot0 + slot), attempt, s);
					state = pc_launch_init(T, Pm, ph, s.x, s.y, s.z, s.dx, s.dy, s.dz, s.ex, s.ey, s.ez);
					if (NE > 1) {
#pragma unroll
						for (int e = 0; e < (NE > 0 ? NE : 1); e++) if (e >= ner) ph.w[NE > 0 ? e : 0] = 0.;
					}
					if (state == LS_MARCH) {
						/* src/polycap-source.c:779-798: start images of the attempt that is now inside a capillary;
						 * the slot belongs to this lane, so a later (transmitted) attempt simply overwrites them.  The start
						 * direction recorded is the photon's after the launch: polycap_photon_launch normalises it once more in
						 * place (src/polycap-photon.c:492) before :785-786 read it */
						cosalpha0 = s.ex*s.dx + s.ey*s.dy + s.ez*s.dz;
						if (a.keep_images) {
							double evx, evy;
							pc_start_elecv_image(s, cosalpha0, evx, evy);
							if (a.img_cursor) {
								/* compact store: the position is known when the photon leaves; until then its line */
								double *ls = a.lane_start + gtid*8;
								ls[0] = s.srcx; ls[1] = s.srcy; ls[2] = s.x; ls[3] = s.y; ls[4] = ph.dx; ls[5] = ph.dy; ls[6] = evx; ls[7] = evy;
							} else {
								pc_write_start_fields<false>(a, slot, s.srcx, s.srcy, s.x, s.y, ph.dx, ph.dy, evx, evy);
							}
						}
					}
				}
			}
			/* gather this phase's contributions into the wave-uniform totals */
			if constexpr (SCAN) {
				/* the finished photons' went to their points above; the launches belong to the points of the lanes' (new) slots */
				unsigned long long pend = __ballot(f_launch);
				while (pend) {
					const long long k = __shfl(sk, __ffsll((long long)pend) - 1, PC_WAVE);
					const unsigned long long grp = __ballot(f_launch && sk == k);
					pend &= ~grp;
					if (k != u_pt) { PC_SCAN_FLUSH(); u_pt = k; }
					u_launch += (unsigned long long)__popcll(grp);
				}
				continue;
			}
			u_not_trans += (unsigned long long)__popcll(__ballot(f_not_trans));
			u_not_entered += (unsigned long long)__popcll(__ballot(f_not_entered));
			u_failed += (unsigned long long)__popcll(__ballot(f_failed));
			u_launch += (unsigned long long)__popcll(__ballot(f_launch));
			const unsigned long long mX = __ballot(f_exit);
			if (mX) {
				u_exit += (unsigned long long)__popcll(mX);
				u_irefl += pc_wave_sum_u64((unsigned long long)f_irefl);
				if (NE == 1) {
					/* exact 128-bit accumulation of the wave's 64-bit fixed-point weights through two 32-bit partial sums */
					const unsigned long long s_low = pc_wave_sum_u64(f_w & 0xffffffffull), s_high = pc_wave_sum_u64(f_w >> 32);
					const unsigned long long lo = s_low + (s_high << 32);
					const unsigned long long hi = (s_high >> 32) + ((lo < s_low) ? 1ull : 0ull);
					const unsigned long long old = u_acc_lo;
					u_acc_lo = old + lo;
					u_acc_hi += hi + ((u_acc_lo < old) ? 1ull : 0ull);
					if (SQ) pc_wave_acc128(f_w2, u_sq_lo, u_sq_hi);
				}
			}
		}
	}

	if constexpr (SCAN) {
		PC_SCAN_FLUSH();
		if (lane == 0) {
			atomicAdd(&a.totals->phase[PC_PH_MARCH], st_march); atomicAdd(&a.totals->phase[PC_PH_MARCH_LANES], st_march_l);
			atomicAdd(&a.totals->phase[PC_PH_EVENT], st_event); atomicAdd(&a.totals->phase[PC_PH_EVENT_LANES], st_event_l);
			atomicAdd(&a.totals->phase[PC_PH_NEW], st_new); atomicAdd(&a.totals->phase[PC_PH_NEW_LANES], st_new_l);
		}
		return;
	}
#undef PC_SCAN_FLUSH
	if (NE != 1 && !EXPLICIT && a.lds_acc) {
		__syncthreads();          /* every wave of the workgroup has finished its photons */
		for (int e = threadIdx.x; e < a.pm.n_energies; e += blockDim.x)
			if (l_acc[2*e] | l_acc[2*e + 1]) pc_atomic_add128(a.sumw + 2*e, l_acc[2*e], l_acc[2*e + 1]);
		if (SQ) {
			const unsigned long long *l_sq = l_acc + 2*a.pm.n_energies;
			for (int e = threadIdx.x; e < a.pm.n_energies; e += blockDim.x)
				if (l_sq[2*e] | l_sq[2*e + 1]) pc_atomic_add128(a.sumw2 + 2*e, l_sq[2*e], l_sq[2*e + 1]);
		}
	}
	if (!EXPLICIT) {
		/* one set of atomics per wave */
		const unsigned long long v0 = u_exit, v1 = u_not_entered, v2 = u_not_trans, v3 = u_irefl, v4 = u_failed, v5 = u_launch;
		if (lane == 0) {
			atomicAdd(&a.totals->counters[PC_CNT_EXIT], v0);
			atomicAdd(&a.totals->counters[PC_CNT_NOT_ENTERED], v1);
			atomicAdd(&a.totals->counters[PC_CNT_NOT_TRANSMITTED], v2);
			atomicAdd(&a.totals->counters[PC_CNT_IREFL], v3);
			if (v4) atomicAdd(&a.totals->counters[PC_CNT_FAILED], v4);
			atomicAdd(&a.totals->counters[PC_CNT_LAUNCHES], v5);
			atomicAdd(&a.totals->phase[PC_PH_MARCH], st_march); atomicAdd(&a.totals->phase[PC_PH_MARCH_LANES], st_march_l);
			atomicAdd(&a.totals->phase[PC_PH_EVENT], st_event); atomicAdd(&a.totals->phase[PC_PH_EVENT_LANES], st_event_l);
			atomicAdd(&a.totals->phase[PC_PH_NEW], st_new); atomicAdd(&a.totals->phase[PC_PH_NEW_LANES], st_new_l);
		}
		if (NE == 1 && lane == 0)
			pc_atomic_add128(a.sumw, u_acc_lo, u_acc_hi);
		if (NE == 1 && lane == 0 && SQ && (u_sq_lo | u_sq_hi))
			pc_atomic_add128(a.sumw2, u_sq_lo, u_sq_hi);
	}
}

#include "pc_pool_kernel.h"
#include "pc_producer_kernel.h"
#ifdef PC_EXPERIMENTS
#include "pc_wave_kernel.h"      /* the one-wave-per-photon experiment (profiles/r03/wave_per_photon_ab.txt): not part of the product build */
#endif
#include "pc_sweep_kernel.h"

/* Compact store: slots that used up their attempts without a transmitted photon wrote nothing (the slot-ordered store writes
 * zero weights for them), so the positions behind the run's cursor hold whatever the buffer held: zero them once the trace
 * kernel has ended -- every plane and the weights -- so that a result with failed slots never carries stale data. */
__global__ void __launch_bounds__(256) pc_compact_tail_kernel(double *soa, long long n_total, int ne, const unsigned long long *cursor)
{
	const long long c = (long long)*cursor;
	if (c >= n_total) return;
	const long long cells = (n_total - c)*(long long)(PC_N_FIELDS + ne);
	for (long long t = (long long)blockIdx.x*blockDim.x + threadIdx.x; t < cells; t += (long long)gridDim.x*blockDim.x) {
		const long long p = c + t / (PC_N_FIELDS + ne);
		const int f = (int)(t % (PC_N_FIELDS + ne));
		if (f < PC_N_FIELDS) soa[(long long)f*n_total + p] = 0.;
		else soa[(long long)PC_N_FIELDS*n_total + p*ne + (f - PC_N_FIELDS)] = 0.;
	}
}

/* Image records (one contiguous record of 17 + n_energies doubles per slot) -> the planes of struct _polycap_images: 17
 * planes of n_total doubles each, then the weights as [slot][n_energies].  A workgroup stages PC_SOA_TILE records in LDS
 * with coalesced reads and writes every plane with coalesced stores: 2 x 144 B of HBM traffic per photon, about a
 * millisecond per 1e7 photons, instead of a strided gather by host threads behind PCIe. */
#define PC_SOA_TILE 128
__global__ void __launch_bounds__(256) pc_soa_kernel(const double *rec, double *soa, long long first, long long count, long long n_total, int ne)
{
	extern __shared__ double tile[];
	const int recd = PC_N_FIELDS + ne;
	const long long j0 = first + (long long)blockIdx.x*PC_SOA_TILE;
	const int m = (int)((first + count - j0 < PC_SOA_TILE) ? first + count - j0 : PC_SOA_TILE);
	if (m <= 0) return;
	const double *src = rec + j0*recd;
	for (int k = threadIdx.x; k < m*recd; k += blockDim.x) tile[k] = src[k];
	__syncthreads();
	for (int k = threadIdx.x; k < m*PC_N_FIELDS; k += blockDim.x) {
		const int plane = k / m, t = k - plane*m;
		soa[(long long)plane*n_total + j0 + t] = tile[t*recd + plane];
	}
	double *w = soa + (long long)PC_N_FIELDS*n_total + j0*ne;
	for (int k = threadIdx.x; k < m*ne; k += blockDim.x) {
		const int t = k / ne, e = k - t*ne;
		w[k] = tile[t*recd + PC_N_FIELDS + e];
	}
}

/* source sampling only (parity of polycap_source_get_photon) */
__global__ void pc_sample_kernel(pc_params pm, unsigned long long seed, long long n,
                                 const long long *slots, const unsigned int *attempts, double *out)
{
	long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	pc_start s;
	if (pm.generic_src) pc_sample_photon<true>(pm, seed, (unsigned long long)slots[j], attempts[j], s);
	else pc_sample_photon<false>(pm, seed, (unsigned long long)slots[j], attempts[j], s);
	double *o = out + 12*j;
	o[0] = s.x; o[1] = s.y; o[2] = s.z; o[3] = s.dx; o[4] = s.dy; o[5] = s.dz;
	o[6] = s.ex; o[7] = s.ey; o[8] = s.ez; o[9] = s.srcx; o[10] = s.srcy; o[11] = 0.;
}

static thread_local std::string g_last_error;

static int pc_fail(int code, const std::string &msg)
{
	g_last_error = msg;
	return code;
}

#define PC_HIP_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) \
	return pc_fail(PC_HIP_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

/* Owners of the GPU resources of a context: each frees what it holds when it is reset or destroyed.  None of them switches
 * devices; whoever resets or destroys one has made its device current. */

/* device buffer of `cap` elements */
template <typename T>
struct pc_dev_buf {
	T *p = nullptr;
	size_t cap = 0;
	pc_dev_buf() = default;
	pc_dev_buf(pc_dev_buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	pc_dev_buf &operator=(pc_dev_buf &&o) noexcept
	{
		if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
		return *this;
	}
	~pc_dev_buf() { reset(); }
	operator T *() const { return p; }
	T *operator->() const { return p; }
	void reset()
	{
		if (p) (void)hipFree(p);
		p = nullptr; cap = 0;
	}
	/* at least `elems` elements: unless it has them, the buffer is replaced (contents lost) by one of max(elems, alloc).  A refused
	 * allocation leaves it empty and no HIP error stored, and is PC_HIP_ERR_MEMORY with `msg`. */
	int grow(size_t elems, const char *msg, size_t alloc = 0)
	{
		if (cap >= elems) return PC_HIP_OK;
		T *old = p;
		p = nullptr; cap = 0;
		if (old) PC_HIP_CHECK(hipFree(old));
		const size_t n = std::max(elems, alloc);
		if (hipMalloc(&p, n*sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			return pc_fail(PC_HIP_ERR_MEMORY, msg);
		}
		cap = n;
		return PC_HIP_OK;
	}
};

/* host buffer of `cap` elements in one of three shapes: pinned, or plain memory when pinning is refused (locked-memory limit);
 * pinned only; mapped into the device (coherent if the runtime grants it), with its device address `dev` */
enum pc_pin_kind { PC_PIN_OR_PLAIN, PC_PIN_ONLY, PC_PIN_MAPPED };

template <typename T, pc_pin_kind KIND>
struct pc_host_buf {
	T *p = nullptr;
	T *dev = nullptr;
	size_t cap = 0;
	bool pinned = false;
	pc_host_buf() = default;
	pc_host_buf(const pc_host_buf &) = delete;
	pc_host_buf &operator=(const pc_host_buf &) = delete;
	~pc_host_buf() { reset(); }
	operator T *() const { return p; }
	void reset()
	{
		if (p) { if (pinned) (void)hipHostFree(p); else free(p); }
		p = dev = nullptr; cap = 0; pinned = false;
	}
	/* as pc_dev_buf::grow */
	int grow(size_t elems, const char *msg, size_t alloc = 0)
	{
		if (cap >= elems) return PC_HIP_OK;
		T *old = p;
		const bool old_pinned = pinned;
		p = dev = nullptr; cap = 0; pinned = false;
		if (old && old_pinned) PC_HIP_CHECK(hipHostFree(old));
		else free(old);
		const size_t n = std::max(elems, alloc);
		void *q = nullptr;
		hipError_t e;
		if (KIND == PC_PIN_MAPPED) {
			e = hipHostMalloc(&q, n*sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
			if (e != hipSuccess) { (void)hipGetLastError(); e = hipHostMalloc(&q, n*sizeof(T), hipHostMallocMapped); }
		} else
			e = hipHostMalloc(&q, n*sizeof(T), hipHostMallocDefault);
		pinned = e == hipSuccess;
		if (!pinned) {
			(void)hipGetLastError();
			/* no pinned memory to be had: copies then go through the runtime's own staging, slower but correct */
			q = (KIND == PC_PIN_OR_PLAIN) ? malloc(n*sizeof(T)) : nullptr;
			if (!q) return pc_fail(PC_HIP_ERR_MEMORY, msg);
		}
		p = (T *)q;
		cap = n;
		if (KIND == PC_PIN_MAPPED) {
			e = hipHostGetDevicePointer((void **)&dev, p, 0);
			if (e != hipSuccess) { reset(); return pc_fail(PC_HIP_ERR_RUNTIME, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e)); }
		}
		return PC_HIP_OK;
	}
};

/* stream, created on first use: non-blocking, at the device's greatest priority when `high` and the device has priorities */
struct pc_stream_handle {
	hipStream_t s = nullptr;
	pc_stream_handle() = default;
	pc_stream_handle(const pc_stream_handle &) = delete;
	pc_stream_handle &operator=(const pc_stream_handle &) = delete;
	~pc_stream_handle() { if (s) (void)hipStreamDestroy(s); }
	operator hipStream_t() const { return s; }
	hipError_t ensure(bool high = false)
	{
		if (s) return hipSuccess;
		int least = 0, greatest = 0;
		if (high) {
			if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least
			    && hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) == hipSuccess)
				return hipSuccess;
			(void)hipGetLastError();
		}
		return hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
	}
};

/* event, created on first use */
struct pc_event_handle {
	hipEvent_t e = nullptr;
	pc_event_handle() = default;
	pc_event_handle(const pc_event_handle &) = delete;
	pc_event_handle &operator=(const pc_event_handle &) = delete;
	~pc_event_handle() { if (e) (void)hipEventDestroy(e); }
	operator hipEvent_t() const { return e; }
	hipError_t ensure(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

#define PC_IMAGES_STORE
#include "pc_images.h"      /* the store and the fetch: behind the kernels and the owner types */
#include "pc_leak_run.h"    /* the owner of leak runs; its functions follow the context and the leak kernels */

/* what a context was last asked to do (pc_hip_ctx::last_call) */
enum { PC_CALL_NONE = 0, PC_CALL_RUN, PC_CALL_RUN_LEAK, PC_CALL_EXPLICIT, PC_CALL_SCAN, PC_CALL_RELAY };

/* what the context a relay was traced into keeps of it, and the scratch of relays into it (pc_relay.h, pc_emit.h) */
struct pc_relay_state {
	pc_dev_buf<long long> d_map;           /* position in the first optic's store of every injected photon */
	pc_dev_buf<unsigned long long> d_scan; /* the scratch of the two compactions, then the finish kernel's counters (PC_RELAY_SCAN_WORDS) */
	pc_dev_buf<int> d_emap;                /* emit relays: which of the first optic's energies every energy of this context takes its weight from */
	pc_dev_buf<double> d_mu;               /* slab emits: the sample's attenuation coefficients, mu_in [the first optic's energies] before mu_out [this context's] */
	int acc_lds = 1;                       /* option "relay_acc_lds": 0 = the finish kernel adds to the global sums at once (tests) */
	int64_t counters[8] = {0};
	int64_t lost[3] = {0, 0, 0};           /* photons lost between the optics, at [outcome - PC_RELAY_REJECT]: rejected by the selection, missed
	                                        * the entrance plane (emit: the sample), missed the detector (emit only) */
	int kind = 0;                          /* PC_RELAY_KIND_*: what the relay it holds was */
};

struct pc_hip_ctx {
	pc_stream_handle stream;               /* first: destroyed after everything that may still be queued on it.  The context's one stream: a launch
	                                        * that goes elsewhere says so in its pc_launch_site */
	int device = 0;
	int n_cu = 256;
	pc_event_handle ev0, ev1;
	pc_host_tables host;
	pc_dev_buf<double> d_tables;           /* z, cap, zh, cap2, hexd, idz, ext: 7 x npts */
	pc_dev_buf<pc_energy_const> d_ec;
	pc_dev_buf<double> d_ec_soa;
	pc_dev_buf<pc_marg4> d_mg;             /* block-certificate records, npts */
	pc_dev_buf<pc_drdev> d_dr;             /* leak path: chord deviations of cap, npts */
	pc_launch_opts opts;                   /* the options that decide a launch (pc_plan.h) */
	double refl_per_launch = -1.;  /* EVENT visits (reflections, mostly) per launch in the last source run of this context; < 0: not known.
	                                * A big first run is preceded by a probe of 32768 slots (results unused) */
	int last_kernel = -1;          /* pc_hip_last_kernel */
	int last_run_plain = 0;        /* the last run was pc_hip_transmission_run (its counters tell refl_per_launch) */
	int run_squares = 0;           /* the last run did so (pc_hip_transmission_moments) */
	pc_dev_buf<double> d_rlog;
	int sweep_cert = 0;            /* pc_sweep_certificate has run */
	double sweep_ct_tame = 1.;
	int sweep_n_proxy = 0, sweep_proxy_e[2] = {0, 0};
	/* last run */
	pc_dev_buf<pc_totals> d_totals;        /* totals_bytes: the layout of pc_totals.h */
	size_t totals_bytes = 0;
	pc_image_store img;                    /* the exit-photon images of the last run, their options and the way out (pc_images.h) */
	pc_dev_buf<unsigned long long> d_work; /* one work counter per part */
	pc_dev_buf<double> d_wscratch;
	/* explicit-photon calls (polycap_photon_launch, polycap_source_get_photon): one device buffer and one pinned host
	 * buffer, kept between calls, so that a single photon costs two copies and a launch instead of ten copies and
	 * as many allocations */
	pc_dev_buf<double> d_batch;
	pc_host_buf<double, PC_PIN_OR_PLAIN> h_batch;
	long long run_slots = 0;
	int run_pending = 0;
	float last_ms = 0.f;
	pc_leak_run leak;                      /* leak_calc=true runs: buffers, options, the run in flight and its event lists (pc_leak_run.h) */
	unsigned long long entries_epoch = 0;  /* grows with every call that replaces the entries a tally reads (source run, leak run, relay into the
	                                        * context, explicit launch; not a scan): a selection's mask belongs to one value (pc_select.h) */
	/* scans (pc_scan.h): buffers of their own, so that a scan leaves everything of the last run as it was */
	pc_dev_buf<pc_totals> d_scan_totals;   /* work counter and scheduler statistics of the last scan launch */
	pc_dev_buf<unsigned long long> d_scan_tot; /* per point: 6 counters, 2*ne weight sums, 2*ne squared-weight sums (pc_kargs::sumw of a scan) */
	pc_dev_buf<pc_scan_point> d_scan_pts;
	pc_dev_buf<double> d_scan_wscratch;    /* more than 8 energies: the scan kernel's per-lane weights */
	pc_dev_buf<double> d_scan_rlog;        /* a scan through the logging kernel: its per-lane reflection logs */
	int scan_log = 0;                      /* option "scan_log": scans that can log their reflections do (pc_plan_input::scan_log; kept here
	                                        * because pc_launch_opts is the fixed list tests/plan/plan_host.cpp counts) */
	int scan_kernel = -1;                  /* pc_hip_scan_last_kernel */
	pc_event_handle ev_scan0, ev_scan1;
	long long scan_points = 0;             /* points of the last scan call (0: none yet) */
	int scan_squares = 0;                  /* the last scan summed the squared weights */
	int scan_pending = 0;                  /* the last scan has not been waited for */
	float scan_ms = 0.f;
	/* relays (pc_relay.h): what a context did last decides whether its exit photons can be relayed, and the context a relay was
	 * traced into keeps the relay's counters beside what a source run leaves */
	int last_call = PC_CALL_NONE;
	std::vector<double> energies;          /* the problem's energy grid as given: two contexts relay only over bit-equal grids */
	pc_relay_state relay;
	long long run_slot0 = 0;               /* first slot of the last source run: an emission draws on the stream of its photon's slot (pc_emit.h) */
	/* gathers of a selection's entries (pc_gather.h) */
	int gather_tile = 0;                   /* option "gather_tile": entries per compaction tile, 0 = automatic */
	long long gather_chunk_rows = 0;       /* option "gather_chunk_rows": rows per staging chunk, 0 = as many as fit in 128 MiB */
};

static void pc_fill_common(pc_hip_ctx *ctx, pc_kargs &a)
{
	const size_t npts = (size_t)ctx->host.pm.nmax + 1;
	memset(&a, 0, sizeof(a));
	a.g_z = ctx->d_tables; a.g_cap = ctx->d_tables + npts; a.g_zh = ctx->d_tables + 2*npts;
	a.g_cap2 = ctx->d_tables + 3*npts; a.g_hexd = ctx->d_tables + 4*npts; a.g_idz = ctx->d_tables + 5*npts;
	a.g_ext = ctx->d_tables + 6*npts; a.g_stp = ctx->d_tables + 7*npts; a.g_istp = ctx->d_tables + 8*npts;
	a.g_mg = ctx->d_mg;
	a.g_dr = ctx->d_dr;
	a.ec = ctx->d_ec;
	a.ec_soa = ctx->d_ec_soa;
	a.pm = ctx->host.pm;
	a.pm.literal = ctx->opts.literal;
	a.event_threshold = ctx->opts.event_threshold;
	a.new_threshold = ctx->opts.new_threshold;
	a.march_burst = ctx->opts.march_burst;
	a.march_stop = (ctx->opts.march_stop > 0 && ctx->opts.march_stop < ctx->opts.event_threshold) ? ctx->opts.march_stop : ctx->opts.event_threshold;
	a.pool_refill = ctx->opts.pool_refill;
	a.totals = ctx->d_totals;
	a.work = &ctx->d_totals->next_slot;
	a.sumw = PC_TOTALS_SUMW(ctx->d_totals.p);
	a.sumw2 = ctx->opts.weight_squares ? PC_TOTALS_SUMW2(ctx->d_totals.p, ctx->host.pm.n_energies) : nullptr;
}

/* What pc_trace_log_kernel needs to know about the run's energies (once per context):
 *   ct_tame -- a cosine of the angle to the surface normal above which every energy's reflectivity stays at least 1e-11 below 1
 *     (and, being a ratio of sums of squares weighted by fs, fp >= -1e-16, above 0): no factor of such a reflection can be
 *     rejected by the reference's range test (src/polycap-capil.c:633-637) and every weight only falls.  Found by evaluating
 *     1 - R_s = 4 c Re(g) / |c + g|^2 and 1 - R_p = 4 c Re(conj(g) n^2) / |g + n^2 c|^2, g = sqrt(n^2 - sin^2) from the device's own
 *     constants (pc_fresnel3), in extended precision on 64 points per decade of c from 1 down to 1e-13, per energy: ct_tame =
 *     4 x the largest grid point at which some energy comes closer than 1e-11 (the device's factors are within 2.1e-12 relative of
 *     the host's at R >= 1e-6; tests/test_gpu_devmath.py checks that they stay below 1 - 1e-12 above ct_tame).
 *     Below the critical angle 1 - R ~ 4 c beta / (2 delta)^1.5, so for glass ct_tame ~ 1e-11.
 *   proxies -- the energies that reflect best at 3 and at 30 mrad (roughness included): the last ones to fall below 1e-4. */
static void pc_sweep_certificate(pc_hip_ctx *ctx)
{
	if (ctx->sweep_cert) return;
	const std::vector<pc_energy_const> &ec = ctx->host.ec;
	const int ne = (int)ec.size();
	auto refl = [](const pc_energy_const &k, long double c, long double &one_minus_rs, long double &one_minus_rp) {
		const long double zr = c*c - (long double)k.d2, zi = k.n2_im;
		const long double mag = sqrtl(zr*zr + zi*zi);
		long double gr = sqrtl(0.5L*(mag + fabsl(zr))), gi = (gr > 0.0L) ? 0.5L*fabsl(zi)/gr : 0.0L;
		if (zr < 0.0L) { const long double x = gr; gr = gi; gi = x; }
		if (zi < 0.0L) gi = -gi;
		const long double ar = (long double)k.n2_re*c, ai = (long double)k.n2_im*c;
		one_minus_rs = 4.0L*c*gr/((c + gr)*(c + gr) + gi*gi);
		one_minus_rp = 4.0L*(gr*ar + gi*ai)/((gr + ar)*(gr + ar) + (gi + ai)*(gi + ai));
	};
	long double worst = 0.0L;               /* largest grid point at which some energy is not safely below 1 */
	const long double step = powl(10.0L, -1.0L/64.0L);
	for (int e = 0; e < ne; e++) {
		long double c = 1.0L;
		for (int k = 0; k <= 13*64; k++, c *= step) {
			long double a, b;
			refl(ec[e], c, a, b);
			if (!(a >= 1.e-11L && b >= 1.e-11L) || !(a <= 1.0L && b <= 1.0L)) { if (c > worst) worst = c; break; }   /* scanning downwards: the first failure is the largest */
		}
	}
	long double tame = 4.0L*worst;
	if (tame < 4.e-13L) tame = 4.e-13L;     /* below the scanned range nothing is certified */
	ctx->sweep_ct_tame = (tame > 2.0L) ? 2.0 : (double)tame;      /* 2: no reflection is tame (cos theta <= 1) */
	int best[2] = {0, 0};
	const long double at[2] = {3.e-3L, 3.e-2L};
	for (int j = 0; j < 2; j++) {
		long double top = -1.0L;
		for (int e = 0; e < ne; e++) {
			long double a, b;
			refl(ec[e], at[j], a, b);
			const long double x = (long double)ec[e].rough_c*at[j];
			const long double r = (1.0L - 0.5L*(a + b))*expl(-x*x);
			if (r > top) { top = r; best[j] = e; }
		}
	}
	ctx->sweep_proxy_e[0] = best[0]; ctx->sweep_proxy_e[1] = best[1];
	ctx->sweep_n_proxy = (best[0] == best[1]) ? 1 : 2;
	ctx->sweep_cert = 1;
}

/* The one place a trace kernel is launched from: grows the per-lane scratch the plan asks for, copies the plan into the kernel
 * arguments, and launches between the context's events as far as the site wants them.  Only source runs have other than lane kernels,
 * and scans the logging kernel (option "scan_log"). */
template <int MODE>
static int pc_launch_planned(pc_hip_ctx *ctx, const pc_launch_site &site, const pc_launch_plan &p, pc_kargs &a)
{
	constexpr bool SOURCE = MODE == PC_MODE_SRC_CIRCULAR || MODE == PC_MODE_SRC_GENERIC;
	constexpr bool SCAN = MODE == PC_MODE_SCAN_CIRCULAR || MODE == PC_MODE_SCAN_GENERIC;
	constexpr bool CAN_SQ = MODE != PC_MODE_EXPLICIT;
	/* a scan has buffers of its own, so that it leaves everything of the last run as it was */
	pc_dev_buf<double> &wscratch = SCAN ? ctx->d_scan_wscratch : ctx->d_wscratch;
	pc_dev_buf<double> &rlog = SCAN ? ctx->d_scan_rlog : ctx->d_rlog;
	int st = wscratch.grow(p.half_w * (size_t)site.halves, SCAN ? "pc_hip_scan_run: could not allocate the per-lane weight scratch"
	                                                            : "could not allocate the per-lane weight scratch");
	if (!st) st = rlog.grow(p.half_l * (size_t)site.halves, SCAN ? "pc_hip_scan_run: could not allocate the reflection logs"
	                                                             : "could not allocate the reflection logs");
	if (st) return st;
	if (p.half_w) a.wscratch = wscratch + (size_t)site.half * p.half_w;
	if (p.half_l) a.rlog = rlog + (size_t)site.half * p.half_l;
	a.total_threads = (long long)p.grid * p.block;
	a.lds_acc = p.lds_acc; a.lds_ec = p.lds_ec; a.sweep_rough = p.sweep_rough;
	a.event_threshold = p.event_threshold; a.new_threshold = p.new_threshold;
	a.pool_event_min = p.pool_event_min; a.event_march = p.event_march;
	a.log_cap = p.log_cap; a.stage_ps = p.stage_ps; a.flush_min = p.flush_min;
	a.sweep_skip = p.sweep_skip; a.sweep_fuse = p.sweep_fuse; a.sweep_exact_every = p.sweep_exact_every;
	if (p.kernel == PC_KERNEL_LOG) {
		pc_sweep_certificate(ctx);
		a.n_proxy = ctx->sweep_n_proxy; a.proxy_e[0] = ctx->sweep_proxy_e[0]; a.proxy_e[1] = ctx->sweep_proxy_e[1];
		a.ct_tame = ctx->sweep_ct_tame;
	}
	if (site.record_ev0) PC_HIP_CHECK(hipEventRecord(ctx->ev0, site.stream));
#define PC_GO(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(p.grid), dim3(p.block), p.dyn_lds, site.stream, a)
#define PC_GO_SQ(K, ...) do { if (CAN_SQ && p.sq) PC_GO(K<__VA_ARGS__, CAN_SQ>); else PC_GO(K<__VA_ARGS__>); } while (0)
	switch (p.kernel) {
	case PC_KERNEL_LANE:     /* long profiles: only the NE = 1 and the any-n_energies kernels are built for the 2048 pitch */
		switch (p.pitch == 1024 ? p.kne : -1 - p.kne) {
		case 1: PC_GO_SQ(pc_trace_kernel, 1, MODE, 1024); break;
		case 4: PC_GO_SQ(pc_trace_kernel, 4, MODE, 1024); break;
		case 8: PC_GO_SQ(pc_trace_kernel, 8, MODE, 1024); break;
		case 0: PC_GO_SQ(pc_trace_kernel, 0, MODE, 1024); break;
		case -2: PC_GO_SQ(pc_trace_kernel, 1, MODE, PC_MAX_PITCH); break;
		case -1: PC_GO_SQ(pc_trace_kernel, 0, MODE, PC_MAX_PITCH); break;
		default: return pc_fail(PC_HIP_ERR_INVALID, "internal: register-weight kernels are built for profiles of up to 1024 points");
		}
		break;
	case PC_KERNEL_POOL: if constexpr (SOURCE) PC_GO_SQ(pc_trace_pool_kernel, MODE); break;
	case PC_KERNEL_LOG: if constexpr (SOURCE || SCAN) PC_GO_SQ(pc_trace_log_kernel, MODE); break;
	case PC_KERNEL_PRODUCER:
		if constexpr (SOURCE) {
			if (p.sq) PC_GO(pc_trace_producer_kernel<MODE, false, true>);
			else if (p.march_stats) PC_GO(pc_trace_producer_kernel<MODE, true>);
			else PC_GO(pc_trace_producer_kernel<MODE, false>);
		}
		break;
#ifdef PC_EXPERIMENTS
	case PC_KERNEL_WAVE: if constexpr (SOURCE) PC_GO(pc_trace_wave_kernel<MODE>); break;
#endif
	}
#undef PC_GO_SQ
#undef PC_GO
	if (SCAN) ctx->scan_kernel = p.kernel; else ctx->last_kernel = p.kernel;
	PC_HIP_CHECK(hipGetLastError());
	if (site.record_ev1) PC_HIP_CHECK(hipEventRecord(ctx->ev1, site.stream));
	return PC_HIP_OK;
}

/* plan, then launch: n_items slots (source runs), photons (explicit launches) or flat indices (scans) with the arguments in a */
template <int MODE>
static int pc_launch_kernel(pc_hip_ctx *ctx, const pc_launch_site &site, pc_kargs &a, long long n_items)
{
	pc_plan_input in;
	in.ne = ctx->host.pm.n_energies; in.npts = ctx->host.pm.nmax + 1; in.n_shells = ctx->host.pm.n_shells;
	for (const pc_energy_const &c : ctx->host.ec) {
		if (c.valid == 0.) in.all_valid = false;
		if (c.rough_c != 0.) in.rough = true;
	}
	in.n_cu = ctx->n_cu; in.refl_per_launch = ctx->refl_per_launch;
	in.mode = MODE == PC_MODE_EXPLICIT ? PC_PLAN_EXPLICIT : (MODE == PC_MODE_SCAN_CIRCULAR || MODE == PC_MODE_SCAN_GENERIC) ? PC_PLAN_SCAN : PC_PLAN_SOURCE;
	in.n_items = n_items; in.n_slots = a.n_slots; in.max_attempts = a.max_attempts; in.keep_images = a.keep_images != 0;
	in.squares = MODE != PC_MODE_EXPLICIT && ctx->opts.weight_squares != 0;
	in.force_lane = site.force_lane; in.halves = site.halves;
	in.scan_log = ctx->scan_log != 0;
	return pc_launch_planned<MODE>(ctx, site, pc_plan_launch(in, ctx->opts), a);
}

/* a big single-energy run of a context that does not know yet how long its photons live is preceded by a probe (pc_probe_lifetime) */
static bool pc_wants_probe(const pc_hip_ctx *ctx, long long n_slots)
{
	return ctx->opts.producer < 0 && ctx->refl_per_launch < 0. && ctx->host.pm.n_energies == 1 && n_slots >= 2000000;
}

#include "pc_leak_kernels.h"
#define PC_LEAK_RUN_BODY
#include "pc_leak_run.h"

extern "C" {

int pc_hip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

const char *pc_hip_last_error(void)
{
	return g_last_error.c_str();
}

void pc_hip_ctx_destroy(pc_hip_ctx *ctx)
{
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	delete ctx;
}

int pc_hip_ctx_create(const pc_hip_problem *problem, int device, pc_hip_ctx **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_ctx_create: ctx must not be NULL");
	*out = nullptr;
	int ndev = pc_hip_device_count();
	if (ndev <= 0) return pc_fail(PC_HIP_ERR_NO_DEVICE, "pc_hip_ctx_create: no HIP device available (the trace path has no CPU fallback)");
	if (device < 0 || device >= ndev) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_ctx_create: device index out of range");
	pc_hip_ctx *ctx = new pc_hip_ctx();
	ctx->device = device;
	std::string err;
	int rc = pc_build_tables(problem, ctx->host, err);
	if (rc) { delete ctx; return pc_fail(rc, "pc_hip_ctx_create: " + err); }
	ctx->energies.assign(problem->energies, problem->energies + problem->n_energies);
	const size_t npts = (size_t)ctx->host.pm.nmax + 1;
	if (npts > PC_MAX_PITCH) { delete ctx; return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_ctx_create: profile too long for the LDS tables (nmax <= 2047)"); }
#define PC_CTX_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::string m = std::string(#expr) + ": " + hipGetErrorString(_e); pc_hip_ctx_destroy(ctx); return pc_fail(PC_HIP_ERR_RUNTIME, m); } } while (0)
#define PC_CTX_GROW(buf, elems, what) do { int _st = (buf).grow((elems), "pc_hip_ctx_create: could not allocate " what); if (_st) { pc_hip_ctx_destroy(ctx); return _st; } } while (0)
	PC_CTX_CHECK(hipSetDevice(device));
	hipDeviceProp_t prop;
	PC_CTX_CHECK(hipGetDeviceProperties(&prop, device));
	ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	PC_CTX_CHECK(ctx->stream.ensure());
	if (const char *e = getenv("POLYCAP_PRODUCER"))          /* tests: force (1) or forbid (0) the launching-wave kernel */
		if (*e == '0' || *e == '1') ctx->opts.producer = *e - '0';
	PC_CTX_CHECK(ctx->ev0.ensure(hipEventDefault));
	PC_CTX_CHECK(ctx->ev1.ensure(hipEventDefault));
	ctx->img.bind(ctx->host.ec.size(), ctx->stream, ctx->ev1);
	PC_CTX_GROW(ctx->d_tables, 9*npts, "the profile tables");
	const std::vector<double> *src[9] = { &ctx->host.z, &ctx->host.cap, &ctx->host.zh, &ctx->host.cap2, &ctx->host.hexd, &ctx->host.idz, &ctx->host.ext,
	                                      &ctx->host.stp, &ctx->host.istp };
	for (int k = 0; k < 9; k++)
		PC_CTX_CHECK(hipMemcpy(ctx->d_tables + k*npts, src[k]->data(), npts*sizeof(double), hipMemcpyHostToDevice));
	PC_CTX_GROW(ctx->d_mg, npts, "the block certificates");
	PC_CTX_CHECK(hipMemcpy(ctx->d_mg, ctx->host.mg.data(), npts*sizeof(pc_marg4), hipMemcpyHostToDevice));
	PC_CTX_GROW(ctx->d_dr, npts, "the chord deviations");
	PC_CTX_CHECK(hipMemcpy(ctx->d_dr, ctx->host.dr.data(), npts*sizeof(pc_drdev), hipMemcpyHostToDevice));
	{
		/* at least 8 entries: the register-weight kernels read NE constants whatever n_energies is (surplus = copies of the last) */
		std::vector<pc_energy_const> ecp(ctx->host.ec);
		while (ecp.size() < 8) ecp.push_back(ecp.back());
		PC_CTX_GROW(ctx->d_ec, ecp.size(), "the energy constants");
		PC_CTX_CHECK(hipMemcpy(ctx->d_ec, ecp.data(), ecp.size()*sizeof(pc_energy_const), hipMemcpyHostToDevice));
	}
	{
		const size_t ne = ctx->host.ec.size();
		/* field-major constants of the weight sweeps (FORM 3): d2, Re n^2, Im n^2, max((Im n^2)^2, 2^-200), rough_c, valid, rough_c^2 */
		std::vector<double> soa(7*ne);
		for (size_t e = 0; e < ne; e++) {
			const pc_energy_const &c = ctx->host.ec[e];
			soa[e] = c.d2; soa[ne + e] = c.n2_re; soa[2*ne + e] = c.n2_im; soa[3*ne + e] = c.zi2;
			soa[4*ne + e] = c.rough_c; soa[5*ne + e] = c.valid; soa[6*ne + e] = c.rough_k2;
		}
		PC_CTX_GROW(ctx->d_ec_soa, soa.size(), "the energy constants");
		PC_CTX_CHECK(hipMemcpy(ctx->d_ec_soa, soa.data(), soa.size()*sizeof(double), hipMemcpyHostToDevice));
	}
	ctx->leak.opts.max_depth = (int)std::min(65536.0, 2.0*ctx->host.pm.n_shells + 16.0);
	ctx->totals_bytes = PC_TOTALS_BYTES(ctx->host.ec.size());
	PC_CTX_GROW(ctx->d_totals, (ctx->totals_bytes + sizeof(pc_totals) - 1)/sizeof(pc_totals), "the totals");
	PC_CTX_CHECK(hipMemset(ctx->d_totals, 0, ctx->totals_bytes));
#undef PC_CTX_CHECK
#undef PC_CTX_GROW
	*out = ctx;
	return PC_HIP_OK;
}

int pc_hip_set_option(pc_hip_ctx *ctx, const char *name, int64_t value)
{
	if (!ctx || !name) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_set_option: NULL argument");
	std::string n(name);
	if (n == "literal_march") ctx->opts.literal = value ? 1 : 0;
	else if (n == "event_threshold") { if (value < 1 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "event_threshold must be in [1,64]"); ctx->opts.event_threshold = (int)value; }
	else if (n == "new_threshold") { if (value < 1 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "new_threshold must be in [1,64]"); ctx->opts.new_threshold = (int)value; }
	else if (n == "march_stop") { if (value < 0 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "march_stop must be in [0,64]"); ctx->opts.march_stop = (int)value; }
	else if (n == "march_burst") { if (value < 1) return pc_fail(PC_HIP_ERR_INVALID, "march_burst must be >= 1"); ctx->opts.march_burst = (int)value; }
	else if (n == "block_size") { if (value < 64 || value > PC_BLOCK || (value % 64) != 0) return pc_fail(PC_HIP_ERR_INVALID, "block_size must be a multiple of 64 up to the compiled maximum"); ctx->opts.block_size = (int)value; }
	else if (n == "blocks_per_cu") { if (value < 1 || value > 8) return pc_fail(PC_HIP_ERR_INVALID, "blocks_per_cu must be in [1,8]"); ctx->opts.blocks_per_cu = (int)value; }
	else if (n == "lds_ec") ctx->opts.lds_ec = value ? 1 : 0;
	else if (n == "batch_reflections") ctx->opts.batch_reflections = value ? 1 : 0;
	else if (n == "log_cap") { if (value < 0 || value > 255) return pc_fail(PC_HIP_ERR_INVALID, "log_cap must be in [0,255] (0 = automatic)"); ctx->opts.log_cap = (int)value; }
	else if (n == "sweep_skip") ctx->opts.sweep_skip = value ? 1 : 0;
	else if (n == "log_min_energies") { if (value < 9) return pc_fail(PC_HIP_ERR_INVALID, "log_min_energies must be >= 9 (up to 8 energies have their weights in registers)"); ctx->opts.log_min_energies = (int)value; }
	else if (n == "flush_max") { if (value < 1 || value > 16) return pc_fail(PC_HIP_ERR_INVALID, "flush_max must be in [1,16]"); ctx->opts.flush_max = (int)value; }
	else if (n == "sweep_exact_every") { if (value < 0 || value > 0x7fffffff) return pc_fail(PC_HIP_ERR_INVALID, "sweep_exact_every must be in [0,2^31-1] (0 = off)"); ctx->opts.sweep_exact_every = (int)value; }
	else if (n == "weight_squares") { if (value < 0 || value > 1) return pc_fail(PC_HIP_ERR_INVALID, "weight_squares must be 0 or 1"); ctx->opts.weight_squares = (int)value; }
	else if (n == "scan_log") { if (value < 0 || value > 1) return pc_fail(PC_HIP_ERR_INVALID, "scan_log must be 0 or 1"); ctx->scan_log = (int)value; }
	else if (n == "sweep_fuse") { if (value < 0 || value > 2) return pc_fail(PC_HIP_ERR_INVALID, "sweep_fuse must be 0, 1 or 2"); ctx->opts.sweep_fuse = (int)value; }
	else if (n == "plane_images") ctx->img.opts.plane_images = value ? 1 : 0;
	else if (n == "compact_images") ctx->img.opts.compact_images = value ? 1 : 0;
	else if (n == "compact_parts") { if (value < 1 || value > PC_MAX_PARTS) return pc_fail(PC_HIP_ERR_INVALID, "compact_parts must be in [1,16]"); ctx->img.opts.compact_parts = (int)value; }
	else if (n == "slot_ids") ctx->img.opts.slot_ids = value ? 1 : 0;
	else if (n == "keep_pinned") ctx->img.opts.keep_pinned = value ? 1 : 0;
	else if (n == "block_shift") { if (value < 7 || value > 30) return pc_fail(PC_HIP_ERR_INVALID, "block_shift must be in [7,30]"); ctx->img.opts.blk_shift = (int)value; }
	else if (n == "run_parts") { if (value < 1 || value > PC_MAX_PARTS) return pc_fail(PC_HIP_ERR_INVALID, "run_parts must be in [1,16]"); ctx->img.opts.run_parts = (int)value; }
	else if (n == "relay_acc_lds") ctx->relay.acc_lds = value ? 1 : 0;
	else if (n == "gather_tile") { if (value < 0 || value > 65536 || (value != 0 && (value < 64 || value % 64 != 0))) return pc_fail(PC_HIP_ERR_INVALID, "gather_tile must be a multiple of 64 in [64,65536] (0 = automatic)"); ctx->gather_tile = (int)value; }
	else if (n == "gather_chunk_rows") { if (value < 0 || value > 0x7fffffff) return pc_fail(PC_HIP_ERR_INVALID, "gather_chunk_rows must be in [0,2^31-1] (0 = automatic)"); ctx->gather_chunk_rows = (long long)value; }
	else if (n == "fetch_threads") { if (value < 0 || value > 256) return pc_fail(PC_HIP_ERR_INVALID, "fetch_threads must be in [0,256]"); ctx->img.opts.fetch_threads = (int)value; }
	else if (n == "pool") ctx->opts.pool = value ? 1 : 0;
	else if (n == "wave_per_photon") {
#ifdef PC_EXPERIMENTS
		ctx->opts.wave_per_photon = value ? 1 : 0;
#else
		if (value) return pc_fail(PC_HIP_ERR_INVALID, "wave_per_photon: the experiment kernel is compiled only with -DPC_EXPERIMENTS (scripts/analysis/wave_per_photon_ab.py)");
#endif
	}
	else if (n == "march_stats") ctx->opts.march_stats = value ? 1 : 0;
	else if (n == "cu_share") { if (value < 1 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "cu_share must be in [1,64]"); ctx->opts.cu_share = (int)value; }
	else if (n == "producer") { if (value < -1 || value > 1) return pc_fail(PC_HIP_ERR_INVALID, "producer must be -1 (automatic), 0 or 1"); ctx->opts.producer = (int)value; }
	else if (n == "producer_new_min") { if (value < 1 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "producer_new_min must be in [1,64]"); ctx->opts.producer_new_min = (int)value; }
	else if (n == "producer_new_first") { if (value < 1 || value > 65) return pc_fail(PC_HIP_ERR_INVALID, "producer_new_first must be in [1,65]"); ctx->opts.producer_new_first = (int)value; }
	else if (n == "pool_refill") { if (value < 1 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "pool_refill must be in [1,64]"); ctx->opts.pool_refill = (int)value; }
	else if (n == "event_march") { if (value < 0 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "event_march must be in [0,64]"); ctx->opts.event_march = (int)value; }
	else if (n == "pool_event_min") { if (value < 1 || value > 128) return pc_fail(PC_HIP_ERR_INVALID, "pool_event_min must be in [1,128]"); ctx->opts.pool_event_min = (int)value; }
	else if (n == "pool_new_min") { if (value < 1 || value > 128) return pc_fail(PC_HIP_ERR_INVALID, "pool_new_min must be in [1,128]"); ctx->opts.pool_new_min = (int)value; }
	else if (n == "pool_march_min") { if (value < 1 || value > 64) return pc_fail(PC_HIP_ERR_INVALID, "pool_march_min must be in [1,64]"); ctx->opts.pool_march_min = (int)value; }
	else if (n == "leak_max_depth") { if (value < 2 || value > (1 << 20)) return pc_fail(PC_HIP_ERR_INVALID, "leak_max_depth must be in [2, 2^20]"); ctx->leak.opts.max_depth = (int)value; }
	else if (n == "leak_stack_mb") { if (value < 1) return pc_fail(PC_HIP_ERR_INVALID, "leak_stack_mb must be >= 1"); ctx->leak.opts.stack_bytes = (size_t)value << 20; }
	else if (n == "leak_order") { ctx->leak.opts.order = value != 0; }
	else if (n == "leak_slot_units") { ctx->leak.opts.slot_units = value != 0; }
	else if (n == "leak_heavy_lanes") { if (value < 0 || value > PC_WAVE) return pc_fail(PC_HIP_ERR_INVALID, "leak_heavy_lanes must be in 0..64"); ctx->leak.opts.heavy_lanes = (int)value; }
	else if (n == "leak_heavy_every") { if (value < 0) return pc_fail(PC_HIP_ERR_INVALID, "leak_heavy_every must be >= 0"); ctx->leak.opts.heavy_every = (int)value; }
	else if (n == "leak_capacity") { if (value < 0) return pc_fail(PC_HIP_ERR_INVALID, "leak_capacity must be >= 0"); ctx->leak.opts.capacity = (long long)value; }
	else return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_set_option: unknown option " + n);
	return PC_HIP_OK;
}

/* device + pinned host buffer of at least `elems` doubles for the explicit-photon calls */
static int pc_batch_buffers(pc_hip_ctx *ctx, size_t elems)
{
	const size_t want = elems < 4096 ? 4096 : elems + elems/4;
	int st = ctx->d_batch.grow(elems, "explicit-photon batch: device allocation failed", want);
	return st ? st : ctx->h_batch.grow(elems, "explicit-photon batch: host allocation failed", want);
}

/* An explicit-photon launch in three stages over one device buffer: 3 inputs [3N], rc [N ints padded], weights [N*ne], 3 outputs
 * [3N], irefl [N], dtravel [N].  upload: the caller's inputs through the pinned host buffer, which mirrors the device buffer (one
 * copy in); trace: the kernel over inputs that are on the device -- whoever put them there (pc_relay.h injects them with a
 * kernel); download: everything behind the inputs (one copy out) into the caller's arrays. */
struct pc_batch {
	size_t N = 0, ne = 0, doubles = 0;
	double *d_start = nullptr, *d_dir = nullptr, *d_ev = nullptr;
	int *d_rc = nullptr;
	double *d_w = nullptr, *d_ec = nullptr, *d_ed = nullptr, *d_ee = nullptr;
	long long *d_ir = nullptr;
	double *d_dt = nullptr;
};

/* the buffer(s) for n photons and where everything lies in them; host = false: the device buffer alone */
static int pc_batch_layout(pc_hip_ctx *ctx, int64_t n, bool host, pc_batch &b)
{
	const size_t ne = (size_t)ctx->host.pm.n_energies;
	const size_t N = (size_t)n;
	b.N = N; b.ne = ne;
	b.doubles = 9*N + N + N*ne + 9*N + N + N;
	int st = host ? pc_batch_buffers(ctx, b.doubles)
	              : ctx->d_batch.grow(b.doubles, "explicit-photon batch: device allocation failed", b.doubles < 4096 ? 4096 : b.doubles + b.doubles/4);
	if (st) return st;
	double *d = ctx->d_batch;
	b.d_start = d; b.d_dir = d + 3*N; b.d_ev = d + 6*N;
	b.d_rc = (int *)(d + 9*N);
	b.d_w = d + 10*N; b.d_ec = b.d_w + N*ne; b.d_ed = b.d_ec + 3*N; b.d_ee = b.d_ed + 3*N;
	b.d_ir = (long long *)(b.d_ee + 3*N);
	b.d_dt = (double *)(b.d_ir + N);
	return PC_HIP_OK;
}

static int pc_batch_upload(pc_hip_ctx *ctx, const pc_batch &b, const double *start_coords, const double *start_dir, const double *start_elecv)
{
	const size_t N = b.N;
	double *h = ctx->h_batch;
	memcpy(h, start_coords, 3*N*sizeof(double));
	memcpy(h + 3*N, start_dir, 3*N*sizeof(double));
	memcpy(h + 6*N, start_elecv, 3*N*sizeof(double));
	PC_HIP_CHECK(hipMemcpyAsync(ctx->d_batch, h, 9*N*sizeof(double), hipMemcpyHostToDevice, ctx->stream));
	return PC_HIP_OK;
}

/* clears the totals and traces the N photons whose inputs are in the device buffer; a leak launch has been waited for when it returns */
static int pc_batch_trace(pc_hip_ctx *ctx, const pc_batch &b, int leak)
{
	const int64_t n = (int64_t)b.N;
	PC_HIP_CHECK(hipMemsetAsync(ctx->d_totals, 0, ctx->totals_bytes, ctx->stream));
	ctx->run_squares = 0;          /* explicit launches keep no sums */
	pc_kargs a;
	pc_fill_common(ctx, a);
	a.n_slots = n; a.slot0 = 0; a.max_attempts = 1; a.keep_images = 0;
	a.sumw2 = nullptr;
	a.in_start = b.d_start; a.in_dir = b.d_dir; a.in_elecv = b.d_ev;
	a.out_rc = b.d_rc; a.out_weights = b.d_w; a.out_exit_coords = b.d_ec; a.out_exit_dir = b.d_ed; a.out_exit_elecv = b.d_ee;
	a.out_irefl = b.d_ir; a.out_dtravel = b.d_dt;
	if (!leak) return pc_launch_kernel<PC_MODE_EXPLICIT>(ctx, pc_launch_site{ctx->stream}, a, n);
	/* polycap_photon_launch(..., leak_calc=true): rerun with a larger record buffer until every event fits */
	pc_leak_run &L = ctx->leak;
	L.slot0 = 0;
	L.begin(n, pc_plan_leak_capacity(L.opts.capacity, (int)b.ne, n, 4096));
	int status = L.enqueue<PC_MODE_EXPLICIT>(*ctx, a);
	if (status) return status;
	PC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return L.run_until_fit(*ctx, &a);
}

static int pc_batch_download(pc_hip_ctx *ctx, const pc_batch &b, const double *start_elecv, int32_t *rc, double *weights, double *exit_coords,
                             double *exit_dir, double *exit_elecv, int64_t *i_refl, double *d_travel, int leak)
{
	const size_t N = b.N, ne = b.ne;
	double *d = ctx->d_batch, *h = ctx->h_batch;
	PC_HIP_CHECK(hipMemcpyAsync(h + 9*N, d + 9*N, (b.doubles - 9*N)*sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
	PC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	{
		const double *o = h + 9*N;        /* rc (ints, padded to N doubles), weights, exit coords / dir / elecv, irefl, dtravel */
		memcpy(rc, o, N*sizeof(int)); o += N;
		memcpy(weights, o, N*ne*sizeof(double)); o += N*ne;
		memcpy(exit_coords, o, 3*N*sizeof(double)); o += 3*N;
		memcpy(exit_dir, o, 3*N*sizeof(double)); o += 3*N;
		memcpy(exit_elecv, o, 3*N*sizeof(double)); o += 3*N;
		memcpy(i_refl, o, N*sizeof(long long)); o += N;
		memcpy(d_travel, o, N*sizeof(double));
	}
	/* The kernels work with the normalised electric vector (polycap_refl_polar normalises it in place at the first
	 * reflection, src/polycap-capil.c:492-494); a photon that never reached a reflection keeps the caller's vector */
	for (size_t j = 0; j < N; j++) {
		const bool untouched = (rc[j] == -2) || (!leak && (rc[j] == 2 || (rc[j] == 1 && i_refl[j] == 0)));
		if (untouched)
			for (int c = 0; c < 3; c++) exit_elecv[3*j + c] = start_elecv[3*j + c];
	}
	return PC_HIP_OK;
}

static int pc_launch_photons_impl(pc_hip_ctx *ctx, int64_t n, const double *start_coords, const double *start_dir, const double *start_elecv,
                                  int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
                                  int64_t *i_refl, double *d_travel, int leak)
{
	if (!ctx || n < 0 || !start_coords || !start_dir || !start_elecv || !rc || !weights || !exit_coords || !exit_dir || !exit_elecv || !i_refl || !d_travel)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_launch_photons: NULL argument");
	if (n == 0) return PC_HIP_OK;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	pc_batch b;
	int status = pc_batch_layout(ctx, n, true, b);
	if (status) return status;
	ctx->last_call = PC_CALL_EXPLICIT;
	ctx->entries_epoch++;
	status = pc_batch_upload(ctx, b, start_coords, start_dir, start_elecv);
	if (!status) status = pc_batch_trace(ctx, b, leak);
	if (!status) status = pc_batch_download(ctx, b, start_elecv, rc, weights, exit_coords, exit_dir, exit_elecv, i_refl, d_travel, leak);
	ctx->img.valid = 0;
	ctx->leak.events_of_run = 0;
	return status;
}

int pc_hip_launch_photons(pc_hip_ctx *ctx, int64_t n, const double *start_coords, const double *start_dir, const double *start_elecv,
                          int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
                          int64_t *i_refl, double *d_travel)
{
	return pc_launch_photons_impl(ctx, n, start_coords, start_dir, start_elecv, rc, weights, exit_coords, exit_dir, exit_elecv, i_refl, d_travel, 0);
}

int pc_hip_launch_photons_leak(pc_hip_ctx *ctx, int64_t n, const double *start_coords, const double *start_dir, const double *start_elecv,
                               int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
                               int64_t *i_refl, double *d_travel)
{
	return pc_launch_photons_impl(ctx, n, start_coords, start_dir, start_elecv, rc, weights, exit_coords, exit_dir, exit_elecv, i_refl, d_travel, 1);
}

int pc_hip_sample_photons(pc_hip_ctx *ctx, uint64_t seed, int64_t n, const int64_t *slots, const uint32_t *attempts, double *out)
{
	if (!ctx || n < 0 || !slots || !attempts || !out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_sample_photons: NULL argument");
	if (n == 0) return PC_HIP_OK;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	const size_t N = (size_t)n;
	/* layout in the batch buffers: slots [N int64], attempts [N uint32, padded to N/2 + 1 doubles], out [12 N] */
	const size_t off_att = N, off_out = N + N/2 + 1, total = off_out + 12*N;
	{
		int st = pc_batch_buffers(ctx, total);
		if (st) return st;
	}
	double *d = ctx->d_batch, *h = ctx->h_batch;
	memcpy(h, slots, N*sizeof(long long));
	memcpy(h + off_att, attempts, N*sizeof(unsigned int));
	int status = PC_HIP_OK;
	hipError_t e = hipMemcpyAsync(d, h, off_out*sizeof(double), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(pc_sample_kernel, dim3((unsigned)((N + 255)/256)), dim3(256), 0, ctx->stream,
		                   ctx->host.pm, (unsigned long long)seed, (long long)n, (const long long *)d, (const unsigned int *)(d + off_att), d + off_out);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(h + off_out, d + off_out, 12*N*sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) status = pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_sample_photons: ") + hipGetErrorString(e));
	else memcpy(out, h + off_out, 12*N*sizeof(double));
	return status;
}

/* How long do photons live on this optic?  32768 slots with the default kernel (3 ms, results unused) set refl_per_launch, by
 * which the context -- or, for a device group, every member -- picks the kernel of its source runs.  Called where pc_wants_probe
 * holds: refl_per_launch is unknown, so the probe itself gets no launching wave, and it is too small to ask for a probe. */
static int pc_probe_lifetime(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, uint32_t max_attempts)
{
	int64_t c[6];
	int st = pc_hip_transmission_run(ctx, seed, slot0, 32768, max_attempts, 0);
	if (st == PC_HIP_OK) st = pc_hip_transmission_totals(ctx, nullptr, c, nullptr);
	return (st == PC_HIP_ERR_ATTEMPTS) ? PC_HIP_OK : st;
}

/* lanes of the largest launch the context makes: one 64-byte line of pc_kargs::lane_start each */
static size_t pc_lane_start_lanes(const pc_hip_ctx *ctx)
{
	return (size_t)ctx->n_cu * (size_t)std::max(ctx->opts.blocks_per_cu*ctx->opts.block_size, 1024);
}

int pc_hip_transmission_run(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, int64_t n_slots, uint32_t max_attempts, int keep_images)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_run: ctx must not be NULL");
	if (n_slots < 1 || slot0 < 0) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_run: n_slots must be >= 1 and slot0 >= 0");
	if (max_attempts < 1) max_attempts = 1;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	const size_t ne = (size_t)ctx->host.pm.n_energies;
	if (pc_wants_probe(ctx, n_slots)) {
		/* first big run of the context: 32768 slots with the default kernel tell how long photons live here (3 ms, results unused) */
		int st = pc_probe_lifetime(ctx, seed, slot0, max_attempts);
		if (st != PC_HIP_OK) return st;
	}
	ctx->last_run_plain = 1;
	ctx->leak.events_of_run = 0;
	ctx->entries_epoch++;
	ctx->run_squares = ctx->opts.weight_squares;
	ctx->last_call = PC_CALL_RUN;
	pc_kargs a;
	pc_fill_common(ctx, a);
	/* option "plane_images" (set by polycap_source_get_transmission_efficiencies): the kernels store the planes of struct
	 * _polycap_images themselves -- 18 scattered 8-byte stores per exit photon instead of two contiguous pieces of a record,
	 * 5 % of the HBM bandwidth at most -- and the fetch is a plain copy of planes into the caller's pinned memory */
	ctx->img.reset();
	pc_image_plan plan = pc_plan_images(n_slots, (int)ne, keep_images != 0, ctx->img.opts);
	/* a compact run's block flags are cleared from the host: a run of this context that is still in flight would set flags of its own
	 * after that (and the fetch of the new run would copy blocks the new kernel has not written) */
	if (plan.layout == PC_IMG_COMPACT && ctx->run_pending) {
		int st = pc_hip_transmission_wait(ctx, nullptr);
		if (st) return st;
	}
	{
		int st = ctx->img.prepare(plan, pc_lane_start_lanes(ctx));
		if (st) return st;
	}
	const bool compact = plan.layout == PC_IMG_COMPACT;
	const int parts = plan.parts;
	const hipStream_t main_stream = ctx->stream;
	pc_launch_site site{main_stream};
	site.halves = plan.halves;
	PC_HIP_CHECK(hipMemsetAsync(ctx->d_totals, 0, ctx->totals_bytes, ctx->stream));
	a.seed = seed; a.max_attempts = max_attempts; a.keep_images = keep_images ? 1 : 0;
	int status = PC_HIP_OK;
	if (parts > 1) {
		/* Parts alternate between two streams.  Every launch fills the device with persistent workgroups, so the
		 * workgroups of part k+1 start exactly as those of part k run out of slots and leave: the tail of one part (its
		 * longest photons) is covered by the head of the next, and the parts still finish in order. */
		PC_HIP_CHECK(ctx->img.stream2.ensure());
		PC_HIP_CHECK(ctx->img.ev_sync.ensure());
		int st = ctx->d_work.grow(PC_MAX_PARTS, "pc_hip_transmission_run: could not allocate the work counters of the parts");
		if (st) return st;
		PC_HIP_CHECK(hipMemsetAsync(ctx->d_work, 0, PC_MAX_PARTS*sizeof(unsigned long long), main_stream));
		PC_HIP_CHECK(hipEventRecord(ctx->ev0, main_stream));
		PC_HIP_CHECK(hipEventRecord(ctx->img.ev_sync, main_stream));
		PC_HIP_CHECK(hipStreamWaitEvent(ctx->img.stream2, ctx->img.ev_sync, 0));     /* totals and counters are zero */
		site.record_ev0 = site.record_ev1 = false;
	}
	for (int k = 0; k < parts && status == PC_HIP_OK; k++) {
		const long long lo = plan.begin[k], hi = plan.begin[k + 1];
		a.slot0 = slot0 + lo; a.n_slots = hi - lo;
		ctx->img.kargs(a, k);
		if (parts > 1) {
			a.work = ctx->d_work + k;
			site.stream = (k & 1) ? (hipStream_t)ctx->img.stream2 : main_stream;
			site.half = k & 1;               /* the launch before and the one after run on the other stream: the other half */
		}
		if (compact) site.record_ev1 = false;    /* the kernel time ends behind the tail kernel below */
		status = ctx->host.pm.generic_src ? pc_launch_kernel<PC_MODE_SRC_GENERIC>(ctx, site, a, hi - lo)
		                                  : pc_launch_kernel<PC_MODE_SRC_CIRCULAR>(ctx, site, a, hi - lo);
		if (status == PC_HIP_OK && parts > 1) {
			PC_HIP_CHECK(ctx->img.ev_part[k].ensure());
			PC_HIP_CHECK(hipEventRecord(ctx->img.ev_part[k], site.stream));
		}
	}
	if (parts > 1 && status == PC_HIP_OK) {
		/* the main stream ends after every part: wait() synchronises it, and the kernel time runs to here */
		for (int k = 0; k < parts; k++)
			if (k & 1) PC_HIP_CHECK(hipStreamWaitEvent(main_stream, ctx->img.ev_part[k], 0));
	}
	if (compact && status == PC_HIP_OK) {
		hipLaunchKernelGGL(pc_compact_tail_kernel, dim3(64), dim3(256), 0, main_stream, ctx->img.d_soa, (long long)n_slots, (int)ne, ctx->img.d_cursor);
		PC_HIP_CHECK(hipGetLastError());
	}
	if ((parts > 1 || compact) && status == PC_HIP_OK)
		PC_HIP_CHECK(hipEventRecord(ctx->ev1, main_stream));
	if (status) return status;
	ctx->run_slots = n_slots;
	ctx->run_slot0 = slot0;
	ctx->run_pending = 1;
	ctx->img.valid = keep_images ? 1 : 0;
	return PC_HIP_OK;
}

int pc_hip_transmission_wait(pc_hip_ctx *ctx, float *kernel_ms)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_wait: ctx must not be NULL");
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	PC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	if (ctx->leak.pending) {
		/* leak run: fetch and order its events, repeating a launch that outgrew the record buffer */
		int st = ctx->leak.run_until_fit(*ctx, nullptr);
		ctx->leak.pending = 0;
		if (st) { ctx->run_pending = 0; return st; }
	}
	if (ctx->run_pending) {
		float ms = 0.f;
		PC_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
		ctx->last_ms = ms;
		ctx->run_pending = 0;
	}
	if (kernel_ms) *kernel_ms = ctx->last_ms;
	return PC_HIP_OK;
}

/* is this host address registered with the HIP runtime (pinned)? */
int pc_hip_host_is_pinned(const void *p)
{
	if (p == nullptr) return 0;
	unsigned int flags = 0;
	if (hipHostGetFlags(&flags, const_cast<void *>(p)) == hipSuccess) return 1;
	(void)hipGetLastError();
	return 0;
}

double pc_hip_fixed_to_double(uint64_t lo, uint64_t hi)
{
	return (double)(pc_exact_value(lo, hi) / PC_EXACT_2P62);
}

int pc_hip_transmission_totals(pc_hip_ctx *ctx, double *sum_weights, int64_t counters[6], uint64_t *sumw_fixed)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_totals: ctx must not be NULL");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	std::vector<unsigned char> buf(ctx->totals_bytes);
	PC_HIP_CHECK(hipMemcpy(buf.data(), ctx->d_totals, ctx->totals_bytes, hipMemcpyDeviceToHost));
	const pc_totals &t = *(const pc_totals *)buf.data();
	const unsigned long long *sw = PC_TOTALS_SUMW(&t);
	const size_t ne = (size_t)ctx->host.pm.n_energies;
	if (counters)
		for (int k = 0; k < PC_N_COUNTERS; k++) counters[k] = (int64_t)t.counters[k];
	if (t.counters[PC_CNT_LAUNCHES] > 0 && ctx->last_run_plain)
		ctx->refl_per_launch = (double)t.phase[PC_PH_EVENT_LANES] / (double)t.counters[PC_CNT_LAUNCHES];   /* segment visits (reflections, mostly) per launch,
		                                                                              * absorbed photons included: what the next run chooses its kernel by */
	for (size_t e = 0; e < ne; e++) {
		if (sum_weights) sum_weights[e] = pc_hip_fixed_to_double(sw[2*e], sw[2*e+1]);
		if (sumw_fixed) { sumw_fixed[2*e] = sw[2*e]; sumw_fixed[2*e+1] = sw[2*e+1]; }
	}
	if (t.counters[PC_CNT_FAILED] != 0)
		return pc_fail(PC_HIP_ERR_ATTEMPTS, "pc_hip_transmission_totals: some slots exhausted max_attempts without a transmitted photon");
	return PC_HIP_OK;
}

int pc_hip_transmission_moments(pc_hip_ctx *ctx, uint64_t *sumw2_fixed)
{
	if (!ctx || !sumw2_fixed) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_moments: NULL argument");
	if (!ctx->run_squares) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_moments: the last run was made without option weight_squares");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	const size_t ne = (size_t)ctx->host.pm.n_energies;
	PC_HIP_CHECK(hipMemcpy(sumw2_fixed, PC_TOTALS_SUMW2(ctx->d_totals.p, ne), 2*ne*sizeof(uint64_t), hipMemcpyDeviceToHost));
	return PC_HIP_OK;
}

void pc_hip_efficiency_stderr(size_t n_energies, const uint64_t *sumw_fixed, const uint64_t *sumw2_fixed, const int64_t counters[6], double *out)
{
	/* N = every started photon: exit photons, not entered, not transmitted (the efficiency's denominator, open_area cancelled) */
	const long double n = (long double)counters[PC_CNT_EXIT] + (long double)counters[PC_CNT_NOT_ENTERED] + (long double)counters[PC_CNT_NOT_TRANSMITTED];
	for (size_t e = 0; e < n_energies; e++) {
		if (!(n >= 2.0L)) { out[e] = NAN; continue; }
		const long double a = pc_exact_value(sumw_fixed[2*e], sumw_fixed[2*e + 1]), b = pc_exact_value(sumw2_fixed[2*e], sumw2_fixed[2*e + 1]);
		out[e] = pc_exact_stderr(a / (n * PC_EXACT_2P62), b / (n * PC_EXACT_2P62), n);
	}
}

int pc_hip_last_kernel(pc_hip_ctx *ctx)
{
	return ctx ? ctx->last_kernel : -1;
}

int pc_hip_phase_stats(pc_hip_ctx *ctx, int64_t stats[6])
{
	if (!ctx || !stats) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_phase_stats: NULL argument");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	pc_totals t;
	PC_HIP_CHECK(hipMemcpy(&t, ctx->d_totals, sizeof(t), hipMemcpyDeviceToHost));
	for (int k = 0; k < PC_N_PHASE; k++) stats[k] = (int64_t)t.phase[k];
	return PC_HIP_OK;
}

int pc_hip_sweep_stats(pc_hip_ctx *ctx, int64_t stats[4], double *ct_tame, int proxies[2])
{
	if (!ctx || !stats) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_sweep_stats: NULL argument");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	pc_totals t;
	PC_HIP_CHECK(hipMemcpy(&t, ctx->d_totals, sizeof(t), hipMemcpyDeviceToHost));
	const bool log_run = ctx->last_kernel == PC_KERNEL_LOG;
	stats[0] = log_run ? (int64_t)t.phase[PC_PH_LOG_PASSES] : 0;
	stats[1] = log_run ? (int64_t)t.phase[PC_PH_LOG_ITERS] : 0;
	stats[2] = log_run ? (int64_t)t.counters[PC_CNT_LOG_LIFE_SUM] : 0;
	stats[3] = log_run ? (int64_t)t.counters[PC_CNT_LOG_LIFE_MAX] : 0;
	if (ct_tame) *ct_tame = ctx->sweep_cert ? ctx->sweep_ct_tame : -1.;
	if (proxies) { proxies[0] = ctx->sweep_cert ? ctx->sweep_proxy_e[0] : -1; proxies[1] = (ctx->sweep_cert && ctx->sweep_n_proxy > 1) ? ctx->sweep_proxy_e[1] : -1; }
	return PC_HIP_OK;
}

/* images [first, first + count) of the last run into the caller's planes (pc_image_planes; or null) or as records into raw */
static int pc_fetch_images(pc_hip_ctx *ctx, int64_t first, int64_t count, void *const *planes, double *raw)
{
	if (!ctx->img.valid) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_images: the last run kept no images");
	if (first < 0 || count < 0 || first + count > ctx->run_slots) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_images: slot range out of bounds");
	/* a leak run is complete (and possibly repeated) only after wait(); a plain run in parts is fetched part by part, and the planes
	 * of a compact run block by block, while it is traced */
	if (ctx->leak.pending || (ctx->img.plan.fetch_parts <= 1 && !(ctx->img.plan.layout == PC_IMG_COMPACT && planes && !raw))) {
		int st = pc_hip_transmission_wait(ctx, nullptr);
		if (st) return st;
	}
	if (count == 0) return PC_HIP_OK;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	return pc_fetch_images(ctx->img, first, count, planes, raw);
}

int pc_hip_transmission_images(pc_hip_ctx *ctx, int64_t first, int64_t count, const pc_hip_images *dst)
{
	if (!ctx || !dst) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_images: NULL argument");
	void *planes[PC_N_FIELDS + 1];
	pc_image_planes(dst, planes);
	return pc_fetch_images(ctx, first, count, planes, nullptr);
}

int pc_hip_transmission_slot_ids(pc_hip_ctx *ctx, int64_t first, int64_t count, int64_t *slots)
{
	if (!ctx || (count > 0 && !slots)) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_slot_ids: NULL argument");
	if (first < 0 || count < 0 || first + count > ctx->run_slots) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_slot_ids: range out of bounds");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	const long long *ids = ctx->img.valid ? ctx->img.device_view().ids : nullptr;
	if (!ids) {
		/* a run that stores every photon at its slot: the identity */
		for (int64_t k = 0; k < count; k++) slots[k] = first + k;
		return PC_HIP_OK;
	}
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	if (count) PC_HIP_CHECK(hipMemcpy(slots, ids + first, (size_t)count*sizeof(long long), hipMemcpyDeviceToHost));
	return PC_HIP_OK;
}

int pc_hip_transmission_records(pc_hip_ctx *ctx, int64_t first, int64_t count, double *records)
{
	if (!ctx || !records) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_records: NULL argument");
	return pc_fetch_images(ctx, first, count, nullptr, records);
}

/* src/polycap-source.c:1066-1076 */
void pc_hip_efficiencies(size_t n_energies, const double *sum_weights, const int64_t counters[6], double *efficiencies)
{
	int64_t sum_iexit = counters[0], sum_not_entered = counters[1], sum_not_transmitted = counters[2];
	double open_area = (double)(sum_iexit+sum_not_transmitted)/(sum_iexit+sum_not_entered+sum_not_transmitted);
	for (size_t i = 0; i < n_energies; i++)
		efficiencies[i] = (sum_weights[i] / ((double)sum_iexit+(double)sum_not_transmitted)) * open_area;
}

void pc_hip_host_unregister(void *ptr)
{
	if (ptr && hipHostUnregister(ptr) != hipSuccess) (void)hipGetLastError();
}

int pc_hip_device_synchronize(pc_hip_ctx *ctx)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_device_synchronize: ctx must not be NULL");
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	PC_HIP_CHECK(hipDeviceSynchronize());
	return PC_HIP_OK;
}

int pc_hip_device_memory(pc_hip_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_device_memory: ctx must not be NULL");
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	size_t f = 0, t = 0;
	PC_HIP_CHECK(hipMemGetInfo(&f, &t));
	if (free_bytes) *free_bytes = f;
	if (total_bytes) *total_bytes = t;
	return PC_HIP_OK;
}

} /* extern "C" */

#include "pc_group.h"
#include "pc_tally.h"
#include "pc_spot.h"
#include "pc_beam.h"
#include "pc_hist.h"
#include "pc_joint.h"
#include "pc_select.h"
#include "pc_gather.h"
#include "pc_draw.h"
#include "pc_scan.h"
#include "pc_relay.h"
#include "pc_emit.h"

/*
 * pc_trace_kernel.h -- the lane trace kernel (pc_trace_kernel: source runs, explicit photons and scans of up to 8 energies in
 * registers, any number in the per-lane scratch), the tunables and device helpers it shares with the pool, launching-wave,
 * logging and leak kernels (image-record stores, exact 128-bit sums, constant loads, lane states, the MODE values), and the
 * sampling-only kernel.  Included by pc_kernels.hip behind pc_kargs.h and pc_images.h (the record fields).
 */
#ifndef PC_TRACE_KERNEL_H
#define PC_TRACE_KERNEL_H

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

#endif /* PC_TRACE_KERNEL_H */

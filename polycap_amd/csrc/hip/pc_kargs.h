/*
 * pc_kargs.h -- the one argument struct of every trace kernel (lane, pool, launching-wave, logging and leak kernels) and the
 * scan's view of it.  A header of its own because the image store (pc_images.h) fills it and precedes the kernels, which in turn
 * write the store's record fields.  No field moves and none is added in the middle: the kernels read their arguments at fixed
 * offsets, and a shifted offset changes the code of every one of them (sumw2 and the scans' reuse of in_start, img_id0 and img_n
 * below are what that rule has cost so far).  Included by pc_kernels.hip.
 */
#ifndef PC_KARGS_H
#define PC_KARGS_H

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
	int n_proxy, proxy_e[2];      /* energies whose weights every lane carries itself (pc_sweep_certify) */
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

#endif /* PC_KARGS_H */

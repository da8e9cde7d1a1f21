/*
 * pc_plan.h -- which kernel a trace launch runs and in what shape: the options the decision reads (pc_launch_opts), what a launch
 * needs (pc_launch_plan) and the one function between them (pc_plan_launch), which works on plain values: no HIP call, no context.
 * So the header compiles for the host (-DPC_PLAN_HOST_ONLY leaves out pc_launch_site; tests/plan/plan_host.cpp).  The only reader
 * of a plan is pc_launch_planned of pc_launch.h.  Also here, because the decision needs them: the kernels' workgroup shapes
 * and LDS size formulas.
 */
#ifndef PC_PLAN_H
#define PC_PLAN_H

#include <algorithm>
#include <cstddef>

/* ---- shapes of the kernels */
#ifndef PC_BLOCK
#define PC_BLOCK 512            /* maximum workgroup size the trace kernel is compiled for */
#endif
#define PC_WAVE 64
#define PC_MAX_PITCH 2048      /* largest profile kept in static LDS: (6 x 8 + 4 x 4) B x 2048 = 128 KB */
/* pc_pool_kernel.h */
#ifndef PQ_BLOCK
#define PQ_BLOCK 768       /* one workgroup per CU */
#endif
#define PQ_WAVES (PQ_BLOCK / PC_WAVE)
#define PQ_PITCH 1024
#ifndef PQ_P
#define PQ_P 64            /* parked photons per wave (at most 64: one mask bit each) */
#endif
/* pc_producer_kernel.h */
#ifndef PC3_BLOCK
#define PC3_BLOCK 1024         /* one workgroup per CU: 1 launching + 15 tracing waves, the tables once in LDS */
#endif
#define PC3_WAVES (PC3_BLOCK / PC_WAVE)
#define PC3_CONSUMERS (PC3_WAVES - 1)
#define PC3_PITCH 1024
#define PC3_MIN_REFL 4.0      /* option "producer" = -1: reflections per launch from which this kernel is used (xos1 at 10-30 keV: 26-12,
                               * always 10-16 % faster; cone.inp: 0.3, 2x slower; scripts/analysis/producer_crossover.py) */
/* pc_sweep_kernel.h */
#ifndef PCS_BLOCK
#define PCS_BLOCK 512          /* 8 waves per CU, 2 per SIMD: 256 registers per lane (at 3 per SIMD and 168 registers a hundred of them lived in
                                * scratch, on the path of every EVENT phase: 28.9 against 28.2 ms at 291 energies, 18.1 against 15.4 ms at 100:
                                * profiles/r04/kernel_history.md); the sweeps keep the SIMD busy with two interleaved chains per wave */
#endif
#define PCS_PITCH 1024
#define PCS_MAXPS 16           /* photons of a wave swept in one round (their logs are staged in LDS) */
#define PCS_ENT 4              /* doubles of a staged log entry: cos sqrt(2), cos^2, fs, fp */
#define PCS_MARG_BYTES 16      /* sizeof(pc_marg4): the block certificates beside the tables in the logging kernel's static LDS */
/* pc_wave_kernel.h */
#define PCW_BLOCK 256

/* ---- dynamic LDS
 * of the any-n_energies kernel: exact sums and per-energy constants */
static size_t pc_ne0_dyn_lds(size_t ne, int lds_acc, int lds_ec, size_t acc_words)
{
	return (lds_acc ? acc_words*ne*sizeof(unsigned long long) : 0) + (lds_ec ? 6*ne*sizeof(double) : 0);
}

/* dynamic LDS of pc_trace_log_kernel: exact sums (with `squares`, those of the squared weights too), per-energy constants
 * (5 fields), per wave the sweep tables (4 x 16 words + 16 doubles) and `stage` doubles of staged logs */
static size_t pcs_dyn_lds(size_t ne, int block, size_t stage_doubles_per_wave, bool squares)
{
	return (squares ? 4 : 2)*ne*sizeof(unsigned long long) + 5*ne*sizeof(double)
	     + (size_t)(block/PC_WAVE)*(4*PCS_MAXPS*sizeof(unsigned int) + PCS_MAXPS*sizeof(double) + stage_doubles_per_wave*sizeof(double));
}

/* pc_trace_log_kernel applies to source runs with more than 8 valid energies on a profile of up to 1024 points whose sums and
 * constants fit in LDS beside a stage of at least one log per wave; returns the stage size (doubles per wave), 0 if not */
static size_t pc_log_stage_doubles(int ne, int log_cap, bool squares)
{
	const size_t fixed = 6*PCS_PITCH*sizeof(double) + PCS_PITCH*PCS_MARG_BYTES + pcs_dyn_lds((size_t)ne, PCS_BLOCK, 0, squares);
	if (fixed >= 163840) return 0;
	size_t per_wave = ((163840 - fixed)/(PCS_BLOCK/PC_WAVE))/sizeof(double);
	const size_t one = PCS_ENT*(size_t)log_cap;
	if (per_wave < one) return 0;
	size_t ps = per_wave/one;
	if (ps > PCS_MAXPS) ps = PCS_MAXPS;
	return ps*one;
}

/* ---- the options the decision reads (pc_hip_set_option writes them; pc_hip_ctx::opts) */
struct pc_launch_opts {
	int literal = 0;
	int event_threshold = 48;      /* lanes that must be marching for a MARCH burst to run before the waiting EVENTs.  With the short flights of
	                                * the current march (5.5 steps) the wave works almost in lockstep: 20 -> 44..48 is 26.2 -> 23.3 ms on xos1
	                                * (profiles/r02/kernel_history.md); optics with long flights (cone.inp) prefer ~24, ellip_l9 with roughness ~32 */
	int new_threshold = 2, march_burst = 16;
	int march_stop = 8;            /* a burst that has started goes on while this many lanes march (0: event_threshold): most flights end within it */
	int blocks_per_cu = 2, block_size = 512;
	int cu_share = 1;              /* option "cu_share": the context's launches fill n_cu / cu_share compute units.  Tried for device groups that list
	                                * a device m times (m kernels side by side on a quarter of the CUs each): the kernels of one process's streams
	                                * did not overlap (21.7 ms against 15.1 ms one after the other, xos1 5e6 slots, 4 members), so groups leave it at 1 */
	int producer = -1;             /* single-energy source runs with a launching wave per workgroup (pc_producer_kernel.h): 1 always, 0 never,
	                                * -1 when photons live long enough for one launching wave per CU to keep up (pc_hip_ctx::refl_per_launch):
	                                * -5 % on xos1 and ellip_l9, but 2.3x slower on cone.inp, whose photons hardly reflect */
	int producer_new_min = 2, producer_new_first = 6;
	int pool = 0;                  /* 1: single-energy source runs on profiles of up to 1024 points use the per-wave photon pool in LDS (pc_pool_kernel.h).
	                                * Was the default up to v14 (+6 %); since flights take 5.5 steps instead of 8.8 the exchanges with the pool cost more
	                                * than its fuller phases save (26.3 ms against 23.3 ms for the one-photon-per-lane kernel) */
	int pool_refill = 20, pool_march_min = 16, pool_event_min = 48, pool_new_min = 48, event_march = 0;
	int lds_ec = 1;                /* many-energy runs: per-energy constants in LDS, one 1024-thread workgroup per CU */
	int batch_reflections = 1;     /* more than 8 energies, source runs: 1 = reflections are logged and a photon's weights swept once per log
	                                * (pc_sweep_kernel.h), 0 = every reflection sweeps the weights at once */
	int log_cap = 0;               /* option "log_cap": reflections per log of pc_trace_log_kernel; 0 = 64 from 64 energies on, 32 below (shorter logs
	                                * leave room in LDS for the logs of more photons per sweep, which few energies need to fill their passes) */
	int log_min_energies = 9;      /* option "log_min_energies": source runs with at least this many energies log their reflections (9: every run whose
	                                * weights are not in registers; measured 9 ... 100 energies: +2 ... +130 % against the immediate sweep) */
	int flush_max = 8;             /* option "flush_max": at most this many finished photons of a wave wait for a common sweep */
	int sweep_skip = 1;            /* option "sweep_skip": histogram-only log runs stop multiplying a weight below 2^-64 */
	int sweep_fuse = 1;            /* option "sweep_fuse": histogram-only log runs add a finished photon's weights to the sums in its sweep; 2 = also when
	                                * its proxies are dead, so that photons the sweep finds dead exercise the take-back pass (tests) */
	int sweep_exact_every = 0;     /* option "sweep_exact_every" (test hook): > 0 = the logs of every photon whose slot is a multiple of it are swept by the
	                                * EXACT loop, so that sweep passes that mix EXACT and FAST photons are common (0 = off) */
	int march_stats = 0;           /* option "march_stats": the launching-wave kernel counts march steps and their lanes (pc_hip_phase_stats); off in
	                                * production runs, bench.py switches it on for one extra launch outside the timed steps */
	int wave_per_photon = 0;       /* EXPERIMENT (pc_wave_kernel.h): 1 = single-energy histogram-only source runs with one wave per photon */
	int weight_squares = 0;        /* option "weight_squares": source runs also sum the squared exit weights (pc_kargs::sumw2) */
};

/* compute units the launches of a context with these options fill */
static int pc_plan_cus(const pc_launch_opts &o, int n_cu)
{
	const int n = n_cu / (o.cu_share > 0 ? o.cu_share : 1);
	return n > 0 ? n : 1;
}

/* ---- the problem and the call, as far as the decision reads them */
enum { PC_PLAN_SOURCE = 0, PC_PLAN_EXPLICIT, PC_PLAN_SCAN };
struct pc_plan_input {
	int ne = 1, npts = 0;          /* pc_params::n_energies, nmax + 1 */
	double n_shells = 0.;
	bool all_valid = true, rough = false;  /* every energy's constants are valid; some energy has a roughness factor */
	int n_cu = 256;                /* the device's compute units */
	double refl_per_launch = -1.;  /* pc_hip_ctx::refl_per_launch */
	int mode = PC_PLAN_SOURCE;
	long long n_items = 0;         /* slots, photons or flat scan indices of this launch */
	long long n_slots = 0; unsigned int max_attempts = 1;     /* of pc_kargs, like keep_images */
	bool keep_images = false, squares = false;      /* squares: the launch sums the squared weights */
	bool force_lane = false; int halves = 1;        /* of the pc_launch_site */
	bool scan_log = false;         /* context option "scan_log" (not one of pc_launch_opts): a scan that can log its reflections does */
};

/* ---- what a launch needs */
enum { PC_KERNEL_LANE = 0, PC_KERNEL_POOL = 1, PC_KERNEL_PRODUCER = 2, PC_KERNEL_WAVE = 3, PC_KERNEL_LOG = 4 };   /* pc_hip_last_kernel */
struct pc_launch_plan {
	int kernel = PC_KERNEL_LANE;
	int kne = 0;                   /* lane kernel: weights in registers for up to 8 energies (kernels NE = 1, 4, 8), in the per-lane scratch beyond (0) */
	int pitch = 1024;              /* table pitch: 1024 entries (48 KB of LDS) covers the reference's generated profiles (nmax = 999) and its
	                                * example decks; long profiles: only the NE = 1 and the any-n_energies kernels are built for PC_MAX_PITCH */
	bool sq = false;               /* option "weight_squares": kernels of their own, so that the default kernels keep their registers */
	bool march_stats = false;
	int grid = 1, block = 0;
	size_t dyn_lds = 0;
	int lds_acc = 0, lds_ec = 0, sweep_rough = 0;
	size_t stage_doubles = 0;      /* logging kernel: staged logs per wave */
	int log_cap = 0, stage_ps = 0, flush_min = 0, sweep_skip = 0, sweep_fuse = 0, sweep_exact_every = 0;
	int event_threshold = 0, new_threshold = 0, pool_event_min = 0, event_march = 0;   /* pc_kargs, per kernel */
	size_t half_w = 0, half_l = 0; /* elements of pc_lane_scratch's d_wscratch and d_rlog per half (pc_launch_site::halves of them) */
};

static pc_launch_plan pc_plan_launch(const pc_plan_input &in, const pc_launch_opts &o)
{
	pc_launch_plan p;
	const int ne = in.ne, cus = pc_plan_cus(o, in.n_cu);
	const bool source = in.mode == PC_PLAN_SOURCE, short_profile = in.npts <= 1024;
	const bool scan_log = in.mode == PC_PLAN_SCAN && in.scan_log;
	/* u64 per energy of the exact sums a workgroup keeps in LDS: (lo, hi) of the weights, and of their squares with "weight_squares" */
	const size_t acc_words = (source && in.squares) ? 4 : 2;
	p.kne = (ne == 1) ? 1 : ((ne <= 4 && short_profile) ? 4 : ((ne <= 8 && short_profile) ? 8 : 0));
	p.pitch = short_profile ? 1024 : PC_MAX_PITCH;
	p.sq = in.mode != PC_PLAN_EXPLICIT && in.squares;
	p.sweep_rough = in.rough ? 1 : 0;
	p.event_threshold = o.event_threshold; p.new_threshold = o.new_threshold;
	if (in.mode == PC_PLAN_SCAN) {
		/* a scan's sums are per point, in global memory; its constants have the LDS to themselves */
		p.lds_ec = (p.kne == 0 && o.lds_ec && short_profile && 48*(size_t)ne <= 28672) ? 1 : 0;
	} else {
		/* with "weight_squares" the squared weights' sums sit beside the weights' and fall back to global atomics with them */
		p.lds_acc = (ne != 1 && acc_words*(size_t)ne*sizeof(unsigned long long) <= 16384) ? 1 : 0;
		/* many energies on a profile of up to 1024 points: one workgroup of 1024 threads per CU (the same 16 waves as two of
		 * 512) leaves room in LDS for the per-energy constants next to the tables and the sums */
		p.lds_ec = (p.kne == 0 && p.lds_acc && o.lds_ec && short_profile && (48 + 8*acc_words)*(size_t)ne <= 28672) ? 1 : 0;
	}
	/* the launching-wave and pool kernels' packed records: one energy, short profile, 24 bits of attempts, 39 of slots */
	const bool packable = ne == 1 && !o.literal && in.max_attempts <= (1u << 24) && in.n_shells < 16000. && in.n_slots < (1ll << 39);
	if (source) {
#ifdef PC_EXPERIMENTS
		if (o.wave_per_photon && ne == 1 && !in.keep_images && short_profile) {
			/* the experiment of pc_wave_kernel.h: one wave per photon, 16 waves per CU */
			p.kernel = PC_KERNEL_WAVE; p.block = PCW_BLOCK;
			p.grid = (int)std::max(1ll, std::min<long long>((in.n_items + 3) / 4, 4ll*in.n_cu));
			return p;
		}
#endif
		const bool want_producer = !in.force_lane && (o.producer == 1 || (o.producer < 0 && in.refl_per_launch >= PC3_MIN_REFL));
		if (want_producer && packable && in.npts <= PC3_PITCH) {
			const long long per_block = (long long)PC3_CONSUMERS*PC_WAVE;
			p.kernel = PC_KERNEL_PRODUCER; p.block = PC3_BLOCK;
			p.grid = (int)std::max(1ll, std::min<long long>((in.n_items + per_block - 1) / per_block, (long long)((PC3_BLOCK > 512) ? 1 : 2)*cus));
			p.new_threshold = o.producer_new_min; p.pool_event_min = o.producer_new_first;
			/* "weight_squares": one instantiation, without the march statistics (diagnostics) */
			p.march_stats = !p.sq && o.march_stats;
			return p;
		}
		/* the pool kernel serves single-energy source runs on profiles of up to 1024 points (what its packed records hold) */
		if (!in.force_lane && o.pool && packable && in.npts <= PQ_PITCH) {
			/* one workgroup per CU; a wave holds 64 + PQ_P photons */
			const long long per_block = (long long)PQ_WAVES*(PC_WAVE + PQ_P);
			p.kernel = PC_KERNEL_POOL; p.block = PQ_BLOCK;
			p.grid = (int)std::max(1ll, std::min<long long>((in.n_items + per_block - 1) / per_block, cus));
			p.event_threshold = o.pool_march_min; p.new_threshold = o.pool_new_min;
			p.pool_event_min = o.pool_event_min; p.event_march = o.event_march;
			return p;
		}
	}
	if (source || scan_log) {
		/* source runs with more than 8 (valid) energies log their reflections (pc_trace_log_kernel), and so do scans with option
		 * "scan_log", by the same rules: a point's log cuts, and with roughness its weights, are then those of a separate run.  (A scan's
		 * sums are per point in global memory: the workgroup's sum area in LDS sits unused, the layout is the source runs'.)  An explicit
		 * photon reports its state at the absorbing reflection, which the logging kernel's speculation overwrites */
		const bool want_log = p.kne == 0 && o.lds_ec && short_profile && ne >= o.log_min_energies && o.batch_reflections && in.all_valid;
		/* log capacity: 64 reflections (32 below 64 energies), halved while not even one log per wave fits in the stage beside
		 * the constants of very many energies (beyond ~450) */
		int log_cap = o.log_cap > 0 ? o.log_cap : (ne >= 64 ? 64 : 32);
		size_t stage = want_log ? pc_log_stage_doubles(ne, log_cap, in.squares) : 0;
		while (want_log && !stage && o.log_cap <= 0 && log_cap > 8) {
			log_cap /= 2;
			stage = pc_log_stage_doubles(ne, log_cap, in.squares);
		}
		if (stage) {
			/* reflections are logged, a photon's weights swept once per log (pc_sweep_kernel.h): one workgroup of 8 waves per CU */
			p.kernel = PC_KERNEL_LOG; p.block = PCS_BLOCK;
			p.grid = (int)std::max(1ll, std::min<long long>((in.n_items + PCS_BLOCK - 1) / PCS_BLOCK, cus));
			p.dyn_lds = pcs_dyn_lds((size_t)ne, PCS_BLOCK, stage, in.squares);
			/* one launch: its own lanes; parts: halves for the largest launch */
			const size_t lanes = (in.halves > 1) ? (size_t)cus * PCS_BLOCK : (size_t)p.grid * PCS_BLOCK;
			p.half_w = (size_t)ne * lanes; p.half_l = 3*(size_t)log_cap * lanes;
			p.log_cap = log_cap; p.stage_doubles = stage; p.stage_ps = (int)(stage/(PCS_ENT*(size_t)log_cap));
			/* photons that wait for a sweep before one is run: the fewest (up to the stage's capacity) whose last pass leaves at
			 * most 3 % of the round's lanes idle, else the count that leaves the fewest */
			int best = 1; double best_w = 2.;
			for (int n = 1; n <= p.stage_ps && n <= o.flush_max; n++) {
				const double w = (double)((64 - (n*ne) % 64) % 64) / (double)(n*ne);
				if (w < best_w - 1e-12) { best_w = w; best = n; }
				if (w <= 0.03) { best = n; break; }
			}
			p.flush_min = best;
			p.sweep_skip = (o.sweep_skip && !in.keep_images) ? 1 : 0;
			p.sweep_fuse = in.keep_images ? 0 : o.sweep_fuse;
			p.sweep_exact_every = o.sweep_exact_every;
			return p;
		}
	}
	/* the lane kernel: blocks_per_cu workgroups per CU with the weights in registers, one with them in the scratch */
	const long long max_blocks = (long long)cus * ((p.kne == 0) ? 1 : o.blocks_per_cu);
	p.block = o.block_size;
	p.grid = (int)std::max(1ll, std::min<long long>((in.n_items + p.block - 1) / p.block, max_blocks));
	p.dyn_lds = (p.kne == 0) ? pc_ne0_dyn_lds((size_t)ne, p.lds_acc, p.lds_ec, acc_words)
	                         : ((p.kne != 1 && p.lds_acc) ? acc_words*(size_t)ne*sizeof(unsigned long long) : 0);
	if (p.kne == 0)
		p.half_w = (size_t)ne * ((in.halves > 1) ? (size_t)max_blocks * (size_t)p.block : (size_t)p.grid * (size_t)p.block);
	return p;
}

#ifndef PC_PLAN_HOST_ONLY
/* ---- what belongs to one launch and not to the context; pc_launch_site{ctx->stream} is a launch timed by the context's events */
struct pc_launch_site {
	hipStream_t stream;
	bool record_ev0 = true, record_ev1 = true;   /* record pc_hip_ctx::ev0 before and ev1 behind the kernel */
	/* per-lane scratch (pc_lane_scratch) of a run cut into parts: launches on the two streams overlap, so the buffers are
	 * allocated twice over (halves = 2), each half sized for the largest launch the run can make, and the launches on
	 * stream2 use the second half (half = 1) */
	int halves = 1, half = 0;
	bool force_lane = false;               /* neither the launching-wave nor the pool kernel, whatever the options say */
};
#endif /* PC_PLAN_HOST_ONLY */

#endif /* PC_PLAN_H */

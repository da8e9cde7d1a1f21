/*
 * pc_totals.h -- the exact totals of a run: where they lie on the device.  No HIP types, compiles for the host.
 *
 * The block a trace kernel adds to -- struct pc_totals, then 2 n_energies u64 of (lo, hi) weight sums, then 2 n_energies u64 of
 * squared-weight sums (option "weight_squares") -- with names for its counters and scheduler statistics, and the block a scan keeps
 * per point.  The kernels' epilogues and every host reader use these names.
 */
#ifndef PC_TOTALS_H
#define PC_TOTALS_H

#include <stddef.h>

/* pc_totals::counters.  The first six are what a run reports (pc_hip_transmission_totals, the six of a scan point, the first six
 * limbs' worth of a device group's vector); the last two are the logging kernel's alone (pc_hip_sweep_stats) */
enum {
	PC_CNT_EXIT = 0, PC_CNT_NOT_ENTERED = 1, PC_CNT_NOT_TRANSMITTED = 2, PC_CNT_IREFL = 3,
	PC_CNT_FAILED = 4,            /* slots that used up max_attempts: PC_HIP_ERR_ATTEMPTS */
	PC_CNT_LAUNCHES = 5,
	PC_N_COUNTERS = 6,
	PC_CNT_LOG_LIFE_SUM = 6, PC_CNT_LOG_LIFE_MAX = 7      /* the waves' lifetimes in shader clock ticks: their sum, the longest */
};

/* pc_totals::phase (pc_hip_phase_stats): phases and the lanes active in them, per phase type; a leak run counts its four classes of
 * units the same way (PC_PH_LEAK_UNITS).  Slots 6 and 7 belong to the kernel that ran. */
enum {
	PC_PH_MARCH = 0, PC_PH_MARCH_LANES = 1, PC_PH_EVENT = 2, PC_PH_EVENT_LANES = 3, PC_PH_NEW = 4, PC_PH_NEW_LANES = 5,
	PC_N_PHASE = 6,
	PC_PH_POOL_SWAPS = 6,                       /* pool kernel */
	PC_PH_PRODUCER_BATCHES = 6,                 /* launching-wave kernel */
	PC_PH_LOG_PASSES = 6, PC_PH_LOG_ITERS = 7   /* logging kernel (pc_hip_sweep_stats) */
};
#define PC_PH_LEAK_UNITS(c) (2*(c))             /* leak kernel, class c = 0..3: units of work ... */
#define PC_PH_LEAK_LANES(c) (2*(c) + 1)         /* ... and the lanes that took them */

struct pc_totals {             /* device-resident totals of one run */
	unsigned long long counters[8];   /* PC_CNT_* */
	unsigned long long phase[8];      /* PC_PH_* */
	unsigned long long next_slot;     /* work counter (relative slot index) */
	unsigned long long pad;
	/* followed by the sums: PC_TOTALS_SUMW, PC_TOTALS_SUMW2 */
};

/* behind the header, in u64: (lo, hi) fixed-point weight sums per energy, then the same of the squared weights */
#define PC_TOTALS_SUMW(t) ((unsigned long long *)((t) + 1))
#define PC_TOTALS_SUMW2(t, ne) (PC_TOTALS_SUMW(t) + 2*(size_t)(ne))
#define PC_TOTALS_BYTES(ne) (sizeof(pc_totals) + 4*(size_t)(ne)*sizeof(unsigned long long))

/* The block of one scan point, in u64 (pc_kargs::sumw of a scan): the six counters, (lo, hi) weight sums, (lo, hi) squared-weight
 * sums.  ne in the type the caller counts in. */
#define PC_SCAN_COUNTERS 0
#define PC_SCAN_SUMS PC_N_COUNTERS
#define PC_SCAN_SQUARES(ne) (PC_N_COUNTERS + 2*(ne))
#define PC_SCAN_STRIDE(ne) (PC_N_COUNTERS + 4*(ne))

#endif /* PC_TOTALS_H */

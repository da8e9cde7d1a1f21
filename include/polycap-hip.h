/*
 * polycap-hip.h -- the thin C-ABI between libpolycap's host C code and its HIP (gfx950) kernels.
 *
 * Plain C: pointers, sizes and ints only; nothing HIP- or torch-typed crosses this boundary, so the
 * same entry points can be bound from C, ctypes, Cython or cgo.  The reference has no such layer (it
 * has no GPU code); each entry point names the reference function whose work it takes over.
 *
 * All functions return 0 on success or a negative pc_hip_status; pc_hip_last_error() gives the text.
 * There is no CPU fallback behind any of them: without a usable HIP device they fail with
 * PC_HIP_ERR_NO_DEVICE.
 */
#ifndef POLYCAP_HIP_H
#define POLYCAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifndef POLYCAP_EXTERN
#define POLYCAP_EXTERN __attribute__((visibility("default"))) extern
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
	PC_HIP_OK = 0,
	PC_HIP_ERR_NO_DEVICE = -1,   /* no HIP device / runtime not usable */
	PC_HIP_ERR_INVALID = -2,     /* bad argument or unsupported problem shape */
	PC_HIP_ERR_RUNTIME = -3,     /* a HIP API call or a kernel failed */
	PC_HIP_ERR_MEMORY = -4,      /* host or device allocation failed */
	PC_HIP_ERR_ATTEMPTS = -5     /* some slot used max_attempts launches without a transmitted photon */
} pc_hip_status;

/* One simulation problem: optic geometry + glass + energy tables + X-ray source.
 * Plain-array mirror of the reference's _polycap_profile / _polycap_description / _polycap_source
 * (src/polycap-private.h:88-122).  amu[]/scatf[] are what polycap_photon_scatf()
 * (src/polycap-photon.c:22-94) computes per launch; here they are computed once by the host.
 * Everything is copied at pc_hip_ctx_create(); the caller keeps ownership. */
typedef struct {
	int32_t nmax;                 /* profile arrays hold nmax+1 points, z strictly increasing, z[0] >= 0 */
	const double *z, *cap, *ext;
	double sig_rough;
	int64_t n_cap;
	double density;
	size_t n_energies;
	const double *energies, *amu, *scatf;
	double d_source, src_x, src_y, src_sigx, src_sigy, src_shiftx, src_shifty, hor_pol;
} pc_hip_problem;

/* Host destination planes for per-exit-photon "images": the SoA of struct _polycap_images
 * (src/polycap-private.h:156-181), leak fields excluded.  Any pointer may be NULL to skip that plane. */
typedef struct {
	double *src_start_coords[2];
	double *pc_start_coords[2];
	double *pc_start_dir[2];
	double *pc_start_elecv[2];
	double *pc_exit_coords[3];
	double *pc_exit_dir[2];
	double *pc_exit_elecv[2];
	int64_t *pc_exit_nrefl;
	double *pc_exit_dtravel;
	double *exit_coord_weights;   /* [count * n_energies], row-major by photon */
} pc_hip_images;

typedef struct pc_hip_ctx pc_hip_ctx;

POLYCAP_EXTERN int pc_hip_device_count(void);
POLYCAP_EXTERN const char *pc_hip_last_error(void);

/* Uploads the problem to `device` (tables resident in HBM, staged into LDS by every workgroup). */
POLYCAP_EXTERN int pc_hip_ctx_create(const pc_hip_problem *problem, int device, pc_hip_ctx **ctx);
POLYCAP_EXTERN void pc_hip_ctx_destroy(pc_hip_ctx *ctx);

/* Tuning / test switches (none of them changes a result):
 *   "literal_march"    1 = visit every segment with the reference's full quadratic, 0 = certified skipping (default)
 *   "event_threshold", "march_stop", "new_threshold", "march_burst", "blocks_per_cu", "block_size"   scheduler / launch shape:
 *                      a MARCH burst starts when event_threshold lanes march (48) and goes on while march_stop do (8)
 *   "lds_ec"           many energies: per-energy constants staged in LDS (default 1)
 *   "producer"         single-energy source runs with a launching wave per workgroup (pc_producer_kernel.h): 1 always, 0 never,
 *                      -1 (default) when photons live long enough (see pc_hip_last_kernel)
 *   "pool", "pool_refill", "pool_march_min", "pool_event_min", "pool_new_min"   single-energy source runs: the kernel
 *                      that parks 64 more photons per wave in LDS (pc_pool_kernel.h); "pool" 0 by default = one photon per lane
 *   "run_parts"        a transmission run that keeps images is traced as this many consecutive launches on two streams,
 *                      so that pc_hip_transmission_images can fetch finished parts while later ones run (default 1;
 *                      polycap_source_get_transmission_efficiencies uses 4 from 2e6 photons on; at most n_slots / 65536
 *                      launches).  Launches on the two streams overlap, so such a run keeps two sets of the kernels'
 *                      per-lane scratch (weight rows, reflection logs, compact start fields), one per stream
 *   "plane_images"     1 = a run that keeps images stores the planes of pc_hip_images itself (no records): pc_hip_transmission_images
 *                      is then a copy-engine transfer into the caller's planes, pinned for the duration of the call;
 *                      pc_hip_transmission_records is not available for such a run.  0 (default) = one record per slot,
 *                      turned into planes on the device when pc_hip_transmission_images asks for them
 *   "compact_images"   with "plane_images": 1 = exit photons are stored in the order in which they leave the optic instead of
 *                      at the position of their slot -- the photons a wave finalises together are one coalesced run per plane
 *                      (the reference's order of photons in its arrays is as arbitrary: it is the order in which OpenMP
 *                      threads with random seeds happen to fill them) -- and the planes are published in blocks of
 *                      2^"block_shift" positions (default 16) while the kernel runs: pc_hip_transmission_images copies the
 *                      blocks that are complete, as many at a time as have piled up.  The set of photons is the same as with 0 (default), bit for bit.
 *   "keep_pinned"      pc_hip_transmission_images leaves the destination planes it pinned (hipHostRegister) pinned: the
 *                      caller reuses them for later runs and unpins them with pc_hip_host_unregister before freeing them
 *   "slot_ids"         compact runs also record which slot sits at which position (pc_hip_transmission_slot_ids)
 *   "leak_order"       leak_calc source runs with two to five slots per lane hand out their slots heaviest first, predicted by
 *                      a plain pre-pass of the same slots, the heaviest n/400 to lanes of their own (default 1; 0 = slot order)
 *   "leak_heavy_lanes", "leak_heavy_every"   which lanes the heaviest slots go to: lanes 0 .. n-1 of every m-th wave (defaults 1, 1)
 *   "leak_slot_units"  leak_calc source runs keep the units of work per slot (pc_hip_leak_slot_units)
 *   "batch_reflections" source runs with more than 8 energies: 1 (default) reflections are logged (24 B each) and a photon's
 *                      weights swept once per log (any energy count whose sums and constants leave room in LDS for a log per
 *                      wave: to ~1400), 0 every reflection sweeps the weights at once
 *   "log_cap"          reflections per log of the logging kernel (1..255; default 0 = 64 from 64 energies on, 32 below, halved
 *                      while a log per wave does not fit beside the constants of more than ~450 energies)
 *   "log_min_energies" fewest energies of a source run that logs its reflections (default 9 = every run whose weights are
 *                      not in registers; >= 9)
 *   "sweep_skip"       histogram-only runs of the logging kernel stop multiplying a weight once it is below 2^-64 (it adds
 *                      nothing to the exact sums any more; default 1)
 *   "flush_max"        the logging kernel lets up to this many finished photons of a wave wait for a common sweep (default 8; the
 *                      count is chosen so that the last pass of a sweep is nearly full: 3 at 291 energies)
 *   "sweep_fuse"       histogram-only runs of the logging kernel: the sweep of a photon that has left the optic adds its weights
 *                      to the sums itself, no weight row is written (default 1; 2: also for photons whose proxy energies are
 *                      dead, which exercises the exact take-back pass; 0: off)
 *   "sweep_exact_every" test hook of the logging kernel: N > 0 sweeps the logs of every photon whose slot is a multiple of N by
 *                      the EXACT loop (range tests at every reflection), as if they held an untame reflection, so that sweep
 *                      passes mixing such photons with others are common; results stay correct (default 0 = off)
 *   "fetch_threads"    host threads of the staging fallback of the image fetch (0 = min(16, cores))
 *   "relay_acc_lds"    relays into this context (pc_hip_relay_run): 1 (default) = the finish kernel gathers a workgroup's exact sums in
 *                      LDS when they fit in 32 KB, 0 = it adds every wave's sums to the global pairs at once, as it does beyond
 *   "gather_tile", "gather_chunk_rows"   pc_hip_select_gather: entries per compaction tile (a multiple of 64 in 64 .. 65536) and rows
 *                      per staging chunk; 0 (default) = automatic for both (see the gathers below)
 *   leak runs: "leak_max_depth" (stack frames per lane = walls one photon may cross), "leak_stack_mb" (HBM for those
 *                      stacks), "leak_capacity" (leak record buffer, 0 = automatic; a run that outgrows it is repeated). */
POLYCAP_EXTERN int pc_hip_set_option(pc_hip_ctx *ctx, const char *name, int64_t value);

/* polycap_photon_launch (src/polycap-photon.c:390-955, leak_calc=false) for n explicit photons.
 * Inputs [3*n] xyz-interleaved host arrays; outputs rc[n] in {1,0,2,-2,-1}, weights[n*n_energies],
 * exit_*[3*n] (state at the last interaction, as polycap_photon_get_exit_*), i_refl[n], d_travel[n]. */
POLYCAP_EXTERN int pc_hip_launch_photons(pc_hip_ctx *ctx, int64_t n,
	const double *start_coords, const double *start_dir, const double *start_elecv,
	int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
	int64_t *i_refl, double *d_travel);

/* polycap_source_get_photon (src/polycap-source.c:23-144) evaluated on the device for the given
 * (slot, attempt) pairs of the Philox stream `seed`; out[12*n] = start(3), dir(3), elecv(3), src_start(3). */
POLYCAP_EXTERN int pc_hip_sample_photons(pc_hip_ctx *ctx, uint64_t seed, int64_t n,
	const int64_t *slots, const uint32_t *attempts, double *out);

/* polycap_source_get_transmission_efficiencies (src/polycap-source.c:448-1087, leak_calc=false) for the
 * exit-photon slots [slot0, slot0+n_slots): enqueue on the context's stream; results stay in HBM.
 * keep_images=0 is the histogram-only mode (no per-photon planes are allocated or written). */
POLYCAP_EXTERN int pc_hip_transmission_run(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, int64_t n_slots,
	uint32_t max_attempts, int keep_images);
/* Waits for the stream; *kernel_ms (optional) = duration of the trace kernel between two HIP events
 * recorded on that stream. */
POLYCAP_EXTERN int pc_hip_transmission_wait(pc_hip_ctx *ctx, float *kernel_ms);
/* Totals of the last run: sum_weights[n_energies]; counters = {iexit, not_entered, not_transmitted,
 * sum_irefl, failed_slots, launches}; sumw_fixed (optional) [2*n_energies] = exact 128-bit fixed-point sums
 * (lo, hi) in units of 2^-62, which add exactly across devices. */
POLYCAP_EXTERN int pc_hip_transmission_totals(pc_hip_ctx *ctx, double *sum_weights, int64_t counters[6], uint64_t *sumw_fixed);
/* ---- standard errors.  Every efficiency is a Monte Carlo mean: eff = sum(w) / N over the N started photons (an exit photon adds
 * its weight, one that did not enter or was not transmitted adds 0; the open_area factor of pc_hip_efficiencies cancels).  With
 * option "weight_squares" = 1 (pc_hip_set_option / pc_hip_group_set_option; default 0) source runs -- leak_calc runs included,
 * explicit-photon launches not -- also keep a second exact sum per energy, of the squared weights.  The contract, for each
 * exit photon and energy, with w the fp64 weight the sums already use (IEEE, no contraction):
 *   A += (uint64)(w * 2^62)            truncated: sumw_fixed, as without the option
 *   B += (uint64)((w * w) * 2^62)      w * w one fp64 product, then the scaling, truncated
 * B is a 128-bit (lo, hi) sum per energy laid out like sumw_fixed.  Both are integer sums, so B does not depend on the launch
 * shape, the kernel, "run_parts", the store, how the slots are split into runs, or the device count.
 * With N = counters[0] + counters[1] + counters[2], m = A / (N 2^62) and q = B / (N 2^62), all in long double:
 *   stderr = sqrt(max(0, q - m*m) / (N - 1)),  NaN when N < 2.
 * pc_hip_transmission_moments: B of the last run, sumw2_fixed [2*n_energies]; PC_HIP_ERR_INVALID when the last run was made
 * without the option.  pc_hip_efficiency_stderr: the formula above (pure host function, out [n_energies]). */
POLYCAP_EXTERN int pc_hip_transmission_moments(pc_hip_ctx *ctx, uint64_t *sumw2_fixed);
POLYCAP_EXTERN void pc_hip_efficiency_stderr(size_t n_energies, const uint64_t *sumw_fixed, const uint64_t *sumw2_fixed,
	const int64_t counters[6], double *out);
/* Copies image planes of slots [first, first+count) (relative to slot0 of the last run) to the host.  May be called
 * before pc_hip_transmission_wait: with "run_parts" > 1 it waits for the run part by part and copies the finished parts
 * while the later ones are traced (pinned staging, host threads build the planes).  NULL planes are skipped. */
POLYCAP_EXTERN int pc_hip_transmission_images(pc_hip_ctx *ctx, int64_t first, int64_t count, const pc_hip_images *dst);
/* The same data as the device keeps it: one record of PC_HIP_N_PLANES + n_energies doubles per slot, the planes of
 * pc_hip_images in their order (the reflection count as int64 bits in its place), then the slot's weights.
 * records: [count][PC_HIP_N_PLANES + n_energies]. */
#define PC_HIP_N_PLANES 17
POLYCAP_EXTERN int pc_hip_transmission_records(pc_hip_ctx *ctx, int64_t first, int64_t count, double *records);
/* Unpins host memory that a fetch with option "keep_pinned" left pinned. */
POLYCAP_EXTERN void pc_hip_host_unregister(void *ptr);
/* Slot (relative to slot0 of the last run) of the photon stored at positions [first, first+count) of the image planes:
 * the identity unless the run was compact ("compact_images" with "slot_ids"). */
POLYCAP_EXTERN int pc_hip_transmission_slot_ids(pc_hip_ctx *ctx, int64_t first, int64_t count, int64_t *slots);
/* leak_calc runs (reference: the static split of the photon loop over OpenMP threads, src/polycap-source.c:744): the order in
 * which the next source runs of exactly n slots hand out their slots -- a permutation of 0 .. n-1, heaviest slot first; the
 * first n_heavy of them are traced by a few lanes of every fourth wave (options leak_heavy_lanes, leak_heavy_every).  n = 0
 * restores slot order.  Results do not depend on the order.  pc_hip_leak_slot_units: units of work the last leak run (option
 * leak_slot_units = 1) spent on each slot. */
POLYCAP_EXTERN int pc_hip_leak_set_order(pc_hip_ctx *ctx, const uint32_t *order, int64_t n, int64_t n_heavy);
POLYCAP_EXTERN int pc_hip_leak_slot_units(pc_hip_ctx *ctx, int64_t first, int64_t count, uint32_t *units);

/* ---- leak_calc = true ("halo" photons): src/polycap-capil.c:610-619, 657-1194, src/polycap-photon.c:171-362, 645-907,
 * src/polycap-source.c:799-879, 925-1032.  Same calls with the fraction of every reflection that is transmitted through
 * the glass followed as well; the leak events of the run are kept by the context until the next run.
 * One event = PC_HIP_LEAK_HDR + n_energies doubles: slot (photon index for pc_hip_launch_photons_leak), attempt,
 * coords xyz, direction xyz, electric vector xyz, n_refl, weights[n_energies] (struct _polycap_leak,
 * include/polycap-photon.h:40-47).  Order = the reference's lists: by slot; inside a slot the events of the transmitted
 * photon first, then those of the earlier attempts. */
#define PC_HIP_LEAK_HDR 12
POLYCAP_EXTERN int pc_hip_launch_photons_leak(pc_hip_ctx *ctx, int64_t n,
	const double *start_coords, const double *start_dir, const double *start_elecv,
	int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
	int64_t *i_refl, double *d_travel);
POLYCAP_EXTERN int pc_hip_transmission_run_leak(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, int64_t n_slots,
	uint32_t max_attempts, int keep_images);
/* number of extleak (left the optic through its side) / intleak (reached the exit plane inside the glass) events */
POLYCAP_EXTERN int pc_hip_leak_counts(pc_hip_ctx *ctx, int64_t *n_ext, int64_t *n_int);
/* events [first, first+count) of kind 0 (extleak) or 1 (intleak) into records[count * (PC_HIP_LEAK_HDR + n_energies)] */
POLYCAP_EXTERN int pc_hip_leak_events(pc_hip_ctx *ctx, int kind, int64_t first, int64_t count, double *records);
/* the same without a copy: *records points at the context's own (pinned) list of *count events of that kind, in the reference's
 * list order (put into it on the device); valid until the context's next leak run or its destruction */
POLYCAP_EXTERN int pc_hip_leak_events_view(pc_hip_ctx *ctx, int kind, const double **records, int64_t *count);

/* Waits until the context's device is idle (hipDeviceSynchronize): every stream, not only the context's own. */
POLYCAP_EXTERN int pc_hip_device_synchronize(pc_hip_ctx *ctx);

/* ---- several devices from one process: the OpenMP team of the reference (src/polycap-source.c:697-745) becomes a group of
 * device contexts, one per entry of `devices` (an index may repeat: the contexts then share that GPU).  A run shards the
 * exit-photon slots [0, n_slots) into contiguous ranges, one per member, enqueued from the calling thread; photons are
 * keyed by (seed, global slot), so the result does not depend on the partition.  The totals of the members -- counters and
 * the exact 128-bit fixed-point weight sums, split into 32-bit limbs -- are added by ONE all-reduce over RCCL
 * (librccl bound at run time, ncclCommInitAll over the group's devices: the reference's omp critical sum, :973-980) when
 * the devices are distinct and RCCL is present, else limb by limb on the host: the same bits either way. */
typedef struct pc_hip_group pc_hip_group;
POLYCAP_EXTERN int pc_hip_group_create(const pc_hip_problem *problem, int n_devices, const int *devices, pc_hip_group **group);
POLYCAP_EXTERN void pc_hip_group_destroy(pc_hip_group *group);
POLYCAP_EXTERN int pc_hip_group_size(const pc_hip_group *group);
POLYCAP_EXTERN int pc_hip_group_set_option(pc_hip_group *group, const char *name, int64_t value);
POLYCAP_EXTERN int pc_hip_group_run(pc_hip_group *group, uint64_t seed, int64_t n_slots, uint32_t max_attempts, int keep_images);
/* leak_calc = true over the group: every member traces its contiguous slot range and orders its events on its own device; the
 * group's event lists are the members' lists one after the other (= slot order, as one device produces them).  Images and
 * totals through pc_hip_group_images / pc_hip_group_totals. */
POLYCAP_EXTERN int pc_hip_group_run_leak(pc_hip_group *group, uint64_t seed, int64_t n_slots, uint32_t max_attempts, int keep_images);
POLYCAP_EXTERN int pc_hip_group_leak_counts(pc_hip_group *group, int64_t *n_ext, int64_t *n_int);
POLYCAP_EXTERN int pc_hip_group_leak_events(pc_hip_group *group, int kind, int64_t first, int64_t count, double *records);
/* kernel that traced member k's share of the last run (as pc_hip_last_kernel) */
POLYCAP_EXTERN int pc_hip_group_last_kernel(pc_hip_group *group, int k);
/* image planes of all n_slots slots of the last run (one host thread per member copies its range into dst) */
POLYCAP_EXTERN int pc_hip_group_images(pc_hip_group *group, const pc_hip_images *dst);
/* totals as pc_hip_transmission_totals; *reduced_by (optional) = 1 when the sum was made by RCCL, 0 on the host;
 * *kernel_ms (optional) = the longest member kernel.  reduce: -1 automatic, 0 host, 1 RCCL (fails when it cannot) */
POLYCAP_EXTERN int pc_hip_group_totals(pc_hip_group *group, int reduce, double *sum_weights, int64_t counters[6], uint64_t *sumw_fixed,
	int *reduced_by, float *kernel_ms);
/* B of the group's last run (option "weight_squares"), summed over the members like the weights -- in the same all-reduce, the
 * packed vector growing to 6 + 8 n_energies int64 -- by the pc_hip_group_totals call for that run, which must come first */
POLYCAP_EXTERN int pc_hip_group_moments(pc_hip_group *group, uint64_t *sumw2_fixed);

/* ---- spot maps: weighted 2-D histograms of where the photons of the last run cross planes perpendicular to the optic axis,
 * downstream of its exit face, one map per selected energy, accumulated on the device in exact integers from what the run left
 * there (no copy to the host, no change to the run).
 *
 * The contract (IEEE fp64, evaluated in the order written, no contraction):
 *   planes     zp_k = z[nmax] + d_k, computed once on the host; d_k >= 0 in cm
 *   per entry  with position (x, y, z), direction (dx, dy, dz) and weights w[e]:
 *              exit photons: dz = sqrt((1 - dx*dx) - dy*dy) (their records carry dx and dy only); leak events: the stored dz
 *              t = (zp - z) / dz,  xd = x + dx*t,  yd = y + dy*t
 *              fx = ((xd - x0) / (x1 - x0)) * nx,  ix = floor(fx);  fy, iy the same way with y0, y1, ny
 *              inside when 0 <= fx < nx and 0 <= fy < ny; anything else is outside: NaN, dz <= 0, off the window
 *   weights    q(w) = round_half_even(w * 2^32) as uint64 (w <= 0 and NaN give 0); a bin holds the sum of q(w[e]) over its
 *              entries, and every (plane, energy) pair has one outside counter for the rest, so that for every map
 *              sum(bins) + outside == sum over the entries of q(w[e]), exactly
 *   entries    one map takes at most 2^32 - 1 entries over all its adds (then no uint64 can wrap); an add past that fails
 * Sums are integer sums: a map depends neither on launch shape ("run_parts", compact or slot order, the kernel that traced the
 * run), nor on how the slots were split into consecutive runs added to one map, nor on the device count.
 * Output layout: bins [plane][selected energy][iy][ix], outside [plane][selected energy]. */
typedef struct {
	int32_t n_planes;             /* 1 .. 64 */
	const double *distances;      /* [n_planes] cm downstream of the exit face, finite, >= 0 */
	double x0, x1, y0, y1;        /* window, cm: finite, x0 < x1, y0 < y1 */
	int32_t nx, ny;               /* bins, >= 1; n_planes * n_selected * nx * ny <= 2^27 */
	int32_t n_energies;           /* selected energies: 0 = all, in order */
	const int32_t *energies;      /* [n_energies] distinct indices into the problem's energies */
	int32_t regime;               /* 0 automatic (= 2, measured: pc_spot.h); 1 LDS tiles, 2 energies across lanes */
} pc_hip_spot_spec;
typedef struct pc_hip_spot pc_hip_spot;
/* PC_HIP_ERR_INVALID with a message unless the spec is valid for a problem of n_energies energies (no device is touched) */
POLYCAP_EXTERN int pc_hip_spot_validate(const pc_hip_spot_spec *spec, size_t n_energies);
/* An empty map on the context's device (the context must outlive it).  The group variant keeps one map per member; reading it
 * sums the members' maps exactly on the host. */
POLYCAP_EXTERN int pc_hip_spot_create(pc_hip_ctx *ctx, const pc_hip_spot_spec *spec, pc_hip_spot **spot);
POLYCAP_EXTERN int pc_hip_group_spot_create(pc_hip_group *group, const pc_hip_spot_spec *spec, pc_hip_spot **spot);
POLYCAP_EXTERN void pc_hip_spot_destroy(pc_hip_spot *spot);
/* Adds the entries of the last run: kind 0 = exit photons (a run that kept images), 1 = extleak, 2 = intleak events (a leak_calc
 * source run).  Enqueued on the context's stream behind the run, so pc_hip_transmission_wait orders it; leak kinds wait for the
 * run first (its events are ordered when it is waited for).  Anything else is PC_HIP_ERR_INVALID. */
POLYCAP_EXTERN int pc_hip_spot_add(pc_hip_spot *spot, int kind);
/* bins [n_planes * n_selected * ny * nx], outside [n_planes * n_selected], *n_entries (any may be NULL); waits for the adds */
POLYCAP_EXTERN int pc_hip_spot_read(pc_hip_spot *spot, uint64_t *bins, uint64_t *outside, int64_t *n_entries);
POLYCAP_EXTERN int pc_hip_spot_reset(pc_hip_spot *spot);
/* dims = {n_planes, n_selected, ny, nx}; *wide (optional) = 1 when the map accumulates with energies across lanes, 0 in LDS tiles */
POLYCAP_EXTERN int pc_hip_spot_info(const pc_hip_spot *spot, int32_t dims[4], int *wide);
/* ---- exit-beam moments: the exact second-moment ("sigma") matrix of the entries of the last run at the optic's exit face, per
 * energy, accumulated on the device in exact integers from what the run left there (pc_beam.h).  From it follow, in closed form
 * and with no planes or window, the centroid, the RMS size at any distance d behind the exit face, the waist (focal) distance and
 * size, and the divergence.  RMS values include the halo tails by definition; spot maps remain the tool for the profile's shape.
 *
 * The contract (IEEE fp64, evaluated in the order written, no contraction):
 *   entries    those pc_hip_spot_add reads: exit photons (kind 0), extleak (1) and intleak (2) events of a leak_calc run
 *   per entry  with position (x, y, z), direction (dx, dy, dz) and weights w[e], on the exit face ze = z[nmax]:
 *              exit photons: dz = sqrt((1 - dx*dx) - dy*dy); leak events: the stored dz
 *              t = (ze - z) / dz,  xe = x + dx*t,  ye = y + dy*t,  sx = dx / dz,  sy = dy / dz
 *              X = rne(xe * 2^24), Y = rne(ye * 2^24), U = rne(sx * 2^24), V = rne(sy * 2^24) as int64 (rne: round half even)
 *              W = round_half_even(w[e] * 2^32) as uint64, 0 for w <= 0 and NaN (the spot maps' q(w))
 *              in range when dz > 0 and |X|, |Y|, |U|, |V| < 2^31 (|position| < 128 cm, |slope| < 128); anything else, NaN
 *              included, adds its W to the (kind, energy) pair's outside counter
 *   sums       per (kind, energy), over the entries in range, 15 signed 128-bit two's-complement sums as (lo, hi) uint64 pairs:
 *              W, WX, WY, WU, WV, WXX, WXY, WXU, WXV, WYY, WYU, WYV, WUU, WUV, WVV (in this order); every term is below 2^94
 *   entries    the sums of one kind take at most 2^32 - 1 entries over all adds (then none can wrap); an add past that fails
 * Sums are integer sums: they depend neither on launch shape ("run_parts", compact or slot order, the kernel that traced the run),
 * nor on how the slots were split into consecutive runs added to one set of sums, nor on the device count.
 *
 * Derived parameters (pc_hip_beam_params, host only), per energy from its 15 sums S, S_a, S_ab (a, b in X, Y, U, V):
 *   N_ab = S*S_ab - S_a*S_b exactly (192 bits suffice); every integer is converted to the nearest double (ties to even) once
 *   s = dbl(S);  weight = s * 2^-32;  mean_a = (dbl(S_a) / s) * 2^-24;  C_ab = (dbl(N_ab) / (s*s)) * 2^-48
 *   waist_x = -C_xx' / C_x'x',  waist_y = -C_yy' / C_y'y',  waist_r = -(C_xx' + C_yy') / (C_x'x' + C_y'y')   (cm behind the exit face)
 *   size_waist_x = sqrt(max(C_xx - (C_xx'*C_xx') / C_x'x', 0)), size_waist_y likewise,
 *   size_waist_r = sqrt(max((C_xx + C_yy) - (B*B) / D, 0)) with B = C_xx' + C_yy', D = C_x'x' + C_y'y'
 *   size_exit_x = sqrt(C_xx), size_exit_y = sqrt(C_yy), size_exit_r = sqrt(C_xx + C_yy), div_x = sqrt(C_x'x'), div_y = sqrt(C_y'y')
 *   a column whose denominator is 0 is NaN; with S == 0 every column but the weight is NaN
 * Columns of a row, in order (cm, rad; x' = dx/dz): weight, x, y, xp, yp, cov_xx, cov_xy, cov_xxp, cov_xyp, cov_yy, cov_yxp,
 * cov_yyp, cov_xpxp, cov_xpyp, cov_ypyp, waist_x, waist_y, waist_r, size_waist_x, size_waist_y, size_waist_r, size_exit_x,
 * size_exit_y, size_exit_r, div_x, div_y (pc_hip_beam_columns).
 * At a distance d (pc_hip_beam_at): x(d) = x + d*xp, y(d) = y + d*yp, vx = (C_xx + (2*d)*C_xx') + (d*d)*C_x'x', vy likewise,
 * size_x = sqrt(max(vx, 0)), size_y = sqrt(max(vy, 0)), size_r = sqrt(max(vx, 0) + max(vy, 0)); NaN when S == 0. */
typedef struct pc_hip_beam pc_hip_beam;
#define PC_HIP_BEAM_NSUMS 15
#define PC_HIP_BEAM_NCOLS 26
#define PC_HIP_BEAM_NAT 5
/* Empty sums for all three kinds on the context's device (the context must outlive them).  The group variant keeps one set per
 * member; reading it adds the members' sums exactly on the host. */
POLYCAP_EXTERN int pc_hip_beam_create(pc_hip_ctx *ctx, pc_hip_beam **beam);
POLYCAP_EXTERN int pc_hip_group_beam_create(pc_hip_group *group, pc_hip_beam **beam);
POLYCAP_EXTERN void pc_hip_beam_destroy(pc_hip_beam *beam);
/* Adds the entries of kind 0, 1 or 2 of the last run, as pc_hip_spot_add: enqueued on the context's stream behind the run; leak kinds
 * wait for the run first (its events are ordered when it is waited for).  Anything else is PC_HIP_ERR_INVALID. */
POLYCAP_EXTERN int pc_hip_beam_add(pc_hip_beam *beam, int kind);
/* sums [3][n_energies][15][2], outside [3][n_energies], n_entries [3] (any may be NULL); waits for the adds */
POLYCAP_EXTERN int pc_hip_beam_read(pc_hip_beam *beam, uint64_t *sums, uint64_t *outside, int64_t *n_entries);
POLYCAP_EXTERN int pc_hip_beam_reset(pc_hip_beam *beam);
POLYCAP_EXTERN int pc_hip_beam_info(const pc_hip_beam *beam, int *n_energies);
/* host only: params [n_energies][26] from sums [n_energies][15][2] of one kind */
POLYCAP_EXTERN void pc_hip_beam_params(size_t n_energies, const uint64_t *sums, double *params);
/* host only: out [n_energies][n_distances][5] = {x, y, size_x, size_y, size_r} at the distances (cm behind the exit face) */
POLYCAP_EXTERN void pc_hip_beam_at(size_t n_energies, const uint64_t *sums, size_t n_distances, const double *distances, double *out);
/* the 26 column names of pc_hip_beam_params, comma-separated */
POLYCAP_EXTERN const char *pc_hip_beam_columns(void);
/* ---- histograms: weighted 1-D histograms of per-entry scalar quantities of the last run, one per axis and selected energy,
 * accumulated on the device in exact integers from what the run left there (pc_hist.h): line and radial profiles of the focal
 * spot at any bin width (full width at half maximum, encircled-energy radii), the distributions of reflection count and path
 * length per energy, the z of the leak events, the entrance radii that transmit.  One pass reads every entry once for all axes.
 *
 * The contract (IEEE fp64, evaluated in the order written, no contraction):
 *   entries    those pc_hip_spot_add reads: exit photons (kind 0; the records of a relay into the context count here), extleak (1)
 *              and intleak (2) events of a leak_calc run.  Sums are kept per kind.
 *   per entry  with position (x, y, z), direction (dx, dy, dz) and weights w[e]:
 *              exit photons: dz = sqrt((1 - dx*dx) - dy*dy); leak events: the stored dz
 *   value v    of an axis with quantity Q, distance d, centre (cx, cy); zp = z[nmax] + d, computed once on the host:
 *              X_AT       t = (zp - z) / dz,  v = x + dx*t
 *              Y_AT       v = y + dy*t
 *              R_AT       a = (x + dx*t) - cx,  b = (y + dy*t) - cy,  v = sqrt(a*a + b*b)
 *              SLOPE_X    v = dx / dz;    SLOPE_Y    v = dy / dz;    TAN_THETA  v = sqrt(dx*dx + dy*dy) / dz
 *              N_REFL     v = (double)n: exit photons, the int64 pc_exit_nrefl; leak events, the record's n_refl
 *              D_TRAVEL   v = pc_exit_dtravel (exit photons only)
 *              R_START    v = sqrt(sx*sx + sy*sy) of pc_start_coords (exit photons only)
 *              Z          v = z
 *   bin        f = ((v - lo) / (hi - lo)) * n_bins; inside when 0 <= f < n_bins, bin = floor(f).  Anything else is outside: NaN,
 *              !(dz > 0) for the six quantities that use dz, off the range, D_TRAVEL and R_START on a leak kind
 *   weights    W = round_half_even(w[e] * 2^32) as uint64, 0 for w <= 0 and NaN (the spot maps' q(w)); a bin holds the sum of W
 *              over its entries, and every (kind, axis, energy) has one outside counter for the rest, so that for each of them
 *              sum(bins) + outside == sum over the kind's entries of W, exactly
 *   entries    one kind takes at most 2^32 - 1 entries over all adds (then no uint64 can wrap); an add past that fails
 * Sums are integer sums: they depend neither on launch shape ("run_parts", compact or slot order, records or planes, the kernel that
 * traced the run, the regime), nor on how the slots were split into consecutive runs added to one object, nor on the device count.
 * Output layout: bins [3][n_selected][total_bins] with the axes one after the other (total_bins = sum of n_bins), outside
 * [3][n_axes][n_selected], n_entries [3].
 *
 * Host helpers on the bins of one (kind, axis, energy), c(b) = lo + ((b + 0.5) / n_bins) * (hi - lo) the centre of bin b:
 *   quantile   T = sum(bins) in integers (the inside weight only); NaN when T == 0 or q is not in [0, 1].  target = q * dbl(T);
 *              b = the first non-empty bin with dbl(C_b) >= target, C_b = bins[0] + .. + bins[b] in integers;
 *              frac = (target - dbl(C_b - bins[b])) / dbl(bins[b]);  result = lo + ((b + frac) / n_bins) * (hi - lo)
 *              (hi when no bin qualifies)
 *   fwhm       p = the first bin of maximal count, half = dbl(bins[p]) / 2.0; i = the first bin below p, walking down, with
 *              dbl(bins[i]) < half; j likewise above p.  NaN (also *left, *right) when the histogram is empty or a walk reaches
 *              the end of the axis.  left = c(i) + (c(i+1) - c(i)) * ((half - bins[i]) / (bins[i+1] - bins[i])),
 *              right = c(j) + (c(j-1) - c(j)) * ((half - bins[j]) / (bins[j-1] - bins[j])), counts as doubles; result = right - left */
enum { PC_HIP_HIST_X_AT = 0, PC_HIP_HIST_Y_AT, PC_HIP_HIST_R_AT, PC_HIP_HIST_SLOPE_X, PC_HIP_HIST_SLOPE_Y,
       PC_HIP_HIST_TAN_THETA, PC_HIP_HIST_N_REFL, PC_HIP_HIST_D_TRAVEL, PC_HIP_HIST_R_START, PC_HIP_HIST_Z };
typedef struct {
	int32_t quantity;             /* PC_HIP_HIST_* */
	double d, cx, cy;             /* cm behind the exit face (X_AT, Y_AT, R_AT; 0 elsewhere), centre (R_AT; 0 elsewhere): finite, d >= 0 */
	double lo, hi;                /* range: finite, lo < hi */
	int32_t n_bins;               /* >= 1 */
} pc_hip_hist_axis;
typedef struct {
	int32_t n_axes;               /* 1 .. 16 */
	const pc_hip_hist_axis *axes;
	int32_t n_energies;           /* selected energies: 0 = all, in order; (sum of n_bins) * n_selected <= 2^24 */
	const int32_t *energies;      /* [n_energies] distinct indices into the problem's energies */
	int32_t regime;               /* 0 automatic (pc_hist.h); 1 workgroup-private LDS histograms, 2 energies across lanes */
} pc_hip_hist_spec;
typedef struct pc_hip_hist pc_hip_hist;
/* PC_HIP_ERR_INVALID with a message that names the field unless the spec is valid for a problem of n_energies energies (no device
 * is touched) */
POLYCAP_EXTERN int pc_hip_hist_validate(const pc_hip_hist_spec *spec, size_t n_energies);
/* Empty histograms for all three kinds on the context's device (the context must outlive them).  The group variant keeps one set
 * per member; reading it adds the members' sums exactly on the host. */
POLYCAP_EXTERN int pc_hip_hist_create(pc_hip_ctx *ctx, const pc_hip_hist_spec *spec, pc_hip_hist **hist);
POLYCAP_EXTERN int pc_hip_group_hist_create(pc_hip_group *group, const pc_hip_hist_spec *spec, pc_hip_hist **hist);
POLYCAP_EXTERN void pc_hip_hist_destroy(pc_hip_hist *hist);
/* Adds the entries of kind 0, 1 or 2 of the last run, as pc_hip_spot_add: enqueued on the context's stream behind the run; leak kinds
 * wait for the run first (its events are ordered when it is waited for).  Anything else is PC_HIP_ERR_INVALID. */
POLYCAP_EXTERN int pc_hip_hist_add(pc_hip_hist *hist, int kind);
/* bins [3][n_selected][total_bins], outside [3][n_axes][n_selected], n_entries [3] (any may be NULL); waits for the adds */
POLYCAP_EXTERN int pc_hip_hist_read(pc_hip_hist *hist, uint64_t *bins, uint64_t *outside, int64_t *n_entries);
POLYCAP_EXTERN int pc_hip_hist_reset(pc_hip_hist *hist);
/* dims = {n_axes, n_selected, total_bins}; offsets [n_axes + 1] (optional): axis a has the bins [offsets[a], offsets[a + 1]) of an
 * energy's row; *regime (optional) = the regime in use, 1 or 2 */
POLYCAP_EXTERN int pc_hip_hist_info(const pc_hip_hist *hist, int32_t dims[3], int32_t *offsets, int *regime);
/* host only, on bins [n_bins] of one (kind, axis, energy): the value below which the fraction q of the inside weight lies (outside,
 * that histogram's outside counter, is not used: the quantile is that of what the range holds) */
POLYCAP_EXTERN double pc_hip_hist_quantile(int32_t n_bins, double lo, double hi, const uint64_t *bins, uint64_t outside, double q);
/* host only: the full width at half maximum; *left and *right (optional) = where the profile crosses half its maximum */
POLYCAP_EXTERN double pc_hip_hist_fwhm(int32_t n_bins, double lo, double hi, const uint64_t *bins, double *left, double *right);
/* ---- joint histograms: weighted 2-D histograms of two per-entry scalar quantities of the last run, one per pair of axes (u, v)
 * and selected energy, accumulated on the device in exact integers from what the run left there (pc_joint.h): phase-space diagrams
 * (x against dx/dz at the exit face or at any distance), the transmission map of the entrance face (start x against start y), the
 * reflection count against the entrance radius, the z of a leak event against its reflection count.  One pass reads every entry
 * once for all pairs.  A spot map of one plane is the pair (X_AT d, Y_AT d) over its window.
 *
 * The contract (IEEE fp64, evaluated in the order written, no contraction):
 *   entries    those pc_hip_hist_add reads: exit photons (kind 0; the records of a relay into the context count here), extleak (1)
 *              and intleak (2) events of a leak_calc run.  Sums are kept per kind.
 *   axes       an axis is a pc_hip_hist_axis: the fields, their validation and the value v of the histogram contract above.  A joint
 *              axis may also have one of two quantities a histogram cannot (pc_hip_hist_validate refuses them):
 *              START_X    v = pc_start_coords[0] (exit photons only);    START_Y    v = pc_start_coords[1] (exit photons only)
 *   bin        per axis as in the histogram contract: f = ((v - lo) / (hi - lo)) * n_bins, inside when 0 <= f < n_bins, bin =
 *              floor(f).  An entry is inside a pair when both of its axes are inside, and its cell is iv * nu + iu.  Anything else
 *              is outside: NaN, !(dz > 0) for a quantity that uses dz, D_TRAVEL, R_START, START_X or START_Y on a leak kind, a value
 *              off either range
 *   weights    W = round_half_even(w[e] * 2^32) as uint64, 0 for w <= 0 and NaN (the spot maps' q(w)); a cell holds the sum of W over
 *              its entries, and every (kind, pair, energy) has one outside counter for the rest, so that for each of them
 *              sum(cells) + outside == sum over the kind's entries of W, exactly
 *   limits     1 .. 8 pairs; (sum over the pairs of nu * nv) * n_selected <= 2^26; one kind takes at most 2^32 - 1 entries over all
 *              adds (then no uint64 can wrap); an add past that fails
 * Sums are integer sums: they depend neither on launch shape ("run_parts", compact or slot order, records or planes, the kernel that
 * traced the run, the regime), nor on how the slots were split into consecutive runs added to one object, nor on the device count.
 * Output layout: cells [3][n_selected][total_cells] with the pairs one after the other, each [iv][iu] (total_cells = sum of
 * nu * nv), outside [3][n_pairs][n_selected], n_entries [3]. */
enum { PC_HIP_JOINT_START_X = 10, PC_HIP_JOINT_START_Y = 11 };
typedef struct { pc_hip_hist_axis u, v; } pc_hip_joint_pair;
typedef struct {
	int32_t n_pairs;              /* 1 .. 8 */
	const pc_hip_joint_pair *pairs;
	int32_t n_energies;           /* selected energies: 0 = all, in order; (sum of nu * nv) * n_selected <= 2^26 */
	const int32_t *energies;      /* [n_energies] distinct indices into the problem's energies */
	int32_t regime;               /* 0 automatic (pc_joint.h); 1 workgroup-private LDS tiles, 2 energies across lanes */
} pc_hip_joint_spec;
typedef struct pc_hip_joint pc_hip_joint;
/* PC_HIP_ERR_INVALID with a message that names the pair, the axis (u or v) and the field unless the spec is valid for a problem of
 * n_energies energies (no device is touched) */
POLYCAP_EXTERN int pc_hip_joint_validate(const pc_hip_joint_spec *spec, size_t n_energies);
/* Empty joint histograms for all three kinds on the context's device (the context must outlive them).  The group variant keeps one
 * set per member; reading it adds the members' sums exactly on the host. */
POLYCAP_EXTERN int pc_hip_joint_create(pc_hip_ctx *ctx, const pc_hip_joint_spec *spec, pc_hip_joint **joint);
POLYCAP_EXTERN int pc_hip_group_joint_create(pc_hip_group *group, const pc_hip_joint_spec *spec, pc_hip_joint **joint);
POLYCAP_EXTERN void pc_hip_joint_destroy(pc_hip_joint *joint);
/* Adds the entries of kind 0, 1 or 2 of the last run, as pc_hip_hist_add.  Anything else is PC_HIP_ERR_INVALID. */
POLYCAP_EXTERN int pc_hip_joint_add(pc_hip_joint *joint, int kind);
/* cells [3][n_selected][total_cells], outside [3][n_pairs][n_selected], n_entries [3] (any may be NULL); waits for the adds */
POLYCAP_EXTERN int pc_hip_joint_read(pc_hip_joint *joint, uint64_t *cells, uint64_t *outside, int64_t *n_entries);
POLYCAP_EXTERN int pc_hip_joint_reset(pc_hip_joint *joint);
/* dims = {n_pairs, n_selected, total_cells}; offsets [n_pairs + 1] (optional): pair p has the cells [offsets[p], offsets[p + 1]) of
 * an energy's row; *regime (optional) = the regime in use, 1 or 2 */
POLYCAP_EXTERN int pc_hip_joint_info(const pc_hip_joint *joint, int32_t dims[3], int32_t *offsets, int *regime);
/* host only, on cells [nv][nu] of one (kind, pair, energy): the exact sums over v (which = 0: out [nu], the histogram of u of what
 * both ranges hold) or over u (which = 1: out [nv]) */
POLYCAP_EXTERN int pc_hip_joint_marginal(int32_t nu, int32_t nv, const uint64_t *cells, int which, uint64_t *out);
/* host only: a value of POLYCAP_JOINT (below) into pairs [8], *n_pairs, energies [n_energies] and *n_selected (0 = all), checked
 * with pc_hip_joint_validate for a problem of n_energies energies.  PC_HIP_ERR_INVALID with the reason (it names the item) in
 * why [why_len] otherwise. */
POLYCAP_EXTERN int pc_hip_joint_parse(const char *value, size_t n_energies, pc_hip_joint_pair *pairs, int32_t *n_pairs,
	int32_t *energies, int32_t *n_selected, char *why, size_t why_len);
/* ---- selections: cuts on per-entry quantities, evaluated once per entry on the device (pc_select.h), through which any of the four
 * tallies above can be filled: the beam moments of the core without the halo tails, a spot map of the photons of few reflections, the
 * flux through a pinhole in the focal plane, the phase space a downstream aperture accepts.
 *
 * The contract:
 *   cut        a pc_hip_hist_axis and a flag negate (0 or 1).  The quantity may be any histogram quantity or START_X / START_Y of the
 *              joint histograms; n_bins must be 1; the other fields are validated as a histogram axis is.  The entry's value v is the
 *              histogram contract's, and the entry is inside exactly when it falls into bin 0 of that one-bin axis.  So NaN,
 *              !(dz > 0) for a quantity that uses dz, a quantity the kind does not have (D_TRAVEL, R_START, START_X, START_Y on a leak
 *              kind) and a value off [lo, hi) are all not inside.  pass_k = inside XOR negate
 *   selection  1 .. 8 cuts; an entry passes when every cut passes
 *   apply      evaluates the cuts on the entries of one kind of the last run (those pc_hip_hist_add reads; the records of a relay into
 *              the context are kind 0) and leaves one mask byte per entry on every member's device, with the exact totals n_pass,
 *              n_seen and, per energy, passed_w = the sum of W over the passing entries and rejected_w = that over the others, W =
 *              round_half_even(w[e] * 2^32) as uint64 (the spot maps' q(w)): passed_w + rejected_w is the sum over all entries,
 *              exactly.  passed_w / (passed_w + rejected_w) is the transmission of the selection, a pinhole's for a cut on R_AT
 *   gated add  pc_hip_{spot,beam,hist,joint}_add_selected is the plain add for which an entry whose mask byte is 0 does not exist
 *              (unlike the plain add it waits for the apply on the context's stream, to learn n_pass, before it enqueues):
 *              it adds to no cell, no sum and no outside counter, n_entries grows by n_pass, and the cap of 2^32 - 1 entries counts
 *              n_pass.  For histograms and joint histograms sum(bins) + outside == passed_w[e] per (kind, axis or pair, energy),
 *              exactly.  Gated and plain adds may be mixed into one tally
 *   refusals   PC_HIP_ERR_INVALID before anything is launched, every object unchanged: the selection and the tally have different
 *              owners (another context, another group, a context against a group); the selection was not applied for that kind; the
 *              mask is stale -- the entries of the kind were replaced since (a source run, a leak run, a relay into the context, an
 *              explicit launch; a scan replaces nothing)
 *   limits     a kind of more than 2^32 - 1 entries cannot be applied (the uint64 sums could wrap)
 * Masks and totals are integers and depend on the set of entries only: not on the layout of the exit photons (records, planes in slot
 * order, compact planes), "run_parts", the kernel that traced the run, how the slots were split into runs, or the device count. */
typedef struct {
	pc_hip_hist_axis axis;        /* n_bins = 1 */
	int32_t negate;               /* 0: pass inside; 1: pass outside */
} pc_hip_select_cut;
typedef struct {
	int32_t n_cuts;               /* 1 .. 8 */
	const pc_hip_select_cut *cuts;
} pc_hip_select_spec;
typedef struct pc_hip_select pc_hip_select;
/* PC_HIP_ERR_INVALID with a message that names the cut and the field unless the spec is valid (no device is touched) */
POLYCAP_EXTERN int pc_hip_select_validate(const pc_hip_select_spec *spec);
/* A selection on the context's device (the context must outlive it); the group variant keeps one mask per member */
POLYCAP_EXTERN int pc_hip_select_create(pc_hip_ctx *ctx, const pc_hip_select_spec *spec, pc_hip_select **select);
POLYCAP_EXTERN int pc_hip_group_select_create(pc_hip_group *group, const pc_hip_select_spec *spec, pc_hip_select **select);
POLYCAP_EXTERN void pc_hip_select_destroy(pc_hip_select *select);
/* Evaluates the cuts on the entries of kind 0, 1 or 2 of the last run: enqueued on the context's stream behind the run, as
 * pc_hip_hist_add is (leak kinds wait for the run first).  A kind applied before is applied anew. */
POLYCAP_EXTERN int pc_hip_select_apply(pc_hip_select *select, int kind);
/* n_pass [3], n_seen [3], passed_w [3][n_energies], rejected_w [3][n_energies] (any may be NULL; all energies of the problem); zeros
 * for a kind that was not applied; waits for the applies */
POLYCAP_EXTERN int pc_hip_select_read(pc_hip_select *select, int64_t *n_pass, int64_t *n_seen, uint64_t *passed_w, uint64_t *rejected_w);
/* *n_cuts, *n_energies (either may be NULL) and cuts [n_cuts] (optional) */
POLYCAP_EXTERN int pc_hip_select_info(const pc_hip_select *select, int32_t *n_cuts, int32_t *n_energies, pc_hip_select_cut *cuts);
/* The adds of the four tallies through a selection applied for that kind (the contract above) */
POLYCAP_EXTERN int pc_hip_spot_add_selected(pc_hip_spot *spot, int kind, pc_hip_select *select);
POLYCAP_EXTERN int pc_hip_beam_add_selected(pc_hip_beam *beam, int kind, pc_hip_select *select);
POLYCAP_EXTERN int pc_hip_hist_add_selected(pc_hip_hist *hist, int kind, pc_hip_select *select);
POLYCAP_EXTERN int pc_hip_joint_add_selected(pc_hip_joint *joint, int kind, pc_hip_select *select);
/* host only: a list of cuts in the axis grammar of POLYCAP_HIST without bins, a cut ending in ",not" being negated, e.g.
 * "axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not", into cuts [8] and *n_cuts, checked with pc_hip_select_validate.
 * PC_HIP_ERR_INVALID with the reason (it names the item) in why [why_len] otherwise. */
POLYCAP_EXTERN int pc_hip_select_parse(const char *value, pc_hip_select_cut *cuts, int32_t *n_cuts, char *why, size_t why_len);
/* ---- gathers: the per-entry data of the entries a selection keeps, compacted in order on the device (pc_gather.h) and copied to the
 * host without the rest of the run: the halo photons outside a radius, the photons of many reflections, what a pinhole accepts as the
 * input of a downstream code, the leak events of one z range.
 *
 * The contract:
 *   numbering  the passing entries of a kind are numbered 0 .. n_pass - 1 in the order of their positions in what pc_hip_select_apply
 *              read.  Kind 0: the positions of the image store -- slot order by default, the order of completion for compact stores,
 *              the records of a relay into the context; kinds 1 and 2: the ordered leak event lists.  For a group the members'
 *              entries come one after the other in member order, and a position is the global one: the member's local position plus
 *              the entry counts of the members before it, the numbering of pc_hip_group_images and pc_hip_group_leak_events
 *   result     the passing entries numbered [first, first + count) are copied to the host
 *   records    kind 0: [count][PC_HIP_N_PLANES + n_energies], row k bit for bit the row pc_hip_transmission_records returns for that
 *              position, the reflection count as int64 bits; where _records is not available ("plane_images", compact stores) the
 *              same row is assembled from the planes.  Kinds 1 and 2: [count][PC_HIP_LEAK_HDR + n_energies], the rows of
 *              pc_hip_leak_events for those events.  Rows are copied as 64-bit patterns, never through a floating-point operation
 *   positions  optional: [count] positions as defined above, strictly increasing
 *   count 0    valid, touches nothing; records and positions may then be NULL
 *   refusals   PC_HIP_ERR_INVALID with a message that names the function and the field, nothing launched, the selection and what it
 *              has cached unchanged: select NULL; kind outside 0 .. 2; first < 0; count < 0; records NULL with count > 0; the
 *              selection was not applied for that kind; the mask is stale (the rule and the wording of the gated adds); first + count
 *              greater than n_pass of that kind
 *   blocking   the call returns when the data are in the caller's memory; on every member's stream it is ordered behind the apply
 * The list of the passing positions (uint32 [n_pass] per member and kind; a kind takes at most 2^32 - 1 entries) is built by the first
 * gather after an apply and kept until that kind is applied again; a compaction that finds another count than the apply is
 * PC_HIP_ERR_RUNTIME.  Two options of pc_hip_set_option / pc_hip_group_set_option, neither of which changes a result:
 *   "gather_tile"       entries per tile of the compaction: a multiple of 64 in 64 .. 65536, 0 (default) = automatic (4096)
 *   "gather_chunk_rows" rows per chunk of the device staging buffer, each chunk one copy to the host: 0 (default) = as many rows as
 *                       fit in 128 MiB, at least 1
 * Both exist so that tests reach many tiles and many chunks at small sizes. */
POLYCAP_EXTERN int pc_hip_select_gather(pc_hip_select *select, int kind, int64_t first, int64_t count, double *records, int64_t *positions);
/* ---- draws: an unweighted sample of the entries a selection keeps (pc_draw.h).  A sample-side Monte Carlo, a detector model or a
 * second run started from explicit photons wants N photons of equal weight, drawn in proportion to the transmitted weight at one
 * energy; a gather returns weighted rows.  Systematic resampling in exact integers, on the device, of what the run left there.
 *
 * The contract:
 *   inputs     a selection applied for `kind`; an energy index `energy` of the problem; a sample size n_draw = N, 1 <= N <= 2^31 - 1;
 *              a phase r (any uint32)
 *   entries    the entries of the kind in the position order of pc_hip_select_gather (the members of a group one after the other,
 *              positions global).  Entry i has V_i = W_i[energy] = round_half_even(w[energy] * 2^32) (the spot maps' q(w)) where its
 *              mask byte is set and 0 otherwise; C_i = V_0 + ... + V_i; T = C_{n-1}, which is passed_w[kind][energy] of
 *              pc_hip_select_read exactly
 *   draw k     0 <= k < N: t_k = floor((k * 2^32 + r) * T / (N * 2^32)), a 128-bit product, 0 <= t_k < T; pos_k = the smallest i with
 *              C_i > t_k.  Positions do not decrease with k; entry i is drawn floor(N V_i / T) or ceil(N V_i / T) times; an entry with
 *              V_i = 0 (one the selection rejects, one without weight at that energy) is never drawn
 *   result     the draws [first, first + count) are copied to the host
 *   records    [count][PC_HIP_N_PLANES + n_energies] for kind 0, [count][PC_HIP_LEAK_HDR + n_energies] for the leak kinds: row k - first
 *              bit for bit the row pc_hip_select_gather / pc_hip_transmission_records / pc_hip_leak_events has at pos_k, copied as
 *              64-bit patterns
 *   positions  optional: [count] pos_k
 *   total      optional: *total = T, so that the caller knows that every draw stands for T * 2^-32 / N of weight per started photon;
 *              it is set whenever the arguments pass, count 0 included
 *   count 0    valid, touches nothing beyond *total; records and positions may then be NULL
 *   refusals   PC_HIP_ERR_INVALID with a message that names the function and the field, nothing launched, the selection and what it
 *              has cached unchanged: the refusals of pc_hip_select_gather (select NULL; kind; first < 0; count < 0; records NULL with
 *              count > 0; not applied; stale mask); energy outside the problem; n_draw outside 1 .. 2^31 - 1; first + count > n_draw;
 *              T == 0 (no weight to draw from)
 *   cost       device memory and time grow with the entries and with count, never with N: a window of 100 draws at the end of
 *              N = 2^31 - 1 costs what it costs at the start
 *   blocking   as pc_hip_select_gather
 * The result depends on the entries, their order, the mask, energy, N and r only: not on "gather_tile" or "gather_chunk_rows" (the two
 * options of the gathers, which the draws share), not on how a window is split into calls, on "run_parts", or on records against
 * slot-ordered planes.  The sums of V over the tiles and their scan are kept per member for one (kind, energy, tile) until that kind
 * is applied again; tile sums that do not add up to the apply's passed_w are PC_HIP_ERR_RUNTIME. */
POLYCAP_EXTERN int pc_hip_select_draw(pc_hip_select *select, int kind, int32_t energy, int64_t n_draw, uint32_t phase, int64_t first,
	int64_t count, double *records, int64_t *positions, uint64_t *total);
/* ---- standard errors of the tallies: a second exact sum per cell, of the squared weights, kept in the same pass as the first, so
 * that every bin of a spot map, a histogram or a joint histogram and the transmission of a selection carry their Monte Carlo error.
 *
 * The contract:
 *   entry      per entry and energy W = round_half_even(w[e] * 2^32) as today (the spot maps' q(w), W <= 2^32).  Its square is the
 *              integer product W*W <= 2^64 in units of 2^-64 -- not a second quantisation of w*w, which at a quantum of 2^-32 would
 *              round the squares of weights below about 1e-5 to nothing -- as a (lo, hi) pair of uint64: lo = W*W mod 2^64, hi = the
 *              upper 64 bits of the product (1 for W = 2^32 only)
 *   cell       wherever the object keeps a weight sum S -- a spot-map bin, a histogram bin, a joint cell, every outside counter --
 *              it also keeps S2 = the sum of W*W over the cell's entries as one (lo, hi) pair.  With the cap of 2^32 - 1 entries
 *              S2 < 2^97 cannot wrap.  For every map, axis or pair: sum(S2 of the cells) + S2 of outside == the sum over the entries
 *              of W*W, exactly.  A gated add obeys the selection contract for S2 as for S: an entry the mask rejects adds to neither
 *   selection  also keeps passed_w2 and rejected_w2 [3][n_energies] as (lo, hi) pairs: the sums of W*W over the passing and over the
 *              rejected entries; gated sum(S2) + outside S2 == passed_w2[e] per (kind, axis or pair, energy)
 * S2 is an integer sum and depends on the set of entries only: not on the layout of the exit photons, "run_parts", the kernel that
 * traced the run, the regime of the tally, how the slots were split into runs, or the device count.
 *
 * pc_hip_{spot,hist,joint}_track_squares turns the tracking on and allocates the zeroed pairs on every member.  Allowed only while the
 * object holds no entries (n_entries all zero: before the first add, or after _reset); PC_HIP_ERR_INVALID and the object unchanged
 * otherwise.  From then on every add, plain or _add_selected, fills S and S2 in one pass that reads each entry once; an object that
 * does not track squares adds exactly as before.  _reset zeroes the pairs and keeps the tracking.
 * pc_hip_{spot,hist,joint}_read_squares: the shapes of the _read calls with a trailing [2] (either pointer may be NULL); they wait
 * for the adds and sum the members of a group with carry; PC_HIP_ERR_INVALID on an object that does not track squares.
 * pc_hip_select_track_squares: refused (PC_HIP_ERR_INVALID, nothing changed) once any kind has been applied.
 * pc_hip_select_read_squares: passed_w2, rejected_w2 [3][n_energies][2] (either may be NULL), zeros for a kind not applied. */
POLYCAP_EXTERN int pc_hip_spot_track_squares(pc_hip_spot *spot);
POLYCAP_EXTERN int pc_hip_spot_read_squares(pc_hip_spot *spot, uint64_t *bins_sq, uint64_t *outside_sq);
POLYCAP_EXTERN int pc_hip_hist_track_squares(pc_hip_hist *hist);
POLYCAP_EXTERN int pc_hip_hist_read_squares(pc_hip_hist *hist, uint64_t *bins_sq, uint64_t *outside_sq);
POLYCAP_EXTERN int pc_hip_joint_track_squares(pc_hip_joint *joint);
POLYCAP_EXTERN int pc_hip_joint_read_squares(pc_hip_joint *joint, uint64_t *cells_sq, uint64_t *outside_sq);
POLYCAP_EXTERN int pc_hip_select_track_squares(pc_hip_select *select);
POLYCAP_EXTERN int pc_hip_select_read_squares(pc_hip_select *select, uint64_t *passed_w2, uint64_t *rejected_w2);
/* host only: the standard error of n_cells cells in weight per started photon, pc_hip_efficiency_stderr's estimator.  sums [n_cells]
 * = S, squares [n_cells][2] = S2, N = n_started = counters 0 + 1 + 2 of the run or runs that were added (the caller's).  Per cell, in
 * long double: m = S 2^-32 / N, q = S2 2^-64 / N, out = sqrt(max(q - m*m, 0) / (N - 1)); NaN for N < 2.  The events of a leak kind
 * that come from one photon are treated as independent entries: each adds its own W*W, so where one photon leaves several events in
 * one cell the error is underestimated by their covariance. */
POLYCAP_EXTERN void pc_hip_tally_stderr(size_t n_cells, const uint64_t *sums, const uint64_t *squares, int64_t n_started, double *out);
/* host only: the transmission of a selection per energy and its error from one kind's rows of pc_hip_select_read and _read_squares:
 * P = passed_w 2^-32, R = rejected_w 2^-32, P2 = passed_w2 2^-64, R2 = rejected_w2 2^-64 ([n_energies] and [n_energies][2]), in long
 * double: T = P / (P + R), T_err = sqrt(R*R*P2 + P*P*R2) / ((P + R)*(P + R)) -- the delta method on two independent Poisson-thinned
 * sums; both NaN when P + R == 0.  T or T_err may be NULL. */
POLYCAP_EXTERN void pc_hip_select_transmission(size_t n_energies, const uint64_t *passed_w, const uint64_t *rejected_w,
	const uint64_t *passed_w2, const uint64_t *rejected_w2, double *T, double *T_err);
/* ---- scans: transmission as a function of where the source sits (alignment curves, the input focal spot, the depth response of
 * a focusing optic) in one launch, with exact totals per point.
 *
 * A scan has P = n_points points, each a source position (d_source, src_shiftx, src_shifty); every other source field (size,
 * divergence, polarisation) and the optic are the context's problem's.  Every point gets n_per_point slots and the scan one
 * max_attempts (0 is taken as 1).  Slot j of point k -- flat index i = k*n_per_point + j -- is traced exactly like slot slot0 + j
 * of a source run: its attempts use the Philox stream (seed, slot0 + j, attempt), and it stops at the first transmitted photon
 * or after max_attempts attempts.  The guarantee: for every point k the scan's counters[6], sumw_fixed and (option
 * "weight_squares") sumw2_fixed are bit-identical to those of pc_hip_transmission_run(ctx_k, seed, slot0, n_per_point,
 * max_attempts, 0) -- read whatever pc_hip_transmission_totals returns -- where ctx_k is a context whose problem equals the
 * scan's but for point k's three fields.  Consequences:
 *   - common random numbers: all points use the same streams (as separate runs with one seed do), so neighbouring points are
 *     positively correlated and curves come out smooth; each point's standard error on its own is still right;
 *   - slots that exhaust max_attempts are no error in a scan: counters[4] reports them per point.  With max_attempts = 1 a point
 *     is a budget of exactly n_per_point started photons.  sum(w) / (counters[0] + counters[1] + counters[2]) stays a
 *     consistent estimator of the efficiency under this stopping rule (Wald's identity), so the efficiency and standard-error
 *     formulas apply row by row (pc_hip_scan_efficiencies);
 *   - a point where nothing entered a capillary has efficiency 0 (pc_hip_efficiencies would divide by zero there).
 * A scan is not a run: the last run's totals, moments, images, records, slot ids, leak events and what pc_hip_spot_add reads
 * stay as they were.  The scan is enqueued on the context's stream behind every launch of the last run (also when that run was
 * cut into parts on two streams) and keeps buffers of its own; a scan call waits for the context's previous scan first.
 * Scans with more than 8 energies use the immediate weight sweep by default: with roughness their weights are those of a run
 * with option "batch_reflections" 0, which differ from a default run's in the last bits (~4e-14), and the sweep is slower than
 * the logging kernel.  Option "scan_log" = 1 (pc_hip_set_option, pc_hip_group_set_option; default 0, other values are refused)
 * sends a scan through the logging kernel when it can log -- the conditions are a source run's: more than 8 energies and at
 * least "log_min_energies", "batch_reflections" and "lds_ec" on, a profile of at most 1024 points, every energy valid, a log
 * stage that fits -- with a source run's log capacity, so that every point equals a run with default options bit for bit,
 * roughness included.  A scan that cannot log keeps the lane kernel; pc_hip_scan_last_kernel says which one ran.
 * Invalid arguments give PC_HIP_ERR_INVALID with a message that names the function and the field. */
typedef struct { double d_source, src_shiftx, src_shifty; } pc_hip_scan_point;
/* host only: d_source > 0 and finite, finite shifts, n_points >= 1, n_per_point >= 1, n_points * n_per_point fits in int64 */
POLYCAP_EXTERN int pc_hip_scan_validate(const pc_hip_scan_point *points, int64_t n_points, int64_t n_per_point);
/* traces the flat indices [first, first + count) of the scan (1 <= count; slot0 >= 0 and slot0 + n_per_point fits in int64);
 * several calls over ranges that cut the flat range into pieces add up to the whole scan, exactly */
POLYCAP_EXTERN int pc_hip_scan_run(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, const pc_hip_scan_point *points, int64_t n_points,
	int64_t n_per_point, int64_t first, int64_t count, uint32_t max_attempts);
/* waits for the last scan call; *kernel_ms (optional) = its kernel time */
POLYCAP_EXTERN int pc_hip_scan_wait(pc_hip_ctx *ctx, float *kernel_ms);
/* waits; totals of the last scan call, per point: counters [P][6] as pc_hip_transmission_totals, sumw_fixed [P][2*n_energies] and
 * sumw2_fixed [P][2*n_energies] (the scan must have been made with option "weight_squares") as (lo, hi) pairs; any may be NULL.
 * Points outside the call's range have zero totals. */
POLYCAP_EXTERN int pc_hip_scan_totals(pc_hip_ctx *ctx, int64_t *counters, uint64_t *sumw_fixed, uint64_t *sumw2_fixed);
/* host only, row by row: efficiencies [P][n_energies] as pc_hip_efficiencies, 0 where counters[0] + counters[2] == 0; with
 * sumw2_fixed and stderr_ (both or neither) the standard errors of pc_hip_efficiency_stderr */
POLYCAP_EXTERN void pc_hip_scan_efficiencies(size_t n_energies, int64_t n_points, const int64_t *counters, const uint64_t *sumw_fixed,
	const uint64_t *sumw2_fixed, double *efficiencies, double *stderr_);
/* the flat range [0, n_points * n_per_point) split over the group's members in contiguous pieces; the totals are the members'
 * added exactly on the host (the same bits as one device); *kernel_ms (optional) of pc_hip_group_scan_wait = the longest member */
POLYCAP_EXTERN int pc_hip_group_scan_run(pc_hip_group *group, uint64_t seed, int64_t slot0, const pc_hip_scan_point *points,
	int64_t n_points, int64_t n_per_point, uint32_t max_attempts);
POLYCAP_EXTERN int pc_hip_group_scan_wait(pc_hip_group *group, float *kernel_ms);
POLYCAP_EXTERN int pc_hip_group_scan_totals(pc_hip_group *group, int64_t *counters, uint64_t *sumw_fixed, uint64_t *sumw2_fixed);
/* the kernel that traced the context's last scan call (member k's share of the group's), in the codes of pc_hip_last_kernel: 0 the
 * lane kernel, 4 the logging kernel; -1 before the first scan.  pc_hip_last_kernel goes on ignoring scans. */
POLYCAP_EXTERN int pc_hip_scan_last_kernel(pc_hip_ctx *ctx);
POLYCAP_EXTERN int pc_hip_group_scan_last_kernel(pc_hip_group *group, int k);

/* ---- relays: the exit beam of one optic through a second one (a focusing lens and a second lens that looks at its focus:
 * confocal set-ups), without a per-photon copy to the host.  Context A holds the first optic and has just made a source run that
 * kept images; context B holds the second optic: its own profile and glass constants, the same energy grid (its source fields are
 * not used).  pc_hip_relay_run flies A's exit photons through free space to B's entrance plane, traces them through B with the
 * explicit-photon kernel of pc_hip_launch_photons, and leaves on B what a source run leaves there.
 *
 * The contract (IEEE fp64, evaluated in the order written, no contraction).  Placement = {gap, off_x, off_y} in cm, all finite,
 * gap >= 0: B's axis is parallel to A's (a tilted B: posed relays, below) and displaced by (off_x, off_y); gap is measured from A's exit plane (pc_exit_coords[2] of
 * A's records) to B's z = 0.
 *   entries    the entries of A's store in the order of their positions (slot order; the order of completion after a run with
 *              "compact_images").  An entry whose slot failed is skipped and counted: it has pc_exit_coords[2] <= 0 (compact
 *              store: every plane zero) or a first weight <= 0 (slot-ordered store: zero weights)
 *              (only the first weight is read: when more entries are skipped than A's run counted failed slots -- a first energy
 *              without valid constants, a first weight that underflowed to 0 -- the relay is refused, PC_HIP_ERR_INVALID)
 *   inject     from A's record: position (x, y) = pc_exit_coords[0..1], direction (dx, dy) = pc_exit_dir, electric vector (ex, ey) =
 *              pc_exit_elecv (the records hold two components of each, as the reference's images do):
 *              dz = sqrt((1 - dx*dx) - dy*dy),  ez = -(ex*dx + ey*dy) / dz,  t = gap / dz
 *              start in B's frame = ((x + dx*t) - off_x, (y + dy*t) - off_y, 0), direction (dx, dy, dz), electric vector (ex, ey, ez)
 *   stage 2    pc_hip_launch_photons of B on these photons: rc in {1, 0, 2, -2, -1}, weights wB[e], state at the last interaction
 *   finish     for every photon with rc 1 and every energy: w = wA[e] * wB[e], one fp64 product;
 *              A += (uint64)(w * 2^62), and with B's option "weight_squares" B += (uint64)((w * w) * 2^62), truncated, into B's
 *              128-bit totals exactly as a source run adds them (see "standard errors" above)
 *   records    the photons with rc 1, in the order of the entries they came from, become B's image records: src_start_coords from
 *              A's record; pc_start_coords, pc_start_dir, pc_start_elecv = the injected state (x, y components); pc_exit_coords (3),
 *              pc_exit_dir and pc_exit_elecv (x, y) = the state stage 2 reports (at the last interaction, not flown to B's exit
 *              plane -- spot maps and beam moments fly every entry to their planes themselves; a photon that met no wall in B keeps
 *              the injected electric vector); pc_exit_nrefl = nA + nB; pc_exit_dtravel = (dA + t) + dB; weights w[e]
 * After the call pc_hip_transmission_records / _images, pc_hip_spot_add (kind 0) and pc_hip_beam_add (kind 0) on B read these
 * records (run size = the number of transmitted photons, which may be 0); pc_hip_transmission_totals on B gives the sums and
 * counters {rc 1, every other photon that was not absorbed, rc 0, reflections of the rc-1 photons in both optics, 0, photons
 * injected}, and pc_hip_transmission_moments the squares' sums.  All sums are integer sums over the set of photons: they depend
 * neither on how A's run was launched or stored nor on the relay's launch shape.  Many-energy relays run the immediate weight
 * sweep (the logging kernel serves source runs only).  The call returns when the relay is complete.
 *
 * Refused with PC_HIP_ERR_INVALID and a message, before anything is launched and with both contexts left as they were: a NULL or
 * repeated context, contexts on different devices, energy grids that are not bit-equal, a negative or non-finite placement, and
 * an A whose last call was not a source run that kept images (no run yet, keep_images 0, a leak_calc run, an explicit-photon
 * launch, a scan, or a relay into A -- relays are not chained). */
typedef struct { double gap, off_x, off_y; } pc_hip_relay_placement;
/* host only: the placement alone */
POLYCAP_EXTERN int pc_hip_relay_validate(const pc_hip_relay_placement *placement);
POLYCAP_EXTERN int pc_hip_relay_run(pc_hip_ctx *ctx_a, pc_hip_ctx *ctx_b, const pc_hip_relay_placement *placement);
/* of the last relay into ctx_b: counters = {n_in (photons injected), exit (rc 1), absorbed (rc 0), glass (rc 2), outside (rc -2),
 * error (rc -1), skipped (failed slots of A), n_started_A (counters[0] + [1] + [2] of A's run)}; sumw_fixed / sumw2_fixed
 * [2*n_energies] (lo, hi) pairs (sumw2_fixed: the relay must have been made with option "weight_squares" on ctx_b); any may be
 * NULL.  PC_HIP_ERR_INVALID when the last call into ctx_b was not a relay. */
POLYCAP_EXTERN int pc_hip_relay_totals(pc_hip_ctx *ctx_b, int64_t counters[8], uint64_t *sumw_fixed, uint64_t *sumw2_fixed);
/* host only: the efficiency of the train, per energy.  Every photon started into A is one trial of the Monte Carlo mean and one
 * lost anywhere -- not entered, absorbed or failed in either optic -- adds 0: eff[e] = A[e] / (n_started_A 2^62) in long double
 * (0 when n_started_A is 0).  A's open-area factor cancels as it does in pc_hip_efficiencies, and B's open area is in the geometry
 * (rc 2), not a factor.  With sumw2_fixed and stderr_ (both or neither): pc_hip_efficiency_stderr with N = n_started_A. */
POLYCAP_EXTERN void pc_hip_relay_efficiencies(size_t n_energies, const uint64_t *sumw_fixed, const uint64_t *sumw2_fixed,
	const int64_t counters[8], double *efficiencies, double *stderr_);

/* ---- posed relays: the second optic tilted against the first one's axis (the other half of a confocal alignment: a rocking curve is
 * a host loop over relays with one tilt each), and an aperture -- a pinhole, a slit, a beam stop -- between the two optics, given as
 * a selection (above) on A's exit photons.  pc_hip_relay_placement and the four calls above stay as they are; a pose is one more
 * placement of one relay.
 *
 * The frame.  In A's exit frame the origin is the centre of A's exit plane and z runs along A's axis.  B's entrance centre is at
 * c = (off_x, off_y, gap); B's x, y and z axes are u, v, n, the columns of Ry(tilt_x) * Rx(-tilt_y) (radians): a positive tilt_x
 * turns B's axis towards +x, a positive tilt_y towards +y.  With sx = sin(tilt_x), cx = cos(tilt_x), sy = sin(tilt_y), cy = cos(tilt_y):
 *   u = (cx, 0, 0 - sx)      v = (0 - sx*sy, cy, 0 - cx*sy)      n = (sx*cy, sy, cx*cy)
 * each entry one fp64 product (and one subtraction from 0, which keeps a zero's plus sign: tilt (0, 0) gives the identity bit for
 * bit).  The basis is computed once on the host and travels to the kernels as nine doubles: no trigonometric function runs on the
 * device, and pc_hip_pose_basis returns exactly these nine numbers (u0 u1 u2 v0 v1 v2 n0 n1 n2).
 * A pose is valid when its five fields are finite, gap >= 0 and |tilt_x|, |tilt_y| < pi/2 strictly (below the double nearest pi/2).
 *
 * The contract replaces the "inject" step of a relay and adds two outcomes to "entries"; every other step is the relay's (IEEE
 * fp64, in the order written, no contraction; (x, y), (dx, dy), (ex, ey) from A's record as above):
 *   dz = sqrt((1 - dx*dx) - dy*dy),  ez = -(ex*dx + ey*dy) / dz
 *   nd = (n0*dx + n1*dy) + n2*dz
 *   np = (n0*(off_x - x) + n1*(off_y - y)) + n2*gap
 *   missed when !(nd > 0) or !(np >= 0): the photon runs parallel to B's entrance plane or away from it, or the plane lies behind
 *          it.  A missed photon is not injected, and is counted.  (nd > 0 is also what lets B's records keep two components of a
 *          direction.)
 *   t = np / nd
 *   r = ((x + dx*t) - off_x, (y + dy*t) - off_y, dz*t - gap)
 *   start in B's frame = ((u0*r0 + u1*r1) + u2*r2, (v0*r0 + v1*r1) + v2*r2, 0)
 *   direction = ((u0*dx + u1*dy) + u2*dz, (v0*dx + v1*dy) + v2*dz, nd)
 *   electric vector = ((u0*ex + u1*ey) + u2*ez, (v0*ex + v1*ey) + v2*ez, (n0*ex + n1*ey) + n2*ez)
 * pc_exit_dtravel = (dA + t) + dB with this t; the records' start fields are the x, y components of this state.
 *   selection  optional: a selection made on context A and applied for kind 0 to A's last run.  An exit photon (the entries'
 *              predicate above) whose mask byte is clear is rejected: not injected, and counted in `rejected`, not in `skipped`.
 *              The mask is asked before the flight: a rejected photon is never counted as missed
 *   counts     entries of A's store = n_in + skipped + missed + rejected, for every relay.  The efficiency of the train stays
 *              sum / (n_started_A 2^62): a photon the aperture stops or that misses B is a photon lost
 *   zero tilt  a pose with both tilts 0 and no selection is the relay of {gap, off_x, off_y}: pc_hip_pose_run then runs what
 *              pc_hip_relay_run runs (the arithmetic of "inject" above, not the general form with the identity, whose sums of products
 *              may turn the sign of a zero), bit for bit in records, sums, squares and counters, with missed = rejected = 0
 * Refused with PC_HIP_ERR_INVALID and a message, before anything is launched and with both contexts and the selection left as they
 * were: what pc_hip_relay_run refuses; an invalid pose; a selection of another owner (context B, any other context, a group); a
 * selection that was not applied for kind 0; a stale mask (the rule and the wording of pc_hip_select_gather). */
typedef struct { double gap, off_x, off_y, tilt_x, tilt_y; } pc_hip_pose;
/* host only: the pose alone */
POLYCAP_EXTERN int pc_hip_pose_validate(const pc_hip_pose *pose);
/* host only: u, v, n of a valid pose */
POLYCAP_EXTERN int pc_hip_pose_basis(const pc_hip_pose *pose, double basis[9]);
/* the relay of ctx_a's exit photons into ctx_b placed at `pose`, through `select` (NULL: no aperture); pc_hip_relay_totals and
 * everything else that reads a relay's result apply as after pc_hip_relay_run */
POLYCAP_EXTERN int pc_hip_pose_run(pc_hip_ctx *ctx_a, pc_hip_ctx *ctx_b, const pc_hip_pose *pose, pc_hip_select *select);
/* of the last relay into ctx_b: counts = {missed, rejected} (both 0 after pc_hip_relay_run).  PC_HIP_ERR_INVALID when the last call
 * into ctx_b was not a relay. */
POLYCAP_EXTERN int pc_hip_pose_counts(pc_hip_ctx *ctx_b, int64_t counts[2]);

/* ---- emit relays: a thin sample between the two optics (confocal XRF: the sample sits in A's focus and re-emits isotropically, B
 * stands at an angle, 90 degrees as a rule, and collects).  A relay flies A's exit photons straight into B; an emit relay flies them
 * to a thin sheet, lets every photon that reaches it re-emit one photon towards a square target in B's entrance plane, and carries
 * the target's solid angle over 4 pi as a weight.  The entries, the second stage, the finish, the records and the totals are the
 * relay's (above); what follows replaces "inject".  IEEE fp64, evaluated in the order written, no contraction.
 *
 * The frame is A's exit frame of the posed relays: origin at the centre of A's exit plane, z along A's axis, a photon at (x, y, 0).
 * The nominal confocal point is c0 = (0, 0, focus).  With b = sample_angle, a = det_angle (radians), sb = sin(b), cb = cos(b),
 * sa = sin(a), ca = cos(a):
 *   n_s = (sb, 0, cb)                                   the sheet's normal; the sheet passes through c0 + depth n_s
 *   h_s = (n_s0*(depth*n_s0) + n_s1*(depth*n_s1)) + n_s2*(focus + depth*n_s2)        its offset n_s . (c0 + depth n_s)
 *   u = (ca, 0, 0 - sa)     v = (0, 1, 0)     n = (sa, 0, ca)        B's x, y and z axes; n points from B's entrance into B
 *   c_B[k] = ((c0[k] + wd*n[k]) + off_u*u[k]) + off_v*v[k]           B's entrance centre
 * det_angle 0 is the in-line geometry, pi/2 the confocal one.  The sixteen numbers (n_s, h_s, u, v, n, c_B in this order) are computed
 * once on the host, a turned sign as "0 - x" so that angles (0, 0) give the identity with plus-signed zeros, and travel to the
 * kernels: no trigonometric function runs on the device, and pc_hip_emit_frame returns exactly these numbers.
 * A spec is valid when its eight doubles are finite, focus >= 0, |sample_angle| < pi/2 strictly (below the double nearest pi/2),
 * |det_angle| <= pi (the double nearest pi), wd > 0 and target_half > 0; map is NULL with n_map 0, or n_map >= 1 indices >= 0.
 *   energies   fluorescence is detected at another energy than it was excited with: with a map, n_map must be B's energy count and
 *              B's energy e takes A's weight of energy map[e], an index into A's grid; the two grids need not agree.  Without a map
 *              both grids must be bit-equal (the relay's rule) and the map is the identity
 *   entries    those of a posed relay, an optional selection included (asked first: a rejected photon is never counted as missed).
 *              Every entry has the slot s of A's run it came from: slot0 + position in a slot-ordered store, slot0 + the id plane's
 *              value in a compact store made with option "slot_ids"; a compact store without it is refused.  The random numbers of
 *              an entry are keyed by s, so the result does not depend on the store's order
 *   emission   from A's record (x, y), (dx, dy) and s, with R = target_half:
 *              dz = sqrt((1 - dx*dx) - dy*dy)
 *              sd = (n_s0*dx + n_s1*dy) + n_s2*dz,   sp = h_s - (n_s0*x + n_s1*y)
 *              missed the sample when !(sd > 0) or !(sp >= 0): not injected, counted
 *              t = sp / sd,   p = (x + dx*t, y + dy*t, dz*t)
 *              u1, u2 = uniforms 0 and 1 of the stream (seed, s, attempt 0) of the source sampler (Philox4x32-10, 53 bits each)
 *              a = (2*u1 - 1)*R,   b = (2*u2 - 1)*R         a point uniform on a square in B's entrance plane: no trigonometry, no
 *                                                           rejection loop; what falls outside B's hexagon is rc -2 of stage 2
 *              q = c_B - p;   f = (a + ((u0*q0 + u1*q1) + u2*q2),  b + ((v0*q0 + v1*q1) + v2*q2),  (n0*q0 + n1*q1) + n2*q2)
 *              missed the detector when !(f2 > 0): the point of emission lies in B's entrance plane or behind it; not injected, counted
 *              r2 = (f0*f0 + f1*f1) + f2*f2,   r = sqrt(r2),   d = (f0/r, f1/r, f2/r)
 *              g = ((R*R)*d2) / (pi*r2)   with pi = 0x1.921fb54442d18p+1: the target's solid angle over 4 pi, per photon
 *              electric vector (unpolarised emission without a random angle): h = sqrt(d2*d2 + d0*d0),
 *              e1 = (d2/h, 0, 0 - d0/h),   e2 = (0 - (d0*d1)/h, h, 0 - (d1*d2)/h);   e1 for even s, e2 for odd s
 *   stage 2    pc_hip_launch_photons of B on the photons (a, b, 0), d, e
 *   finish     for every photon with rc 1 and every energy e of B: w = (wA[map[e]] * g) * wB[e]; sums, squares and counters as a relay
 *   records    as a relay's, with pc_start_* = the injected state, pc_exit_dtravel = ((dA + t) + r) + dB, pc_exit_nrefl = nA + nB
 *   counts     entries of A's store = n_in + skipped + missed_sample + missed_detector + rejected, always
 * pc_hip_relay_totals and pc_hip_relay_efficiencies apply unchanged (pc_hip_pose_counts: missed = missed_sample + missed_detector).
 * The efficiency is that of detected photons per photon started into A, per unit interaction probability in the sheet, for isotropic
 * emission: the caller multiplies by mu t / cos and the yield.
 * Refused with PC_HIP_ERR_INVALID and a message, before anything is launched and with both contexts and the selection left as they
 * were: what pc_hip_pose_run refuses (without a map: unequal grids); an invalid spec; a compact A without slot ids; a map of the wrong
 * length or with an index outside A's grid. */
typedef struct {
	double focus, sample_angle, depth, det_angle, wd, off_u, off_v, target_half;
	uint64_t seed;
	int32_t n_map;
	const int32_t *map;
} pc_hip_emit;
/* host only: the spec alone (the map against the contexts' grids: pc_hip_emit_run) */
POLYCAP_EXTERN int pc_hip_emit_validate(const pc_hip_emit *spec);
/* host only: n_s (3), h_s, u (3), v (3), n (3), c_B (3) of a valid spec */
POLYCAP_EXTERN int pc_hip_emit_frame(const pc_hip_emit *spec, double frame[16]);
/* the emit relay of ctx_a's exit photons into ctx_b, through `select` (NULL: no aperture) */
POLYCAP_EXTERN int pc_hip_emit_run(pc_hip_ctx *ctx_a, pc_hip_ctx *ctx_b, const pc_hip_emit *spec, pc_hip_select *select);
/* of the last relay into ctx_b, which must have been an emit relay: counts = {missed_sample, missed_detector, rejected} */
POLYCAP_EXTERN int pc_hip_emit_counts(pc_hip_ctx *ctx_b, int64_t counts[3]);

/* ---- slab emits: an emit relay through a thick sample.  The sample is a laterally infinite slab whose front face is the emit's sheet
 * (the plane through c0 + depth n_s with the normal n_s) and which extends `thickness` (T, cm) along +n_s.  The excitation is
 * attenuated on its way to the depth of interaction, the fluorescence on its way out towards B; the sample's linear attenuation
 * coefficients (1/cm) come as two tables, mu_in[n_energies of A] and mu_out[n_energies of B].  IEEE fp64, evaluated in the order
 * written, no contraction, no fma.
 *   frame      the emit's sixteen numbers (the same code, the same bits), then k = (n_s.u, n_s.v, n_s.n), every dot product as
 *              (a0*b0 + a1*b1) + a2*b2, then T: twenty numbers, computed once on the host (pc_hip_slab_frame)
 *   entries, selection, slots: the emit's
 *   emission   dz, sd, sp, "missed the sample", t and p as in an emit, then
 *              L = T / sd                                       the path through the whole slab
 *              u1, u2, u3 = uniforms 0, 1 and 2 of the entry's stream: 0 and 1 are the emit's, so that a thin and a thick emit with
 *                                                               one seed aim at the same target point
 *              s = u3*L,   zn = s*sd                            the path to the interaction, uniform on [0, L), and its depth
 *              p' = (p0 + dx*s, p1 + dy*s, p2 + dz*s)
 *              a, b, q = c_B - p', f, "missed the detector", r2, r, d, g and the electric vector as in an emit, p' in the place of p
 *              cn = ((k0*f0 + k1*f1) + k2*f2) / r               the emitted ray's cosine to n_s
 *              cn > 0 (it leaves through the back):   tz = T - zn, set to 0 when negative;   s_out = tz/cn
 *              cn < 0 (through the front, the reflection geometry):   s_out = zn/(0 - cn)
 *              otherwise: missed the detector
 *              gl = g*L;   missed the sample when !(gl < 1): grazing incidence on a slab so thick that the estimator's weight would
 *              leave the range of the exact sums
 *   finish     for every photon with rc 1 and every energy e of B:
 *              a_e = mu_in[map[e]]*s + mu_out[e]*s_out,   att = E(0 - a_e),   w = ((wA[map[e]]*gl)*att)*wB[e]
 *              E(x), x <= 0: +0 when x < -700 (no subnormal arises), else with k = rint(x*1.4426950408889634074):
 *              r = (x - k*6.93147180369123816490e-01) - k*1.90821492927058770002e-10,   the degree-11 Horner polynomial
 *              p = p*r + c with c = 1/11!, 1/10!, ..., 1/2, 1, 1 (the doubles pc_emit.h writes),   E = ldexp(p, k); within 1e-14
 *              relative of exp(x); E(0) = 1 exactly; a NaN gives a NaN
 *   records    as an emit's, with pc_exit_dtravel = (((dA + t) + s) + r) + dB
 *   counts     the emit's, and their identity; pc_hip_emit_counts and pc_hip_pose_counts answer after a slab emit too
 * The interaction depth is sampled uniformly along the path, not exponentially: one geometry serves every energy, and a depth scan
 * keeps common random numbers.  The efficiency is that of detected photons per photon started into A, per unit fluorescence-
 * production coefficient (1/cm), for isotropic emission: the caller multiplies by that coefficient and the yield.
 * A spec is valid when its emit is, thickness is finite and in (0, 1] cm, both tables are given with at least one entry, and every mu
 * is finite and >= 0.  Refused with PC_HIP_ERR_INVALID and a message that names the field, before anything is launched and with both
 * contexts and the selection left as they were: what pc_hip_emit_run refuses; an invalid spec; n_mu_in other than A's energy count,
 * n_mu_out other than B's. */
typedef struct {
	pc_hip_emit emit;
	double thickness;
	int32_t n_mu_in;
	const double *mu_in;
	int32_t n_mu_out;
	const double *mu_out;
} pc_hip_slab;
/* host only: the spec alone (the map and the tables' lengths against the contexts' grids: pc_hip_slab_run) */
POLYCAP_EXTERN int pc_hip_slab_validate(const pc_hip_slab *spec);
/* host only: the emit's sixteen numbers, k (3), T of a valid spec */
POLYCAP_EXTERN int pc_hip_slab_frame(const pc_hip_slab *spec, double frame[20]);
/* the slab emit of ctx_a's exit photons into ctx_b, through `select` (NULL: no aperture); everything that reads an emit relay's
 * result applies unchanged */
POLYCAP_EXTERN int pc_hip_slab_run(pc_hip_ctx *ctx_a, pc_hip_ctx *ctx_b, const pc_hip_slab *spec, pc_hip_select *select);

/* ---- layered emits: an emit relay through a stack of sample layers (varnish over paint over ground, a coating on a substrate, a
 * buried marker layer).  The stack sits behind the emit's sheet as the slab does: layer 0 starts at the front face, each further
 * layer lies along +n_s.  Layer j has a thickness T_j (cm), attenuation coefficients mu_in[j][eA] at A's energies and mu_out[j][eB]
 * at B's (1/cm), and a fluorescence-production coefficient production[j][eB] (1/cm): the coefficient a slab emit leaves to the
 * caller, here per layer.  The tables are row-major by layer.  1 <= n_layers <= PC_HIP_MAX_LAYERS.  IEEE fp64, evaluated in the
 * order written, no contraction, no fma.
 *   bounds     Z_0 = 0,   Z_{j+1} = Z_j + T_j   summed left to right on the host;   T = Z_n
 *   tables     summed once per call on the host in plain doubles, each product formed before its add:
 *              Pin[j][ea]  = sum_{k<j} mu_in[k][ea]*T_k    added left to right
 *              Pout[j][e]  = sum_{k<j} mu_out[k][e]*T_k    added left to right
 *              Sout[j][e]  = sum_{k>j} mu_out[k][e]*T_k    added right to left
 *              qmax = the largest entry of production
 *   frame      the slab's twenty numbers for the thickness T (the same code, the same bits), then qmax: twenty-one numbers
 *              (pc_hip_layers_frame)
 *   entries, selection, slots: the emit's
 *   emission   the slab's for the thickness T, operation for operation: dz, sd, sp, "missed the sample", t, p, L = T/sd, u1, u2, u3,
 *              s = u3*L, zn = s*sd, p', a, b, q, f, "missed the detector", r2, r, d, g, the electric vector,
 *              cn = ((k0*f0 + k1*f1) + k2*f2) / r,   missed the detector unless cn > 0 or cn < 0,   gl = g*L.  Then, once per photon:
 *              missed the sample when !(gl*qmax < 1): the slab's guard for a production coefficient other than 1.  With wA <= 1,
 *              E <= 1, wB <= 1 and monotone rounding every weight then stays below 1, inside the range of the exact sums
 *              j = the number of inner boundaries Z_k, k = 1 .. n_layers - 1, with zn >= Z_k: the layer of the interaction.  A point
 *              on a boundary belongs to the layer behind it; a zn that rounding carried past T stays in the last layer
 *              za = zn - Z_j,   zb = Z_{j+1} - zn, set to 0 when negative
 *   finish     for every photon with rc 1 and every energy e of B, with ea = map[e]:
 *              tau_in  = (Pin[j][ea] + mu_in[j][ea]*za) / sd
 *              tau_out = (Sout[j][e] + mu_out[j][e]*zb) / cn              when cn > 0 (out through the back)
 *                      = (Pout[j][e] + mu_out[j][e]*za) / (0 - cn)        when cn < 0 (out through the front)
 *              w = ((wA[ea]*gl) * (production[j][e] * E(0 - (tau_in + tau_out)))) * wB[e]          E: the slab's
 *   records    the slab's: pc_start_* = the injected state, pc_exit_dtravel = (((dA + t) + s) + r) + dB.  Every column but the weights
 *              is bit for bit that of a slab emit of thickness T
 *   counts     the emit's, and their identity; pc_hip_emit_counts and pc_hip_pose_counts answer after a layered emit too
 * The efficiency is that of detected photons per photon started into A, for isotropic emission: the production coefficients are in
 * the weights, the caller multiplies by the yield only.  Since the weight is linear in production, the emit with a table equals, photon
 * by photon and in the exact sums, the sum of the emits with one layer's row kept and the others zero.
 * A spec is valid when its emit is, 1 <= n_layers <= PC_HIP_MAX_LAYERS, every thickness is finite and in (0, 1] cm, T <= 1 cm, the
 * four arrays are given with n_mu_in >= 1 and n_mu_out >= 1, and every mu and production entry is finite and >= 0.  Refused with
 * PC_HIP_ERR_INVALID and a message that names the table, the layer and the index, before anything is launched and with both contexts
 * and the selection left as they were: what pc_hip_emit_run refuses; an invalid spec; n_mu_in other than A's energy count, n_mu_out
 * other than B's. */
#define PC_HIP_MAX_LAYERS 16
typedef struct {
	pc_hip_emit emit;
	int32_t n_layers;
	const double *thickness;           /* [n_layers] */
	int32_t n_mu_in;
	const double *mu_in;               /* [n_layers*n_mu_in] */
	int32_t n_mu_out;
	const double *mu_out;              /* [n_layers*n_mu_out] */
	const double *production;          /* [n_layers*n_mu_out] */
} pc_hip_layers;
/* host only: the spec alone (the map and the tables' row lengths against the contexts' grids: pc_hip_layers_run) */
POLYCAP_EXTERN int pc_hip_layers_validate(const pc_hip_layers *spec);
/* host only: the slab's twenty numbers with T = the total thickness, then qmax */
POLYCAP_EXTERN int pc_hip_layers_frame(const pc_hip_layers *spec, double frame[21]);
/* the layered emit of ctx_a's exit photons into ctx_b, through `select` (NULL: no aperture); everything that reads an emit relay's
 * result applies unchanged */
POLYCAP_EXTERN int pc_hip_layers_run(pc_hip_ctx *ctx_a, pc_hip_ctx *ctx_b, const pc_hip_layers *spec, pc_hip_select *select);

/* free and total memory of the context's device, bytes */
POLYCAP_EXTERN int pc_hip_device_memory(pc_hip_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* Scheduler statistics of the last transmission run (diagnostics): {march steps, march lane-steps, event phases,
 * event lanes, new phases, new lanes}, summed over all waves; lanes/phases = average active lanes per phase. */
POLYCAP_EXTERN int pc_hip_phase_stats(pc_hip_ctx *ctx, int64_t stats[6]);
/* Which kernel traced the last source run: 0 one photon per lane (pc_trace_kernel), 1 LDS photon pool (option "pool"),
 * 2 launching wave per workgroup (option "producer"; by default chosen when the photons of the context's last run made at
 * least 4 segment visits (reflections, mostly; absorbed photons included) per launch -- a first run of 2e6 slots or more is preceded by a 32768-slot probe),
 * 3 one wave per photon (experiment builds only), 4 logged reflections (pc_trace_log_kernel: source runs with more than 8
 * energies, option "batch_reflections" 1), 5 leak_calc runs (pc_leak_kernel; explicit-photon leak launches included).  -1: none yet. */
POLYCAP_EXTERN int pc_hip_last_kernel(pc_hip_ctx *ctx);
/* The weight sweeps of the last run when pc_trace_log_kernel traced it: stats = {wave-level passes over 64 (photon, energy)
 * pairs, wave-level (pass, reflection) iterations, sum over the waves of their lifetimes in shader clock ticks, the longest
 * lifetime (mean / longest = how evenly the waves finished)}; *ct_tame (optional) = the grazing cosine above which the host certified
 * every energy's reflectivity inside [0, 1 - 1e-11] (-1: no log run yet); proxies (optional) = the one or two energy indices
 * every lane follows itself (-1: none) */
POLYCAP_EXTERN int pc_hip_sweep_stats(pc_hip_ctx *ctx, int64_t stats[4], double *ct_tame, int proxies[2]);

/* 1 when the host address lies in memory registered with (pinned by) the HIP runtime */
POLYCAP_EXTERN int pc_hip_host_is_pinned(const void *p);

/* efficiency formula of src/polycap-source.c:1066-1076 from (summed) totals */
POLYCAP_EXTERN void pc_hip_efficiencies(size_t n_energies, const double *sum_weights, const int64_t counters[6], double *efficiencies);
/* exact fixed-point (lo,hi) pair -> double */
POLYCAP_EXTERN double pc_hip_fixed_to_double(uint64_t lo, uint64_t hi);


/* Host-side helper with no reference counterpart: builds the polycap_transmission_efficiencies result object from
 * totals and (optional) image planes produced elsewhere -- summed over several GPUs / ranks by the caller -- so the
 * getters and the HDF5 writer serve a sharded run exactly as a single-device one.  `source` is a polycap_source*
 * (it must outlive the result, as in the reference); counters as pc_hip_transmission_totals(); planes hold n_exit
 * entries each (NULL planes read as zeros); the efficiency formula is that of src/polycap-source.c:1066-1076.
 * Returns a polycap_transmission_efficiencies* or NULL with *error (a polycap_error**) set. */
POLYCAP_EXTERN void *pc_transmission_efficiencies_from_totals(void *source, int64_t n_exit, const double *sum_weights,
	const int64_t counters[6], const pc_hip_images *planes, void *error);

/* Spot maps of a result of polycap_source_get_transmission_efficiencies made with POLYCAP_SPOT set (efficiencies: a
 * polycap_transmission_efficiencies*, error: a polycap_error**).  kind 0 = exit photons, 1 = extleak, 2 = intleak (leak_calc runs).
 * dims = {n_planes, n_energies, ny, nx}; window = {x0, x1, y0, y1} cm; *distances [n_planes] cm, *energies [n_energies] keV,
 * *maps [plane][energy][iy][ix] and *outside [plane][energy] are copies to be freed with polycap_free (any of them may be NULL).
 * The maps are in efficiency units: map = efficiency[e] * S_bin / (S_inside + S_outside) from the exact sums, so that a map plus
 * its outside part sums to the efficiency.  Returns 1, or 0 with *error set. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_spot(void *efficiencies, int kind, int32_t dims[4], double **distances, double window[4],
	double **energies, double **maps, double **outside, void *error);

/* Standard errors of a result of polycap_source_get_transmission_efficiencies made with POLYCAP_STDERR=1 (every path of the call:
 * one device, POLYCAP_HIP_DEVICES groups, leak_calc, POLYCAP_IMAGES=0 with the chunked POLYCAP_SPOT runs): *stderr [n_energies],
 * pc_hip_efficiency_stderr of the run's exact moments, to be freed with polycap_free.  _get_moments: N (started photons) and
 * copies of the exact (lo, hi) sums A and B [2*n_energies] (either may be NULL), so that the results of several seeds can be pooled
 * exactly.  A result made without the variable is an error.  Return 1, or 0 with *error (a polycap_error**) set. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_stderr(void *efficiencies, size_t *n_energies, double **stderr_, void *error);
POLYCAP_EXTERN int pc_transmission_efficiencies_get_moments(void *efficiencies, int64_t *n_started, uint64_t **sumw_fixed,
	uint64_t **sumw2_fixed, void *error);

/* Exit-beam moments of a result made with POLYCAP_BEAM=1 (every path of the call: one device, POLYCAP_HIP_DEVICES groups, leak_calc,
 * POLYCAP_IMAGES=0 with the chunked runs of POLYCAP_SPOT_SHARE).  kind 0 = exit photons, 1 = extleak, 2 = intleak (leak_calc runs).
 * _get_beam: *params [n_energies][26], pc_hip_beam_params of the run's exact sums (columns: pc_hip_beam_columns).  _get_beam_sums:
 * copies of the sums [n_energies][15][2] and outside counters [n_energies] (either may be NULL) and the entry count, so that the
 * results of several seeds can be pooled exactly (add the sums as 128-bit integers, then pc_hip_beam_params).  Copies are freed
 * with polycap_free.  A result made without the variable is an error.  Return 1, or 0 with *error (a polycap_error**) set. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_beam(void *efficiencies, int kind, size_t *n_energies, double **params, void *error);
POLYCAP_EXTERN int pc_transmission_efficiencies_get_beam_sums(void *efficiencies, int kind, size_t *n_energies, uint64_t **sums,
	uint64_t **outside, int64_t *n_entries, void *error);

/* Histograms of a result made with POLYCAP_HIST set (every path of the call that POLYCAP_BEAM serves), e.g.
 * POLYCAP_HIST="axis=x,d=0.5,range=-0.01:0.01,bins=2048;axis=r,d=0.5,centre=0:0,range=0:0.02,bins=1024;axis=nrefl,range=0:256,bins=256;energies=all"
 * (axes: x y r slope_x slope_y tan_theta nrefl dtravel r_start z; cm; energies as in POLYCAP_SPOT).  kind 0 = exit photons, 1 =
 * extleak, 2 = intleak (leak_calc runs).  dims = {n_axes, n_selected, total_bins}; copies, to be freed with polycap_free (any may be
 * NULL): *offsets [n_axes + 1], *axes [n_axes], *energies [n_selected] keV, the exact sums *bins [n_selected][total_bins] and
 * *outside [n_axes][n_selected] of pc_hip_hist_read, so that the results of several seeds pool exactly; *n_entries.  A result made
 * without the variable is an error.  Returns 1, or 0 with *error (a polycap_error**) set. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_hist(void *efficiencies, int kind, int32_t dims[3], int32_t **offsets,
	pc_hip_hist_axis **axes, double **energies, uint64_t **bins, uint64_t **outside, int64_t *n_entries, void *error);

/* Joint histograms of a result made with POLYCAP_JOINT set (every path of the call that POLYCAP_HIST serves), e.g.
 * POLYCAP_JOINT="axis=x,d=0.5,range=-0.01:0.01,bins=256*axis=slope_x,range=-0.005:0.005,bins=256;axis=start_x,range=-0.3:0.3,bins=512*axis=start_y,range=-0.3:0.3,bins=512;energies=all"
 * (items separated by ';': a pair is two axes of the POLYCAP_HIST grammar joined by '*', u first; axes as there, and start_x
 * start_y; energies as there).  kind 0 = exit photons, 1 = extleak, 2 = intleak (leak_calc runs).  dims = {n_pairs, n_selected,
 * total_cells}; copies, to be freed with polycap_free (any may be NULL): *offsets [n_pairs + 1], *pairs [n_pairs], *energies
 * [n_selected] keV, the exact sums *cells [n_selected][total_cells] and *outside [n_pairs][n_selected] of pc_hip_joint_read, so that
 * the results of several seeds pool exactly; *n_entries.  A result made without the variable is an error.  Returns 1, or 0 with
 * *error (a polycap_error**) set. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_joint(void *efficiencies, int kind, int32_t dims[3], int32_t **offsets,
	pc_hip_joint_pair **pairs, double **energies, uint64_t **cells, uint64_t **outside, int64_t *n_entries, void *error);

/* The selection of a result made with POLYCAP_SELECT set (every path of the call that POLYCAP_JOINT serves), e.g.
 * POLYCAP_SELECT="axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not"
 * (cuts separated by ';' in the axis grammar of POLYCAP_HIST without bins, a cut with the word "not" being negated; the grammar of
 * pc_hip_select_parse).  When set, every tally of the call (POLYCAP_SPOT, _BEAM, _HIST, _JOINT) is filled through the selection for
 * every kind it tallies.  Returns 1 and (free each array with polycap_free): *n_cuts, *cuts [n_cuts][7] rows of quantity, d, cx, cy,
 * lo, hi, negate; *n_energies; n_pass [3] and n_seen [3] (exit photons, extleak, intleak; zeros for the leak kinds of a plain run);
 * the exact sums *passed_w [3][n_energies] and *rejected_w [3][n_energies] of pc_hip_select_read, so that the results of several
 * seeds pool exactly.  A result made without POLYCAP_SELECT fails with POLYCAP_ERROR_INVALID_ARGUMENT. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_select(void *efficiencies, int32_t *n_cuts, double **cuts, size_t *n_energies,
	int64_t n_pass[3], int64_t n_seen[3], uint64_t **passed_w, uint64_t **rejected_w, void *error);

/* The selected photons themselves: POLYCAP_SELECT_RECORDS=N (an integer 1 .. 2^31 - 1; anything else, or the variable without
 * POLYCAP_SELECT, is POLYCAP_ERROR_INVALID_ARGUMENT before any device is used) makes the result carry, for every kind the call applies
 * the selection to (exit photons always, extleak and intleak for leak_calc runs), the first N passing entries in order as rows of
 * pc_hip_select_gather: only those rows leave the device, on every path POLYCAP_SELECT serves.  N bounds the host memory; n_pass stays
 * available from _get_select.  Order and position are those of the concatenation of everything the call's applies saw: the chunks of a
 * POLYCAP_IMAGES=0 run in slot-range order, the members of a device group in member order; a row's position is the entries seen by
 * the earlier applies plus its position inside its apply.  For a call that keeps its images these are the positions of the result's
 * own exit arrays.  Returns 1 and (free each array with polycap_free; records and positions may be NULL): *n_rows = min(N, n_pass),
 * *row_doubles (PC_HIP_N_PLANES + n_energies for kind 0 with the reflection count as int64 bits, PC_HIP_LEAK_HDR + n_energies for the
 * leak kinds), *records [n_rows][row_doubles], *positions [n_rows].  A result made without the variable, or a kind the call did not
 * apply, fails with POLYCAP_ERROR_INVALID_ARGUMENT.  write_hdf5 adds /Select/<Kind>_Records (double [n_rows][row_doubles]) and
 * /Select/<Kind>_Positions (int64 [n_rows]) per kind present, and /Select/Records_Limit. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_select_records(void *efficiencies, int kind, int64_t *n_rows, int32_t *row_doubles,
	double **records, int64_t **positions, void *error);

/* An unweighted sample of the beam: POLYCAP_DRAW="n=100000,energy=3,phase=12345" (n: the sample size, 1 .. 2^31 - 1; energy: an index
 * into the source's energies, default 0; phase: a uint32, default 0, so that the call stays reproducible; an unknown key, a missing n,
 * a value outside those ranges or an empty value is POLYCAP_ERROR_INVALID_ARGUMENT naming the item, before any device is used and
 * behind the refusals of every other variable) makes the result carry, for every kind the call has (exit photons always, extleak and
 * intleak for leak_calc runs), the n draws of pc_hip_select_draw at that energy: through the selection of POLYCAP_SELECT when it is
 * set, through one that every entry passes otherwise (the result then reports no selection).  A kind without weight at that energy
 * carries no rows and is not an error.  It works with POLYCAP_IMAGES=0 and POLYCAP_HIP_DEVICES; a POLYCAP_IMAGES=0 run whose exit data
 * exceed POLYCAP_SPOT_SHARE of the device's memory, which is traced as several slot ranges, has no one beam on the device and is
 * refused with POLYCAP_ERROR_INVALID_ARGUMENT.  Returns 1 and (free each array with polycap_free; any pointer but n_rows may be NULL):
 * *n_rows = n or 0, *row_doubles, *records [n_rows][row_doubles] and *positions [n_rows] as in _get_select_records, *total = T of the
 * kind (a draw stands for T * 2^-32 / n of weight per started photon), and the request in *n, *energy, *phase.  A result made without
 * the variable, or a kind the call does not have, fails with POLYCAP_ERROR_INVALID_ARGUMENT.  write_hdf5 adds the group /Draw with the
 * attributes n, energy_index, energy_keV, phase and, per kind present, <Kind>_total (uint64) and <Kind>_weight, and the datasets
 * /Draw/<Kind>_Records and /Draw/<Kind>_Positions of every kind that has rows. */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_draw(void *efficiencies, int kind, int64_t *n_rows, int32_t *row_doubles, double **records,
	int64_t **positions, uint64_t *total, int64_t *n, int32_t *energy, uint32_t *phase, void *error);

/* Standard errors of the tallies through the public call: POLYCAP_TALLY_STDERR=1 (0 or unset: none; anything else is
 * POLYCAP_ERROR_INVALID_ARGUMENT; it is not POLYCAP_STDERR, whose outputs stay as they are) makes every tally of the call (POLYCAP_SPOT,
 * _HIST, _JOINT) and its POLYCAP_SELECT selection track squares (pc_hip_*_track_squares), on every path those variables serve: chunked
 * POLYCAP_IMAGES=0 runs, device groups, leak runs.  N is the call's own: counters 0 + 1 + 2.
 * _get_tally_squares: which = 0 (POLYCAP_SPOT), 1 (_HIST), 2 (_JOINT); kind as in the tally's own getter.  Returns 1 and (free each array
 * with polycap_free; any pointer may be NULL): *n_cells and *n_outside, the cell and outside counts of the tally's getter ([plane][energy]
 * [iy][ix] and [plane][energy]; [energy][total_bins] and [axis][energy]; [energy][total_cells] and [pair][energy]); the exact sums
 * *sums [n_cells] and *outside [n_outside] (for the spot maps these are the uint64 sums behind the maps); *squares [n_cells][2] and
 * *outside_squares [n_outside][2]; *stderrs [n_cells] and *outside_stderrs [n_outside] = pc_hip_tally_stderr with N = *n_started.
 * _get_select_squares: *passed_w2 and *rejected_w2 [3][n_energies][2], and *transmission and *transmission_stderr [3][n_energies] of
 * pc_hip_select_transmission per kind.  A result made without POLYCAP_TALLY_STDERR=1, or without the tally's variable, fails with
 * POLYCAP_ERROR_INVALID_ARGUMENT.  write_hdf5 adds, beside each bins or cells dataset: /Spot/<Kind>_Squares, _Outside_Squares, _StdErr,
 * _Outside_StdErr; /Hist/<Kind>/Bins_Squares, Outside_Squares, Bins_StdErr, Outside_StdErr; /Joint/<Kind>/Cells_Squares, Outside_Squares,
 * Cells_StdErr, Outside_StdErr; /Select/Passed_Squares, Rejected_Squares, Transmission, Transmission_StdErr (uint64 with a trailing
 * dimension 2, and doubles). */
POLYCAP_EXTERN int pc_transmission_efficiencies_get_tally_squares(void *efficiencies, int which, int kind, size_t *n_cells, size_t *n_outside,
	uint64_t **sums, uint64_t **outside, uint64_t **squares, uint64_t **outside_squares, double **stderrs, double **outside_stderrs,
	int64_t *n_started, void *error);
POLYCAP_EXTERN int pc_transmission_efficiencies_get_select_squares(void *efficiencies, size_t *n_energies, uint64_t **passed_w2,
	uint64_t **rejected_w2, double **transmission, double **transmission_stderr, void *error);

#ifdef __cplusplus
}
#endif
#endif

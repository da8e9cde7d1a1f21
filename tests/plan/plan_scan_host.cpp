/* The launch planner of pc_plan.h compiled for the host, with pc_plan_input::scan_log among the inputs (context option "scan_log":
 * scans through the logging kernel): what tests/test_scan_log_plan_cpu.py calls.  plan_host.cpp beside it leaves the field at its
 * default.  Options, inputs and plan fields cross the boundary as arrays in the order of the name lists below. */
#define PC_PLAN_HOST_ONLY
#include "pc_plan.h"

#include <cstdint>

#define PLAN_OPTS(X) X(literal) X(event_threshold) X(new_threshold) X(march_burst) X(march_stop) X(blocks_per_cu) X(block_size) X(cu_share) \
	X(producer) X(producer_new_min) X(producer_new_first) X(pool) X(pool_refill) X(pool_march_min) X(pool_event_min) X(pool_new_min) \
	X(event_march) X(lds_ec) X(batch_reflections) X(log_cap) X(log_min_energies) X(flush_max) X(sweep_skip) X(sweep_fuse) \
	X(sweep_exact_every) X(march_stats) X(wave_per_photon) X(weight_squares)
#define PLAN_INPUTS(X) X(ne) X(npts) X(n_shells) X(all_valid) X(rough) X(n_cu) X(refl_per_launch) X(mode) X(n_items) X(n_slots) \
	X(max_attempts) X(keep_images) X(squares) X(force_lane) X(halves) X(scan_log)
#define PLAN_FIELDS(X) X(kernel) X(kne) X(pitch) X(sq) X(march_stats) X(grid) X(block) X(dyn_lds) X(lds_acc) X(lds_ec) X(sweep_rough) \
	X(log_cap) X(stage_doubles) X(stage_ps) X(flush_min) X(sweep_skip) X(sweep_fuse) X(sweep_exact_every) X(event_threshold) \
	X(new_threshold) X(pool_event_min) X(event_march) X(half_w) X(half_l)

#define NAME(f) #f " "
#define COUNT(f) + 1
static_assert(sizeof(pc_launch_opts) == (0 PLAN_OPTS(COUNT))*sizeof(int), "PLAN_OPTS lists every option of pc_launch_opts");

extern "C" {

const char *plan_opt_names(void) { return PLAN_OPTS(NAME); }
const char *plan_input_names(void) { return PLAN_INPUTS(NAME); }
const char *plan_field_names(void) { return PLAN_FIELDS(NAME); }

void plan_default_opts(int32_t *opts)
{
	const pc_launch_opts o;
#define GET(f) *opts++ = o.f;
	PLAN_OPTS(GET)
#undef GET
}

void plan_launch(const int32_t *opts, const double *inputs, int64_t *fields)
{
	pc_launch_opts o;
	pc_plan_input in;
#define SET(f) o.f = *opts++;
	PLAN_OPTS(SET)
#undef SET
#define SET(f) in.f = (decltype(in.f))*inputs++;
	PLAN_INPUTS(SET)
#undef SET
	const pc_launch_plan p = pc_plan_launch(in, o);
#define GET(f) *fields++ = (int64_t)p.f;
	PLAN_FIELDS(GET)
#undef GET
}

}

/*
 * pc_options.h -- pc_hip_set_option: one chain of names, each with its own range and words, over the four owners that hold the
 * values (pc_launch_opts, the image store, the leak run, the context with its scan and relay state).  Included by pc_kernels.hip.
 */
#ifndef PC_OPTIONS_H
#define PC_OPTIONS_H

extern "C" {

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
	else if (n == "scan_log") { if (value < 0 || value > 1) return pc_fail(PC_HIP_ERR_INVALID, "scan_log must be 0 or 1"); ctx->scan.log = (int)value; }
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

} /* extern "C" */

#endif /* PC_OPTIONS_H */

/*
 * pc_launch.h -- from a context to a running trace kernel: the arguments every launch shares (pc_fill_common), the one place a
 * trace kernel is launched from (pc_launch_planned, the only reader of a pc_launch_plan) and plan-then-launch (pc_launch_kernel).
 * Included by pc_kernels.hip behind the kernels and the context.
 */
#ifndef PC_LAUNCH_H
#define PC_LAUNCH_H

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
	pc_lane_scratch &lanes = SCAN ? ctx->scan.lanes : ctx->lanes;
	int st = lanes.grow(p.half_w * (size_t)site.halves, p.half_l * (size_t)site.halves);
	if (st) return st;
	if (p.half_w) a.wscratch = lanes.d_wscratch + (size_t)site.half * p.half_w;
	if (p.half_l) a.rlog = lanes.d_rlog + (size_t)site.half * p.half_l;
	a.total_threads = (long long)p.grid * p.block;
	a.lds_acc = p.lds_acc; a.lds_ec = p.lds_ec; a.sweep_rough = p.sweep_rough;
	a.event_threshold = p.event_threshold; a.new_threshold = p.new_threshold;
	a.pool_event_min = p.pool_event_min; a.event_march = p.event_march;
	a.log_cap = p.log_cap; a.stage_ps = p.stage_ps; a.flush_min = p.flush_min;
	a.sweep_skip = p.sweep_skip; a.sweep_fuse = p.sweep_fuse; a.sweep_exact_every = p.sweep_exact_every;
	if (p.kernel == PC_KERNEL_LOG) {
		if (!ctx->cert.known) ctx->cert = pc_sweep_certify(ctx->host.ec);
		a.n_proxy = ctx->cert.n_proxy; a.proxy_e[0] = ctx->cert.proxy_e[0]; a.proxy_e[1] = ctx->cert.proxy_e[1];
		a.ct_tame = ctx->cert.ct_tame;
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
	if (SCAN) ctx->scan.kernel = p.kernel; else ctx->last_kernel = p.kernel;
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
	in.scan_log = ctx->scan.log != 0;
	return pc_launch_planned<MODE>(ctx, site, pc_plan_launch(in, ctx->opts), a);
}

/* a big single-energy run of a context that does not know yet how long its photons live is preceded by a probe (pc_probe_lifetime) */
static bool pc_wants_probe(const pc_hip_ctx *ctx, long long n_slots)
{
	return ctx->opts.producer < 0 && ctx->refl_per_launch < 0. && ctx->host.pm.n_energies == 1 && n_slots >= 2000000;
}

#endif /* PC_LAUNCH_H */

/*
 * pc_scan.h -- scans: transmission as a function of the source position, one launch for a whole grid of points with exact
 * totals per point (include/polycap-hip.h, pc_hip_scan_*).  The kernel is pc_trace_kernel with MODE PC_MODE_SCAN_CIRCULAR /
 * _GENERIC (pc_trace_kernel.h) or, with option "scan_log" and a plan that can log (pc_plan_launch), pc_trace_log_kernel with those
 * modes (pc_sweep_kernel.h); the mapping of a flat index to its point and the per-point source are pc_scan_map /
 * pc_sample_photon_at of pc_device.h.  Included at the end of pc_kernels.hip.
 */
#ifndef PC_SCAN_H
#define PC_SCAN_H

static_assert(sizeof(pc_scan_point) == sizeof(pc_hip_scan_point), "pc_scan_point mirrors pc_hip_scan_point");

static int pc_scan_check(const char *fn, const pc_hip_scan_point *pts, int64_t n_points, int64_t n_per_point)
{
	const std::string f(fn);
	if (n_points < 1) return pc_fail(PC_HIP_ERR_INVALID, f + ": n_points must be >= 1");
	if (n_per_point < 1) return pc_fail(PC_HIP_ERR_INVALID, f + ": n_per_point must be >= 1");
	if (n_points > INT64_MAX / n_per_point) return pc_fail(PC_HIP_ERR_INVALID, f + ": n_points * n_per_point overflows int64");
	if (!pts) return pc_fail(PC_HIP_ERR_INVALID, f + ": points must not be NULL");
	for (int64_t k = 0; k < n_points; k++) {
		const std::string at = f + ": point " + std::to_string((long long)k) + ": ";
		if (!(pts[k].d_source > 0.)) return pc_fail(PC_HIP_ERR_INVALID, at + "d_source must be greater than 0");
		if (!std::isfinite(pts[k].d_source)) return pc_fail(PC_HIP_ERR_INVALID, at + "d_source must be finite");
		if (!std::isfinite(pts[k].src_shiftx)) return pc_fail(PC_HIP_ERR_INVALID, at + "src_shiftx must be finite");
		if (!std::isfinite(pts[k].src_shifty)) return pc_fail(PC_HIP_ERR_INVALID, at + "src_shifty must be finite");
	}
	return PC_HIP_OK;
}

/* device buffers of a scan of n_points points (the per-lane weights and reflection logs of more than 8 energies: pc_launch_planned) */
int pc_scan_state::buffers(size_t ne, int64_t n_points)
{
	int st = d_totals.grow(1, "pc_hip_scan_run: could not allocate the scan totals");
	if (st) return st;
	PC_HIP_CHECK(ev0.ensure(hipEventDefault));
	PC_HIP_CHECK(ev1.ensure(hipEventDefault));
	st = d_pts.grow((size_t)n_points, "pc_hip_scan_run: could not allocate the point table");
	if (!st) st = d_tot.grow((size_t)n_points*PC_SCAN_STRIDE(ne), "pc_hip_scan_run: could not allocate the per-point totals");
	return st;
}

extern "C" {

int pc_hip_scan_validate(const pc_hip_scan_point *points, int64_t n_points, int64_t n_per_point)
{
	return pc_scan_check("pc_hip_scan_validate", points, n_points, n_per_point);
}

int pc_hip_scan_wait(pc_hip_ctx *ctx, float *kernel_ms)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_wait: ctx must not be NULL");
	if (!ctx->scan.points) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_wait: no scan has been made on this context");
	if (ctx->scan.pending) {
		PC_HIP_CHECK(hipSetDevice(ctx->device));
		PC_HIP_CHECK(hipEventSynchronize(ctx->scan.ev1));
		float ms = 0.f;
		PC_HIP_CHECK(hipEventElapsedTime(&ms, ctx->scan.ev0, ctx->scan.ev1));
		ctx->scan.ms = ms;
		ctx->scan.pending = 0;
	}
	if (kernel_ms) *kernel_ms = ctx->scan.ms;
	return PC_HIP_OK;
}

int pc_hip_scan_run(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, const pc_hip_scan_point *points, int64_t n_points,
                    int64_t n_per_point, int64_t first, int64_t count, uint32_t max_attempts)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_run: ctx must not be NULL");
	int st = pc_scan_check("pc_hip_scan_run", points, n_points, n_per_point);
	if (st) return st;
	if (slot0 < 0) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_run: slot0 must be >= 0");
	if (slot0 > INT64_MAX - n_per_point) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_run: slot0 + n_per_point overflows int64");
	const int64_t total = n_points*n_per_point;
	if (first < 0 || count < 1 || first > total - count)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_run: first and count must select a non-empty range of [0, n_points * n_per_point)");
	if (max_attempts < 1) max_attempts = 1;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	/* the previous scan's kernel may still read the point table and add to the totals that are reused below */
	if (ctx->scan.pending) {
		st = pc_hip_scan_wait(ctx, nullptr);
		if (st) return st;
	}
	ctx->scan.points = 0;       /* until this scan is enqueued */
	ctx->last_call = PC_CALL_SCAN;
	/* behind every launch of the last run: a run cut into parts ends its main stream behind the parts on stream2 already
	 * (pc_hip_transmission_run); this also orders the scan after anything else enqueued there */
	if (ctx->img.stream2) {
		PC_HIP_CHECK(hipEventRecord(ctx->img.ev_sync, ctx->img.stream2));
		PC_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->img.ev_sync, 0));
	}
	const int ne = ctx->host.pm.n_energies;
	st = ctx->scan.buffers((size_t)ne, n_points);
	if (st) return st;
	PC_HIP_CHECK(hipMemcpy(ctx->scan.d_pts, points, (size_t)n_points*sizeof(pc_scan_point), hipMemcpyHostToDevice));
	PC_HIP_CHECK(hipMemsetAsync(ctx->scan.d_totals, 0, sizeof(pc_totals), ctx->stream));
	PC_HIP_CHECK(hipMemsetAsync(ctx->scan.d_tot, 0, (size_t)n_points*PC_SCAN_STRIDE((size_t)ne)*sizeof(unsigned long long), ctx->stream));
	pc_kargs a;
	pc_fill_common(ctx, a);
	a.totals = ctx->scan.d_totals;
	a.work = &ctx->scan.d_totals->next_slot;
	/* the scan's arguments in pc_kargs (PC_SCAN_*): point table, per-point totals, first flat index, slots per point */
	a.in_start = (const double *)ctx->scan.d_pts.p;
	a.sumw = ctx->scan.d_tot;
	a.sumw2 = nullptr;
	a.img_id0 = first;
	a.img_n = n_per_point;
	a.seed = seed; a.slot0 = slot0; a.n_slots = count; a.max_attempts = max_attempts; a.keep_images = 0;
	/* the lane kernel or the logging kernel in its scan mode (pc_plan_launch), between the scan's own events */
	pc_launch_site site{ctx->stream};
	site.record_ev0 = site.record_ev1 = false;
	PC_HIP_CHECK(hipEventRecord(ctx->scan.ev0, ctx->stream));
	st = ctx->host.pm.generic_src ? pc_launch_kernel<PC_MODE_SCAN_GENERIC>(ctx, site, a, count)
	                              : pc_launch_kernel<PC_MODE_SCAN_CIRCULAR>(ctx, site, a, count);
	if (st) return st;
	PC_HIP_CHECK(hipEventRecord(ctx->scan.ev1, ctx->stream));
	ctx->scan.points = n_points;
	ctx->scan.squares = ctx->opts.weight_squares ? 1 : 0;
	ctx->scan.pending = 1;
	return PC_HIP_OK;
}

int pc_hip_scan_last_kernel(pc_hip_ctx *ctx)
{
	return ctx ? ctx->scan.kernel : -1;
}

int pc_hip_group_scan_last_kernel(pc_hip_group *g, int k)
{
	return (g && k >= 0 && (size_t)k < g->ctx.size()) ? g->ctx[(size_t)k]->scan.kernel : -1;
}

int pc_hip_scan_totals(pc_hip_ctx *ctx, int64_t *counters, uint64_t *sumw_fixed, uint64_t *sumw2_fixed)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_totals: ctx must not be NULL");
	if (!ctx->scan.points) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_totals: no scan has been made on this context");
	if (sumw2_fixed && !ctx->scan.squares)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_scan_totals: sumw2_fixed: the last scan was made without option weight_squares");
	int st = pc_hip_scan_wait(ctx, nullptr);
	if (st) return st;
	const size_t ne = (size_t)ctx->host.pm.n_energies, stride = PC_SCAN_STRIDE(ne), P = (size_t)ctx->scan.points;
	std::vector<unsigned long long> buf(P*stride);
	PC_HIP_CHECK(hipMemcpy(buf.data(), ctx->scan.d_tot, buf.size()*sizeof(unsigned long long), hipMemcpyDeviceToHost));
	for (size_t k = 0; k < P; k++) {
		const unsigned long long *t = buf.data() + k*stride;
		if (counters) for (int c = 0; c < PC_N_COUNTERS; c++) counters[PC_N_COUNTERS*k + c] = (int64_t)t[PC_SCAN_COUNTERS + c];
		if (sumw_fixed) std::copy_n(t + PC_SCAN_SUMS, 2*ne, sumw_fixed + 2*ne*k);
		if (sumw2_fixed) std::copy_n(t + PC_SCAN_SQUARES(ne), 2*ne, sumw2_fixed + 2*ne*k);
	}
	return PC_HIP_OK;
}

void pc_hip_scan_efficiencies(size_t n_energies, int64_t n_points, const int64_t *counters, const uint64_t *sumw_fixed,
                              const uint64_t *sumw2_fixed, double *efficiencies, double *stderr_)
{
	std::vector<double> sw(n_energies);
	for (int64_t k = 0; k < n_points; k++) {
		const int64_t *c = counters + 6*k;
		const uint64_t *a = sumw_fixed + 2*n_energies*k;
		double *eff = efficiencies + n_energies*k;
		if (c[0] + c[2] == 0) {
			/* nothing entered a capillary (or nothing was started): efficiency 0 */
			for (size_t e = 0; e < n_energies; e++) eff[e] = 0.;
		} else {
			for (size_t e = 0; e < n_energies; e++) sw[e] = pc_hip_fixed_to_double(a[2*e], a[2*e + 1]);
			pc_hip_efficiencies(n_energies, sw.data(), c, eff);
		}
		if (sumw2_fixed && stderr_)
			pc_hip_efficiency_stderr(n_energies, a, sumw2_fixed + 2*n_energies*k, c, stderr_ + n_energies*k);
	}
}

int pc_hip_group_scan_run(pc_hip_group *g, uint64_t seed, int64_t slot0, const pc_hip_scan_point *points, int64_t n_points,
                          int64_t n_per_point, uint32_t max_attempts)
{
	if (!g) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_run: group must not be NULL");
	int st = pc_scan_check("pc_hip_group_scan_run", points, n_points, n_per_point);
	if (st) return st;
	if (slot0 < 0) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_run: slot0 must be >= 0");
	if (slot0 > INT64_MAX - n_per_point) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_run: slot0 + n_per_point overflows int64");
	const size_t N = g->ctx.size();
	const long long total = n_points*n_per_point;
	g->scan_points = 0;
	g->scan_count.assign(N, 0);
	std::vector<long long> first(N, 0);
	for (size_t k = 0; k < N; k++) {
		/* contiguous ranges that differ by at most one flat index (a range may cut through a point: the sums are exact) */
		const long long lo = (long long)((__int128)total*(long long)k/(long long)N), hi = (long long)((__int128)total*(long long)(k + 1)/(long long)N);
		first[k] = lo; g->scan_count[k] = hi - lo;
	}
	std::vector<int> status(N, PC_HIP_OK);
	std::vector<std::string> msg(N);
	auto enqueue = [&](size_t k) {
		if (g->scan_count[k] == 0) return;
		status[k] = pc_hip_scan_run(g->ctx[k], seed, slot0, points, n_points, n_per_point, first[k], g->scan_count[k], max_attempts);
		if (status[k]) msg[k] = g_last_error;       /* the error text is per thread */
	};
	{
		std::vector<std::thread> th;
		for (size_t k = 1; k < N; k++) th.emplace_back(enqueue, k);
		enqueue(0);
		for (auto &t : th) t.join();
	}
	for (size_t k = 0; k < N; k++) {
		if (status[k] == PC_HIP_OK) continue;
		for (size_t j = 0; j < N; j++)
			if (g->ctx[j]->scan.pending) (void)pc_hip_scan_wait(g->ctx[j], nullptr);
		g->scan_count.assign(N, 0);
		return pc_fail(status[k], msg[k]);
	}
	g->scan_points = n_points;
	return PC_HIP_OK;
}

int pc_hip_group_scan_wait(pc_hip_group *g, float *kernel_ms)
{
	if (!g) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_wait: group must not be NULL");
	if (!g->scan_points) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_wait: no scan has been made on this group");
	float longest = 0.f;
	for (size_t k = 0; k < g->ctx.size(); k++) {
		if (!g->scan_count[k]) continue;
		float ms = 0.f;
		int st = pc_hip_scan_wait(g->ctx[k], &ms);
		if (st) return st;
		longest = std::max(longest, ms);
	}
	if (kernel_ms) *kernel_ms = longest;
	return PC_HIP_OK;
}

int pc_hip_group_scan_totals(pc_hip_group *g, int64_t *counters, uint64_t *sumw_fixed, uint64_t *sumw2_fixed)
{
	if (!g) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_totals: group must not be NULL");
	if (!g->scan_points) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_scan_totals: no scan has been made on this group");
	const size_t P = (size_t)g->scan_points, ne2 = 2*(size_t)g->ctx[0]->host.pm.n_energies;
	std::vector<int64_t> c(6*P), c_sum(6*P, 0);
	std::vector<uint64_t> a(ne2*P), b(sumw2_fixed ? ne2*P : 0);
	std::vector<uint64_t> a_sum(ne2*P, 0), b_sum(sumw2_fixed ? ne2*P : 0, 0);
	for (size_t k = 0; k < g->ctx.size(); k++) {
		if (!g->scan_count[k]) continue;
		int st = pc_hip_scan_totals(g->ctx[k], c.data(), a.data(), sumw2_fixed ? b.data() : nullptr);
		if (st) return pc_fail(st, std::string("pc_hip_group_scan_totals: ") + g_last_error);
		for (size_t i = 0; i < 6*P; i++) c_sum[i] += c[i];
		pc_exact_add_pairs(a_sum.data(), a.data(), ne2/2*P);
		if (sumw2_fixed) pc_exact_add_pairs(b_sum.data(), b.data(), ne2/2*P);
	}
	if (counters) memcpy(counters, c_sum.data(), 6*P*sizeof(int64_t));
	if (sumw_fixed) std::copy(a_sum.begin(), a_sum.end(), sumw_fixed);
	if (sumw2_fixed) std::copy(b_sum.begin(), b_sum.end(), sumw2_fixed);
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_SCAN_H */

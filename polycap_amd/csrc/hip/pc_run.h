/*
 * pc_run.h -- the plain source run of a context (pc_hip_transmission_run, _wait) and every read-back of what a run left: totals,
 * moments, images, slot ids, records, kernel and phase statistics, the sweep certificate; the efficiency formulas and the small
 * device and host helpers of the C-ABI.  Included by pc_kernels.hip.
 */
#ifndef PC_RUN_H
#define PC_RUN_H

extern "C" {

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
	if (ct_tame) *ct_tame = ctx->cert.known ? ctx->cert.ct_tame : -1.;
	if (proxies) { proxies[0] = ctx->cert.known ? ctx->cert.proxy_e[0] : -1; proxies[1] = (ctx->cert.known && ctx->cert.n_proxy > 1) ? ctx->cert.proxy_e[1] : -1; }
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

#endif /* PC_RUN_H */

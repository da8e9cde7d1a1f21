/*
 * pc_leak_run.h -- the host side of leak_calc=true runs: one owner (pc_leak_run, held as pc_hip_ctx::leak) of their buffers,
 * options and the run in flight, and the C calls that start a leak run and read its events.  What it decides -- grid, record
 * capacity, the order of the slots -- it asks pc_leak_plan.h; the kernels are in pc_leak_kernels.h.  Included twice by
 * pc_kernels.hip, the only header that is: the struct before the context that holds it (pc_ctx.h), and everything that needs
 * the context, the launch code (pc_launch.h) and the kernels once pc_leak_kernels.h has been included.
 */
#ifndef PC_LEAK_RUN_H
#define PC_LEAK_RUN_H

#include "pc_leak_plan.h"

struct pc_hip_ctx;
struct pc_kargs;

/* one of the two event lists of the last leak run, on the device and in pinned host memory */
struct pc_leak_list { const double *dev, *host; long long n; };

struct pc_leak_run {
	/* ---- options (pc_hip_set_option) */
	struct {
		int max_depth = 0;                 /* frames per lane; default 2*n_shells + 16 (one frame per wall crossed) */
		size_t stack_bytes = (size_t)8 << 30;
		long long capacity = 0;            /* record buffer size of the next run; 0 = 16 + 8 n_energies per slot, grown on demand */
		int order = 1;                     /* 1 = source runs of two to five slots per lane order their slots by a plain pre-pass, 0 = slot order */
		int slot_units = 0;                /* keep the units of work per slot of leak runs (pc_hip_leak_slot_units) */
		int heavy_lanes = 1, heavy_every = 1;
	} opts;
	/* ---- buffers */
	pc_dev_buf<double> d_frames;
	pc_dev_buf<double> d_records;
	pc_dev_buf<unsigned long long> d_cursor;
	pc_dev_buf<double> d_amu;              /* copied when it is allocated, once */
	pc_dev_buf<unsigned int> d_attempts;
	pc_dev_buf<unsigned long long> d_timing; /* POLYCAP_LEAK_TIMING diagnostics */
	long long timing_waves = 0;
	pc_dev_buf<unsigned int> d_order;      /* order in which the next leak run hands out its slots (pc_hip_leak_set_order, auto_order); empty: none */
	pc_dev_buf<unsigned int> d_work_est;   /* what the plain pre-pass predicts per slot */
	pc_dev_buf<unsigned int> d_slot_units;
	pc_dev_buf<char> d_order_tmp;
	/* events of the last leak run in the reference's list order, PC_HIP_LEAK_HDR + n_energies doubles each: the extleak list, then
	 * the intleak list, ordered on the device (collect) and kept in pinned host memory */
	pc_dev_buf<double> d_out;
	pc_host_buf<double, PC_PIN_ONLY> h_out;
	/* ---- the run in flight */
	unsigned long long seed = 0;
	long long slot0 = 0, n_slots = 0;
	unsigned int max_attempts = 0;
	int keep_images = 0;
	long long capacity_used = 0;
	bool timing = false;                   /* POLYCAP_LEAK_TIMING was set when the run started */
	int ev0_done = 0;                      /* ev0 of the run in flight was recorded before its pre-pass */
	/* ---- the order of the slots */
	int order_user = 0;                    /* the order was set by the caller */
	long long order_n = 0, n_heavy = 0;
	unsigned long long order_seed = 0; long long order_slot0 = -1; unsigned int order_attempts = 0;   /* what the automatic order was made for */
	/* ---- what the last run left */
	int pending = 0;                       /* a leak transmission run is in flight: wait() collects its events */
	int events_of_run = 0;                 /* the event lists are those of the last source run (a leak run): tallies may read them */
	long long n_ext = 0, n_int = 0;

	/* which: 0 = the extleak list, 1 = the intleak list behind it (the `kind` of the C calls) */
	pc_leak_list list(int which, size_t n_energies) const
	{
		const size_t off = which == 0 ? 0 : (size_t)n_ext*(PC_HIP_LEAK_HDR + n_energies);
		return pc_leak_list{d_out + off, h_out + off, which == 0 ? n_ext : n_int};
	}
	void begin(long long n, long long first_capacity)
	{
		n_slots = n; capacity_used = first_capacity; ev0_done = 0;
		timing = getenv("POLYCAP_LEAK_TIMING") != nullptr;
	}
	void drop_order() { order_n = 0; order_slot0 = -1; }
	int buffers(pc_hip_ctx &ctx, long long lanes);
	template <int MODE> int enqueue(pc_hip_ctx &ctx, pc_kargs &a);
	int enqueue_source(pc_hip_ctx &ctx);
	int collect(pc_hip_ctx &ctx, bool explicit_mode, long long *needed);
	int auto_order(pc_hip_ctx &ctx);
	int run_until_fit(pc_hip_ctx &ctx, pc_kargs *explicit_args);
};

#endif /* PC_LEAK_RUN_H */

/* ---- the second pass: behind the context, the launch code and the leak kernels */
#if defined(PC_LEAK_KERNELS_H) && !defined(PC_LEAK_RUN_BODY_H)
#define PC_LEAK_RUN_BODY_H

static pc_leak_grid pc_leak_grid_of(const pc_hip_ctx &ctx, long long n_items)
{
	return pc_plan_leak_grid(n_items, ctx.host.pm.n_energies, ctx.leak.opts.max_depth, ctx.leak.opts.stack_bytes, ctx.n_cu);
}

int pc_leak_run::buffers(pc_hip_ctx &ctx, long long lanes)
{
	const size_t ne = (size_t)ctx.host.pm.n_energies;
	const size_t frames = (size_t)lanes * (size_t)opts.max_depth * (PC_LF_HDR + ne);
	int st = d_frames.grow(frames, "leak run: could not allocate the per-lane stacks (lower leak_stack_mb or leak_max_depth)");
	if (!st) st = d_records.grow((size_t)capacity_used * (PC_LR_HDR + ne), "leak run: could not allocate the leak record buffer");
	if (!st) st = d_cursor.grow(4, "leak run: could not allocate the record cursor");
	if (!st && !d_amu) {
		st = d_amu.grow(ne, "leak run: could not allocate the attenuation table");
		if (!st) PC_HIP_CHECK(hipMemcpy(d_amu, ctx.host.amu.data(), ne*sizeof(double), hipMemcpyHostToDevice));
	}
	if (!st) st = d_attempts.grow((size_t)n_slots, "leak run: could not allocate the per-slot attempt table");
	return st;
}

/* one launch of the run in flight (begin) over its n_slots items with a record buffer of capacity_used, between the context's events */
template <int MODE>
int pc_leak_run::enqueue(pc_hip_ctx &ctx, pc_kargs &a)
{
	const pc_leak_grid g = pc_leak_grid_of(ctx, n_slots);
	int st = buffers(ctx, g.lanes);
	if (st) return st;
	pc_leak_kargs lk;
	lk.amu = d_amu; lk.frames = d_frames; lk.max_depth = opts.max_depth;
	lk.records = d_records; lk.cursor = d_cursor; lk.capacity = capacity_used;
	lk.final_attempt = d_attempts;
	lk.timing = nullptr;
	lk.order = nullptr; lk.n_heavy = 0; lk.heavy_lanes = 0; lk.heavy_every = 0; lk.slot_units = nullptr;
	if (MODE != PC_MODE_EXPLICIT) {
		if (d_order && order_n == n_slots) {
			lk.order = d_order;
			lk.heavy_lanes = opts.heavy_lanes; lk.heavy_every = opts.heavy_every;
			lk.n_heavy = (lk.heavy_lanes > 0 && lk.heavy_every > 0) ? std::min<long long>(n_heavy, n_slots) : 0;
		}
		if (opts.slot_units) {
			st = d_slot_units.grow((size_t)n_slots, "leak run: could not allocate the units of work per slot");
			if (st) return st;
			PC_HIP_CHECK(hipMemsetAsync(d_slot_units, 0, (size_t)n_slots*sizeof(unsigned int), ctx.stream));
			lk.slot_units = d_slot_units;
		}
	}
	if (timing) {
		/* diagnostics: where the waves of the leak kernel spend their time (printed by collect) */
		const size_t nb = (size_t)(g.lanes / PC_WAVE) * 8 * sizeof(unsigned long long);
		st = d_timing.grow(nb/sizeof(unsigned long long), "leak run: could not allocate the timing records");
		if (st) return st;
		PC_HIP_CHECK(hipMemsetAsync(d_timing, 0, nb, ctx.stream));
		lk.timing = d_timing;
		timing_waves = g.lanes / PC_WAVE;
	}
	a.total_threads = g.lanes;
	PC_HIP_CHECK(hipMemsetAsync(d_cursor, 0, 4*sizeof(unsigned long long), ctx.stream));
	PC_HIP_CHECK(hipMemsetAsync(ctx.d_totals, 0, ctx.totals_bytes, ctx.stream));
	if (!ev0_done) PC_HIP_CHECK(hipEventRecord(ctx.ev0, ctx.stream));
	/* option "weight_squares": kernels of their own (SQ), so that the default kernels keep their registers */
	constexpr bool CAN_SQ = MODE != PC_MODE_EXPLICIT;
	const bool sq = CAN_SQ && a.sumw2 != nullptr;
	if (ctx.host.pm.nmax + 1 <= 1024) {
		if (sq) hipLaunchKernelGGL((pc_leak_kernel<MODE, 1024, CAN_SQ>), dim3(g.blocks), dim3(PC_LEAK_BLOCK), 0, ctx.stream, a, lk);
		else hipLaunchKernelGGL((pc_leak_kernel<MODE, 1024>), dim3(g.blocks), dim3(PC_LEAK_BLOCK), 0, ctx.stream, a, lk);
	} else {
		if (sq) hipLaunchKernelGGL((pc_leak_kernel<MODE, PC_MAX_PITCH, CAN_SQ>), dim3(g.blocks), dim3(PC_LEAK_BLOCK), 0, ctx.stream, a, lk);
		else hipLaunchKernelGGL((pc_leak_kernel<MODE, PC_MAX_PITCH>), dim3(g.blocks), dim3(PC_LEAK_BLOCK), 0, ctx.stream, a, lk);
	}
	PC_HIP_CHECK(hipGetLastError());
	ctx.last_kernel = 5;
	PC_HIP_CHECK(hipEventRecord(ctx.ev1, ctx.stream));
	return PC_HIP_OK;
}

/* the launch of a source run (pc_hip_transmission_run_leak), and its repetitions */
int pc_leak_run::enqueue_source(pc_hip_ctx &ctx)
{
	pc_kargs a;
	pc_fill_common(&ctx, a);
	ctx.img.set_img(a, keep_images ? PC_IMG_RECORDS : PC_IMG_NONE, n_slots, 0);
	a.seed = seed; a.slot0 = slot0; a.n_slots = n_slots;
	a.max_attempts = max_attempts; a.keep_images = keep_images;
	return ctx.host.pm.generic_src ? enqueue<PC_MODE_SRC_GENERIC>(ctx, a) : enqueue<PC_MODE_SRC_CIRCULAR>(ctx, a);
}

/* The launch that was enqueued has ended: fetch and order its events; a launch that outgrew the record buffer is repeated with a
 * larger one until every event fits (the photon streams are counter-based, so the repetition is the same run).  explicit_args: the
 * arguments of an explicit-photon launch, null for a source run. */
int pc_leak_run::run_until_fit(pc_hip_ctx &ctx, pc_kargs *explicit_args)
{
	for (;;) {
		long long needed = 0;
		int st = collect(ctx, explicit_args != nullptr, &needed);
		if (st != 1) return st;
		capacity_used = pc_plan_leak_grown(needed);
		st = explicit_args ? enqueue<PC_MODE_EXPLICIT>(ctx, *explicit_args) : enqueue_source(ctx);
		if (st) return st;
		PC_HIP_CHECK(hipStreamSynchronize(ctx.stream));
	}
}

static void pc_leak_print_timing(const std::vector<unsigned long long> &t, size_t nw)
{
	double sum[8] = {0}, mx[8] = {0}; size_t ran = 0;
	unsigned long long t0 = ~0ull, t1 = 0;
	for (size_t w = 0; w < nw; w++) {
		if (t[w*8+5] == 0) continue;
		ran++;
		for (int k = 0; k < 7; k++) { sum[k] += (double)t[w*8+k]; if ((double)t[w*8+k] > mx[k]) mx[k] = (double)t[w*8+k]; }
		if (t[w*8+7] < t0) t0 = t[w*8+7];
		if (t[w*8+7] + t[w*8+5] > t1) t1 = t[w*8+7] + t[w*8+5];
	}
	std::vector<unsigned long long> life;
	for (size_t w = 0; w < nw; w++) if (t[w*8+5]) life.push_back(t[w*8+5]);
	std::sort(life.begin(), life.end());
	const double tick = 1e-5;     /* wall_clock64: 100 MHz -> ms */
	fprintf(stderr, "leak timing: %zu waves ran; span %.1f ms; per wave mean (max) in ms: wall %.1f (%.1f) probe %.1f (%.1f) march %.1f (%.1f) other %.1f (%.1f) driver %.1f (%.1f) | life %.1f (%.1f) median %.1f p90 %.1f | first idle lane after %.1f (%.1f)\n",
	        ran, (double)(t1 - t0)*tick, sum[0]/ran*tick, mx[0]*tick, sum[1]/ran*tick, mx[1]*tick, sum[2]/ran*tick, mx[2]*tick, sum[3]/ran*tick, mx[3]*tick,
	        sum[4]/ran*tick, mx[4]*tick, sum[5]/ran*tick, mx[5]*tick, life.empty() ? 0. : (double)life[life.size()/2]*tick, life.empty() ? 0. : (double)life[life.size()*9/10]*tick,
	        sum[6]/ran*tick, mx[6]*tick);
}

/* ---------------------------------------------------------------------------------------------------------------------
 * The events of a finished run, put into the two lists of the reference (src/polycap-source.c:799-879) ON THE DEVICE: attempts
 * that appended a VOID record are dropped, the rest is ordered by slot, inside a slot the transmitted attempt first and then the
 * earlier attempts in attempt order, inside an attempt by seq; extleak and intleak events go to lists of their own in that
 * order.  Round 3 fetched the raw records (120 B each) and did this with host threads: 243 ms for the 2.46e6 events of the leak
 * bench, more than the kernel.  Now: keys -> two stable radix sorts (seq, then (slot, order)) -> flags and positions (prefix sums)
 * -> one gather into the output rows (PC_HIP_LEAK_HDR + n_energies doubles), which are copied once into pinned host memory.
 *
 * Orders the event records of the finished launch on the device and brings the two lists to the host (pinned memory, kept by the
 * owner until its next leak run).  Returns PC_HIP_OK, or 1 when the record buffer was too small (*needed = records the launch
 * produced). */
int pc_leak_run::collect(pc_hip_ctx &ctx, bool explicit_mode, long long *needed)
{
	unsigned long long cur[2] = {0, 0};
	PC_HIP_CHECK(hipMemcpy(cur, d_cursor, sizeof(cur), hipMemcpyDeviceToHost));
	if (timing) {
		const size_t nw = (size_t)timing_waves;
		std::vector<unsigned long long> t(nw*8);
		PC_HIP_CHECK(hipMemcpy(t.data(), d_timing, nw*8*sizeof(unsigned long long), hipMemcpyDeviceToHost));
		pc_leak_print_timing(t, nw);
	}
	n_ext = n_int = 0;
	if (cur[1] != 0)
		return pc_fail(PC_HIP_ERR_RUNTIME, "leak run: the chain of wall crossings was deeper than leak_max_depth for " + std::to_string(cur[1]) + " lane(s); raise the option leak_max_depth");
	if ((long long)cur[0] > capacity_used) { *needed = (long long)cur[0]; return 1; }
	const size_t ne = (size_t)ctx.host.pm.n_energies, stride = PC_LR_HDR + ne, ostride = PC_HIP_LEAK_HDR + ne, n = (size_t)cur[0];
	if (n == 0) return PC_HIP_OK;
	if (n >= (1ull << 31) - 2) return pc_fail(PC_HIP_ERR_INVALID, "leak run: more than 2^31 event records in one run (the sorts count in int); trace the slots in several runs");
	hipStream_t st = ctx.stream;
	const int end_bit = 64;
	/* temporary storage of the library calls: the largest of the three sorts and the prefix sum */
	size_t tb = 0, t1 = 0;
	PC_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, (const unsigned int *)nullptr, (unsigned int *)nullptr, (const unsigned int *)nullptr, (unsigned int *)nullptr, (int)n, 0, 32, st)); tb = std::max(tb, t1);
	PC_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const unsigned int *)nullptr, (unsigned int *)nullptr, (int)n, 0, end_bit, st)); tb = std::max(tb, t1);
	PC_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, t1, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)n, 0, end_bit, st)); tb = std::max(tb, t1);
	PC_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (const unsigned int *)nullptr, (unsigned int *)nullptr, (int)n + 1, st)); tb = std::max(tb, t1);
	{
		/* keys n x 8 x 3, seq n x 4 x 2, idx n x 4 x 3, flags + positions (n + 1) x 4 x 4, void keys n x 8 x 2, counters */
		const size_t need = n*8*3 + n*4*2 + n*4*3 + (n + 1)*4*4 + n*8*2 + 256 + tb + 4096;
		int rc = d_order_tmp.grow(need, "leak run: could not allocate the ordering buffers");
		const size_t out_elems = n*ostride;
		if (!rc) rc = d_out.grow(out_elems, "leak run: could not allocate the event lists", out_elems + out_elems/8);
		if (!rc) rc = h_out.grow(out_elems, "leak run: could not allocate the event lists", out_elems + out_elems/8);
		if (rc) return rc;
	}
	char *base = (char *)d_order_tmp;
	auto take = [&](size_t bytes) { char *p = base; base += (bytes + 255) & ~(size_t)255; return (void *)p; };
	unsigned long long *key = (unsigned long long *)take(n*8), *key2 = (unsigned long long *)take(n*8), *key3 = (unsigned long long *)take(n*8);
	unsigned int *seq = (unsigned int *)take(n*4), *seq2 = (unsigned int *)take(n*4);
	unsigned int *idx = (unsigned int *)take(n*4), *idx2 = (unsigned int *)take(n*4), *idx3 = (unsigned int *)take(n*4);
	unsigned int *f_ext = (unsigned int *)take((n + 1)*4), *f_int = (unsigned int *)take((n + 1)*4), *p_ext = (unsigned int *)take((n + 1)*4), *p_int = (unsigned int *)take((n + 1)*4);
	unsigned long long *vk = (unsigned long long *)take(n*8), *vk2 = (unsigned long long *)take(n*8);
	unsigned int *cnt = (unsigned int *)take(64);       /* [0] void records, [1] records with a slot or attempt outside the run */
	void *tmp = take(tb);
	const unsigned blocks = (unsigned)((n + 255)/256);
	PC_HIP_CHECK(hipMemsetAsync(cnt, 0, 64, st));
	hipLaunchKernelGGL(pc_leak_keys_kernel, dim3(blocks), dim3(256), 0, st, d_records, (long long)stride, (long long)n, (long long)slot0, n_slots,
	                   explicit_mode ? (const unsigned int *)nullptr : d_attempts, key, seq, idx, vk, cnt, cnt + 1);
	PC_HIP_CHECK(hipGetLastError());
	unsigned int hc[2] = {0, 0};
	PC_HIP_CHECK(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, st));
	PC_HIP_CHECK(hipStreamSynchronize(st));
	if (hc[1]) return pc_fail(PC_HIP_ERR_RUNTIME, "leak run: event record with a slot or attempt outside the run");
	if (hc[0]) PC_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(tmp, tb, vk, vk2, (int)hc[0], 0, end_bit, st));
	/* stable sorts: by seq, then by (slot, order) */
	PC_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, seq, seq2, idx, idx2, (int)n, 0, 32, st));
	hipLaunchKernelGGL(pc_leak_gather_keys_kernel, dim3(blocks), dim3(256), 0, st, key, idx2, (long long)n, key2);
	PC_HIP_CHECK(hipGetLastError());
	PC_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key2, key3, idx2, idx3, (int)n, 0, end_bit, st));
	hipLaunchKernelGGL(pc_leak_flags_kernel, dim3((unsigned)((n + 1 + 255)/256)), dim3(256), 0, st, d_records, (long long)stride, key3, idx3, (long long)n,
	                   hc[0] ? vk2 : vk, cnt, f_ext, f_int);
	PC_HIP_CHECK(hipGetLastError());
	PC_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, f_ext, p_ext, (int)n + 1, st));
	PC_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, f_int, p_int, (int)n + 1, st));
	const unsigned long long cells = (unsigned long long)n*ostride;
	hipLaunchKernelGGL(pc_leak_rows_kernel, dim3((unsigned)((cells + 255)/256)), dim3(256), 0, st, d_records, (long long)stride, idx3, (long long)n, (int)ne,
	                   f_ext, f_int, p_ext, p_int, d_out);
	PC_HIP_CHECK(hipGetLastError());
	unsigned int tot[2] = {0, 0};
	PC_HIP_CHECK(hipMemcpyAsync(&tot[0], p_ext + n, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	PC_HIP_CHECK(hipMemcpyAsync(&tot[1], p_int + n, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
	PC_HIP_CHECK(hipStreamSynchronize(st));
	const size_t rows = (size_t)tot[0] + (size_t)tot[1];
	if (rows) PC_HIP_CHECK(hipMemcpyAsync(h_out, d_out, rows*ostride*sizeof(double), hipMemcpyDeviceToHost, st));
	PC_HIP_CHECK(hipStreamSynchronize(st));
	n_ext = (long long)tot[0];
	n_int = (long long)tot[1];
	return PC_HIP_OK;
}

/* Heaviest slots first.  A leak launch ends with its longest slot: 20 000 units of work on one lane, which advances several
 * times faster alone in its wave than among 63 others (a wave runs one class of work at a time).  Which slots are long is known
 * beforehand to a good approximation (correlation 0.95 with the units of the leak run, scripts/analysis/leak_units.py): a plain
 * run of the same slots -- the same photons without their leaks, a hundredth of the leak run's time -- counts the reflections
 * of every attempt per slot.  The slots are then handed out in descending order of that count, the first n/400 of them to lane
 * 0 of the waves, whose other lanes wait while such a slot is at work (pc_leak_kargs::order).  The results do not depend on the
 * order (photon streams are keyed by slot and attempt, events are ordered by slot on the host). */
int pc_leak_run::auto_order(pc_hip_ctx &ctx)
{
	const long long n = n_slots;
	if (order_user) return PC_HIP_OK;                                 /* the caller's order (used if it is for n slots) */
	const long long lanes = pc_leak_grid_of(ctx, n).lanes;
	if (!pc_plan_leak_order_considered(opts.order != 0, n, lanes)) {
		d_order.reset();
		drop_order();
		return PC_HIP_OK;
	}
	if (d_order && order_n == n && order_seed == seed && order_slot0 == slot0 && order_attempts == max_attempts)
		return PC_HIP_OK;                                               /* the same slots as last time */
	int st = d_work_est.grow((size_t)n, "leak run: could not allocate the work estimate");
	if (st) return st;
	const auto t_0 = std::chrono::steady_clock::now();
	/* the time of the launch starts here */
	PC_HIP_CHECK(hipEventRecord(ctx.ev0, ctx.stream));
	ev0_done = 1;
	PC_HIP_CHECK(hipMemsetAsync(d_work_est, 0, (size_t)n*sizeof(unsigned int), ctx.stream));
	PC_HIP_CHECK(hipMemsetAsync(ctx.d_totals, 0, ctx.totals_bytes, ctx.stream));
	pc_kargs a;
	pc_fill_common(&ctx, a);
	a.seed = seed; a.max_attempts = max_attempts; a.keep_images = 0;
	a.slot0 = slot0; a.n_slots = n;
	a.work_est = d_work_est;
	pc_launch_site site{ctx.stream};      /* the lane kernel, no events of its own */
	site.record_ev0 = site.record_ev1 = false;
	site.force_lane = true;
	st = ctx.host.pm.generic_src ? pc_launch_kernel<PC_MODE_SRC_GENERIC>(&ctx, site, a, n) : pc_launch_kernel<PC_MODE_SRC_CIRCULAR>(&ctx, site, a, n);
	if (st) return st;
	std::vector<unsigned int> est((size_t)n), order;
	PC_HIP_CHECK(hipMemcpyAsync(est.data(), d_work_est, (size_t)n*sizeof(unsigned int), hipMemcpyDeviceToHost, ctx.stream));
	PC_HIP_CHECK(hipStreamSynchronize(ctx.stream));
	const auto t_1 = std::chrono::steady_clock::now();
	const pc_leak_order_plan p = pc_plan_leak_order(est.data(), n, lanes, ctx.n_cu, order);
	if (!p.ordered) {
		drop_order();                                                   /* the buffer stays for the next run; it is not used */
		if (timing) fprintf(stderr, "leak order: slot order kept (longest slot %u of %llu predicted units, %lld lanes)\n", p.top, p.total, lanes);
		return PC_HIP_OK;
	}
	const auto t_2 = std::chrono::steady_clock::now();
	st = d_order.grow((size_t)n, "leak run: could not allocate the slot order");
	if (st) return st;
	PC_HIP_CHECK(hipMemcpyAsync(d_order, order.data(), (size_t)n*sizeof(unsigned int), hipMemcpyHostToDevice, ctx.stream));
	PC_HIP_CHECK(hipStreamSynchronize(ctx.stream));      /* `order` leaves scope */
	if (timing) {
		const auto t_3 = std::chrono::steady_clock::now();
		auto ms = [](auto x, auto y) { return std::chrono::duration<double, std::milli>(y - x).count(); };
		fprintf(stderr, "leak order: plain pre-pass + copy %.2f ms, sort %.2f ms, upload %.2f ms\n", ms(t_0, t_1), ms(t_1, t_2), ms(t_2, t_3));
	}
	order_n = n; n_heavy = p.n_heavy;
	order_seed = seed; order_slot0 = slot0; order_attempts = max_attempts;
	return PC_HIP_OK;
}

extern "C" {

int pc_hip_transmission_run_leak(pc_hip_ctx *ctx, uint64_t seed, int64_t slot0, int64_t n_slots, uint32_t max_attempts, int keep_images)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_run_leak: ctx must not be NULL");
	if (n_slots < 1 || slot0 < 0) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_run_leak: n_slots must be >= 1 and slot0 >= 0");
	if (max_attempts < 1) max_attempts = 1;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	ctx->img.reset();
	ctx->entries_epoch++;
	ctx->last_call = PC_CALL_RUN_LEAK;
	if (keep_images) {
		int st = ctx->img.keep_records(n_slots, "pc_hip_transmission_run_leak: could not allocate the image planes; use keep_images=0");
		if (st) return st;
	}
	ctx->last_run_plain = 0;
	ctx->run_squares = ctx->opts.weight_squares;
	pc_leak_run &L = ctx->leak;
	L.events_of_run = 1;
	L.seed = seed; L.slot0 = slot0; L.max_attempts = max_attempts; L.keep_images = keep_images ? 1 : 0;
	L.begin(n_slots, pc_plan_leak_capacity(L.opts.capacity, ctx->host.pm.n_energies, n_slots, 65536));
	int status = L.auto_order(*ctx);
	if (status) return status;
	status = L.enqueue_source(*ctx);
	if (status) return status;
	ctx->run_slots = n_slots;
	ctx->run_pending = 1;
	L.pending = 1;
	ctx->img.valid = keep_images ? 1 : 0;
	return PC_HIP_OK;
}

int pc_hip_leak_counts(pc_hip_ctx *ctx, int64_t *n_ext, int64_t *n_int)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_counts: ctx must not be NULL");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	if (n_ext) *n_ext = ctx->leak.n_ext;
	if (n_int) *n_int = ctx->leak.n_int;
	return PC_HIP_OK;
}

int pc_hip_leak_events(pc_hip_ctx *ctx, int kind, int64_t first, int64_t count, double *records)
{
	if (!ctx || (count > 0 && !records)) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_events: NULL argument");
	if (kind != 0 && kind != 1) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_events: kind must be 0 (extleak) or 1 (intleak)");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	const size_t ne = (size_t)ctx->host.pm.n_energies, stride = PC_HIP_LEAK_HDR + ne;
	const pc_leak_list l = ctx->leak.list(kind, ne);
	if (first < 0 || count < 0 || first + count > l.n) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_events: range out of bounds");
	if (count) memcpy(records, l.host + (size_t)first*stride, (size_t)count*stride*sizeof(double));
	return PC_HIP_OK;
}

int pc_hip_leak_events_view(pc_hip_ctx *ctx, int kind, const double **records, int64_t *count)
{
	if (!ctx || !records || !count) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_events_view: NULL argument");
	if (kind != 0 && kind != 1) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_events_view: kind must be 0 (extleak) or 1 (intleak)");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	const pc_leak_list l = ctx->leak.list(kind, (size_t)ctx->host.pm.n_energies);
	*count = l.n;
	*records = (l.n > 0) ? l.host : nullptr;
	return PC_HIP_OK;
}

int pc_hip_leak_set_order(pc_hip_ctx *ctx, const uint32_t *order, int64_t n, int64_t n_heavy)
{
	if (!ctx || n < 0 || (n > 0 && !order) || n_heavy < 0) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_set_order: invalid argument");
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	pc_leak_run &L = ctx->leak;
	L.d_order.reset();
	L.drop_order(); L.n_heavy = 0; L.order_user = 0;
	if (n == 0) return PC_HIP_OK;
	{
		/* a permutation of 0 .. n-1, or slots would be traced twice or not at all */
		std::vector<unsigned char> seen((size_t)n, 0);
		for (int64_t k = 0; k < n; k++) {
			if ((int64_t)order[k] >= n || seen[order[k]]) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_set_order: order is not a permutation of the slots");
			seen[order[k]] = 1;
		}
	}
	st = L.d_order.grow((size_t)n, "pc_hip_leak_set_order: could not allocate the order");
	if (st) return st;
	PC_HIP_CHECK(hipMemcpy(L.d_order, order, (size_t)n*sizeof(unsigned int), hipMemcpyHostToDevice));
	L.order_n = n; L.n_heavy = n_heavy; L.order_user = 1;
	return PC_HIP_OK;
}

int pc_hip_leak_slot_units(pc_hip_ctx *ctx, int64_t first, int64_t count, uint32_t *units)
{
	if (!ctx || (count > 0 && !units) || first < 0 || count < 0) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_slot_units: invalid argument");
	int st = pc_hip_transmission_wait(ctx, nullptr);
	if (st) return st;
	const pc_dev_buf<unsigned int> &u = ctx->leak.d_slot_units;
	if (!u || (size_t)(first + count) > u.cap) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_leak_slot_units: no leak run with the option leak_slot_units covers this range");
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	if (count) PC_HIP_CHECK(hipMemcpy(units, u + first, (size_t)count*sizeof(unsigned int), hipMemcpyDeviceToHost));
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_LEAK_RUN_BODY_H */

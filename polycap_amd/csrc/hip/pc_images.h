/*
 * pc_images.h -- the exit-photon images of a context's last run: one owner (pc_image_store), three layouts, one way out.
 *
 *   records   one record of 17 + n_energies doubles per slot (d_img).  Written by the trace kernels (option "plane_images" 0),
 *             by leak runs and by a relay's finish kernel; fetched through the staging pipeline, or turned into planes behind
 *             the trace (pc_soa_kernel) when planes are asked for.
 *   planes    17 planes of the run's n_slots doubles, then the weights [slot][n_energies] (d_soa), a photon at its slot.  Written
 *             by the trace kernels (option "plane_images"); copied straight into the caller's pinned planes, part by part.
 *   compact   the same planes with photons in their order of completion, published block by block while the kernel runs
 *             (option "compact_images"); copied group of blocks by group of blocks.
 * Readers on the device (the tallies of pc_tally.h, the relay, the slot ids) take pc_image_store::device_view().
 *
 * Two halves.  The pure one -- what a run stores and in how many launches (pc_plan_images), where an element lies
 * (pc_layout_of), which positions a group of blocks holds (pc_block_span), the caller's planes in field order (pc_image_planes) --
 * works on plain values and compiles for the host (tests/plan/images_host.cpp).  The store and the fetch, with the two kernels
 * they launch, need the owner types (pc_host.h) and pc_kargs (pc_kargs.h) and are for hipcc alone.  pc_kernels.hip includes the
 * header once, ahead of the trace kernels, which use the record fields.
 */
#ifndef PC_IMAGES_H
#define PC_IMAGES_H

#include <algorithm>
#include <cstddef>

#include "polycap-hip.h"

/* Per-exit-photon image record in HBM: one contiguous record per slot (17 + n_energies doubles) so that a lane
 * writes whole 64/128-byte segments instead of 18 scattered 8-byte words.
 * Field order = pc_hip_images / the reference's plane order. */
enum { PC_F_SRCX = 0, PC_F_SRCY, PC_F_STARTX, PC_F_STARTY, PC_F_SDIRX, PC_F_SDIRY, PC_F_SEVX, PC_F_SEVY,
       PC_F_EXITX, PC_F_EXITY, PC_F_EXITZ, PC_F_EDIRX, PC_F_EDIRY, PC_F_EEVX, PC_F_EEVY, PC_F_NREFL, PC_F_DTRAVEL,
       PC_F_WEIGHTS, PC_N_FIELDS = 17 };

#define PC_MAX_PARTS 16

/* ---- the options the store reads (pc_hip_set_option writes them) */
struct pc_image_opts {
	int plane_images = 0;          /* option "plane_images": runs that keep images write the planes themselves (no records) */
	/* option "compact_images" (with plane_images): exit photons are stored in the order of completion, one coalesced run per
	 * plane and batch, and the planes are published block by block while the kernel runs (pc_kargs::img_cursor) */
	int compact_images = 0;
	int compact_parts = 1;         /* option "compact_parts": launches a compact run of 4e6 slots or more is traced in (alternating between two
	                                * streams, each with its own half of the per-lane scratch: pc_launch_site).  Measured, not adopted: 2 launches 20.95 ms against 19.6 ms for one (1e7 slots; profiles/r04/kernel_history.md) */
	int slot_ids = 0;              /* option "slot_ids": compact runs also store which slot sits at which position */
	int blk_shift = 16;            /* option "block_shift": published blocks of 2^blk_shift positions (65536: 512 KB per plane; the fetch
	                                * copies all the blocks that are complete at a time in one go) */
	/* a transmission run can be cut into parts (kernel launches over consecutive slot ranges, same totals): the images of
	 * a finished part are fetched while the next part is traced */
	int run_parts = 1;
	int fetch_threads = 0;         /* host threads that scatter a fetched chunk into the caller's planes; 0 = min(16, cores) */
	int keep_pinned = 0;           /* option "keep_pinned": pc_hip_transmission_images leaves the destination planes pinned */
	int dst_prepinned = 0;         /* the caller (a device group) has pinned the destination planes itself: the fetch pins nothing */
};

/* First slot of part k of `parts`.  The fetch of the images can start when the first part is done and has the last part
 * left when the kernel ends, so with three or more parts the first and the last are half the size of the others. */
static long long pc_part_begin(long long n_slots, int parts, int k)
{
	if (k <= 0) return 0;
	if (k >= parts) return n_slots;
	if (parts < 3) return n_slots*k/parts;
	const double unit = 1.0/(double)(parts - 1);           /* 1/2 + (parts - 2) + 1/2 units */
	return (long long)((double)n_slots*unit*((double)k - 0.5));
}

/* ---- what a run stores, and in how many launches */
enum { PC_IMG_NONE = 0, PC_IMG_RECORDS, PC_IMG_PLANES, PC_IMG_COMPACT };
struct pc_image_plan {
	int layout = PC_IMG_NONE;
	long long n_slots = 0;
	size_t elems = 0;              /* doubles of the layout's buffer */
	int parts = 1;                 /* launches: part k traces slots [begin[k], begin[k + 1]) */
	int fetch_parts = 1;           /* what the fetch goes by: a compact run is fetched block by block whatever its launches */
	int halves = 1;                /* launches in flight at the same time (parts on two streams) must not share per-lane scratch: two halves of it */
	long long begin[PC_MAX_PARTS + 1] = {0};
	int blk_shift = 16;            /* compact: blocks of 2^blk_shift positions, `blocks` of them */
	long long blocks = 0;
};

static pc_image_plan pc_plan_images(long long n_slots, int ne, bool keep_images, const pc_image_opts &o)
{
	pc_image_plan p;
	const bool planes = keep_images && o.plane_images, compact = planes && o.compact_images;
	p.layout = !keep_images ? PC_IMG_NONE : compact ? PC_IMG_COMPACT : planes ? PC_IMG_PLANES : PC_IMG_RECORDS;
	p.n_slots = n_slots;
	p.elems = keep_images ? ((size_t)PC_N_FIELDS + (size_t)ne) * (size_t)n_slots : 0;
	/* parts: consecutive slot ranges traced by consecutive launches into the same totals and image records (a photon
	 * depends on its global slot number only, so the result does not depend on the cut) */
	/* A compact run publishes its blocks itself: it needs no parts for the copy-back.  Option "compact_parts" > 1 traces a big one
	 * as that many launches on two streams all the same (the positions, block counters and totals are the run's, so a launch simply
	 * goes on where the one before leaves off): meant to cover the tail of one launch with the head of the next, it costs more
	 * than it saves (default 1). */
	int parts = (keep_images && o.run_parts > 1 && !compact) ? o.run_parts : 1;
	if (compact && o.compact_parts > 1 && n_slots >= 4000000) parts = o.compact_parts;
	if (parts > PC_MAX_PARTS) parts = PC_MAX_PARTS;
	if ((long long)parts > n_slots / 65536) parts = (int)(n_slots / 65536);
	if (parts < 1) parts = 1;
	p.parts = parts;
	p.fetch_parts = compact ? 1 : parts;
	p.halves = (parts > 1) ? 2 : 1;
	for (int k = 0; k <= parts; k++) p.begin[k] = pc_part_begin(n_slots, parts, k);
	if (compact) {
		p.blk_shift = o.blk_shift;
		p.blocks = (n_slots + (1ll << o.blk_shift) - 1) >> o.blk_shift;
	}
	return p;
}

/* ---- where an element lies: field f of the entry at position lo + i at base + i*ss + f*fs, its weight e at w_base + i*ws + e
 * (elements of the layout's buffer; pc_kargs::img) */
struct pc_image_layout { long long ss, fs, ws; size_t base, w_base; };

static pc_image_layout pc_layout_of(int layout, long long n_total, long long ne, long long lo)
{
	const long long rec = PC_N_FIELDS + ne;
	switch (layout) {
	case PC_IMG_PLANES: case PC_IMG_COMPACT:
		return { 1, n_total, ne, (size_t)lo, (size_t)((long long)PC_N_FIELDS*n_total + lo*ne) };
	case PC_IMG_RECORDS:
		return { rec, 1, rec, (size_t)(lo*rec), (size_t)(lo*rec + PC_N_FIELDS) };
	}
	return { 0, 0, 0, 0, 0 };
}

/* the positions [lo, hi) that the compact blocks [b, e) add to a fetch of [first, first + count) of a run of n_total */
static void pc_block_span(long long first, long long count, long long n_total, int blk_shift, long long b, long long e, long long &lo, long long &hi)
{
	lo = std::max(b << blk_shift, first);
	hi = std::min(std::min(e << blk_shift, n_total), first + count);
}

/* the caller's planes in the kernels' field order, the weights last */
static void pc_image_planes(const pc_hip_images *d, void *out[PC_N_FIELDS + 1])
{
	void *p[PC_N_FIELDS + 1] = {
		d->src_start_coords[0], d->src_start_coords[1], d->pc_start_coords[0], d->pc_start_coords[1],
		d->pc_start_dir[0], d->pc_start_dir[1], d->pc_start_elecv[0], d->pc_start_elecv[1],
		d->pc_exit_coords[0], d->pc_exit_coords[1], d->pc_exit_coords[2],
		d->pc_exit_dir[0], d->pc_exit_dir[1], d->pc_exit_elecv[0], d->pc_exit_elecv[1],
		d->pc_exit_nrefl, d->pc_exit_dtravel, d->exit_coord_weights };
	std::copy(p, p + PC_N_FIELDS + 1, out);
}

/* ---- the store and the fetch: device code and the owner types, so nothing below is for a host compiler */
#ifdef __HIPCC__

/* Compact store: slots that used up their attempts without a transmitted photon wrote nothing (the slot-ordered store writes
 * zero weights for them), so the positions behind the run's cursor hold whatever the buffer held: zero them once the trace
 * kernel has ended -- every plane and the weights -- so that a result with failed slots never carries stale data. */
__global__ void __launch_bounds__(256) pc_compact_tail_kernel(double *soa, long long n_total, int ne, const unsigned long long *cursor)
{
	const long long c = (long long)*cursor;
	if (c >= n_total) return;
	const long long cells = (n_total - c)*(long long)(PC_N_FIELDS + ne);
	for (long long t = (long long)blockIdx.x*blockDim.x + threadIdx.x; t < cells; t += (long long)gridDim.x*blockDim.x) {
		const long long p = c + t / (PC_N_FIELDS + ne);
		const int f = (int)(t % (PC_N_FIELDS + ne));
		if (f < PC_N_FIELDS) soa[(long long)f*n_total + p] = 0.;
		else soa[(long long)PC_N_FIELDS*n_total + p*ne + (f - PC_N_FIELDS)] = 0.;
	}
}

/* Image records (one contiguous record of 17 + n_energies doubles per slot) -> the planes of struct _polycap_images: 17
 * planes of n_total doubles each, then the weights as [slot][n_energies].  A workgroup stages PC_SOA_TILE records in LDS
 * with coalesced reads and writes every plane with coalesced stores: 2 x 144 B of HBM traffic per photon, about a
 * millisecond per 1e7 photons, instead of a strided gather by host threads behind PCIe. */
#define PC_SOA_TILE 128
__global__ void __launch_bounds__(256) pc_soa_kernel(const double *rec, double *soa, long long first, long long count, long long n_total, int ne)
{
	extern __shared__ double tile[];
	const int recd = PC_N_FIELDS + ne;
	const long long j0 = first + (long long)blockIdx.x*PC_SOA_TILE;
	const int m = (int)((first + count - j0 < PC_SOA_TILE) ? first + count - j0 : PC_SOA_TILE);
	if (m <= 0) return;
	const double *src = rec + j0*recd;
	for (int k = threadIdx.x; k < m*recd; k += blockDim.x) tile[k] = src[k];
	__syncthreads();
	for (int k = threadIdx.x; k < m*PC_N_FIELDS; k += blockDim.x) {
		const int plane = k / m, t = k - plane*m;
		soa[(long long)plane*n_total + j0 + t] = tile[t*recd + plane];
	}
	double *w = soa + (long long)PC_N_FIELDS*n_total + j0*ne;
	for (int k = threadIdx.x; k < m*ne; k += blockDim.x) {
		const int t = k / ne, e = k - t*ne;
		w[k] = tile[t*recd + PC_N_FIELDS + e];
	}
}

/* what a reader on the device gets: n entries at p and their weights at w, strides in l */
struct pc_image_view {
	const double *p, *w;
	pc_image_layout l;
	long long n;
	const long long *ids;          /* compact runs with option "slot_ids": the slot at every position; else null */
};

struct pc_image_store {
	pc_dev_buf<double> d_img;              /* image records: n_slots x (17 + n_energies) doubles */
	pc_host_buf<double, PC_PIN_OR_PLAIN> h_stage; /* image fetches: two pinned chunks of records on the host */
	pc_event_handle ev_fetch[2];
	pc_stream_handle fetch_stream;         /* copies of finished parts run beside the kernel of the next part */
	pc_stream_handle fetch_stream_b;       /* compact runs: the planes of a group of blocks alternate between two copy streams */
	pc_event_handle ev_group[2][4];        /* compact runs: end of a group of copies, per stream, ring of 4 */
	pc_stream_handle stream2;              /* odd parts: a part's first workgroups start as the previous part's last ones leave */
	pc_event_handle ev_sync;
	pc_event_handle ev_part[PC_MAX_PARTS]; /* end of every part of a run in parts */
	/* plane (SoA) copy of the image records on the device: 17 planes of the run's n_slots doubles, then the weights [slot][n_energies].
	 * pc_hip_transmission_images copies from here straight into the caller's (registered) planes -- no host transposition */
	pc_dev_buf<double> d_soa;
	pc_dev_buf<unsigned long long> d_cursor;
	pc_dev_buf<unsigned int> d_blk_done;
	pc_host_buf<unsigned int, PC_PIN_MAPPED> h_blk_flag; /* mapped into the device (h_blk_flag.dev): 1 when a block is complete */
	pc_dev_buf<long long> d_ids;
	pc_dev_buf<double> d_lane_start;
	pc_image_opts opts;
	/* of the context, for good (bind) */
	size_t ne = 1;
	hipStream_t run_stream = nullptr;      /* the context's stream: a run ends on it */
	hipEvent_t run_end = nullptr;          /* the event behind a run's last kernel */
	/* the last run */
	pc_image_plan plan;
	int valid = 0;                         /* it kept images, and they are here */
	size_t lanes = 0;                      /* compact: lanes of a set of start-image lines (d_lane_start) */

	void bind(size_t n_energies, hipStream_t stream, hipEvent_t end) { ne = n_energies; run_stream = stream; run_end = end; }
	/* nothing of a run is here */
	void reset() { plan = pc_image_plan(); valid = 0; }

	pc_image_view device_view() const
	{
		const bool planes = plan.layout >= PC_IMG_PLANES;
		const double *buf = planes ? d_soa : d_img;
		pc_image_view v;
		v.l = pc_layout_of(planes ? PC_IMG_PLANES : PC_IMG_RECORDS, plan.n_slots, (long long)ne, 0);
		v.p = buf + v.l.base; v.w = buf + v.l.w_base;
		v.n = plan.n_slots;
		v.ids = (plan.layout == PC_IMG_COMPACT && opts.slot_ids) ? (const long long *)d_ids : nullptr;
		return v;
	}

	/* where a launch for slots [lo, ...) of a run of n_total slots stores its images: see pc_kargs::img */
	void set_img(pc_kargs &a, int layout, long long n_total, long long lo) const
	{
		double *buf = layout == PC_IMG_NONE ? nullptr : layout == PC_IMG_RECORDS ? (double *)d_img : (double *)d_soa;
		const pc_image_layout l = pc_layout_of(layout, n_total, (long long)ne, lo);
		a.img = buf ? buf + l.base : nullptr; a.img_w = buf ? buf + l.w_base : nullptr;
		a.img_ss = l.ss; a.img_fs = l.fs; a.img_ws = l.ws;
	}

	/* n records in one part, of a run that is not planned here (leak runs, relays) */
	int keep_records(long long n, const char *msg)
	{
		pc_image_opts o;
		plan = pc_plan_images(n, (int)ne, true, o);
		return d_img.grow(((size_t)PC_N_FIELDS + ne) * (size_t)std::max<long long>(n, 1), msg);
	}

	/* The buffers of the run that p plans, counters and flags cleared on the context's stream.  A run that wants planes and cannot
	 * have the buffer for them keeps records: p is planned again without them.  A compact run clears its block flags from the host:
	 * the context's previous run has been waited for.  `max_lanes`: lanes of the largest launch the context makes. */
	int prepare(pc_image_plan &p, size_t max_lanes)
	{
		if (p.layout >= PC_IMG_PLANES && d_soa.grow(p.elems, "could not allocate the device image planes") != PC_HIP_OK) {
			pc_image_opts o = opts;
			o.plane_images = 0;
			p = pc_plan_images(p.n_slots, (int)ne, true, o);
		}
		if (p.layout == PC_IMG_COMPACT) {
			/* position counter, per-block counters, the host-visible block flags, the lanes' start-image lines (`halves` sets of them)
			 * and, on request, the plane of slot indices */
			const size_t blocks = (size_t)p.blocks, cap = blocks + blocks/2 + 16;
			int st = d_cursor.grow(1, "pc_hip_transmission_run: could not allocate the position counter");
			if (!st) st = d_blk_done.grow(blocks, "pc_hip_transmission_run: could not allocate the block counters", cap);
			if (!st) st = h_blk_flag.grow(blocks, "pc_hip_transmission_run: could not allocate the block flags", cap);
			if (!st && opts.slot_ids) st = d_ids.grow((size_t)p.n_slots, "pc_hip_transmission_run: could not allocate the slot-index plane");
			/* one 64-byte line per lane of the largest launch the context makes, per half */
			if (!st) st = d_lane_start.grow(8*max_lanes*(size_t)p.halves, "pc_hip_transmission_run: could not allocate the lanes' start-image lines");
			if (st) return st;
			lanes = max_lanes;
			memset(h_blk_flag, 0, blocks*sizeof(unsigned int));      /* nobody looks at them now */
			PC_HIP_CHECK(hipMemsetAsync(d_cursor, 0, sizeof(unsigned long long), run_stream));
			PC_HIP_CHECK(hipMemsetAsync(d_blk_done, 0, blocks*sizeof(unsigned int), run_stream));
		}
		if (p.layout == PC_IMG_RECORDS) {
			int st = d_img.grow(p.elems, "pc_hip_transmission_run: could not allocate the image planes; use keep_images=0");
			if (st) return st;
		}
		plan = p;
		return PC_HIP_OK;
	}

	/* the image arguments of the launch of part k */
	void kargs(pc_kargs &a, int k) const
	{
		const bool compact = plan.layout == PC_IMG_COMPACT;
		set_img(a, plan.layout, plan.n_slots, compact ? 0 : plan.begin[k]);      /* compact: positions are the run's, not the part's */
		if (!compact) return;
		a.img_cursor = d_cursor;
		a.img_ids = opts.slot_ids ? (long long *)d_ids : nullptr;
		a.blk_done = d_blk_done;
		a.blk_flag = h_blk_flag.dev;
		a.blk_shift = plan.blk_shift;
		a.img_n = plan.n_slots;
		/* the launch before and the one after run on the other stream: the other set of lines.  Slot ids are the run's */
		a.lane_start = d_lane_start + (size_t)(k & 1)*8*lanes;
		a.img_id0 = plan.begin[k];
	}
};

/* records of slots [lo, lo + count) of the last run -> planes (pitch = the run's n_slots), on `stream` */
static int pc_soa_launch(pc_image_store &st, hipStream_t stream, long long lo, long long count)
{
	const int ne = (int)st.ne;
	const size_t lds = (size_t)PC_SOA_TILE*(PC_N_FIELDS + ne)*sizeof(double);
	if (lds > 65536) return PC_HIP_ERR_INVALID;
	const unsigned blocks = (unsigned)((count + PC_SOA_TILE - 1)/PC_SOA_TILE);
	hipLaunchKernelGGL(pc_soa_kernel, dim3(blocks), dim3(256), lds, stream, st.d_img, st.d_soa, lo, count, st.plan.n_slots, ne);
	PC_HIP_CHECK(hipGetLastError());
	return PC_HIP_OK;
}

/* host threads that turn fetched image records (AoS, `rec` doubles per slot) into the caller's SoA planes */
struct pc_copy_piece { const double *from; size_t slot; size_t n; };      /* n records at `from` belong to slots [slot, slot + n) */

class pc_copy_workers {
public:
	explicit pc_copy_workers(int n)
	{
		for (int t = 1; t < n; t++) threads_.emplace_back([this]() { loop(); });
	}
	~pc_copy_workers()
	{
		{ std::lock_guard<std::mutex> g(m_); stop_ = true; }
		cv_work_.notify_all();
		for (auto &t : threads_) t.join();
	}
	/* scatters every piece; returns when all are done (the calling thread works too) */
	void run(const std::vector<pc_copy_piece> &pieces, void *const *planes, double *weights, size_t rec, size_t ne, double *raw = nullptr)
	{
		{
			std::lock_guard<std::mutex> g(m_);
			pieces_ = &pieces; planes_ = planes; weights_ = weights; rec_ = rec; ne_ = ne; raw_ = raw;
			next_.store(0); busy_ = (int)threads_.size(); gen_++;
		}
		cv_work_.notify_all();
		drain();
		std::unique_lock<std::mutex> g(m_);
		cv_done_.wait(g, [this]() { return busy_ == 0; });
		pieces_ = nullptr;
	}
private:
	void drain()
	{
		const std::vector<pc_copy_piece> &pieces = *pieces_;
		const size_t rec = rec_, ne = ne_;
		const size_t nplanes = rec - ne;
		for (size_t j = next_.fetch_add(1); j < pieces.size(); j = next_.fetch_add(1)) {
			const pc_copy_piece &p = pieces[j];
			if (raw_) { memcpy(raw_ + p.slot*rec, p.from, p.n*rec*sizeof(double)); continue; }     /* records as they are */
			/* plane by plane: strided reads of a piece that fits the cache, contiguous writes (8-byte words: the
			 * reflection count is an int64 plane) */
			for (size_t k = 0; k < nplanes; k++) {
				if (!planes_[k]) continue;
				double *to = (double *)planes_[k] + p.slot;
				const double *from = p.from + k;
				for (size_t i = 0; i < p.n; i++) to[i] = from[i*rec];
			}
			if (weights_) {
				if (ne == 1) {
					double *to = weights_ + p.slot;
					const double *from = p.from + nplanes;
					for (size_t i = 0; i < p.n; i++) to[i] = from[i*rec];
				} else {
					for (size_t i = 0; i < p.n; i++)
						memcpy(weights_ + (p.slot + i)*ne, p.from + i*rec + nplanes, ne*sizeof(double));
				}
			}
		}
	}
	void loop()
	{
		unsigned long seen = 0;
		for (;;) {
			{
				std::unique_lock<std::mutex> g(m_);
				cv_work_.wait(g, [&]() { return stop_ || gen_ != seen; });
				if (stop_) return;
				seen = gen_;
			}
			drain();
			{
				std::lock_guard<std::mutex> g(m_);
				if (--busy_ == 0) cv_done_.notify_all();
			}
		}
	}
	std::vector<std::thread> threads_;
	std::mutex m_;
	std::condition_variable cv_work_, cv_done_;
	const std::vector<pc_copy_piece> *pieces_ = nullptr;
	void *const *planes_ = nullptr;
	double *weights_ = nullptr, *raw_ = nullptr;
	size_t rec_ = 0, ne_ = 0;
	std::atomic<size_t> next_{0};
	unsigned long gen_ = 0;
	int busy_ = 0;
	bool stop_ = false;
};

/* is this host address pinned already (an earlier fetch with "keep_pinned", a slab from the host pool, the caller's own
 * hipHostRegister / hipHostMalloc)?  Pinning a range inside an existing registration a second time is not something to try. */
static bool pc_host_is_pinned(void *p)
{
	unsigned int flags = 0;
	if (hipHostGetFlags(&flags, p) == hipSuccess) return true;
	(void)hipGetLastError();
	return false;
}

/* Pins the host ranges (address, bytes) for the copy engine: rounded out to pages, overlapping or touching ranges merged (small
 * planes from malloc share pages with their neighbours, and a page cannot be registered twice), ranges that are pinned already
 * left alone.  All or nothing: when one range cannot be pinned the ones pinned here are released again and false is returned
 * -- a destination that is pinned only in part is not something to hand to hipMemcpyAsync.  `pinned` receives what to
 * hipHostUnregister afterwards. */
static bool pc_pin_ranges(std::vector<std::pair<char *, size_t>> ranges, unsigned int flags, std::vector<void *> &pinned)
{
	const uintptr_t page = 4096;
	std::vector<std::pair<uintptr_t, uintptr_t>> r;
	for (auto &x : ranges) {
		if (!x.first || !x.second) continue;
		const uintptr_t lo = (uintptr_t)x.first & ~(page - 1), hi = ((uintptr_t)x.first + x.second + page - 1) & ~(page - 1);
		r.emplace_back(lo, hi);
	}
	std::sort(r.begin(), r.end());
	std::vector<std::pair<uintptr_t, uintptr_t>> m;
	for (auto &x : r) {
		if (!m.empty() && x.first <= m.back().second) m.back().second = std::max(m.back().second, x.second);
		else m.push_back(x);
	}
	const size_t before = pinned.size();
	for (auto &x : m) {
		if (pc_host_is_pinned((void *)x.first) && pc_host_is_pinned((void *)(x.second - 1))) continue;
		if (hipHostRegister((void *)x.first, (size_t)(x.second - x.first), flags) != hipSuccess) {
			(void)hipGetLastError();
			while (pinned.size() > before) { (void)hipHostUnregister(pinned.back()); pinned.pop_back(); }
			return false;
		}
		pinned.push_back((void *)x.first);
	}
	return true;
}

static double pc_now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* The caller's planes, pinned for one direct fetch of `count` positions and released when it is over (or kept, "keep_pinned").
 * Planes at one common stride (polycap_source_get_transmission_efficiencies allocates its result as one slab): pinned in one
 * piece, and a group of blocks is ONE pitched copy of 17 (one energy: 18, the weights are the 18th plane) rows instead of as
 * many linear ones -- a copy costs the engine 4-5 us whatever its size (scripts/analysis/copy2d_probe.hip: 56.5 against
 * 49 GB/s at 0.5 M positions per group).  Other planes are pinned by merged ranges; `ok` is false when that fails (a plane run
 * is then copied unpinned: slower, still right).  With "dst_prepinned" nothing is pinned here. */
struct pc_pinned_dst {
	long long slab_stride = 0;      /* bytes between two planes, 0: no common stride */
	int slab_rows = 0;
	bool ok = true;
	double t_begin, t_pinned;
	pc_pinned_dst(const pc_image_store &st, void *const *planes, double *weights, int64_t count) : keep_slab(st.opts.keep_pinned != 0)
	{
		const size_t ne = st.ne;
		t_begin = pc_now_ms();
		const bool pin_here = !st.opts.dst_prepinned;
		if (st.plan.layout == PC_IMG_COMPACT && planes[0] && planes[1]) {
			const long long s = (long long)((char *)planes[1] - (char *)planes[0]);
			bool uniform = s >= (long long)((size_t)count*sizeof(double));
			for (int f = 2; f < PC_N_FIELDS && uniform; f++)
				uniform = planes[f] && (char *)planes[f] - (char *)planes[0] == (long long)f*s;
			if (uniform) {
				slab_stride = s;
				slab_rows = PC_N_FIELDS;
				if (ne == 1 && weights && (char *)weights - (char *)planes[0] == (long long)PC_N_FIELDS*s) slab_rows = PC_N_FIELDS + 1;
			}
		}
		if (slab_stride && pin_here) {
			const bool w_in = weights && (char *)weights - (char *)planes[0] == (long long)PC_N_FIELDS*slab_stride;
			const size_t bytes = w_in ? (size_t)PC_N_FIELDS*(size_t)slab_stride + (size_t)count*ne*sizeof(double)
			                          : (size_t)(PC_N_FIELDS - 1)*(size_t)slab_stride + (size_t)count*sizeof(double);
			const hipError_t re = pc_host_is_pinned(planes[0]) ? hipErrorHostMemoryAlreadyRegistered : hipHostRegister(planes[0], bytes, hipHostRegisterDefault);
			if (re == hipSuccess) pinned.push_back(planes[0]);
			else {
				(void)hipGetLastError();
				if (re != hipErrorHostMemoryAlreadyRegistered) { slab_stride = 0; slab_rows = 0; }      /* plane by plane below */
			}
			if (slab_stride && weights && !w_in) {
				const hipError_t rw = pc_host_is_pinned(weights) ? hipErrorHostMemoryAlreadyRegistered : hipHostRegister(weights, (size_t)count*ne*sizeof(double), hipHostRegisterDefault);
				if (rw == hipSuccess) pinned.push_back(weights); else (void)hipGetLastError();
			}
		}
		if (!slab_stride && pin_here) {
			std::vector<std::pair<char *, size_t>> ranges;
			for (int k = 0; k <= PC_N_FIELDS; k++) {
				void *p = (k < PC_N_FIELDS) ? planes[k] : (void *)weights;
				if (p) ranges.emplace_back((char *)p, (size_t)count*sizeof(double)*(k < PC_N_FIELDS ? 1 : ne));
			}
			ok = pc_pin_ranges(ranges, hipHostRegisterDefault, pinned);
		}
		t_pinned = pc_now_ms();
	}
	pc_pinned_dst(const pc_pinned_dst &) = delete;
	pc_pinned_dst &operator=(const pc_pinned_dst &) = delete;
	~pc_pinned_dst() { release(); }
	void release()
	{
		if (keep_slab && slab_stride) pinned.clear();      /* the caller keeps its slab pinned (and unpins it itself: pc_hip_host_unregister) */
		for (void *p : pinned) (void)hipHostUnregister(p);
		pinned.clear();
	}
private:
	std::vector<void *> pinned;
	bool keep_slab;
};

/* Positions [lo, hi) of the device planes -> the caller's planes, which begin at position `first`: one pitched copy on
 * streams[0] for a slab (and the weights on streams[1] unless they are its last row), else plane f on streams[f & 1] */
static hipError_t pc_copy_planes(const pc_image_store &st, void *const *planes, double *weights, const pc_pinned_dst &slab,
                                 long long lo, long long hi, long long first, const hipStream_t streams[2])
{
	const pc_image_layout l = pc_layout_of(PC_IMG_PLANES, st.plan.n_slots, (long long)st.ne, lo);
	const double *src = st.d_soa + l.base, *src_w = st.d_soa + l.w_base;
	const size_t bytes = (size_t)(hi - lo)*sizeof(double), w_bytes = bytes*st.ne;
	double *to_w = weights ? weights + (size_t)(lo - first)*st.ne : nullptr;
	hipError_t err = hipSuccess;
	if (slab.slab_stride) {
		err = hipMemcpy2DAsync((double *)planes[0] + (lo - first), (size_t)slab.slab_stride, src, (size_t)l.fs*sizeof(double),
		                       bytes, (size_t)slab.slab_rows, hipMemcpyDeviceToHost, streams[0]);
		if (err == hipSuccess && weights && slab.slab_rows == PC_N_FIELDS)
			err = hipMemcpyAsync(to_w, src_w, w_bytes, hipMemcpyDeviceToHost, streams[1]);
		return err;
	}
	for (int f = 0; f < PC_N_FIELDS && err == hipSuccess; f++)
		if (planes[f])
			err = hipMemcpyAsync((double *)planes[f] + (lo - first), src + (size_t)f*l.fs, bytes, hipMemcpyDeviceToHost, streams[f & 1]);
	if (err == hipSuccess && weights) err = hipMemcpyAsync(to_w, src_w, w_bytes, hipMemcpyDeviceToHost, streams[PC_N_FIELDS & 1]);
	return err;
}

/* A compact run: the kernel publishes its planes block by block (pc_blocks_written): every block is copied as soon as its flag
 * is up, while the kernel goes on.  The kernel's end also ends the wait (every block is complete then). */
static int pc_fetch_compact(pc_image_store &st, const pc_pinned_dst &slab, int64_t first, int64_t count, void *const *planes, double *weights)
{
	const int shift = st.plan.blk_shift;
	const long long b_end = std::min<long long>(st.plan.blocks, (first + count + (1ll << shift) - 1) >> shift);
	bool kernel_done = false;
	long long b = first >> shift;
	int group = 0, status = PC_HIP_OK;
	/* POLYCAP_FETCH_STREAMS (1 or 2, default 2): copy streams the planes of a group alternate between; POLYCAP_FETCH_DEPTH
	 * (1..3, default 2): groups of copies in flight */
	int n_streams = 2, depth = 2;
	if (const char *ev = getenv("POLYCAP_FETCH_STREAMS")) n_streams = (*ev == '1') ? 1 : 2;
	if (const char *ev = getenv("POLYCAP_FETCH_DEPTH")) depth = (*ev >= '1' && *ev <= '3') ? *ev - '0' : 2;
	if (n_streams == 2) PC_HIP_CHECK(st.fetch_stream_b.ensure(true));
	for (int k = 0; k < 2; k++)
		for (int j = 0; j < 4; j++)
			PC_HIP_CHECK(st.ev_group[k][j].ensure());
	const hipStream_t streams[2] = { st.fetch_stream, n_streams == 2 ? st.fetch_stream_b : st.fetch_stream };
	while (b < b_end && status == PC_HIP_OK) {
		volatile unsigned int *flag = st.h_blk_flag;
		unsigned long spins = 0;
		while (!kernel_done && flag[b] == 0u) {
			if ((++spins & 63ul) == 0ul) {
				const hipError_t q = hipEventQuery(st.run_end);
				if (q == hipSuccess) kernel_done = true;
				else if (q != hipErrorNotReady) { status = pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_transmission_images (kernel event query): ") + hipGetErrorString(q)); break; }
				(void)hipGetLastError();
			}
			std::this_thread::yield();
		}
		if (status != PC_HIP_OK) break;
		/* `depth` groups of copies are kept in flight: the next one is put together when the oldest has finished, from every
		 * block that is complete by then.  The first block is ready a fraction of a millisecond into the run; as the kernel
		 * produces faster than PCIe carries, every group is larger than the one before (up to 64 blocks) and the copy engines
		 * never wait -- nor are they fed thousands of small copies (4-5 us each, whatever their size). */
		if (group >= depth) {
			for (int k = 0; k < n_streams && status == PC_HIP_OK; k++) {
				const hipError_t we = hipEventSynchronize(st.ev_group[k][(group - depth) & 3]);
				if (we != hipSuccess) status = pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_transmission_images (wait for a group of copies): ") + hipGetErrorString(we));
			}
			if (status != PC_HIP_OK) break;
		}
		long long e = b + 1;
		while (e < b_end && e - b < 64 && (kernel_done || flag[e] != 0u)) e++;
		std::atomic_thread_fence(std::memory_order_acquire);
		long long lo, hi;
		pc_block_span(first, count, st.plan.n_slots, shift, b, e, lo, hi);
		hipError_t err = pc_copy_planes(st, planes, weights, slab, lo, hi, first, streams);
		if (err != hipSuccess) status = pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_transmission_images (copy of a group of blocks): ") + hipGetErrorString(err));
		for (int k = 0; k < n_streams && err == hipSuccess; k++) {
			err = hipEventRecord(st.ev_group[k][group & 3], streams[k]);
			if (err != hipSuccess) status = pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_transmission_images (event after a group of copies): ") + hipGetErrorString(err));
		}
		b = e;
		group++;
	}
	if (n_streams == 2 && hipStreamSynchronize(st.fetch_stream_b) != hipSuccess && status == PC_HIP_OK)
		status = pc_fail(PC_HIP_ERR_RUNTIME, "pc_hip_transmission_images: the plane copies failed");
	return status;
}

/* A run of records or planes: every part is copied behind its trace (and, if the run kept records, behind its turn into
 * planes).  A run in one part has been waited for by the caller. */
static int pc_fetch_parts(pc_image_store &st, const pc_pinned_dst &slab, int64_t first, int64_t count, void *const *planes, double *weights)
{
	const int parts = st.plan.fetch_parts;
	const hipStream_t streams[2] = { st.fetch_stream, st.fetch_stream };
	for (int k = 0; k < parts; k++) {
		const long long plo = st.plan.begin[k], phi = st.plan.begin[k + 1];
		const long long lo = std::max<long long>(plo, first), hi = std::min<long long>(phi, first + count);
		if (hi <= lo) continue;
		hipError_t e = hipSuccess;
		if (parts > 1) e = hipStreamWaitEvent(st.fetch_stream, st.ev_part[k], 0);         /* traced, and turned into planes if eager */
		else PC_HIP_CHECK(hipStreamSynchronize(st.run_stream));
		if (e == hipSuccess && st.plan.layout == PC_IMG_RECORDS) {
			/* the run kept records: turn the part into planes now, behind its trace */
			int s = pc_soa_launch(st, st.fetch_stream, plo, phi - plo);
			if (s) return s;
		}
		if (e == hipSuccess) e = pc_copy_planes(st, planes, weights, slab, lo, hi, first, streams);
		if (e != hipSuccess) return pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_transmission_images: ") + hipGetErrorString(e));
	}
	return PC_HIP_OK;
}

/* The stream of the image copies.  HIP multiplexes a process's streams over a few hardware queues (4 by default): with one
 * more context alive in the process the copies of a finished part landed in the queue of the next part's kernel and waited
 * for it (40 -> 54 ms per 1e7 photons through the C API, scripts/analysis/api_time2.py).  A stream of the highest priority
 * gets a queue of its own class, apart from the kernels' queues. */
static hipError_t pc_fetch_stream_ensure(pc_image_store &st)
{
	return st.fetch_stream.ensure(!getenv("POLYCAP_FETCH_PRIORITY_OFF"));
}

/* Can the copy engine write the caller's planes straight from the device's planes?  Always for a run that stored planes; a
 * record run needs its records to fit the LDS tile of pc_soa_kernel and a plane buffer on the device. */
static bool pc_fetch_direct_ready(pc_image_store &st)
{
	if (st.plan.layout >= PC_IMG_PLANES) return true;
	return (size_t)PC_SOA_TILE*(PC_N_FIELDS + st.ne)*sizeof(double) <= 65536
	       && st.d_soa.grow(st.plan.elems, "could not allocate the device image planes") == PC_HIP_OK;
}

/* the direct path behind the pinning: enqueue, wait, unpin */
static int pc_fetch_direct(pc_image_store &st, pc_pinned_dst &dst, int64_t first, int64_t count, void *const *planes, double *weights)
{
	const bool timing = getenv("POLYCAP_TIMING") != nullptr;
	int status = st.plan.layout == PC_IMG_COMPACT ? pc_fetch_compact(st, dst, first, count, planes, weights)
	                                              : pc_fetch_parts(st, dst, first, count, planes, weights);
	const double t_queued = pc_now_ms();
	if (hipStreamSynchronize(st.fetch_stream) != hipSuccess && status == PC_HIP_OK)
		status = pc_fail(PC_HIP_ERR_RUNTIME, "pc_hip_transmission_images: the plane copies failed");
	const double t_copied = pc_now_ms();
	dst.release();
	if (timing)
		fprintf(stderr, "polycap timing [ms]: plane fetch: pin %.1f, enqueue %.1f, wait for trace + copies %.1f, unpin %.1f\n",
		        dst.t_pinned - dst.t_begin, t_queued - dst.t_pinned, t_copied - t_queued, pc_now_ms() - t_copied);
	return status;
}

/* Pipeline over chunks of <= 16 MB of records: one asynchronous copy (DMA engine, no compute units) of the chunk into
 * pinned host memory, then host threads turn the records of the previous chunk into the caller's SoA planes while the
 * next one is in flight.  The copies run on their own stream and wait only for the part of the run that holds the
 * chunk, so they overlap the kernel of the following parts. */
static int pc_fetch_staged(pc_image_store &st, int64_t first, int64_t count, void *const *planes, double *weights, double *raw)
{
	const size_t ne = st.ne, rec = (size_t)PC_N_FIELDS + ne;
	const int n_parts = st.plan.fetch_parts;
	const hipStream_t stream = n_parts > 1 ? (hipStream_t)st.fetch_stream : st.run_stream;
	size_t chunk = ((size_t)16 << 20) / (rec*sizeof(double));
	if (chunk < 256) chunk = 256;
	if (chunk > (size_t)count) chunk = (size_t)count;
	int s = st.h_stage.grow(2*chunk*rec, "pc_hip_transmission_images: could not allocate the staging buffer");
	if (s) return s;
	for (int k = 0; k < 2; k++)
		PC_HIP_CHECK(st.ev_fetch[k].ensure());
	PC_HIP_CHECK(pc_fetch_stream_ensure(st));
	int nthreads = st.opts.fetch_threads;
	if (nthreads <= 0) {
		const unsigned hw = std::thread::hardware_concurrency();
		nthreads = (int)(hw == 0 ? 4 : (hw > 16 ? 16 : hw));
	}
	if ((size_t)count*rec*sizeof(double) < ((size_t)4 << 20)) nthreads = 1;
	pc_copy_workers workers(nthreads);
	std::vector<pc_copy_piece> pieces;
	/* records [done, done + n) in the pinned buffer `src` -> planes: pieces of 4096 records for the worker threads */
	auto scatter = [&](const double *src, size_t done, size_t n) {
		pieces.clear();
		for (size_t o = 0; o < n; o += 4096)
			pieces.push_back({src + o*rec, done + o, n - o < 4096 ? n - o : 4096});
		workers.run(pieces, planes, weights, rec, ne, raw);
	};
	size_t prev_done = 0, prev_n = 0;
	int c = 0, part = 0, waited = -1;
	for (size_t done = 0; done < (size_t)count; done += chunk, c++) {
		const size_t n = ((size_t)count - done < chunk) ? (size_t)count - done : chunk;
		const int b = c & 1;
		double *h_buf = st.h_stage + (size_t)b*chunk*rec;
		if (n_parts > 1) {
			/* the last slot of the chunk decides which part has to be finished */
			const long long last = first + (long long)(done + n) - 1;
			while (part < n_parts - 1 && st.plan.begin[part + 1] <= last) part++;
			/* every part up to that one: consecutive parts run on two streams, so the event of part p says nothing
			 * about part p-1, whose tail a chunk that straddles the boundary also reads */
			for (int q = waited + 1; q <= part; q++)
				PC_HIP_CHECK(hipStreamWaitEvent(st.fetch_stream, st.ev_part[q], 0));
			if (part > waited) waited = part;
		}
		PC_HIP_CHECK(hipMemcpyAsync(h_buf, st.d_img + ((size_t)first + done)*rec, n*rec*sizeof(double), hipMemcpyDeviceToHost, stream));
		PC_HIP_CHECK(hipEventRecord(st.ev_fetch[b], stream));
		if (c > 0) {
			PC_HIP_CHECK(hipEventSynchronize(st.ev_fetch[b ^ 1]));
			scatter(st.h_stage + (size_t)(b ^ 1)*chunk*rec, prev_done, prev_n);
		}
		prev_done = done; prev_n = n;
	}
	PC_HIP_CHECK(hipEventSynchronize(st.ev_fetch[(c - 1) & 1]));
	scatter(st.h_stage + (size_t)((c - 1) & 1)*chunk*rec, prev_done, prev_n);
	return PC_HIP_OK;
}

/* `count` > 0 images from position `first` of the last run, which kept some, into the planes dst (pc_image_planes) or as
 * records into raw.
 * Plane destinations of a run that stored planes, or of 1 MB per plane and more, take the direct path: the caller's planes are
 * pinned for the duration of the call (hipHostRegister: 3 ms for 1.4 GB of faulted-in memory) and the copy engine writes them
 * straight from the device's planes, part by part behind the trace.  No host thread touches the data.  Anything that does not
 * fit (a record too long for the LDS tile, a record run whose destination cannot be pinned) takes the staging pipeline. */
static int pc_fetch_images(pc_image_store &st, int64_t first, int64_t count, void *const *dst, double *raw)
{
	const bool to_planes = dst && !raw, stored_planes = st.plan.layout >= PC_IMG_PLANES;
	if (stored_planes && !to_planes)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_transmission_records: the last run stored planes (option plane_images); fetch them with pc_hip_transmission_images");
	void *const none[PC_N_FIELDS + 1] = {nullptr};
	void *const *planes = dst ? dst : none;
	double *weights = (double *)planes[PC_N_FIELDS];
	if (to_planes && (stored_planes || (size_t)count*sizeof(double) >= ((size_t)1 << 20)) && pc_fetch_direct_ready(st)) {
		PC_HIP_CHECK(pc_fetch_stream_ensure(st));
		PC_HIP_CHECK(st.ev_sync.ensure());
		pc_pinned_dst pin(st, planes, weights, count);
		if (pin.ok || stored_planes) return pc_fetch_direct(st, pin, first, count, planes, weights);
		/* a record run: the staging pipeline copies without pinning the destination */
	}
	return pc_fetch_staged(st, first, count, planes, weights, raw);
}

#endif /* __HIPCC__ */

#endif /* PC_IMAGES_H */

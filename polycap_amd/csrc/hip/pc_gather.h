/*
 * pc_gather.h -- the per-entry data of the entries a selection keeps (include/polycap-hip.h, pc_hip_select_gather): an ordered stream
 * compaction of a selection's mask (pc_select.h) into the ascending list of the passing positions, and a gather of the rows at
 * those positions into a staging buffer that one copy per chunk takes to the caller.  A post-pass like the tallies: it reads what
 * the run and the apply left on the device through pc_spot_src, so one row kernel serves records, planes, compact planes and the
 * leak event lists.  Rows travel as 64-bit patterns, never through a floating-point operation.
 *
 * The index list of a member and kind is built by the first gather after an apply and kept until the next apply of that kind:
 *   a. pc_gather_count_kernel   the mask bytes set in every tile of `tile` entries
 *   b. pc_gather_scan_kernel    the exclusive scan of the tile counts, by one workgroup that loops over the tiles with a carry
 *   c. pc_gather_write_kernel   per wave of 64 entries a ballot of the mask bytes, a lane's rank the popcount of the lanes below it,
 *                               the waves' offsets inside the tile through LDS, the tile's offset from (b)
 * The order is ascending by construction: no atomic decides a place.
 *
 * The first part (the argument check, the tile planner, the chunk split) compiles for the host as well: -DPC_GATHER_HOST_ONLY stops
 * the header after it.
 */
#ifndef PC_GATHER_H
#define PC_GATHER_H

#include <stdint.h>
#include <string>

#define PC_GATHER_TILE_MIN 64
#define PC_GATHER_TILE_MAX 65536
#define PC_GATHER_TILE_AUTO 4096                       /* 2442 tiles at 1e7 entries: ten steps of the scan's one workgroup */
#define PC_GATHER_STAGE_BYTES ((long long)128 << 20)    /* the staging buffer of "gather_chunk_rows" = 0 */

/* option "gather_tile": a multiple of 64 in 64 .. 65536, 0 = automatic */
static inline bool pc_gather_tile_ok(long long v)
{
	return v == 0 || (v >= PC_GATHER_TILE_MIN && v <= PC_GATHER_TILE_MAX && v % 64 == 0);
}

/* The tiles of n entries: tile t holds the positions [t*tile, min((t + 1)*tile, n)), every one a whole tile but the last */
struct pc_gather_tiling {
	long long tile, tiles;
};

static inline pc_gather_tiling pc_gather_plan(long long n, long long tile_option)
{
	const long long tile = tile_option > 0 ? tile_option : PC_GATHER_TILE_AUTO;
	const pc_gather_tiling t = { tile, n > 0 ? (n + tile - 1)/tile : 0 };
	return t;
}

static inline void pc_gather_tile_span(const pc_gather_tiling &p, long long n, long long t, long long *lo, long long *hi)
{
	*lo = t*p.tile;
	*hi = (*lo + p.tile < n) ? *lo + p.tile : n;
}

/* rows of a staging chunk: the option, or as many rows of row_doubles doubles as fit in 128 MiB, at least 1 */
static inline long long pc_gather_chunk_rows(long long option, long long row_doubles)
{
	if (option > 0) return option;
	const long long rows = PC_GATHER_STAGE_BYTES / (row_doubles*(long long)sizeof(double));
	return rows < 1 ? 1 : rows;
}

/* the chunks of the window [first, first + count): chunk k is [lo, lo + n), n <= rows, one after the other */
static inline long long pc_gather_n_chunks(long long count, long long rows)
{
	return count > 0 ? (count + rows - 1)/rows : 0;
}

static inline void pc_gather_chunk(long long first, long long count, long long rows, long long k, long long *lo, long long *n)
{
	*lo = first + k*rows;
	const long long left = first + count - *lo;
	*n = left < rows ? left : rows;
}

/* what pc_hip_select_gather refuses before it looks at the device: the reason names the function and the field */
static inline bool pc_gather_args_check(const void *select, int kind, long long first, long long count, const void *records, std::string *why)
{
	if (!select) *why = "pc_hip_select_gather: select must not be NULL";
	else if (kind < 0 || kind > 2) *why = "pc_hip_select_gather: kind must be 0 (exit photons), 1 (extleak) or 2 (intleak), got " + std::to_string(kind);
	else if (first < 0) *why = "pc_hip_select_gather: first must be >= 0, got " + std::to_string(first);
	else if (count < 0) *why = "pc_hip_select_gather: count must be >= 0, got " + std::to_string(count);
	else if (count > 0 && !records) *why = "pc_hip_select_gather: records must not be NULL when count > 0";
	return why->empty();
}

/* the window against the passing entries of the kind (known once the selection was applied) */
static inline bool pc_gather_window_check(long long first, long long count, long long n_pass, std::string *why)
{
	if (first > n_pass || count > n_pass - first)
		*why = "pc_hip_select_gather: first + count = " + std::to_string(first) + " + " + std::to_string(count) + " exceeds n_pass = "
		       + std::to_string(n_pass) + " of that kind";
	return why->empty();
}

#ifndef PC_GATHER_HOST_ONLY

#define PC_GATHER_BLOCK 256

/* a. cnt[t] = the mask bytes set in tile t; workgroup x takes the tiles x, x + gridDim.x, ... */
__global__ void __launch_bounds__(PC_GATHER_BLOCK) pc_gather_count_kernel(const unsigned char *mask, long long n, long long tile, long long tiles,
	unsigned int *cnt)
{
	__shared__ unsigned int part[PC_GATHER_BLOCK/64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
		const long long lo = t*tile, hi = (lo + tile < n) ? lo + tile : n;
		unsigned int c = 0;
		for (long long base = lo + wave*64; base < hi; base += PC_GATHER_BLOCK) {      /* uniform over the wave */
			const long long i = base + lane;
			const int pass = (i < hi) ? (mask[i] != 0) : 0;
			c += (unsigned int)__popcll(__ballot(pass));
		}
		if (lane == 0) part[wave] = c;
		__syncthreads();
		if (threadIdx.x == 0) {
			unsigned int s = 0;
			for (int w = 0; w < PC_GATHER_BLOCK/64; w++) s += part[w];
			cnt[t] = s;
		}
		__syncthreads();
	}
}

/* b. off[t] = cnt[0] + ... + cnt[t - 1] for t = 0 .. tiles (off[tiles] = the last tile's offset plus its count: all that pass).
 * One workgroup; PC_GATHER_BLOCK tiles per step, the sum of the steps before carried along. */
__global__ void __launch_bounds__(PC_GATHER_BLOCK) pc_gather_scan_kernel(const unsigned int *cnt, long long tiles, unsigned int *off)
{
	__shared__ unsigned int wsum[PC_GATHER_BLOCK/64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned int carry = 0;
	for (long long base = 0; base < tiles; base += PC_GATHER_BLOCK) {
		const long long t = base + threadIdx.x;
		const unsigned int v = (t < tiles) ? cnt[t] : 0u;
		unsigned int incl = v;      /* inclusive scan over the wave */
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned int up = __shfl_up(incl, d);
			if (lane >= d) incl += up;
		}
		if (lane == 63) wsum[wave] = incl;
		__syncthreads();
		unsigned int before = 0, total = 0;
		for (int w = 0; w < PC_GATHER_BLOCK/64; w++) {
			if (w < wave) before += wsum[w];
			total += wsum[w];
		}
		if (t < tiles) off[t] = carry + before + incl - v;
		carry += total;
		__syncthreads();
	}
	if (threadIdx.x == 0) off[tiles] = carry;
}

/* c. idx[off[t] + rank inside the tile] = position, for every position of tile t whose mask byte is set.  n_idx: the list's length,
 * beyond which nothing is written whatever the mask says. */
__global__ void __launch_bounds__(PC_GATHER_BLOCK) pc_gather_write_kernel(const unsigned char *mask, long long n, long long tile, long long tiles,
	const unsigned int *off, unsigned int *idx, long long n_idx)
{
	__shared__ unsigned int part[PC_GATHER_BLOCK/64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
		const long long lo = t*tile, hi = (lo + tile < n) ? lo + tile : n;
		long long at = off[t];      /* the next free place: uniform over the workgroup */
		for (long long base = lo; base < hi; base += PC_GATHER_BLOCK) {
			const long long i = base + threadIdx.x;
			const int pass = (i < hi) ? (mask[i] != 0) : 0;
			const unsigned long long verdicts = __ballot(pass);
			const int rank = __popcll(verdicts & ((1ull << lane) - 1ull));
			if (lane == 0) part[wave] = (unsigned int)__popcll(verdicts);
			__syncthreads();
			unsigned int before = 0, total = 0;
			for (int w = 0; w < PC_GATHER_BLOCK/64; w++) {
				if (w < wave) before += part[w];
				total += part[w];
			}
			const long long to = at + before + rank;
			if (pass && to < n_idx) idx[to] = (unsigned int)i;
			at += total;
			__syncthreads();
		}
	}
}

/* Rows r0 .. r0 + nrows - 1 of the index list into out [nrows][row]: (row, field) flattened across the lanes, so that a wave writes
 * contiguous 8-byte words.  Field f < nf of entry i is the 64-bit word at p[i*ss + f*fs], f >= nf the weight f - nf at w[i*ws + f - nf]. */
__global__ void __launch_bounds__(PC_GATHER_BLOCK) pc_gather_rows_kernel(pc_spot_src s, int nf, int row, const unsigned int *idx, long long r0,
	long long nrows, unsigned long long *out)
{
	const unsigned long long *p = (const unsigned long long *)s.p, *w = (const unsigned long long *)s.w;
	const long long total = nrows*row;
	for (long long j = (long long)blockIdx.x*blockDim.x + threadIdx.x; j < total; j += (long long)gridDim.x*blockDim.x) {
		const long long r = j / row;
		const int f = (int)(j - r*row);
		const long long i = idx[r0 + r];
		if (i >= s.n) continue;      /* never, the list holds positions of the mask */
		out[j] = (f < nf) ? p[i*s.ss + (long long)f*s.fs] : w[i*s.ws + (f - nf)];
	}
}

/* the index list of member mb and kind, built on its stream (its device is current) unless it is there */
static int pc_gather_index(pc_select_member &mb, int kind)
{
	if (mb.idx_valid[kind]) return PC_HIP_OK;
	pc_hip_ctx *c = mb.ctx;
	const long long n = mb.n[kind], n_pass = mb.n_pass[kind];
	const pc_gather_tiling tl = pc_gather_plan(n, c->gather_tile);
	int st = mb.d_idx[kind].grow((size_t)n_pass, "pc_hip_select_gather: could not allocate the index list");
	if (!st) st = mb.d_tile_cnt.grow((size_t)tl.tiles, "pc_hip_select_gather: could not allocate the tile counts");
	if (!st) st = mb.d_tile_off.grow((size_t)tl.tiles + 1, "pc_hip_select_gather: could not allocate the tile offsets");
	if (st) return st;
	const unsigned char *mask = mb.d_mask[kind];
	const long long cap = 8ll*c->n_cu;
	const unsigned grid = (unsigned)(tl.tiles < cap ? tl.tiles : cap);
	hipLaunchKernelGGL(pc_gather_count_kernel, dim3(grid), dim3(PC_GATHER_BLOCK), 0, c->stream, mask, n, tl.tile, tl.tiles, (unsigned int *)mb.d_tile_cnt);
	PC_HIP_CHECK(hipGetLastError());
	hipLaunchKernelGGL(pc_gather_scan_kernel, dim3(1), dim3(PC_GATHER_BLOCK), 0, c->stream, (const unsigned int *)mb.d_tile_cnt, tl.tiles,
	                   (unsigned int *)mb.d_tile_off);
	PC_HIP_CHECK(hipGetLastError());
	hipLaunchKernelGGL(pc_gather_write_kernel, dim3(grid), dim3(PC_GATHER_BLOCK), 0, c->stream, mask, n, tl.tile, tl.tiles,
	                   (const unsigned int *)mb.d_tile_off, (unsigned int *)mb.d_idx[kind], n_pass);
	PC_HIP_CHECK(hipGetLastError());
	unsigned int total = 0;
	PC_HIP_CHECK(hipMemcpyAsync(&total, mb.d_tile_off + tl.tiles, sizeof(total), hipMemcpyDeviceToHost, c->stream));
	PC_HIP_CHECK(hipStreamSynchronize(c->stream));
	if ((long long)total != n_pass)
		return pc_fail(PC_HIP_ERR_RUNTIME, "pc_hip_select_gather: the compaction found " + std::to_string(total) + " passing entries where the apply counted "
		               + std::to_string(n_pass));
	mb.idx_valid[kind] = 1;
	return PC_HIP_OK;
}

/* passing entries [lo, lo + cnt) of member mb (its own numbering) to records and positions (either may be NULL); pos0: the member's
 * first global position */
static int pc_gather_member(pc_select_member &mb, const pc_spot_src &src, int kind, int nf, int row, long long lo, long long cnt, long long pos0,
	double *records, int64_t *positions)
{
	pc_hip_ctx *c = mb.ctx;
	PC_HIP_CHECK(hipSetDevice(c->device));
	int st = pc_gather_index(mb, kind);
	if (st) return st;
	const unsigned int *idx = mb.d_idx[kind];
	if (positions) {
		std::vector<unsigned int> local((size_t)cnt);
		PC_HIP_CHECK(hipMemcpyAsync(local.data(), idx + lo, (size_t)cnt*sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
		PC_HIP_CHECK(hipStreamSynchronize(c->stream));
		for (long long k = 0; k < cnt; k++) positions[k] = pos0 + (int64_t)local[(size_t)k];
	}
	if (!records) return PC_HIP_OK;
	long long rows = pc_gather_chunk_rows(c->gather_chunk_rows, row);
	if (rows > cnt) rows = cnt;
	st = mb.d_stage.grow((size_t)rows*(size_t)row, "pc_hip_select_gather: could not allocate the staging buffer");
	if (st) return st;
	const long long chunks = pc_gather_n_chunks(cnt, rows);
	for (long long k = 0; k < chunks; k++) {
		long long r0, nr;
		pc_gather_chunk(lo, cnt, rows, k, &r0, &nr);
		const long long bx = pc_tally_grid_cap(8ll*c->n_cu, nr*row, PC_GATHER_BLOCK);
		hipLaunchKernelGGL(pc_gather_rows_kernel, dim3((unsigned)bx), dim3(PC_GATHER_BLOCK), 0, c->stream, src, nf, row, idx, r0, nr,
		                   (unsigned long long *)mb.d_stage);
		PC_HIP_CHECK(hipGetLastError());
		PC_HIP_CHECK(hipMemcpyAsync(records + (size_t)(r0 - lo)*(size_t)row, mb.d_stage, (size_t)nr*(size_t)row*sizeof(double), hipMemcpyDeviceToHost, c->stream));
		PC_HIP_CHECK(hipStreamSynchronize(c->stream));      /* the next chunk writes the same buffer */
	}
	return PC_HIP_OK;
}

extern "C" {

int pc_hip_select_gather(pc_hip_select *sel, int kind, int64_t first, int64_t count, double *records, int64_t *positions)
{
	static const char *who = "pc_hip_select_gather";
	std::string why;
	if (!pc_gather_args_check(sel, kind, first, count, records, &why)) return pc_fail(PC_HIP_ERR_INVALID, why);
	if (!sel->applied[kind])
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_gather: the selection was not applied for kind " + std::to_string(kind) + " (pc_hip_select_apply)");
	std::vector<pc_hip_ctx *> ctxs;
	for (const pc_select_member &mb : sel->m) ctxs.push_back(mb.ctx);
	std::vector<pc_spot_src> src;
	long long n = 0;
	int st = pc_tally_sources(ctxs, sel->group, kind, who, src, &n);
	if (st) return st;
	for (size_t k = 0; k < ctxs.size(); k++)
		if (sel->m[k].epoch[kind] != ctxs[k]->entries_epoch || sel->m[k].n[kind] != src[k].n)
			return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_gather: the selection's mask is stale: the entries of kind " + std::to_string(kind)
			               + " were replaced after it was applied");
	st = pc_select_fetch(sel, kind);
	if (st) return st;
	long long n_pass = 0;
	for (const pc_select_member &mb : sel->m) n_pass += mb.n_pass[kind];
	if (!pc_gather_window_check(first, count, n_pass, &why)) return pc_fail(PC_HIP_ERR_INVALID, why);
	if (count == 0) return PC_HIP_OK;
	const int ne = sel->ne, nf = kind == 0 ? PC_N_FIELDS : PC_HIP_LEAK_HDR, row = nf + ne;
	/* the members' passing entries one after the other; a member's positions begin behind the entries of the members before it */
	long long pass0 = 0, pos0 = 0;
	for (size_t k = 0; k < sel->m.size(); k++) {
		pc_select_member &mb = sel->m[k];
		const long long lo = std::max<long long>(first, pass0), hi = std::min<long long>(first + count, pass0 + mb.n_pass[kind]);
		if (hi > lo) {
			st = pc_gather_member(mb, src[k], kind, nf, row, lo - pass0, hi - lo, pos0, records + (size_t)(lo - first)*(size_t)row,
			                      positions ? positions + (lo - first) : nullptr);
			if (st) return st;
		}
		pass0 += mb.n_pass[kind];
		pos0 += mb.n[kind];
	}
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_GATHER_HOST_ONLY */
#endif /* PC_GATHER_H */

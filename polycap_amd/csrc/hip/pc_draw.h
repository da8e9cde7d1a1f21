/*
 * pc_draw.h -- an unweighted sample of the entries a selection keeps (include/polycap-hip.h, pc_hip_select_draw): systematic resampling
 * in exact integers.  Entry i of a kind, in the position order of the gathers, has V_i = q(w[e]) where its mask byte is set and 0
 * otherwise, C_i = V_0 + ... + V_i, T = C_{n-1}.  Draw k of N with phase r has the threshold
 *     t_k = floor((k*2^32 + r)*T / (N*2^32))            0 <= t_k < T, non-decreasing in k
 * and lands on the smallest i with C_i > t_k.  A post-pass like the gathers: it reads the mask and one weight column through
 * pc_spot_src, and the rows leave through pc_gather_rows_kernel and the gathers' staging buffer.
 *
 * Per member of the selection:
 *   a. pc_draw_sum_kernel    the sum of V over every tile of "gather_tile" entries
 *   b. pc_draw_scan_kernel   the exclusive scan of the tile sums, by one workgroup that loops over the tiles with a carry; its last
 *                            element is the member's T_j.  (a) and (b) are kept per member for one (kind, energy, tile) until the
 *                            next apply
 *   c. the host gives the member its base B_j, the sum of the T of the members before it, and the draws [K(B_j), K(B_j + T_j)) cut to
 *      the window, where K(c) = #{k : t_k < c}
 *   d. pc_draw_place_kernel  one workgroup per tile: the tile's draws from K at its two cumulative bounds, cut to the member's; the
 *                            tile's V scanned in passes of a workgroup's width with a running carry; every draw of a pass finds its
 *                            entry by a search in the pass's scanned values in LDS and writes the entry's local position at k - k_lo
 *   e. pc_gather_rows_kernel the rows of that list, chunk by chunk
 * Every draw has exactly one tile, one pass and one lane: no atomic decides a place, and the cost grows with the entries and the
 * window, never with N.
 *
 * The first part (the arithmetic, the argument and window checks) compiles for the host as well and is written on 32- and 64-bit limbs
 * for both sides: -DPC_DRAW_HOST_ONLY stops the header after it.
 */
#ifndef PC_DRAW_H
#define PC_DRAW_H

#include <stdint.h>
#include <string>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define PC_DRAW_N_MAX 0x7fffffffll

/* a*b as (lo, hi), from four 32 x 32 -> 64 products */
static inline __host__ __device__ void pc_draw_mul64(unsigned long long a, unsigned long long b, unsigned long long *lo, unsigned long long *hi)
{
	const unsigned long long M = 0xffffffffull;
	const unsigned long long a0 = a & M, a1 = a >> 32, b0 = b & M, b1 = b >> 32;
	const unsigned long long p00 = a0*b0, p01 = a0*b1, p10 = a1*b0, p11 = a1*b1;
	const unsigned long long mid = (p00 >> 32) + (p01 & M) + (p10 & M);      /* < 3 * 2^32 */
	*lo = (p00 & M) | (mid << 32);
	*hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

/* t_k for 0 <= k < N, 1 <= N <= 2^31 - 1: the product (k*2^32 + r)*T < 2^127, its upper 96 bits (the shift by 32 commutes with the
 * floor of the division), and those divided by N limb by limb.  The quotient is below T, so its top limb is 0. */
static inline __host__ __device__ unsigned long long pc_draw_threshold(unsigned long long k, unsigned int phase, unsigned long long T, unsigned long long N)
{
	const unsigned long long M = 0xffffffffull;
	unsigned long long lo, hi;
	pc_draw_mul64((k << 32) | (unsigned long long)phase, T, &lo, &hi);
	const unsigned long long q2 = hi >> 32, q1 = hi & M, q0 = lo >> 32;
	unsigned long long cur = ((q2 % N) << 32) | q1;
	const unsigned long long d1 = cur / N;
	cur = ((cur % N) << 32) | q0;
	return (d1 << 32) | (cur / N);
}

/* K(c) = #{k in [0, N) : t_k < c}: t_k does not decrease with k, so the smallest k with t_k >= c, by bisection; N where there is none */
static inline __host__ __device__ unsigned long long pc_draw_below(unsigned long long c, unsigned int phase, unsigned long long T, unsigned long long N)
{
	unsigned long long lo = 0, hi = N;      /* every k < lo has t_k < c, every k >= hi has t_k >= c */
	while (lo < hi) {
		const unsigned long long mid = lo + ((hi - lo) >> 1);
		if (pc_draw_threshold(mid, phase, T, N) < c) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

/* what pc_hip_select_draw refuses before it looks at the device: the reason names the function and the field */
static inline bool pc_draw_args_check(const void *select, int kind, long long energy, long long n_energies, long long n_draw, long long first,
	long long count, const void *records, std::string *why)
{
	if (!select) *why = "pc_hip_select_draw: select must not be NULL";
	else if (kind < 0 || kind > 2) *why = "pc_hip_select_draw: kind must be 0 (exit photons), 1 (extleak) or 2 (intleak), got " + std::to_string(kind);
	else if (energy < 0 || energy >= n_energies)
		*why = "pc_hip_select_draw: energy must be an index in [0, " + std::to_string(n_energies) + "), got " + std::to_string(energy);
	else if (n_draw < 1 || n_draw > PC_DRAW_N_MAX) *why = "pc_hip_select_draw: n_draw must be in [1, 2^31 - 1], got " + std::to_string(n_draw);
	else if (first < 0) *why = "pc_hip_select_draw: first must be >= 0, got " + std::to_string(first);
	else if (count < 0) *why = "pc_hip_select_draw: count must be >= 0, got " + std::to_string(count);
	else if (count > 0 && !records) *why = "pc_hip_select_draw: records must not be NULL when count > 0";
	return why->empty();
}

/* the window against the sample, and the weight there is to draw from (known once the selection was applied) */
static inline bool pc_draw_window_check(long long first, long long count, long long n_draw, unsigned long long total, std::string *why)
{
	if (first > n_draw || count > n_draw - first)
		*why = "pc_hip_select_draw: first + count = " + std::to_string(first) + " + " + std::to_string(count) + " exceeds n_draw = "
		       + std::to_string(n_draw);
	else if (total == 0)
		*why = "pc_hip_select_draw: total is 0: no weight to draw from (no passing entry of that kind has weight at that energy)";
	return why->empty();
}

/* the draws of the cumulative range [c_lo, c_hi) that fall into [first, first + count): [*k_lo, *k_hi), empty as k_lo = k_hi */
static inline __host__ __device__ void pc_draw_range(unsigned long long c_lo, unsigned long long c_hi, unsigned int phase, unsigned long long T,
	unsigned long long N, unsigned long long first, unsigned long long count, unsigned long long *k_lo, unsigned long long *k_hi)
{
	unsigned long long a = pc_draw_below(c_lo, phase, T, N), b = pc_draw_below(c_hi, phase, T, N);
	if (a < first) a = first;
	if (b > first + count) b = first + count;
	if (b < a) b = a;
	*k_lo = a; *k_hi = b;
}

#ifndef PC_DRAW_HOST_ONLY

#define PC_DRAW_BLOCK 256

/* V of entry i at energy e */
static __device__ __forceinline__ unsigned long long pc_draw_v(const pc_spot_src &s, const unsigned char *mask, int e, long long i)
{
	return mask[i] ? pc_spot_q(s.w[i*s.ws + e]) : 0ull;
}

/* a. sum[t] = the sum of V over tile t; workgroup x takes the tiles x, x + gridDim.x, ... */
__global__ void __launch_bounds__(PC_DRAW_BLOCK) pc_draw_sum_kernel(pc_spot_src s, const unsigned char *mask, int e, long long tile, long long tiles,
	unsigned long long *sum)
{
	__shared__ unsigned long long part[PC_DRAW_BLOCK/64];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
		const long long lo = t*tile, hi = (lo + tile < s.n) ? lo + tile : s.n;
		unsigned long long v = 0ull;
		for (long long i = lo + threadIdx.x; i < hi; i += PC_DRAW_BLOCK) v += pc_draw_v(s, mask, e, i);
		for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
		if (lane == 0) part[wave] = v;
		__syncthreads();
		if (threadIdx.x == 0) {
			unsigned long long a = 0ull;
			for (int w = 0; w < PC_DRAW_BLOCK/64; w++) a += part[w];
			sum[t] = a;
		}
		__syncthreads();
	}
}

/* the inclusive scan of v over the workgroup: *before = the sum of the lanes below this one, *total = the workgroup's sum.  wsum:
 * PC_DRAW_BLOCK/64 words of LDS, free again after the call's last barrier. */
static __device__ __forceinline__ unsigned long long pc_draw_block_scan(unsigned long long v, unsigned long long *wsum, unsigned long long *total)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long incl = v;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long up = __shfl_up(incl, d);
		if (lane >= d) incl += up;
	}
	if (lane == 63) wsum[wave] = incl;
	__syncthreads();
	unsigned long long before = 0ull, all = 0ull;
	for (int w = 0; w < PC_DRAW_BLOCK/64; w++) {
		if (w < wave) before += wsum[w];
		all += wsum[w];
	}
	__syncthreads();
	*total = all;
	return before + incl;
}

/* b. off[t] = sum[0] + ... + sum[t - 1] for t = 0 .. tiles (off[tiles] = the member's T).  One workgroup. */
__global__ void __launch_bounds__(PC_DRAW_BLOCK) pc_draw_scan_kernel(const unsigned long long *sum, long long tiles, unsigned long long *off)
{
	__shared__ unsigned long long wsum[PC_DRAW_BLOCK/64];
	unsigned long long carry = 0ull;
	for (long long base = 0; base < tiles; base += PC_DRAW_BLOCK) {
		const long long t = base + threadIdx.x;
		const unsigned long long v = (t < tiles) ? sum[t] : 0ull;
		unsigned long long total;
		const unsigned long long incl = pc_draw_block_scan(v, wsum, &total);
		if (t < tiles) off[t] = carry + incl - v;
		carry += total;
	}
	if (threadIdx.x == 0) off[tiles] = carry;
}

/* what (d) needs beside the entries */
struct pc_draw_job {
	unsigned long long T, N;            /* of the whole selection */
	unsigned long long base;            /* B_j: the T of the members before this one */
	unsigned long long k_lo, k_hi;      /* the member's draws inside the window; list[k - k_lo] */
	unsigned int phase;
	int e;
};

/* d. workgroup t places the draws of tile t.  The tile's draws are those with base + off[t] <= t_k < base + off[t + 1]; a pass scans
 * PC_DRAW_BLOCK entries into cum[] (C_i of the whole selection, inclusive), and since t_k does not decrease with k the draws of the
 * pass are the next ones in line: lane j tries draw k_cur + j, and as many as were below the pass's upper bound are consumed. */
__global__ void __launch_bounds__(PC_DRAW_BLOCK) pc_draw_place_kernel(pc_spot_src s, const unsigned char *mask, long long tile, long long tiles,
	const unsigned long long *off, pc_draw_job jb, unsigned int *list)
{
	__shared__ unsigned long long cum[PC_DRAW_BLOCK];
	__shared__ unsigned long long wsum[PC_DRAW_BLOCK/64];
	__shared__ unsigned long long kr[2];
	__shared__ unsigned int taken[PC_DRAW_BLOCK/64];
	const long long t = blockIdx.x;
	if (t >= tiles) return;
	const unsigned long long c_lo = jb.base + off[t], c_hi = jb.base + off[t + 1];
	if (c_hi == c_lo) return;                      /* nothing to land on */
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	/* the two bisections side by side, on the first lanes of two waves */
	if (threadIdx.x == 0) kr[0] = pc_draw_below(c_lo, jb.phase, jb.T, jb.N);
	if (threadIdx.x == 64) kr[1] = pc_draw_below(c_hi, jb.phase, jb.T, jb.N);
	__syncthreads();
	unsigned long long k_cur = kr[0] > jb.k_lo ? kr[0] : jb.k_lo;
	const unsigned long long k_end = kr[1] < jb.k_hi ? kr[1] : jb.k_hi;
	if (k_cur >= k_end) return;                    /* uniform over the workgroup */
	const long long lo = t*tile, hi = (lo + tile < s.n) ? lo + tile : s.n;
	unsigned long long carry = c_lo;
	for (long long base = lo; base < hi && k_cur < k_end; base += PC_DRAW_BLOCK) {
		const long long i = base + threadIdx.x;
		const unsigned long long v = (i < hi) ? pc_draw_v(s, mask, jb.e, i) : 0ull;
		unsigned long long total;
		cum[threadIdx.x] = carry + pc_draw_block_scan(v, wsum, &total);
		const unsigned long long top = carry + total;
		__syncthreads();
		for (;;) {
			const unsigned long long k = k_cur + threadIdx.x;
			int in = 0;
			if (k < k_end) {
				const unsigned long long tk = pc_draw_threshold(k, jb.phase, jb.T, jb.N);
				if (tk < top) {
					in = 1;
					int a = 0, b = PC_DRAW_BLOCK - 1;      /* the smallest j with cum[j] > tk: cum[BLOCK - 1] = top > tk */
					while (a < b) {
						const int m = (a + b) >> 1;
						if (cum[m] > tk) b = m;
						else a = m + 1;
					}
					if (k >= jb.k_lo && base + a < hi) list[k - jb.k_lo] = (unsigned int)(base + a);
				}
			}
			const unsigned int mine = (unsigned int)__popcll(__ballot(in));
			if (lane == 0) taken[wave] = mine;
			__syncthreads();
			unsigned int cnt = 0;
			for (int w = 0; w < PC_DRAW_BLOCK/64; w++) cnt += taken[w];
			__syncthreads();
			k_cur += cnt;
			if (cnt < PC_DRAW_BLOCK) break;            /* a draw of this round belongs to a later pass, or none is left */
		}
		carry = top;
	}
}

/* the tile sums and their scan of member mb for (kind, energy, tile), on its stream (its device is current) unless they are there */
static int pc_draw_sums(pc_select_member &mb, const pc_spot_src &src, int kind, int e, const pc_gather_tiling &tl)
{
	if (mb.draw_valid && mb.draw_kind == kind && mb.draw_energy == e && mb.draw_tile == tl.tile) return PC_HIP_OK;
	pc_hip_ctx *c = mb.ctx;
	mb.draw_valid = 0;
	mb.draw_total = 0ull;
	if (tl.tiles > 0) {
		int st = mb.d_draw_sum.grow((size_t)tl.tiles, "pc_hip_select_draw: could not allocate the tile sums");
		if (!st) st = mb.d_draw_off.grow((size_t)tl.tiles + 1, "pc_hip_select_draw: could not allocate the tile offsets");
		if (st) return st;
		const long long cap = 8ll*c->n_cu;
		const unsigned grid = (unsigned)(tl.tiles < cap ? tl.tiles : cap);
		hipLaunchKernelGGL(pc_draw_sum_kernel, dim3(grid), dim3(PC_DRAW_BLOCK), 0, c->stream, src, (const unsigned char *)mb.d_mask[kind], e, tl.tile, tl.tiles,
		                   (unsigned long long *)mb.d_draw_sum);
		PC_HIP_CHECK(hipGetLastError());
		hipLaunchKernelGGL(pc_draw_scan_kernel, dim3(1), dim3(PC_DRAW_BLOCK), 0, c->stream, (const unsigned long long *)mb.d_draw_sum, tl.tiles,
		                   (unsigned long long *)mb.d_draw_off);
		PC_HIP_CHECK(hipGetLastError());
		PC_HIP_CHECK(hipMemcpyAsync(&mb.draw_total, mb.d_draw_off + tl.tiles, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
		PC_HIP_CHECK(hipStreamSynchronize(c->stream));
	}
	mb.draw_kind = kind; mb.draw_energy = e; mb.draw_tile = tl.tile;
	mb.draw_valid = 1;
	return PC_HIP_OK;
}

/* draws [jb.k_lo, jb.k_hi) of member mb to records and positions (positions may be NULL); pos0: the member's first global position */
static int pc_draw_member(pc_select_member &mb, const pc_spot_src &src, int kind, const pc_gather_tiling &tl, const pc_draw_job &jb, int nf, int row,
	long long pos0, double *records, int64_t *positions)
{
	pc_hip_ctx *c = mb.ctx;
	const long long cnt = (long long)(jb.k_hi - jb.k_lo);
	int st = mb.d_draw_list.grow((size_t)cnt, "pc_hip_select_draw: could not allocate the list of the draws");
	if (st) return st;
	unsigned int *list = mb.d_draw_list;
	/* a draw that no tile placed would leave its word as it was: 0xff.. is no position (a kind has at most 2^32 - 1 entries) */
	PC_HIP_CHECK(hipMemsetAsync(list, 0xff, (size_t)cnt*sizeof(unsigned int), c->stream));
	hipLaunchKernelGGL(pc_draw_place_kernel, dim3((unsigned)tl.tiles), dim3(PC_DRAW_BLOCK), 0, c->stream, src, (const unsigned char *)mb.d_mask[kind], tl.tile,
	                   tl.tiles, (const unsigned long long *)mb.d_draw_off, jb, list);
	PC_HIP_CHECK(hipGetLastError());
	std::vector<unsigned int> local((size_t)cnt);
	PC_HIP_CHECK(hipMemcpyAsync(local.data(), list, (size_t)cnt*sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
	PC_HIP_CHECK(hipStreamSynchronize(c->stream));
	for (long long k = 0; k < cnt; k++) {
		if ((long long)local[(size_t)k] >= src.n)
			return pc_fail(PC_HIP_ERR_RUNTIME, "pc_hip_select_draw: draw " + std::to_string(jb.k_lo + (unsigned long long)k) + " was not placed");
		if (positions) positions[k] = pos0 + (int64_t)local[(size_t)k];
	}
	long long rows = pc_gather_chunk_rows(c->gather_chunk_rows, row);
	if (rows > cnt) rows = cnt;
	st = mb.d_stage.grow((size_t)rows*(size_t)row, "pc_hip_select_draw: could not allocate the staging buffer");
	if (st) return st;
	const long long chunks = pc_gather_n_chunks(cnt, rows);
	for (long long k = 0; k < chunks; k++) {
		long long r0, nr;
		pc_gather_chunk(0, cnt, rows, k, &r0, &nr);
		const long long bx = pc_tally_grid_cap(8ll*c->n_cu, nr*row, PC_GATHER_BLOCK);
		hipLaunchKernelGGL(pc_gather_rows_kernel, dim3((unsigned)bx), dim3(PC_GATHER_BLOCK), 0, c->stream, src, nf, row, (const unsigned int *)list, r0, nr,
		                   (unsigned long long *)mb.d_stage);
		PC_HIP_CHECK(hipGetLastError());
		PC_HIP_CHECK(hipMemcpyAsync(records + (size_t)r0*(size_t)row, mb.d_stage, (size_t)nr*(size_t)row*sizeof(double), hipMemcpyDeviceToHost, c->stream));
		PC_HIP_CHECK(hipStreamSynchronize(c->stream));      /* the next chunk writes the same buffer */
	}
	return PC_HIP_OK;
}

extern "C" {

int pc_hip_select_draw(pc_hip_select *sel, int kind, int32_t energy, int64_t n_draw, uint32_t phase, int64_t first, int64_t count, double *records,
	int64_t *positions, uint64_t *total)
{
	static const char *who = "pc_hip_select_draw";
	std::string why;
	if (!pc_draw_args_check(sel, kind, energy, sel ? sel->ne : 0, n_draw, first, count, records, &why)) return pc_fail(PC_HIP_ERR_INVALID, why);
	if (!sel->applied[kind])
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_draw: the selection was not applied for kind " + std::to_string(kind) + " (pc_hip_select_apply)");
	std::vector<pc_hip_ctx *> ctxs;
	for (const pc_select_member &mb : sel->m) ctxs.push_back(mb.ctx);
	std::vector<pc_spot_src> src;
	long long n = 0;
	int st = pc_tally_sources(ctxs, sel->group, kind, who, src, &n);
	if (st) return st;
	for (size_t k = 0; k < ctxs.size(); k++)
		if (sel->m[k].epoch[kind] != ctxs[k]->entries_epoch || sel->m[k].n[kind] != src[k].n)
			return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_draw: the selection's mask is stale: the entries of kind " + std::to_string(kind)
			               + " were replaced after it was applied");
	st = pc_select_fetch(sel, kind);
	if (st) return st;
	const unsigned long long T = sel->tot[(size_t)kind*(2 + 2*(size_t)sel->ne) + 2 + (size_t)energy];      /* passed_w[kind][energy] */
	if (!pc_draw_window_check(first, count, n_draw, T, &why)) return pc_fail(PC_HIP_ERR_INVALID, why);
	if (total) *total = T;
	if (count == 0) return PC_HIP_OK;
	/* a, b: every member's tile sums and its T_j; together they are what the apply summed */
	std::vector<pc_gather_tiling> tl(sel->m.size());
	unsigned long long sum = 0ull;
	for (size_t k = 0; k < sel->m.size(); k++) {
		pc_select_member &mb = sel->m[k];
		tl[k] = pc_gather_plan(mb.n[kind], mb.ctx->gather_tile);
		PC_HIP_CHECK(hipSetDevice(mb.ctx->device));
		st = pc_draw_sums(mb, src[k], kind, energy, tl[k]);
		if (st) return st;
		sum += mb.draw_total;
	}
	if (sum != T) {
		for (pc_select_member &mb : sel->m) mb.draw_valid = 0;
		return pc_fail(PC_HIP_ERR_RUNTIME, "pc_hip_select_draw: the tile sums add up to " + std::to_string(sum) + " where the apply summed " + std::to_string(T));
	}
	const int ne = sel->ne, nf = kind == 0 ? PC_N_FIELDS : PC_HIP_LEAK_HDR, row = nf + ne;
	/* c, d, e: the members' cumulative ranges one after the other; a member's positions begin behind the entries of the members before it */
	unsigned long long base = 0ull;
	long long pos0 = 0;
	for (size_t k = 0; k < sel->m.size(); k++) {
		pc_select_member &mb = sel->m[k];
		pc_draw_job jb;
		jb.T = T; jb.N = (unsigned long long)n_draw; jb.base = base; jb.phase = phase; jb.e = energy;
		pc_draw_range(base, base + mb.draw_total, phase, T, jb.N, (unsigned long long)first, (unsigned long long)count, &jb.k_lo, &jb.k_hi);
		if (mb.draw_total > 0 && jb.k_hi > jb.k_lo) {
			PC_HIP_CHECK(hipSetDevice(mb.ctx->device));
			const long long at = (long long)jb.k_lo - first;
			st = pc_draw_member(mb, src[k], kind, tl[k], jb, nf, row, pos0, records + (size_t)at*(size_t)row, positions ? positions + at : nullptr);
			if (st) return st;
		}
		base += mb.draw_total;
		pos0 += mb.n[kind];
	}
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_DRAW_HOST_ONLY */
#endif /* PC_DRAW_H */

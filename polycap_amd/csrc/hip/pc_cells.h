/*
 * pc_cells.h -- the device half of the two binned tallies, histograms (pc_hist.h) and joint histograms (pc_joint.h), written once.
 * Both tally groups of A axes: a histogram is a group of one axis, whose cell is the axis' bin (pc_hist_axis_bin); a joint histogram
 * is a group of two, whose cell is pc_joint_cell of the pair.  Here are the geometry record the kernels take, the loader of an entry,
 * the two kernels (template <A, M, Q>), the regime rule, and the object with its make, launch, add, read and unpack.  pc_hist.h and
 * pc_joint.h keep the per-entry arithmetic, the check of their spec, its translation into axes, and their C functions.
 *
 * pc_hist.h includes this header between its host part and its C functions; it is not meant to be included from elsewhere.
 */
#ifndef PC_CELLS_H
#define PC_CELLS_H

static inline __host__ __device__ int pc_joint_cell(const pc_hist_axis_k &u, const pc_hist_axis_k &v, const pc_hist_entry &e);      /* pc_joint.h, in the part its host tests compile */

/* Cells.  Every group has nc + 1 cells per selected energy: its bins (A = 1: n_bins) or its [iv][iu] cells (A = 2: nu*nv), then its
 * outside counter; the cells of the groups follow each other, tc = total_cells + ng per energy.  cell0[p] = where group p starts.
 * Group p has the axes ax[A*p .. A*p + A - 1] (A = 2: u, then v), so there are PC_HIST_MAX_AXES / A groups at the most. */
struct pc_cells_geo {
	pc_hist_axis_k ax[PC_HIST_MAX_AXES];
	int cell0[PC_HIST_MAX_AXES], nc[PC_HIST_MAX_AXES];
	const int *sel;          /* [ns] energy indices */
	int ng, ns, tc;
	int need_start, need_travel, need_n;      /* which of the optional fields some axis reads */
};

/* entry i with the optional fields that some axis or cut (pc_select.h) reads: the need_* flags of the caller's record, by reference so
 * that each is read where it is used */
static __device__ __forceinline__ void pc_hist_load(const pc_spot_src &s, long long i, const int &need_start, const int &need_travel, const int &need_n,
	pc_hist_entry &e)
{
	const pc_entry b = pc_entry_load(s, i);
	const double *p = s.p + i*s.ss;
	e.x = b.x; e.y = b.y; e.z = b.z; e.dx = b.dx; e.dy = b.dy; e.dz = b.dz;
	e.leak = s.has_dz;
	e.n = e.dtravel = e.sx = e.sy = 0.;
	if (s.has_dz) {          /* a leak event: slot, attempt, coords, direction, electric vector, n_refl */
		if (need_n) e.n = p[11*s.fs];
	} else {                 /* an image record: pc_start_coords in planes 2, 3; pc_exit_nrefl (int64) in 15; pc_exit_dtravel in 16 */
		if (need_n) e.n = (double)((const long long *)p)[15*s.fs];
		if (need_travel) e.dtravel = p[16*s.fs];
		if (need_start) { e.sx = p[2*s.fs]; e.sy = p[3*s.fs]; }
	}
}

/* cell of an entry in group p, or -1 when an axis of the group puts it outside */
template <int A>
static __device__ __forceinline__ int pc_cells_cell(const pc_cells_geo &g, int p, const pc_hist_entry &e)
{
	static_assert(A == 1 || A == 2, "a group is one axis or a pair");
	if constexpr (A == 1) return pc_hist_axis_bin(g.ax[p], e);
	else return pc_joint_cell(g.ax[2*p], g.ax[2*p + 1], e);
}

/* Regime 1: workgroup-private tiles.  The cells [energy][tc] are cut into tiles of PC_CELLS_TILE uint64; workgroup (x, y) adds the
 * entries x, x + gridDim.x, ... whose cells fall into tile y to a private copy of it in LDS (ds_add_u64), one entry per lane, then
 * adds every non-zero cell of the copy to the global cells with one atomic.  Several tiles are several passes over the entries; a
 * pass of the joint histograms evaluates only the pairs that have cells in its tile.  64 KiB of LDS per workgroup: two workgroups
 * per CU (pc_tally_grid_tiles).  Where the squares are tracked (Q) a tile is TC = PC_CELLS_TILE / 3 cells (pc_tally_tile_cells):
 * their weight sums in tile[0, TC), their square sums as (lo, hi) pairs behind them, flushed with pc_atomic_add128 to sq [cell][2]. */
#define PC_CELLS_TILE 8192
#define PC_CELLS_LDS_BLOCK 512
/* M: a gated add, s.mask is set (pc_select.h); the plain build reads no mask.  Q: the squares are tracked; the build without reads no sq */
template <int A, bool M, bool Q>
__global__ void __launch_bounds__(PC_CELLS_LDS_BLOCK) pc_cells_lds_kernel(pc_spot_src s, pc_cells_geo g, unsigned long long *cells, unsigned long long *sq)
{
	__shared__ unsigned long long tile[PC_CELLS_TILE];
	constexpr long long TC = pc_tally_tile_cells(PC_CELLS_TILE, Q);
	const long long total = (long long)g.ns*g.tc;
	const long long t0 = (long long)blockIdx.y*TC;
	const long long t1 = (t0 + TC < total) ? t0 + TC : total;
	const int k0 = (int)(t0 / g.tc), k1 = (int)((t1 - 1) / g.tc);      /* the energies with cells in this tile */
	/* pair p has cells in [t0, t1) when its run of energy k0 ends behind t0 or that of a later energy starts before t1 */
	unsigned active = 0u;
	if constexpr (A == 2)
		for (int p = 0; p < g.ng; p++) {
			const long long c0 = g.cell0[p], c1 = c0 + g.nc[p] + 1;
			for (int k = k0; k <= k1; k++)
				if ((long long)k*g.tc + c1 > t0 && (long long)k*g.tc + c0 < t1) active |= 1u << p;
		}
	for (int k = threadIdx.x; k < PC_CELLS_TILE; k += blockDim.x) tile[k] = 0ull;
	__syncthreads();
	for (long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x; i < s.n; i += (long long)gridDim.x*blockDim.x) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		pc_hist_entry e;
		pc_hist_load(s, i, g.need_start, g.need_travel, g.need_n, e);
		for (int p = 0; p < g.ng; p++) {
			if (A == 2 && !(active >> p & 1u)) continue;
			const int b = pc_cells_cell<A>(g, p, e);
			const long long c = g.cell0[p] + (b >= 0 ? b : g.nc[p]);
			for (int k = k0; k <= k1; k++) {
				const long long cell = (long long)k*g.tc + c;
				if (cell < t0 || cell >= t1) continue;
				const unsigned long long q = pc_spot_q(s.w[i*s.ws + g.sel[k]]);
				if (q) {
					atomicAdd(&tile[cell - t0], q);
					if (Q) pc_tally_lds_add_sq(&tile[TC + 2*(cell - t0)], q);
				}
			}
		}
	}
	__syncthreads();
	for (long long k = threadIdx.x; k < t1 - t0; k += blockDim.x) {
		const unsigned long long v = tile[k];
		if (v) {
			atomicAdd(&cells[t0 + k], v);
			if (Q) pc_atomic_add128(sq + 2*(t0 + k), tile[TC + 2*k], tile[TC + 2*k + 1]);      /* a cell without weight has no square */
		}
	}
}

/* Regime 2: energies across lanes.  The cells are laid out [tc][energy] with the energies innermost: the lanes of a wave take the
 * energies of one entry (64 / gw entries per wave when fewer than 64 are selected, gw = the next power of two), so that one wave
 * instruction is a contiguous run of 8-byte global atomics.  Workgroup (x, c) does energies [c*EC, ...), EC = pc_cells_echunk; the
 * outside counters of those energies are summed in LDS first (every entry that misses a range adds to the same few counters): 512
 * energies for each of the 16 / A groups there can be, 64 KiB for the histograms and 32 KiB for the joint histograms.  Where the
 * squares are tracked (Q) every add to a cell is followed by pc_tally_add_sq on its pair in sq [cell][2], the outside counters' pairs
 * follow the counters in LDS, and the chunk is 2048 energies over the 16 / A groups: 48 KiB in all. */
#define PC_CELLS_ECHUNK 512
#define PC_CELLS_WIDE_BLOCK 256
static inline constexpr __host__ __device__ int pc_cells_echunk(int A, bool squares)
{
	return squares ? 2048/(PC_HIST_MAX_AXES/A) : PC_CELLS_ECHUNK;
}

template <int A, bool M, bool Q>
__global__ void __launch_bounds__(PC_CELLS_WIDE_BLOCK) pc_cells_wide_kernel(pc_spot_src s, pc_cells_geo g, unsigned long long *cells, unsigned long long *sq)
{
	constexpr int NG = PC_HIST_MAX_AXES/A, EC = pc_cells_echunk(A, Q);
	__shared__ unsigned long long out[NG*EC*(Q ? 3 : 1)];
	unsigned long long *out_sq = out + g.ng*EC;      /* [group*EC + k][2] behind the counters of the ng groups, Q only */
	const int s0 = blockIdx.y*EC;
	const int sn = (g.ns - s0 < EC) ? g.ns - s0 : EC;
	for (int k = threadIdx.x; k < g.ng*EC*(Q ? 3 : 1); k += blockDim.x) out[k] = 0ull;
	__syncthreads();
	const pc_tally_lanes l = pc_tally_lane_map(sn);
	for (long long i = l.first; i < s.n; i += l.stride) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		pc_hist_entry e;
		pc_hist_load(s, i, g.need_start, g.need_travel, g.need_n, e);
		int cell[NG];
#pragma unroll
		for (int p = 0; p < NG; p++)
			cell[p] = (p < g.ng) ? pc_cells_cell<A>(g, p, e) : -1;
		for (int k = l.sub; k < sn; k += l.gw) {
			const unsigned long long q = pc_spot_q(s.w[i*s.ws + g.sel[s0 + k]]);
			if (!q) continue;
#pragma unroll
			for (int p = 0; p < NG; p++) {
				if (p >= g.ng) break;
				if (cell[p] >= 0) {
					const long long c = (long long)(g.cell0[p] + cell[p])*g.ns + s0 + k;
					atomicAdd(cells + c, q);
					if (Q) pc_tally_add_sq(sq + 2*c, q);
				} else {
					atomicAdd(&out[p*EC + k], q);
					if (Q) pc_tally_lds_add_sq(&out_sq[2*(p*EC + k)], q);
				}
			}
		}
	}
	__syncthreads();
	for (int k = threadIdx.x; k < g.ng*EC; k += blockDim.x) {
		const int p = k / EC, j = k % EC;
		const unsigned long long v = out[k];
		if (v) {
			const long long c = (long long)(g.cell0[p] + g.nc[p])*g.ns + s0 + j;
			atomicAdd(cells + c, v);
			if (Q) pc_atomic_add128(sq + 2*c, out_sq[2*k], out_sq[2*k + 1]);
		}
	}
}

/* Regime of an object (spec->regime 0): private LDS tiles (1) when all cells of a kind fit one tile, energies across lanes (2)
 * otherwise, where regime 1 would pass over the entries once per tile.  Not measured: scripts/bench_hist.py times one add per regime
 * (one N_REFL axis of 256 bins, one X_AT axis of 2048 bins, eight mixed axes; xos1, 1e7 exit photons, 1 and 291 energies) next to the
 * spot map that holds the same X_AT axis, and scripts/bench_joint.py does so for the joint histograms (the pair (X_AT, Y_AT) at 256^2
 * and 1024^2 at one energy and at 64^2 with 291 energies, each next to the spot-map add of the same shape, and a four-pair spec) and
 * writes profiles/joint_ab.txt.  A wave-level pre-sum of lanes that hit the same cell was not built.
 * The rule is applied when the object is made and not again when it starts to track squares: with 2731 to 8192 cells a tracking
 * object stays in regime 1 and makes two or three passes over the entries (pc_tally_tile_split).  Whether regime 2 is faster there
 * has not been measured. */
static int pc_cells_auto_regime(long long ns, long long tc)
{
	return (ns*tc <= PC_CELLS_TILE) ? 1 : 2;
}

/* cells [kind][energy][tc] (regime 1) or [kind][tc][energy] (regime 2); struct pc_hip_hist and struct pc_hip_joint are this */
struct pc_cells : pc_tally {
	pc_cells_geo geo;                 /* sel is the member's own */
	std::vector<int> offsets;         /* [ng + 1] into the cells of one energy, without the outside counters */
	int regime = 0;
	size_t per_kind = 0;              /* ns * tc */
};

/* The object (T: pc_hip_hist or pc_hip_joint) of a checked spec whose groups are axes[A*p .. A*p + A - 1]; `who` is the call */
template <int A, typename T>
static int pc_cells_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const std::vector<pc_hip_hist_axis> &axes, int n_sel, const int *energies,
	int regime, const char *who, T **out)
{
	const pc_hip_ctx *c0 = ctxs[0];
	T *h = new T();
	const std::vector<int> sel = pc_sel_fill(n_sel, energies, (size_t)c0->host.pm.n_energies);
	pc_cells_geo &g = h->geo;
	memset(&g, 0, sizeof(g));
	g.ng = (int)axes.size()/A;
	g.ns = (int)sel.size();
	const double zexit = c0->host.z[c0->host.pm.nmax];
	int cells = 0;
	for (int p = 0; p < g.ng; p++) {
		g.nc[p] = 1;
		for (int w = 0; w < A; w++) {
			const pc_hip_hist_axis &x = axes[A*p + w];
			pc_hist_axis_k &a = g.ax[A*p + w];
			a.zp = zexit + x.d;          /* once, on the host */
			a.cx = x.cx; a.cy = x.cy; a.lo = x.lo; a.hi = x.hi;
			a.quantity = x.quantity; a.n_bins = x.n_bins;
			if (x.quantity == PC_HIST_N_REFL) g.need_n = 1;
			if (x.quantity == PC_HIST_D_TRAVEL) g.need_travel = 1;
			if (x.quantity == PC_HIST_R_START || x.quantity == PC_JOINT_START_X || x.quantity == PC_JOINT_START_Y) g.need_start = 1;
			g.nc[p] *= x.n_bins;
		}
		g.cell0[p] = cells + p;
		h->offsets.push_back(cells);
		cells += g.nc[p];
	}
	h->offsets.push_back(cells);
	g.tc = cells + g.ng;
	h->per_kind = (size_t)g.ns*g.tc;
	h->regime = regime ? regime : pc_cells_auto_regime(g.ns, g.tc);
	int st = pc_tally_make(*h, ctxs, group, 3*h->per_kind, who);
	if (!st) st = pc_tally_upload(*h, sel, std::vector<double>(), who);
	if (st) { delete h; return st; }
	*out = h;
	return PC_HIP_OK;
}

template <int A>
static int pc_cells_launch(pc_cells *h, pc_tally_member &m, const pc_spot_src &s, int kind)
{
	pc_hip_ctx *c = m.ctx;
	pc_cells_geo g = h->geo;
	g.sel = m.d_sel;
	unsigned long long *cells = m.d_cells + (size_t)kind*h->per_kind;
	unsigned long long *sq = h->squares ? m.d_sq + 2*(size_t)kind*h->per_kind : nullptr;
	if (h->regime == 1) {
		const long long tiles = pc_tally_tile_split((long long)h->per_kind, PC_CELLS_TILE, h->squares).tiles;
		const long long bx = pc_tally_grid_tiles(c->n_cu, tiles, s.n, PC_CELLS_LDS_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_cells_lds_kernel<A, true, true> : pc_cells_lds_kernel<A, false, true>)
		               : (s.mask ? pc_cells_lds_kernel<A, true, false> : pc_cells_lds_kernel<A, false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)tiles), dim3(PC_CELLS_LDS_BLOCK), 0, c->stream, s, g, cells, sq);
	} else {
		const int ec = pc_cells_echunk(A, sq != nullptr);
		const long long chunks = (g.ns + ec - 1)/ec;
		const long long bx = pc_tally_grid_wide(c->n_cu, chunks, g.ns, s.n, PC_CELLS_WIDE_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_cells_wide_kernel<A, true, true> : pc_cells_wide_kernel<A, false, true>)
		               : (s.mask ? pc_cells_wide_kernel<A, true, false> : pc_cells_wide_kernel<A, false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)chunks), dim3(PC_CELLS_WIDE_BLOCK), 0, c->stream, s, g, cells, sq);
	}
	return PC_HIP_OK;
}

/* pc_hip_{hist,joint}_add and _add_selected (pc_select.h) behind their NULL checks */
template <int A>
static int pc_cells_add(pc_cells *h, int kind, const char *who, pc_hip_select *sel = nullptr)
{
	return pc_tally_add(*h, kind, who, [h](size_t k, const pc_spot_src &s, int kd) { return pc_cells_launch<A>(h, h->m[k], s, kd); }, sel);
}

/* the members' summed cells (limbs = 1) or square pairs (limbs = 2) from the device layout of the regime into cells
 * [3][ns][total_cells][limbs] and outside [3][ng][ns][limbs]; either may be NULL */
static void pc_cells_unpack(const pc_cells *h, const std::vector<unsigned long long> &sum, size_t limbs, uint64_t *cells, uint64_t *outside)
{
	const pc_cells_geo &g = h->geo;
	const size_t ns = (size_t)g.ns, tc = (size_t)g.tc, total = tc - (size_t)g.ng;
	for (size_t kind = 0; kind < 3; kind++)
		for (size_t s = 0; s < ns; s++)
			for (int p = 0; p < g.ng; p++) {
				const size_t c0 = (size_t)g.cell0[p], nc = (size_t)g.nc[p];
				for (size_t b = 0; b <= nc; b++) {
					const unsigned long long *v = &sum[limbs*(kind*h->per_kind + (h->regime == 1 ? s*tc + c0 + b : (c0 + b)*ns + s))];
					uint64_t *to = nullptr;
					if (b < nc) { if (cells) to = cells + limbs*((kind*ns + s)*total + (size_t)h->offsets[p] + b); }
					else if (outside) to = outside + limbs*((kind*(size_t)g.ng + (size_t)p)*ns + s);
					for (size_t l = 0; to && l < limbs; l++) to[l] = v[l];
				}
			}
}

/* pc_hip_{hist,joint}_read, _read_squares and _info behind their NULL checks */
static int pc_cells_read(pc_cells *h, uint64_t *cells, uint64_t *outside, int64_t *n_entries)
{
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum(*h, 1, sum);
	if (st) return st;
	pc_cells_unpack(h, sum, 1, cells, outside);
	if (n_entries)
		for (int k = 0; k < 3; k++) n_entries[k] = h->n_entries[k];
	return PC_HIP_OK;
}

static int pc_cells_read_squares(pc_cells *h, const char *who, uint64_t *cells_sq, uint64_t *outside_sq)
{
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum_squares(*h, who, sum);
	if (st) return st;
	pc_cells_unpack(h, sum, 2, cells_sq, outside_sq);
	return PC_HIP_OK;
}

static int pc_cells_info(const pc_cells *h, int32_t dims[3], int32_t *offsets, int *regime)
{
	dims[0] = h->geo.ng; dims[1] = h->geo.ns; dims[2] = h->offsets.back();
	if (offsets)
		for (size_t k = 0; k < h->offsets.size(); k++) offsets[k] = h->offsets[k];
	if (regime) *regime = h->regime;
	return PC_HIP_OK;
}

#endif /* PC_CELLS_H */

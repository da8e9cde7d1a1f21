/*
 * pc_joint.h -- joint histograms: weighted 2-D histograms of two per-entry scalar quantities of the last run, one per pair of axes
 * (u, v) and selected energy (include/polycap-hip.h, pc_hip_joint_*): phase-space diagrams (x against dx/dz), the transmission map
 * of the entrance face (start x against start y), reflection count against entrance radius.  A spot map is the pair (X_AT d, Y_AT d).
 * One post-pass over the entries a histogram reads (pc_spot_source) computes both bins of every pair of an entry once and adds its
 * weights; nothing is uploaded and no trace kernel is involved.  Sums are exact integer sums (uint64, weights quantised to 2^-32),
 * kept per kind, so they depend on the set of entries only: not on launch shape, entry order, how the slots were split into runs,
 * or the device count.
 *
 * The value and the bin of an axis are pc_hist.h's (pc_hist_value with the two start coordinates, pc_hist_bin), the weights are
 * pc_spot.h's (pc_spot_q), the object is pc_tally.h's.  The first part (the cell of an entry, the marginals, the check of a spec) compiles for the host
 * as well: -DPC_JOINT_HOST_ONLY stops the header after it.
 */
#ifndef PC_JOINT_H
#define PC_JOINT_H

#include "pc_hist.h"

#define PC_JOINT_MAX_PAIRS 8

/* cell of an entry in a pair's [iv][iu] cells, or -1 when either axis puts it outside */
static inline __host__ __device__ int pc_joint_cell(const pc_hist_axis_k &u, const pc_hist_axis_k &v, const pc_hist_entry &e)
{
	const int iu = pc_hist_axis_bin(u, e), iv = pc_hist_axis_bin(v, e);
	return (iu >= 0 && iv >= 0) ? iv*u.n_bins + iu : -1;
}

/* pc_hip_joint_marginal: the sums over v (which = 0: out [nu]) or over u (which = 1: out [nv]) of cells [nv][nu] */
static inline void pc_joint_marginal(int32_t nu, int32_t nv, const uint64_t *cells, int which, uint64_t *out)
{
	for (int32_t k = 0; k < (which ? nv : nu); k++) out[k] = 0;
	for (int32_t iv = 0; iv < nv; iv++)
		for (int32_t iu = 0; iu < nu; iu++)
			out[which ? iv : iu] += cells[(size_t)iv*nu + iu];
}

/* pc_hip_joint_validate (Spec: pc_hip_joint_spec): false and the reason in *why (it names the field) when the spec is refused */
template <typename Spec>
static bool pc_joint_spec_check(const Spec *spec, size_t n_energies, std::string *why)
{
	const auto no = [why](const std::string &w) { *why = w; return false; };
	if (!spec) return no("spec must not be NULL");
	if (spec->n_pairs < 1 || spec->n_pairs > PC_JOINT_MAX_PAIRS || !spec->pairs)
		return no("n_pairs: 1 to 8 pairs are needed, got " + std::to_string(spec->n_pairs));
	double cells = 0.;
	for (int p = 0; p < spec->n_pairs; p++) {
		for (int w = 0; w < 2; w++) {
			std::string bad;
			if (!pc_hist_axis_check(w ? spec->pairs[p].v : spec->pairs[p].u, PC_JOINT_N_QUANTITIES, &bad))
				return no("pair " + std::to_string(p) + ": axis " + (w ? "v" : "u") + ": " + bad);
		}
		cells += (double)spec->pairs[p].u.n_bins*(double)spec->pairs[p].v.n_bins;
	}
	if (spec->regime < 0 || spec->regime > 2)
		return no("regime must be 0 (automatic), 1 (private LDS tiles) or 2 (energies across lanes)");
	if (!pc_sel_check(spec->n_energies, spec->energies, n_energies, why))
		return false;
	const double ns = spec->n_energies ? (double)spec->n_energies : (double)n_energies;
	if (cells*ns > (double)(1ll << 26))
		return no("n_bins: (sum of the pairs' cells nu * nv) * selected energies exceeds 2^26");
	return true;
}

#ifndef PC_JOINT_HOST_ONLY

/* Cells.  Every pair has nu*nv + 1 cells per selected energy: its [iv][iu] cells, then its outside counter; the cells of the pairs
 * follow each other, tc = total_cells + n_pairs per energy.  cell0[p] = where pair p starts, nc[p] = nu*nv. */
struct pc_joint_geo {
	pc_hist_axis_k ax[2*PC_JOINT_MAX_PAIRS];      /* u of pair p at 2p, v at 2p + 1 */
	int cell0[PC_JOINT_MAX_PAIRS], nc[PC_JOINT_MAX_PAIRS];
	const int *sel;          /* [ns] energy indices */
	int np, ns, tc;
	int need_start, need_travel, need_n;      /* which of the optional fields some axis reads (pc_hist_load) */
};

/* Regime 1: workgroup-private tiles.  The cells [energy][tc] are cut into tiles of PC_JOINT_TILE uint64; workgroup (x, y) adds the
 * entries x, x + gridDim.x, ... whose cells fall into tile y to a private copy of it in LDS (ds_add_u64), one entry per lane, then
 * adds every non-zero cell of the copy to the global cells with one atomic.  Several tiles are several passes over the entries;
 * a pass evaluates only the pairs that have cells in its tile.  64 KiB of LDS per workgroup: two workgroups per CU
 * (pc_tally_grid_tiles).  Where the squares are tracked (Q) a tile is TC = PC_JOINT_TILE / 3 cells (pc_tally_tile_cells): their
 * weight sums in tile[0, TC), their square sums as (lo, hi) pairs behind them, flushed with pc_atomic_add128 to sq [cell][2]. */
#define PC_JOINT_TILE 8192
#define PC_JOINT_LDS_BLOCK 512
/* M: a gated add, s.mask is set (pc_select.h); the plain build reads no mask.  Q: the squares are tracked; the build without reads no sq */
template <bool M, bool Q>
__global__ void __launch_bounds__(PC_JOINT_LDS_BLOCK) pc_joint_lds_kernel(pc_spot_src s, pc_joint_geo g, unsigned long long *cells, unsigned long long *sq)
{
	__shared__ unsigned long long tile[PC_JOINT_TILE];
	constexpr long long TC = pc_tally_tile_cells(PC_JOINT_TILE, Q);
	const long long total = (long long)g.ns*g.tc;
	const long long t0 = (long long)blockIdx.y*TC;
	const long long t1 = (t0 + TC < total) ? t0 + TC : total;
	const int k0 = (int)(t0 / g.tc), k1 = (int)((t1 - 1) / g.tc);      /* the energies with cells in this tile */
	/* pair p has cells in [t0, t1) when its run of energy k0 ends behind t0 or that of a later energy starts before t1 */
	unsigned active = 0u;
	for (int p = 0; p < g.np; p++) {
		const long long c0 = g.cell0[p], c1 = c0 + g.nc[p] + 1;
		for (int k = k0; k <= k1; k++)
			if ((long long)k*g.tc + c1 > t0 && (long long)k*g.tc + c0 < t1) active |= 1u << p;
	}
	for (int k = threadIdx.x; k < PC_JOINT_TILE; k += blockDim.x) tile[k] = 0ull;
	__syncthreads();
	for (long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x; i < s.n; i += (long long)gridDim.x*blockDim.x) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		pc_hist_entry e;
		pc_hist_load(s, g, i, e);
		for (int p = 0; p < g.np; p++) {
			if (!(active >> p & 1u)) continue;
			const int b = pc_joint_cell(g.ax[2*p], g.ax[2*p + 1], e);
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
 * instruction is a contiguous run of 8-byte global atomics.  Workgroup (x, c) does energies [c*PC_JOINT_ECHUNK, ...); the outside
 * counters of those energies are summed in LDS first (every entry that misses a range adds to the same few counters; 32 KiB).
 * Where the squares are tracked (Q) every add to a cell is followed by pc_tally_add_sq on its pair in sq [cell][2], the chunk is
 * PC_JOINT_ECHUNK_SQ energies and the outside counters' pairs follow the counters in LDS (48 KiB in all). */
#define PC_JOINT_ECHUNK 512
#define PC_JOINT_ECHUNK_SQ 256
#define PC_JOINT_WIDE_BLOCK 256
template <bool M, bool Q>
__global__ void __launch_bounds__(PC_JOINT_WIDE_BLOCK) pc_joint_wide_kernel(pc_spot_src s, pc_joint_geo g, unsigned long long *cells, unsigned long long *sq)
{
	constexpr int EC = Q ? PC_JOINT_ECHUNK_SQ : PC_JOINT_ECHUNK;
	__shared__ unsigned long long out[PC_JOINT_MAX_PAIRS*EC*(Q ? 3 : 1)];
	unsigned long long *out_sq = out + g.np*EC;      /* [pair*EC + k][2] behind the counters of the np pairs, Q only */
	const int s0 = blockIdx.y*EC;
	const int sn = (g.ns - s0 < EC) ? g.ns - s0 : EC;
	for (int k = threadIdx.x; k < g.np*EC*(Q ? 3 : 1); k += blockDim.x) out[k] = 0ull;
	__syncthreads();
	const pc_tally_lanes l = pc_tally_lane_map(sn);
	for (long long i = l.first; i < s.n; i += l.stride) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		pc_hist_entry e;
		pc_hist_load(s, g, i, e);
		int cell[PC_JOINT_MAX_PAIRS];
#pragma unroll
		for (int p = 0; p < PC_JOINT_MAX_PAIRS; p++)
			cell[p] = (p < g.np) ? pc_joint_cell(g.ax[2*p], g.ax[2*p + 1], e) : -1;
		for (int k = l.sub; k < sn; k += l.gw) {
			const unsigned long long q = pc_spot_q(s.w[i*s.ws + g.sel[s0 + k]]);
			if (!q) continue;
#pragma unroll
			for (int p = 0; p < PC_JOINT_MAX_PAIRS; p++) {
				if (p >= g.np) break;
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
	for (int k = threadIdx.x; k < g.np*EC; k += blockDim.x) {
		const int p = k / EC, j = k % EC;
		const unsigned long long v = out[k];
		if (v) {
			const long long c = (long long)(g.cell0[p] + g.nc[p])*g.ns + s0 + j;
			atomicAdd(cells + c, v);
			if (Q) pc_atomic_add128(sq + 2*c, out_sq[2*k], out_sq[2*k + 1]);
		}
	}
}

/* Regime of an object (spec->regime 0), the histograms' rule: private LDS tiles (1) when all cells of a kind fit one tile, energies
 * across lanes (2) otherwise, where regime 1 would pass over the entries once per tile.  Not measured for this tally:
 * scripts/bench_joint.py times one add per regime (the pair (X_AT, Y_AT) at 256^2 and 1024^2 at one energy and at 64^2 with 291
 * energies, each next to the spot-map add of the same shape, and a four-pair spec; xos1, 1e7 exit photons) and writes
 * profiles/joint_ab.txt.  As for the histograms the rule is not applied again when the object starts to track squares (two or three
 * passes in regime 1 with 2731 to 8192 cells; not measured against regime 2). */
static int pc_joint_auto_regime(long long ns, long long tc)
{
	return (ns*tc <= PC_JOINT_TILE) ? 1 : 2;
}

/* cells [kind][energy][tc] (regime 1) or [kind][tc][energy] (regime 2) */
struct pc_hip_joint : pc_tally {
	pc_joint_geo geo;                 /* sel is the member's own */
	std::vector<int> offsets;         /* [np + 1] into the cells of one energy */
	int regime = 0;
	size_t per_kind = 0;              /* ns * tc */
};

static int pc_joint_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const pc_hip_joint_spec *spec, pc_hip_joint **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_create: joint must not be NULL");
	*out = nullptr;
	const pc_hip_ctx *c0 = ctxs[0];
	int st = pc_hip_joint_validate(spec, (size_t)c0->host.pm.n_energies);
	if (st) return st;
	pc_hip_joint *h = new pc_hip_joint();
	const std::vector<int> sel = pc_sel_fill(spec->n_energies, spec->energies, (size_t)c0->host.pm.n_energies);
	pc_joint_geo &g = h->geo;
	memset(&g, 0, sizeof(g));
	g.np = spec->n_pairs;
	g.ns = (int)sel.size();
	const double zexit = c0->host.z[c0->host.pm.nmax];
	int cells = 0;
	for (int p = 0; p < g.np; p++) {
		for (int w = 0; w < 2; w++) {
			const pc_hip_hist_axis &x = w ? spec->pairs[p].v : spec->pairs[p].u;
			pc_hist_axis_k &a = g.ax[2*p + w];
			a.zp = zexit + x.d;          /* once, on the host */
			a.cx = x.cx; a.cy = x.cy; a.lo = x.lo; a.hi = x.hi;
			a.quantity = x.quantity; a.n_bins = x.n_bins;
			if (x.quantity == PC_HIST_N_REFL) g.need_n = 1;
			if (x.quantity == PC_HIST_D_TRAVEL) g.need_travel = 1;
			if (x.quantity == PC_HIST_R_START || x.quantity == PC_JOINT_START_X || x.quantity == PC_JOINT_START_Y) g.need_start = 1;
		}
		g.nc[p] = spec->pairs[p].u.n_bins*spec->pairs[p].v.n_bins;
		g.cell0[p] = cells + p;
		h->offsets.push_back(cells);
		cells += g.nc[p];
	}
	h->offsets.push_back(cells);
	g.tc = cells + g.np;
	h->per_kind = (size_t)g.ns*g.tc;
	h->regime = spec->regime ? spec->regime : pc_joint_auto_regime(g.ns, g.tc);
	st = pc_tally_make(*h, ctxs, group, 3*h->per_kind, "pc_hip_joint_create");
	if (!st) st = pc_tally_upload(*h, sel, std::vector<double>(), "pc_hip_joint_create");
	if (st) { delete h; return st; }
	*out = h;
	return PC_HIP_OK;
}

static int pc_joint_launch(pc_hip_joint *h, pc_tally_member &m, const pc_spot_src &s, int kind)
{
	pc_hip_ctx *c = m.ctx;
	pc_joint_geo g = h->geo;
	g.sel = m.d_sel;
	unsigned long long *cells = m.d_cells + (size_t)kind*h->per_kind;
	unsigned long long *sq = h->squares ? m.d_sq + 2*(size_t)kind*h->per_kind : nullptr;
	if (h->regime == 1) {
		const long long tiles = pc_tally_tile_split((long long)h->per_kind, PC_JOINT_TILE, h->squares).tiles;
		const long long bx = pc_tally_grid_tiles(c->n_cu, tiles, s.n, PC_JOINT_LDS_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_joint_lds_kernel<true, true> : pc_joint_lds_kernel<false, true>)
		               : (s.mask ? pc_joint_lds_kernel<true, false> : pc_joint_lds_kernel<false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)tiles), dim3(PC_JOINT_LDS_BLOCK), 0, c->stream, s, g, cells, sq);
	} else {
		const int ec = sq ? PC_JOINT_ECHUNK_SQ : PC_JOINT_ECHUNK;
		const long long chunks = (g.ns + ec - 1)/ec;
		const long long bx = pc_tally_grid_wide(c->n_cu, chunks, g.ns, s.n, PC_JOINT_WIDE_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_joint_wide_kernel<true, true> : pc_joint_wide_kernel<false, true>)
		               : (s.mask ? pc_joint_wide_kernel<true, false> : pc_joint_wide_kernel<false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)chunks), dim3(PC_JOINT_WIDE_BLOCK), 0, c->stream, s, g, cells, sq);
	}
	return PC_HIP_OK;
}

/* the members' summed cells (limbs = 1) or square pairs (limbs = 2) from the device layout of the regime into cells
 * [3][ns][total_cells][limbs] and outside [3][np][ns][limbs]; either may be NULL */
static void pc_joint_unpack(const pc_hip_joint *joint, const std::vector<unsigned long long> &sum, size_t limbs, uint64_t *cells, uint64_t *outside)
{
	const pc_joint_geo &g = joint->geo;
	const size_t ns = (size_t)g.ns, tc = (size_t)g.tc, total = tc - (size_t)g.np;
	for (size_t kind = 0; kind < 3; kind++)
		for (size_t s = 0; s < ns; s++)
			for (int p = 0; p < g.np; p++) {
				const size_t c0 = (size_t)g.cell0[p], nc = (size_t)g.nc[p];
				for (size_t b = 0; b <= nc; b++) {
					const unsigned long long *v = &sum[limbs*(kind*joint->per_kind + (joint->regime == 1 ? s*tc + c0 + b : (c0 + b)*ns + s))];
					uint64_t *to = nullptr;
					if (b < nc) { if (cells) to = cells + limbs*((kind*ns + s)*total + (size_t)joint->offsets[p] + b); }
					else if (outside) to = outside + limbs*((kind*(size_t)g.np + (size_t)p)*ns + s);
					for (size_t l = 0; to && l < limbs; l++) to[l] = v[l];
				}
			}
}

extern "C" {

int pc_hip_joint_validate(const pc_hip_joint_spec *spec, size_t n_energies)
{
	std::string why;
	return pc_joint_spec_check(spec, n_energies, &why) ? PC_HIP_OK : pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_validate: " + why);
}

int pc_hip_joint_create(pc_hip_ctx *ctx, const pc_hip_joint_spec *spec, pc_hip_joint **joint)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_create: ctx must not be NULL");
	return pc_joint_make(std::vector<pc_hip_ctx *>{ctx}, nullptr, spec, joint);
}

int pc_hip_group_joint_create(pc_hip_group *group, const pc_hip_joint_spec *spec, pc_hip_joint **joint)
{
	if (!group) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_joint_create: group must not be NULL");
	return pc_joint_make(group->ctx, group, spec, joint);
}

void pc_hip_joint_destroy(pc_hip_joint *joint)
{
	delete joint;
}

int pc_hip_joint_add(pc_hip_joint *joint, int kind)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_add: joint must not be NULL");
	return pc_tally_add(*joint, kind, "pc_hip_joint_add",
		[joint](size_t k, const pc_spot_src &s, int kd) { return pc_joint_launch(joint, joint->m[k], s, kd); });
}

int pc_hip_joint_read(pc_hip_joint *joint, uint64_t *cells, uint64_t *outside, int64_t *n_entries)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_read: joint must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum(*joint, 1, sum);
	if (st) return st;
	pc_joint_unpack(joint, sum, 1, cells, outside);
	if (n_entries)
		for (int k = 0; k < 3; k++) n_entries[k] = joint->n_entries[k];
	return PC_HIP_OK;
}

int pc_hip_joint_track_squares(pc_hip_joint *joint)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_track_squares: joint must not be NULL");
	return pc_tally_track_squares(*joint, "pc_hip_joint_track_squares");
}

int pc_hip_joint_read_squares(pc_hip_joint *joint, uint64_t *cells_sq, uint64_t *outside_sq)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_read_squares: joint must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum_squares(*joint, "pc_hip_joint_read_squares", sum);
	if (st) return st;
	pc_joint_unpack(joint, sum, 2, cells_sq, outside_sq);
	return PC_HIP_OK;
}

int pc_hip_joint_reset(pc_hip_joint *joint)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_reset: joint must not be NULL");
	return pc_tally_reset(*joint);
}

int pc_hip_joint_info(const pc_hip_joint *joint, int32_t dims[3], int32_t *offsets, int *regime)
{
	if (!joint || !dims) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_info: NULL argument");
	dims[0] = joint->geo.np; dims[1] = joint->geo.ns; dims[2] = joint->offsets.back();
	if (offsets)
		for (size_t k = 0; k < joint->offsets.size(); k++) offsets[k] = joint->offsets[k];
	if (regime) *regime = joint->regime;
	return PC_HIP_OK;
}

int pc_hip_joint_marginal(int32_t nu, int32_t nv, const uint64_t *cells, int which, uint64_t *out)
{
	if (nu < 1 || nv < 1 || !cells || !out || which < 0 || which > 1)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_marginal: nu and nv must be >= 1, which 0 (u) or 1 (v), cells and out not NULL");
	pc_joint_marginal(nu, nv, cells, which, out);
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_JOINT_HOST_ONLY */
#endif /* PC_JOINT_H */

/*
 * pc_spot.h -- spot maps: weighted 2-D histograms of where the photons of the last run cross planes perpendicular to the optic
 * axis downstream of its exit face (include/polycap-hip.h, pc_hip_spot_*).  A post-pass over data the run left in HBM: the exit
 * photons (image records or planes) and the ordered leak event lists.  Nothing is uploaded from the host and no trace kernel is
 * involved.  Sums are exact integer sums (uint64, weights quantised to 2^-32), so a map depends on the set of entries only:
 * not on launch shape, entry order, how the slots were split into runs, or the device count.
 *
 * The first part (the per-entry arithmetic and the check of a spec) compiles for the host as well: -DPC_SPOT_HOST_ONLY stops the
 * header after it.
 */
#ifndef PC_SPOT_H
#define PC_SPOT_H

#include <math.h>
#include <stdint.h>
#include <cmath>
#include <string>

#if defined(PC_SPOT_HOST_ONLY) && !defined(PC_TALLY_HOST_ONLY)
#define PC_TALLY_HOST_ONLY      /* the host part stands on pc_tally.h's (pc_sel_check) */
#endif
#include "pc_tally.h"

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

/* Bin of one entry on the plane z = zp, in [0, nx*ny) as iy*nx + ix, or -1 when it is outside (NaN anywhere, dz <= 0, off the
 * window).  The contract of include/polycap-hip.h, operation by operation (the library is built with -ffp-contract=off). */
static inline __host__ __device__ long long pc_spot_bin(double x, double y, double z, double dx, double dy, double dz, double zp,
	double x0, double x1, double y0, double y1, int nx, int ny)
{
	const double t = (zp - z) / dz;
	const double xd = x + dx*t, yd = y + dy*t;
	const double fx = ((xd - x0) / (x1 - x0)) * (double)nx;
	const double fy = ((yd - y0) / (y1 - y0)) * (double)ny;
	if (!(dz > 0.) || !(fx >= 0. && fx < (double)nx && fy >= 0. && fy < (double)ny))
		return -1;
	return (long long)floor(fy) * nx + (long long)floor(fx);
}

/* exit photons carry the x and y components of their direction only */
static inline __host__ __device__ double pc_spot_exit_dz(double dx, double dy)
{
	return sqrt((1. - dx*dx) - dy*dy);
}

/* q(w) = round_half_even(w * 2^32); weights are in [0, 1], anything not above zero (NaN included) counts 0 */
static inline __host__ __device__ unsigned long long pc_spot_q(double w)
{
	const double v = w * 4294967296.0;
	return (v > 0.) ? (unsigned long long)rint(v) : 0ull;
}

/* pc_hip_spot_validate (Spec: pc_hip_spot_spec of include/polycap-hip.h): false and the message in *why when the spec is refused */
template <typename Spec>
static bool pc_spot_spec_check(const Spec *spec, size_t n_energies, std::string *why)
{
	const auto no = [why](const std::string &w) { *why = w; return false; };
	if (!spec) return no("spot spec must not be NULL");
	if (spec->n_planes < 1 || spec->n_planes > 64 || !spec->distances)
		return no("spot spec: 1 to 64 plane distances are needed, got " + std::to_string(spec->n_planes));
	for (int k = 0; k < spec->n_planes; k++)
		if (!(spec->distances[k] >= 0.) || !std::isfinite(spec->distances[k]))
			return no("spot spec: plane distances must be finite and >= 0");
	if (!std::isfinite(spec->x0) || !std::isfinite(spec->x1) || !std::isfinite(spec->y0) || !std::isfinite(spec->y1)
	    || !(spec->x0 < spec->x1) || !(spec->y0 < spec->y1))
		return no("spot spec: the window needs finite x0 < x1 and y0 < y1");
	if (spec->nx < 1 || spec->ny < 1)
		return no("spot spec: nx and ny must be >= 1");
	if (spec->regime < 0 || spec->regime > 2)
		return no("spot spec: regime must be 0 (automatic), 1 (LDS tiles) or 2 (energies across lanes)");
	std::string sel;
	if (!pc_sel_check(spec->n_energies, spec->energies, n_energies, &sel))
		return no("spot spec: " + sel);
	const double ns = spec->n_energies ? (double)spec->n_energies : (double)n_energies;
	if ((double)spec->n_planes*ns*(double)spec->nx*(double)spec->ny > (double)(1ll << 27))
		return no("spot spec: n_planes * n_energies * nx * ny exceeds 2^27 bins");
	return true;
}

#ifndef PC_SPOT_HOST_ONLY

struct pc_spot_geo {
	const double *zp;       /* [np] plane positions */
	const int *sel;         /* [ns] energy indices */
	double x0, x1, y0, y1;
	int nx, ny, np, ns;
};

static __device__ __forceinline__ long long pc_spot_entry_bin(const pc_spot_src &s, const pc_spot_geo &g, long long i, int p)
{
	const pc_entry e = pc_entry_load(s, i);
	return pc_spot_bin(e.x, e.y, e.z, e.dx, e.dy, e.dz, g.zp[p], g.x0, g.x1, g.y0, g.y1, g.nx, g.ny);
}

/* Small maps.  The flat map [plane][energy][iy][ix] followed by the outside counters [plane][energy] is cut into tiles of
 * PC_SPOT_TILE uint64 bins; workgroup (x, y) adds the entries x, x + gridDim.x, ... that fall into tile y to a private copy of it
 * in LDS (ds_add_u64), then adds each non-zero bin of that copy to the map with one global atomic.  Maps of several tiles are
 * several passes over the entries (blockIdx.y).  Where the squares are tracked (Q) a tile is TC = PC_SPOT_TILE / 3 bins
 * (pc_tally_tile_cells): their weight sums in tile[0, TC), their square sums as (lo, hi) pairs behind them, flushed with
 * pc_atomic_add128 to sq [bin][2]. */
#define PC_SPOT_TILE 8192
#define PC_SPOT_LDS_BLOCK 512
/* M: a gated add, s.mask is set (pc_select.h); the plain build reads no mask.  Q: the squares are tracked; the build without reads no sq */
template <bool M, bool Q>
__global__ void __launch_bounds__(PC_SPOT_LDS_BLOCK) pc_spot_lds_kernel(pc_spot_src s, pc_spot_geo g, unsigned long long *map, unsigned long long *sq)
{
	__shared__ unsigned long long tile[PC_SPOT_TILE];
	constexpr long long TC = pc_tally_tile_cells(PC_SPOT_TILE, Q);
	const long long nb = (long long)g.nx*g.ny, n_bins = (long long)g.np*g.ns*nb, total = n_bins + (long long)g.np*g.ns;
	const long long t0 = (long long)blockIdx.y*TC;
	const long long t1 = (t0 + TC < total) ? t0 + TC : total;
	for (int k = threadIdx.x; k < PC_SPOT_TILE; k += blockDim.x) tile[k] = 0ull;
	__syncthreads();
	for (long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x; i < s.n; i += (long long)gridDim.x*blockDim.x) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		for (int p = 0; p < g.np; p++) {
			const long long b = pc_spot_entry_bin(s, g, i, p);
			/* the entry's cells for energies 0 .. ns-1: base + k*step */
			const long long base = (b >= 0) ? (long long)p*g.ns*nb + b : n_bins + (long long)p*g.ns;
			const long long step = (b >= 0) ? nb : 1;
			if (base >= t1) continue;
			const long long k_lo = (base >= t0) ? 0 : (t0 - base + step - 1)/step;
			long long k_hi = (t1 - 1 - base)/step + 1;
			if (k_hi > g.ns) k_hi = g.ns;
			for (long long k = k_lo; k < k_hi; k++) {
				const unsigned long long q = pc_spot_q(s.w[i*s.ws + g.sel[k]]);
				if (q) {
					atomicAdd(&tile[base + k*step - t0], q);
					if (Q) pc_tally_lds_add_sq(&tile[TC + 2*(base + k*step - t0)], q);
				}
			}
		}
	}
	__syncthreads();
	for (long long k = threadIdx.x; k < t1 - t0; k += blockDim.x) {
		const unsigned long long v = tile[k];
		if (v) {
			atomicAdd(&map[t0 + k], v);
			if (Q) pc_atomic_add128(sq + 2*(t0 + k), tile[TC + 2*k], tile[TC + 2*k + 1]);      /* a bin without weight has no square */
		}
	}
}

/* Many selected energies.  The bins are laid out [plane][iy][ix][energy] with the energies innermost: the lanes of a wave take
 * the energies of one entry (64 / gw entries per wave when fewer than 64 are selected, gw = the next power of two), so that one
 * wave instruction is a contiguous run of 8-byte global atomics.  Workgroup (x, p, c) does plane p for energies
 * [c*PC_SPOT_ECHUNK, ...); the outside counters of those energies are summed in LDS first (every entry that misses the window
 * adds to the same few counters).  Where the squares are tracked (Q) every add to a bin is followed by pc_tally_add_sq on its pair
 * in sq [bin][2], and the Q instance takes chunks of PC_SPOT_ECHUNK_SQ = 1024 energies: their outside counters and, behind them, the
 * counters' pairs are 24 KiB of LDS. */
#define PC_SPOT_ECHUNK 4096
#define PC_SPOT_ECHUNK_SQ 1024
#define PC_SPOT_WIDE_BLOCK 256
template <bool M, bool Q>
__global__ void __launch_bounds__(PC_SPOT_WIDE_BLOCK) pc_spot_wide_kernel(pc_spot_src s, pc_spot_geo g, unsigned long long *map, unsigned long long *sq)
{
	constexpr int EC = Q ? PC_SPOT_ECHUNK_SQ : PC_SPOT_ECHUNK;
	__shared__ unsigned long long out[EC*(Q ? 3 : 1)];
	unsigned long long *out_sq = out + EC;      /* [k][2], Q only */
	const int p = blockIdx.y, s0 = blockIdx.z*EC;
	const int sn = (g.ns - s0 < EC) ? g.ns - s0 : EC;
	const long long nb = (long long)g.nx*g.ny, n_bins = (long long)g.np*g.ns*nb;
	for (int k = threadIdx.x; k < sn; k += blockDim.x) out[k] = 0ull;
	if (Q)
		for (int k = threadIdx.x; k < 2*sn; k += blockDim.x) out_sq[k] = 0ull;
	__syncthreads();
	const pc_tally_lanes l = pc_tally_lane_map(sn);
	for (long long i = l.first; i < s.n; i += l.stride) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		const long long b = pc_spot_entry_bin(s, g, i, p);
		unsigned long long *cell = map + ((long long)p*nb + (b >= 0 ? b : 0))*g.ns + s0;
		for (int k = l.sub; k < sn; k += l.gw) {
			const unsigned long long q = pc_spot_q(s.w[i*s.ws + g.sel[s0 + k]]);
			if (!q) continue;
			if (b >= 0) {
				atomicAdd(cell + k, q);
				if (Q) pc_tally_add_sq(sq + 2*((cell - map) + k), q);
			} else {
				atomicAdd(&out[k], q);
				if (Q) pc_tally_lds_add_sq(&out_sq[2*k], q);
			}
		}
	}
	__syncthreads();
	for (int k = threadIdx.x; k < sn; k += blockDim.x) {
		const unsigned long long v = out[k];
		if (v) {
			atomicAdd(&map[n_bins + (long long)p*g.ns + s0 + k], v);
			if (Q) pc_atomic_add128(sq + 2*(n_bins + (long long)p*g.ns + s0 + k), out_sq[2*k], out_sq[2*k + 1]);
		}
	}
}

/* Regime of a map (spec->regime 0): energies across lanes.  Measured on an MI355X (scripts/bench_spot.py; xos1, 1e7 exit photons,
 * one plane, window +-0.02 cm): at 10 keV 128^2 LDS tiles 0.86 ms per add against 0.38 ms, 1024^2 37.1 ms (128 passes) against
 * 0.37 ms; at 291 energies x 64^2 with 3 / 9 / 291 energies selected 1.03 / 4.16 / 1117 ms against 0.83 / 2.51 / 15.5 ms.  The
 * LDS tiles won no measured case, so there is no crossover to apply: they stay available as regime 1 (maps of a single tile with
 * a very concentrated spot are where they could still win; not measured). */

/* one map for all kinds (pc_tally: shared): elems = np*ns*nx*ny bins + np*ns outside counters */
struct pc_hip_spot : pc_tally {
	int np = 0, ns = 0, nx = 0, ny = 0, wide = 0;
	double x0 = 0., x1 = 0., y0 = 0., y1 = 0.;
};

static int pc_spot_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const pc_hip_spot_spec *spec, pc_hip_spot **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_create: spot must not be NULL");
	*out = nullptr;
	const pc_hip_ctx *c0 = ctxs[0];
	int st = pc_hip_spot_validate(spec, (size_t)c0->host.pm.n_energies);
	if (st) return st;
	pc_hip_spot *sp = new pc_hip_spot();
	sp->shared = 1;
	sp->np = spec->n_planes; sp->nx = spec->nx; sp->ny = spec->ny;
	sp->x0 = spec->x0; sp->x1 = spec->x1; sp->y0 = spec->y0; sp->y1 = spec->y1;
	const std::vector<int> sel = pc_sel_fill(spec->n_energies, spec->energies, (size_t)c0->host.pm.n_energies);
	sp->ns = (int)sel.size();
	sp->wide = spec->regime != 1;
	/* zp = z[nmax] + d, once, on the host */
	std::vector<double> zp(sp->np);
	const double zexit = c0->host.z[c0->host.pm.nmax];
	for (int k = 0; k < sp->np; k++) zp[k] = zexit + spec->distances[k];
	const long long cells = (long long)sp->np*sp->ns*((long long)sp->nx*sp->ny + 1);
	st = pc_tally_make(*sp, ctxs, group, (size_t)cells, "pc_hip_spot_create");
	if (!st) st = pc_tally_upload(*sp, sel, zp, "pc_hip_spot_create");
	if (st) { delete sp; return st; }
	*out = sp;
	return PC_HIP_OK;
}

static int pc_spot_launch(pc_hip_spot *sp, pc_tally_member &m, const pc_spot_src &s)
{
	pc_hip_ctx *c = m.ctx;
	pc_spot_geo g;
	g.zp = m.d_zp; g.sel = m.d_sel;
	g.x0 = sp->x0; g.x1 = sp->x1; g.y0 = sp->y0; g.y1 = sp->y1;
	g.nx = sp->nx; g.ny = sp->ny; g.np = sp->np; g.ns = sp->ns;
	unsigned long long *sq = sp->squares ? m.d_sq.p : nullptr;
	if (!sp->wide) {
		const long long tiles = pc_tally_tile_split((long long)sp->elems, PC_SPOT_TILE, sp->squares).tiles;
		const long long bx = pc_tally_grid_tiles(c->n_cu, tiles, s.n, PC_SPOT_LDS_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_spot_lds_kernel<true, true> : pc_spot_lds_kernel<false, true>)
		               : (s.mask ? pc_spot_lds_kernel<true, false> : pc_spot_lds_kernel<false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)tiles), dim3(PC_SPOT_LDS_BLOCK), 0, c->stream, s, g, m.d_cells.p, sq);
	} else {
		const int ec = sq ? PC_SPOT_ECHUNK_SQ : PC_SPOT_ECHUNK;
		const long long chunks = (sp->ns + ec - 1)/ec;
		const long long bx = pc_tally_grid_wide(c->n_cu, sp->np*chunks, sp->ns, s.n, PC_SPOT_WIDE_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_spot_wide_kernel<true, true> : pc_spot_wide_kernel<false, true>)
		               : (s.mask ? pc_spot_wide_kernel<true, false> : pc_spot_wide_kernel<false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)sp->np, (unsigned)chunks), dim3(PC_SPOT_WIDE_BLOCK), 0, c->stream, s, g, m.d_cells.p, sq);
	}
	return PC_HIP_OK;
}

/* the members' summed bins (limbs = 1) or square pairs (limbs = 2) from the device layout into bins [np][ns][ny][nx][limbs] and
 * outside [np][ns][limbs]; either may be NULL */
static void pc_spot_unpack(const pc_hip_spot *spot, const std::vector<unsigned long long> &sum, size_t limbs, uint64_t *bins, uint64_t *outside)
{
	const size_t nb = (size_t)spot->nx*spot->ny, n_bins = (size_t)spot->np*spot->ns*nb, n_out = (size_t)spot->np*spot->ns;
	if (bins) {
		if (!spot->wide)
			memcpy(bins, sum.data(), limbs*n_bins*sizeof(uint64_t));
		else      /* [plane][iy][ix][energy] -> [plane][energy][iy][ix] */
			for (int p = 0; p < spot->np; p++)
				for (size_t b = 0; b < nb; b++)
					for (int s = 0; s < spot->ns; s++)
						for (size_t l = 0; l < limbs; l++)
							bins[limbs*(((size_t)p*spot->ns + s)*nb + b) + l] = sum[limbs*(((size_t)p*nb + b)*spot->ns + s) + l];
	}
	if (outside) memcpy(outside, sum.data() + limbs*n_bins, limbs*n_out*sizeof(uint64_t));
}

extern "C" {

int pc_hip_spot_validate(const pc_hip_spot_spec *spec, size_t n_energies)
{
	std::string why;
	return pc_spot_spec_check(spec, n_energies, &why) ? PC_HIP_OK : pc_fail(PC_HIP_ERR_INVALID, why);
}

int pc_hip_spot_create(pc_hip_ctx *ctx, const pc_hip_spot_spec *spec, pc_hip_spot **spot)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_create: ctx must not be NULL");
	return pc_spot_make(std::vector<pc_hip_ctx *>{ctx}, nullptr, spec, spot);
}

int pc_hip_group_spot_create(pc_hip_group *group, const pc_hip_spot_spec *spec, pc_hip_spot **spot)
{
	if (!group) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_spot_create: group must not be NULL");
	return pc_spot_make(group->ctx, group, spec, spot);
}

void pc_hip_spot_destroy(pc_hip_spot *spot)
{
	delete spot;
}

int pc_hip_spot_add(pc_hip_spot *spot, int kind)
{
	if (!spot) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_add: spot must not be NULL");
	return pc_tally_add(*spot, kind, "pc_hip_spot_add",
		[spot](size_t k, const pc_spot_src &s, int) { return pc_spot_launch(spot, spot->m[k], s); });
}

int pc_hip_spot_read(pc_hip_spot *spot, uint64_t *bins, uint64_t *outside, int64_t *n_entries)
{
	if (!spot) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_read: spot must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum(*spot, 1, sum);
	if (st) return st;
	pc_spot_unpack(spot, sum, 1, bins, outside);
	if (n_entries) *n_entries = spot->n_entries[0] + spot->n_entries[1] + spot->n_entries[2];
	return PC_HIP_OK;
}

int pc_hip_spot_track_squares(pc_hip_spot *spot)
{
	if (!spot) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_track_squares: spot must not be NULL");
	return pc_tally_track_squares(*spot, "pc_hip_spot_track_squares");
}

int pc_hip_spot_read_squares(pc_hip_spot *spot, uint64_t *bins_sq, uint64_t *outside_sq)
{
	if (!spot) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_read_squares: spot must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum_squares(*spot, "pc_hip_spot_read_squares", sum);
	if (st) return st;
	pc_spot_unpack(spot, sum, 2, bins_sq, outside_sq);
	return PC_HIP_OK;
}

int pc_hip_spot_reset(pc_hip_spot *spot)
{
	if (!spot) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_reset: spot must not be NULL");
	return pc_tally_reset(*spot);
}

int pc_hip_spot_info(const pc_hip_spot *spot, int32_t dims[4], int *wide)
{
	if (!spot || !dims) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_info: NULL argument");
	dims[0] = spot->np; dims[1] = spot->ns; dims[2] = spot->ny; dims[3] = spot->nx;
	if (wide) *wide = spot->wide;
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_SPOT_HOST_ONLY */
#endif /* PC_SPOT_H */

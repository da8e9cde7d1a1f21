/*
 * pc_hist.h -- histograms: weighted 1-D histograms of per-entry scalar quantities of the last run (position and radius on a plane
 * behind the exit face, slopes, reflection count, path length, entrance radius, z), one histogram per axis and selected energy
 * (include/polycap-hip.h, pc_hip_hist_*).  One post-pass over the entries a spot map reads (pc_spot_source: exit photons as image
 * records or planes, the ordered leak event lists) computes every axis' bin of an entry; nothing is uploaded and no trace kernel is
 * involved.  Sums are exact integer sums (uint64, weights quantised to 2^-32), kept per kind, so they depend on the set of entries
 * only: not on launch shape, entry order, how the slots were split into runs, or the device count.  Full width at half maximum
 * and quantiles (encircled-energy radii) follow on the host (pc_hip_hist_fwhm, pc_hip_hist_quantile).
 *
 * The first part (the per-entry arithmetic, the host formulas and the check of a spec) compiles for the host as well: -DPC_HIST_HOST_ONLY stops the
 * header after it.
 */
#ifndef PC_HIST_H
#define PC_HIST_H

#include <math.h>
#include <stdint.h>
#include <cmath>
#include <string>

#if defined(PC_HIST_HOST_ONLY) && !defined(PC_TALLY_HOST_ONLY)
#define PC_TALLY_HOST_ONLY      /* the host part stands on pc_tally.h's (pc_sel_check) */
#endif
#include "pc_tally.h"

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define PC_HIST_MAX_AXES 16
enum { PC_HIST_X_AT = 0, PC_HIST_Y_AT, PC_HIST_R_AT, PC_HIST_SLOPE_X, PC_HIST_SLOPE_Y, PC_HIST_TAN_THETA, PC_HIST_N_REFL,
       PC_HIST_D_TRAVEL, PC_HIST_R_START, PC_HIST_Z, PC_HIST_N_QUANTITIES,
       /* joint histograms only (pc_joint.h): the start coordinates themselves; pc_hip_hist_validate refuses them */
       PC_JOINT_START_X = PC_HIST_N_QUANTITIES, PC_JOINT_START_Y, PC_JOINT_N_QUANTITIES };

/* one entry: position, direction, reflection count (as a double), and for exit photons the path length and the start
 * coordinates in the optic's entrance plane; leak = 1 for leak events, which have neither of the last two */
struct pc_hist_entry {
	double x, y, z, dx, dy, dz, n, dtravel, sx, sy;
	int leak;
};

/* one axis as the kernels take it: zp = z[nmax] + d, made once on the host */
struct pc_hist_axis_k {
	double zp, cx, cy, lo, hi;
	int quantity, n_bins;
};

/* Value of `quantity` for an entry, and *ok = 0 when the entry is outside whatever its value: a quantity that needs dz with
 * !(dz > 0), or an exit-photon quantity on a leak event.  The contract of include/polycap-hip.h, operation by operation (the
 * library is built with -ffp-contract=off). */
static inline __host__ __device__ double pc_hist_value(const pc_hist_axis_k &a, const pc_hist_entry &e, int *ok)
{
	*ok = 1;
	switch (a.quantity) {
	case PC_HIST_X_AT: case PC_HIST_Y_AT: case PC_HIST_R_AT: {
		*ok = e.dz > 0.;
		const double t = (a.zp - e.z) / e.dz;
		if (a.quantity == PC_HIST_X_AT) return e.x + e.dx*t;
		if (a.quantity == PC_HIST_Y_AT) return e.y + e.dy*t;
		const double p = (e.x + e.dx*t) - a.cx, q = (e.y + e.dy*t) - a.cy;
		return sqrt(p*p + q*q);
	}
	case PC_HIST_SLOPE_X: *ok = e.dz > 0.; return e.dx / e.dz;
	case PC_HIST_SLOPE_Y: *ok = e.dz > 0.; return e.dy / e.dz;
	case PC_HIST_TAN_THETA: *ok = e.dz > 0.; return sqrt(e.dx*e.dx + e.dy*e.dy) / e.dz;
	case PC_HIST_N_REFL: return e.n;
	case PC_HIST_D_TRAVEL: *ok = !e.leak; return e.dtravel;
	case PC_HIST_R_START: *ok = !e.leak; return sqrt(e.sx*e.sx + e.sy*e.sy);
	case PC_HIST_Z: return e.z;
	case PC_JOINT_START_X: *ok = !e.leak; return e.sx;
	case PC_JOINT_START_Y: *ok = !e.leak; return e.sy;
	}
	*ok = 0;
	return 0.;
}

/* bin of a value in [0, n_bins), or -1 when it is off the range (NaN included) */
static inline __host__ __device__ int pc_hist_bin(double v, double lo, double hi, int n_bins)
{
	const double f = ((v - lo) / (hi - lo)) * (double)n_bins;
	if (!(f >= 0. && f < (double)n_bins)) return -1;
	return (int)floor(f);
}

static inline __host__ __device__ int pc_hist_axis_bin(const pc_hist_axis_k &a, const pc_hist_entry &e)
{
	int ok;
	const double v = pc_hist_value(a, e, &ok);
	return ok ? pc_hist_bin(v, a.lo, a.hi, a.n_bins) : -1;
}

/* centre of bin b */
static inline double pc_hist_centre(int n_bins, double lo, double hi, int64_t b)
{
	return lo + (((double)b + 0.5) / (double)n_bins) * (hi - lo);
}

/* pc_hip_hist_quantile: the formula of include/polycap-hip.h in its order */
static inline double pc_hist_quantile(int32_t n_bins, double lo, double hi, const uint64_t *bins, double q)
{
	uint64_t total = 0;
	for (int32_t b = 0; b < n_bins; b++) total += bins[b];
	if (total == 0 || !(q >= 0. && q <= 1.)) return NAN;
	const double target = q * (double)total;
	uint64_t before = 0;
	for (int32_t b = 0; b < n_bins; b++) {
		const uint64_t upto = before + bins[b];
		if (bins[b] != 0 && (double)upto >= target) {
			const double frac = (target - (double)before) / (double)bins[b];
			return lo + (((double)b + frac) / (double)n_bins) * (hi - lo);
		}
		before = upto;
	}
	return hi;
}

/* pc_hip_hist_fwhm: the formula of include/polycap-hip.h in its order */
static inline double pc_hist_fwhm(int32_t n_bins, double lo, double hi, const uint64_t *bins, double *left, double *right)
{
	if (left) *left = NAN;
	if (right) *right = NAN;
	if (n_bins < 1) return NAN;
	int32_t peak = 0;
	for (int32_t b = 1; b < n_bins; b++)
		if (bins[b] > bins[peak]) peak = b;
	if (bins[peak] == 0) return NAN;
	const double half = (double)bins[peak] / 2.0;
	int32_t i = peak - 1, j = peak + 1;
	while (i >= 0 && !((double)bins[i] < half)) i--;
	while (j < n_bins && !((double)bins[j] < half)) j++;
	if (i < 0 || j >= n_bins) return NAN;
	const double ci = pc_hist_centre(n_bins, lo, hi, i), ci1 = pc_hist_centre(n_bins, lo, hi, i + 1);
	const double cj = pc_hist_centre(n_bins, lo, hi, j), cj1 = pc_hist_centre(n_bins, lo, hi, j - 1);
	const double l = ci + (ci1 - ci) * ((half - (double)bins[i]) / ((double)bins[i + 1] - (double)bins[i]));
	const double r = cj + (cj1 - cj) * ((half - (double)bins[j]) / ((double)bins[j - 1] - (double)bins[j]));
	if (left) *left = l;
	if (right) *right = r;
	return r - l;
}

/* One axis of a spec (Axis: pc_hip_hist_axis of include/polycap-hip.h): false and the reason in *why (it names the field) when it is
 * refused.  n_quantities = PC_HIST_N_QUANTITIES for a histogram, PC_JOINT_N_QUANTITIES for a joint histogram or a cut (pc_select.h). */
template <typename Axis>
static bool pc_hist_axis_check(const Axis &x, int n_quantities, std::string *why)
{
	static const char *names[PC_JOINT_N_QUANTITIES] = { "X_AT", "Y_AT", "R_AT", "SLOPE_X", "SLOPE_Y", "TAN_THETA", "N_REFL", "D_TRAVEL", "R_START", "Z",
	                                                    "START_X", "START_Y" };
	*why = "";
	if (x.quantity < 0 || x.quantity >= n_quantities)
		*why = std::string("quantity must be one of PC_HIP_HIST_X_AT .. ") + (n_quantities == PC_HIST_N_QUANTITIES ? "PC_HIP_HIST_Z" : "PC_HIP_JOINT_START_Y")
		     + ", got " + std::to_string(x.quantity);
	else if (!std::isfinite(x.d) || !(x.d >= 0.) || (x.quantity > PC_HIST_R_AT && x.d != 0.))
		*why = std::string("d must be finite and >= 0, and 0 for ") + names[x.quantity] + " (X_AT, Y_AT and R_AT use it)";
	else if (!std::isfinite(x.cx) || !std::isfinite(x.cy) || (x.quantity != PC_HIST_R_AT && (x.cx != 0. || x.cy != 0.)))
		*why = std::string("cx and cy must be finite, and 0 for ") + names[x.quantity] + " (R_AT uses them)";
	else if (!std::isfinite(x.lo) || !std::isfinite(x.hi) || !(x.lo < x.hi))
		*why = "lo and hi must be finite with lo < hi";
	else if (x.n_bins < 1)
		*why = "n_bins must be >= 1";
	return why->empty();
}

/* pc_hip_hist_validate (Spec: pc_hip_hist_spec): false and the reason in *why (it names the field) when the spec is refused */
template <typename Spec>
static bool pc_hist_spec_check(const Spec *spec, size_t n_energies, std::string *why)
{
	const auto no = [why](const std::string &w) { *why = w; return false; };
	if (!spec) return no("spec must not be NULL");
	if (spec->n_axes < 1 || spec->n_axes > PC_HIST_MAX_AXES || !spec->axes)
		return no("n_axes: 1 to 16 axes are needed, got " + std::to_string(spec->n_axes));
	double bins = 0.;
	for (int a = 0; a < spec->n_axes; a++) {
		std::string w;
		if (!pc_hist_axis_check(spec->axes[a], PC_HIST_N_QUANTITIES, &w))
			return no("axis " + std::to_string(a) + ": " + w);
		bins += (double)spec->axes[a].n_bins;
	}
	if (spec->regime < 0 || spec->regime > 2)
		return no("regime must be 0 (automatic), 1 (private LDS histograms) or 2 (energies across lanes)");
	if (!pc_sel_check(spec->n_energies, spec->energies, n_energies, why))
		return false;
	const double ns = spec->n_energies ? (double)spec->n_energies : (double)n_energies;
	if (bins*ns > (double)(1ll << 24))
		return no("n_bins: (sum of n_bins) * selected energies exceeds 2^24");
	return true;
}

#ifndef PC_HIST_HOST_ONLY

/* Cells.  Every axis has n_bins + 1 cells per selected energy: its bins, then its outside counter; the cells of the axes follow
 * each other, tc = total_bins + n_axes per energy.  cell0[a] = where axis a starts. */
struct pc_hist_geo {
	pc_hist_axis_k ax[PC_HIST_MAX_AXES];
	int cell0[PC_HIST_MAX_AXES];
	const int *sel;          /* [ns] energy indices */
	int na, ns, tc;
	int need_start, need_travel, need_n;      /* which of the optional fields some axis reads */
};

/* entry i with the optional fields that g says some axis reads (Geo: pc_hist_geo, or pc_joint_geo of pc_joint.h) */
template <typename Geo>
static __device__ __forceinline__ void pc_hist_load(const pc_spot_src &s, const Geo &g, long long i, pc_hist_entry &e)
{
	const pc_entry b = pc_entry_load(s, i);
	const double *p = s.p + i*s.ss;
	e.x = b.x; e.y = b.y; e.z = b.z; e.dx = b.dx; e.dy = b.dy; e.dz = b.dz;
	e.leak = s.has_dz;
	e.n = e.dtravel = e.sx = e.sy = 0.;
	if (s.has_dz) {          /* a leak event: slot, attempt, coords, direction, electric vector, n_refl */
		if (g.need_n) e.n = p[11*s.fs];
	} else {                 /* an image record: pc_start_coords in planes 2, 3; pc_exit_nrefl (int64) in 15; pc_exit_dtravel in 16 */
		if (g.need_n) e.n = (double)((const long long *)p)[15*s.fs];
		if (g.need_travel) e.dtravel = p[16*s.fs];
		if (g.need_start) { e.sx = p[2*s.fs]; e.sy = p[3*s.fs]; }
	}
}

/* Regime 1: workgroup-private histograms.  The cells [energy][tc] are cut into tiles of PC_HIST_TILE uint64; workgroup (x, y)
 * adds the entries x, x + gridDim.x, ... whose cells fall into tile y to a private copy of it in LDS (ds_add_u64), one entry per
 * lane, then adds every non-zero cell of the copy to the global cells with one atomic.  Several tiles are several passes over
 * the entries.  Where the squares are tracked (Q) a tile is TC = PC_HIST_TILE / 3 cells (pc_tally_tile_cells): their weight sums
 * in tile[0, TC), their square sums as (lo, hi) pairs behind them, flushed with pc_atomic_add128 to sq [cell][2]. */
#define PC_HIST_TILE 8192
#define PC_HIST_LDS_BLOCK 512
/* M: a gated add, s.mask is set (pc_select.h); the plain build reads no mask.  Q: the squares are tracked; the build without reads no sq */
template <bool M, bool Q>
__global__ void __launch_bounds__(PC_HIST_LDS_BLOCK) pc_hist_lds_kernel(pc_spot_src s, pc_hist_geo g, unsigned long long *cells, unsigned long long *sq)
{
	__shared__ unsigned long long tile[PC_HIST_TILE];
	constexpr long long TC = pc_tally_tile_cells(PC_HIST_TILE, Q);
	const long long total = (long long)g.ns*g.tc;
	const long long t0 = (long long)blockIdx.y*TC;
	const long long t1 = (t0 + TC < total) ? t0 + TC : total;
	const int k0 = (int)(t0 / g.tc), k1 = (int)((t1 - 1) / g.tc);      /* the energies with cells in this tile */
	for (int k = threadIdx.x; k < PC_HIST_TILE; k += blockDim.x) tile[k] = 0ull;
	__syncthreads();
	for (long long i = (long long)blockIdx.x*blockDim.x + threadIdx.x; i < s.n; i += (long long)gridDim.x*blockDim.x) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		pc_hist_entry e;
		pc_hist_load(s, g, i, e);
		for (int a = 0; a < g.na; a++) {
			const int b = pc_hist_axis_bin(g.ax[a], e);
			const long long c = g.cell0[a] + (b >= 0 ? b : g.ax[a].n_bins);
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

/* Regime 2: energies across lanes.  The cells are laid out [tc][energy] with the energies innermost: the lanes of a wave take
 * the energies of one entry (64 / gw entries per wave when fewer than 64 are selected, gw = the next power of two), so that one
 * wave instruction is a contiguous run of 8-byte global atomics.  Workgroup (x, c) does energies [c*PC_HIST_ECHUNK, ...); the
 * outside counters of those energies are summed in LDS first (every entry that misses a range adds to the same few counters).
 * Where the squares are tracked (Q) every add to a cell is followed by pc_tally_add_sq on its pair in sq [cell][2], the chunk is
 * PC_HIST_ECHUNK_SQ energies and the outside counters' pairs follow the counters in LDS (48 KiB in all). */
#define PC_HIST_ECHUNK 512
#define PC_HIST_ECHUNK_SQ 128
#define PC_HIST_WIDE_BLOCK 256
template <bool M, bool Q>
__global__ void __launch_bounds__(PC_HIST_WIDE_BLOCK) pc_hist_wide_kernel(pc_spot_src s, pc_hist_geo g, unsigned long long *cells, unsigned long long *sq)
{
	constexpr int EC = Q ? PC_HIST_ECHUNK_SQ : PC_HIST_ECHUNK;
	__shared__ unsigned long long out[PC_HIST_MAX_AXES*EC*(Q ? 3 : 1)];
	unsigned long long *out_sq = out + g.na*EC;      /* [axis*EC + k][2] behind the counters of the na axes, Q only */
	const int s0 = blockIdx.y*EC;
	const int sn = (g.ns - s0 < EC) ? g.ns - s0 : EC;
	for (int k = threadIdx.x; k < g.na*EC*(Q ? 3 : 1); k += blockDim.x) out[k] = 0ull;
	__syncthreads();
	const pc_tally_lanes l = pc_tally_lane_map(sn);
	for (long long i = l.first; i < s.n; i += l.stride) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		pc_hist_entry e;
		pc_hist_load(s, g, i, e);
		int bin[PC_HIST_MAX_AXES];
#pragma unroll
		for (int a = 0; a < PC_HIST_MAX_AXES; a++)
			bin[a] = (a < g.na) ? pc_hist_axis_bin(g.ax[a], e) : -1;
		for (int k = l.sub; k < sn; k += l.gw) {
			const unsigned long long q = pc_spot_q(s.w[i*s.ws + g.sel[s0 + k]]);
			if (!q) continue;
#pragma unroll
			for (int a = 0; a < PC_HIST_MAX_AXES; a++) {
				if (a >= g.na) break;
				if (bin[a] >= 0) {
					const long long c = (long long)(g.cell0[a] + bin[a])*g.ns + s0 + k;
					atomicAdd(cells + c, q);
					if (Q) pc_tally_add_sq(sq + 2*c, q);
				} else {
					atomicAdd(&out[a*EC + k], q);
					if (Q) pc_tally_lds_add_sq(&out_sq[2*(a*EC + k)], q);
				}
			}
		}
	}
	__syncthreads();
	for (int k = threadIdx.x; k < g.na*EC; k += blockDim.x) {
		const int a = k / EC, j = k % EC;
		const unsigned long long v = out[k];
		if (v) {
			const long long c = (long long)(g.cell0[a] + g.ax[a].n_bins)*g.ns + s0 + j;
			atomicAdd(cells + c, v);
			if (Q) pc_atomic_add128(sq + 2*c, out_sq[2*k], out_sq[2*k + 1]);
		}
	}
}

/* Regime of an object (spec->regime 0): private LDS histograms (1) when all its cells fit one tile, energies across lanes (2)
 * otherwise, where regime 1 would pass over the entries once per tile.  Not measured: scripts/bench_hist.py times one add per
 * regime (one N_REFL axis of 256 bins, one X_AT axis of 2048 bins, eight mixed axes; xos1, 1e7 exit photons, 1 and 291 energies)
 * next to the spot map that holds the same X_AT axis.  A wave-level pre-sum of lanes that hit the same cell was not built.
 * The rule is applied when the object is made and not again when it starts to track squares: with 2731 to 8192 cells a tracking
 * object stays in regime 1 and makes two or three passes over the entries (pc_tally_tile_split).  Whether regime 2 is faster there
 * has not been measured. */
static int pc_hist_auto_regime(long long ns, long long tc)
{
	return (ns*tc <= PC_HIST_TILE) ? 1 : 2;
}

/* cells [kind][energy][tc] (regime 1) or [kind][tc][energy] (regime 2) */
struct pc_hip_hist : pc_tally {
	pc_hist_geo geo;                  /* sel is the member's own */
	std::vector<int> offsets;         /* [na + 1] into the bins of one energy */
	int regime = 0;
	size_t per_kind = 0;              /* ns * tc */
};

static int pc_hist_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const pc_hip_hist_spec *spec, pc_hip_hist **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_create: hist must not be NULL");
	*out = nullptr;
	const pc_hip_ctx *c0 = ctxs[0];
	int st = pc_hip_hist_validate(spec, (size_t)c0->host.pm.n_energies);
	if (st) return st;
	pc_hip_hist *h = new pc_hip_hist();
	const std::vector<int> sel = pc_sel_fill(spec->n_energies, spec->energies, (size_t)c0->host.pm.n_energies);
	pc_hist_geo &g = h->geo;
	memset(&g, 0, sizeof(g));
	g.na = spec->n_axes;
	g.ns = (int)sel.size();
	const double zexit = c0->host.z[c0->host.pm.nmax];
	int bins = 0;
	for (int a = 0; a < g.na; a++) {
		const pc_hip_hist_axis &x = spec->axes[a];
		g.ax[a].zp = zexit + x.d;          /* once, on the host */
		g.ax[a].cx = x.cx; g.ax[a].cy = x.cy; g.ax[a].lo = x.lo; g.ax[a].hi = x.hi;
		g.ax[a].quantity = x.quantity; g.ax[a].n_bins = x.n_bins;
		g.cell0[a] = bins + a;
		h->offsets.push_back(bins);
		bins += x.n_bins;
		if (x.quantity == PC_HIST_N_REFL) g.need_n = 1;
		if (x.quantity == PC_HIST_D_TRAVEL) g.need_travel = 1;
		if (x.quantity == PC_HIST_R_START) g.need_start = 1;
	}
	h->offsets.push_back(bins);
	g.tc = bins + g.na;
	h->per_kind = (size_t)g.ns*g.tc;
	h->regime = spec->regime ? spec->regime : pc_hist_auto_regime(g.ns, g.tc);
	st = pc_tally_make(*h, ctxs, group, 3*h->per_kind, "pc_hip_hist_create");
	if (!st) st = pc_tally_upload(*h, sel, std::vector<double>(), "pc_hip_hist_create");
	if (st) { delete h; return st; }
	*out = h;
	return PC_HIP_OK;
}

static int pc_hist_launch(pc_hip_hist *h, pc_tally_member &m, const pc_spot_src &s, int kind)
{
	pc_hip_ctx *c = m.ctx;
	pc_hist_geo g = h->geo;
	g.sel = m.d_sel;
	unsigned long long *cells = m.d_cells + (size_t)kind*h->per_kind;
	unsigned long long *sq = h->squares ? m.d_sq + 2*(size_t)kind*h->per_kind : nullptr;
	if (h->regime == 1) {
		const long long tiles = pc_tally_tile_split((long long)h->per_kind, PC_HIST_TILE, h->squares).tiles;
		const long long bx = pc_tally_grid_tiles(c->n_cu, tiles, s.n, PC_HIST_LDS_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_hist_lds_kernel<true, true> : pc_hist_lds_kernel<false, true>)
		               : (s.mask ? pc_hist_lds_kernel<true, false> : pc_hist_lds_kernel<false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)tiles), dim3(PC_HIST_LDS_BLOCK), 0, c->stream, s, g, cells, sq);
	} else {
		const int ec = sq ? PC_HIST_ECHUNK_SQ : PC_HIST_ECHUNK;
		const long long chunks = (g.ns + ec - 1)/ec;
		const long long bx = pc_tally_grid_wide(c->n_cu, chunks, g.ns, s.n, PC_HIST_WIDE_BLOCK).bx;
		auto kern = sq ? (s.mask ? pc_hist_wide_kernel<true, true> : pc_hist_wide_kernel<false, true>)
		               : (s.mask ? pc_hist_wide_kernel<true, false> : pc_hist_wide_kernel<false, false>);
		hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)chunks), dim3(PC_HIST_WIDE_BLOCK), 0, c->stream, s, g, cells, sq);
	}
	return PC_HIP_OK;
}

/* the members' summed cells (limbs = 1) or square pairs (limbs = 2) from the device layout of the regime into bins
 * [3][ns][total_bins][limbs] and outside [3][na][ns][limbs]; either may be NULL */
static void pc_hist_unpack(const pc_hip_hist *hist, const std::vector<unsigned long long> &sum, size_t limbs, uint64_t *bins, uint64_t *outside)
{
	const pc_hist_geo &g = hist->geo;
	const size_t ns = (size_t)g.ns, tc = (size_t)g.tc, tb = tc - (size_t)g.na;
	for (size_t kind = 0; kind < 3; kind++)
		for (size_t s = 0; s < ns; s++)
			for (int a = 0; a < g.na; a++) {
				const size_t c0 = (size_t)g.cell0[a], nb = (size_t)g.ax[a].n_bins;
				for (size_t b = 0; b <= nb; b++) {
					const unsigned long long *v = &sum[limbs*(kind*hist->per_kind + (hist->regime == 1 ? s*tc + c0 + b : (c0 + b)*ns + s))];
					uint64_t *to = nullptr;
					if (b < nb) { if (bins) to = bins + limbs*((kind*ns + s)*tb + (size_t)hist->offsets[a] + b); }
					else if (outside) to = outside + limbs*((kind*(size_t)g.na + (size_t)a)*ns + s);
					for (size_t l = 0; to && l < limbs; l++) to[l] = v[l];
				}
			}
}

extern "C" {

int pc_hip_hist_validate(const pc_hip_hist_spec *spec, size_t n_energies)
{
	std::string why;
	return pc_hist_spec_check(spec, n_energies, &why) ? PC_HIP_OK : pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_validate: " + why);
}

int pc_hip_hist_create(pc_hip_ctx *ctx, const pc_hip_hist_spec *spec, pc_hip_hist **hist)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_create: ctx must not be NULL");
	return pc_hist_make(std::vector<pc_hip_ctx *>{ctx}, nullptr, spec, hist);
}

int pc_hip_group_hist_create(pc_hip_group *group, const pc_hip_hist_spec *spec, pc_hip_hist **hist)
{
	if (!group) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_hist_create: group must not be NULL");
	return pc_hist_make(group->ctx, group, spec, hist);
}

void pc_hip_hist_destroy(pc_hip_hist *hist)
{
	delete hist;
}

int pc_hip_hist_add(pc_hip_hist *hist, int kind)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_add: hist must not be NULL");
	return pc_tally_add(*hist, kind, "pc_hip_hist_add",
		[hist](size_t k, const pc_spot_src &s, int kd) { return pc_hist_launch(hist, hist->m[k], s, kd); });
}

int pc_hip_hist_read(pc_hip_hist *hist, uint64_t *bins, uint64_t *outside, int64_t *n_entries)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_read: hist must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum(*hist, 1, sum);
	if (st) return st;
	pc_hist_unpack(hist, sum, 1, bins, outside);
	if (n_entries)
		for (int k = 0; k < 3; k++) n_entries[k] = hist->n_entries[k];
	return PC_HIP_OK;
}

int pc_hip_hist_track_squares(pc_hip_hist *hist)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_track_squares: hist must not be NULL");
	return pc_tally_track_squares(*hist, "pc_hip_hist_track_squares");
}

int pc_hip_hist_read_squares(pc_hip_hist *hist, uint64_t *bins_sq, uint64_t *outside_sq)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_read_squares: hist must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum_squares(*hist, "pc_hip_hist_read_squares", sum);
	if (st) return st;
	pc_hist_unpack(hist, sum, 2, bins_sq, outside_sq);
	return PC_HIP_OK;
}

int pc_hip_hist_reset(pc_hip_hist *hist)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_reset: hist must not be NULL");
	return pc_tally_reset(*hist);
}

int pc_hip_hist_info(const pc_hip_hist *hist, int32_t dims[3], int32_t *offsets, int *regime)
{
	if (!hist || !dims) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_info: NULL argument");
	dims[0] = hist->geo.na; dims[1] = hist->geo.ns; dims[2] = hist->offsets.back();
	if (offsets)
		for (size_t k = 0; k < hist->offsets.size(); k++) offsets[k] = hist->offsets[k];
	if (regime) *regime = hist->regime;
	return PC_HIP_OK;
}

double pc_hip_hist_quantile(int32_t n_bins, double lo, double hi, const uint64_t *bins, uint64_t outside, double q)
{
	(void)outside;      /* the quantile is that of the inside weight */
	return (bins != nullptr) ? pc_hist_quantile(n_bins, lo, hi, bins, q) : NAN;
}

double pc_hip_hist_fwhm(int32_t n_bins, double lo, double hi, const uint64_t *bins, double *left, double *right)
{
	return (bins != nullptr) ? pc_hist_fwhm(n_bins, lo, hi, bins, left, right) : NAN;
}

} /* extern "C" */

#endif /* PC_HIST_HOST_ONLY */
#endif /* PC_HIST_H */

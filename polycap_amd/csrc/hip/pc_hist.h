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
 * header after it.  Behind it come pc_cells.h -- the kernels and the object, which the joint histograms (pc_joint.h) share: a histogram
 * is a group of one axis -- and the C functions.
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

#include "pc_cells.h"      /* the cells, the kernels and the object: a histogram is a group of one axis */

struct pc_hip_hist : pc_cells {};

static int pc_hist_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const pc_hip_hist_spec *spec, pc_hip_hist **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_create: hist must not be NULL");
	*out = nullptr;
	const int st = pc_hip_hist_validate(spec, (size_t)ctxs[0]->host.pm.n_energies);
	if (st) return st;
	return pc_cells_make<1>(ctxs, group, std::vector<pc_hip_hist_axis>(spec->axes, spec->axes + spec->n_axes), spec->n_energies, spec->energies, spec->regime,
	                        "pc_hip_hist_create", out);
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
	return pc_cells_add<1>(hist, kind, "pc_hip_hist_add");
}

int pc_hip_hist_read(pc_hip_hist *hist, uint64_t *bins, uint64_t *outside, int64_t *n_entries)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_read: hist must not be NULL");
	return pc_cells_read(hist, bins, outside, n_entries);
}

int pc_hip_hist_track_squares(pc_hip_hist *hist)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_track_squares: hist must not be NULL");
	return pc_tally_track_squares(*hist, "pc_hip_hist_track_squares");
}

int pc_hip_hist_read_squares(pc_hip_hist *hist, uint64_t *bins_sq, uint64_t *outside_sq)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_read_squares: hist must not be NULL");
	return pc_cells_read_squares(hist, "pc_hip_hist_read_squares", bins_sq, outside_sq);
}

int pc_hip_hist_reset(pc_hip_hist *hist)
{
	if (!hist) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_reset: hist must not be NULL");
	return pc_tally_reset(*hist);
}

int pc_hip_hist_info(const pc_hip_hist *hist, int32_t dims[3], int32_t *offsets, int *regime)
{
	if (!hist || !dims) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_info: NULL argument");
	return pc_cells_info(hist, dims, offsets, regime);
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

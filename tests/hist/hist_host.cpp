/* Host compile of the first part of polycap_amd/csrc/hip/pc_hist.h (-DPC_HIST_HOST_ONLY): the per-entry value and bin and the
 * host formulas, as tests/test_hist_cpu.py calls them. */
#define PC_SPOT_HOST_ONLY
#define PC_HIST_HOST_ONLY
#include "pc_spot.h"
#include "pc_hist.h"

extern "C" {

/* entries [n][10] = x, y, z, dx, dy, dz, n_refl, dtravel, sx, sy; axis = zp, cx, cy, lo, hi; values [n], ok [n], bins [n] */
void hist_bins_n(int64_t n, const double *entries, int leak, int quantity, const double *axis, int n_bins, double *values, int32_t *oks,
	int32_t *bins)
{
	pc_hist_axis_k a;
	a.zp = axis[0]; a.cx = axis[1]; a.cy = axis[2]; a.lo = axis[3]; a.hi = axis[4];
	a.quantity = quantity; a.n_bins = n_bins;
	for (int64_t i = 0; i < n; i++) {
		const double *p = entries + 10*i;
		pc_hist_entry e;
		e.x = p[0]; e.y = p[1]; e.z = p[2]; e.dx = p[3]; e.dy = p[4]; e.dz = p[5]; e.n = p[6]; e.dtravel = p[7]; e.sx = p[8]; e.sy = p[9];
		e.leak = leak;
		int ok;
		values[i] = pc_hist_value(a, e, &ok);
		oks[i] = ok;
		bins[i] = pc_hist_axis_bin(a, e);
	}
}

void hist_q_n(int64_t n, const double *w, uint64_t *q)
{
	for (int64_t i = 0; i < n; i++) q[i] = pc_spot_q(w[i]);
}

double hist_exit_dz(double dx, double dy)
{
	return pc_spot_exit_dz(dx, dy);
}

double hist_quantile(int32_t n_bins, double lo, double hi, const uint64_t *bins, double q)
{
	return pc_hist_quantile(n_bins, lo, hi, bins, q);
}

double hist_fwhm(int32_t n_bins, double lo, double hi, const uint64_t *bins, double *left, double *right)
{
	return pc_hist_fwhm(n_bins, lo, hi, bins, left, right);
}

}

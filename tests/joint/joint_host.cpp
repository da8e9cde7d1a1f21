/* Host compile of the first part of polycap_amd/csrc/hip/pc_joint.h (-DPC_JOINT_HOST_ONLY, over the first parts of pc_spot.h and
 * pc_hist.h): the cell of an entry in a pair and the marginals, as tests/test_joint_cpu.py calls them. */
#define PC_SPOT_HOST_ONLY
#define PC_HIST_HOST_ONLY
#define PC_JOINT_HOST_ONLY
#include "pc_spot.h"
#include "pc_joint.h"

static pc_hist_axis_k axis_of(const double *a)
{
	pc_hist_axis_k k;
	k.quantity = (int)a[0]; k.zp = a[1]; k.cx = a[2]; k.cy = a[3]; k.lo = a[4]; k.hi = a[5]; k.n_bins = (int)a[6];
	return k;
}

extern "C" {

/* entries [n][10] = x, y, z, dx, dy, dz, n_refl, dtravel, sx, sy; u, v = quantity, zp, cx, cy, lo, hi, n_bins; cells [n] (-1 outside) */
void joint_cells_n(int64_t n, const double *entries, int leak, const double *u, const double *v, int32_t *cells)
{
	const pc_hist_axis_k au = axis_of(u), av = axis_of(v);
	for (int64_t i = 0; i < n; i++) {
		const double *p = entries + 10*i;
		pc_hist_entry e;
		e.x = p[0]; e.y = p[1]; e.z = p[2]; e.dx = p[3]; e.dy = p[4]; e.dz = p[5]; e.n = p[6]; e.dtravel = p[7]; e.sx = p[8]; e.sy = p[9];
		e.leak = leak;
		cells[i] = pc_joint_cell(au, av, e);
	}
}

void joint_marginal(int32_t nu, int32_t nv, const uint64_t *cells, int which, uint64_t *out)
{
	pc_joint_marginal(nu, nv, cells, which, out);
}

}

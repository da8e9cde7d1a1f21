/* Host compile of the first part of polycap_amd/csrc/hip/pc_select.h (-DPC_SELECT_HOST_ONLY, over the first parts of pc_spot.h and
 * pc_hist.h): pc_select_pass, the check of a spec and the parser of POLYCAP_SELECT, as tests/test_select_cpu.py calls them.  With
 * -DSELECT_HOST_MAIN it is a program of its own, which the same test builds with -fsanitize=address,undefined and runs once. */
#define PC_SPOT_HOST_ONLY
#define PC_HIST_HOST_ONLY
#define PC_SELECT_HOST_ONLY
#include "pc_spot.h"
#include "pc_select.h"

#include <stdio.h>
#include <vector>

/* rows [n_cuts][7] = quantity, d, cx, cy, lo, hi, negate */
static std::vector<pc_hip_select_cut> cuts_of(int n_cuts, const double *rows)
{
	std::vector<pc_hip_select_cut> cuts((size_t)(n_cuts > 0 ? n_cuts : 0));
	for (int k = 0; k < n_cuts; k++) {
		const double *r = rows + 7*k;
		cuts[k].axis.quantity = (int32_t)r[0]; cuts[k].axis.d = r[1]; cuts[k].axis.cx = r[2]; cuts[k].axis.cy = r[3];
		cuts[k].axis.lo = r[4]; cuts[k].axis.hi = r[5]; cuts[k].axis.n_bins = 1;
		cuts[k].negate = (int32_t)r[6];
	}
	return cuts;
}

extern "C" {

/* entries [n][10] = x, y, z, dx, dy, dz, n_refl, dtravel, sx, sy; pass [n] = 0 or 1; -1 when the spec is refused */
int select_pass_n(int64_t n, const double *entries, int leak, int n_cuts, const double *rows, double zexit, uint8_t *pass)
{
	const std::vector<pc_hip_select_cut> cuts = cuts_of(n_cuts, rows);
	const pc_hip_select_spec spec = { n_cuts, cuts.data() };
	std::string why;
	if (!pc_select_spec_check(&spec, &why)) return -1;
	const pc_select_geo g = pc_select_make_geo(&spec, zexit);
	for (int64_t i = 0; i < n; i++) {
		const double *p = entries + 10*i;
		pc_hist_entry e;
		e.x = p[0]; e.y = p[1]; e.z = p[2]; e.dx = p[3]; e.dy = p[4]; e.dz = p[5]; e.n = p[6]; e.dtravel = p[7]; e.sx = p[8]; e.sy = p[9];
		e.leak = leak;
		pass[i] = (uint8_t)pc_select_pass(g, e);
	}
	return 0;
}

/* 0 and rows [8][7], *n_cuts; or -1 and the reason */
int select_parse(const char *value, double *rows, int *n_cuts, char *why, size_t why_len)
{
	pc_hip_select_cut cuts[PC_SELECT_MAX_CUTS];
	std::string bad;
	const bool ok = pc_select_parse(value, cuts, n_cuts, &bad);
	snprintf(why, why_len, "%s", bad.c_str());
	if (!ok) return -1;
	for (int k = 0; k < *n_cuts; k++) {
		double *r = rows + 7*k;
		r[0] = cuts[k].axis.quantity; r[1] = cuts[k].axis.d; r[2] = cuts[k].axis.cx; r[3] = cuts[k].axis.cy;
		r[4] = cuts[k].axis.lo; r[5] = cuts[k].axis.hi; r[6] = cuts[k].negate;
	}
	return 0;
}

}

#ifdef SELECT_HOST_MAIN
/* every function of the host part once, on values that reach its branches: good and refused specs, all twelve quantities on both
 * kinds of entry with NaN, dz <= 0 and values on lo and hi, and the parser on good and malformed values */
int main(void)
{
	int failures = 0;
	const double nan_ = NAN;
	std::vector<double> E;
	const double vals[] = { -1., 0., 0.5, 1., 2., nan_ };
	for (double a : vals)
		for (double dz : { 1., 0., -1., nan_ })
			for (double n : { 0., 3., 300. }) {
				const double row[10] = { a, 0.25*a, 0., 0.1*a, -0.1*a, dz, n, 10.*a, a, -a };
				E.insert(E.end(), row, row + 10);
			}
	const int64_t n = (int64_t)(E.size()/10);
	std::vector<uint8_t> pass((size_t)n);
	for (int q = 0; q < 12; q++)
		for (int negate = 0; negate < 2; negate++)
			for (int leak = 0; leak < 2; leak++) {
				const double rows[14] = { (double)q, q < 3 ? 0.5 : 0., q == 2 ? 0.1 : 0., 0., 0., 1., (double)negate,
				                          6., 0., 0., 0., 0., 256., 0. };
				if (select_pass_n(n, E.data(), leak, 2, rows, 0., pass.data()) != 0) failures++;
				int64_t np = 0;
				for (uint8_t b : pass) np += b;
				if (np < 0 || np > n) failures++;
			}
	{       /* refused specs */
		const double bad_q[7] = { 12., 0., 0., 0., 0., 1., 0. }, bad_range[7] = { 0., 0., 0., 0., 1., 1., 0. }, bad_neg[7] = { 0., 0., 0., 0., 0., 1., 2. };
		std::vector<double> nine;
		for (int k = 0; k < 9; k++) nine.insert(nine.end(), bad_neg, bad_neg + 6), nine.push_back(0.);
		if (select_pass_n(n, E.data(), 0, 1, bad_q, 0., pass.data()) != -1) failures++;
		if (select_pass_n(n, E.data(), 0, 1, bad_range, 0., pass.data()) != -1) failures++;
		if (select_pass_n(n, E.data(), 0, 1, bad_neg, 0., pass.data()) != -1) failures++;
		if (select_pass_n(n, E.data(), 0, 9, nine.data(), 0., pass.data()) != -1) failures++;
		if (select_pass_n(n, E.data(), 0, 0, nullptr, 0., pass.data()) != -1) failures++;
	}
	{
		double rows[8*7];
		int nc = 0;
		char why[256];
		const char *good[] = { "axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not", "axis=start_x,range=-1:1", "axis=z,range=0:1;;axis=z,range=0:1,not;" };
		const char *bad[] = { "", ";", "axis=q,range=0:1", "axis=x", "axis=x,range=0", "axis=x,range=0:1,bins=4", "axis=x,range=1:0", "not", "axis=x,range=0:1,",
		                      "axis=nrefl,d=1,range=0:1", "axis=x,range=0:1,d=", "axis=x,range=0:1,centre=1",
		                      "axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1;axis=z,range=0:1" };
		for (const char *v : good)
			if (select_parse(v, rows, &nc, why, sizeof why) != 0 || nc < 1) { failures++; fprintf(stderr, "refused: %s: %s\n", v, why); }
		for (const char *v : bad)
			if (select_parse(v, rows, &nc, why, sizeof why) != -1 || !why[0]) { failures++; fprintf(stderr, "accepted: %s\n", v); }
		if (select_parse(nullptr, rows, &nc, why, sizeof why) != -1) failures++;
	}
	printf("select_host: %d failures\n", failures);
	return failures ? 1 : 0;
}
#endif

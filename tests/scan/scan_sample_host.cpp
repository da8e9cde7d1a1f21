// TEST-ONLY: host compile of the scan mapping and the per-point sampler of pc_device.h (pc_scan_map, pc_scan_sample), built by
// tests/test_scan_cpu.py into a temporary directory; never part of libpolycap.  Same flags as tests/emul (no contraction).
#include <string>

#include "pc_problem.h"

extern "C" {

// out[12*n]: start(3), dir(3), elecv(3), src_start x, y, 0 -- the layout of pc_hip_sample_photons
int scan_sample_host(const pc_hip_problem *p, const pc_hip_scan_point *pts, int64_t n_per_point, int64_t slot0, uint64_t seed,
                     int64_t n, const int64_t *flat, const uint32_t *attempts, double *out, int64_t *point_of)
{
	pc_host_tables t;
	std::string err;
	if (pc_build_tables(p, t, err)) return -1;
	const pc_scan_point *sp = (const pc_scan_point *)pts;
	for (int64_t i = 0; i < n; i++) {
		pc_start s;
		if (t.pm.generic_src) pc_scan_sample<true>(t.pm, sp, n_per_point, slot0, seed, flat[i], attempts[i], s);
		else pc_scan_sample<false>(t.pm, sp, n_per_point, slot0, seed, flat[i], attempts[i], s);
		double *o = out + 12*i;
		o[0] = s.x; o[1] = s.y; o[2] = s.z; o[3] = s.dx; o[4] = s.dy; o[5] = s.dz;
		o[6] = s.ex; o[7] = s.ey; o[8] = s.ez; o[9] = s.srcx; o[10] = s.srcy; o[11] = 0.;
		long long k, j;
		pc_scan_map(flat[i], n_per_point, k, j);
		point_of[2*i] = k; point_of[2*i + 1] = j;
	}
	return 0;
}

}

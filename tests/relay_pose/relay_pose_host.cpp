/* The arithmetic of a posed relay (pc_relay.h: a tilted second optic) compiled for the host alone: what tests/test_relay_pose_cpu.py
 * checks against numpy and mpmath and what tests/test_gpu_relay_pose.py applies to fetched records for the host round trip. */
#define PC_RELAY_HOST_ONLY
#include "pc_relay.h"

extern "C" {

/* in [n][6] = x, y, dx, dy, ex, ey; out [n][10], written where hit [n] is 1 */
void relay_fly_posed_n(int64_t n, const double *in, double gap, double off_x, double off_y, const double *basis, double *out, int32_t *hit)
{
	for (int64_t i = 0; i < n; i++)
		hit[i] = pc_relay_fly_posed(in[6*i], in[6*i + 1], in[6*i + 2], in[6*i + 3], in[6*i + 4], in[6*i + 5], gap, off_x, off_y, basis, out + 10*i);
}

void relay_pose_basis(double tilt_x, double tilt_y, double *basis) { pc_relay_pose_basis(tilt_x, tilt_y, basis); }

int relay_pose_ok(double gap, double off_x, double off_y, double tilt_x, double tilt_y) { return pc_relay_pose_ok(gap, off_x, off_y, tilt_x, tilt_y); }

int relay_pose_plain(double tilt_x, double tilt_y, int selected) { return pc_relay_pose_plain(tilt_x, tilt_y, selected); }

}

/* The pc_hip_* functions pc_request.c calls, for tests/request/request_host.c: the checks of the first parts of pc_spot.h, pc_hist.h,
 * pc_joint.h and pc_select.h (-DPC_*_HOST_ONLY) behind the same wrappers and texts as the library's, the message of the last refusal,
 * and no device. */
#define PC_SPOT_HOST_ONLY
#define PC_HIST_HOST_ONLY
#define PC_JOINT_HOST_ONLY
#define PC_SELECT_HOST_ONLY
#include "pc_spot.h"
#include "pc_joint.h"
#include "pc_select.h"

#include <stdio.h>

static thread_local std::string g_last_error;

static int pc_fail(int code, const std::string &msg)
{
	g_last_error = msg;
	return code;
}

extern "C" {

const char *pc_hip_last_error(void)
{
	return g_last_error.c_str();
}

int pc_hip_device_count(void)
{
	return 0;
}

int pc_hip_spot_validate(const pc_hip_spot_spec *spec, size_t n_energies)
{
	std::string why;
	return pc_spot_spec_check(spec, n_energies, &why) ? PC_HIP_OK : pc_fail(PC_HIP_ERR_INVALID, why);
}

int pc_hip_hist_validate(const pc_hip_hist_spec *spec, size_t n_energies)
{
	std::string why;
	return pc_hist_spec_check(spec, n_energies, &why) ? PC_HIP_OK : pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_validate: " + why);
}

int pc_hip_joint_validate(const pc_hip_joint_spec *spec, size_t n_energies)
{
	std::string why;
	return pc_joint_spec_check(spec, n_energies, &why) ? PC_HIP_OK : pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_validate: " + why);
}

int pc_hip_select_parse(const char *value, pc_hip_select_cut *cuts, int32_t *n_cuts, char *why, size_t why_len)
{
	pc_hip_select_cut tmp[PC_SELECT_MAX_CUTS];
	int n = 0;
	std::string bad;
	const bool ok = pc_select_parse(value, tmp, &n, &bad);
	if (why && why_len > 0) snprintf(why, why_len, "%s", ok ? "" : bad.c_str());
	if (!ok) return PC_HIP_ERR_INVALID;
	if (cuts) memcpy(cuts, tmp, sizeof(pc_hip_select_cut)*(size_t)n);
	if (n_cuts) *n_cuts = n;
	return PC_HIP_OK;
}

}

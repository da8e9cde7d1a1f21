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
 * pc_spot.h's (pc_spot_q), the kernels and the object are pc_cells.h's with groups of two axes.  The first part (the cell of an entry, the marginals, the check of a spec) compiles for the host
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

struct pc_hip_joint : pc_cells {};      /* pc_cells.h: a joint histogram is a group of two axes, u of pair p at 2p and v at 2p + 1 */

static int pc_joint_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const pc_hip_joint_spec *spec, pc_hip_joint **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_create: joint must not be NULL");
	*out = nullptr;
	const int st = pc_hip_joint_validate(spec, (size_t)ctxs[0]->host.pm.n_energies);
	if (st) return st;
	std::vector<pc_hip_hist_axis> axes;
	for (int p = 0; p < spec->n_pairs; p++) {
		axes.push_back(spec->pairs[p].u);
		axes.push_back(spec->pairs[p].v);
	}
	return pc_cells_make<2>(ctxs, group, axes, spec->n_energies, spec->energies, spec->regime, "pc_hip_joint_create", out);
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
	return pc_cells_add<2>(joint, kind, "pc_hip_joint_add");
}

int pc_hip_joint_read(pc_hip_joint *joint, uint64_t *cells, uint64_t *outside, int64_t *n_entries)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_read: joint must not be NULL");
	return pc_cells_read(joint, cells, outside, n_entries);
}

int pc_hip_joint_track_squares(pc_hip_joint *joint)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_track_squares: joint must not be NULL");
	return pc_tally_track_squares(*joint, "pc_hip_joint_track_squares");
}

int pc_hip_joint_read_squares(pc_hip_joint *joint, uint64_t *cells_sq, uint64_t *outside_sq)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_read_squares: joint must not be NULL");
	return pc_cells_read_squares(joint, "pc_hip_joint_read_squares", cells_sq, outside_sq);
}

int pc_hip_joint_reset(pc_hip_joint *joint)
{
	if (!joint) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_reset: joint must not be NULL");
	return pc_tally_reset(*joint);
}

int pc_hip_joint_info(const pc_hip_joint *joint, int32_t dims[3], int32_t *offsets, int *regime)
{
	if (!joint || !dims) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_info: NULL argument");
	return pc_cells_info(joint, dims, offsets, regime);
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

/* Host compile of the first part of polycap_amd/csrc/hip/pc_tally.h (-DPC_TALLY_HOST_ONLY): the energy selection, the grid sizing
 * and the 128-bit add, as tests/test_tally_cpu.py calls them. */
#define PC_TALLY_HOST_ONLY
#include <stdint.h>
#include <string.h>
#include "pc_tally.h"

extern "C" {

/* 1 when the selection is accepted; else 0 and the reason in why[cap] */
int tally_sel_check(int n_sel, const int *sel, int64_t n_energies, char *why, int cap)
{
	std::string w;
	const bool ok = pc_sel_check(n_sel, sel, (size_t)n_energies, &w);
	strncpy(why, w.c_str(), (size_t)cap - 1);
	why[cap - 1] = 0;
	return ok ? 1 : 0;
}

/* the expansion into out[n_energies]; returns how many indices it holds */
int tally_sel_fill(int n_sel, const int *sel, int64_t n_energies, int *out)
{
	const std::vector<int> v = pc_sel_fill(n_sel, sel, (size_t)n_energies);
	for (size_t k = 0; k < v.size(); k++) out[k] = v[k];
	return (int)v.size();
}

int64_t tally_grid_tiles(int64_t cus, int64_t tiles, int64_t n_entries, int block)
{
	return pc_tally_grid_tiles(cus, tiles, n_entries, block).bx;
}

int64_t tally_grid_wide(int64_t cus, int64_t groups, int n_sel, int64_t n_entries, int block, int *gw)
{
	const pc_tally_grid g = pc_tally_grid_wide(cus, groups, n_sel, n_entries, block);
	*gw = g.gw;
	return g.bx;
}

/* v = (lo, hi) += (add_lo, add_hi) */
void tally_add128(uint64_t *v, uint64_t add_lo, uint64_t add_hi)
{
	unsigned long long lo = v[0], hi = v[1];
	pc_add128(lo, hi, add_lo, add_hi);
	v[0] = lo; v[1] = hi;
}

}

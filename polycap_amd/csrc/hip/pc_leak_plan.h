/*
 * pc_leak_plan.h -- the host's decisions about a leak_calc=true run as functions of plain values, like pc_plan.h: no HIP call, no
 * context, so the header compiles for the host (tests/plan/leak_host.cpp).  The grid of the leak kernel, the size of the record
 * buffer and whether and how the slots are handed out heaviest first.  The only reader is pc_leak_run (pc_leak_run.h).  Also here,
 * because the grid needs them: the leak kernel's workgroup size and the size of a frame's header.
 */
#ifndef PC_LEAK_PLAN_H
#define PC_LEAK_PLAN_H

#include <algorithm>
#include <cstddef>
#include <vector>

#ifndef PC_LEAK_BLOCK
#define PC_LEAK_BLOCK 256
#endif
#define PC_LF_HDR 24           /* doubles of a suspended parent frame before its weights (the PC_LF_ fields of pc_leak.h) */

/* grid of the leak kernel: as many lanes as the stack budget allows, at most two resident blocks per CU */
struct pc_leak_grid { int blocks; long long lanes; };
static pc_leak_grid pc_plan_leak_grid(long long n_items, int n_energies, int max_depth, size_t stack_bytes, int n_cu)
{
	const size_t per_lane = (size_t)max_depth * (PC_LF_HDR + (size_t)n_energies) * sizeof(double);
	long long by_mem = (long long)(stack_bytes / per_lane);
	long long want = (n_items + PC_LEAK_BLOCK - 1) / PC_LEAK_BLOCK;
	long long max_blocks = (long long)n_cu * 2;
	long long blocks = std::min(want, max_blocks);
	blocks = std::min(blocks, std::max(1ll, by_mem / PC_LEAK_BLOCK));
	if (blocks < 1) blocks = 1;
	return pc_leak_grid{(int)blocks, blocks * PC_LEAK_BLOCK};
}

/* record buffer of a run's first launch: events per slot grow with the number of energies (a leak is kept while ANY energy holds
 * >= 1e-4): 9 per slot at one energy, 29 at seven on the reference's test optic; a run that outgrows the buffer is repeated, so
 * the first guess is generous (16 + 8 n_energies records per slot, at least `floor`) unless the option "leak_capacity" sets it */
static long long pc_plan_leak_capacity(long long option, int n_energies, long long n, long long floor)
{
	return option > 0 ? option : std::max<long long>(floor, (16 + 8*(long long)n_energies)*n);
}

/* and of the repetition of a launch that produced `needed` records */
static long long pc_plan_leak_grown(long long needed)
{
	return needed + needed/4 + 1024;
}

/* An automatic order is considered when every lane gets two to five slots: with fewer there is nothing to order, with more the
 * launch is not bound by its longest slot (the check of pc_plan_leak_order, made beforehand with the reference optic's ratio of
 * longest to mean slot, 11.6) */
static bool pc_plan_leak_order_considered(bool enabled, long long n, long long lanes)
{
	return enabled && 2*lanes <= n && n < 5*lanes && n < (1ll << 32);
}

/* From the predicted units of work of the n slots (est): are they handed out heaviest first (order = the slots in descending order
 * of est, equal ones in slot order; the first n_heavy of them to lanes with a wave to themselves), or in slot order? */
struct pc_leak_order_plan {
	bool ordered = false;
	unsigned int top = 0;          /* the longest slot's and all slots' predicted units */
	unsigned long long total = 0;
	long long n_heavy = 0;
};
static pc_leak_order_plan pc_plan_leak_order(const unsigned int *est, long long n, long long lanes, int n_cu, std::vector<unsigned int> &order)
{
	pc_leak_order_plan p;
	/* Is the launch bound by its longest slot?  A lone lane works through a unit in about 4 us, a lane among the 64 of a busy wave
	 * in about 13 us: with the slots in slot order the launch lasts about (all work / lanes) x 13 us, the longest slot alone
	 * (its work) x 4 us.  When the second is not most of the first (launches of many slots per lane), handing the heaviest slots
	 * to lanes of their own only takes lanes away from the rest: slot order stays (measured: 524288 and 1048576 slots lose 4-7 %,
	 * 262144 gain 10-15 %). */
	for (long long k = 0; k < n; k++) { if (est[k] > p.top) p.top = est[k]; p.total += est[k]; }
	if (!((double)p.top * 4.0 * (double)lanes > 0.8 * 13.0 * (double)p.total)) return p;
	const unsigned int top = p.top;
	/* descending counting sort (stable: equal counts keep slot order) */
	order.resize((size_t)n);
	if (top < (1u << 22)) {
		std::vector<unsigned int> first((size_t)top + 2, 0);
		for (long long k = 0; k < n; k++) first[(size_t)(top - est[k]) + 1]++;
		for (size_t v = 0; v + 1 < first.size(); v++) first[v + 1] += first[v];
		for (long long k = 0; k < n; k++) order[first[(size_t)(top - est[k])]++] = (unsigned int)k;
	} else {
		for (long long k = 0; k < n; k++) order[(size_t)k] = (unsigned int)k;
		std::stable_sort(order.begin(), order.end(), [&](unsigned int x, unsigned int y) { return est[x] > est[y]; });
	}
	p.ordered = true;
	/* one heavy slot per wave at most: the wave is the heavy lane's alone while it lasts */
	p.n_heavy = std::min<long long>(n / 400, (long long)n_cu * 2);
	return p;
}

#endif /* PC_LEAK_PLAN_H */

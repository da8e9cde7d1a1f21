/* The leak planner of pc_leak_plan.h compiled for the host: what tests/test_leak_plan_cpu.py calls (tests/plan/pyleakplan.py builds
 * it as a shared library).  With -DLEAK_HOST_MAIN it is a program that walks the same cases, for a run under
 * -fsanitize=address,undefined:
 *     g++ -std=c++17 -g -fsanitize=address,undefined -DLEAK_HOST_MAIN -I polycap_amd/csrc/hip tests/plan/leak_host.cpp -o leak_host && ./leak_host */
#include "pc_leak_plan.h"

#include <cstdint>

extern "C" {

int leak_block(void) { return PC_LEAK_BLOCK; }
int leak_frame_header(void) { return PC_LF_HDR; }

/* out: blocks, lanes */
void leak_grid(int64_t n_items, int32_t ne, int32_t max_depth, uint64_t stack_bytes, int32_t n_cu, int64_t *out)
{
	const pc_leak_grid g = pc_plan_leak_grid(n_items, ne, max_depth, (size_t)stack_bytes, n_cu);
	out[0] = g.blocks; out[1] = g.lanes;
}

int64_t leak_capacity(int64_t option, int32_t ne, int64_t n, int64_t floor) { return pc_plan_leak_capacity(option, ne, n, floor); }
int64_t leak_grown(int64_t needed) { return pc_plan_leak_grown(needed); }
int leak_order_considered(int enabled, int64_t n, int64_t lanes) { return pc_plan_leak_order_considered(enabled != 0, n, lanes) ? 1 : 0; }

/* out: top, total, n_heavy; order[n] is written when the return value is 1 (ordered), else left alone (slot order kept) */
int leak_order(const uint32_t *est, int64_t n, int64_t lanes, int32_t n_cu, uint32_t *order, uint64_t *out)
{
	std::vector<unsigned int> o;
	const pc_leak_order_plan p = pc_plan_leak_order(est, n, lanes, n_cu, o);
	out[0] = p.top; out[1] = p.total; out[2] = (uint64_t)p.n_heavy;
	if (p.ordered) std::copy(o.begin(), o.end(), order);
	return p.ordered ? 1 : 0;
}

}

#ifdef LEAK_HOST_MAIN
#include <cstdio>
#include <cstdlib>
#include <numeric>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "leak_host: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static int64_t blocks_of(int64_t n, int ne, int depth, uint64_t bytes)
{
	int64_t g[2];
	leak_grid(n, ne, depth, bytes, 256, g);
	CHECK(g[1] == g[0]*PC_LEAK_BLOCK);
	return g[0];
}

/* is `order` the descending stable order of est? */
static void check_order(const std::vector<uint32_t> &est, int64_t lanes, int expect_ordered)
{
	const int64_t n = (int64_t)est.size();
	std::vector<uint32_t> order((size_t)n, 0xffffffffu), want((size_t)n);
	uint64_t out[3];
	const int ordered = leak_order(est.data(), n, lanes, 256, order.data(), out);
	CHECK(ordered == expect_ordered);
	CHECK(out[0] == *std::max_element(est.begin(), est.end()));
	CHECK(out[1] == std::accumulate(est.begin(), est.end(), (uint64_t)0));
	if (!ordered) { CHECK(out[2] == 0); return; }
	CHECK(out[2] == (uint64_t)std::min<int64_t>(n/400, 512));
	std::iota(want.begin(), want.end(), 0u);
	std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return est[x] > est[y]; });
	CHECK(order == want);
}

int main(void)
{
	const uint64_t big = (uint64_t)8 << 30;
	const uint64_t per_lane1 = 40*(PC_LF_HDR + 1)*8, per_lane7 = 40*(PC_LF_HDR + 7)*8;
	CHECK(blocks_of(1, 1, 40, big) == 1 && blocks_of(256, 1, 40, big) == 1 && blocks_of(257, 1, 40, big) == 2 && blocks_of(10000000, 1, 40, big) == 512);
	CHECK(blocks_of(10000000, 1, 40, 3*256*per_lane1 + 1) == 3 && blocks_of(10000000, 1, 40, 256*per_lane1 - 1) == 1);
	CHECK(blocks_of(10000000, 7, 40, 3*256*per_lane7 + 1) == 3 && blocks_of(10000000, 7, 40, 3*256*per_lane7 - 1) == 2);
	CHECK(leak_capacity(5, 1, 1000000, 65536) == 5 && leak_capacity(0, 1, 1, 65536) == 65536 && leak_capacity(0, 7, 10000, 65536) == 720000
	      && leak_capacity(0, 1, 1, 4096) == 4096);
	CHECK(leak_grown(0) == 1024 && leak_grown(7) == 1032 && leak_grown(1000000000) == 1250001024);
	CHECK(!leak_order_considered(1, 511, 256) && leak_order_considered(1, 512, 256) && leak_order_considered(1, 1279, 256)
	      && !leak_order_considered(1, 1280, 256) && !leak_order_considered(0, 600, 256));
	CHECK(!leak_order_considered(1, 200000, 131072) && leak_order_considered(1, 262144, 131072) && !leak_order_considered(1, 1ll << 32, 1ll << 31));
	check_order(std::vector<uint32_t>(600, 10), 256, 0);
	{
		std::vector<uint32_t> est(600, 1);
		est[123] = 1000;
		check_order(est, 256, 1);
	}
	check_order(std::vector<uint32_t>(5000, 0), 256, 0);          /* total = 0: the bound is false */
	{
		/* many ties; lanes chosen so large that the launch counts as bound by its longest slot */
		std::vector<uint32_t> est(5000);
		uint32_t x = 12345;
		for (uint32_t &e : est) { x = x*1664525u + 1013904223u; e = (x >> 16) % 51; }
		check_order(est, 1 << 20, 1);
		est[777] = (1u << 22) - 1; check_order(est, 1 << 20, 1);      /* the counting sort's largest value */
		est[777] = 1u << 22; check_order(est, 1 << 20, 1);            /* the comparison sort's smallest */
	}
	for (int64_t n : {399, 400, 204800, 1000000}) {
		std::vector<uint32_t> est((size_t)n, 1);
		est[0] = 1u << 30;
		check_order(est, 256, 1);                                     /* checks n_heavy = min(n/400, 512) */
	}
	puts("leak_host: ok");
	return 0;
}
#endif

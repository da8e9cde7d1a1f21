/* Host compile of the first part of polycap_amd/csrc/hip/pc_gather.h (-DPC_GATHER_HOST_ONLY): the tile planner of the compaction, the
 * chunk split of a window and the argument check of pc_hip_select_gather, as tests/test_gather_cpu.py calls them.  With
 * -DGATHER_HOST_MAIN it is a program of its own, which the same test builds with -fsanitize=address,undefined and runs once. */
#define PC_GATHER_HOST_ONLY
#include "pc_gather.h"

#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" {

/* the tiles of n entries under option `tile`: spans [cap][2] = lo, hi of the first min(tiles, cap); returns the tile count; *tile_used */
int64_t gather_plan(int64_t n, int64_t tile, int64_t cap, int64_t *spans, int64_t *tile_used)
{
	const pc_gather_tiling p = pc_gather_plan(n, tile);
	*tile_used = p.tile;
	for (int64_t t = 0; t < p.tiles && t < cap; t++) {
		long long lo, hi;
		pc_gather_tile_span(p, n, t, &lo, &hi);
		spans[2*t] = lo; spans[2*t + 1] = hi;
	}
	return p.tiles;
}

int gather_tile_ok(int64_t v)
{
	return pc_gather_tile_ok(v) ? 1 : 0;
}

int64_t gather_chunk_rows(int64_t option, int64_t row_doubles)
{
	return pc_gather_chunk_rows(option, row_doubles);
}

/* the chunks of [first, first + count) at `rows` rows each: chunks [cap][2] = lo, n; returns the chunk count */
int64_t gather_chunks(int64_t first, int64_t count, int64_t rows, int64_t cap, int64_t *chunks)
{
	const long long nc = pc_gather_n_chunks(count, rows);
	for (long long k = 0; k < nc && k < cap; k++) {
		long long lo, n;
		pc_gather_chunk(first, count, rows, k, &lo, &n);
		chunks[2*k] = lo; chunks[2*k + 1] = n;
	}
	return nc;
}

/* 0 when the arguments pass (n_pass < 0: the window is not checked), else -2 and the reason */
int gather_check(int have_select, int kind, int64_t first, int64_t count, int have_records, int64_t n_pass, char *why, size_t why_len)
{
	static int object;
	std::string bad;
	bool ok = pc_gather_args_check(have_select ? &object : nullptr, kind, first, count, have_records ? &object : nullptr, &bad);
	if (ok && n_pass >= 0) ok = pc_gather_window_check(first, count, n_pass, &bad);
	snprintf(why, why_len, "%s", bad.c_str());
	return ok ? 0 : -2;
}

}

#ifdef GATHER_HOST_MAIN
/* every function of the host part once, on values that reach its branches */
int main(void)
{
	int failures = 0;
	std::vector<int64_t> buf(2*20000);
	const int64_t ns[] = { 0, 1, 63, 64, 65, 4095, 4096, 4097, 1000001 }, tiles[] = { 0, 64, 128, 4096, 65536 };
	for (int64_t n : ns)
		for (int64_t tile : tiles) {
			int64_t used = 0;
			const int64_t nt = gather_plan(n, tile, 20000, buf.data(), &used);
			int64_t at = 0;
			for (int64_t t = 0; t < nt && t < 20000; t++) {
				if (buf[2*t] != at || buf[2*t + 1] <= at || buf[2*t + 1] - at > used) failures++;
				at = buf[2*t + 1];
			}
			if (nt <= 20000 && at != n) failures++;
			if (used != (tile ? tile : PC_GATHER_TILE_AUTO)) failures++;
		}
	for (int64_t v : { 0, 64, 128, 65536 }) if (!gather_tile_ok(v)) failures++;
	for (int64_t v : { -64, 1, 63, 65, 100, 65600, 131072 }) if (gather_tile_ok(v)) failures++;
	if (gather_chunk_rows(7, 18) != 7 || gather_chunk_rows(0, 18) != (128ll << 20)/(18*8) || gather_chunk_rows(0, 1ll << 40) != 1) failures++;
	for (int64_t rows : { 1, 7, 1000 })
		for (int64_t first : { 0, 5, 9000 })
			for (int64_t count : { 0, 1, 6, 7, 8, 1001 }) {
				const int64_t nc = gather_chunks(first, count, rows, 20000, buf.data());
				int64_t at = first;
				for (int64_t k = 0; k < nc; k++) {
					if (buf[2*k] != at || buf[2*k + 1] < 1 || buf[2*k + 1] > rows) failures++;
					at += buf[2*k + 1];
				}
				if (at != first + count) failures++;
			}
	char why[256];
	if (gather_check(1, 0, 0, 0, 0, -1, why, sizeof why) != 0 || why[0]) failures++;
	if (gather_check(1, 2, 3, 4, 1, 7, why, sizeof why) != 0) failures++;
	if (gather_check(0, 0, 0, 1, 1, -1, why, sizeof why) != -2 || !strstr(why, "select")) failures++;
	if (gather_check(1, 3, 0, 1, 1, -1, why, sizeof why) != -2 || !strstr(why, "kind")) failures++;
	if (gather_check(1, -1, 0, 1, 1, -1, why, sizeof why) != -2 || !strstr(why, "kind")) failures++;
	if (gather_check(1, 0, -1, 1, 1, -1, why, sizeof why) != -2 || !strstr(why, "first")) failures++;
	if (gather_check(1, 0, 0, -1, 1, -1, why, sizeof why) != -2 || !strstr(why, "count")) failures++;
	if (gather_check(1, 0, 0, 1, 0, -1, why, sizeof why) != -2 || !strstr(why, "records")) failures++;
	if (gather_check(1, 0, 3, 5, 1, 7, why, sizeof why) != -2 || !strstr(why, "n_pass")) failures++;
	if (gather_check(1, 0, 8, 0, 1, 7, why, sizeof why) != -2 || !strstr(why, "n_pass")) failures++;
	if (gather_check(1, 0, INT64_MAX, INT64_MAX, 1, 7, why, sizeof why) != -2) failures++;
	printf("gather_host: %d failures\n", failures);
	return failures ? 1 : 0;
}
#endif

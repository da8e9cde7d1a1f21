/* Host compile of what the squared-weight sums of the tallies do off the device: the first parts of polycap_amd/csrc/hip/pc_tally.h
 * (-DPC_TALLY_HOST_ONLY: the per-entry square, the carry add, the tile split, pc_hip_tally_stderr and pc_hip_select_transmission) and
 * of pc_spot.h (the quantisation), as tests/test_tally_squares_cpu.py calls them.  With -DSQUARES_HOST_MAIN it is a program of its own,
 * which the same test builds with -fsanitize=address,undefined and runs once. */
#define PC_TALLY_HOST_ONLY
#define PC_SPOT_HOST_ONLY
#include <stdint.h>
#include <stdio.h>
#include "pc_tally.h"
#include "pc_spot.h"

extern "C" {

/* W = pc_spot_q(w), and its square as out = (lo, hi) */
uint64_t squares_entry(double w, uint64_t *out)
{
	const unsigned long long W = pc_spot_q(w);
	unsigned long long lo, hi;
	pc_tally_sq(W, lo, hi);
	out[0] = lo; out[1] = hi;
	return W;
}

/* v = (lo, hi) += the squares of W[0 .. n): what a cell's pair holds after these entries */
void squares_accumulate(uint64_t *v, int64_t n, const uint64_t *W)
{
	unsigned long long lo = v[0], hi = v[1];
	for (int64_t k = 0; k < n; k++) {
		unsigned long long a, b;
		pc_tally_sq(W[k], a, b);
		pc_add128(lo, hi, a, b);
	}
	v[0] = lo; v[1] = hi;
}

/* out = (cells of a tile, tiles) */
void squares_tile_split(int64_t total, int64_t tile, int squares, int64_t *out)
{
	const pc_tally_tiling t = pc_tally_tile_split(total, tile, squares);
	out[0] = t.cells; out[1] = t.tiles;
}

void squares_stderr(int64_t n_cells, const uint64_t *sums, const uint64_t *squares, int64_t n_started, double *out)
{
	pc_tally_stderr((size_t)n_cells, sums, squares, n_started, out);
}

void squares_transmission(int64_t ne, const uint64_t *pw, const uint64_t *rw, const uint64_t *pw2, const uint64_t *rw2, double *T, double *T_err)
{
	pc_tally_transmission((size_t)ne, pw, rw, pw2, rw2, T, T_err);
}

}

#ifdef SQUARES_HOST_MAIN
/* every function once, on values that reach its branches: the weights of the test, W = 2^32, a pair whose lo wraps, both tile
 * seams, N < 2, S = 0, a clipped variance, P + R = 0 and NULL outputs */
int main(void)
{
	int failures = 0;
	const double ws[] = { 0., -1., NAN, 0x1p-33, 1e-6, 0.5, 1. - 0x1p-53, 1. };
	uint64_t pair[2] = { 0, 0 }, one[2];
	std::vector<uint64_t> W;
	for (double w : ws) W.push_back(squares_entry(w, one));
	if (one[0] != 0 || one[1] != 1 || W.back() != (1ull << 32)) failures++;          /* w = 1: W = 2^32, W*W = 2^64 */
	for (int k = 0; k < 9; k++) W.push_back(0xfffffff0ull + (uint64_t)k);
	squares_accumulate(pair, (int64_t)W.size(), W.data());
	if (pair[1] < 9) failures++;                                                       /* nine squares near 2^64 and 2^64 itself */
	int64_t t[2];
	for (int sq = 0; sq < 2; sq++)
		for (int64_t total : { 1ll, 2729ll, 2730ll, 2731ll, 8191ll, 8192ll, 8193ll, 1ll << 26 }) {
			squares_tile_split(total, 8192, sq, t);
			if (t[0] != (sq ? 2730 : 8192) || t[1]*t[0] < total || (t[1] - 1)*t[0] >= total) failures++;
		}
	const uint64_t S[4] = { 0, 1ull << 31, 1ull << 32, 3ull << 30 };
	const uint64_t S2[8] = { 0, 0, 1ull << 62, 0, 0, 1, 0, 0 };                        /* the last: q - m*m < 0, clipped */
	double out[4];
	for (int64_t n : { -1ll, 0ll, 1ll, 2ll, 1000ll }) {
		squares_stderr(4, S, S2, n, out);
		for (double v : out)
			if ((n < 2) != (v != v) || v < 0.) failures++;
	}
	if (out[0] != 0. || out[3] != 0.) failures++;
	const uint64_t P[3] = { 0, 1ull << 31, 5 }, R[3] = { 0, 1ull << 30, 0 }, P2[6] = { 0, 0, 1ull << 61, 0, 25, 0 }, R2[6] = { 0, 0, 1ull << 60, 0, 0, 0 };
	double T[3], E[3];
	squares_transmission(3, P, R, P2, R2, T, E);
	if (T[0] == T[0] || E[0] == E[0] || !(T[1] > 0.66 && T[1] < 0.67) || !(E[1] > 0.) || T[2] != 1. || E[2] != 0.) failures++;
	squares_transmission(3, P, R, P2, R2, nullptr, E);
	squares_transmission(3, P, R, P2, R2, T, nullptr);
	printf("squares_host: %d failures\n", failures);
	return failures ? 1 : 0;
}
#endif

/* Host compile of the first part of polycap_amd/csrc/hip/pc_draw.h (-DPC_DRAW_HOST_ONLY): the thresholds of the draws, their inverse,
 * the draws of a cumulative range and the argument and window checks of pc_hip_select_draw, as tests/test_draw_cpu.py calls them: the
 * very arithmetic the device runs.  With -DDRAW_HOST_MAIN it is a program of its own, which the same test builds with
 * -fsanitize=address,undefined and runs once. */
#define PC_DRAW_HOST_ONLY
#include "pc_draw.h"

#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" {

/* out[j] = t_k for k = ks[j] */
void draw_thresholds(int64_t n, const uint64_t *ks, uint32_t phase, uint64_t T, uint64_t N, uint64_t *out)
{
	for (int64_t j = 0; j < n; j++) out[j] = pc_draw_threshold(ks[j], phase, T, N);
}

/* out[j] = K(cs[j]) */
void draw_belows(int64_t n, const uint64_t *cs, uint32_t phase, uint64_t T, uint64_t N, uint64_t *out)
{
	for (int64_t j = 0; j < n; j++) out[j] = pc_draw_below(cs[j], phase, T, N);
}

void draw_mul64(uint64_t a, uint64_t b, uint64_t *lo, uint64_t *hi)
{
	unsigned long long l, h;
	pc_draw_mul64(a, b, &l, &h);
	*lo = l; *hi = h;
}

void draw_range(uint64_t c_lo, uint64_t c_hi, uint32_t phase, uint64_t T, uint64_t N, uint64_t first, uint64_t count, uint64_t *k_lo, uint64_t *k_hi)
{
	unsigned long long a, b;
	pc_draw_range(c_lo, c_hi, phase, T, N, first, count, &a, &b);
	*k_lo = a; *k_hi = b;
}

/* 0 when the arguments pass (have_total = 0: the window and the total are not checked), else -2 and the reason */
int draw_check(int have_select, int kind, int64_t energy, int64_t n_energies, int64_t n_draw, int64_t first, int64_t count, int have_records,
	int have_total, uint64_t total, char *why, size_t why_len)
{
	static int object;
	std::string bad;
	bool ok = pc_draw_args_check(have_select ? &object : nullptr, kind, energy, n_energies, n_draw, first, count, have_records ? &object : nullptr, &bad);
	if (ok && have_total) ok = pc_draw_window_check(first, count, n_draw, total, &bad);
	snprintf(why, why_len, "%s", bad.c_str());
	return ok ? 0 : -2;
}

}

#ifdef DRAW_HOST_MAIN
/* every function of the host part once, on values that reach its branches and the ends of its ranges; what needs no big integers is
 * checked here: t_k < T, t_k does not decrease, K inverts it */
int main(void)
{
	int failures = 0;
	const uint64_t Ts[] = { 1, 0xffffffffull, 1ull << 32, (1ull << 32) + 1, 1ull << 63, 0xffffffffull << 32 };
	const uint64_t Ns[] = { 1, 2, 3, 65537, 0x7fffffffull };
	const uint32_t phases[] = { 0u, 1u, 0x80000000u, 0xffffffffu };
	for (uint64_t T : Ts)
		for (uint64_t N : Ns)
			for (uint32_t r : phases) {
				const uint64_t ks[] = { 0, N > 1 ? 1 : 0, N/2, N - 1 };
				uint64_t t[4];
				draw_thresholds(4, ks, r, T, N, t);
				for (int j = 0; j < 4; j++) {
					if (t[j] >= T) failures++;
					if (j && t[j] < t[j - 1]) failures++;
					/* K(t_k) <= k < K(t_k + 1) */
					const uint64_t cs[] = { t[j], t[j] + 1 };
					uint64_t K[2];
					draw_belows(2, cs, r, T, N, K);
					if (!(K[0] <= ks[j] && ks[j] < K[1])) failures++;
				}
				const uint64_t ends[] = { 0, T };
				uint64_t K[2];
				draw_belows(2, ends, r, T, N, K);
				if (K[0] != 0 || K[1] != N) failures++;
				uint64_t a, b;
				draw_range(0, T, r, T, N, 0, N, &a, &b);
				if (a != 0 || b != N) failures++;
				draw_range(0, T, r, T, N, N/2, 1, &a, &b);
				if (a != N/2 || b != N/2 + 1) failures++;
				draw_range(T, T, r, T, N, 0, N, &a, &b);
				if (a != b) failures++;
			}
	uint64_t lo, hi;
	draw_mul64(~0ull, ~0ull, &lo, &hi);
	if (lo != 1ull || hi != ~0ull - 1) failures++;
	draw_mul64(0x7fffffffffffffffull, 0xffffffff00000000ull, &lo, &hi);
	if (lo != 0x0000000100000000ull || hi != 0x7fffffff7fffffffull) failures++;
	char why[256];
	if (draw_check(1, 0, 0, 1, 1, 0, 0, 0, 0, 0, why, sizeof why) != 0 || why[0]) failures++;
	if (draw_check(1, 2, 11, 12, 0x7fffffff, 0x7fffffff - 100, 100, 1, 1, 5, why, sizeof why) != 0) failures++;
	if (draw_check(0, 0, 0, 1, 1, 0, 1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "select")) failures++;
	if (draw_check(1, 3, 0, 1, 1, 0, 1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "kind")) failures++;
	if (draw_check(1, 0, 1, 1, 1, 0, 1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "energy")) failures++;
	if (draw_check(1, 0, -1, 1, 1, 0, 1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "energy")) failures++;
	if (draw_check(1, 0, 0, 1, 0, 0, 0, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "n_draw")) failures++;
	if (draw_check(1, 0, 0, 1, 0x80000000ll, 0, 1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "n_draw")) failures++;
	if (draw_check(1, 0, 0, 1, 5, -1, 1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "first")) failures++;
	if (draw_check(1, 0, 0, 1, 5, 0, -1, 1, 0, 0, why, sizeof why) != -2 || !strstr(why, "count")) failures++;
	if (draw_check(1, 0, 0, 1, 5, 0, 1, 0, 0, 0, why, sizeof why) != -2 || !strstr(why, "records")) failures++;
	if (draw_check(1, 0, 0, 1, 5, 3, 3, 1, 1, 9, why, sizeof why) != -2 || !strstr(why, "n_draw")) failures++;
	if (draw_check(1, 0, 0, 1, 5, INT64_MAX, INT64_MAX, 1, 1, 9, why, sizeof why) != -2) failures++;
	if (draw_check(1, 0, 0, 1, 5, 0, 5, 1, 1, 0, why, sizeof why) != -2 || !strstr(why, "total")) failures++;
	printf("draw_host: %d failures\n", failures);
	return failures ? 1 : 0;
}
#endif

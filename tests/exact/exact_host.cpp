/* pc_exact.h compiled for the host: what tests/test_exact_cpu.py calls (tests/exact/pyexact.py builds it as a shared library).  With
 * -DEXACT_HOST_MAIN it is a program that walks the same ground, for a run under -fsanitize=address,undefined:
 *     g++ -std=c++17 -g -fsanitize=address,undefined -DEXACT_HOST_MAIN -I polycap_amd/csrc/hip tests/exact/exact_host.cpp -o exact_host && ./exact_host */
#include "pc_exact.h"

#include <cstdint>
#include <cstdio>

extern "C" {

/* long doubles leave as %La strings: exact, and no ctypes long double is needed */
void exact_value_hex(uint64_t lo, uint64_t hi, char *buf, int n) { snprintf(buf, (size_t)n, "%La", pc_exact_value(lo, hi)); }
void exact_scales_hex(char *buf, int n) { snprintf(buf, (size_t)n, "%La %La %La", PC_EXACT_2P32, PC_EXACT_2P62, PC_EXACT_2P64); }

void exact_add(uint64_t lo, uint64_t hi, uint64_t add_lo, uint64_t add_hi, uint64_t *out)
{
	const pc_exact_pair s = pc_exact_add(lo, hi, add_lo, add_hi);
	out[0] = s.lo; out[1] = s.hi;
}

void exact_add_pairs(uint64_t *acc, const uint64_t *part, size_t n) { pc_exact_add_pairs(acc, part, n); }

void exact_split(uint64_t lo, uint64_t hi, int64_t *limb)
{
	long long l[4];
	pc_exact_split(lo, hi, l);
	for (int k = 0; k < 4; k++) limb[k] = l[k];
}

void exact_join(const int64_t *limb, uint64_t *out)
{
	const long long l[4] = { limb[0], limb[1], limb[2], limb[3] };
	const pc_exact_pair s = pc_exact_join(l);
	out[0] = s.lo; out[1] = s.hi;
}

/* the standard error of an efficiency from its exact sums A, B (units of 2^-62) over n started photons */
double exact_stderr(uint64_t a_lo, uint64_t a_hi, uint64_t b_lo, uint64_t b_hi, int64_t n_started)
{
	const long double n = (long double)n_started;
	return pc_exact_stderr(pc_exact_value(a_lo, a_hi) / (n * PC_EXACT_2P62), pc_exact_value(b_lo, b_hi) / (n * PC_EXACT_2P62), n);
}

}

#ifdef EXACT_HOST_MAIN
#include <cstdlib>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "exact_host: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

typedef unsigned __int128 u128;

static u128 of(pc_exact_pair p) { return ((u128)p.hi << 64) | p.lo; }

int main(void)
{
	const uint64_t top = ~0ull;
	CHECK(pc_exact_value(0, 0) == 0.0L && pc_exact_value(top, 0) == 18446744073709551615.0L && pc_exact_value(0, 1) == PC_EXACT_2P64);
	CHECK(pc_exact_value(0, 1ull << 62) == PC_EXACT_2P64*PC_EXACT_2P62 && PC_EXACT_2P32*PC_EXACT_2P32 == PC_EXACT_2P64 && PC_EXACT_2P62*4.0L == PC_EXACT_2P64);
	/* adds: carries across lo, and modulo 2^128 */
	uint64_t x = 88172645463325252ull;
	auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
	const uint64_t edge[6] = { 0, 1, top, top - 1, 1ull << 63, (1ull << 32) - 1 };
	for (int k = 0; k < 20000; k++) {
		uint64_t v[4];
		for (uint64_t &w : v) w = (next() % 3) ? next() : edge[next() % 6];
		const u128 a = ((u128)v[1] << 64) | v[0], b = ((u128)v[3] << 64) | v[2];
		CHECK(of(pc_exact_add(v[0], v[1], v[2], v[3])) == (u128)(a + b));
		long long l[4];
		pc_exact_split(v[0], v[1], l);
		for (long long q : l) CHECK(q >= 0 && q < (1ll << 32));
		CHECK(of(pc_exact_join(l)) == a);
	}
	CHECK(of(pc_exact_add(top, top, 1, 0)) == 0);
	/* 64 members' limbs, summed: every limb sum stays below 2^38, and the join is the integer sum mod 2^128 */
	for (int round = 0; round < 200; round++) {
		long long sum[4] = { 0, 0, 0, 0 };
		u128 want = 0;
		for (int m = 0; m < 64; m++) {
			const uint64_t lo = (round & 1) ? top : next(), hi = (round & 2) ? top : next() >> (round % 40);
			long long l[4];
			pc_exact_split(lo, hi, l);
			for (int q = 0; q < 4; q++) sum[q] += l[q];
			want += ((u128)hi << 64) | lo;
		}
		for (long long q : sum) CHECK(q >= 0 && q < (1ll << 38));
		CHECK(of(pc_exact_join(sum)) == want);
	}
	{
		uint64_t acc[6] = { top, 0, top, top, 5, 7 };
		const uint64_t part[6] = { 1, 0, 1, 0, 6, 8 };
		pc_exact_add_pairs(acc, part, 3);
		CHECK(acc[0] == 0 && acc[1] == 1 && acc[2] == 0 && acc[3] == 0 && acc[4] == 11 && acc[5] == 15);
	}
	/* the tail: every weight 1/2 gives variance 0 exactly; the clamp; a Bernoulli sample */
	CHECK(exact_stderr(1ull << 63, 0, 1ull << 62, 0, 4) == 0.);                       /* 4 photons of weight 1/2: A = 4 2^61, B = 4 2^60 */
	CHECK(exact_stderr(1ull << 63, 0, 0, 0, 4) == 0.);                                /* q < m^2: clamped */
	const double s = exact_stderr(0, 1, 0, 1, 16);                                    /* 4 of 16 photons with weight 1: sqrt(3/16 / 15) */
	CHECK(s > 0.1118033988749 && s < 0.1118033988750);
	puts("exact_host: ok");
	return 0;
}
#endif

/*
 * pc_exact.h -- the arithmetic of exact sums, once.  A sum is an unsigned 128-bit integer kept as a (lo, hi) pair of uint64: the
 * weights' in units of 2^-62 (floor(w 2^62) per photon), the tallies' squares in units of 2^-64, their cells in units of 2^-32.
 * Here: the pair's value as long double and the three scales, the exact add, the four 32-bit limbs a device group all-reduces,
 * and the tail every standard error ends with.  The formulas of include/polycap-hip.h are made of these in the order written there.
 *
 * The common subset of C11 and C++17, nothing of HIP: the host C sources include it as well as the kernels' translation unit, where
 * the integer functions (PC_EXACT_FN) are callable from device code too.
 */
#ifndef PC_EXACT_H
#define PC_EXACT_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PC_EXACT_FN static inline __host__ __device__
#else
#define PC_EXACT_FN static inline
#endif

#define PC_EXACT_2P32 4294967296.0L
#define PC_EXACT_2P62 4611686018427387904.0L
#define PC_EXACT_2P64 18446744073709551616.0L

typedef struct { uint64_t lo, hi; } pc_exact_pair;

/* hi 2^64 + lo, rounded once where the sum has more than 64 significant bits */
static inline long double pc_exact_value(uint64_t lo, uint64_t hi)
{
	return (long double)hi * PC_EXACT_2P64 + (long double)lo;
}

/* (lo, hi) + (add_lo, add_hi) mod 2^128: unsigned, and so two's complement signed as well.  The one definition of the carry. */
PC_EXACT_FN pc_exact_pair pc_exact_add(uint64_t lo, uint64_t hi, uint64_t add_lo, uint64_t add_hi)
{
	pc_exact_pair s;
	s.lo = lo + add_lo;
	s.hi = hi + (add_hi + (s.lo < lo ? 1u : 0u));
	return s;
}

/* acc[2k], acc[2k + 1] += part[2k], part[2k + 1] for n pairs */
static inline void pc_exact_add_pairs(uint64_t *acc, const uint64_t *part, size_t n)
{
	for (size_t k = 0; k < n; k++) {
		const pc_exact_pair s = pc_exact_add(acc[2*k], acc[2*k + 1], part[2*k], part[2*k + 1]);
		acc[2*k] = s.lo; acc[2*k + 1] = s.hi;
	}
}

/* A pair as four 32-bit limbs, least significant first, in int64: limbs of up to 2^31 members add without overflow (64 members
 * stay below 2^38), so an integer all-reduce of the limbs is the exact sum. */
PC_EXACT_FN void pc_exact_split(uint64_t lo, uint64_t hi, long long limb[4])
{
	limb[0] = (long long)(lo & 0xffffffffull);
	limb[1] = (long long)(lo >> 32);
	limb[2] = (long long)(hi & 0xffffffffull);
	limb[3] = (long long)(hi >> 32);
}

/* sum of limb[l] 2^(32 l) mod 2^128, whatever the limbs have grown to */
PC_EXACT_FN pc_exact_pair pc_exact_join(const long long limb[4])
{
	const uint64_t l1 = (uint64_t)limb[1];
	return pc_exact_add((uint64_t)limb[0], (uint64_t)limb[2] + ((uint64_t)limb[3] << 32), l1 << 32, l1 >> 32);
}

/* standard error of a mean from the mean m and the mean square q of n >= 2 samples: sqrt(max(q - m^2, 0) / (n - 1)) */
static inline double pc_exact_stderr(long double m, long double q, long double n)
{
	long double v = q - m*m;
	if (v < 0.0L) v = 0.0L;
	return (double)sqrtl(v / (n - 1.0L));
}

#endif /* PC_EXACT_H */

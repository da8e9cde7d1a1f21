/* pc_moments.h -- the quantisation of the squared exit weights (option "weight_squares", include/polycap-hip.h), shared by every
 * kernel that sums them.  Compiles for the host as well (tests/test_stderr_cpu.py checks it against numpy). */
#ifndef PC_MOMENTS_H
#define PC_MOMENTS_H

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

/* (uint64)((w * w) * 2^62): one fp64 product, then the scaling, truncated like the weight's own (uint64)(w * 2^62).  The exit
 * weights lie in [0, 1], so the result does too and the conversion cannot overflow. */
static inline __host__ __device__ unsigned long long pc_fix_sq(double w)
{
	const double w2 = w*w;
	return (unsigned long long)(w2 * 4611686018427387904.0);
}

#endif /* PC_MOMENTS_H */

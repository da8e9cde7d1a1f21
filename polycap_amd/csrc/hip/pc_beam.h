/*
 * pc_beam.h -- exit-beam moments: the exact second-moment ("sigma") matrix of the photons of the last run, per energy, at the optic's
 * exit face (include/polycap-hip.h, pc_hip_beam_*).  A post-pass over the entries a spot map reads (pc_spot_source: exit photons as
 * image records or planes, the ordered leak event lists); nothing is uploaded and no trace kernel is involved.  Positions and slopes
 * are quantised to 2^-24 and weights to 2^-32; the 15 sums per (kind, energy) are signed 128-bit integers, so the result depends on
 * the set of entries only: not on launch shape, entry order, how the slots were split into runs, or the device count.  Focal
 * distance, waist size and divergence follow on the host in closed form (pc_hip_beam_params).
 *
 * The first part (the per-entry arithmetic and the host formulas) compiles for the host as well: -DPC_BEAM_HOST_ONLY stops the
 * header after it.
 */
#ifndef PC_BEAM_H
#define PC_BEAM_H

#include <math.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#define PC_BEAM_NSUMS 15          /* W, WX, WY, WU, WV, WXX, WXY, WXU, WXV, WYY, WYU, WYV, WUU, WUV, WVV */
#define PC_BEAM_NCOLS 26          /* columns of pc_hip_beam_params, named by PC_BEAM_COLUMNS */
#define PC_BEAM_NAT 5             /* columns of pc_hip_beam_at: x, y, size_x, size_y, size_r */
#define PC_BEAM_COLUMNS "weight,x,y,xp,yp,cov_xx,cov_xy,cov_xxp,cov_xyp,cov_yy,cov_yxp,cov_yyp,cov_xpxp,cov_xpyp,cov_ypyp," \
	"waist_x,waist_y,waist_r,size_waist_x,size_waist_y,size_waist_r,size_exit_x,size_exit_y,size_exit_r,div_x,div_y"

/* the quantised exit-face coordinates {X, Y, U, V} of one entry, and 1 when it is in range; 0 (q untouched) otherwise.  The contract
 * of include/polycap-hip.h, operation by operation (the library is built with -ffp-contract=off). */
static inline __host__ __device__ int pc_beam_entry(double x, double y, double z, double dx, double dy, double dz, double ze, long long q[4])
{
	const double t = (ze - z) / dz;
	const double xe = x + dx*t, ye = y + dy*t;
	const double sx = dx / dz, sy = dy / dz;
	const double r0 = rint(xe * 16777216.0), r1 = rint(ye * 16777216.0), r2 = rint(sx * 16777216.0), r3 = rint(sy * 16777216.0);
	if (!(dz > 0.) || !(fabs(r0) < 2147483648.0) || !(fabs(r1) < 2147483648.0) || !(fabs(r2) < 2147483648.0) || !(fabs(r3) < 2147483648.0))
		return 0;
	q[0] = (long long)r0; q[1] = (long long)r1; q[2] = (long long)r2; q[3] = (long long)r3;
	return 1;
}

/* ---- host formulas of the derived parameters.  A signed integer of 256 bits as four uint64 limbs, little end first (the
 * numerators need 192; two's complement throughout) */
struct pc_beam_i256 { uint64_t w[4]; };

static inline pc_beam_i256 pc_beam_from128(uint64_t lo, uint64_t hi)
{
	const uint64_t s = (hi >> 63) ? ~0ull : 0ull;
	pc_beam_i256 r = {{lo, hi, s, s}};
	return r;
}

static inline pc_beam_i256 pc_beam_neg(pc_beam_i256 a)
{
	uint64_t c = 1;
	for (int k = 0; k < 4; k++) {
		const uint64_t v = ~a.w[k] + c;
		c = (c && v == 0) ? 1 : 0;
		a.w[k] = v;
	}
	return a;
}

static inline pc_beam_i256 pc_beam_sub(pc_beam_i256 a, const pc_beam_i256 &b)
{
	uint64_t br = 0;
	for (int k = 0; k < 4; k++) {
		const uint64_t d = a.w[k] - b.w[k], d2 = d - br;
		br = (a.w[k] < b.w[k] || d < br) ? 1 : 0;
		a.w[k] = d2;
	}
	return a;
}

/* exact product of two signed 128-bit (lo, hi) values */
static inline pc_beam_i256 pc_beam_mul(const uint64_t *a, const uint64_t *b)
{
	pc_beam_i256 x = pc_beam_from128(a[0], a[1]), y = pc_beam_from128(b[0], b[1]);
	const int neg = (int)(x.w[3] >> 63) ^ (int)(y.w[3] >> 63);
	if (x.w[3] >> 63) x = pc_beam_neg(x);
	if (y.w[3] >> 63) y = pc_beam_neg(y);
	pc_beam_i256 r = {{0, 0, 0, 0}};
	for (int i = 0; i < 2; i++) {
		uint64_t c = 0;
		for (int j = 0; j < 2; j++) {
			const unsigned __int128 p = (unsigned __int128)x.w[i] * y.w[j] + r.w[i + j] + c;
			r.w[i + j] = (uint64_t)p;
			c = (uint64_t)(p >> 64);
		}
		r.w[i + 2] = c;
	}
	return neg ? pc_beam_neg(r) : r;
}

/* the nearest double (ties to even), as Python's float(int) */
static inline double pc_beam_to_double(pc_beam_i256 a)
{
	const int neg = (int)(a.w[3] >> 63);
	if (neg) a = pc_beam_neg(a);
	int top = 3;
	while (top > 0 && a.w[top] == 0) top--;
	const int n = top*64 + (a.w[top] ? 64 - __builtin_clzll(a.w[top]) : 0);       /* bit length */
	double d;
	if (n <= 64) {
		d = (double)a.w[0];
	} else {
		/* the top 64 bits, with every bit below them ORed into the last one (a sticky bit: rounding to 53 bits is unchanged) */
		const int k = n - 64, lw = k / 64, lb = k % 64;
		uint64_t m = lb ? (a.w[lw] >> lb) | (a.w[lw + 1] << (64 - lb)) : a.w[lw];
		uint64_t sticky = lb ? (a.w[lw] & ((1ull << lb) - 1)) : 0;
		for (int j = 0; j < lw; j++) sticky |= a.w[j];
		d = ldexp((double)(m | (sticky ? 1ull : 0ull)), k);
	}
	return neg ? -d : d;
}

/* one row of pc_hip_beam_params from the 15 (lo, hi) sums of one energy: the formulas of include/polycap-hip.h in their order */
static inline void pc_beam_params_row(const uint64_t *s, double *row)
{
	const double nan_ = NAN;
	const pc_beam_i256 S = pc_beam_from128(s[0], s[1]);
	const double sw = pc_beam_to_double(S);
	row[0] = sw * 0x1p-32;
	if (!(sw > 0.)) {
		for (int k = 1; k < PC_BEAM_NCOLS; k++) row[k] = nan_;
		return;
	}
	for (int a = 0; a < 4; a++)
		row[1 + a] = (pc_beam_to_double(pc_beam_from128(s[2*(1 + a)], s[2*(1 + a) + 1])) / sw) * 0x1p-24;
	const double ss = sw * sw;
	int k = 5;
	for (int a = 0; a < 4; a++)
		for (int b = a; b < 4; b++, k++) {
			/* N_ab = S * S_ab - S_a * S_b, exact */
			const pc_beam_i256 n = pc_beam_sub(pc_beam_mul(s, s + 2*k), pc_beam_mul(s + 2*(1 + a), s + 2*(1 + b)));
			row[k] = (pc_beam_to_double(n) / ss) * 0x1p-48;
		}
	const double cxx = row[5], cxu = row[7], cyy = row[9], cyv = row[11], cuu = row[12], cvv = row[14];
	const double b_r = cxu + cyv, d_r = cuu + cvv;
	row[15] = (cuu != 0.) ? -cxu / cuu : nan_;
	row[16] = (cvv != 0.) ? -cyv / cvv : nan_;
	row[17] = (d_r != 0.) ? -b_r / d_r : nan_;
	row[18] = (cuu != 0.) ? sqrt(fmax(cxx - (cxu*cxu) / cuu, 0.)) : nan_;
	row[19] = (cvv != 0.) ? sqrt(fmax(cyy - (cyv*cyv) / cvv, 0.)) : nan_;
	row[20] = (d_r != 0.) ? sqrt(fmax((cxx + cyy) - (b_r*b_r) / d_r, 0.)) : nan_;
	row[21] = sqrt(cxx);
	row[22] = sqrt(cyy);
	row[23] = sqrt(cxx + cyy);
	row[24] = sqrt(cuu);
	row[25] = sqrt(cvv);
}

/* centroid and RMS size at distance d behind the exit face from a row of pc_beam_params_row: {x, y, size_x, size_y, size_r} */
static inline void pc_beam_at_row(const double *row, double d, double *out)
{
	const double vx = (row[5] + (2.*d)*row[7]) + (d*d)*row[12];
	const double vy = (row[9] + (2.*d)*row[11]) + (d*d)*row[14];
	const double px = fmax(vx, 0.), py = fmax(vy, 0.);
	out[0] = row[1] + d*row[3];
	out[1] = row[2] + d*row[4];
	out[2] = sqrt(px);
	out[3] = sqrt(py);
	out[4] = sqrt(px + py);
	if (!(row[0] > 0.))
		for (int k = 0; k < PC_BEAM_NAT; k++) out[k] = NAN;
}

#ifndef PC_BEAM_HOST_ONLY

/* W * P as a signed 128-bit value added to (lo, hi): the unsigned product W * |P| (low and high halves), negated for P < 0 */
static __device__ __forceinline__ void pc_beam_mac(unsigned long long &lo, unsigned long long &hi, unsigned long long w, long long p)
{
	const unsigned long long a = (p < 0) ? 0ull - (unsigned long long)p : (unsigned long long)p;
	unsigned long long pl = w*a, ph = __umul64hi(w, a);
	if (p < 0) {
		pl = ~pl + 1ull;
		ph = ~ph + (pl == 0ull ? 1ull : 0ull);
	}
	pc_add128(lo, hi, pl, ph);
}

/* The sums [energy][16][2]: the 15 signed (lo, hi) sums, then the outside counter as (lo, 0).
 *
 * Workgroup (x, c) does energies [64c, 64c + 64) of the entries x, x + gridDim.x, ... .  As in pc_spot_wide_kernel the lanes of a
 * wave take the energies of one entry (gw = the next power of two above the chunk's energy count; 64 / gw entries per wave), so
 * that every lane keeps one energy for the whole pass and accumulates its 15 sums in registers over all its entries.  At the end
 * the lanes of one energy are summed across the wave (shuffles), the waves in LDS, and the workgroup adds its sums to the global
 * ones with one 128-bit atomic per sum: one set per workgroup and energy, not per entry. */
#define PC_BEAM_BLOCK 256
#define PC_BEAM_SLOTS 16
template <bool M>      /* M: a gated add, s.mask is set (pc_select.h); the plain build reads no mask */
__global__ void __launch_bounds__(PC_BEAM_BLOCK) pc_beam_kernel(pc_spot_src s, double ze, int ne, unsigned long long *sums)
{
	__shared__ unsigned long long red[64*PC_BEAM_SLOTS*2];
	const int e0 = blockIdx.y*64;
	const int en = (ne - e0 < 64) ? ne - e0 : 64;
	for (int k = threadIdx.x; k < 64*PC_BEAM_SLOTS*2; k += blockDim.x) red[k] = 0ull;
	__syncthreads();
	const pc_tally_lanes l = pc_tally_lane_map(en);
	unsigned long long acc[PC_BEAM_SLOTS][2];
#pragma unroll
	for (int k = 0; k < PC_BEAM_SLOTS; k++) acc[k][0] = acc[k][1] = 0ull;
	const int e = e0 + l.sub;
	for (long long i = (l.sub < en) ? l.first : s.n; i < s.n; i += l.stride) {
		if (M && !s.mask[i]) continue;      /* gated add: the entry does not exist */
		const unsigned long long w = pc_spot_q(s.w[i*s.ws + e]);
		if (!w) continue;
		const pc_entry t = pc_entry_load(s, i);
		long long q[4];
		if (!pc_beam_entry(t.x, t.y, t.z, t.dx, t.dy, t.dz, ze, q)) {
			acc[15][0] += w;
			continue;
		}
		pc_beam_mac(acc[0][0], acc[0][1], w, 1);
#pragma unroll
		for (int a = 0; a < 4; a++) pc_beam_mac(acc[1 + a][0], acc[1 + a][1], w, q[a]);
		int k = 5;
#pragma unroll
		for (int a = 0; a < 4; a++)
#pragma unroll
			for (int b = a; b < 4; b++, k++) pc_beam_mac(acc[k][0], acc[k][1], w, q[a]*q[b]);
	}
	/* lanes lane ^ gw, lane ^ 2gw, ... have the same energy */
	for (int off = l.gw; off < 64; off <<= 1)
#pragma unroll
		for (int k = 0; k < PC_BEAM_SLOTS; k++) {
			const unsigned long long lo = __shfl_xor(acc[k][0], off), hi = __shfl_xor(acc[k][1], off);
			pc_add128(acc[k][0], acc[k][1], lo, hi);
		}
	if (l.lane < l.gw && l.sub < en)
#pragma unroll
		for (int k = 0; k < PC_BEAM_SLOTS; k++) {
			if (!(acc[k][0] | acc[k][1])) continue;
			unsigned long long *r = red + (l.sub*PC_BEAM_SLOTS + k)*2;
			const unsigned long long old = atomicAdd(&r[0], acc[k][0]);
			const unsigned long long c = (old + acc[k][0] < old) ? 1ull : 0ull;
			if (acc[k][1] + c) atomicAdd(&r[1], acc[k][1] + c);
		}
	__syncthreads();
	for (int k = threadIdx.x; k < en*PC_BEAM_SLOTS; k += blockDim.x) {
		const unsigned long long lo = red[2*k], hi = red[2*k + 1];
		if (lo | hi) pc_atomic_add128(sums + ((long long)e0*PC_BEAM_SLOTS + k)*2, lo, hi);
	}
}

/* cells [kind][energy][16][2] */
struct pc_hip_beam : pc_tally {
	int ne = 0;
	double ze = 0.;
};

static int pc_beam_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, pc_hip_beam **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_create: beam must not be NULL");
	*out = nullptr;
	const pc_hip_ctx *c0 = ctxs[0];
	pc_hip_beam *b = new pc_hip_beam();
	b->ne = c0->host.pm.n_energies;
	b->ze = c0->host.z[c0->host.pm.nmax];
	const int st = pc_tally_make(*b, ctxs, group, (size_t)3*b->ne*PC_BEAM_SLOTS*2, "pc_hip_beam_create");
	if (st) { delete b; return st; }
	*out = b;
	return PC_HIP_OK;
}

static int pc_beam_launch(pc_hip_beam *b, pc_tally_member &m, const pc_spot_src &s, int kind)
{
	pc_hip_ctx *c = m.ctx;
	const long long chunks = (b->ne + 63) / 64;
	const long long bx = pc_tally_grid_wide(c->n_cu, chunks, b->ne, s.n, PC_BEAM_BLOCK).bx;
	unsigned long long *sums = m.d_cells + (size_t)kind*b->ne*PC_BEAM_SLOTS*2;
	auto kern = s.mask ? pc_beam_kernel<true> : pc_beam_kernel<false>;
	hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)chunks), dim3(PC_BEAM_BLOCK), 0, c->stream, s, b->ze, b->ne, sums);
	return PC_HIP_OK;
}

extern "C" {

int pc_hip_beam_create(pc_hip_ctx *ctx, pc_hip_beam **beam)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_create: ctx must not be NULL");
	return pc_beam_make(std::vector<pc_hip_ctx *>{ctx}, nullptr, beam);
}

int pc_hip_group_beam_create(pc_hip_group *group, pc_hip_beam **beam)
{
	if (!group) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_beam_create: group must not be NULL");
	return pc_beam_make(group->ctx, group, beam);
}

void pc_hip_beam_destroy(pc_hip_beam *beam)
{
	delete beam;
}

int pc_hip_beam_add(pc_hip_beam *beam, int kind)
{
	if (!beam) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_add: beam must not be NULL");
	return pc_tally_add(*beam, kind, "pc_hip_beam_add",
		[beam](size_t k, const pc_spot_src &s, int kd) { return pc_beam_launch(beam, beam->m[k], s, kd); });
}

int pc_hip_beam_read(pc_hip_beam *beam, uint64_t *sums, uint64_t *outside, int64_t *n_entries)
{
	if (!beam) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_read: beam must not be NULL");
	std::vector<unsigned long long> sum;
	const int st = pc_tally_sum(*beam, 2, sum);      /* 128-bit two's complement */
	if (st) return st;
	const size_t rows = (size_t)3*beam->ne;
	for (size_t r = 0; r < rows; r++) {
		const unsigned long long *q = sum.data() + r*PC_BEAM_SLOTS*2;
		if (sums) memcpy(sums + r*PC_BEAM_NSUMS*2, q, PC_BEAM_NSUMS*2*sizeof(uint64_t));
		if (outside) outside[r] = q[PC_BEAM_NSUMS*2];
	}
	if (n_entries)
		for (int k = 0; k < 3; k++) n_entries[k] = beam->n_entries[k];
	return PC_HIP_OK;
}

int pc_hip_beam_reset(pc_hip_beam *beam)
{
	if (!beam) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_reset: beam must not be NULL");
	return pc_tally_reset(*beam);
}

int pc_hip_beam_info(const pc_hip_beam *beam, int *n_energies)
{
	if (!beam || !n_energies) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_info: NULL argument");
	*n_energies = beam->ne;
	return PC_HIP_OK;
}

void pc_hip_beam_params(size_t n_energies, const uint64_t *sums, double *params)
{
	for (size_t e = 0; e < n_energies; e++)
		pc_beam_params_row(sums + e*PC_BEAM_NSUMS*2, params + e*PC_BEAM_NCOLS);
}

void pc_hip_beam_at(size_t n_energies, const uint64_t *sums, size_t n_distances, const double *distances, double *out)
{
	double row[PC_BEAM_NCOLS];
	for (size_t e = 0; e < n_energies; e++) {
		pc_beam_params_row(sums + e*PC_BEAM_NSUMS*2, row);
		for (size_t k = 0; k < n_distances; k++)
			pc_beam_at_row(row, distances[k], out + (e*n_distances + k)*PC_BEAM_NAT);
	}
}

const char *pc_hip_beam_columns(void)
{
	return PC_BEAM_COLUMNS;
}

} /* extern "C" */

#endif /* PC_BEAM_HOST_ONLY */
#endif /* PC_BEAM_H */

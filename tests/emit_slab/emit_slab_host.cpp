/* The slab part of pc_emit.h (frame, spec check, per-entry arithmetic, exponential, weight and path of a slab emit) compiled for the
 * host alone: what tests/test_emit_slab_cpu.py checks against numpy and mpmath and what tests/test_gpu_emit_slab.py applies to fetched
 * records for the host round trip. */
#define PC_EMIT_HOST_ONLY
#include "pc_emit.h"

extern "C" {

/* in [n][4] = x, y, dx, dy; slots [n]; frame [20]; out [n][14], written where what [n] is PC_EMIT_INJECT (1); 3: missed the sample,
 * 4: missed the detector */
void slab_state_n(int64_t n, const double *in, const uint64_t *slots, const double *frame, double R, uint64_t seed, double *out, int32_t *what)
{
	for (int64_t i = 0; i < n; i++)
		what[i] = pc_emit_slab_state(in[4*i], in[4*i + 1], in[4*i + 2], in[4*i + 3], slots[i], frame, R, seed, out + PC_SLAB_N_STATE*i);
}

/* the same with the three uniforms given: u [n][3]; odd [n] */
void slab_at_n(int64_t n, const double *in, const int32_t *odd, const double *u, const double *frame, double R, double *out, int32_t *what)
{
	for (int64_t i = 0; i < n; i++)
		what[i] = pc_emit_slab_at(in[4*i], in[4*i + 1], in[4*i + 2], in[4*i + 3], odd[i], frame, R, u[3*i], u[3*i + 1], u[3*i + 2], out + PC_SLAB_N_STATE*i);
}

/* spec [8] in the order of pc_hip_emit */
void slab_frame(const double *spec, double thickness, double *frame) { pc_emit_slab_frame(spec, thickness, frame); }

int slab_bad(double thickness, int n_in, const double *mu_in, int n_out, const double *mu_out, int *at)
{
	return pc_emit_slab_bad(thickness, n_in, mu_in, n_out, mu_out, at);
}

void slab_exp_neg_n(int64_t n, const double *x, double *y)
{
	for (int64_t i = 0; i < n; i++) y[i] = pc_emit_exp_neg(x[i]);
}

void slab_weight_n(int64_t n, const double *wa, const double *gl, const double *mu_in, const double *s, const double *mu_out, const double *s_out,
	const double *wb, double *w)
{
	for (int64_t i = 0; i < n; i++) w[i] = pc_emit_slab_weight(wa[i], gl[i], mu_in[i], s[i], mu_out[i], s_out[i], wb[i]);
}

void slab_dtravel_n(int64_t n, const double *da, const double *t, const double *s, const double *r, const double *db, double *out)
{
	for (int64_t i = 0; i < n; i++) out[i] = pc_emit_slab_dtravel(da[i], t[i], s[i], r[i], db[i]);
}

}

/* The first part of pc_emit.h (the frame, the spec check and the per-entry arithmetic of an emit relay) compiled for the host alone:
 * what tests/test_emit_cpu.py checks against numpy and mpmath and what tests/test_gpu_emit.py applies to fetched records for the host
 * round trip. */
#define PC_EMIT_HOST_ONLY
#include "pc_emit.h"

extern "C" {

/* in [n][4] = x, y, dx, dy; slots [n]; frame [16]; out [n][12], written where what [n] is PC_EMIT_INJECT (1); 3: missed the
 * sample, 4: missed the detector */
void emit_state_n(int64_t n, const double *in, const uint64_t *slots, const double *frame, double R, uint64_t seed, double *out, int32_t *what)
{
	for (int64_t i = 0; i < n; i++)
		what[i] = pc_emit_state(in[4*i], in[4*i + 1], in[4*i + 2], in[4*i + 3], slots[i], frame, R, seed, out + 12*i);
}

/* spec [8] in the order of pc_hip_emit */
void emit_frame(const double *spec, double *frame) { pc_emit_frame(spec, frame); }

int emit_spec_bad(const double *spec) { return pc_emit_spec_bad(spec); }

const char *emit_field_name(int k) { return pc_emit_field_name(k); }

void emit_finish_n(int64_t n, const double *wa, const double *g, const double *wb, double *w)
{
	for (int64_t i = 0; i < n; i++) w[i] = pc_emit_weight(wa[i], g[i], wb[i]);
}

void emit_dtravel_n(int64_t n, const double *da, const double *t, const double *r, const double *db, double *out)
{
	for (int64_t i = 0; i < n; i++) out[i] = pc_emit_dtravel(da[i], t[i], r[i], db[i]);
}

}

/* The per-photon arithmetic of pc_relay.h compiled for the host alone: what tests/test_relay_cpu.py checks against numpy and what
 * tests/test_gpu_relay.py applies to fetched records for the host round trip. */
#define PC_RELAY_HOST_ONLY
#include "pc_relay.h"
#include "pc_moments.h"

extern "C" {

/* in [n][6] = x, y, dx, dy, ex, ey; out [n][10] */
void relay_fly_n(int64_t n, const double *in, double gap, double off_x, double off_y, double *out)
{
	for (int64_t i = 0; i < n; i++)
		pc_relay_fly(in[6*i], in[6*i + 1], in[6*i + 2], in[6*i + 3], in[6*i + 4], in[6*i + 5], gap, off_x, off_y, out + 10*i);
}

void relay_valid_n(int64_t n, const double *exit_z, const double *w0, int32_t *out)
{
	for (int64_t i = 0; i < n; i++) out[i] = pc_relay_entry_valid(exit_z[i], w0[i]);
}

/* w = wa * wb and what it adds to the two exact sums */
void relay_finish_n(int64_t n, const double *wa, const double *wb, double *w, uint64_t *a, uint64_t *b)
{
	for (int64_t i = 0; i < n; i++) {
		w[i] = pc_relay_weight(wa[i], wb[i]);
		a[i] = pc_relay_fix(w[i]);
		b[i] = pc_fix_sq(w[i]);
	}
}

void relay_dtravel_n(int64_t n, const double *da, const double *t, const double *db, double *out)
{
	for (int64_t i = 0; i < n; i++) out[i] = pc_relay_dtravel(da[i], t[i], db[i]);
}

int relay_placement_ok(double gap, double off_x, double off_y) { return pc_relay_placement_ok(gap, off_x, off_y); }

double relay_efficiency(uint64_t lo, uint64_t hi, int64_t n_started) { return pc_relay_efficiency(lo, hi, n_started); }

}

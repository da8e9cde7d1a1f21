/* The host+device part of pc_emit_layers.h (bounds, prefix tables, spec check, frame, per-entry arithmetic, optical depths, weight
 * and path of a layered emit) compiled for the host alone: what tests/test_emit_layers_cpu.py checks against numpy and exact
 * fractions and what tests/test_gpu_emit_layers.py applies to fetched records for the host round trip. */
#define PC_EMIT_HOST_ONLY
#include "pc_emit_layers.h"

extern "C" {

/* in [n][4] = x, y, dx, dy; slots [n]; frame [21]; Z [nl + 1]; out [n][18], written where what [n] is PC_EMIT_INJECT (1) */
void layers_state_n(int64_t n, const double *in, const uint64_t *slots, const double *frame, double R, int nl, const double *Z, uint64_t seed,
	double *out, int32_t *what)
{
	for (int64_t i = 0; i < n; i++)
		what[i] = pc_emit_layers_state(in[4*i], in[4*i + 1], in[4*i + 2], in[4*i + 3], slots[i], frame, R, nl, Z, seed, out + PC_LAYERS_N_STATE*i);
}

/* the same with the three uniforms given: u [n][3]; odd [n] */
void layers_at_n(int64_t n, const double *in, const int32_t *odd, const double *u, const double *frame, double R, int nl, const double *Z,
	double *out, int32_t *what)
{
	for (int64_t i = 0; i < n; i++)
		what[i] = pc_emit_layers_at(in[4*i], in[4*i + 1], in[4*i + 2], in[4*i + 3], odd[i], frame, R, nl, Z, u[3*i], u[3*i + 1], u[3*i + 2],
		                            out + PC_LAYERS_N_STATE*i);
}

void layers_bounds(int nl, const double *thickness, double *Z) { pc_emit_layers_bounds(nl, thickness, Z); }

/* spec [8] in the order of pc_hip_emit */
void layers_frame(const double *spec, double T, double qmax, double *frame) { pc_emit_layers_frame(spec, T, qmax, frame); }

double layers_qmax(int nl, int n_out, const double *production) { return pc_emit_layers_qmax(nl, n_out, production); }

void layers_tables(int nl, const double *thickness, int n_in, const double *mu_in, int n_out, const double *mu_out, double *pin, double *pout,
	double *sout)
{
	pc_emit_layers_tables(nl, thickness, n_in, mu_in, n_out, mu_out, pin, pout, sout);
}

int layers_bad(int nl, const double *thickness, int n_in, const double *mu_in, int n_out, const double *mu_out, const double *production,
	int *layer, int *at)
{
	return pc_emit_layers_bad(nl, thickness, n_in, mu_in, n_out, mu_out, production, layer, at);
}

/* per photon i: state [n][18]; wa, wb [n]; the tables as the library lays them out, mu_in and pin [nl][n_in], the others [nl][n_out];
 * ea, e: the energy of the first and of the second optic.  w [n] */
void layers_weight_n(int64_t n, const double *state, const double *wa, const double *wb, int n_in, int ea, int n_out, int e, const double *pin,
	const double *mu_in, const double *sout, const double *pout, const double *mu_out, const double *prod, double *w)
{
	for (int64_t i = 0; i < n; i++) {
		const double *o = state + PC_LAYERS_N_STATE*i;
		const long long j = (long long)o[PC_LAYERS_J];
		w[i] = pc_emit_layers_weight_at(o, wa[i], pin, mu_in, j*n_in + ea, sout, pout, mu_out, prod, j*n_out + e, wb[i]);
	}
}

/* the optical depth and the weight alone, elementwise */
void layers_tau_n(int64_t n, const double *acc, const double *mu, const double *x, const double *c, double *tau)
{
	for (int64_t i = 0; i < n; i++) tau[i] = pc_emit_layers_tau(acc[i], mu[i], x[i], c[i]);
}

void layers_w_n(int64_t n, const double *wa, const double *gl, const double *q, const double *tau_in, const double *tau_out, const double *wb, double *w)
{
	for (int64_t i = 0; i < n; i++) w[i] = pc_emit_layers_weight(wa[i], gl[i], q[i], tau_in[i], tau_out[i], wb[i]);
}

void layers_dtravel_n(int64_t n, const double *da, const double *t, const double *s, const double *r, const double *db, double *out)
{
	for (int64_t i = 0; i < n; i++) out[i] = pc_emit_layers_dtravel(da[i], t[i], s[i], r[i], db[i]);
}

}

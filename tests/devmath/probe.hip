/*
 * probe.hip -- TEST-ONLY: the arithmetic of pc_device.h on the device, element by element (tests/test_gpu_devmath.py).
 *
 * One kernel per primitive or Fresnel form (pc_probe_eval<OP>, tests/devmath/probe_ops.h); the per-energy constants come from
 * the product's own setup (pc_build_tables, pc_problem.h) of the problem passed in.  Op MARCH (tests/test_gpu_devmath_march.py) runs
 * one photon per thread through pc_launch_init, pc_march_step and pc_event_pre on the problem's whole profile, tables in global
 * memory.  Ops WALL, OUTER and HEX (tests/test_gpu_devmath_leak.py) run the wall search of pc_leak.h the same way; op FLIGHTS
 * (tests/test_gpu_devmath_flights.py) is op MARCH carried on through the reflections (pc_event_post).  Ops SINCOS, UNIFORM, ENTER and EXIT
 * (tests/test_gpu_devmath_ends.py) are the two ends of a photon's life: the sampler's sine / cosine and random stream, pc_launch_init
 * and pc_in_exit_window.  Built by tests/devmath/pyprobe.py with the library's flags (polycap_amd._build.HIPFLAGS) into
 * tests/devmath/libpc_probe.so; never part of libpolycap.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pc_problem.h"
#include "probe_ops.h"

namespace {

template <int OP>
__global__ void __launch_bounds__(256) pc_probe_kernel(int64_t n_groups, const pc_energy_const *__restrict__ ec,
                                                       const int32_t *__restrict__ e, const double *__restrict__ in,
                                                       double *__restrict__ out, int32_t *__restrict__ code)
{
	constexpr int G = (OP == PC_PROBE_F3X2) ? 2 : 1;
	const int64_t t = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (t >= n_groups) return;
	const int64_t i = t*G;
	int cd[G];
	double o[2*G];
	pc_probe_eval<OP>(ec[e[i]], in + i*PC_PROBE_IN, o, cd);
	for (int j = 0; j < G; j++) {
		out[2*(i + j)] = o[2*j]; out[2*(i + j) + 1] = o[2*j + 1];
		code[i + j] = cd[j];
	}
}

template <int OP>
void launch(int64_t n_groups, const pc_energy_const *ec, const int32_t *e, const double *in, double *out, int32_t *code)
{
	const unsigned blocks = (unsigned)((n_groups + 255)/256);
	hipLaunchKernelGGL(pc_probe_kernel<OP>, dim3(blocks), dim3(256), 0, 0, n_groups, ec, e, in, out, code);
}

typedef void (*launch_fn)(int64_t, const pc_energy_const *, const int32_t *, const double *, double *, int32_t *);
const launch_fn LAUNCH[PC_PROBE_NOPS] = {
	launch<0>, launch<1>, launch<2>, launch<3>, launch<4>, launch<5>, launch<6>, launch<7>, launch<8>, launch<9>, launch<10>,
	launch<11>, launch<12>};

/* one thread per element of a geometry op; an element whose profile the setup rejected (code preset on the host) is left alone */
template <int OP>
__global__ void __launch_bounds__(256) pc_probe_geom_kernel(int64_t n, const pc_energy_const *__restrict__ ec,
                                                            const int32_t *__restrict__ e, const double *__restrict__ in,
                                                            const double *__restrict__ tab, double *__restrict__ out,
                                                            int32_t *__restrict__ code)
{
	constexpr int WI = (OP == PC_PROBE_SEGMENT) ? PC_PROBE_SEG_IN : PC_PROBE_VEC_IN;
	const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (code[i] == PC_PROBE_SETUP_REJECT) return;
	double o[PC_PROBE_GEOM_OUT];
	int cd = 0;
	pc_probe_geom_eval<OP>(ec[e[i]], in + i*WI, (OP == PC_PROBE_SEGMENT) ? tab + i*PC_PROBE_SEG_TAB : nullptr, o, &cd);
	for (int j = 0; j < PC_PROBE_GEOM_OUT; j++) out[i*PC_PROBE_GEOM_OUT + j] = o[j];
	code[i] = cd;
}

template <int OP>
void launch_geom(int64_t n, const pc_energy_const *ec, const int32_t *e, const double *in, const double *tab, double *out,
                 int32_t *code)
{
	const unsigned blocks = (unsigned)((n + 255)/256);
	hipLaunchKernelGGL(pc_probe_geom_kernel<OP>, dim3(blocks), dim3(256), 0, 0, n, ec, e, in, tab, out, code);
}

/* one thread per photon of a MARCH call; the profile tables lie in global memory */
__global__ void __launch_bounds__(64) pc_probe_march_kernel(int64_t n, pc_params pm, int nodes, const double *__restrict__ tab,
                                                            const pc_marg4 *__restrict__ mg, const double *__restrict__ in,
                                                            double *__restrict__ out, int32_t *__restrict__ code)
{
	const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	pc_tables T;
	pc_probe_march_tables(T, tab, mg, nodes);
	int cd = 0;
	pc_probe_march_eval(T, pm, in + i*PC_PROBE_MARCH_IN, out + i*PC_PROBE_MARCH_OUT, &cd);
	code[i] = cd;
}

/* one thread per photon of a FLIGHTS call; the profile tables lie in global memory */
__global__ void __launch_bounds__(64) pc_probe_flights_kernel(int64_t n, pc_params pm, int nodes, const double *__restrict__ tab,
                                                              const pc_marg4 *__restrict__ mg, const double *__restrict__ in,
                                                              double *__restrict__ out, int32_t *__restrict__ code)
{
	const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	pc_tables T;
	pc_probe_march_tables(T, tab, mg, nodes);
	int cd = 0;
	pc_probe_flights_eval(T, pm, in + i*PC_PROBE_FLIGHTS_IN, out + i*PC_PROBE_FLIGHTS_OUT, &cd);
	code[i] = cd;
}

/* one thread per row of a leak op (WALL, OUTER, HEX); the profile tables lie in global memory */
template <int OP>
__global__ void __launch_bounds__(64) pc_probe_leak_kernel(int64_t n, pc_params pm, int nodes, const double *__restrict__ tab,
                                                           const pc_marg4 *__restrict__ mg, const pc_drdev *__restrict__ dr,
                                                           const double *__restrict__ in, double *__restrict__ out,
                                                           int32_t *__restrict__ code)
{
	const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	pc_tables T;
	pc_probe_leak_tables(T, tab, mg, dr, nodes);
	int cd = 0;
	if constexpr (OP == PC_PROBE_WALL) pc_probe_wall_eval(T, pm, in + i*PC_PROBE_WALL_IN, out + i*PC_PROBE_WALL_OUT, &cd);
	else if constexpr (OP == PC_PROBE_OUTER) pc_probe_outer_eval(T, pm, in + i*PC_PROBE_OUTER_IN, out + i*PC_PROBE_OUTER_OUT, &cd);
	else pc_probe_hex_eval(in + i*PC_PROBE_HEX_IN, out + i*PC_PROBE_HEX_OUT, &cd);
	code[i] = cd;
}

/* a leak op on n rows of the whole profile of p: what the three entry points below share */
int run_leak(const pc_hip_problem *p, int op, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	err[0] = 0;
	pc_host_tables t;
	std::string msg;
	if (pc_build_tables(p, t, msg)) { snprintf(err, 256, "%s", msg.c_str()); return -2; }
	if (pc_probe_leak_check(p, op, n, in_w, out_w, in, PC_PROBE_WALL_UNITS_DEVICE)) { snprintf(err, 256, "invalid size, width or row (non-finite value, dz == 0, literal flag, hint, max_units, zz <= 0)"); return -2; }
	if (n == 0) return 0;
	const size_t nodes = (size_t)p->nmax + 1;
	std::vector<double> tab;
	tab.reserve(PC_PROBE_LEAK_TAB*nodes);
	const std::vector<double> *cols[PC_PROBE_LEAK_TAB] = {&t.z, &t.cap, &t.zh, &t.cap2, &t.hexd, &t.idz, &t.ext, &t.stp, &t.istp};
	for (int c = 0; c < PC_PROBE_LEAK_TAB; c++) tab.insert(tab.end(), cols[c]->begin(), cols[c]->end());
	int32_t *d_code = nullptr;
	double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
	pc_marg4 *d_mg = nullptr;
	pc_drdev *d_dr = nullptr;
	int rc = 0;
	hipError_t s = hipSuccess;
#define PC_PROBE_TRY(call) do { if (s == hipSuccess) { s = (call); if (s != hipSuccess) snprintf(err, 256, "%s: %s", #call, hipGetErrorString(s)); } } while (0)
	PC_PROBE_TRY(hipMalloc(&d_code, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_in, n*in_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_out, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_tab, tab.size()*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_mg, nodes*sizeof(pc_marg4)));
	PC_PROBE_TRY(hipMalloc(&d_dr, nodes*sizeof(pc_drdev)));
	PC_PROBE_TRY(hipMemset(d_code, 0, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMemset(d_out, 0, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMemcpy(d_in, in, n*in_w*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_tab, tab.data(), tab.size()*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_mg, t.mg.data(), nodes*sizeof(pc_marg4), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_dr, t.dr.data(), nodes*sizeof(pc_drdev), hipMemcpyHostToDevice));
	if (s == hipSuccess) {
		const dim3 blocks((unsigned)((n + 63)/64)), threads(64);
		if (op == PC_PROBE_WALL)
			hipLaunchKernelGGL(pc_probe_leak_kernel<PC_PROBE_WALL>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_dr, d_in, d_out, d_code);
		else if (op == PC_PROBE_OUTER)
			hipLaunchKernelGGL(pc_probe_leak_kernel<PC_PROBE_OUTER>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_dr, d_in, d_out, d_code);
		else
			hipLaunchKernelGGL(pc_probe_leak_kernel<PC_PROBE_HEX>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_dr, d_in, d_out, d_code);
		PC_PROBE_TRY(hipGetLastError());
	}
	PC_PROBE_TRY(hipDeviceSynchronize());
	PC_PROBE_TRY(hipMemcpy(out, d_out, n*out_w*sizeof(double), hipMemcpyDeviceToHost));
	PC_PROBE_TRY(hipMemcpy(code, d_code, n*sizeof(int32_t), hipMemcpyDeviceToHost));
	if (s != hipSuccess) rc = -3;
	const hipError_t f[6] = {hipFree(d_code), hipFree(d_in), hipFree(d_out), hipFree(d_tab), hipFree(d_mg), hipFree(d_dr)};
	for (int j = 0; j < 6 && rc == 0; j++)
		if (f[j] != hipSuccess) { snprintf(err, 256, "hipFree: %s", hipGetErrorString(f[j])); rc = -3; }
#undef PC_PROBE_TRY
	return rc;
}

/* op MARCH, or op FLIGHTS, on n photons through the whole profile of p: what their two entry points share */
int run_march(const pc_hip_problem *p, bool flights, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code,
              char *err)
{
	err[0] = 0;
	pc_host_tables t;
	std::string msg;
	if (pc_build_tables(p, t, msg)) { snprintf(err, 256, "%s", msg.c_str()); return -2; }
	if (flights ? pc_probe_flights_check(p, n, in_w, out_w, in) : pc_probe_march_check(p, n, in_w, out_w, in)) { snprintf(err, 256, "invalid size, width, profile, literal flag, K or NB"); return -2; }
	if (n == 0) return 0;
	const size_t nodes = (size_t)p->nmax + 1;
	std::vector<double> tab;
	tab.reserve(PC_PROBE_MARCH_TAB*nodes);
	const std::vector<double> *cols[PC_PROBE_MARCH_TAB] = {&t.z, &t.cap, &t.zh, &t.cap2, &t.hexd, &t.idz, &t.ext};
	for (int c = 0; c < PC_PROBE_MARCH_TAB; c++) tab.insert(tab.end(), cols[c]->begin(), cols[c]->end());
	int32_t *d_code = nullptr;
	double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
	pc_marg4 *d_mg = nullptr;
	int rc = 0;
	hipError_t s = hipSuccess;
#define PC_PROBE_TRY(call) do { if (s == hipSuccess) { s = (call); if (s != hipSuccess) snprintf(err, 256, "%s: %s", #call, hipGetErrorString(s)); } } while (0)
	PC_PROBE_TRY(hipMalloc(&d_code, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_in, n*in_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_out, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_tab, tab.size()*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_mg, nodes*sizeof(pc_marg4)));
	PC_PROBE_TRY(hipMemset(d_code, 0, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMemset(d_out, 0, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMemcpy(d_in, in, n*in_w*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_tab, tab.data(), tab.size()*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_mg, t.mg.data(), nodes*sizeof(pc_marg4), hipMemcpyHostToDevice));
	if (s == hipSuccess) {
		const unsigned blocks = (unsigned)((n + 63)/64);
		if (flights) hipLaunchKernelGGL(pc_probe_flights_kernel, dim3(blocks), dim3(64), 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_in, d_out, d_code);
		else hipLaunchKernelGGL(pc_probe_march_kernel, dim3(blocks), dim3(64), 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_in, d_out, d_code);
		PC_PROBE_TRY(hipGetLastError());
	}
	PC_PROBE_TRY(hipDeviceSynchronize());
	PC_PROBE_TRY(hipMemcpy(out, d_out, n*out_w*sizeof(double), hipMemcpyDeviceToHost));
	PC_PROBE_TRY(hipMemcpy(code, d_code, n*sizeof(int32_t), hipMemcpyDeviceToHost));
	if (s != hipSuccess) rc = -3;
	const hipError_t f[5] = {hipFree(d_code), hipFree(d_in), hipFree(d_out), hipFree(d_tab), hipFree(d_mg)};
	for (int j = 0; j < 5 && rc == 0; j++)
		if (f[j] != hipSuccess) { snprintf(err, 256, "hipFree: %s", hipGetErrorString(f[j])); rc = -3; }
#undef PC_PROBE_TRY
	return rc;
}

/* one thread per row of an ends op (SINCOS, UNIFORM, ENTER, EXIT); the profile tables lie in global memory */
template <int OP>
__global__ void __launch_bounds__(64) pc_probe_ends_kernel(int64_t n, pc_params pm, int nodes, const double *__restrict__ tab,
                                                           const pc_marg4 *__restrict__ mg, const double *__restrict__ in,
                                                           double *__restrict__ out, int32_t *__restrict__ code)
{
	constexpr int WI = (OP == PC_PROBE_SINCOS) ? PC_PROBE_SINCOS_IN : (OP == PC_PROBE_UNIFORM) ? PC_PROBE_UNIFORM_IN
	                 : (OP == PC_PROBE_ENTER) ? PC_PROBE_ENTER_IN : PC_PROBE_EXIT_IN;
	constexpr int WO = (OP == PC_PROBE_SINCOS) ? PC_PROBE_SINCOS_OUT : (OP == PC_PROBE_UNIFORM) ? PC_PROBE_UNIFORM_OUT
	                 : (OP == PC_PROBE_ENTER) ? PC_PROBE_ENTER_OUT : PC_PROBE_EXIT_OUT;
	const int64_t i = (int64_t)blockIdx.x*blockDim.x + threadIdx.x;
	if (i >= n) return;
	pc_tables T;
	pc_probe_march_tables(T, tab, mg, nodes);
	double o[WO];
	int cd = 0;
	pc_probe_ends_eval<OP>(T, pm, in + i*WI, o, &cd);
	for (int j = 0; j < WO; j++) out[i*WO + j] = o[j];
	code[i] = cd;
}

/* an ends op on n rows, tables and parameters of the whole profile of p: what the four entry points share */
int run_ends(const pc_hip_problem *p, int op, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	err[0] = 0;
	pc_host_tables t;
	std::string msg;
	if (pc_build_tables(p, t, msg)) { snprintf(err, 256, "%s", msg.c_str()); return -2; }
	if (pc_probe_ends_check(p, op, n, in_w, out_w, in)) { snprintf(err, 256, "invalid op, size, width or row (non-finite value, x outside [0, 2], not a 32-bit value, d too large)"); return -2; }
	if (n == 0) return 0;
	const size_t nodes = (size_t)p->nmax + 1;
	std::vector<double> tab;
	tab.reserve(PC_PROBE_MARCH_TAB*nodes);
	const std::vector<double> *cols[PC_PROBE_MARCH_TAB] = {&t.z, &t.cap, &t.zh, &t.cap2, &t.hexd, &t.idz, &t.ext};
	for (int c = 0; c < PC_PROBE_MARCH_TAB; c++) tab.insert(tab.end(), cols[c]->begin(), cols[c]->end());
	int32_t *d_code = nullptr;
	double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
	pc_marg4 *d_mg = nullptr;
	int rc = 0;
	hipError_t s = hipSuccess;
#define PC_PROBE_TRY(call) do { if (s == hipSuccess) { s = (call); if (s != hipSuccess) snprintf(err, 256, "%s: %s", #call, hipGetErrorString(s)); } } while (0)
	PC_PROBE_TRY(hipMalloc(&d_code, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_in, n*in_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_out, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_tab, tab.size()*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_mg, nodes*sizeof(pc_marg4)));
	PC_PROBE_TRY(hipMemset(d_code, 0, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMemset(d_out, 0, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMemcpy(d_in, in, n*in_w*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_tab, tab.data(), tab.size()*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_mg, t.mg.data(), nodes*sizeof(pc_marg4), hipMemcpyHostToDevice));
	if (s == hipSuccess) {
		const dim3 blocks((unsigned)((n + 63)/64)), threads(64);
		if (op == PC_PROBE_SINCOS)
			hipLaunchKernelGGL(pc_probe_ends_kernel<PC_PROBE_SINCOS>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_in, d_out, d_code);
		else if (op == PC_PROBE_UNIFORM)
			hipLaunchKernelGGL(pc_probe_ends_kernel<PC_PROBE_UNIFORM>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_in, d_out, d_code);
		else if (op == PC_PROBE_ENTER)
			hipLaunchKernelGGL(pc_probe_ends_kernel<PC_PROBE_ENTER>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_in, d_out, d_code);
		else
			hipLaunchKernelGGL(pc_probe_ends_kernel<PC_PROBE_EXIT>, blocks, threads, 0, 0, n, t.pm, (int)nodes, d_tab, d_mg, d_in, d_out, d_code);
		PC_PROBE_TRY(hipGetLastError());
	}
	PC_PROBE_TRY(hipDeviceSynchronize());
	PC_PROBE_TRY(hipMemcpy(out, d_out, n*out_w*sizeof(double), hipMemcpyDeviceToHost));
	PC_PROBE_TRY(hipMemcpy(code, d_code, n*sizeof(int32_t), hipMemcpyDeviceToHost));
	if (s != hipSuccess) rc = -3;
	const hipError_t f[5] = {hipFree(d_code), hipFree(d_in), hipFree(d_out), hipFree(d_tab), hipFree(d_mg)};
	for (int j = 0; j < 5 && rc == 0; j++)
		if (f[j] != hipSuccess) { snprintf(err, 256, "hipFree: %s", hipGetErrorString(f[j])); rc = -3; }
#undef PC_PROBE_TRY
	return rc;
}

} // namespace

extern "C" {

/* Evaluates op on n elements: e[n] energy indices, in[n][PC_PROBE_IN], out[n][2], code[n] (host arrays).  Returns 0, -2 on
 * invalid arguments, -3 on a HIP error (message in err[256]). */
__attribute__((visibility("default")))
int probe_run(const pc_hip_problem *p, int op, int64_t n, const int32_t *e, const double *in, double *out, int32_t *code,
              char *err)
{
	err[0] = 0;
	pc_host_tables t;
	std::string msg;
	if (pc_build_tables(p, t, msg)) { snprintf(err, 256, "%s", msg.c_str()); return -2; }
	if (pc_probe_check(op, n, e, (int)t.ec.size())) { snprintf(err, 256, "invalid op, size or energy index"); return -2; }
	if (n == 0) return 0;
	pc_energy_const *d_ec = nullptr;
	int32_t *d_e = nullptr, *d_code = nullptr;
	double *d_in = nullptr, *d_out = nullptr;
	int rc = 0;
	hipError_t s = hipSuccess;
#define PC_PROBE_TRY(call) do { if (s == hipSuccess) { s = (call); if (s != hipSuccess) snprintf(err, 256, "%s: %s", #call, hipGetErrorString(s)); } } while (0)
	const size_t ne = t.ec.size();
	PC_PROBE_TRY(hipMalloc(&d_ec, ne*sizeof(pc_energy_const)));
	PC_PROBE_TRY(hipMalloc(&d_e, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_code, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_in, n*PC_PROBE_IN*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_out, n*2*sizeof(double)));
	PC_PROBE_TRY(hipMemcpy(d_ec, t.ec.data(), ne*sizeof(pc_energy_const), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_e, e, n*sizeof(int32_t), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_in, in, n*PC_PROBE_IN*sizeof(double), hipMemcpyHostToDevice));
	if (s == hipSuccess) {
		LAUNCH[op](n/pc_probe_group(op), d_ec, d_e, d_in, d_out, d_code);
		PC_PROBE_TRY(hipGetLastError());
	}
	PC_PROBE_TRY(hipDeviceSynchronize());
	PC_PROBE_TRY(hipMemcpy(out, d_out, n*2*sizeof(double), hipMemcpyDeviceToHost));
	PC_PROBE_TRY(hipMemcpy(code, d_code, n*sizeof(int32_t), hipMemcpyDeviceToHost));
	if (s != hipSuccess) rc = -3;
	/* frees run whatever happened above; their status is reported only when everything before succeeded */
	const hipError_t f[5] = {hipFree(d_ec), hipFree(d_e), hipFree(d_code), hipFree(d_in), hipFree(d_out)};
	for (int j = 0; j < 5 && rc == 0; j++)
		if (f[j] != hipSuccess) { snprintf(err, 256, "hipFree: %s", hipGetErrorString(f[j])); rc = -3; }
#undef PC_PROBE_TRY
	return rc;
}

/* A geometry op (PC_PROBE_SEGMENT, PC_PROBE_GEOM, PC_PROBE_BOUNCE) on n elements: in[n][in_w], out[n][out_w], code[n], widths as
 * pc_probe_in_width / pc_probe_out_width give them.  Same return values as probe_run. */
__attribute__((visibility("default")))
int probe_run_geom(const pc_hip_problem *p, int op, int64_t n, const int32_t *e, const double *in, int in_w, double *out,
                   int out_w, int32_t *code, char *err)
{
	err[0] = 0;
	pc_host_tables t;
	std::string msg;
	if (pc_build_tables(p, t, msg)) { snprintf(err, 256, "%s", msg.c_str()); return -2; }
	if (pc_probe_geom_check(op, n, in_w, out_w, e, (int)t.ec.size())) { snprintf(err, 256, "invalid op, size, width or energy index"); return -2; }
	if (n == 0) return 0;
	const bool seg = op == PC_PROBE_SEGMENT;
	std::vector<double> tab(seg ? (size_t)n*PC_PROBE_SEG_TAB : 1);
	for (int64_t i = 0; i < n; i++) {
		code[i] = 0;
		for (int j = 0; j < out_w; j++) out[i*out_w + j] = 0.;
		if (seg && pc_probe_seg_table(p, in + i*in_w, tab.data() + i*PC_PROBE_SEG_TAB)) code[i] = PC_PROBE_SETUP_REJECT;
	}
	pc_energy_const *d_ec = nullptr;
	int32_t *d_e = nullptr, *d_code = nullptr;
	double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
	int rc = 0;
	hipError_t s = hipSuccess;
#define PC_PROBE_TRY(call) do { if (s == hipSuccess) { s = (call); if (s != hipSuccess) snprintf(err, 256, "%s: %s", #call, hipGetErrorString(s)); } } while (0)
	const size_t ne = t.ec.size();
	PC_PROBE_TRY(hipMalloc(&d_ec, ne*sizeof(pc_energy_const)));
	PC_PROBE_TRY(hipMalloc(&d_e, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_code, n*sizeof(int32_t)));
	PC_PROBE_TRY(hipMalloc(&d_in, n*in_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_out, n*out_w*sizeof(double)));
	PC_PROBE_TRY(hipMalloc(&d_tab, tab.size()*sizeof(double)));
	PC_PROBE_TRY(hipMemcpy(d_ec, t.ec.data(), ne*sizeof(pc_energy_const), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_e, e, n*sizeof(int32_t), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_code, code, n*sizeof(int32_t), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_in, in, n*in_w*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_out, out, n*out_w*sizeof(double), hipMemcpyHostToDevice));
	PC_PROBE_TRY(hipMemcpy(d_tab, tab.data(), tab.size()*sizeof(double), hipMemcpyHostToDevice));
	if (s == hipSuccess) {
		if (op == PC_PROBE_SEGMENT) launch_geom<PC_PROBE_SEGMENT>(n, d_ec, d_e, d_in, d_tab, d_out, d_code);
		else if (op == PC_PROBE_GEOM) launch_geom<PC_PROBE_GEOM>(n, d_ec, d_e, d_in, d_tab, d_out, d_code);
		else launch_geom<PC_PROBE_BOUNCE>(n, d_ec, d_e, d_in, d_tab, d_out, d_code);
		PC_PROBE_TRY(hipGetLastError());
	}
	PC_PROBE_TRY(hipDeviceSynchronize());
	PC_PROBE_TRY(hipMemcpy(out, d_out, n*out_w*sizeof(double), hipMemcpyDeviceToHost));
	PC_PROBE_TRY(hipMemcpy(code, d_code, n*sizeof(int32_t), hipMemcpyDeviceToHost));
	if (s != hipSuccess) rc = -3;
	const hipError_t f[6] = {hipFree(d_ec), hipFree(d_e), hipFree(d_code), hipFree(d_in), hipFree(d_out), hipFree(d_tab)};
	for (int j = 0; j < 6 && rc == 0; j++)
		if (f[j] != hipSuccess) { snprintf(err, 256, "hipFree: %s", hipGetErrorString(f[j])); rc = -3; }
#undef PC_PROBE_TRY
	return rc;
}

/* Op MARCH on n photons through the whole profile of p (at most PC_PROBE_MARCH_NODES nodes): in[n][PC_PROBE_MARCH_IN],
 * out[n][PC_PROBE_MARCH_OUT], code[n].  Same return values as probe_run. */
__attribute__((visibility("default")))
int probe_run_march(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code,
                    char *err)
{
	return run_march(p, false, n, in, in_w, out, out_w, code, err);
}

/* Op FLIGHTS on n photons through the whole profile of p, flight after flight: in[n][PC_PROBE_FLIGHTS_IN],
 * out[n][PC_PROBE_FLIGHTS_OUT], code[n].  Same return values as probe_run. */
__attribute__((visibility("default")))
int probe_run_flights(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code,
                      char *err)
{
	return run_march(p, true, n, in, in_w, out, out_w, code, err);
}

/* Op WALL on n photons in the glass of p's whole profile: in[n][PC_PROBE_WALL_IN], out[n][PC_PROBE_WALL_OUT], code[n].  A row with
 * a non-finite value, dz == 0 or max_units above PC_PROBE_WALL_UNITS_DEVICE is refused before anything runs.  Same return values as
 * probe_run. */
__attribute__((visibility("default")))
int probe_run_wall(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_leak(p, PC_PROBE_WALL, n, in, in_w, out, out_w, code, err);
}

/* Op OUTER: pc_outer_intersect per row, in[n][PC_PROBE_OUTER_IN], out[n][PC_PROBE_OUTER_OUT] */
__attribute__((visibility("default")))
int probe_run_outer(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_leak(p, PC_PROBE_OUTER, n, in, in_w, out, out_w, code, err);
}

/* Op HEX: pc_hex_index per row, in[n][PC_PROBE_HEX_IN], out[n][PC_PROBE_HEX_OUT] */
__attribute__((visibility("default")))
int probe_run_hex(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_leak(p, PC_PROBE_HEX, n, in, in_w, out, out_w, code, err);
}

/* Op SINCOS: pc_sincos_quadrant per row, in[n][1], out[n][2] */
__attribute__((visibility("default")))
int probe_run_sincos(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_ends(p, PC_PROBE_SINCOS, n, in, in_w, out, out_w, code, err);
}

/* Op UNIFORM: uniform #d of the stream (seed, slot, attempt) per row, in[n][6], out[n][1] */
__attribute__((visibility("default")))
int probe_run_uniform(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_ends(p, PC_PROBE_UNIFORM, n, in, in_w, out, out_w, code, err);
}

/* Op ENTER: everything pc_launch_init leaves, per row, in[n][9], out[n][PC_PROBE_ENTER_OUT] */
__attribute__((visibility("default")))
int probe_run_enter(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_ends(p, PC_PROBE_ENTER, n, in, in_w, out, out_w, code, err);
}

/* Op EXIT: pc_in_exit_window per row, in[n][6], out[n][1] */
__attribute__((visibility("default")))
int probe_run_exit(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code, char *err)
{
	return run_ends(p, PC_PROBE_EXIT, n, in, in_w, out, out_w, code, err);
}

} // extern "C"

/* A stand-alone comparison for the tracing waves of pc_trace_producer_kernel (pc_producer_kernel.h): the same EVENT visit
 * and hot march step around one photon in registers, with nothing else in the loop -- no rings, no phase choice, no
 * launching wave.  Its listing shows what the two phases need by themselves (registers, spills) and has no block of register
 * copies inside its loop; it is not a lower bound for the real kernel's loop, since its total includes the staging of the tables and the
 * photon's load and store.  Compiled, never run:
 *
 *     python scripts/analysis/producer_listing.py --probe
 */
#include <hip/hip_runtime.h>

#include "pc_device.h"

#define PROBE_PITCH 1024

struct probe_args {
	const double *g_z, *g_cap, *g_zh, *g_cap2, *g_hexd, *g_idz, *g_ext;
	const pc_marg4 *g_mg;
	const pc_energy_const *ec;
	pc_params pm;
	pc_photon<1> *photons;     /* one per thread, in and out */
	int *states;
	int turns;
};

__global__ void __launch_bounds__(1024, 4)
pc_event_probe_kernel(probe_args a)
{
	__shared__ double lds[6*PROBE_PITCH];
	__shared__ pc_marg4 ldsg[PROBE_PITCH];
	const int npts = a.pm.nmax + 1;
	for (int k = threadIdx.x; k < npts && k < PROBE_PITCH; k += blockDim.x) {
		lds[k] = a.g_z[k];
		lds[PROBE_PITCH + k] = a.g_cap[k];
		lds[2*PROBE_PITCH + k] = a.g_zh[k];
		lds[3*PROBE_PITCH + k] = a.g_cap2[k];
		lds[4*PROBE_PITCH + k] = a.g_hexd[k];
		lds[5*PROBE_PITCH + k] = a.g_idz[k];
		ldsg[k] = a.g_mg[k];
	}
	__syncthreads();
	pc_tables T;
	T.z = lds; T.cap = lds + PROBE_PITCH; T.zh = lds + 2*PROBE_PITCH; T.cap2 = lds + 3*PROBE_PITCH;
	T.hexd = lds + 4*PROBE_PITCH; T.idz = lds + 5*PROBE_PITCH; T.ext = a.g_ext; T.mg = ldsg;
	const size_t t = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
	pc_photon<1> ph = a.photons[t];
	int state = a.states[t];
	for (int k = 0; k < a.turns; k++) {
		if (state == PC_ST_EVENT) state = pc_event<1, true>(T, a.pm, a.ec, ph);
		if (state == PC_ST_MARCH) state = pc_march_step_hot(T, a.pm, ph);
	}
	a.photons[t] = ph;
	a.states[t] = state;
}

/*
 * pc_sweep_cert.h -- what the host certifies about a run's energies for the logging kernel (pc_sweep_kernel.h): a pure function
 * of the per-energy constants with no HIP type in it, so a host compiler takes it too (tests/test_sweep_cert_cpu.py).
 * Included by pc_kernels.hip behind pc_device.h (pc_energy_const); a context keeps the result (pc_hip_ctx::cert).
 */
#ifndef PC_SWEEP_CERT_H
#define PC_SWEEP_CERT_H

#include <cmath>
#include <vector>

struct pc_sweep_cert {
	double ct_tame = 1.;
	int n_proxy = 0;
	int proxy_e[2] = {0, 0};
	bool known = false;            /* pc_sweep_certify has run */
};

/* What pc_trace_log_kernel needs to know about the run's energies (once per context):
 *   ct_tame -- a cosine of the angle to the surface normal above which every energy's reflectivity stays at least 1e-11 below 1
 *     (and, being a ratio of sums of squares weighted by fs, fp >= -1e-16, above 0): no factor of such a reflection can be
 *     rejected by the reference's range test (src/polycap-capil.c:633-637) and every weight only falls.  Found by evaluating
 *     1 - R_s = 4 c Re(g) / |c + g|^2 and 1 - R_p = 4 c Re(conj(g) n^2) / |g + n^2 c|^2, g = sqrt(n^2 - sin^2) from the device's own
 *     constants (pc_fresnel3), in extended precision on 64 points per decade of c from 1 down to 1e-13, per energy: ct_tame =
 *     4 x the largest grid point at which some energy comes closer than 1e-11 (the device's factors are within 2.1e-12 relative of
 *     the host's at R >= 1e-6; tests/test_gpu_devmath.py checks that they stay below 1 - 1e-12 above ct_tame).
 *     Below the critical angle 1 - R ~ 4 c beta / (2 delta)^1.5, so for glass ct_tame ~ 1e-11.
 *   proxies -- the energies that reflect best at 3 and at 30 mrad (roughness included): the last ones to fall below 1e-4. */
static pc_sweep_cert pc_sweep_certify(const std::vector<pc_energy_const> &ec)
{
	pc_sweep_cert cert;
	const int ne = (int)ec.size();
	auto refl = [](const pc_energy_const &k, long double c, long double &one_minus_rs, long double &one_minus_rp) {
		const long double zr = c*c - (long double)k.d2, zi = k.n2_im;
		const long double mag = sqrtl(zr*zr + zi*zi);
		long double gr = sqrtl(0.5L*(mag + fabsl(zr))), gi = (gr > 0.0L) ? 0.5L*fabsl(zi)/gr : 0.0L;
		if (zr < 0.0L) { const long double x = gr; gr = gi; gi = x; }
		if (zi < 0.0L) gi = -gi;
		const long double ar = (long double)k.n2_re*c, ai = (long double)k.n2_im*c;
		one_minus_rs = 4.0L*c*gr/((c + gr)*(c + gr) + gi*gi);
		one_minus_rp = 4.0L*(gr*ar + gi*ai)/((gr + ar)*(gr + ar) + (gi + ai)*(gi + ai));
	};
	long double worst = 0.0L;               /* largest grid point at which some energy is not safely below 1 */
	const long double step = powl(10.0L, -1.0L/64.0L);
	for (int e = 0; e < ne; e++) {
		long double c = 1.0L;
		for (int k = 0; k <= 13*64; k++, c *= step) {
			long double a, b;
			refl(ec[e], c, a, b);
			if (!(a >= 1.e-11L && b >= 1.e-11L) || !(a <= 1.0L && b <= 1.0L)) { if (c > worst) worst = c; break; }   /* scanning downwards: the first failure is the largest */
		}
	}
	long double tame = 4.0L*worst;
	if (tame < 4.e-13L) tame = 4.e-13L;     /* below the scanned range nothing is certified */
	cert.ct_tame = (tame > 2.0L) ? 2.0 : (double)tame;      /* 2: no reflection is tame (cos theta <= 1) */
	int best[2] = {0, 0};
	const long double at[2] = {3.e-3L, 3.e-2L};
	for (int j = 0; j < 2; j++) {
		long double top = -1.0L;
		for (int e = 0; e < ne; e++) {
			long double a, b;
			refl(ec[e], at[j], a, b);
			const long double x = (long double)ec[e].rough_c*at[j];
			const long double r = (1.0L - 0.5L*(a + b))*expl(-x*x);
			if (r > top) { top = r; best[j] = e; }
		}
	}
	cert.proxy_e[0] = best[0]; cert.proxy_e[1] = best[1];
	cert.n_proxy = (best[0] == best[1]) ? 1 : 2;
	cert.known = true;
	return cert;
}

#endif /* PC_SWEEP_CERT_H */

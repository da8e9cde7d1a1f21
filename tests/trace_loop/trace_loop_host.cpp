/*
 * trace_loop_host.cpp -- TEST-ONLY host compile of the device header (polycap_amd/csrc/hip/pc_device.h).
 *
 * Traces every photon twice, in lockstep, with the product's own functions: once as the one-photon-per-lane kernel does
 * (pc_event<1, true>: a reflection leaves the photon on the first segment of its next flight, first = 1, and the MARCH phase
 * takes that first step), once as the launching-wave kernel does (pc_event<1, true, true>: the visit takes the first step
 * itself where it can).  After every visit -- and the first step of the lanes that still have it before them -- both
 * photons must be equal bit for bit: node, certificate value, first, stride cap, state and every other field.
 * Built by tests/test_trace_loop_cpu.py into a temporary directory; never linked into or shipped with libpolycap.
 */
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pc_problem.h"

namespace {

struct Host {
	pc_host_tables t;
	pc_tables T;
};

int setup(const pc_hip_problem *p, Host &E)
{
	std::string err;
	int rc = pc_build_tables(p, E.t, err);
	if (rc) return rc;
	E.t.pm.literal = 0;
	E.T.z = E.t.z.data(); E.T.cap = E.t.cap.data(); E.T.zh = E.t.zh.data();
	E.T.cap2 = E.t.cap2.data(); E.T.hexd = E.t.hexd.data(); E.T.idz = E.t.idz.data(); E.T.ext = E.t.ext.data();
	E.T.mg = E.t.mg.data();
	E.T.stp = E.t.stp.data(); E.T.istp = E.t.istp.data(); E.T.dr = E.t.dr.data();
	return 0;
}

typedef pc_photon<1> photon;

uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

bool same(const photon &a, const photon &b)
{
	const double da[] = { a.Px, a.Py, a.Pz, a.dx, a.dy, a.dz, a.ex, a.ey, a.ez, a.kx, a.ky, a.sx, a.sy, a.ox, a.oy, a.idzd, a.dtravel, a.kn, a.w[0] };
	const double db[] = { b.Px, b.Py, b.Pz, b.dx, b.dy, b.dz, b.ex, b.ey, b.ez, b.kx, b.ky, b.sx, b.sy, b.ox, b.oy, b.idzd, b.dtravel, b.kn, b.w[0] };
	for (size_t k = 0; k < sizeof da/sizeof da[0]; k++)
		if (bits(da[k]) != bits(db[k])) return false;
	return bits(a.C0) == bits(b.C0) && a.i == b.i && a.irefl == b.irefl && a.first == b.first && a.bnd == b.bnd && a.wset == b.wset &&
	       a.lv == b.lv && a.rc == b.rc && a.qr == b.qr;
}

/* what a MARCH phase does with a lane: the first step of a flight where it is still due, else a step of the tight loop */
int march(const Host &E, photon &ph)
{
	return ph.first ? pc_march_step<1>(E.T, E.t.pm, ph) : pc_march_step_hot<1>(E.T, E.t.pm, ph);
}

/* stats: 0 visits, 1 visits that ended in a reflection, 2 of those: the visit took the first step itself (fused), 3 of those:
 * the fused step failed its certificate (EVENT), 4 reflections with the hit on a node (ix == i + 1), 5 reflections that left
 * dz < 0, 6 reflections in a boundary capillary, 7 comparisons that differed, 8 photons whose final record or rc differed,
 * 9 photons traced */
enum { N_STATS = 10 };

void trace_pair(const Host &E, photon a, int st, int64_t *stats)
{
	photon b = a;
	int sa = st, sb = st;
	stats[9]++;
	while (sa != PC_ST_DONE || sb != PC_ST_DONE) {
		if (sa != sb) { stats[7]++; break; }
		if (sa == PC_ST_MARCH) {
			sa = march(E, a);
			sb = march(E, b);
		} else {
			/* the segment this visit looks at and where its hit lies, from a copy */
			{
				photon c = a;
				pc_hit h;
				if (pc_event_pre(E.T, E.t.pm, c, h) == PC_ST_REFLECT && h.ix == c.i + 1) stats[4]++;
			}
			stats[0]++;
			sa = pc_event<1, true, false>(E.T, E.t.pm, E.t.ec.data(), a);
			sb = pc_event<1, true, true>(E.T, E.t.pm, E.t.ec.data(), b);
			if (sa == PC_ST_MARCH && a.first) {
				stats[1]++;
				if (a.dz < 0.) stats[5]++;
				if (a.bnd) stats[6]++;
				if (!(sb == PC_ST_MARCH && b.first)) { stats[2]++; if (sb == PC_ST_EVENT) stats[3]++; }
				sa = march(E, a);                                  /* the first step, as the next MARCH phase takes it */
			}
			if (sb == PC_ST_MARCH && b.first) sb = march(E, b);
		}
		if (sa != sb || !same(a, b)) { stats[7]++; break; }
	}
	if (sa != sb || !same(a, b)) stats[8]++;
}

} // namespace

extern "C" {

/* photons of the source: slots from slot0 on, every attempt of a slot up to the one that leaves through the exit window, until
 * n_entered photons have entered a capillary (or max_slots slots are used up) */
int trace_loop_source(const pc_hip_problem *p, uint64_t seed, int64_t slot0, int64_t n_entered, int64_t max_slots, int64_t *stats)
{
	Host E;
	int r = setup(p, E);
	if (r) return r;
	if (p->n_energies != 1) return -1;
	for (int k = 0; k < N_STATS; k++) stats[k] = 0;
	for (int64_t j = 0; j < max_slots && stats[9] < n_entered; j++) {
		for (uint32_t attempt = 0; attempt < (1u << 20) && stats[9] < n_entered; attempt++) {
			pc_start s;
			if (E.t.pm.generic_src) pc_sample_photon<true>(E.t.pm, seed, (uint64_t)(slot0 + j), attempt, s);
			else pc_sample_photon<false>(E.t.pm, seed, (uint64_t)(slot0 + j), attempt, s);
			photon ph; ph.wmem = nullptr; ph.wstride = 0;
			const int st = pc_launch_init(E.T, E.t.pm, ph, s.x, s.y, s.z, s.dx, s.dy, s.dz, s.ex, s.ey, s.ez);
			if (st != PC_ST_MARCH) continue;
			trace_pair(E, ph, st, stats);
			/* the same end of the slot as the driver loop's: a photon that leaves through the exit window */
			photon q = ph;
			int sq = st;
			while (sq != PC_ST_DONE) sq = (sq == PC_ST_MARCH) ? pc_march_step<1>(E.T, E.t.pm, q) : pc_event<1, true>(E.T, E.t.pm, E.t.ec.data(), q);
			if (q.rc == 1 && pc_in_exit_window(E.t.pm, q)) break;
		}
	}
	return 0;
}

/* explicit photons: start[3n], dir[3n], elecv[3n]; per_photon[n x N_STATS] holds each photon's own counts */
int trace_loop_explicit(const pc_hip_problem *p, int64_t n, const double *start, const double *dir, const double *elecv,
                        int64_t *stats, int64_t *per_photon)
{
	Host E;
	int r = setup(p, E);
	if (r) return r;
	if (p->n_energies != 1) return -1;
	for (int k = 0; k < N_STATS; k++) stats[k] = 0;
	for (int64_t j = 0; j < n; j++) {
		int64_t mine[N_STATS] = { 0 };
		photon ph; ph.wmem = nullptr; ph.wstride = 0;
		const int st = pc_launch_init(E.T, E.t.pm, ph, start[3*j], start[3*j+1], start[3*j+2], dir[3*j], dir[3*j+1], dir[3*j+2],
		                              elecv[3*j], elecv[3*j+1], elecv[3*j+2]);
		if (st == PC_ST_MARCH) trace_pair(E, ph, st, mine);
		for (int k = 0; k < N_STATS; k++) { stats[k] += mine[k]; if (per_photon) per_photon[N_STATS*j + k] = mine[k]; }
	}
	return 0;
}

} // extern "C"

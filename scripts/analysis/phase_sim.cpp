/* Phase simulator of a tracing wave of pc_trace_producer_kernel (host only; driven by phase_sim.py).
 *
 * 64 lanes run the product's own pc_march_step, pc_march_step_hot and pc_event<1, true> (host compile of pc_device.h through
 * tests/emul/pc_emul.cpp) inside a copy of the tracing wave's phase loop: the same choice of the phase from the lane counts,
 * the same burst rule, a ring of PC3_CAP = 28 launched photons per wave.  What the launching wave does is replaced by a feed
 * per wave, filled before the run: the entered photons of slots 0 .. n_slots-1 (every attempt up to the one that leaves
 * through the exit window), dealt to the waves by a routing policy.  The simulator counts phases and their lanes; a modelled
 * cost weighs them with instruction counts per phase taken from the listing (scripts/analysis/producer_listing.py).
 * Nothing here measures time: the tool answers "does another threshold / stride / routing change the number of wave-phases". */
#include "../../tests/emul/pc_emul.cpp"
#include <algorithm>
#include <cstdio>
#include <vector>

enum { S_NEED = 0, S_MARCH = 1, S_EVENT = 2, S_DONE = 3 };
enum { RING = 28, UNROLL = 4 };

struct Ent { pc_photon<1> ph; double kn; int nrefl; };
struct Cost { double march_steps = 0, march_lanes = 0, first_blocks = 0, first_lanes = 0, ev = 0, ev_lanes = 0, nw = 0, nw_lanes = 0, turns = 0; };
struct Knobs { int event_threshold, march_stop, march_burst, new_threshold, pool_event_min; };

static int next_state(int s) { return s == PC_ST_MARCH ? S_MARCH : (s == PC_ST_EVENT ? S_EVENT : S_DONE); }

/* the loop of pc_producer_kernel.h's tracing wave, phase by phase */
static void sim_wave(const Emul &E, const std::vector<Ent *> &feed, Cost &c, const Knobs &k)
{
	const pc_params &Pm = E.t.pm;
	const pc_tables &T = E.T;
	pc_photon<1> ph[64];
	int st[64];
	for (int l = 0; l < 64; l++) st[l] = S_NEED;
	size_t head = 0;
	for (;;) {
		int nM = 0, nE = 0, nD = 0, nQ = 0;
		for (int l = 0; l < 64; l++) { nM += st[l] == S_MARCH; nE += st[l] == S_EVENT; nD += st[l] == S_DONE; nQ += st[l] == S_NEED; }
		const long avail = std::min<long>((long)(feed.size() - head), RING);
		const int nN = nD + (int)std::min<long>(nQ, avail);
		const bool do_new = (nN >= k.new_threshold) || (nM == 0 && nE == 0);
		c.turns++;
		if (nM + nE + nD == 0 && avail == 0) break;
		if (nM > 0 && (nM >= k.event_threshold || (nE == 0 && !(do_new && nN > 0))) && !(nN >= k.pool_event_min)) {
			/* MARCH: the first-segment step of the lanes that start a flight, then bursts of UNROLL hot steps */
			int fl = 0;
			for (int l = 0; l < 64; l++)
				if (st[l] == S_MARCH && ph[l].first) { fl++; st[l] = next_state(pc_march_step(T, Pm, ph[l])); }
			if (fl) { c.first_blocks++; c.first_lanes += fl; }
			for (int b = 0; b < k.march_burst; b++) {
				for (int u = 0; u < UNROLL; u++) {
					int m = 0;
					for (int l = 0; l < 64; l++)
						if (st[l] == S_MARCH) { m++; st[l] = next_state(pc_march_step_hot(T, Pm, ph[l])); }
					if (m) { c.march_steps++; c.march_lanes += m; }
				}
				int cM = 0;
				for (int l = 0; l < 64; l++) cM += st[l] == S_MARCH;
				if (cM == 0) break;
				if (cM < k.march_stop && (cM != nM || do_new || nE > 0)) break;
			}
		} else if (nE > 0 && !(do_new && nN > nE) && !(nN >= k.pool_event_min)) {
			c.ev++; c.ev_lanes += nE;
			for (int l = 0; l < 64; l++)
				if (st[l] == S_EVENT) st[l] = next_state(pc_event<1, true>(T, Pm, E.t.ec.data(), ph[l]));
		} else if (nN > 0) {
			c.nw++; c.nw_lanes += nN;
			for (int l = 0; l < 64; l++) if (st[l] == S_DONE) st[l] = S_NEED;
			long av = std::min<long>((long)(feed.size() - head), RING);
			for (int l = 0; l < 64 && av > 0; l++)
				if (st[l] == S_NEED) { ph[l] = feed[head++]->ph; st[l] = S_MARCH; av--; }
		} else break;
	}
}

/* policy: 0 entered photons dealt to the waves in arrival order (what the product does), 1 bands of kn over the whole run,
 * 2 every batch of 64 sorted by kn and dealt in bands, 3 bands of the true reflection count (an oracle).
 * cost[4] = instructions per hot march step, first-segment block, EVENT visit, NEW phase.
 * out[13] = entered photons, march wave-steps, their lanes, first blocks, their lanes, EVENT phases, their lanes, NEW phases,
 * their lanes, loop turns, modelled cost summed over the waves, the largest wave's cost, correlation of kn with reflections */
extern "C" int phase_sim_run(const pc_hip_problem *p, uint64_t seed, int64_t n_slots, int policy, int nwaves,
                             int event_threshold, int march_stop, const double *cost, double *out)
{
	Emul E;
	int r = setup(p, 0, E);
	if (r) return r;
	std::vector<Ent> pool;
	pool.reserve((size_t)n_slots*2);
	for (int64_t j = 0; j < n_slots; j++)
		for (uint32_t att = 0; att < (1u << 20); att++) {
			pc_start s;
			pc_sample_photon<false>(E.t.pm, seed, (uint64_t)j, att, s);
			Ent e;
			e.ph.wmem = nullptr; e.ph.wstride = 0;
			int st = pc_launch_init(E.T, E.t.pm, e.ph, s.x, s.y, s.z, s.dx, s.dy, s.dz, s.ex, s.ey, s.ez);
			if (st != PC_ST_MARCH) continue;
			pc_photon<1> q = e.ph;
			while (st != PC_ST_DONE) st = (st == PC_ST_MARCH) ? pc_march_step(E.T, E.t.pm, q) : pc_event<1, true>(E.T, E.t.pm, E.t.ec.data(), q);
			e.nrefl = q.irefl; e.kn = e.ph.kn;
			pool.push_back(e);
			if (q.rc == 1 && pc_in_exit_window(E.t.pm, q)) break;
		}
	const size_t N = pool.size();
	std::vector<std::vector<Ent *>> feeds(nwaves);
	std::vector<Ent *> order(N);
	for (size_t k = 0; k < N; k++) order[k] = &pool[k];
	if (policy == 0) {
		for (size_t k = 0; k < N; k++) feeds[k % nwaves].push_back(order[k]);
	} else if (policy == 1 || policy == 3) {
		if (policy == 1) std::stable_sort(order.begin(), order.end(), [](Ent *a, Ent *b) { return a->kn < b->kn; });
		else std::stable_sort(order.begin(), order.end(), [](Ent *a, Ent *b) { return a->nrefl < b->nrefl; });
		for (size_t k = 0; k < N; k++) feeds[k*nwaves/N].push_back(order[k]);
		for (auto &f : feeds) std::sort(f.begin(), f.end());      /* within a band: arrival order */
	} else {
		for (size_t b = 0; b < N; b += 64) {
			const size_t e = std::min(N, b + 64);
			std::stable_sort(order.begin() + b, order.begin() + e, [](Ent *x, Ent *y) { return x->kn < y->kn; });
			for (size_t k = b; k < e; k++) feeds[(k - b)*nwaves/(e - b)].push_back(order[k]);
		}
	}
	const Knobs kn = { event_threshold, march_stop, 16, 2, 6 };      /* the rest: the product's defaults */
	Cost c;
	double maxw = 0, sumw = 0;
	for (int w = 0; w < nwaves; w++) {
		Cost cw;
		sim_wave(E, feeds[w], cw, kn);
		const double wi = cost[0]*cw.march_steps + cost[1]*cw.first_blocks + cost[2]*cw.ev + cost[3]*cw.nw + 15*cw.turns;
		maxw = std::max(maxw, wi); sumw += wi;
		c.march_steps += cw.march_steps; c.march_lanes += cw.march_lanes; c.first_blocks += cw.first_blocks; c.first_lanes += cw.first_lanes;
		c.ev += cw.ev; c.ev_lanes += cw.ev_lanes; c.nw += cw.nw; c.nw_lanes += cw.nw_lanes; c.turns += cw.turns;
	}
	out[0] = (double)N; out[1] = c.march_steps; out[2] = c.march_lanes; out[3] = c.first_blocks; out[4] = c.first_lanes;
	out[5] = c.ev; out[6] = c.ev_lanes; out[7] = c.nw; out[8] = c.nw_lanes; out[9] = c.turns; out[10] = sumw; out[11] = maxw;
	double sk = 0, sn = 0, skk = 0, snn = 0, skn = 0;
	for (auto &e : pool) { sk += e.kn; sn += e.nrefl; skk += e.kn*e.kn; snn += (double)e.nrefl*e.nrefl; skn += e.kn*e.nrefl; }
	const double mk = sk/N, mn = sn/N;
	out[12] = (skn/N - mk*mn)/std::sqrt((skk/N - mk*mk)*(snn/N - mn*mn));
	return 0;
}

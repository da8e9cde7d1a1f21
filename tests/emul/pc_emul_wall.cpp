/*
 * pc_emul_wall.cpp -- TEST-ONLY host compile of probe op WALL (tests/devmath/probe_ops.h) with the unit counters of pc_leak.h
 * (PC_LEAK_STATS, as scripts/analysis/leak_units.cpp uses them): the counter that moves during a unit of the wall search says what
 * kind of unit it was -- certified stretch, literal step, probe skip at level 0 / 1 / 2, probe visit -- which cannot be told from
 * the outside (a certified stretch may be one step long).  A library of its own (tests/emul/libpc_emul_wall.so), so that no entry
 * point of pc_emul.cpp is compiled any differently.  Rows run one after the other on the calling thread: the counters are global.
 */
#define PC_LEAK_STATS 1
#include <cstdint>
#include <string>
#include <vector>

#include "pc_problem.h"
#include "pc_leak.h"
#include "../devmath/probe_ops.h"

long long pc_leak_stats[16];

extern "C" {

/* the host build of probe.hip's probe_run_wall; max_units may go up to PC_PROBE_WALL_UNITS_HOST here */
int emul_probe_run_wall(const pc_hip_problem *p, int64_t n, const double *in, int in_w, double *out, int out_w, int32_t *code)
{
	pc_host_tables t;
	std::string err;
	int r = pc_build_tables(p, t, err);
	if (r) return r;
	if (pc_probe_leak_check(p, PC_PROBE_WALL, n, in_w, out_w, in, PC_PROBE_WALL_UNITS_HOST)) return -2;
	pc_tables T;
	T.z = t.z.data(); T.cap = t.cap.data(); T.zh = t.zh.data(); T.cap2 = t.cap2.data(); T.hexd = t.hexd.data();
	T.idz = t.idz.data(); T.ext = t.ext.data(); T.mg = t.mg.data();
	T.stp = t.stp.data(); T.istp = t.istp.data(); T.dr = t.dr.data();
	for (int64_t i = 0; i < n; i++) {
		int cd = 0;
		double *o = out + i*out_w;
		for (int j = 0; j < out_w; j++) o[j] = 0.;
		pc_probe_wall_eval(T, t.pm, in + i*in_w, o, &cd);
		code[i] = cd;
	}
	return 0;
}

} // extern "C"

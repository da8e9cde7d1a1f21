/* What pc_run_request_parse (polycap_amd/csrc/host/pc_request.c) makes of an environment, as text: a program of its own that links
 * pc_request.c, pc_error.c and request_validators.cpp -- no device, no library, nothing loaded into python.  tests/test_request_cpu.py
 * builds it plain and with -fsanitize=address,undefined; scripts/record_call_requests.py builds it with -DREQUEST_HOST_SOURCE="file.c"
 * over another commit's file that holds the parsers (they were static in pc_source.c) to record tests/golden/call_requests.json.
 *
 * Standard input holds cases: a line "ne leak_calc n_photons n_vars", then n_vars lines NAME=VALUE.  For each case every POLYCAP_*
 * variable of the call is unset, the case's are set, and the program prints "case K", then "error CODE MESSAGE" or one line per field
 * of struct pc_run_request (doubles as %a, lists element by element, what a spec points to as data), then "end". */
#define _GNU_SOURCE
#ifdef REQUEST_HOST_SOURCE
#include REQUEST_HOST_SOURCE
#else
#include "pc_private.h"
#endif

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char *const variables[] = { "POLYCAP_TIMING", "POLYCAP_STDERR", "POLYCAP_TALLY_STDERR", "POLYCAP_BEAM", "POLYCAP_SPOT", "POLYCAP_SPOT_SHARE",
	"POLYCAP_HIST", "POLYCAP_JOINT", "POLYCAP_SELECT", "POLYCAP_SELECT_RECORDS", "POLYCAP_DRAW", "POLYCAP_HIP_DEVICES", "POLYCAP_IMAGES",
	"POLYCAP_RUN_PARTS", "POLYCAP_COMPACT", "POLYCAP_BLOCK_SHIFT", "POLYCAP_RCCL", "POLYCAP_MAX_ATTEMPTS", "POLYCAP_SEED" };

static void dump_doubles(const char *name, const double *v, int n)
{
	printf("%s =", name);
	for (int k = 0; v != NULL && k < n; k++) printf(" %a", v[k]);
	printf("%s\n", v == NULL ? " NULL" : "");
}

static void dump_ints(const char *name, const int32_t *v, int n)
{
	printf("%s =", name);
	for (int k = 0; v != NULL && k < n; k++) printf(" %d", (int)v[k]);
	printf("%s\n", v == NULL ? " NULL" : "");
}

static void dump_axis(const char *name, int k, const char *part, const pc_hip_hist_axis *a)
{
	printf("%s[%d]%s = quantity %d d %a cx %a cy %a lo %a hi %a n_bins %d\n", name, k, part, (int)a->quantity, a->d, a->cx, a->cy, a->lo, a->hi, (int)a->n_bins);
}

static void dump_axes(const char *name, const pc_hip_hist_axis *a, int n)
{
	if (a == NULL) printf("%s = NULL\n", name);
	for (int k = 0; a != NULL && k < n; k++) dump_axis(name, k, "", &a[k]);
}

static void dump_pairs(const char *name, const pc_hip_joint_pair *p, int n)
{
	if (p == NULL) printf("%s = NULL\n", name);
	for (int k = 0; p != NULL && k < n; k++) {
		dump_axis(name, k, ".u", &p[k].u);
		dump_axis(name, k, ".v", &p[k].v);
	}
}

static void dump_cuts(const char *name, const pc_hip_select_cut *c, int n)
{
	if (c == NULL) printf("%s = NULL\n", name);
	for (int k = 0; c != NULL && k < n; k++) {
		dump_axis(name, k, ".axis", &c[k].axis);
		printf("%s[%d].negate = %d\n", name, k, (int)c[k].negate);
	}
}

static void dump(const struct pc_run_request *r)
{
	printf("timing = %d\ntally_stderr_on = %d\nstderr_on = %d\nbeam_on = %d\n", r->timing, r->tally_stderr_on, r->stderr_on, r->beam_on);
	printf("spot.set = %d\nspot.n_dist = %d\n", r->spot.set, r->spot.n_dist);
	dump_doubles("spot.dist", r->spot.dist, r->spot.n_dist);
	printf("spot.n_energies = %d\n", r->spot.n_energies);
	dump_ints("spot.energies", r->spot.energies, r->spot.n_energies);
	printf("spot.share = %a\nspot.spec.n_planes = %d\n", r->spot.share, (int)r->spot.spec.n_planes);
	dump_doubles("spot.spec.distances", r->spot.spec.distances, r->spot.spec.n_planes);
	printf("spot.spec.window = %a %a %a %a\nspot.spec.bins = %d %d\nspot.spec.n_energies = %d\n", r->spot.spec.x0, r->spot.spec.x1, r->spot.spec.y0,
		r->spot.spec.y1, (int)r->spot.spec.nx, (int)r->spot.spec.ny, (int)r->spot.spec.n_energies);
	dump_ints("spot.spec.energies", r->spot.spec.energies, r->spot.spec.n_energies);
	printf("spot.spec.regime = %d\n", (int)r->spot.spec.regime);

	printf("hist.set = %d\nhist.n_axes = %d\n", r->hist.set, r->hist.n_axes);
	dump_axes("hist.axes", r->hist.axes, r->hist.n_axes);
	printf("hist.n_energies = %d\n", r->hist.n_energies);
	dump_ints("hist.energies", r->hist.energies, r->hist.n_energies);
	printf("hist.spec.n_axes = %d\n", (int)r->hist.spec.n_axes);
	dump_axes("hist.spec.axes", r->hist.spec.axes, r->hist.spec.n_axes);
	printf("hist.spec.n_energies = %d\n", (int)r->hist.spec.n_energies);
	dump_ints("hist.spec.energies", r->hist.spec.energies, r->hist.spec.n_energies);
	printf("hist.spec.regime = %d\n", (int)r->hist.spec.regime);

	printf("joint.set = %d\njoint.n_pairs = %d\n", r->joint.set, r->joint.n_pairs);
	dump_pairs("joint.pairs", r->joint.pairs, r->joint.n_pairs);
	printf("joint.n_energies = %d\n", r->joint.n_energies);
	dump_ints("joint.energies", r->joint.energies, r->joint.n_energies);
	printf("joint.spec.n_pairs = %d\n", (int)r->joint.spec.n_pairs);
	dump_pairs("joint.spec.pairs", r->joint.spec.pairs, r->joint.spec.n_pairs);
	printf("joint.spec.n_energies = %d\n", (int)r->joint.spec.n_energies);
	dump_ints("joint.spec.energies", r->joint.spec.energies, r->joint.spec.n_energies);
	printf("joint.spec.regime = %d\n", (int)r->joint.spec.regime);

	printf("select.set = %d\nselect.n_cuts = %d\n", r->select.set, (int)r->select.n_cuts);
	dump_cuts("select.cuts", r->select.cuts, r->select.n_cuts);
	printf("select.spec.n_cuts = %d\n", (int)r->select.spec.n_cuts);
	dump_cuts("select.spec.cuts", r->select.spec.cuts, r->select.spec.n_cuts);
	printf("select.records = %" PRId64 "\n", r->select.records);

	printf("draw.set = %d\ndraw.implicit = %d\ndraw.n = %" PRId64 "\ndraw.energy = %d\ndraw.phase = %" PRIu32 "\n", r->draw.set, r->draw.implicit, r->draw.n,
		(int)r->draw.energy, r->draw.phase);
	printf("n_devices = %d\n", r->n_devices);
	dump_ints("devices", (const int32_t *)r->devices, r->n_devices);
	printf("keep_images = %d\nrun_parts = %d\ncompact = %d\nhave_block_shift = %d\nblock_shift = %" PRId64 "\nrccl = %d\nmax_attempts = %" PRIu32 "\n",
		r->keep_images, r->run_parts, r->compact, r->have_block_shift, r->block_shift, r->rccl, r->max_attempts);
	printf("have_seed = %d\nseed = %" PRIu64 "\n", r->have_seed, r->seed);
}

int main(void)
{
	char *line = NULL;
	size_t cap = 0;
	int n_case = 0;
	while (getline(&line, &cap, stdin) > 0) {
		size_t ne = 0;
		int leak_calc = 0, n_photons = 0, n_vars = 0;
		if (sscanf(line, "%zu %d %d %d", &ne, &leak_calc, &n_photons, &n_vars) != 4) {
			fprintf(stderr, "request_host: bad case header: %s", line);
			free(line);
			return 2;
		}
		for (size_t k = 0; k < sizeof(variables)/sizeof(variables[0]); k++)
			unsetenv(variables[k]);
		for (int k = 0; k < n_vars; k++) {
			const ssize_t len = getline(&line, &cap, stdin);
			char *eq = len > 0 ? strchr(line, '=') : NULL;
			if (eq == NULL) {
				fprintf(stderr, "request_host: case %d: NAME=VALUE expected\n", n_case);
				free(line);
				return 2;
			}
			if (line[len - 1] == '\n') line[len - 1] = '\0';
			*eq = '\0';
			setenv(line, eq + 1, 1);
		}
		struct pc_run_request req;
		polycap_error *error = NULL;
		printf("case %d\n", n_case++);
		if (pc_run_request_parse(&req, ne, leak_calc, n_photons, &error) != 0)
			printf("error %d %s\n", error != NULL ? (int)error->code : -1, error != NULL ? error->message : "(no error was set)");
		else
			dump(&req);
		printf("end\n");
		pc_run_request_free(&req);
		polycap_error_free(error);
	}
	free(line);
	return 0;
}

/*
 * pc_request.c -- everything polycap_source_get_transmission_efficiencies takes from the environment (struct pc_run_request,
 * pc_private.h), read and checked by pc_run_request_parse before any device is used.
 *
 * One convention for the parsers of a variable or of a part of one: they return NULL, or the reason of the refusal -- a literal, or
 * text written into the caller's `why` [PC_WHY].  pc_refused turns a reason into the call's error, in one place.  A parser never
 * frees: what a request holds is freed by pc_run_request_free, after a refusal as well.
 */
#define _GNU_SOURCE
#include "pc_private.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

#define PC_CALL "polycap_source_get_transmission_efficiencies: "
#define PC_WHY 320

/* 0 when bad is NULL; otherwise -1 and the error "<the call>: NAME=<its value>: <bad>" */
static int pc_refused(polycap_error **error, const char *name, const char *bad)
{
	if (bad == NULL)
		return 0;
	polycap_set_error(error, POLYCAP_ERROR_INVALID_ARGUMENT, PC_CALL "%s=%s: %s", name, getenv(name), bad);
	return -1;
}

/* the message of the pc_hip_* call that has just refused, into why */
static const char *pc_hip_reason(char *why)
{
	snprintf(why, PC_WHY, "%s", pc_hip_last_error());
	return why;
}

static uint64_t pc_env_u64(const char *name, uint64_t fallback, int *present)
{
	const char *env = getenv(name);
	if (present) *present = 0;
	if (env == NULL || *env == '\0')
		return fallback;
	char *end = NULL;
	unsigned long long v = strtoull(env, &end, 0);
	if (end == env)
		return fallback;
	if (present) *present = 1;
	return (uint64_t)v;
}

/* POLYCAP_HIP_DEVICES = "all" or a comma-separated list of device indices (an index may repeat).  *n = 0 when unset. */
static int pc_env_devices(int devices[64], int *n, polycap_error **error)
{
	*n = 0;
	const char *env = getenv("POLYCAP_HIP_DEVICES");
	if (env == NULL || *env == '\0')
		return 0;
	if (strcmp(env, "all") == 0) {
		int count = pc_hip_device_count();
		if (count < 1) {
			polycap_set_error_literal(error, POLYCAP_ERROR_RUNTIME, PC_CALL "POLYCAP_HIP_DEVICES=all but no HIP device is visible (the trace path has no CPU fallback)");
			return -1;
		}
		if (count > 64) count = 64;
		for (int k = 0; k < count; k++) devices[k] = k;
		*n = count;
		return 0;
	}
	const char *p = env;
	while (*p != '\0') {
		char *end = NULL;
		long v = strtol(p, &end, 10);
		if (end == p || v < 0 || *n >= 64 || (*end != ',' && *end != '\0')) {
			polycap_set_error(error, POLYCAP_ERROR_INVALID_ARGUMENT, PC_CALL "cannot parse POLYCAP_HIP_DEVICES=%s (all, or up to 64 comma-separated device indices)", env);
			return -1;
		}
		devices[(*n)++] = (int)v;
		p = (*end == ',') ? end + 1 : end;
	}
	return 0;
}

/* POLYCAP_STDERR, _TALLY_STDERR, _BEAM: 1 turns *on, 0 or unset leaves it off */
static const char *pc_flag_parse(const char *value, int *on)
{
	*on = value != NULL && strcmp(value, "1") == 0;
	return (value == NULL || *on || strcmp(value, "0") == 0) ? NULL : "must be 0 or 1";
}

/* POLYCAP_SPOT_SHARE into *share: the fraction of the device's memory the exit data of one run may take; unset or empty: 0.5 */
static const char *pc_share_parse(const char *value, double *share)
{
	*share = 0.5;
	if (value == NULL || *value == '\0')
		return NULL;
	char *end = NULL;
	*share = strtod(value, &end);
	return (*end != '\0' || !(*share > 0. && *share <= 1.)) ? "must be a fraction in (0, 1]" : NULL;
}

/* "a,b,..." into at most max doubles */
static int pc_parse_doubles(const char *v, double *out, int max, int *n)
{
	*n = 0;
	while (*v != '\0') {
		char *end = NULL;
		errno = 0;
		const double d = strtod(v, &end);
		if (end == v || errno != 0 || *n >= max)
			return -1;
		out[(*n)++] = d;
		v = end;
		if (*v == ',')
			v++;
		else if (*v != '\0')
			return -1;
	}
	return *n > 0 ? 0 : -1;
}

/* "A:B" into two doubles */
static int pc_parse_pair(const char *v, double *a, double *b)
{
	char *end = NULL;
	errno = 0;
	*a = strtod(v, &end);
	if (end == v || errno != 0 || *end != ':')
		return -1;
	v = end + 1;
	*b = strtod(v, &end);
	return (end == v || errno != 0 || *end != '\0') ? -1 : 0;
}

/* the value of an energies= item of POLYCAP_SPOT, _HIST or _JOINT into *list (malloc'd, NULL for "all") and *n; an index that no
 * int32 holds becomes -1, which the validation refuses by name */
static const char *pc_parse_energies(const char *v, size_t n_energies, int32_t **list, int *n)
{
	static const char *const bad = "energies must be all or a list of energy indices";
	free(*list);
	*list = NULL;
	*n = 0;
	if (strcmp(v, "all") == 0)
		return NULL;
	*list = malloc(sizeof(int32_t) * (n_energies + 1));
	while (*list != NULL && *v != '\0') {
		char *end = NULL;
		const long e = strtol(v, &end, 10);
		if (end == v || (size_t)*n > n_energies)
			return bad;
		(*list)[(*n)++] = (e < -1 || e > 1 << 30) ? -1 : (int32_t)e;
		v = end;
		if (*v == ',') v++;
		else if (*v != '\0') return bad;
	}
	return *n == 0 ? bad : NULL;
}

/* one axis of POLYCAP_HIST or _JOINT: comma-separated key=value parts, the first being axis=NAME.  n_names: 10 for a histogram axis,
 * 12 for an axis of a joint histogram (start_x and start_y as well) */
static const char *pc_parse_axis(char *item, pc_hip_hist_axis *ax, int n_names)
{
	static const char *names[] = { "x", "y", "r", "slope_x", "slope_y", "tan_theta", "nrefl", "dtravel", "r_start", "z", "start_x", "start_y" };
	int have_axis = 0, have_range = 0, have_bins = 0;
	char *save = NULL;
	memset(ax, 0, sizeof(*ax));
	for (char *kv = strtok_r(item, ",", &save); kv != NULL; kv = strtok_r(NULL, ",", &save)) {
		char *eq = strchr(kv, '=');
		if (eq == NULL)
			return "every part of an axis must be key=value";
		*eq = '\0';
		const char *v = eq + 1;
		char *end = NULL;
		if (strcmp(kv, "axis") == 0) {
			ax->quantity = -1;
			for (int q = 0; q < n_names; q++)
				if (strcmp(v, names[q]) == 0)
					ax->quantity = q;
			if (ax->quantity < 0)
				return n_names == 10 ? "axis must be one of x y r slope_x slope_y tan_theta nrefl dtravel r_start z"
				                     : "axis must be one of x y r slope_x slope_y tan_theta nrefl dtravel r_start z start_x start_y";
			have_axis = 1;
		} else if (strcmp(kv, "d") == 0) {
			errno = 0;
			ax->d = strtod(v, &end);
			if (end == v || errno != 0 || *end != '\0')
				return "d must be a distance in cm";
		} else if (strcmp(kv, "centre") == 0) {
			if (pc_parse_pair(v, &ax->cx, &ax->cy) != 0)
				return "centre must be CX:CY in cm";
		} else if (strcmp(kv, "range") == 0) {
			if (pc_parse_pair(v, &ax->lo, &ax->hi) != 0)
				return "range must be LO:HI";
			have_range = 1;
		} else if (strcmp(kv, "bins") == 0) {
			const long n = strtol(v, &end, 10);
			if (end == v || *end != '\0' || n < 0 || n > 1 << 24)
				return "bins must be a count";
			ax->n_bins = (int32_t)n;
			have_bins = 1;
		} else {
			return "unknown key of an axis (axis, d, centre, range, bins)";
		}
	}
	return (have_axis && have_range && have_bins) ? NULL : "an axis needs axis, range and bins";
}

/* POLYCAP_SPOT; an empty value counts as unset.  POLYCAP_SPOT_SHARE is read here, behind the grammar and before the validation, and
 * a bad one is refused as part of POLYCAP_SPOT */
static const char *pc_spot_request_parse(struct pc_spot_request *r, const char *value, size_t n_energies, char *why)
{
	if (value == NULL || *value == '\0')
		return NULL;
	r->set = 1;
	char *buf = strdup(value), *save = NULL;
	const char *bad = NULL;
	int have_dist = 0, have_window = 0, have_bins = 0;
	for (char *item = strtok_r(buf, ";", &save); item != NULL && bad == NULL; item = strtok_r(NULL, ";", &save)) {
		char *eq = strchr(item, '=');
		if (eq == NULL) { bad = "every item must be key=value"; break; }
		*eq = '\0';
		const char *key = item, *v = eq + 1;
		if (strcmp(key, "dist") == 0) {
			if (pc_parse_doubles(v, r->dist, 65, &r->n_dist) != 0) bad = "dist must be a list of at most 64 distances in cm";
			have_dist = 1;
		} else if (strcmp(key, "window") == 0) {
			double w[4];
			int n = 0;
			if (pc_parse_doubles(v, w, 4, &n) != 0 || n != 4) { bad = "window must be x0,x1,y0,y1 in cm"; break; }
			r->spec.x0 = w[0]; r->spec.x1 = w[1]; r->spec.y0 = w[2]; r->spec.y1 = w[3];
			have_window = 1;
		} else if (strcmp(key, "bins") == 0) {
			char *end = NULL;
			const long nx = strtol(v, &end, 10);
			if (end == v || (*end != 'x' && *end != 'X')) { bad = "bins must be NXxNY"; break; }
			const char *v2 = end + 1;
			const long ny = strtol(v2, &end, 10);
			if (end == v2 || *end != '\0' || nx < 0 || ny < 0 || nx > 1 << 27 || ny > 1 << 27) { bad = "bins must be NXxNY"; break; }
			r->spec.nx = (int32_t)nx; r->spec.ny = (int32_t)ny;
			have_bins = 1;
		} else if (strcmp(key, "energies") == 0) {
			bad = pc_parse_energies(v, n_energies, &r->energies, &r->n_energies);
		} else {
			bad = "unknown key (dist, window, bins, energies)";
		}
	}
	free(buf);
	if (bad == NULL && !(have_dist && have_window && have_bins))
		bad = "dist, window and bins are required";
	if (bad == NULL && pc_share_parse(getenv("POLYCAP_SPOT_SHARE"), &r->share) != NULL)
		bad = "POLYCAP_SPOT_SHARE must be a fraction in (0, 1]";
	if (bad != NULL)
		return bad;
	r->spec.n_planes = r->n_dist;
	r->spec.distances = r->dist;
	r->spec.n_energies = r->n_energies;
	r->spec.energies = r->energies;
	return pc_hip_spot_validate(&r->spec, n_energies) == PC_HIP_OK ? NULL : pc_hip_reason(why);
}

/* POLYCAP_HIST; an empty value counts as set, and is refused */
static const char *pc_hist_request_parse(struct pc_hist_request *r, const char *value, size_t n_energies, char *why)
{
	if (value == NULL)
		return NULL;
	r->set = 1;
	char *buf = strdup(value), *save = NULL;
	const char *bad = NULL;
	for (char *item = strtok_r(buf, ";", &save); item != NULL && bad == NULL; item = strtok_r(NULL, ";", &save)) {
		if (strncmp(item, "axis=", 5) == 0) {
			if (r->n_axes >= 17) { bad = "at most 16 axes"; break; }
			bad = pc_parse_axis(item, &r->axes[r->n_axes++], 10);
		} else if (strncmp(item, "energies=", 9) == 0) {
			bad = pc_parse_energies(item + 9, n_energies, &r->energies, &r->n_energies);
		} else {
			bad = "every item must be an axis (axis=NAME,...) or energies=";
		}
	}
	free(buf);
	if (bad == NULL && r->n_axes == 0)
		bad = "at least one axis is needed";
	if (bad != NULL)
		return bad;
	r->spec.n_axes = r->n_axes;
	r->spec.axes = r->axes;
	r->spec.n_energies = r->n_energies;
	r->spec.energies = r->energies;
	return pc_hip_hist_validate(&r->spec, n_energies) == PC_HIP_OK ? NULL : pc_hip_reason(why);
}

/* POLYCAP_JOINT, and the value of pc_hip_joint_parse; an empty value counts as set, and is refused.  The reason names the item */
static const char *pc_joint_request_parse(struct pc_joint_request *r, const char *value, size_t n_energies, char *why)
{
	if (value == NULL)
		return NULL;
	r->set = 1;
	char *buf = strdup(value), *save = NULL;
	const char *bad = NULL;
	int n_item = 0;
	for (char *item = strtok_r(buf, ";", &save); item != NULL && bad == NULL; item = strtok_r(NULL, ";", &save), n_item++) {
		if (strncmp(item, "axis=", 5) == 0) {
			char *star = strchr(item, '*');
			if (r->n_pairs >= 9) { bad = "at most 8 pairs"; break; }
			if (star == NULL || strncmp(star + 1, "axis=", 5) != 0 || strchr(star + 1, '*') != NULL)
				bad = "a pair must be two axes joined by '*' (axis=NAME,...*axis=NAME,...)";
			else {
				*star = '\0';
				pc_hip_joint_pair *pr = &r->pairs[r->n_pairs++];
				bad = pc_parse_axis(item, &pr->u, 12);
				if (bad == NULL)
					bad = pc_parse_axis(star + 1, &pr->v, 12);
			}
		} else if (strncmp(item, "energies=", 9) == 0) {
			bad = pc_parse_energies(item + 9, n_energies, &r->energies, &r->n_energies);
		} else {
			bad = "every item must be a pair (axis=NAME,...*axis=NAME,...) or energies=";
		}
		if (bad != NULL) {
			snprintf(why, PC_WHY, "item %d: %s", n_item, bad);
			bad = why;
		}
	}
	free(buf);
	if (bad == NULL && r->n_pairs == 0)
		bad = "at least one pair is needed";
	if (bad != NULL)
		return bad;
	r->spec.n_pairs = r->n_pairs;
	r->spec.pairs = r->pairs;
	r->spec.n_energies = r->n_energies;
	r->spec.energies = r->energies;
	return pc_hip_joint_validate(&r->spec, n_energies) == PC_HIP_OK ? NULL : pc_hip_reason(why);
}

int pc_hip_joint_parse(const char *value, size_t n_energies, pc_hip_joint_pair *pairs, int32_t *n_pairs, int32_t *energies, int32_t *n_selected,
	char *why, size_t why_len)
{
	struct pc_joint_request r;
	char reason[PC_WHY];
	memset(&r, 0, sizeof(r));
	const char *bad = value != NULL ? pc_joint_request_parse(&r, value, n_energies, reason) : "value must not be NULL";
	if (why != NULL && why_len > 0)
		snprintf(why, why_len, "%s", bad != NULL ? bad : "");
	if (bad == NULL) {
		if (pairs != NULL) memcpy(pairs, r.pairs, sizeof(pc_hip_joint_pair)*(size_t)r.n_pairs);
		if (n_pairs != NULL) *n_pairs = r.n_pairs;
		if (energies != NULL && r.n_energies > 0) memcpy(energies, r.energies, sizeof(int32_t)*(size_t)r.n_energies);
		if (n_selected != NULL) *n_selected = r.n_energies;
	}
	free(r.energies);
	return bad == NULL ? PC_HIP_OK : PC_HIP_ERR_INVALID;
}

/* POLYCAP_SELECT_RECORDS */
static const char *pc_records_parse(const char *value, int64_t *records)
{
	if (value == NULL)
		return NULL;
	char *end = NULL;
	errno = 0;
	const long long v = strtoll(value, &end, 10);
	if (end == value || *end != '\0' || errno != 0 || v < 1 || v > 2147483647ll)
		return "must be an integer in 1 .. 2^31 - 1";
	*records = (int64_t)v;
	return NULL;
}

/* POLYCAP_SELECT: the grammar is pc_hip_select_parse's; an empty value counts as set, and is refused */
static const char *pc_select_request_parse(struct pc_select_request *r, const char *value, char *why)
{
	if (value == NULL)
		return NULL;
	if (pc_hip_select_parse(value, r->cuts, &r->n_cuts, why, PC_WHY) != PC_HIP_OK)
		return why;
	r->set = 1;
	r->spec.n_cuts = r->n_cuts;
	r->spec.cuts = r->cuts;
	return NULL;
}

/* POLYCAP_DRAW: n=N[,energy=INDEX][,phase=UINT32]; an empty value is refused.  The reason names the item */
static const char *pc_draw_request_parse(struct pc_draw_request *r, const char *value, size_t ne, char *why)
{
	if (value == NULL)
		return NULL;
	int have_n = 0;
	if (*value == '\0')
		return "the value is empty: n=N[,energy=INDEX][,phase=UINT32] is needed";
	for (const char *at = value; ; ) {
		const char *comma = strchr(at, ',');
		const size_t len = comma != NULL ? (size_t)(comma - at) : strlen(at);
		char item[64];
		if (len >= sizeof item) {
			snprintf(why, PC_WHY, "item %.40s...: unknown key (n, energy, phase)", at);
			return why;
		}
		memcpy(item, at, len);
		item[len] = '\0';
		char *eq = strchr(item, '=');
		char *end = NULL;
		errno = 0;
		const long long v = eq != NULL ? strtoll(eq + 1, &end, 10) : 0;
		const int number = eq != NULL && end != eq + 1 && *end == '\0' && errno == 0;
		if (eq != NULL)
			*eq = '\0';
		if (eq == NULL || (strcmp(item, "n") != 0 && strcmp(item, "energy") != 0 && strcmp(item, "phase") != 0)) {
			snprintf(why, PC_WHY, "item %s: unknown key (n, energy, phase)", item);
			return why;
		}
		if (strcmp(item, "n") == 0) {
			if (!number || v < 1 || v > 2147483647ll) {
				snprintf(why, PC_WHY, "n=%s: must be an integer in 1 .. 2^31 - 1", eq + 1);
				return why;
			}
			r->n = (int64_t)v;
			have_n = 1;
		} else if (strcmp(item, "energy") == 0) {
			if (!number || v < 0 || v >= (long long)ne) {
				snprintf(why, PC_WHY, "energy=%s: must be an index into the source's %zu energies", eq + 1, ne);
				return why;
			}
			r->energy = (int32_t)v;
		} else {
			if (!number || v < 0 || v > 4294967295ll) {
				snprintf(why, PC_WHY, "phase=%s: must be a uint32", eq + 1);
				return why;
			}
			r->phase = (uint32_t)v;
		}
		if (comma == NULL)
			break;
		at = comma + 1;
	}
	if (!have_n)
		return "n is missing: the size of the sample, n=N";
	r->set = 1;
	return NULL;
}

void pc_run_request_free(struct pc_run_request *r)
{
	free(r->spot.energies);
	free(r->hist.energies);
	free(r->joint.energies);
}

/* Top to bottom the order of validation: the first variable that is refused answers.  Numbers that do not parse fall back to their
 * defaults; out-of-range option values fail when the option is set. */
int pc_run_request_parse(struct pc_run_request *r, size_t ne, int leak_calc, int n_photons, polycap_error **error)
{
	char why[PC_WHY], draw_why[PC_WHY];
	memset(r, 0, sizeof(*r));
	r->timing = getenv("POLYCAP_TIMING") != NULL;
	if (pc_refused(error, "POLYCAP_STDERR", pc_flag_parse(getenv("POLYCAP_STDERR"), &r->stderr_on))) return -1;
	if (pc_refused(error, "POLYCAP_TALLY_STDERR", pc_flag_parse(getenv("POLYCAP_TALLY_STDERR"), &r->tally_stderr_on))) return -1;
	if (pc_refused(error, "POLYCAP_BEAM", pc_flag_parse(getenv("POLYCAP_BEAM"), &r->beam_on))) return -1;
	if (pc_refused(error, "POLYCAP_SPOT", pc_spot_request_parse(&r->spot, getenv("POLYCAP_SPOT"), ne, why))) return -1;
	if (pc_refused(error, "POLYCAP_HIST", pc_hist_request_parse(&r->hist, getenv("POLYCAP_HIST"), ne, why))) return -1;
	if (pc_refused(error, "POLYCAP_JOINT", pc_joint_request_parse(&r->joint, getenv("POLYCAP_JOINT"), ne, why))) return -1;
	if (pc_refused(error, "POLYCAP_SELECT_RECORDS", pc_records_parse(getenv("POLYCAP_SELECT_RECORDS"), &r->select.records))) return -1;
	if (r->select.records > 0 && getenv("POLYCAP_SELECT") == NULL) {
		polycap_set_error(error, POLYCAP_ERROR_INVALID_ARGUMENT, PC_CALL "POLYCAP_SELECT_RECORDS=%s needs POLYCAP_SELECT: there is no selection to take the rows from",
			getenv("POLYCAP_SELECT_RECORDS"));
		return -1;
	}
	if (pc_refused(error, "POLYCAP_SELECT", pc_select_request_parse(&r->select, getenv("POLYCAP_SELECT"), why))) return -1;
	/* POLYCAP_DRAW is read here, for the selection it may need, and refused last: behind every other variable's refusal */
	const char *draw_bad = pc_draw_request_parse(&r->draw, getenv("POLYCAP_DRAW"), ne, draw_why);
	if (draw_bad == NULL && r->draw.set && !r->select.set) {      /* no POLYCAP_SELECT: every entry passes, a reflection count in [0, 2^62) */
		r->draw.implicit = 1;
		r->select.cuts[0].axis = (pc_hip_hist_axis){ .quantity = PC_HIP_HIST_N_REFL, .lo = 0., .hi = 4611686018427387904., .n_bins = 1 };
		r->select.n_cuts = r->select.spec.n_cuts = 1;
		r->select.spec.cuts = r->select.cuts;
		r->select.set = 1;
	}
	/* POLYCAP_SPOT_SHARE covers the chunked runs of beam moments, (joint) histograms and selections too: without POLYCAP_SPOT it is
	 * read here, and refused under its own name */
	if ((r->beam_on || r->hist.set || r->joint.set || r->select.set) && !r->spot.set
	    && pc_refused(error, "POLYCAP_SPOT_SHARE", pc_share_parse(getenv("POLYCAP_SPOT_SHARE"), &r->spot.share))) return -1;
	if (pc_env_devices(r->devices, &r->n_devices, error) != 0) return -1;
	const char *img_env = getenv("POLYCAP_IMAGES");
	r->keep_images = !(img_env != NULL && strcmp(img_env, "0") == 0);
	if (leak_calc && !r->keep_images) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, PC_CALL "POLYCAP_IMAGES=0 cannot be combined with leak_calc (leak events are per-photon data)");
		return -1;
	}
	/* big plain runs are traced in four parts so that the images of a finished part cross PCIe while the next part runs */
	r->run_parts = (!leak_calc && r->keep_images && n_photons >= 2000000) ? (int)pc_env_u64("POLYCAP_RUN_PARTS", 4, NULL) : 1;
	/* Plain runs store their exit photons in the order of completion (option "compact_images": coalesced plane stores, blocks
	 * copied to the host while the kernel runs); the reference's own order is the order in which randomly seeded threads fill
	 * the arrays.  POLYCAP_COMPACT=0 keeps every photon at the position of its slot (reproducible order for a given POLYCAP_SEED). */
	const char *compact_env = getenv("POLYCAP_COMPACT");
	r->compact = !(compact_env != NULL && strcmp(compact_env, "0") == 0) && !leak_calc;
	r->have_block_shift = getenv("POLYCAP_BLOCK_SHIFT") != NULL;
	r->block_shift = (int64_t)pc_env_u64("POLYCAP_BLOCK_SHIFT", 18, NULL);
	const char *rccl = getenv("POLYCAP_RCCL");
	r->rccl = (rccl != NULL && *rccl != '\0') ? atoi(rccl) : -1;
	r->max_attempts = (uint32_t)pc_env_u64("POLYCAP_MAX_ATTEMPTS", 1u << 20, NULL);
	r->seed = pc_env_u64("POLYCAP_SEED", 0, &r->have_seed);
	return pc_refused(error, "POLYCAP_DRAW", draw_bad);
}

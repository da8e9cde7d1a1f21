/*
 * pc_source.c -- polycap_source: X-ray source + optic + energy grid, and the photon-loop driver.
 *
 * API and error behaviour of the reference's src/polycap-source.c:
 *   polycap_source_new :147-225, polycap_source_new_from_file :228-445 (legacy positional .inp deck),
 *   polycap_source_get_photon :23-144, polycap_source_get_transmission_efficiencies :448-1087,
 *   polycap_source_free / polycap_source_get_description :1090-1109.
 * The photon loop (the reference's OpenMP region :697-1049) runs on the GPU: this file only validates,
 * uploads the problem once, enqueues pc_hip_transmission_run for the n_photons exit-photon slots and copies
 * the image planes back.  Photon streams are Philox(seed, slot, attempt): the reference seeds one mt19937 per
 * OpenMP thread from /dev/urandom, so its runs are not reproducible; here POLYCAP_SEED fixes the key.
 */
#define _GNU_SOURCE
#include "pc_private.h"
#include "pc_exact.h"

#include <errno.h>
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

polycap_source *polycap_source_new(polycap_description *description, double d_source, double src_x, double src_y,
	double src_sigx, double src_sigy, double src_shiftx, double src_shifty, double hor_pol,
	size_t n_energies, double *energies, polycap_error **error)
{
	if (description == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: description cannot be NULL");
		return NULL;
	}
	if (d_source <= 0.) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: d_source must be greater than 0");
		return NULL;
	}
	if (src_x <= 0.) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: src_x must be greater than 0");
		return NULL;
	}
	if (src_y <= 0.) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: src_y must be greater than 0");
		return NULL;
	}
	if (fabs(hor_pol) > 1.) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: hor_pol must be greater than or equal to -1 and smaller than or equal to 1");
		return NULL;
	}
	if (n_energies <= 0.) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: n_energies must be greater than 0");
		return NULL;
	}
	if (energies == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: energies cannot be NULL");
		return NULL;
	}
	for (size_t i = 0; i < n_energies; i++) {
		if (energies[i] < 1. || energies[i] > 100.) {
			polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: energies must be greater than 1 and smaller than 100");
			return NULL;
		}
	}
	if (polycap_profile_validate(description->profile, description->n_cap, error) != 1) {
		polycap_clear_error(error);
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: description->profile is faulty. Some capillary coordinates are outside of the external radius.");
		return NULL;
	}

	polycap_source *source = calloc(1, sizeof(polycap_source));
	if (source != NULL)
		source->energies = malloc(sizeof(double)*n_energies);
	if (source == NULL || source->energies == NULL) {
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_source_new: could not allocate memory for source -> %s", strerror(errno));
		polycap_source_free(source);
		return NULL;
	}
	source->d_source = d_source;
	source->src_x = src_x;
	source->src_y = src_y;
	source->src_sigx = src_sigx;
	source->src_sigy = src_sigy;
	source->src_shiftx = src_shiftx;
	source->src_shifty = src_shifty;
	source->hor_pol = hor_pol;
	source->n_energies = n_energies;
	memcpy(source->energies, energies, sizeof(double)*n_energies);
	source->rng = polycap_rng_new();
	/* the source keeps its own deep copy of the description (tests free the original right away) */
	source->description = polycap_description_new(description->profile, description->sig_rough, description->n_cap,
		description->nelem, description->iz, description->wi, description->density, NULL);
	if (source->description == NULL) {
		polycap_clear_error(error);
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new: description->profile is faulty. Some capillary coordinates are outside of the external radius.");
		polycap_source_free(source);
		return NULL;
	}
	return source;
}

/* opens `name`; a relative name that does not exist in the working directory is retried next to the .inp deck */
static char *pc_resolve_near(const char *deck, const char *name)
{
	FILE *probe = fopen(name, "r");
	if (probe != NULL) {
		fclose(probe);
		return strdup(name);
	}
	const char *slash = strrchr(deck, '/');
	if (name[0] == '/' || slash == NULL)
		return strdup(name);
	size_t dirlen = (size_t)(slash - deck) + 1;
	char *joined = malloc(dirlen + strlen(name) + 1);
	if (joined == NULL)
		return NULL;
	memcpy(joined, deck, dirlen);
	strcpy(joined + dirlen, name);
	return joined;
}

polycap_source *polycap_source_new_from_file(const char *filename, polycap_error **error)
{
	if (filename == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new_from_file: filename cannot be NULL");
		return NULL;
	}
	polycap_description *description = calloc(1, sizeof(polycap_description));
	polycap_source *source = calloc(1, sizeof(polycap_source));
	if (description == NULL || source == NULL) {
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_source_new_from_file: could not allocate memory for source -> %s", strerror(errno));
		free(description);
		free(source);
		return NULL;
	}
	source->description = description;
	source->rng = polycap_rng_new();

	FILE *fptr = fopen(filename, "r");
	if (fptr == NULL) {
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_source_new_from_file: could not open %s -> %s", filename, strerror(errno));
		polycap_source_free(source);
		return NULL;
	}

	/* positional deck, reference src/polycap-source.c:273-369 */
	double e_start = 0., e_final = 0., delta_e = 1.;
	int nphotons = 0, type = 0;
	int ok = 1;
	ok &= fscanf(fptr, "%lf", &description->sig_rough) == 1;
	ok &= fscanf(fptr, "%lf", &source->d_source) == 1;
	ok &= fscanf(fptr, "%lf %lf", &source->src_x, &source->src_y) == 2;
	ok &= fscanf(fptr, "%lf %lf", &source->src_sigx, &source->src_sigy) == 2;
	ok &= fscanf(fptr, "%lf %lf", &source->src_shiftx, &source->src_shifty) == 2;
	ok &= fscanf(fptr, "%lf", &source->hor_pol) == 1;
	ok &= fscanf(fptr, "%u", &description->nelem) == 1;
	if (!ok || description->nelem < 1 || description->nelem > 111) {
		fclose(fptr);
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_source_new_from_file: could not read the source/composition header of %s", filename);
		polycap_source_free(source);
		return NULL;
	}
	description->iz = malloc(sizeof(int)*description->nelem);
	description->wi = malloc(sizeof(double)*description->nelem);
	if (description->iz == NULL || description->wi == NULL) {
		fclose(fptr);
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_source_new_from_file: could not allocate memory for description->iz -> %s", strerror(errno));
		polycap_source_free(source);
		return NULL;
	}
	for (unsigned int i = 0; i < description->nelem; i++) {
		ok &= fscanf(fptr, "%d %lf", &description->iz[i], &description->wi[i]) == 2;
		description->wi[i] /= 100.0;
	}
	ok &= fscanf(fptr, "%lf", &description->density) == 1;
	ok &= fscanf(fptr, "%lf %lf %lf", &e_start, &e_final, &delta_e) == 3;
	if (!ok) {
		fclose(fptr);
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_source_new_from_file: could not read composition/energies from %s", filename);
		polycap_source_free(source);
		return NULL;
	}
	source->n_energies = (size_t)((e_final-e_start)/delta_e + 1);
	if (source->n_energies <= 0. || source->n_energies > 100000000u) {
		fclose(fptr);
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new_from_file: source->n_energies must be greater than 0");
		polycap_source_free(source);
		return NULL;
	}
	source->energies = malloc(sizeof(double)*source->n_energies);
	if (source->energies == NULL) {
		fclose(fptr);
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_source_new_from_file: could not allocate memory for source->energies -> %s", strerror(errno));
		polycap_source_free(source);
		return NULL;
	}
	for (size_t i = 0; i < source->n_energies; i++)
		source->energies[i] = e_start + i*delta_e;
	ok &= fscanf(fptr, "%d", &nphotons) == 1;   /* read and ignored, as in the reference (:343) */
	ok &= fscanf(fptr, "%d", &type) == 1;
	if (ok && (type == 0 || type == 1 || type == 2)) {
		double length, rad_ext_upstream, rad_ext_downstream, rad_int_upstream, rad_int_downstream, focal_dist_upstream, focal_dist_downstream;
		if (fscanf(fptr, "%lf %lf %lf %lf %lf %lf %lf", &length, &rad_ext_upstream, &rad_ext_downstream, &rad_int_upstream,
		           &rad_int_downstream, &focal_dist_upstream, &focal_dist_downstream) != 7) {
			fclose(fptr);
			polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_source_new_from_file: could not read the profile shape from %s", filename);
			polycap_source_free(source);
			return NULL;
		}
		description->profile = polycap_profile_new((polycap_profile_type)type, length, rad_ext_upstream, rad_ext_downstream,
			rad_int_upstream, rad_int_downstream, focal_dist_upstream, focal_dist_downstream, error);
	} else if (ok) {
		fgetc(fptr); /* rest of the "type" line */
		char *names[3] = { NULL, NULL, NULL };
		for (int k = 0; k < 3; k++) {
			char *raw = polycap_read_input_line(fptr, NULL);
			names[k] = raw ? pc_resolve_near(filename, raw) : NULL;
			free(raw);
		}
		if (names[0] && names[1] && names[2])
			description->profile = polycap_profile_new_from_file(names[0], names[1], names[2], error);
		for (int k = 0; k < 3; k++)
			free(names[k]);
	}
	if (!ok || description->profile == NULL) {
		fclose(fptr);
		if (error != NULL && *error == NULL)
			polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_source_new_from_file: could not read the profile section of %s", filename);
		polycap_source_free(source);
		return NULL;
	}
	if (fscanf(fptr, "%" SCNd64, &description->n_cap) != 1)
		description->n_cap = 0;
	fclose(fptr);

	polycap_description_check_weight(description->nelem, description->wi, error);

	double n_cap = (pc_n_shells(description->n_cap)+0.5)*6.;
	n_cap = (n_cap*n_cap+3)/12;
	description->open_area = (description->profile->cap[0]*description->profile->cap[0]*M_PI)*n_cap/(3.*sin(M_PI/3)*description->profile->ext[0]*description->profile->ext[0]);

	/* sanity checks of the reference, :380-437 */
	const char *problem = NULL;
	if (source->d_source < 0.0) problem = "polycap_source_new_from_file: source_temp->d_source must be greater than 0.0";
	else if (source->src_x < 0.0) problem = "polycap_source_new_from_file: source_temp->src_x must be greater than 0.0";
	else if (source->src_y < 0.0) problem = "polycap_source_new_from_file: source_temp->src_y must be greater than 0.0";
	else if (description->n_cap < 1) problem = "polycap_source_new_from_file: description->n_cap must be greater than 1";
	else if (description->open_area < 0 || description->open_area > 1) problem = "polycap_source_new_from_file: description->open_area must be greater than 0 and less than 1";
	else if (description->density < 0.0) problem = "polycap_source_new_from_file: description->density must be greater than 0.0";
	for (size_t i = 0; problem == NULL && i < source->n_energies; i++)
		if (source->energies[i] < 1. || source->energies[i] > 100.)
			problem = "polycap_source_new_from_file: source->energies must be greater than 1 and smaller than 100";
	for (unsigned int i = 0; problem == NULL && i < description->nelem; i++)
		if (description->iz[i] < 1 || description->iz[i] > 94)
			problem = "polycap_source_new_from_file: description->iz[i] must be greater than 0 and less than 94";
	if (problem != NULL) {
		polycap_clear_error(error);
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, problem);
		polycap_source_free(source);
		return NULL;
	}
	if (polycap_profile_validate(description->profile, description->n_cap, error) != 1) {
		polycap_clear_error(error);
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_new_from_file: description->profile is faulty. Some capillary coordinates are outside of the external radius.");
		polycap_source_free(source);
		return NULL;
	}
	return source;
}

/* One photon of the stream (rng->seed, photon index rng->counter++), sampled by the device sampler. */
polycap_photon *polycap_source_get_photon(polycap_source *source, polycap_rng *rng, polycap_error **error)
{
	if (source == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_get_photon: source cannot be NULL");
		return NULL;
	}
	polycap_description *description = source->description;
	if (description == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_get_photon: description cannot be NULL");
		return NULL;
	}
	if (rng == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_get_photon: rng cannot be NULL");
		return NULL;
	}
	pc_hip_ctx *ctx = pc_ctx_for(&source->cache, description, source->n_energies, source->energies, source, "polycap_source_get_photon", error);
	if (ctx == NULL)
		return NULL;
	int64_t slot = (int64_t)(rng->counter++ & 0x7fffffffffffffffull);
	uint32_t attempt = 0;
	double out[12];
	int status = pc_hip_sample_photons(ctx, rng->seed, 1, &slot, &attempt, out);
	if (status != PC_HIP_OK) {
		pc_set_hip_error(error, "polycap_source_get_photon", status);
		return NULL;
	}
	polycap_vector3 start_coords = { out[0], out[1], out[2] };
	polycap_vector3 start_direction = { out[3], out[4], out[5] };
	polycap_vector3 start_electric_vector = { out[6], out[7], out[8] };
	polycap_photon *photon = polycap_photon_new(description, start_coords, start_direction, start_electric_vector, error);
	if (photon == NULL)
		return NULL;
	photon->src_start_coords.x = out[9];
	photon->src_start_coords.y = out[10];
	photon->src_start_coords.z = 0.;
	return photon;
}

/* POLYCAP_TIMING=1: stage times of polycap_source_get_transmission_efficiencies on stderr */
static double pc_now_ms(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec*1e3 + ts.tv_nsec*1e-6;
}

/* the tallies of one call and the selection they are filled through (any may be NULL); tot: the selection's totals summed over the
 * applies of the call, n_pass [3], n_seen [3], then passed_w [3][ne], rejected_w [3][ne] */
struct pc_tallies {
	pc_hip_spot *spot[3];          /* exit photons, extleak, intleak */
	pc_hip_beam *beam;
	pc_hip_hist *hist;
	pc_hip_joint *joint;
	pc_hip_select *select;
	int64_t sel_n[6];
	uint64_t *sel_w;               /* [2][3][ne] */
	int squares;                   /* POLYCAP_TALLY_STDERR=1: every tally and the selection track squares */
	uint64_t *sel_w2;              /* [2][3][ne][2] with squares: passed_w2, rejected_w2 summed over the applies with carry */
	/* POLYCAP_SELECT_RECORDS: the first rec_limit passing entries per kind over the applies of the call (pc_hip_select_gather) */
	int64_t rec_limit;
	int rec_applied[3];
	int64_t rec_n[3];
	double *rec[3];                /* [rec_n][PC_HIP_N_PLANES or PC_HIP_LEAK_HDR, + ne] */
	int64_t *rec_pos[3];           /* positions in the concatenation of what the applies saw */
	/* POLYCAP_DRAW: the draws of every kind (pc_hip_select_draw); a kind is applied once, a draw needs all its entries on the device */
	struct pc_draw_request draw;
	int draw_chunked;              /* the run would have been traced as several slot ranges: refused */
	int draw_applied[3];
	int64_t draw_rows[3];
	uint64_t draw_total[3];
	double *draw_rec[3];
	int64_t *draw_pos[3];
};

/* every tally of the call and its selection track squares: before the first add and the first apply */
static int pc_tallies_track_squares(struct pc_tallies *ta, size_t ne)
{
	int st = PC_HIP_OK;
	ta->squares = 1;
	if (ta->select != NULL) {
		ta->sel_w2 = calloc(12*ne, sizeof(uint64_t));
		st = ta->sel_w2 == NULL ? PC_HIP_ERR_MEMORY : pc_hip_select_track_squares(ta->select);
	}
	for (int kind = 0; kind <= 2 && st == PC_HIP_OK; kind++)
		if (ta->spot[kind] != NULL)
			st = pc_hip_spot_track_squares(ta->spot[kind]);
	if (st == PC_HIP_OK && ta->hist != NULL)
		st = pc_hip_hist_track_squares(ta->hist);
	if (st == PC_HIP_OK && ta->joint != NULL)
		st = pc_hip_joint_track_squares(ta->joint);
	return st;
}

static void *pc_beam_dup(const void *p, size_t bytes);

/* the entries of `kind` of the last run into every tally, through the selection if there is one (applied here, its totals added) */
static int pc_tallies_add(struct pc_tallies *ta, int kind, size_t ne)
{
	int st = PC_HIP_OK;
	pc_hip_select *s = ta->select;
	if (s != NULL) {
		int64_t n_pass[3], n_seen[3];
		uint64_t *w = malloc(sizeof(uint64_t)*6*ne);
		st = (w != NULL) ? pc_hip_select_apply(s, kind) : PC_HIP_ERR_MEMORY;
		if (st == PC_HIP_OK)
			st = pc_hip_select_read(s, n_pass, n_seen, w, w + 3*ne);
		if (st == PC_HIP_OK && ta->rec_limit > 0) {
			/* the rows of what passed, as long as the limit has room: only they leave the device */
			const size_t row = (size_t)(kind == 0 ? PC_HIP_N_PLANES : PC_HIP_LEAK_HDR) + ne;
			const int64_t have = ta->rec_n[kind], room = ta->rec_limit - have, take = n_pass[kind] < room ? n_pass[kind] : room;
			ta->rec_applied[kind] = 1;
			if (take > 0) {
				double *rec = realloc(ta->rec[kind], sizeof(double)*row*(size_t)(have + take));
				if (rec != NULL)
					ta->rec[kind] = rec;
				int64_t *pos = realloc(ta->rec_pos[kind], sizeof(int64_t)*(size_t)(have + take));
				if (pos != NULL)
					ta->rec_pos[kind] = pos;
				st = (rec != NULL && pos != NULL) ? pc_hip_select_gather(s, kind, 0, take, rec + row*(size_t)have, pos + have) : PC_HIP_ERR_MEMORY;
				for (int64_t k = 0; st == PC_HIP_OK && k < take; k++)
					pos[have + k] += ta->sel_n[3 + kind];      /* behind the entries the earlier applies saw */
				if (st == PC_HIP_OK)
					ta->rec_n[kind] = have + take;
			}
		}
		if (st == PC_HIP_OK && ta->draw.set) {
			/* the sample of this kind; one without weight at that energy carries no rows */
			const size_t row = (size_t)(kind == 0 ? PC_HIP_N_PLANES : PC_HIP_LEAK_HDR) + ne;
			const int64_t n = ta->draw.n;
			ta->draw_applied[kind] = 1;
			ta->draw_total[kind] = w[kind*ne + (size_t)ta->draw.energy];
			if (ta->draw_total[kind] > 0) {
				ta->draw_rec[kind] = malloc(sizeof(double)*row*(size_t)n);
				ta->draw_pos[kind] = malloc(sizeof(int64_t)*(size_t)n);
				st = (ta->draw_rec[kind] != NULL && ta->draw_pos[kind] != NULL)
				   ? pc_hip_select_draw(s, kind, ta->draw.energy, n, ta->draw.phase, 0, n, ta->draw_rec[kind], ta->draw_pos[kind], NULL) : PC_HIP_ERR_MEMORY;
				if (st == PC_HIP_OK)
					ta->draw_rows[kind] = n;
			}
		}
		if (st == PC_HIP_OK) {
			ta->sel_n[kind] += n_pass[kind];
			ta->sel_n[3 + kind] += n_seen[kind];
			for (size_t e = 0; e < ne; e++) {
				ta->sel_w[kind*ne + e] += w[kind*ne + e];
				ta->sel_w[(3 + kind)*ne + e] += w[(3 + kind)*ne + e];
			}
		}
		free(w);
		if (st == PC_HIP_OK && ta->squares) {
			uint64_t *w2 = malloc(sizeof(uint64_t)*12*ne);
			st = (w2 != NULL) ? pc_hip_select_read_squares(s, w2, w2 + 6*ne) : PC_HIP_ERR_MEMORY;
			if (st == PC_HIP_OK) {
				pc_exact_add_pairs(ta->sel_w2 + 2*kind*ne, w2 + 2*kind*ne, ne);
				pc_exact_add_pairs(ta->sel_w2 + 6*ne + 2*kind*ne, w2 + 6*ne + 2*kind*ne, ne);
			}
			free(w2);
		}
	}
	if (st == PC_HIP_OK && ta->spot[kind] != NULL)
		st = s != NULL ? pc_hip_spot_add_selected(ta->spot[kind], kind, s) : pc_hip_spot_add(ta->spot[kind], kind);
	if (st == PC_HIP_OK && ta->beam != NULL)
		st = s != NULL ? pc_hip_beam_add_selected(ta->beam, kind, s) : pc_hip_beam_add(ta->beam, kind);
	if (st == PC_HIP_OK && ta->hist != NULL)
		st = s != NULL ? pc_hip_hist_add_selected(ta->hist, kind, s) : pc_hip_hist_add(ta->hist, kind);
	if (st == PC_HIP_OK && ta->joint != NULL)
		st = s != NULL ? pc_hip_joint_add_selected(ta->joint, kind, s) : pc_hip_joint_add(ta->joint, kind);
	return st;
}

/* POLYCAP_IMAGES=0 with spot maps, beam moments, histograms or joint histograms on one context: the exit data of the run stay on the device, and a run whose exit
 * data would take more than the stated share of the device's memory is traced as consecutive slot ranges (photons are keyed by
 * (seed, slot): the same photons).  Counters and the exact fixed-point sums of the ranges are added on the host, and every range is
 * added to the map, to the beam sums, to the histograms and to the joint histograms (any may be NULL).  fixed [2*ne] receives the weights' sums; fixed2 (NULL unless
 * POLYCAP_STDERR) those of the squared weights. */
static int pc_spot_chunked(pc_hip_ctx *ctx, struct pc_tallies *ta, uint64_t seed, int64_t n_photons, int64_t chunk, uint32_t max_attempts,
	size_t ne, double *sum_weights, int64_t counters[6], uint64_t *fixed, uint64_t *fixed2)
{
	uint64_t *part = malloc(2*ne*sizeof(uint64_t));
	int st = (part != NULL) ? PC_HIP_OK : PC_HIP_ERR_MEMORY;
	memset(fixed, 0, 2*ne*sizeof(uint64_t));
	if (fixed2 != NULL)
		memset(fixed2, 0, 2*ne*sizeof(uint64_t));
	for (int k = 0; k < 6; k++)
		counters[k] = 0;
	for (int64_t lo = 0; lo < n_photons && st == PC_HIP_OK; lo += chunk) {
		const int64_t n = (n_photons - lo < chunk) ? n_photons - lo : chunk;
		int64_t c[6];
		st = pc_hip_transmission_run(ctx, seed, lo, n, max_attempts, 1);
		if (st == PC_HIP_OK)
			st = pc_tallies_add(ta, 0, ne);      /* through POLYCAP_SELECT if it is set */
		if (st == PC_HIP_OK)
			st = pc_hip_transmission_totals(ctx, NULL, c, part);
		if (st != PC_HIP_OK)
			break;
		for (int k = 0; k < 6; k++)
			counters[k] += c[k];
		pc_exact_add_pairs(fixed, part, ne);      /* 128-bit (lo, hi) sums */
		if (fixed2 != NULL) {
			st = pc_hip_transmission_moments(ctx, part);
			if (st != PC_HIP_OK)
				break;
			pc_exact_add_pairs(fixed2, part, ne);
		}
	}
	for (size_t e = 0; st == PC_HIP_OK && e < ne; e++)
		sum_weights[e] = pc_hip_fixed_to_double(fixed[2*e], fixed[2*e + 1]);
	free(part);
	return st;
}

/* the maps of `spot` in efficiency units into the result.  A failure after eff->spot was created leaves the maps stored so far
 * (and the plane distances and energy selection) in it: polycap_transmission_efficiencies_free frees them with the result. */
static int pc_spot_store(polycap_transmission_efficiencies *eff, pc_hip_spot *spot, const struct pc_spot_request *r, int kind)
{
	int32_t dims[4];
	int st = pc_hip_spot_info(spot, dims, NULL);
	if (st != PC_HIP_OK)
		return st;
	const size_t n_out = (size_t)dims[0]*dims[1], nb = (size_t)dims[2]*dims[3];
	struct pc_spot_result *sp = eff->spot;
	if (sp == NULL) {
		sp = eff->spot = calloc(1, sizeof(*sp));
		if (sp == NULL)
			return PC_HIP_ERR_MEMORY;
		sp->n_planes = dims[0]; sp->n_sel = dims[1]; sp->ny = dims[2]; sp->nx = dims[3];
		sp->distances = malloc(sizeof(double)*dims[0]);
		sp->sel = malloc(sizeof(int32_t)*dims[1]);
		if (sp->distances == NULL || sp->sel == NULL)
			return PC_HIP_ERR_MEMORY;
		memcpy(sp->distances, r->dist, sizeof(double)*dims[0]);
		for (int32_t k = 0; k < dims[1]; k++)
			sp->sel[k] = r->n_energies ? r->energies[k] : k;
		sp->window[0] = r->spec.x0; sp->window[1] = r->spec.x1; sp->window[2] = r->spec.y0; sp->window[3] = r->spec.y1;
	}
	uint64_t *bins = malloc(sizeof(uint64_t)*n_out*nb), *out = malloc(sizeof(uint64_t)*n_out);
	double *map = malloc(sizeof(double)*n_out*nb), *outside = malloc(sizeof(double)*n_out);
	st = (bins != NULL && out != NULL && map != NULL && outside != NULL) ? pc_hip_spot_read(spot, bins, out, NULL) : PC_HIP_ERR_MEMORY;
	if (st == PC_HIP_OK && eff->tally_n_started > 0) {      /* POLYCAP_TALLY_STDERR: the sums behind the maps, and their squares */
		struct pc_squares_result *sq = &sp->sq[kind];
		sq->n_cells = n_out*nb; sq->n_outside = n_out; sq->owns_sums = 1;
		sq->sums = pc_beam_dup(bins, sizeof(uint64_t)*n_out*nb);
		sq->outside = pc_beam_dup(out, sizeof(uint64_t)*n_out);
		sq->squares = malloc(sizeof(uint64_t)*2*n_out*nb);
		sq->outside_squares = malloc(sizeof(uint64_t)*2*n_out);
		st = (sq->sums != NULL && sq->outside != NULL && sq->squares != NULL && sq->outside_squares != NULL)
		   ? pc_hip_spot_read_squares(spot, sq->squares, sq->outside_squares) : PC_HIP_ERR_MEMORY;
	}
	for (size_t m = 0; st == PC_HIP_OK && m < n_out; m++) {
		/* map = efficiency[e] * S_bin / (S_inside + S_outside): a map and its outside part sum to the efficiency */
		uint64_t total = out[m];
		for (size_t b = 0; b < nb; b++)
			total += bins[m*nb + b];
		const double eff_e = eff->efficiencies[sp->sel[m % (size_t)dims[1]]];
		const double tot = (double)total;
		for (size_t b = 0; b < nb; b++)
			map[m*nb + b] = total ? eff_e * (double)bins[m*nb + b] / tot : 0.;
		outside[m] = total ? eff_e * (double)out[m] / tot : 0.;
	}
	if (st == PC_HIP_OK) {
		sp->maps[kind] = map; sp->outside[kind] = outside;
		map = outside = NULL;
	}
	free(bins); free(out); free(map); free(outside);
	return st;
}

static void *pc_beam_dup(const void *p, size_t bytes)
{
	void *q = malloc(bytes ? bytes : 1);
	if (q != NULL && bytes)
		memcpy(q, p, bytes);
	return q;
}

/* the exact beam sums of every kind the run has (exit photons; leak runs also extleak and intleak) into the result */
static int pc_beam_store(polycap_transmission_efficiencies *eff, pc_hip_beam *beam, int leak_calc)
{
	const size_t ne = eff->n_energies, per_kind = ne*PC_HIP_BEAM_NSUMS*2;
	struct pc_beam_result *br = eff->beam = calloc(1, sizeof(*br));
	uint64_t *sums = malloc(sizeof(uint64_t)*3*per_kind), *out = malloc(sizeof(uint64_t)*3*ne);
	int st = (br != NULL && sums != NULL && out != NULL) ? pc_hip_beam_read(beam, sums, out, br->n_entries) : PC_HIP_ERR_MEMORY;
	for (int kind = 0; kind <= (leak_calc ? 2 : 0) && st == PC_HIP_OK; kind++) {
		br->sums[kind] = pc_beam_dup(sums + kind*per_kind, sizeof(uint64_t)*per_kind);
		br->outside[kind] = pc_beam_dup(out + kind*ne, sizeof(uint64_t)*ne);
		if (br->sums[kind] == NULL || br->outside[kind] == NULL)
			st = PC_HIP_ERR_MEMORY;
	}
	free(sums);
	free(out);
	return st;
}

/* the squares of one kind of a histogram or joint result beside its own sums (not owned) */
static int pc_squares_store(struct pc_squares_result *sq, size_t n_cells, size_t n_outside, uint64_t *sums, uint64_t *outside,
	const uint64_t *squares, const uint64_t *outside_squares)
{
	sq->n_cells = n_cells; sq->n_outside = n_outside;
	sq->sums = sums; sq->outside = outside; sq->owns_sums = 0;
	sq->squares = pc_beam_dup(squares, sizeof(uint64_t)*2*n_cells);
	sq->outside_squares = pc_beam_dup(outside_squares, sizeof(uint64_t)*2*n_outside);
	return (sq->squares != NULL && sq->outside_squares != NULL) ? PC_HIP_OK : PC_HIP_ERR_MEMORY;
}

/* the exact histograms of every kind the run has into the result */
static int pc_hist_store(polycap_transmission_efficiencies *eff, pc_hip_hist *hist, const struct pc_hist_request *r, int leak_calc)
{
	int32_t dims[3];
	int st = pc_hip_hist_info(hist, dims, NULL, NULL);
	if (st != PC_HIP_OK)
		return st;
	const size_t na = (size_t)dims[0], ns = (size_t)dims[1], tb = (size_t)dims[2];
	struct pc_hist_result *hr = eff->hist = calloc(1, sizeof(*hr));
	if (hr == NULL)
		return PC_HIP_ERR_MEMORY;
	hr->n_axes = dims[0]; hr->n_sel = dims[1]; hr->total_bins = dims[2];
	hr->axes = pc_beam_dup(r->axes, sizeof(pc_hip_hist_axis)*na);
	hr->offsets = malloc(sizeof(int32_t)*(na + 1));
	hr->sel = malloc(sizeof(int32_t)*(ns ? ns : 1));
	uint64_t *bins = malloc(sizeof(uint64_t)*3*ns*tb), *out = malloc(sizeof(uint64_t)*3*na*ns);
	if (hr->axes == NULL || hr->offsets == NULL || hr->sel == NULL || bins == NULL || out == NULL)
		st = PC_HIP_ERR_MEMORY;
	if (st == PC_HIP_OK)
		st = pc_hip_hist_info(hist, dims, hr->offsets, NULL);
	if (st == PC_HIP_OK)
		st = pc_hip_hist_read(hist, bins, out, hr->n_entries);
	for (size_t k = 0; st == PC_HIP_OK && k < ns; k++)
		hr->sel[k] = r->n_energies ? r->energies[k] : (int32_t)k;
	for (int kind = 0; kind <= (leak_calc ? 2 : 0) && st == PC_HIP_OK; kind++) {
		hr->bins[kind] = pc_beam_dup(bins + kind*ns*tb, sizeof(uint64_t)*ns*tb);
		hr->outside[kind] = pc_beam_dup(out + kind*na*ns, sizeof(uint64_t)*na*ns);
		if (hr->bins[kind] == NULL || hr->outside[kind] == NULL)
			st = PC_HIP_ERR_MEMORY;
	}
	free(bins);
	free(out);
	if (st == PC_HIP_OK && eff->tally_n_started > 0) {      /* POLYCAP_TALLY_STDERR */
		uint64_t *sq = malloc(sizeof(uint64_t)*2*3*ns*tb), *osq = malloc(sizeof(uint64_t)*2*3*na*ns);
		st = (sq != NULL && osq != NULL) ? pc_hip_hist_read_squares(hist, sq, osq) : PC_HIP_ERR_MEMORY;
		for (int kind = 0; kind <= (leak_calc ? 2 : 0) && st == PC_HIP_OK; kind++)
			st = pc_squares_store(&hr->sq[kind], ns*tb, na*ns, hr->bins[kind], hr->outside[kind], sq + 2*kind*ns*tb, osq + 2*kind*na*ns);
		free(sq);
		free(osq);
	}
	return st;
}

/* the exact joint histograms of every kind the run has into the result */
static int pc_joint_store(polycap_transmission_efficiencies *eff, pc_hip_joint *joint, const struct pc_joint_request *r, int leak_calc)
{
	int32_t dims[3];
	int st = pc_hip_joint_info(joint, dims, NULL, NULL);
	if (st != PC_HIP_OK)
		return st;
	const size_t np = (size_t)dims[0], ns = (size_t)dims[1], tc = (size_t)dims[2];
	struct pc_joint_result *jr = eff->joint = calloc(1, sizeof(*jr));
	if (jr == NULL)
		return PC_HIP_ERR_MEMORY;
	jr->n_pairs = dims[0]; jr->n_sel = dims[1]; jr->total_cells = dims[2];
	jr->pairs = pc_beam_dup(r->pairs, sizeof(pc_hip_joint_pair)*np);
	jr->offsets = malloc(sizeof(int32_t)*(np + 1));
	jr->sel = malloc(sizeof(int32_t)*(ns ? ns : 1));
	uint64_t *cells = malloc(sizeof(uint64_t)*3*ns*tc), *out = malloc(sizeof(uint64_t)*3*np*ns);
	if (jr->pairs == NULL || jr->offsets == NULL || jr->sel == NULL || cells == NULL || out == NULL)
		st = PC_HIP_ERR_MEMORY;
	if (st == PC_HIP_OK)
		st = pc_hip_joint_info(joint, dims, jr->offsets, NULL);
	if (st == PC_HIP_OK)
		st = pc_hip_joint_read(joint, cells, out, jr->n_entries);
	for (size_t k = 0; st == PC_HIP_OK && k < ns; k++)
		jr->sel[k] = r->n_energies ? r->energies[k] : (int32_t)k;
	for (int kind = 0; kind <= (leak_calc ? 2 : 0) && st == PC_HIP_OK; kind++) {
		jr->cells[kind] = pc_beam_dup(cells + kind*ns*tc, sizeof(uint64_t)*ns*tc);
		jr->outside[kind] = pc_beam_dup(out + kind*np*ns, sizeof(uint64_t)*np*ns);
		if (jr->cells[kind] == NULL || jr->outside[kind] == NULL)
			st = PC_HIP_ERR_MEMORY;
	}
	free(cells);
	free(out);
	if (st == PC_HIP_OK && eff->tally_n_started > 0) {      /* POLYCAP_TALLY_STDERR */
		uint64_t *sq = malloc(sizeof(uint64_t)*2*3*ns*tc), *osq = malloc(sizeof(uint64_t)*2*3*np*ns);
		st = (sq != NULL && osq != NULL) ? pc_hip_joint_read_squares(joint, sq, osq) : PC_HIP_ERR_MEMORY;
		for (int kind = 0; kind <= (leak_calc ? 2 : 0) && st == PC_HIP_OK; kind++)
			st = pc_squares_store(&jr->sq[kind], ns*tc, np*ns, jr->cells[kind], jr->outside[kind], sq + 2*kind*ns*tc, osq + 2*kind*np*ns);
		free(sq);
		free(osq);
	}
	return st;
}

/* the argument checks of the reference call, in its order: the message of the first one that fails, or NULL */
static const char *pc_transmission_args_bad(const polycap_source *source, const polycap_progress_monitor *progress_monitor, int n_photons)
{
	if (source == NULL)
		return "source cannot be NULL";
	if (progress_monitor != NULL)
		return "progress_monitor must be NULL as polycap_progress_monitor currently has no implementation";
	if (source->description == NULL)
		return "description cannot be NULL";
	if (source->n_energies < 1)
		return "source->n_energies must be greater than or equal to 1";
	if (source->energies == NULL)
		return "source->energies cannot be NULL";
	for (size_t i = 0; i < source->n_energies; i++)
		if (source->energies[i] < 1. || source->energies[i] > 100.)
			return "source->energies[i] must be greater than 1 and less than 100";
	return n_photons < 1 ? "n_photons must be greater than 1" : NULL;
}

/* where a run goes: one device or a device group, exactly one of them set (both belong to the source's context cache) */
struct pc_target {
	pc_hip_ctx *ctx;
	pc_hip_group *group;
};

/* Trace stage: with POLYCAP_SPOT the maps are made first (exit photons; leak runs also extleak and intleak), with POLYCAP_BEAM the
 * beam sums, with POLYCAP_HIST the histograms, with POLYCAP_JOINT the joint histograms, then the options are set and the run is
 * enqueued.  *chunked = 1 when pc_spot_chunked traced the run: it also read the totals and moments, and added every range to spot[0],
 * *beam, *hist and *joint. */
static int pc_trace(struct pc_target t, const struct pc_run_request *r, int leak_calc, uint64_t seed, int64_t n_photons, size_t ne,
	struct pc_tallies *ta, int *chunked, double *sum_weights, int64_t counters[6], uint64_t *fixed, uint64_t *fixed2)
{
	int st = PC_HIP_OK;
	int64_t chunk = 0;
	pc_hip_spot **spot = ta->spot;
	pc_hip_beam **beam = &ta->beam;
	pc_hip_hist **hist = &ta->hist;
	pc_hip_joint **joint = &ta->joint;
	if (r->select.set) {
		ta->sel_w = calloc(6*ne, sizeof(uint64_t));
		ta->rec_limit = r->select.records;
		ta->draw = r->draw;
		st = ta->sel_w == NULL ? PC_HIP_ERR_MEMORY
		   : t.group != NULL ? pc_hip_group_select_create(t.group, &r->select.spec, &ta->select) : pc_hip_select_create(t.ctx, &r->select.spec, &ta->select);
	}
	if (r->spot.set)
		for (int kind = 0; kind <= (leak_calc ? 2 : 0) && st == PC_HIP_OK; kind++)
			st = t.group != NULL ? pc_hip_group_spot_create(t.group, &r->spot.spec, &spot[kind]) : pc_hip_spot_create(t.ctx, &r->spot.spec, &spot[kind]);
	if (r->beam_on && st == PC_HIP_OK)
		st = t.group != NULL ? pc_hip_group_beam_create(t.group, beam) : pc_hip_beam_create(t.ctx, beam);
	if (r->hist.set && st == PC_HIP_OK)
		st = t.group != NULL ? pc_hip_group_hist_create(t.group, &r->hist.spec, hist) : pc_hip_hist_create(t.ctx, &r->hist.spec, hist);
	if (r->joint.set && st == PC_HIP_OK)
		st = t.group != NULL ? pc_hip_group_joint_create(t.group, &r->joint.spec, joint) : pc_hip_joint_create(t.ctx, &r->joint.spec, joint);
	if (r->tally_stderr_on && st == PC_HIP_OK)
		st = pc_tallies_track_squares(ta, ne);
	if (r->spot.set || r->beam_on || r->hist.set || r->joint.set || r->select.set) {
		/* POLYCAP_IMAGES=0 with spot maps, beam moments or (joint) histograms is chunked on one device only: a group traces the whole run at once */
		if (st == PC_HIP_OK && t.group == NULL && !r->keep_images && !leak_calc) {
			uint64_t total_b = 0;
			st = pc_hip_device_memory(t.ctx, NULL, &total_b);
			chunk = (int64_t)(r->spot.share * (double)total_b / ((17. + (double)ne) * 8.));
			if (chunk < 1)
				chunk = 1;
		}
	}
	/* the context or group is cached, so every option is set on every call */
	const struct { const char *name; int64_t value; int set; } opt[] = {
		{ "run_parts", r->run_parts, 1 },
		{ "weight_squares", r->stderr_on, 1 },
		{ "compact_images", r->compact, 1 },
		{ "block_shift", r->block_shift, r->have_block_shift && t.group == NULL },    /* one device only */
		{ "plane_images", leak_calc ? 0 : 1, 1 },      /* the result object wants planes: let the kernel write them */
	};
	for (size_t k = 0; k < sizeof(opt)/sizeof(opt[0]) && st == PC_HIP_OK; k++)
		if (opt[k].set)
			st = t.group != NULL ? pc_hip_group_set_option(t.group, opt[k].name, opt[k].value) : pc_hip_set_option(t.ctx, opt[k].name, opt[k].value);
	if (st != PC_HIP_OK)
		return st;
	if (chunk > 0 && chunk < n_photons && r->draw.set) {      /* a draw needs the exit data of the whole run on the device at once */
		ta->draw_chunked = 1;
		return PC_HIP_ERR_INVALID;
	}
	if (chunk > 0 && chunk < n_photons) {
		*chunked = 1;
		return pc_spot_chunked(t.ctx, ta, seed, n_photons, chunk, r->max_attempts, ne, sum_weights, counters, fixed, fixed2);
	}
	/* POLYCAP_SPOT, POLYCAP_BEAM, POLYCAP_HIST, POLYCAP_JOINT: the run keeps its exit data on the device even with POLYCAP_IMAGES=0 (then nothing is copied back) */
	const int device_images = r->keep_images || r->spot.set || r->beam_on || r->hist.set || r->joint.set || r->select.set;
	if (leak_calc)
		return t.group != NULL ? pc_hip_group_run_leak(t.group, seed, n_photons, r->max_attempts, 1)
		                       : pc_hip_transmission_run_leak(t.ctx, seed, 0, n_photons, r->max_attempts, 1);
	return t.group != NULL ? pc_hip_group_run(t.group, seed, n_photons, r->max_attempts, device_images)
	                       : pc_hip_transmission_run(t.ctx, seed, 0, n_photons, r->max_attempts, device_images);
}

/* Image stage, while the kernel is still running; *t_prefault = the time the prefault ended */
static int pc_fetch_images(struct pc_target t, polycap_transmission_efficiencies *eff, int64_t n_photons, double *t_prefault)
{
	pc_transeff_prefault(eff, (size_t)n_photons);    /* the kernel is running: fault the result pages in meanwhile */
	*t_prefault = pc_now_ms();
	pc_hip_images dst;
	pc_transeff_plane_pointers(eff, &dst);
	if (t.group != NULL)
		return pc_hip_group_images(t.group, &dst);
	/* One device only: a result in one slab stays pinned while it lives and in the pool after it (pc_transeff.c); planes of their
	 * own are pinned for the call only */
	const int keep_pinned = eff->images->slab != NULL;
	if (keep_pinned)
		(void)pc_hip_set_option(t.ctx, "keep_pinned", 1);
	const int st = pc_hip_transmission_images(t.ctx, 0, n_photons, &dst);    /* block by block behind the kernel (a leak run: after it) */
	if (keep_pinned) {
		(void)pc_hip_set_option(t.ctx, "keep_pinned", 0);
		pc_transeff_planes_pinned(eff);      /* also after a failure: what the fetch pinned stays pinned until the slab is freed */
	}
	return st;
}

polycap_transmission_efficiencies *polycap_source_get_transmission_efficiencies(polycap_source *source, int max_threads, int n_photons,
	bool leak_calc, polycap_progress_monitor *progress_monitor, polycap_error **error)
{
	(void)max_threads; /* host-thread cap in the reference (:492-493); the photon loop runs on the GPU here */
	const char *bad = pc_transmission_args_bad(source, progress_monitor, n_photons);
	if (bad != NULL) {
		polycap_set_error(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_get_transmission_efficiencies: %s", bad);
		return NULL;
	}

	/* everything owned starts empty; every failure below sets the error once and goes to `out`, which frees what is set */
	const size_t ne = source->n_energies;
	struct pc_run_request req;
	struct pc_target t = { NULL, NULL };
	polycap_transmission_efficiencies *eff = NULL, *result = NULL;
	double *sum_weights = NULL;
	uint64_t *sum_fixed = NULL, *sum_fixed2 = NULL;      /* the exact moments A and B; B and the result's copy only with POLYCAP_STDERR */
	struct pc_tallies ta;                                /* POLYCAP_SPOT, _BEAM, _HIST, _JOINT and the POLYCAP_SELECT they are filled through */
	memset(&ta, 0, sizeof(ta));
	pc_hip_spot **spot = ta.spot;
	int64_t counters[6] = { 0, 0, 0, 0, 0, 0 };
	int status = PC_HIP_OK, chunked = 0, reduced_by = 0;      /* a failed HIP call: its error is set at `out` */
	double t_stage[6];

	if (pc_run_request_parse(&req, ne, leak_calc, n_photons, error) != 0)
		goto out;
	t_stage[0] = pc_now_ms();
	eff = pc_transeff_alloc(source, req.keep_images ? (size_t)n_photons : 0, 0, "polycap_source_get_transmission_efficiencies", error);
	if (eff == NULL)
		goto out;
	sum_weights = malloc(sizeof(double)*ne);
	sum_fixed = malloc(sizeof(uint64_t)*2*ne);
	sum_fixed2 = req.stderr_on ? malloc(sizeof(uint64_t)*2*ne) : NULL;
	if (sum_weights == NULL || sum_fixed == NULL || (req.stderr_on && sum_fixed2 == NULL)) {
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_source_get_transmission_efficiencies: could not allocate memory for efficiencies -> %s", strerror(errno));
		goto out;
	}

	if (req.n_devices > 1 || (req.n_devices > 0 && !leak_calc))      /* leak runs are sharded like plain runs (reference :744-884, 925-1032) */
		t.group = pc_group_for(&source->cache, source->description, ne, source->energies, source, req.n_devices, req.devices,
		                       "polycap_source_get_transmission_efficiencies", error);
	else      /* a one-entry list selects the device of a leak run; none: POLYCAP_HIP_DEVICE, default 0 */
		t.ctx = pc_ctx_for_device(&source->cache, source->description, ne, source->energies, source, req.n_devices >= 1 ? req.devices[0] : -1,
		                          "polycap_source_get_transmission_efficiencies", error);
	if (t.ctx == NULL && t.group == NULL)
		goto out;
	t_stage[1] = pc_now_ms();
	/* the run index moves only once a device was obtained: the seeds of all later runs depend on it */
	const uint64_t seed = req.have_seed ? req.seed : source->rng->seed + 0x9E3779B97F4A7C15ull * source->run_index;
	source->run_index++;

	status = pc_trace(t, &req, leak_calc, seed, n_photons, ne, &ta, &chunked, sum_weights, counters, sum_fixed, sum_fixed2);
	t_stage[2] = t_stage[3] = pc_now_ms();
	if (status == PC_HIP_OK && req.keep_images)
		status = pc_fetch_images(t, eff, n_photons, &t_stage[3]);
	t_stage[4] = pc_now_ms();
	if (status == PC_HIP_OK && !chunked && t.group != NULL) {
		status = pc_hip_group_totals(t.group, req.rccl, sum_weights, counters, req.stderr_on ? sum_fixed : NULL, &reduced_by, NULL);
		if (status == PC_HIP_OK && req.stderr_on)
			status = pc_hip_group_moments(t.group, sum_fixed2);
	} else if (status == PC_HIP_OK && !chunked) {
		status = pc_hip_transmission_wait(t.ctx, NULL);      /* one device: the run has finished before its totals are read */
		if (status == PC_HIP_OK)
			status = pc_hip_transmission_totals(t.ctx, sum_weights, counters, req.stderr_on ? sum_fixed : NULL);
		if (status == PC_HIP_OK && req.stderr_on)
			status = pc_hip_transmission_moments(t.ctx, sum_fixed2);
	}
	t_stage[5] = pc_now_ms();
	if (req.timing)
		fprintf(stderr, "polycap timing [ms]: alloc+context %.1f, enqueue %.1f, prefault %.1f, images (incl. waiting for the kernel) %.1f, totals %.1f%s\n",
			t_stage[1] - t_stage[0], t_stage[2] - t_stage[1], t_stage[3] - t_stage[2], t_stage[4] - t_stage[3], t_stage[5] - t_stage[4],
			t.group != NULL ? (reduced_by ? " (devices summed by RCCL all-reduce)" : " (devices summed on the host)") : "");
	if (status == PC_HIP_OK && leak_calc)
		status = pc_transeff_fetch_leaks(eff, t.ctx, t.group);      /* reference :925-1032 */
	pc_hip_beam *beam = ta.beam;
	pc_hip_hist *hist = ta.hist;
	pc_hip_joint *joint = ta.joint;
	for (int kind = chunked ? 1 : 0; kind <= (leak_calc ? 2 : 0) && status == PC_HIP_OK; kind++)      /* a chunked run has added its exit photons */
		status = pc_tallies_add(&ta, kind, ne);
	if (status != PC_HIP_OK)
		goto out;

	/* totals, summary lines and efficiency formula of the reference, :1055-1076 */
	const polycap_description *description = source->description;
	int64_t sum_iexit = counters[0], sum_not_entered = counters[1], sum_not_transmitted = counters[2], sum_irefl = counters[3];
	printf("Average number of reflections: %lf, Simulated photons: %" PRId64 "\n", (double)sum_irefl/n_photons, sum_iexit+sum_not_entered+sum_not_transmitted);
	printf("Open area Calculated: %lf, Simulated: %lf\n",
		((pc_n_shells(description->n_cap)+0.5)*6.)*((pc_n_shells(description->n_cap)+0.5)*6.)/12.*(description->profile->cap[0]*description->profile->cap[0]*M_PI)/(3.*sin(M_PI/3)*description->profile->ext[0]*description->profile->ext[0]),
		(double)(sum_iexit+sum_not_transmitted)/(sum_iexit+sum_not_entered+sum_not_transmitted));
	printf("iexit: %" PRId64 ", no enter: %" PRId64 ", no trans: %" PRId64 "\n", sum_iexit, sum_not_entered, sum_not_transmitted);
	pc_transeff_finish(eff, sum_weights, counters);
	eff->synthetic_constants = source->cache.synthetic;
	eff->tally_n_started = req.tally_stderr_on ? counters[0] + counters[1] + counters[2] : 0;
	for (int kind = 0; kind <= 2 && status == PC_HIP_OK; kind++)
		if (spot[kind] != NULL)
			status = pc_spot_store(eff, spot[kind], &req.spot, kind);
	if (status == PC_HIP_OK && beam != NULL)
		status = pc_beam_store(eff, beam, leak_calc);
	if (status == PC_HIP_OK && hist != NULL)
		status = pc_hist_store(eff, hist, &req.hist, leak_calc);
	if (status == PC_HIP_OK && joint != NULL)
		status = pc_joint_store(eff, joint, &req.joint, leak_calc);
	if (status == PC_HIP_OK && ta.draw.set) {
		struct pc_draw_result *dr = eff->draw = calloc(1, sizeof(*dr));
		if (dr == NULL)
			status = PC_HIP_ERR_MEMORY;
		else {
			dr->n = ta.draw.n; dr->energy = ta.draw.energy; dr->phase = ta.draw.phase;
			for (int kind = 0; kind <= 2; kind++) {      /* the result owns the rows from here on */
				dr->applied[kind] = ta.draw_applied[kind];
				dr->rows[kind] = ta.draw_rows[kind];
				dr->row[kind] = (int32_t)((kind == 0 ? PC_HIP_N_PLANES : PC_HIP_LEAK_HDR) + ne);
				dr->total[kind] = ta.draw_total[kind];
				dr->rec[kind] = ta.draw_rec[kind]; dr->pos[kind] = ta.draw_pos[kind];
				ta.draw_rec[kind] = NULL; ta.draw_pos[kind] = NULL;
			}
		}
	}
	if (status == PC_HIP_OK && ta.select != NULL && !ta.draw.implicit) {
		struct pc_select_result *sr = eff->select = calloc(1, sizeof(*sr));
		if (sr == NULL)
			status = PC_HIP_ERR_MEMORY;
		else {
			sr->n_cuts = req.select.n_cuts;
			memcpy(sr->cuts, req.select.cuts, sizeof(sr->cuts));
			memcpy(sr->n_pass, ta.sel_n, sizeof(sr->n_pass));
			memcpy(sr->n_seen, ta.sel_n + 3, sizeof(sr->n_seen));
			sr->passed_w = pc_beam_dup(ta.sel_w, sizeof(uint64_t)*3*ne);
			sr->rejected_w = pc_beam_dup(ta.sel_w + 3*ne, sizeof(uint64_t)*3*ne);
			if (sr->passed_w == NULL || sr->rejected_w == NULL)
				status = PC_HIP_ERR_MEMORY;
			sr->rec_limit = ta.rec_limit;
			for (int kind = 0; kind <= 2; kind++) {      /* the result owns the rows from here on */
				sr->rec_applied[kind] = ta.rec_applied[kind];
				sr->rec_n[kind] = ta.rec_n[kind];
				sr->rec_row[kind] = (int32_t)((kind == 0 ? PC_HIP_N_PLANES : PC_HIP_LEAK_HDR) + ne);
				sr->rec[kind] = ta.rec[kind]; sr->rec_pos[kind] = ta.rec_pos[kind];
				ta.rec[kind] = NULL; ta.rec_pos[kind] = NULL;
			}
			if (status == PC_HIP_OK && ta.sel_w2 != NULL) {      /* POLYCAP_TALLY_STDERR */
				sr->passed_w2 = pc_beam_dup(ta.sel_w2, sizeof(uint64_t)*6*ne);
				sr->rejected_w2 = pc_beam_dup(ta.sel_w2 + 6*ne, sizeof(uint64_t)*6*ne);
				if (sr->passed_w2 == NULL || sr->rejected_w2 == NULL)
					status = PC_HIP_ERR_MEMORY;
			}
		}
	}
	if (status != PC_HIP_OK)
		goto out;
	if (req.stderr_on) {      /* without POLYCAP_STDERR the result keeps no moments, and its stderr and moment getters fail */
		eff->n_started = counters[0] + counters[1] + counters[2];
		eff->stderrs = malloc(sizeof(double)*ne);
		if (eff->stderrs == NULL) {
			polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_source_get_transmission_efficiencies: could not allocate memory for the standard errors -> %s", strerror(errno));
			goto out;
		}
		pc_hip_efficiency_stderr(ne, sum_fixed, sum_fixed2, counters, eff->stderrs);
		eff->sumw_fixed = sum_fixed; eff->sumw2_fixed = sum_fixed2;      /* the result is complete: it owns them from here on */
		sum_fixed = sum_fixed2 = NULL;
	}
	if (!req.keep_images)
		eff->images->i_exit = 0;     /* no per-photon planes were kept: the exit/start getters report no events */
	result = eff;
	eff = NULL;

out:
	if (ta.draw_chunked)
		polycap_set_error(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_source_get_transmission_efficiencies: POLYCAP_DRAW=%s: the exit data of %d photons "
			"exceed POLYCAP_SPOT_SHARE of the device's memory, and a POLYCAP_IMAGES=0 run that is traced as several slot ranges has no one beam to draw from",
			getenv("POLYCAP_DRAW"), n_photons);
	else if (status != PC_HIP_OK)
		pc_set_hip_error(error, "polycap_source_get_transmission_efficiencies", status);
	for (int kind = 0; kind <= 2; kind++)
		pc_hip_spot_destroy(spot[kind]);
	pc_hip_beam_destroy(ta.beam);
	pc_hip_hist_destroy(ta.hist);
	pc_hip_joint_destroy(ta.joint);
	pc_hip_select_destroy(ta.select);
	free(ta.sel_w);
	free(ta.sel_w2);
	for (int kind = 0; kind <= 2; kind++) {
		free(ta.rec[kind]);
		free(ta.rec_pos[kind]);
		free(ta.draw_rec[kind]);
		free(ta.draw_pos[kind]);
	}
	pc_run_request_free(&req);
	free(sum_weights);
	free(sum_fixed);
	free(sum_fixed2);
	polycap_transmission_efficiencies_free(eff);
	return result;
}

void polycap_source_free(polycap_source *source)
{
	if (source == NULL)
		return;
	pc_ctx_cache_clear(&source->cache);
	polycap_description_free(source->description);
	polycap_rng_free(source->rng);
	free(source->energies);
	free(source);
}

const polycap_description *polycap_source_get_description(polycap_source *source)
{
	return source->description;
}

/* Fills *p with the plain-array view of `source` (pointers borrowed from the source, valid while it lives);
 * amu/scatf are computed by the optical-constants provider into caller-owned arrays of n_energies doubles.
 * Used by the Python layer to build problems from .inp decks with the one C parser. Returns 0 on success. */
POLYCAP_EXTERN int pc_source_problem(polycap_source *source, pc_hip_problem *p, double *amu, double *scatf, int *synthetic, polycap_error **error);
int pc_source_problem(polycap_source *source, pc_hip_problem *p, double *amu, double *scatf, int *synthetic, polycap_error **error)
{
	if (source == NULL || p == NULL || source->description == NULL || source->description->profile == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "pc_source_problem: source and p cannot be NULL");
		return -1;
	}
	polycap_description *d = source->description;
	memset(p, 0, sizeof(*p));
	p->nmax = d->profile->nmax;
	p->z = d->profile->z; p->cap = d->profile->cap; p->ext = d->profile->ext;
	p->sig_rough = d->sig_rough; p->n_cap = d->n_cap; p->density = d->density;
	p->n_energies = source->n_energies; p->energies = source->energies;
	p->d_source = source->d_source; p->src_x = source->src_x; p->src_y = source->src_y;
	p->src_sigx = source->src_sigx; p->src_sigy = source->src_sigy;
	p->src_shiftx = source->src_shiftx; p->src_shifty = source->src_shifty; p->hor_pol = source->hor_pol;
	if (amu != NULL && scatf != NULL) {
		if (pc_optconst_scatf(d->nelem, d->iz, d->wi, d->density, source->n_energies, source->energies, amu, scatf, synthetic, error) != 0)
			return -1;
		p->amu = amu; p->scatf = scatf;
	}
	return 0;
}

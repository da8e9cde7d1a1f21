/*
 * pc_private.h -- internal structures of libpolycap's host side (C11).
 *
 * Field meaning follows the reference's src/polycap-private.h:88-181 (profile, description, source,
 * photon, transmission_efficiencies, images); the HIP context handles are additions of this build.
 */
#ifndef PC_PRIVATE_H
#define PC_PRIVATE_H

#include "polycap.h"

#include <stdio.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
#define PC_COSPI_6 0.86602540378443864676

struct _polycap_profile {
	int nmax;          /* arrays hold nmax+1 points */
	double *z;
	double *cap;
	double *ext;
};

/* cached device context for one (description, energy grid, source) combination */
typedef struct {
	pc_hip_ctx *ctx;
	pc_hip_group *group;      /* POLYCAP_HIP_DEVICES: one context per listed device instead of `ctx` */
	int n_devices;
	int devices[64];
	int device;               /* device of `ctx` */
	int synthetic;            /* the optical constants of this context come from the built-in tables away from their pinned points */
	size_t n_energies;
	double *energies;
	int has_source;
	double src[8];
} pc_ctx_cache;

struct _polycap_description {
	double sig_rough;
	int64_t n_cap;
	double open_area;
	unsigned int nelem;
	int *iz;
	double *wi;
	double density;
	polycap_profile *profile;
	pc_ctx_cache cache;   /* used by polycap_photon_launch */
};

struct _polycap_rng {
	uint64_t seed;     /* Philox key */
	uint64_t counter;  /* next photon index of this stream */
};

struct _polycap_source {
	polycap_description *description;
	polycap_rng *rng;
	double d_source;
	double src_x;
	double src_y;
	double src_sigx;
	double src_sigy;
	double src_shiftx;
	double src_shifty;
	double hor_pol;
	size_t n_energies;
	double *energies;
	pc_ctx_cache cache;   /* used by get_photon / get_transmission_efficiencies */
	uint64_t run_index;   /* successive get_transmission_efficiencies calls use distinct Philox keys */
};

struct _polycap_photon {
	polycap_description *description;
	polycap_leak **extleak;
	polycap_leak **intleak;
	int64_t n_extleak;
	int64_t n_intleak;
	polycap_vector3 start_coords;
	polycap_vector3 start_direction;
	polycap_vector3 start_electric_vector;
	polycap_vector3 exit_coords;
	polycap_vector3 exit_direction;
	polycap_vector3 exit_electric_vector;
	polycap_vector3 src_start_coords;
	size_t n_energies;
	double *energies;
	double *weight;
	double *amu;
	double *scatf;
	int64_t i_refl;
	double d_travel;
};

struct _polycap_images {
	/* The 17 planes + the weights of a result with images are ONE allocation ("slab", pc_transeff.c): plane k at
	 * slab + k*slab_stride bytes, in the order of pc_hip_images, the weights last -- so that the device's planes cross PCIe as
	 * one pitched copy per group of blocks and the whole result is pinned in one piece.  NULL: every plane on its own. */
	void *slab;
	size_t slab_stride;
	int64_t i_start;
	int64_t i_exit;
	double *src_start_coords[2];
	double *pc_start_coords[2];
	double *pc_start_dir[2];
	double *pc_start_elecv[2];
	double *pc_exit_coords[3];
	double *pc_exit_dir[2];
	double *pc_exit_elecv[2];
	int64_t *pc_exit_nrefl;
	double *pc_exit_dtravel;
	double *exit_coord_weights;
	/* leak_calc=true: events that left the optic through its side (extleak) or reached the exit plane inside the glass
	 * (intleak); planes of i_extleak / i_intleak entries, weights row-major by event (reference :168-180) */
	int64_t i_extleak;
	int64_t i_intleak;
	double *extleak_coords[3];
	double *extleak_dir[2];
	int64_t *extleak_n_refl;
	double *extleak_coord_weights;
	double *intleak_coords[3];
	double *intleak_dir[2];
	double *intleak_elecv[2];
	int64_t *intleak_n_refl;
	double *intleak_coord_weights;
};

/* extension: what POLYCAP_TALLY_STDERR=1 adds to a tally's result of one kind (pc_transmission_efficiencies_get_tally_squares); all
 * NULL without it.  sums / outside: the exact weight sums the squares belong to (a copy for the spot maps, which keep doubles only;
 * for the other tallies the result's own arrays, not owned) */
struct pc_squares_result {
	size_t n_cells, n_outside;
	uint64_t *sums, *outside;
	int owns_sums;
	uint64_t *squares, *outside_squares;      /* [n_cells][2], [n_outside][2] */
};

/* extension: spot maps of a run made with POLYCAP_SPOT set, in efficiency units (pc_transmission_efficiencies_get_spot) */
struct pc_spot_result {
	int32_t n_planes, n_sel, ny, nx;
	double *distances;         /* [n_planes] cm behind the exit face */
	double window[4];          /* x0, x1, y0, y1, cm */
	int32_t *sel;              /* [n_sel] energy indices */
	double *maps[3];           /* exit photons, extleak, intleak: [plane][energy][iy][ix], NULL when the run has none */
	double *outside[3];        /* [plane][energy] */
	struct pc_squares_result sq[3];
};

/* extension: exact exit-beam sums of a run made with POLYCAP_BEAM=1 (pc_transmission_efficiencies_get_beam / _get_beam_sums) */
struct pc_beam_result {
	uint64_t *sums[3];         /* exit photons, extleak, intleak: [energy][15][2] (lo, hi), NULL when the run has none */
	uint64_t *outside[3];      /* [energy] */
	int64_t n_entries[3];
};

/* extension: exact histograms of a run made with POLYCAP_HIST set (pc_transmission_efficiencies_get_hist) */
struct pc_hist_result {
	int32_t n_axes, n_sel, total_bins;
	pc_hip_hist_axis *axes;    /* [n_axes] */
	int32_t *offsets;          /* [n_axes + 1] */
	int32_t *sel;              /* [n_sel] energy indices */
	uint64_t *bins[3];         /* exit photons, extleak, intleak: [energy][total_bins], NULL when the run has none */
	uint64_t *outside[3];      /* [axis][energy] */
	int64_t n_entries[3];
	struct pc_squares_result sq[3];
};

/* extension: exact joint histograms of a run made with POLYCAP_JOINT set (pc_transmission_efficiencies_get_joint) */
struct pc_joint_result {
	int32_t n_pairs, n_sel, total_cells;
	pc_hip_joint_pair *pairs;  /* [n_pairs] */
	int32_t *offsets;          /* [n_pairs + 1] */
	int32_t *sel;              /* [n_sel] energy indices */
	uint64_t *cells[3];        /* exit photons, extleak, intleak: [energy][total_cells], NULL when the run has none */
	uint64_t *outside[3];      /* [pair][energy] */
	int64_t n_entries[3];
	struct pc_squares_result sq[3];
};

/* extension: the cuts and the exact totals of a run made with POLYCAP_SELECT set (pc_transmission_efficiencies_get_select) */
struct pc_select_result {
	int32_t n_cuts;
	pc_hip_select_cut cuts[8];
	int64_t n_pass[3], n_seen[3];   /* exit photons, extleak, intleak (zeros where the run has none) */
	uint64_t *passed_w, *rejected_w; /* [3][n_energies] */
	uint64_t *passed_w2, *rejected_w2; /* [3][n_energies][2] with POLYCAP_TALLY_STDERR=1, NULL otherwise */
	/* POLYCAP_SELECT_RECORDS=N (pc_transmission_efficiencies_get_select_records): per kind the call applied the selection to, the first
	 * min(N, n_pass) passing entries in order as rows of pc_hip_select_gather and their positions; rec_limit 0: the variable was not set */
	int64_t rec_limit;
	int rec_applied[3];
	int64_t rec_n[3];
	int32_t rec_row[3];             /* doubles per row */
	double *rec[3];                 /* [rec_n][rec_row] */
	int64_t *rec_pos[3];            /* [rec_n] */
};

/* extension: the unweighted sample of a run made with POLYCAP_DRAW set (pc_transmission_efficiencies_get_draw): per kind the call has
 * (exit photons, and extleak and intleak for leak_calc runs) the n draws of pc_hip_select_draw at one energy, none where the kind has
 * no weight there */
struct pc_draw_result {
	int64_t n;                      /* the sample size asked for */
	int32_t energy;                 /* index into the result's energies */
	uint32_t phase;
	int applied[3];
	int64_t rows[3];                /* n, or 0 where total is 0 */
	int32_t row[3];                 /* doubles per row */
	uint64_t total[3];              /* T: the exact sum of the quantised weights drawn from */
	double *rec[3];                 /* [rows][row] */
	int64_t *pos[3];                /* [rows] */
};

struct _polycap_transmission_efficiencies {
	size_t n_energies;
	double *energies;
	double *efficiencies;
	struct _polycap_images *images;
	polycap_source *source;
	int synthetic_constants;   /* extension: see pc_transmission_efficiencies_synthetic */
	struct pc_spot_result *spot;
	struct pc_beam_result *beam;
	struct pc_hist_result *hist;
	struct pc_joint_result *joint;
	struct pc_select_result *select;
	struct pc_draw_result *draw;
	/* extension: the exact moments of a run made with POLYCAP_STDERR=1 (pc_transmission_efficiencies_get_stderr / _get_moments),
	 * NULL otherwise: started photons, (lo, hi) sums of the weights and of the squared weights per energy (include/polycap-hip.h) */
	int64_t n_started;
	uint64_t *sumw_fixed, *sumw2_fixed;
	double *stderrs;           /* [n_energies] pc_hip_efficiency_stderr of the moments */
	int64_t tally_n_started;   /* extension: POLYCAP_TALLY_STDERR=1: counters 0 + 1 + 2 of the call, the N of the tallies' standard errors; 0 otherwise */
};

/* POLYCAP_SPOT, e.g. "dist=0.5,1,2;window=-0.02,0.02,-0.02,0.02;bins=256x256;energies=all" (cm; energy indices into the source's
 * list, or all): spot maps of the run (include/polycap-hip.h, pc_hip_spot_*) */
struct pc_spot_request {
	int set;
	double dist[65];
	int n_dist;
	int32_t *energies;
	int n_energies;
	pc_hip_spot_spec spec;
	double share;              /* POLYCAP_SPOT_SHARE: fraction of the device's memory the exit data of one run may take (0.5) */
};

/* POLYCAP_HIST, e.g. "axis=x,d=0.5,range=-0.01:0.01,bins=2048;axis=r,d=0.5,centre=0:0,range=0:0.02,bins=1024;axis=nrefl,range=0:256,bins=256;energies=all":
 * histograms of the run (include/polycap-hip.h, pc_hip_hist_*).  Items are separated by ';': an axis (comma-separated key=value
 * pairs, the first being axis=NAME) or energies= as in POLYCAP_SPOT */
struct pc_hist_request {
	int set;
	pc_hip_hist_axis axes[17];
	int n_axes;
	int32_t *energies;
	int n_energies;
	pc_hip_hist_spec spec;
};

/* POLYCAP_JOINT, e.g. "axis=x,d=0.5,range=-0.01:0.01,bins=256*axis=slope_x,range=-0.005:0.005,bins=256;axis=start_x,range=-0.3:0.3,bins=512*axis=start_y,range=-0.3:0.3,bins=512;energies=all":
 * joint histograms of the run (include/polycap-hip.h, pc_hip_joint_*).  Items are separated by ';': a pair (two axes of the
 * POLYCAP_HIST grammar joined by '*', u first; start_x and start_y are axes here too) or energies= as in POLYCAP_HIST */
struct pc_joint_request {
	int set;
	pc_hip_joint_pair pairs[9];
	int n_pairs;
	int32_t *energies;
	int n_energies;
	pc_hip_joint_spec spec;
};

/* POLYCAP_SELECT, e.g. "axis=r,d=0.5,centre=0:0,range=0:0.005;axis=nrefl,range=0:40,not": cuts through which every tally of the call is
 * filled (include/polycap-hip.h, pc_hip_select_*; the grammar is pc_hip_select_parse's) */
struct pc_select_request {
	int set;
	pc_hip_select_cut cuts[8];
	int32_t n_cuts;
	pc_hip_select_spec spec;
	int64_t records;               /* POLYCAP_SELECT_RECORDS=N: the result keeps the first N passing entries of every kind; 0: unset */
};

/* POLYCAP_DRAW, e.g. "n=100000,energy=3,phase=12345": the result carries an unweighted sample of n entries per kind, drawn at the
 * energy of that index (default 0) with that phase (default 0: the call stays reproducible) through the call's selection, or through
 * one that every entry passes when POLYCAP_SELECT is not set (include/polycap-hip.h, pc_hip_select_draw) */
struct pc_draw_request {
	int set;
	int implicit;                  /* the selection of the call is the all-pass one made for the draw: the result reports none */
	int64_t n;
	int32_t energy;
	uint32_t phase;
};

/* Everything polycap_source_get_transmission_efficiencies takes from the environment, read by pc_run_request_parse (pc_request.c)
 * before any device is used.  These are extensions of the reference call, all through the environment so that the signature stays
 * the reference's:
 *   POLYCAP_HIP_DEVICES=all | i,j,...  the photon loop is sharded over these devices from this one process (the reference's OpenMP
 *       team, :697-745, becomes a team of GPUs); totals are summed by one RCCL all-reduce (:973-980)
 *   POLYCAP_IMAGES=0                   histogram-only result: efficiencies and counts, no per-photon planes (at 1e8 photons x 291
 *       energies the weight plane alone is 233 GB); the start/exit getters then report no events */
struct pc_run_request {
	int timing;                /* POLYCAP_TIMING: stage times on stderr */
	int tally_stderr_on;       /* POLYCAP_TALLY_STDERR=1: the tallies and the selection of the call track squares; unset or 0: not */
	int stderr_on;             /* POLYCAP_STDERR=1: a standard error per energy (option "weight_squares"); unset or 0: none */
	int beam_on;               /* POLYCAP_BEAM=1: exact exit-beam moments per energy (pc_hip_beam_*); unset or 0: none */
	struct pc_spot_request spot;
	struct pc_hist_request hist;   /* POLYCAP_HIST: exact 1-D histograms per energy (pc_hip_hist_*) */
	struct pc_joint_request joint; /* POLYCAP_JOINT: exact joint 2-D histograms per energy (pc_hip_joint_*) */
	struct pc_select_request select; /* POLYCAP_SELECT: cuts through which every tally is filled (pc_hip_select_*) */
	struct pc_draw_request draw;   /* POLYCAP_DRAW: an unweighted sample of every kind (pc_hip_select_draw) */
	int devices[64], n_devices;
	int keep_images;
	int run_parts;             /* POLYCAP_RUN_PARTS, for big plain runs with images only */
	int compact;               /* POLYCAP_COMPACT, plain runs only */
	int have_block_shift;      /* POLYCAP_BLOCK_SHIFT set (one device only) */
	int64_t block_shift;
	int rccl;                  /* POLYCAP_RCCL: 0 host sum, 1 RCCL or fail, -1 (unset) RCCL when possible */
	uint32_t max_attempts;     /* POLYCAP_MAX_ATTEMPTS */
	int have_seed;             /* POLYCAP_SEED given: seed, else derived from the source */
	uint64_t seed;
};

/* 0, or -1 with the error set; after either, pc_run_request_free frees what the request holds */
int pc_run_request_parse(struct pc_run_request *r, size_t ne, int leak_calc, int n_photons, polycap_error **error);
void pc_run_request_free(struct pc_run_request *r);

/* internal helpers */
char *polycap_read_input_line(FILE *fptr, polycap_error **error);
void polycap_description_check_weight(size_t nelem, double wi[], polycap_error **error);
double pc_n_shells(int64_t n_cap);
int polycap_photon_within_pc_boundary(double polycap_radius, polycap_vector3 photon_coord, polycap_error **error);

/* optical constants (what polycap_photon_scatf computes in the reference, src/polycap-photon.c:22-94) */
POLYCAP_EXTERN int pc_optconst_scatf(unsigned int nelem, const int *iz, const double *wi, double density,
	size_t n_energies, const double *energies, double *amu, double *scatf, int *synthetic, polycap_error **error);
POLYCAP_EXTERN const char *pc_optconst_provider(void);
POLYCAP_EXTERN const char *pc_optconst_library(void);
/* 1 when the efficiencies were computed with optical constants from the built-in tables away from the points the reference's
 * tests pin (no xraylib on the machine); 0 with xraylib or at the pinned points */
POLYCAP_EXTERN int pc_transmission_efficiencies_synthetic(const polycap_transmission_efficiencies *efficiencies);
/* name of the HDF5 shared library bound at run time by the result writer, or "none" */
POLYCAP_EXTERN const char *pc_hdf5_provider(void);

/* result object construction (pc_transeff.c) */
/* zeroed: planes zeroed like calloc's (0: the caller overwrites every entry; planes reused from the pool keep old contents) */
polycap_transmission_efficiencies *pc_transeff_alloc(polycap_source *source, size_t np, int zeroed, const char *caller, polycap_error **error);
void pc_transeff_planes_pinned(polycap_transmission_efficiencies *eff);
POLYCAP_EXTERN void pc_host_pool_clear(void);
POLYCAP_EXTERN int pc_transmission_efficiencies_slab(const polycap_transmission_efficiencies *efficiencies, void **base, size_t *stride);
void pc_transeff_prefault(polycap_transmission_efficiencies *eff, size_t np);
void pc_transeff_plane_pointers(polycap_transmission_efficiencies *eff, pc_hip_images *dst);
void pc_transeff_finish(polycap_transmission_efficiencies *eff, const double *sum_weights, const int64_t counters[6]);
int pc_transeff_fetch_leaks(polycap_transmission_efficiencies *eff, pc_hip_ctx *ctx, pc_hip_group *group);   /* one of ctx / group; returns a pc_hip_status */

/* leak events of the last leak_calc run of `ctx` as polycap_leak lists (pc_photon.c); *list is malloc'd, NULL when empty */
int pc_fetch_leaks(pc_hip_ctx *ctx, int kind, size_t n_energies, polycap_leak ***list, int64_t *n, int64_t **slots,
	const char *caller, polycap_error **error);
void pc_leak_list_free(polycap_leak **list, int64_t n);
bool pc_leak_list_copy(polycap_leak **src, int64_t n_src, polycap_leak ***leaks, int64_t *n_leaks, const char *caller, const char *what,
	polycap_error **error);

/* device context management */
void pc_ctx_cache_clear(pc_ctx_cache *c);
pc_hip_ctx *pc_ctx_for(pc_ctx_cache *c, polycap_description *description, size_t n_energies, const double *energies,
	const polycap_source *source, const char *caller, polycap_error **error);
/* the same on an explicit device (< 0: POLYCAP_HIP_DEVICE, default 0); the cache is keyed on the device too */
pc_hip_ctx *pc_ctx_for_device(pc_ctx_cache *c, polycap_description *description, size_t n_energies, const double *energies,
	const polycap_source *source, int device, const char *caller, polycap_error **error);
/* the same for a device list (POLYCAP_HIP_DEVICES): a group of contexts, one per entry */
pc_hip_group *pc_group_for(pc_ctx_cache *c, polycap_description *description, size_t n_energies, const double *energies,
	const polycap_source *source, int n_devices, const int *devices, const char *caller, polycap_error **error);
void pc_set_hip_error(polycap_error **error, const char *caller, int status);
void pc_spot_result_free(struct pc_spot_result *spot);
void pc_beam_result_free(struct pc_beam_result *beam);
void pc_hist_result_free(struct pc_hist_result *hist);
void pc_joint_result_free(struct pc_joint_result *joint);
void pc_select_result_free(struct pc_select_result *select);
void pc_draw_result_free(struct pc_draw_result *draw);
void pc_squares_result_free(struct pc_squares_result *sq);

#endif

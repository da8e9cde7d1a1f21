/*
 * pc_hdf5.c -- polycap_transmission_efficiencies_write_hdf5: the result file of a transmission run.
 *
 * File layout = what the reference's writer produces (src/polycap-transmission-efficiencies.c:229-780,
 * leak_calc=false): every dataset is native fp64 with a fixed-length string attribute "Units";
 *
 *   /Energies [nE] keV                      /Transmission_Efficiencies [nE] a.u.
 *   /PC_Start/Coordinates|Direction|Electric_Vector [2, i_exit] "[cm,cm]"
 *   /PC_Exit/Coordinates [3, i_exit] "[cm,cm,cm]"   /PC_Exit/Direction|Electric_Vector [2, i_exit] "[cm,cm]"
 *   /PC_Exit/N_Reflections [i_exit] a.u.    /PC_Exit/D_Travel [i_exit] "[cm]"
 *   /PC_Exit/Weights [i_exit, nE] "[keV,a.u.]"
 *   /Source_Start_Coordinates [2, i_exit] "[cm,cm]"
 *   /Input/PC_Shape [2, nmax] (z, ext)   /Input/Cap_Shape [2, nmax] (z, cap)   "[cm,cm]"
 *   /Input/N_Capillaries a.u. | Surface_Roughness Angstrom | Open_Area a.u. | PC_Density g/cm3 | Src_PC_Dist cm   [1]
 *   /Input/PC_Composition [2, nelem] "[Z,w%]"
 *
 *   after a leak_calc run with events of the kind (:518-700), for <G> in ExternalLeaks, InternalLeaks:
 *   /<G>/Coordinates [3, n] "[cm,cm,cm]"   /<G>/Direction [2, n] "[cm,cm]"   /<G>/Weights [n, nE] "[keV,a.u.]"
 *   /<G>/Weight_Total [nE] a.u. (sum of the event weights / started photons)   /<G>/N_Reflections [n] a.u.
 *   /InternalLeaks/Electric_Vector [2, n] "[cm,cm]"
 *
 *   extensions: /Transmission_Efficiencies_StdErr (POLYCAP_STDERR=1), /Spot (POLYCAP_SPOT), and with POLYCAP_BEAM=1, for <K> in Exit,
 *   ExtLeak, IntLeak (the kinds the run has): /Beam/<K>_Sums [nE, 15, 2] uint64, /Beam/<K>_Outside [nE] uint64,
 *   /Beam/<K>_Entries [1] uint64 and /Beam/<K> [nE, 26] fp64 with a "Columns" attribute (include/polycap-hip.h); with POLYCAP_HIST
 *   the groups /Hist/<K>: Axes [n_axes, 8] fp64 (Columns: quantity,d,cx,cy,lo,hi,n_bins,offset), Energies [nS] keV, Bins
 *   [nS, total_bins] and Outside [n_axes, nS] uint64 (the exact sums), Entries [1] uint64, and Efficiency [nS, total_bins] with
 *   Efficiency_Outside [n_axes, nS] fp64: per axis and energy they sum to the efficiency; with POLYCAP_JOINT the groups /Joint/<K>,
 *   shaped alike: Pairs [n_pairs, 15] fp64 (Columns: the seven axis fields of u, those of v, offset), Energies [nS] keV, Cells
 *   [nS, total_cells] (the pairs one after the other, each [iv][iu]) and Outside [n_pairs, nS] uint64, Entries [1] uint64, Efficiency
 *   [nS, total_cells] with Efficiency_Outside [n_pairs, nS] fp64
 *
 * libhdf5 is bound at run time (dlopen), like xraylib in pc_optconst.c, so libpolycap.so carries no link-time
 * dependency on it: hosts without HDF5 get POLYCAP_ERROR_UNSUPPORTED from this one function and nothing else changes.
 * POLYCAP_HDF5_LIB names the library explicitly.
 */
#include "pc_private.h"

#include <dlfcn.h>
#include <errno.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

/* the handful of HDF5 1.10+ ABI types and constants used here (H5public.h, H5Ipublic.h, H5Fpublic.h, H5Spublic.h) */
typedef int64_t pc_hid;
typedef int pc_herr;
typedef unsigned long long pc_hsize;
#define PC_H5P_DEFAULT ((pc_hid)0)
#define PC_H5S_ALL ((pc_hid)0)
#define PC_H5F_ACC_TRUNC 0x0002u
#define PC_H5S_SCALAR 0
#define PC_H5E_DEFAULT ((pc_hid)0)

static struct {
	void *handle;
	int tried;
	pc_herr (*open)(void);
	pc_herr (*get_libversion)(unsigned *, unsigned *, unsigned *);
	pc_herr (*eset_auto2)(pc_hid, void *, void *);
	pc_hid (*fcreate)(const char *, unsigned, pc_hid, pc_hid);
	pc_herr (*fclose)(pc_hid);
	pc_hid (*gcreate2)(pc_hid, const char *, pc_hid, pc_hid, pc_hid);
	pc_herr (*gclose)(pc_hid);
	pc_hid (*screate_simple)(int, const pc_hsize *, const pc_hsize *);
	pc_hid (*screate)(int);
	pc_herr (*sclose)(pc_hid);
	pc_hid (*dcreate2)(pc_hid, const char *, pc_hid, pc_hid, pc_hid, pc_hid, pc_hid);
	pc_herr (*dwrite)(pc_hid, pc_hid, pc_hid, pc_hid, pc_hid, const void *);
	pc_herr (*dclose)(pc_hid);
	pc_hid (*tcopy)(pc_hid);
	pc_herr (*tset_size)(pc_hid, size_t);
	pc_herr (*tclose)(pc_hid);
	pc_hid (*acreate2)(pc_hid, const char *, pc_hid, pc_hid, pc_hid, pc_hid);
	pc_herr (*awrite)(pc_hid, pc_hid, const void *);
	pc_herr (*aclose)(pc_hid);
	pc_hid *native_double;   /* H5T_NATIVE_DOUBLE_g, valid after H5open() */
	pc_hid *native_ullong;   /* H5T_NATIVE_ULLONG_g (the /Beam sums) */
	pc_hid *native_llong;    /* H5T_NATIVE_LLONG_g (the positions of /Select/<Kind>_Records) */
	pc_hid *c_s1;            /* H5T_C_S1_g */
	char name[256];
} h5;
static pthread_mutex_t h5_mutex = PTHREAD_MUTEX_INITIALIZER;

static int pc_h5_bind(void *handle)
{
#define PC_SYM(field, sym) do { *(void **)(&h5.field) = dlsym(handle, sym); if (h5.field == NULL) return 0; } while (0)
	PC_SYM(open, "H5open");
	PC_SYM(get_libversion, "H5get_libversion");
	PC_SYM(eset_auto2, "H5Eset_auto2");
	PC_SYM(fcreate, "H5Fcreate");
	PC_SYM(fclose, "H5Fclose");
	PC_SYM(gcreate2, "H5Gcreate2");
	PC_SYM(gclose, "H5Gclose");
	PC_SYM(screate_simple, "H5Screate_simple");
	PC_SYM(screate, "H5Screate");
	PC_SYM(sclose, "H5Sclose");
	PC_SYM(dcreate2, "H5Dcreate2");
	PC_SYM(dwrite, "H5Dwrite");
	PC_SYM(dclose, "H5Dclose");
	PC_SYM(tcopy, "H5Tcopy");
	PC_SYM(tset_size, "H5Tset_size");
	PC_SYM(tclose, "H5Tclose");
	PC_SYM(acreate2, "H5Acreate2");
	PC_SYM(awrite, "H5Awrite");
	PC_SYM(aclose, "H5Aclose");
	PC_SYM(native_double, "H5T_NATIVE_DOUBLE_g");
	PC_SYM(native_ullong, "H5T_NATIVE_ULLONG_g");
	PC_SYM(native_llong, "H5T_NATIVE_LLONG_g");
	PC_SYM(c_s1, "H5T_C_S1_g");
#undef PC_SYM
	unsigned maj = 0, min = 0, rel = 0;
	/* hid_t is 64-bit from HDF5 1.10 on; older libraries have a different ABI */
	if (h5.get_libversion(&maj, &min, &rel) < 0 || maj != 1 || min < 10)
		return 0;
	if (h5.open() < 0)
		return 0;
	h5.eset_auto2(PC_H5E_DEFAULT, NULL, NULL);   /* errors are reported through polycap_error, not on stderr */
	return 1;
}

static int pc_h5_load(void)
{
	pthread_mutex_lock(&h5_mutex);
	if (!h5.tried) {
		h5.tried = 1;
		const char *env = getenv("POLYCAP_HDF5_LIB");
		const char *candidates[] = { env, "libhdf5.so", "libhdf5_serial.so", "libhdf5.so.310", "libhdf5.so.200", "libhdf5.so.103",
			"libhdf5_serial.so.103", "/opt/conda/lib/libhdf5.so", "/usr/lib/x86_64-linux-gnu/hdf5/serial/libhdf5.so" };
		for (size_t k = 0; k < sizeof(candidates)/sizeof(candidates[0]) && h5.handle == NULL; k++) {
			if (candidates[k] == NULL || candidates[k][0] == '\0')
				continue;
			void *handle = dlopen(candidates[k], RTLD_NOW | RTLD_LOCAL);
			if (handle == NULL)
				continue;
			if (pc_h5_bind(handle)) {
				h5.handle = handle;
				strncpy(h5.name, candidates[k], sizeof(h5.name) - 1);
			} else {
				dlclose(handle);
			}
		}
	}
	int ok = h5.handle != NULL;
	pthread_mutex_unlock(&h5_mutex);
	return ok;
}

const char *pc_hdf5_provider(void)
{
	return pc_h5_load() ? h5.name : "none";
}

/* one string attribute of a dataset */
static bool pc_h5_attr(pc_hid dset, const char *name, const char *value)
{
	pc_hid aspace = -1, atype = -1, attr = -1;
	bool ok = false;
	if ((aspace = h5.screate(PC_H5S_SCALAR)) < 0) goto fail;
	if ((atype = h5.tcopy(*h5.c_s1)) < 0) goto fail;
	if (h5.tset_size(atype, strlen(value)) < 0) goto fail;
	if ((attr = h5.acreate2(dset, name, atype, aspace, PC_H5P_DEFAULT, PC_H5P_DEFAULT)) < 0) goto fail;
	if (h5.awrite(attr, atype, value) < 0) goto fail;
	ok = true;
fail:
	if (attr >= 0 && h5.aclose(attr) < 0) ok = false;
	if (atype >= 0 && h5.tclose(atype) < 0) ok = false;
	if (aspace >= 0 && h5.sclose(aspace) < 0) ok = false;
	return ok;
}

/* extension: one dataset of a native type (uint64 or fp64, non-empty) with its "Units" attribute and, when columns is not NULL, a
 * "Columns" attribute naming the last dimension's entries */
static bool pc_h5_typed(pc_hid file, int rank, const pc_hsize *dim, const char *name, pc_hid type, const void *data, const char *units,
	const char *columns, polycap_error **error)
{
	pc_hid space = -1, dset = -1;
	bool ok = false;
	if ((space = h5.screate_simple(rank, dim, NULL)) < 0) goto fail;
	if ((dset = h5.dcreate2(file, name, type, space, PC_H5P_DEFAULT, PC_H5P_DEFAULT, PC_H5P_DEFAULT)) < 0) goto fail;
	if (h5.dwrite(dset, type, PC_H5S_ALL, PC_H5S_ALL, PC_H5P_DEFAULT, data) < 0) goto fail;
	if (!pc_h5_attr(dset, "Units", units)) goto fail;
	if (columns != NULL && !pc_h5_attr(dset, "Columns", columns)) goto fail;
	ok = true;
fail:
	if (dset >= 0 && h5.dclose(dset) < 0) ok = false;
	if (space >= 0 && h5.sclose(space) < 0) ok = false;
	if (!ok)
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_transmission_efficiencies_write_hdf5: could not write dataset %s", name);
	return ok;
}

/* one fp64 dataset + its "Units" attribute (reference :229-318) */
static bool pc_h5_dataset(pc_hid file, int rank, const pc_hsize *dim, const char *name, const double *data, const char *units,
	polycap_error **error)
{
	pc_hid space = -1, dset = -1, aspace = -1, atype = -1, attr = -1;
	bool ok = false;
	/* HDF5 has no zero-sized simple extents in this usage; an empty run writes one zero instead of failing */
	static const double zero = 0.;
	pc_hsize d[4] = { dim[0], rank > 1 ? dim[1] : 1, rank > 2 ? dim[2] : 1, rank > 3 ? dim[3] : 1 };
	if (rank <= 2 && d[0] * d[1] == 0) {
		d[0] = d[0] ? d[0] : 1;
		d[1] = d[1] ? d[1] : 1;
		if (d[0] * d[1] != 1) {
			polycap_set_error(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_transmission_efficiencies_write_hdf5: dataset %s is empty", name);
			return false;
		}
		data = &zero;
	}
	if ((space = h5.screate_simple(rank, d, NULL)) < 0) goto fail;
	if ((dset = h5.dcreate2(file, name, *h5.native_double, space, PC_H5P_DEFAULT, PC_H5P_DEFAULT, PC_H5P_DEFAULT)) < 0) goto fail;
	if (h5.dwrite(dset, *h5.native_double, PC_H5S_ALL, PC_H5S_ALL, PC_H5P_DEFAULT, data) < 0) goto fail;
	if ((aspace = h5.screate(PC_H5S_SCALAR)) < 0) goto fail;
	if ((atype = h5.tcopy(*h5.c_s1)) < 0) goto fail;
	if (h5.tset_size(atype, strlen(units)) < 0) goto fail;
	if ((attr = h5.acreate2(dset, "Units", atype, aspace, PC_H5P_DEFAULT, PC_H5P_DEFAULT)) < 0) goto fail;
	if (h5.awrite(attr, atype, units) < 0) goto fail;
	ok = true;
fail:
	if (attr >= 0 && h5.aclose(attr) < 0) ok = false;
	if (atype >= 0 && h5.tclose(atype) < 0) ok = false;
	if (aspace >= 0 && h5.sclose(aspace) < 0) ok = false;
	if (dset >= 0 && h5.dclose(dset) < 0) ok = false;
	if (space >= 0 && h5.sclose(space) < 0) ok = false;
	if (!ok)
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_transmission_efficiencies_write_hdf5: could not write dataset %s", name);
	return ok;
}

/* extension, POLYCAP_TALLY_STDERR=1: beside a bins or cells dataset `stem` of `rank` dimensions `dim` its squares (uint64, a trailing
 * dimension 2) and its standard errors (double; pc_hip_tally_stderr with N = n_started); nothing when the result has none */
static bool pc_h5_squares(pc_hid file, int rank, const pc_hsize *dim, const char *stem, const uint64_t *sums, const uint64_t *squares,
	int64_t n_started, polycap_error **error)
{
	if (squares == NULL)
		return true;
	char name[96];
	pc_hsize d[5] = { 1, 1, 1, 1, 2 };
	size_t n = 1;
	for (int k = 0; k < rank; k++) {
		d[k] = dim[k];
		n *= (size_t)dim[k];
	}
	d[rank] = 2;
	double *err = malloc(sizeof(double) * (n ? n : 1));
	if (err == NULL) {
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_transmission_efficiencies_write_hdf5: could not allocate memory -> %s", strerror(errno));
		return false;
	}
	pc_hip_tally_stderr(n, sums, squares, n_started, err);
	snprintf(name, sizeof name, "%s_Squares", stem);
	bool ok = pc_h5_typed(file, rank + 1, d, name, *h5.native_ullong, squares, "2^-64", "lo,hi", error);
	snprintf(name, sizeof name, "%s_StdErr", stem);
	ok = ok && pc_h5_typed(file, rank, d, name, *h5.native_double, err, "weight per started photon", NULL, error);
	free(err);
	return ok;
}

/* planes[k][0..n) stacked into one [nplanes, n] dataset */
static bool pc_h5_planes(pc_hid file, const char *name, int nplanes, double *const *planes, size_t n, const char *units, double *tmp,
	polycap_error **error)
{
	for (int k = 0; k < nplanes; k++)
		memcpy(tmp + (size_t)k * n, planes[k], sizeof(double) * n);
	pc_hsize dim[2] = { (pc_hsize)nplanes, (pc_hsize)n };
	return pc_h5_dataset(file, 2, dim, name, tmp, units, error);
}

static bool pc_h5_scalar(pc_hid file, const char *name, double value, const char *units, polycap_error **error)
{
	pc_hsize one = 1;
	return pc_h5_dataset(file, 1, &one, name, &value, units, error);
}

static bool pc_h5_group(pc_hid file, const char *name, polycap_error **error)
{
	pc_hid g = h5.gcreate2(file, name, PC_H5P_DEFAULT, PC_H5P_DEFAULT, PC_H5P_DEFAULT);
	if (g < 0 || h5.gclose(g) < 0) {
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_transmission_efficiencies_write_hdf5: could not create group %s", name);
		return false;
	}
	return true;
}

/* one scalar attribute of a native type on an open object */
static bool pc_h5_num_attr(pc_hid loc, const char *name, pc_hid type, const void *value)
{
	pc_hid aspace = -1, attr = -1;
	bool ok = false;
	if ((aspace = h5.screate(PC_H5S_SCALAR)) < 0) goto fail;
	if ((attr = h5.acreate2(loc, name, type, aspace, PC_H5P_DEFAULT, PC_H5P_DEFAULT)) < 0) goto fail;
	if (h5.awrite(attr, type, value) < 0) goto fail;
	ok = true;
fail:
	if (attr >= 0 && h5.aclose(attr) < 0) ok = false;
	if (aspace >= 0 && h5.sclose(aspace) < 0) ok = false;
	return ok;
}

/* extension: the group /Draw of POLYCAP_DRAW with the request and the kinds' totals as its attributes */
static bool pc_h5_draw_group(pc_hid file, const struct pc_draw_result *dr, double energy_keV, polycap_error **error)
{
	static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
	const pc_hid g = h5.gcreate2(file, "/Draw", PC_H5P_DEFAULT, PC_H5P_DEFAULT, PC_H5P_DEFAULT);
	const long long n = (long long)dr->n, e = (long long)dr->energy;
	const unsigned long long phase = dr->phase;
	bool ok = g >= 0;
	ok = ok && pc_h5_num_attr(g, "n", *h5.native_llong, &n) && pc_h5_num_attr(g, "energy_index", *h5.native_llong, &e)
	        && pc_h5_num_attr(g, "energy_keV", *h5.native_double, &energy_keV) && pc_h5_num_attr(g, "phase", *h5.native_ullong, &phase);
	for (int k = 0; k < 3 && ok; k++) {
		if (!dr->applied[k])
			continue;
		char name[32];
		const unsigned long long total = dr->total[k];
		const double weight = (double)dr->total[k] / 4294967296.0 / (double)dr->n;
		snprintf(name, sizeof name, "%s_total", names[k]);
		ok = pc_h5_num_attr(g, name, *h5.native_ullong, &total);
		snprintf(name, sizeof name, "%s_weight", names[k]);
		ok = ok && pc_h5_num_attr(g, name, *h5.native_double, &weight);
	}
	if (g >= 0 && h5.gclose(g) < 0)
		ok = false;
	if (!ok)
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_transmission_efficiencies_write_hdf5: could not create group %s", "/Draw");
	return ok;
}

bool polycap_transmission_efficiencies_write_hdf5(polycap_transmission_efficiencies *efficiencies, const char *filename, polycap_error **error)
{
	if (filename == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_transmission_efficiencies_write_hdf5: filename cannot be NULL");
		return false;
	}
	if (efficiencies == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_transmission_efficiencies_write_hdf5: efficiencies cannot be NULL");
		return false;
	}
	const struct _polycap_images *im = efficiencies->images;
	const polycap_source *src = efficiencies->source;
	if (im == NULL || src == NULL || src->description == NULL || src->description->profile == NULL) {
		polycap_set_error_literal(error, POLYCAP_ERROR_INVALID_ARGUMENT, "polycap_transmission_efficiencies_write_hdf5: efficiencies hold no images or source");
		return false;
	}
	if (!pc_h5_load()) {
		polycap_set_error_literal(error, POLYCAP_ERROR_UNSUPPORTED, "polycap_transmission_efficiencies_write_hdf5: no HDF5 (>= 1.10) shared library found; set POLYCAP_HDF5_LIB or use the getters");
		return false;
	}
	const polycap_description *desc = src->description;
	const struct _polycap_profile *prof = desc->profile;
	const size_t n = (size_t)im->i_exit, ne = efficiencies->n_energies;
	const size_t nprof = (size_t)prof->nmax;          /* the reference writes nmax (not nmax+1) profile points (:709-737) */
	size_t tmp_len = 3 * (n ? n : 1);
	if (2 * nprof > tmp_len) tmp_len = 2 * nprof;
	if (2 * (size_t)desc->nelem > tmp_len) tmp_len = 2 * (size_t)desc->nelem;
	double *tmp = malloc(sizeof(double) * tmp_len);
	if (tmp == NULL) {
		polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_transmission_efficiencies_write_hdf5: could not allocate memory -> %s", strerror(errno));
		return false;
	}

	pthread_mutex_lock(&h5_mutex);     /* the writer makes no assumption about a thread-safe HDF5 build */
	bool ok = false;
	pc_hid file = h5.fcreate(filename, PC_H5F_ACC_TRUNC, PC_H5P_DEFAULT, PC_H5P_DEFAULT);
	if (file < 0) {
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_transmission_efficiencies_write_hdf5: unable to create file %s", filename);
		goto done;
	}
	pc_hsize dim[2];
	dim[0] = ne;
	if (!pc_h5_dataset(file, 1, dim, "/Energies", efficiencies->energies, "keV", error)) goto close;
	if (!pc_h5_dataset(file, 1, dim, "/Transmission_Efficiencies", efficiencies->efficiencies, "a.u.", error)) goto close;
	/* extension: the standard errors of a run made with POLYCAP_STDERR=1 */
	if (efficiencies->stderrs != NULL && !pc_h5_dataset(file, 1, dim, "/Transmission_Efficiencies_StdErr", efficiencies->stderrs, "a.u.", error)) goto close;

	if (!pc_h5_group(file, "/PC_Start", error)) goto close;
	if (!pc_h5_planes(file, "/PC_Start/Coordinates", 2, im->pc_start_coords, n, "[cm,cm]", tmp, error)) goto close;
	if (!pc_h5_planes(file, "/PC_Start/Direction", 2, im->pc_start_dir, n, "[cm,cm]", tmp, error)) goto close;
	if (!pc_h5_planes(file, "/PC_Start/Electric_Vector", 2, im->pc_start_elecv, n, "[cm,cm]", tmp, error)) goto close;

	if (!pc_h5_group(file, "/PC_Exit", error)) goto close;
	if (!pc_h5_planes(file, "/PC_Exit/Coordinates", 3, im->pc_exit_coords, n, "[cm,cm,cm]", tmp, error)) goto close;
	for (size_t j = 0; j < n; j++)
		tmp[j] = (double)im->pc_exit_nrefl[j];
	dim[0] = n;
	if (!pc_h5_dataset(file, 1, dim, "/PC_Exit/N_Reflections", tmp, "a.u.", error)) goto close;
	if (!pc_h5_planes(file, "/PC_Exit/Direction", 2, im->pc_exit_dir, n, "[cm,cm]", tmp, error)) goto close;
	if (!pc_h5_planes(file, "/PC_Exit/Electric_Vector", 2, im->pc_exit_elecv, n, "[cm,cm]", tmp, error)) goto close;
	dim[0] = n; dim[1] = ne;
	if (!pc_h5_dataset(file, 2, dim, "/PC_Exit/Weights", im->exit_coord_weights, "[keV,a.u.]", error)) goto close;
	dim[0] = n;
	if (!pc_h5_dataset(file, 1, dim, "/PC_Exit/D_Travel", im->pc_exit_dtravel, "[cm]", error)) goto close;

	if (!pc_h5_planes(file, "/Source_Start_Coordinates", 2, im->src_start_coords, n, "[cm,cm]", tmp, error)) goto close;

	for (int kind = 0; kind < 2; kind++) {
		const size_t nl = (size_t)(kind == 0 ? im->i_extleak : im->i_intleak);
		if (nl == 0)
			continue;
		double *const *coords = kind == 0 ? im->extleak_coords : im->intleak_coords;
		double *const *dirs = kind == 0 ? im->extleak_dir : im->intleak_dir;
		const int64_t *nrefl = kind == 0 ? im->extleak_n_refl : im->intleak_n_refl;
		const double *lw = kind == 0 ? im->extleak_coord_weights : im->intleak_coord_weights;
		const char *g = kind == 0 ? "/ExternalLeaks" : "/InternalLeaks";
		char name[64];
		size_t need = 3*nl > ne ? 3*nl : ne;
		double *ltmp = malloc(sizeof(double) * need);
		if (ltmp == NULL) {
			polycap_set_error(error, POLYCAP_ERROR_MEMORY, "polycap_transmission_efficiencies_write_hdf5: could not allocate memory -> %s", strerror(errno));
			goto close;
		}
		bool lok = pc_h5_group(file, g, error);
		snprintf(name, sizeof name, "%s/Coordinates", g);
		lok = lok && pc_h5_planes(file, name, 3, coords, nl, "[cm,cm,cm]", ltmp, error);
		snprintf(name, sizeof name, "%s/Direction", g);
		lok = lok && pc_h5_planes(file, name, 2, dirs, nl, "[cm,cm]", ltmp, error);
		if (kind == 1)
			lok = lok && pc_h5_planes(file, "/InternalLeaks/Electric_Vector", 2, im->intleak_elecv, nl, "[cm,cm]", ltmp, error);
		dim[0] = nl; dim[1] = ne;
		snprintf(name, sizeof name, "%s/Weights", g);
		lok = lok && pc_h5_dataset(file, 2, dim, name, lw, "[keV,a.u.]", error);
		for (size_t j = 0; j < ne; j++) {
			ltmp[j] = 0.0;
			for (size_t k = 0; k < nl; k++)
				ltmp[j] += lw[k*ne + j];
			ltmp[j] = ltmp[j] / (double)im->i_start;
		}
		dim[0] = ne;
		snprintf(name, sizeof name, "%s/Weight_Total", g);
		lok = lok && pc_h5_dataset(file, 1, dim, name, ltmp, "a.u.", error);
		for (size_t j = 0; j < nl; j++)
			ltmp[j] = (double)nrefl[j];
		dim[0] = nl;
		snprintf(name, sizeof name, "%s/N_Reflections", g);
		lok = lok && pc_h5_dataset(file, 1, dim, name, ltmp, "a.u.", error);
		free(ltmp);
		if (!lok) goto close;
	}

	if (efficiencies->spot != NULL) {
		/* extension: the spot maps of POLYCAP_SPOT, in efficiency units; [plane][energy][iy][ix] */
		const struct pc_spot_result *sp = efficiencies->spot;
		static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
		bool sok = pc_h5_group(file, "/Spot", error);
		double *sel_e = malloc(sizeof(double) * (size_t)sp->n_sel);
		sok = sok && sel_e != NULL;
		for (int32_t k = 0; sok && k < sp->n_sel; k++)
			sel_e[k] = efficiencies->energies[sp->sel[k]];
		pc_hsize sd[4];
		sd[0] = (pc_hsize)sp->n_planes;
		sok = sok && pc_h5_dataset(file, 1, sd, "/Spot/Distances", sp->distances, "cm", error);
		sd[0] = 4;
		sok = sok && pc_h5_dataset(file, 1, sd, "/Spot/Window", sp->window, "cm", error);
		sd[0] = (pc_hsize)sp->n_sel;
		sok = sok && pc_h5_dataset(file, 1, sd, "/Spot/Energies", sel_e, "keV", error);
		for (int k = 0; k < 3 && sok; k++) {
			if (sp->maps[k] == NULL)
				continue;
			char name[64];
			sd[0] = (pc_hsize)sp->n_planes; sd[1] = (pc_hsize)sp->n_sel; sd[2] = (pc_hsize)sp->ny; sd[3] = (pc_hsize)sp->nx;
			snprintf(name, sizeof name, "/Spot/%s", names[k]);
			sok = sok && pc_h5_dataset(file, 4, sd, name, sp->maps[k], "a.u.", error);
			snprintf(name, sizeof name, "/Spot/%s_Outside", names[k]);
			sok = sok && pc_h5_dataset(file, 2, sd, name, sp->outside[k], "a.u.", error);
			snprintf(name, sizeof name, "/Spot/%s", names[k]);
			sok = sok && pc_h5_squares(file, 4, sd, name, sp->sq[k].sums, sp->sq[k].squares, efficiencies->tally_n_started, error);
			snprintf(name, sizeof name, "/Spot/%s_Outside", names[k]);
			sok = sok && pc_h5_squares(file, 2, sd, name, sp->sq[k].outside, sp->sq[k].outside_squares, efficiencies->tally_n_started, error);
		}
		free(sel_e);
		if (!sok) goto close;
	}

	if (efficiencies->beam != NULL) {
		/* extension: the exact exit-beam sums of POLYCAP_BEAM=1 and their derived rows (include/polycap-hip.h) */
		const struct pc_beam_result *br = efficiencies->beam;
		static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
		bool bok = pc_h5_group(file, "/Beam", error);
		double *rows = malloc(sizeof(double) * PC_HIP_BEAM_NCOLS * (ne ? ne : 1));
		bok = bok && rows != NULL;
		for (int k = 0; k < 3 && bok; k++) {
			if (br->sums[k] == NULL)
				continue;
			char name[64];
			pc_hsize bd[3] = { (pc_hsize)ne, PC_HIP_BEAM_NSUMS, 2 };
			const uint64_t n_entries = (uint64_t)br->n_entries[k];
			snprintf(name, sizeof name, "/Beam/%s_Sums", names[k]);
			bok = bok && pc_h5_typed(file, 3, bd, name, *h5.native_ullong, br->sums[k], "2^-32 x (1, 2^-24 cm|rad, 2^-48 cm^2|cm rad|rad^2)",
			                         "W,WX,WY,WU,WV,WXX,WXY,WXU,WXV,WYY,WYU,WYV,WUU,WUV,WVV", error);
			snprintf(name, sizeof name, "/Beam/%s_Outside", names[k]);
			bok = bok && pc_h5_typed(file, 1, bd, name, *h5.native_ullong, br->outside[k], "2^-32", NULL, error);
			snprintf(name, sizeof name, "/Beam/%s_Entries", names[k]);
			pc_hsize one = 1;
			bok = bok && pc_h5_typed(file, 1, &one, name, *h5.native_ullong, &n_entries, "a.u.", NULL, error);
			pc_hip_beam_params(ne, br->sums[k], rows);
			pc_hsize pd[2] = { (pc_hsize)ne, PC_HIP_BEAM_NCOLS };
			snprintf(name, sizeof name, "/Beam/%s", names[k]);
			bok = bok && pc_h5_typed(file, 2, pd, name, *h5.native_double, rows, "a.u., cm, rad", pc_hip_beam_columns(), error);
		}
		free(rows);
		if (!bok) goto close;
	}

	if (efficiencies->hist != NULL) {
		/* extension: the exact histograms of POLYCAP_HIST (include/polycap-hip.h) and the same in efficiency units */
		const struct pc_hist_result *hr = efficiencies->hist;
		static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
		const size_t na = (size_t)hr->n_axes, ns = (size_t)hr->n_sel, tb = (size_t)hr->total_bins;
		bool hok = pc_h5_group(file, "/Hist", error);
		double *table = malloc(sizeof(double) * 8 * na), *sel_e = malloc(sizeof(double) * (ns ? ns : 1));
		double *in = malloc(sizeof(double) * ns * tb), *out = malloc(sizeof(double) * na * ns);      /* all three are >= 1 */
		hok = hok && table != NULL && sel_e != NULL && in != NULL && out != NULL;
		for (size_t a = 0; hok && a < na; a++) {
			const pc_hip_hist_axis *x = &hr->axes[a];
			const double row[8] = { (double)x->quantity, x->d, x->cx, x->cy, x->lo, x->hi, (double)x->n_bins, (double)hr->offsets[a] };
			memcpy(table + 8*a, row, sizeof row);
		}
		for (size_t k = 0; hok && k < ns; k++)
			sel_e[k] = efficiencies->energies[hr->sel[k]];
		for (int k = 0; k < 3 && hok; k++) {
			if (hr->bins[k] == NULL)
				continue;
			char g[32], name[64];
			snprintf(g, sizeof g, "/Hist/%s", names[k]);
			hok = hok && pc_h5_group(file, g, error);
			pc_hsize hd[2] = { (pc_hsize)na, 8 };
			snprintf(name, sizeof name, "%s/Axes", g);
			hok = hok && pc_h5_typed(file, 2, hd, name, *h5.native_double, table, "a.u., cm", "quantity,d,cx,cy,lo,hi,n_bins,offset", error);
			hd[0] = (pc_hsize)ns;
			snprintf(name, sizeof name, "%s/Energies", g);
			hok = hok && pc_h5_dataset(file, 1, hd, name, sel_e, "keV", error);
			hd[0] = (pc_hsize)ns; hd[1] = (pc_hsize)tb;
			snprintf(name, sizeof name, "%s/Bins", g);
			hok = hok && pc_h5_typed(file, 2, hd, name, *h5.native_ullong, hr->bins[k], "2^-32", NULL, error);
			hok = hok && pc_h5_squares(file, 2, hd, name, hr->bins[k], hr->sq[k].squares, efficiencies->tally_n_started, error);
			hd[0] = (pc_hsize)na; hd[1] = (pc_hsize)ns;
			snprintf(name, sizeof name, "%s/Outside", g);
			hok = hok && pc_h5_typed(file, 2, hd, name, *h5.native_ullong, hr->outside[k], "2^-32", NULL, error);
			hok = hok && pc_h5_squares(file, 2, hd, name, hr->outside[k], hr->sq[k].outside_squares, efficiencies->tally_n_started, error);
			const uint64_t n_entries = (uint64_t)hr->n_entries[k];
			pc_hsize one = 1;
			snprintf(name, sizeof name, "%s/Entries", g);
			hok = hok && pc_h5_typed(file, 1, &one, name, *h5.native_ullong, &n_entries, "a.u.", NULL, error);
			/* efficiency[e] * S_bin / (S_inside + S_outside), the spot maps' normalisation: per axis and energy the bins and the
			 * outside part sum to the efficiency */
			for (size_t a = 0; hok && a < na; a++)
				for (size_t s = 0; s < ns; s++) {
					const uint64_t *b = hr->bins[k] + s*tb + (size_t)hr->offsets[a];
					const size_t nb = (size_t)(hr->offsets[a + 1] - hr->offsets[a]);
					uint64_t total = hr->outside[k][a*ns + s];
					for (size_t j = 0; j < nb; j++)
						total += b[j];
					const double eff_e = efficiencies->efficiencies[hr->sel[s]], tot = (double)total;
					for (size_t j = 0; j < nb; j++)
						in[s*tb + (size_t)hr->offsets[a] + j] = total ? eff_e * (double)b[j] / tot : 0.;
					out[a*ns + s] = total ? eff_e * (double)hr->outside[k][a*ns + s] / tot : 0.;
				}
			hd[0] = (pc_hsize)ns; hd[1] = (pc_hsize)tb;
			snprintf(name, sizeof name, "%s/Efficiency", g);
			hok = hok && pc_h5_dataset(file, 2, hd, name, in, "a.u.", error);
			hd[0] = (pc_hsize)na; hd[1] = (pc_hsize)ns;
			snprintf(name, sizeof name, "%s/Efficiency_Outside", g);
			hok = hok && pc_h5_dataset(file, 2, hd, name, out, "a.u.", error);
		}
		free(table); free(sel_e); free(in); free(out);
		if (!hok) goto close;
	}

	if (efficiencies->joint != NULL) {
		/* extension: the exact joint histograms of POLYCAP_JOINT (include/polycap-hip.h) and the same in efficiency units */
		const struct pc_joint_result *jr = efficiencies->joint;
		static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
		const size_t np = (size_t)jr->n_pairs, ns = (size_t)jr->n_sel, tc = (size_t)jr->total_cells;
		bool jok = pc_h5_group(file, "/Joint", error);
		double *table = malloc(sizeof(double) * 15 * np), *sel_e = malloc(sizeof(double) * (ns ? ns : 1));
		double *in = malloc(sizeof(double) * ns * tc), *out = malloc(sizeof(double) * np * ns);      /* all three are >= 1 */
		jok = jok && table != NULL && sel_e != NULL && in != NULL && out != NULL;
		for (size_t p = 0; jok && p < np; p++) {
			const pc_hip_hist_axis *u = &jr->pairs[p].u, *v = &jr->pairs[p].v;
			const double row[15] = { (double)u->quantity, u->d, u->cx, u->cy, u->lo, u->hi, (double)u->n_bins,
			                         (double)v->quantity, v->d, v->cx, v->cy, v->lo, v->hi, (double)v->n_bins, (double)jr->offsets[p] };
			memcpy(table + 15*p, row, sizeof row);
		}
		for (size_t k = 0; jok && k < ns; k++)
			sel_e[k] = efficiencies->energies[jr->sel[k]];
		for (int k = 0; k < 3 && jok; k++) {
			if (jr->cells[k] == NULL)
				continue;
			char g[32], name[64];
			snprintf(g, sizeof g, "/Joint/%s", names[k]);
			jok = jok && pc_h5_group(file, g, error);
			pc_hsize jd[2] = { (pc_hsize)np, 15 };
			snprintf(name, sizeof name, "%s/Pairs", g);
			jok = jok && pc_h5_typed(file, 2, jd, name, *h5.native_double, table, "a.u., cm",
			                         "u_quantity,u_d,u_cx,u_cy,u_lo,u_hi,u_n_bins,v_quantity,v_d,v_cx,v_cy,v_lo,v_hi,v_n_bins,offset", error);
			jd[0] = (pc_hsize)ns;
			snprintf(name, sizeof name, "%s/Energies", g);
			jok = jok && pc_h5_dataset(file, 1, jd, name, sel_e, "keV", error);
			jd[0] = (pc_hsize)ns; jd[1] = (pc_hsize)tc;
			snprintf(name, sizeof name, "%s/Cells", g);
			jok = jok && pc_h5_typed(file, 2, jd, name, *h5.native_ullong, jr->cells[k], "2^-32", NULL, error);
			jok = jok && pc_h5_squares(file, 2, jd, name, jr->cells[k], jr->sq[k].squares, efficiencies->tally_n_started, error);
			jd[0] = (pc_hsize)np; jd[1] = (pc_hsize)ns;
			snprintf(name, sizeof name, "%s/Outside", g);
			jok = jok && pc_h5_typed(file, 2, jd, name, *h5.native_ullong, jr->outside[k], "2^-32", NULL, error);
			jok = jok && pc_h5_squares(file, 2, jd, name, jr->outside[k], jr->sq[k].outside_squares, efficiencies->tally_n_started, error);
			const uint64_t n_entries = (uint64_t)jr->n_entries[k];
			pc_hsize one = 1;
			snprintf(name, sizeof name, "%s/Entries", g);
			jok = jok && pc_h5_typed(file, 1, &one, name, *h5.native_ullong, &n_entries, "a.u.", NULL, error);
			/* efficiency[e] * S_cell / (S_inside + S_outside), the spot maps' normalisation: per pair and energy the cells and the
			 * outside part sum to the efficiency */
			for (size_t p = 0; jok && p < np; p++)
				for (size_t s = 0; s < ns; s++) {
					const uint64_t *b = jr->cells[k] + s*tc + (size_t)jr->offsets[p];
					const size_t nb = (size_t)(jr->offsets[p + 1] - jr->offsets[p]);
					uint64_t total = jr->outside[k][p*ns + s];
					for (size_t j = 0; j < nb; j++)
						total += b[j];
					const double eff_e = efficiencies->efficiencies[jr->sel[s]], tot = (double)total;
					for (size_t j = 0; j < nb; j++)
						in[s*tc + (size_t)jr->offsets[p] + j] = total ? eff_e * (double)b[j] / tot : 0.;
					out[p*ns + s] = total ? eff_e * (double)jr->outside[k][p*ns + s] / tot : 0.;
				}
			jd[0] = (pc_hsize)ns; jd[1] = (pc_hsize)tc;
			snprintf(name, sizeof name, "%s/Efficiency", g);
			jok = jok && pc_h5_dataset(file, 2, jd, name, in, "a.u.", error);
			jd[0] = (pc_hsize)np; jd[1] = (pc_hsize)ns;
			snprintf(name, sizeof name, "%s/Efficiency_Outside", g);
			jok = jok && pc_h5_dataset(file, 2, jd, name, out, "a.u.", error);
		}
		free(table); free(sel_e); free(in); free(out);
		if (!jok) goto close;
	}

	if (efficiencies->select != NULL) {
		/* extension: the cuts of POLYCAP_SELECT and the exact totals of what passed them (include/polycap-hip.h); rows of Passed,
		 * Rejected and Entries: exit photons, extleak, intleak */
		const struct pc_select_result *sr = efficiencies->select;
		const size_t nc = (size_t)sr->n_cuts, ne = efficiencies->n_energies;
		bool sok = pc_h5_group(file, "/Select", error);
		double *table = malloc(sizeof(double) * 7 * nc);
		sok = sok && table != NULL;
		for (size_t k = 0; sok && k < nc; k++) {
			const pc_hip_hist_axis *x = &sr->cuts[k].axis;
			const double row[7] = { (double)x->quantity, x->d, x->cx, x->cy, x->lo, x->hi, (double)sr->cuts[k].negate };
			memcpy(table + 7*k, row, sizeof row);
		}
		pc_hsize sd[2] = { (pc_hsize)nc, 7 };
		sok = sok && pc_h5_typed(file, 2, sd, "/Select/Cuts", *h5.native_double, table, "a.u., cm", "quantity,d,cx,cy,lo,hi,negate", error);
		sd[0] = 3; sd[1] = (pc_hsize)ne;
		sok = sok && pc_h5_typed(file, 2, sd, "/Select/Passed", *h5.native_ullong, sr->passed_w, "2^-32", NULL, error);
		sok = sok && pc_h5_typed(file, 2, sd, "/Select/Rejected", *h5.native_ullong, sr->rejected_w, "2^-32", NULL, error);
		if (sr->passed_w2 != NULL) {      /* POLYCAP_TALLY_STDERR=1 */
			pc_hsize qd[3] = { 3, (pc_hsize)ne, 2 };
			double *t = malloc(sizeof(double) * 6 * (ne ? ne : 1));
			sok = sok && t != NULL;
			for (size_t k = 0; sok && k < 3; k++)
				pc_hip_select_transmission(ne, sr->passed_w + k*ne, sr->rejected_w + k*ne, sr->passed_w2 + 2*k*ne, sr->rejected_w2 + 2*k*ne,
				                           t + k*ne, t + (3 + k)*ne);
			sok = sok && pc_h5_typed(file, 3, qd, "/Select/Passed_Squares", *h5.native_ullong, sr->passed_w2, "2^-64", "lo,hi", error);
			sok = sok && pc_h5_typed(file, 3, qd, "/Select/Rejected_Squares", *h5.native_ullong, sr->rejected_w2, "2^-64", "lo,hi", error);
			sok = sok && pc_h5_typed(file, 2, qd, "/Select/Transmission", *h5.native_double, t, "a.u.", NULL, error);
			sok = sok && pc_h5_typed(file, 2, qd, "/Select/Transmission_StdErr", *h5.native_double, t + 3*ne, "a.u.", NULL, error);
			free(t);
		}
		uint64_t entries[6];
		for (int k = 0; k < 3; k++) {
			entries[2*k] = (uint64_t)sr->n_pass[k];
			entries[2*k + 1] = (uint64_t)sr->n_seen[k];
		}
		sd[0] = 3; sd[1] = 2;
		sok = sok && pc_h5_typed(file, 2, sd, "/Select/Entries", *h5.native_ullong, entries, "a.u.", "n_pass,n_seen", error);
		if (sr->rec_limit > 0) {      /* POLYCAP_SELECT_RECORDS: the first rows of what passed, per kind that has some */
			static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
			const uint64_t limit = (uint64_t)sr->rec_limit;
			pc_hsize one = 1;
			sok = sok && pc_h5_typed(file, 1, &one, "/Select/Records_Limit", *h5.native_ullong, &limit, "a.u.", NULL, error);
			for (int k = 0; k < 3 && sok; k++) {
				if (!sr->rec_applied[k] || sr->rec_n[k] == 0)
					continue;
				char name[64];
				pc_hsize rd[2] = { (pc_hsize)sr->rec_n[k], (pc_hsize)sr->rec_row[k] };
				snprintf(name, sizeof name, "/Select/%s_Records", names[k]);
				sok = sok && pc_h5_typed(file, 2, rd, name, *h5.native_double, sr->rec[k], "[cm,a.u.]",
				                         k == 0 ? "the planes of an exit photon in their order (n_refl as int64 bits), then the weights"
				                                : "slot,attempt,x,y,z,dir x y z,elecv x y z,n_refl, then the weights", error);
				snprintf(name, sizeof name, "/Select/%s_Positions", names[k]);
				sok = sok && pc_h5_typed(file, 1, rd, name, *h5.native_llong, sr->rec_pos[k], "a.u.", NULL, error);
			}
		}
		free(table);
		if (!sok) goto close;
	}

	if (efficiencies->draw != NULL) {
		/* extension: the unweighted sample of POLYCAP_DRAW (include/polycap-hip.h): the rows of every kind that has some */
		const struct pc_draw_result *dr = efficiencies->draw;
		static const char *const names[3] = { "Exit", "ExtLeak", "IntLeak" };
		bool dok = pc_h5_draw_group(file, dr, efficiencies->energies[dr->energy], error);
		for (int k = 0; k < 3 && dok; k++) {
			if (!dr->applied[k] || dr->rows[k] == 0)
				continue;
			char name[64];
			pc_hsize rd[2] = { (pc_hsize)dr->rows[k], (pc_hsize)dr->row[k] };
			snprintf(name, sizeof name, "/Draw/%s_Records", names[k]);
			dok = dok && pc_h5_typed(file, 2, rd, name, *h5.native_double, dr->rec[k], "[cm,a.u.]",
			                         k == 0 ? "the planes of an exit photon in their order (n_refl as int64 bits), then the weights"
			                                : "slot,attempt,x,y,z,dir x y z,elecv x y z,n_refl, then the weights", error);
			snprintf(name, sizeof name, "/Draw/%s_Positions", names[k]);
			dok = dok && pc_h5_typed(file, 1, rd, name, *h5.native_llong, dr->pos[k], "a.u.", NULL, error);
		}
		if (!dok) goto close;
	}

	if (!pc_h5_group(file, "/Input", error)) goto close;
	{
		double *const shape_ext[2] = { prof->z, prof->ext }, *const shape_cap[2] = { prof->z, prof->cap };
		if (!pc_h5_planes(file, "/Input/PC_Shape", 2, shape_ext, nprof, "[cm,cm]", tmp, error)) goto close;
		if (!pc_h5_planes(file, "/Input/Cap_Shape", 2, shape_cap, nprof, "[cm,cm]", tmp, error)) goto close;
	}
	if (!pc_h5_scalar(file, "/Input/N_Capillaries", (double)desc->n_cap, "a.u.", error)) goto close;
	if (!pc_h5_scalar(file, "/Input/Surface_Roughness", desc->sig_rough, "Angstrom", error)) goto close;
	if (!pc_h5_scalar(file, "/Input/Open_Area", desc->open_area, "a.u.", error)) goto close;
	for (unsigned int j = 0; j < desc->nelem; j++) {
		tmp[j] = (double)desc->iz[j];
		tmp[j + desc->nelem] = desc->wi[j];
	}
	dim[0] = 2; dim[1] = desc->nelem;
	if (!pc_h5_dataset(file, 2, dim, "/Input/PC_Composition", tmp, "[Z,w%]", error)) goto close;
	if (!pc_h5_scalar(file, "/Input/PC_Density", desc->density, "g/cm3", error)) goto close;
	if (!pc_h5_scalar(file, "/Input/Src_PC_Dist", src->d_source, "cm", error)) goto close;
	ok = true;
close:
	if (h5.fclose(file) < 0 && ok) {
		polycap_set_error(error, POLYCAP_ERROR_IO, "polycap_transmission_efficiencies_write_hdf5: could not close file %s", filename);
		ok = false;
	}
done:
	pthread_mutex_unlock(&h5_mutex);
	free(tmp);
	return ok;
}

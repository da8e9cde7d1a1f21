/*
 * pc_tally.h -- what spot maps (pc_spot.h), exit-beam moments (pc_beam.h) and histograms (pc_hist.h) share.  Each of them is a
 * tally: a post-pass over the entries the last run left on the device (exit photons as image records or planes, the ordered leak
 * event lists), accumulated exactly into uint64 cells, per kind, per member of a device group.  Here is the one copy of the
 * energy selection, the grid sizing, the 128-bit carry add, the entry source and its loader, the lane mapping of the
 * energies-across-lanes kernels, and the object's lifetime, add, read-back sum and reset.  A tally's own header keeps its per-entry
 * arithmetic, kernels, cell layout and host formulas.  Here too is what the standard errors of the tallies need (include/polycap-hip.h):
 * the square of an entry's quantised weight as a (lo, hi) pair, its adds in LDS and in global memory, the split of the cells into LDS
 * tiles with and without the pairs, the second buffer of a member and the two host estimators.
 *
 * The first part (plain functions, no HIP types) compiles for the host as well: -DPC_TALLY_HOST_ONLY stops the header after it.
 */
#ifndef PC_TALLY_H
#define PC_TALLY_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "pc_exact.h"

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

/* The energy selection of a spec: n_sel indices into the problem's n_energies, each once; n_sel = 0 selects all.  false and the
 * reason in *why (it starts with the spec's field at fault) when it is refused. */
static inline bool pc_sel_check(int n_sel, const int *sel, size_t n_energies, std::string *why)
{
	if (n_sel < 0 || (size_t)n_sel > n_energies || (n_sel > 0 && !sel)) {
		*why = "n_energies: between 1 and the problem's energy count of indices (0 = all energies)";
		return false;
	}
	std::vector<char> seen(n_energies, 0);
	for (int k = 0; k < n_sel; k++) {
		const int e = sel[k];
		if (e < 0 || (size_t)e >= n_energies) {
			*why = "energies: index " + std::to_string(e) + " out of range (" + std::to_string(n_energies) + " energies)";
			return false;
		}
		if (seen[e]) {
			*why = "energies: index " + std::to_string(e) + " given twice";
			return false;
		}
		seen[e] = 1;
	}
	return true;
}

/* the indices a checked selection stands for */
static inline std::vector<int> pc_sel_fill(int n_sel, const int *sel, size_t n_energies)
{
	std::vector<int> out;
	if (n_sel == 0)
		for (size_t e = 0; e < n_energies; e++) out.push_back((int)e);
	else
		out.assign(sel, sel + n_sel);
	return out;
}

/* lanes that share one entry when n energies go across the lanes of a wave: the next power of two, 64 at the most */
static inline __host__ __device__ int pc_tally_gw(int n)
{
	int gw = 1;
	while (gw < n && gw < 64) gw <<= 1;
	return gw;
}

/* gridDim.x of an add, and gw where the energies go across the lanes (0 otherwise) */
struct pc_tally_grid {
	long long bx;
	int gw;
};

/* no more workgroups than the entries fill, and one at least */
static inline long long pc_tally_grid_cap(long long bx, long long work, int block)
{
	const long long need = (work + block - 1)/block;
	if (bx > need) bx = need;
	return (bx < 1) ? 1 : bx;
}

/* LDS-tile kernels, one lane per entry and gridDim.y = tiles: two workgroups per CU in all (LDS: 64 KiB each) */
static inline pc_tally_grid pc_tally_grid_tiles(long long cus, long long tiles, long long n_entries, int block)
{
	const pc_tally_grid g = { pc_tally_grid_cap((2*cus + tiles - 1)/tiles, n_entries, block), 0 };
	return g;
}

/* Cells of one LDS tile of `tile` uint64, and the tiles that `total` cells take.  A tile holds `tile` weight cells; where the squares
 * are tracked (squares != 0) a cell is three uint64 -- its weight sum and the (lo, hi) pair of its square sum -- and a tile holds
 * tile / 3 cells: [cells] weight sums, then [cells][2] pairs. */
struct pc_tally_tiling {
	long long cells, tiles;
};

static inline constexpr __host__ __device__ long long pc_tally_tile_cells(long long tile, int squares)
{
	return squares ? tile/3 : tile;
}

static inline pc_tally_tiling pc_tally_tile_split(long long total, long long tile, int squares)
{
	const long long cells = pc_tally_tile_cells(tile, squares);
	const pc_tally_tiling t = { cells, (total + cells - 1)/cells };
	return t;
}

/* energies-across-lanes kernels, gw lanes per entry and `groups` workgroups for every gridDim.x: eight workgroups per CU in all */
static inline pc_tally_grid pc_tally_grid_wide(long long cus, long long groups, int n_sel, long long n_entries, int block)
{
	const int gw = pc_tally_gw(n_sel);
	const pc_tally_grid g = { pc_tally_grid_cap((8*cus + groups - 1)/groups, n_entries*gw, block), gw };
	return g;
}

/* (lo, hi) += (add_lo, add_hi) mod 2^128: the device spelling of pc_exact_add */
static inline __host__ __device__ void pc_add128(unsigned long long &lo, unsigned long long &hi, unsigned long long add_lo, unsigned long long add_hi)
{
	const pc_exact_pair s = pc_exact_add(lo, hi, add_lo, add_hi);
	lo = s.lo; hi = s.hi;
}

/* The square of one entry's quantised weight W = pc_spot_q(w) <= 2^32: the integer product W*W <= 2^64 in units of 2^-64, as
 * lo = W*W mod 2^64 and hi = the product's upper half (1 for W = 2^32 only) */
static inline __host__ __device__ void pc_tally_sq(unsigned long long W, unsigned long long &lo, unsigned long long &hi)
{
	lo = W*W;
#ifdef __HIP_DEVICE_COMPILE__
	hi = __umul64hi(W, W);
#else
	hi = (unsigned long long)(((unsigned __int128)W*W) >> 64);
#endif
}

/* pc_hip_tally_stderr: the formula of include/polycap-hip.h in its order */
static inline void pc_tally_stderr(size_t n_cells, const uint64_t *sums, const uint64_t *squares, int64_t n_started, double *out)
{
	const long double n = (long double)n_started;
	for (size_t k = 0; k < n_cells; k++) {
		if (!(n >= 2.0L)) { out[k] = NAN; continue; }
		const long double a = (long double)sums[k], b = pc_exact_value(squares[2*k], squares[2*k + 1]);
		out[k] = pc_exact_stderr(a / (n * PC_EXACT_2P32), b / (n * PC_EXACT_2P64), n);
	}
}

/* pc_hip_select_transmission: the formula of include/polycap-hip.h in its order */
static inline void pc_tally_transmission(size_t n_energies, const uint64_t *passed_w, const uint64_t *rejected_w, const uint64_t *passed_w2,
	const uint64_t *rejected_w2, double *T, double *T_err)
{
	for (size_t e = 0; e < n_energies; e++) {
		const long double P = (long double)passed_w[e] / PC_EXACT_2P32, R = (long double)rejected_w[e] / PC_EXACT_2P32;
		const long double P2 = pc_exact_value(passed_w2[2*e], passed_w2[2*e + 1]) / PC_EXACT_2P64;
		const long double R2 = pc_exact_value(rejected_w2[2*e], rejected_w2[2*e + 1]) / PC_EXACT_2P64;
		const long double tot = P + R;
		if (!(tot > 0.0L)) {
			if (T) T[e] = NAN;
			if (T_err) T_err[e] = NAN;
			continue;
		}
		if (T) T[e] = (double)(P / tot);
		if (T_err) T_err[e] = (double)(sqrtl(R*R*P2 + P*P*R2) / (tot*tot));
	}
}

#ifndef PC_TALLY_HOST_ONLY

/* W*W of one entry added to a (lo, hi) pair in LDS: ds_add_u64 on lo, the carry from the old value it returns, and with it the
 * product's own upper half on hi.  Adds commute, so the pair is exact in whatever order the lanes arrive. */
static __device__ __forceinline__ void pc_tally_lds_add_sq(unsigned long long *lohi, unsigned long long W)
{
	unsigned long long lo, hi;
	pc_tally_sq(W, lo, hi);
	const unsigned long long old = atomicAdd(&lohi[0], lo);
	hi += (old + lo < old) ? 1ull : 0ull;
	if (hi) atomicAdd(&lohi[1], hi);
}

/* the same on a pair of global cells: two 8-byte atomics at the most */
static __device__ __forceinline__ void pc_tally_add_sq(unsigned long long *lohi, unsigned long long W)
{
	unsigned long long lo, hi;
	pc_tally_sq(W, lo, hi);
	pc_atomic_add128(lohi, lo, hi);
}

/* Where the entries are: field f of entry i at p[i*ss + f*fs], weight e at w[i*ws + e] */
struct pc_spot_src {
	const double *p;
	long long ss, fs, n;
	int f_x, f_dx;          /* x, y, z at f_x .. f_x + 2; dx, dy (, dz when has_dz) from f_dx on */
	int has_dz;
	const double *w;
	long long ws;
	const unsigned char *mask;      /* a selection's byte per entry (pc_select.h): an entry with 0 does not exist for the tally; NULL: all do */
};

struct pc_entry { double x, y, z, dx, dy, dz; };

static inline __host__ __device__ double pc_spot_exit_dz(double dx, double dy);      /* pc_spot.h, in the part its host tests compile */

/* position and direction of entry i */
static __device__ __forceinline__ pc_entry pc_entry_load(const pc_spot_src &s, long long i)
{
	const double *p = s.p + i*s.ss;
	pc_entry e;
	e.x = p[(long long)s.f_x*s.fs]; e.y = p[(long long)(s.f_x + 1)*s.fs]; e.z = p[(long long)(s.f_x + 2)*s.fs];
	e.dx = p[(long long)s.f_dx*s.fs]; e.dy = p[(long long)(s.f_dx + 1)*s.fs];
	e.dz = s.has_dz ? p[(long long)(s.f_dx + 2)*s.fs] : pc_spot_exit_dz(e.dx, e.dy);
	return e;
}

/* Energies across lanes: the lanes of a wave take the n (<= 64 at a time) energies of one entry, 64 / gw entries per wave.  Lane
 * `lane` holds energy sub, sub + gw, ... of the entries first, first + stride, ... */
struct pc_tally_lanes {
	int gw, lane, sub;
	long long first, stride;
};

static __device__ __forceinline__ pc_tally_lanes pc_tally_lane_map(int n)
{
	pc_tally_lanes l;
	l.gw = pc_tally_gw(n);
	l.lane = threadIdx.x & 63;
	l.sub = l.lane & (l.gw - 1);
	const int per_wave = 64 / l.gw;
	const long long wave = ((long long)blockIdx.x*blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x*blockDim.x) >> 6;
	l.first = wave*per_wave + l.lane / l.gw;
	l.stride = n_waves*per_wave;
	return l;
}

/* the entries of `kind` that the last run of c left on its device; `who` is the call that asks */
static int pc_spot_source(pc_hip_ctx *c, int kind, pc_spot_src &s, const char *who)
{
	const long long ne = c->host.pm.n_energies;
	memset(&s, 0, sizeof(s));
	if (kind == 0) {
		if (!c->img.valid)
			return pc_fail(PC_HIP_ERR_INVALID, std::string(who) + ": the last run kept no exit photons (run it with keep_images)");
		if (c->leak.pending) {       /* a leak run may be repeated with a larger record buffer when it is waited for */
			int st = pc_hip_transmission_wait(c, nullptr);
			if (st) return st;
		}
		const pc_image_view v = c->img.device_view();
		s.n = v.n; s.f_x = PC_F_EXITX; s.f_dx = PC_F_EDIRX; s.has_dz = 0;
		s.p = v.p; s.ss = v.l.ss; s.fs = v.l.fs;
		s.w = v.w; s.ws = v.l.ws;
		return PC_HIP_OK;
	}
	if (!c->leak.events_of_run)
		return pc_fail(PC_HIP_ERR_INVALID, std::string(who) + ": leak events need a leak_calc source run (pc_hip_transmission_run_leak) as the last run");
	int st = pc_hip_transmission_wait(c, nullptr);      /* the events are ordered into their lists when the run is waited for */
	if (st) return st;
	const long long stride = PC_HIP_LEAK_HDR + ne;
	const pc_leak_list l = c->leak.list(kind - 1, (size_t)ne);   /* a tally's kinds 1, 2 are the lists 0 (extleak), 1 (intleak) */
	s.n = l.n;
	s.p = l.dev;
	s.ss = stride; s.fs = 1; s.f_x = 2; s.f_dx = 5; s.has_dz = 1;
	s.w = s.p + PC_HIP_LEAK_HDR; s.ws = stride;
	return PC_HIP_OK;
}

/* ---- the object: one set of cells per member of the group (one member without a group) */
struct pc_tally_member {
	pc_hip_ctx *ctx = nullptr;
	pc_dev_buf<unsigned long long> d_cells;
	pc_dev_buf<unsigned long long> d_sq;           /* [elems][2]: the cells' square sums as (lo, hi) pairs, where the tally tracks them */
	pc_dev_buf<int> d_sel;          /* the selected energies' indices, where the tally selects */
	pc_dev_buf<double> d_zp;        /* plane positions, where it has planes */
};

struct pc_tally {
	std::vector<pc_tally_member> m;
	pc_hip_group *group = nullptr;
	long long n_entries[3] = {0, 0, 0};       /* added so far, per kind */
	size_t elems = 0;                         /* cells of a member */
	int shared = 0;                           /* the kinds add to the same cells: the entry cap holds for them together */
	int squares = 0;                          /* every add fills d_sq beside d_cells (pc_tally_track_squares) */
	~pc_tally();
};

/* what was enqueued on a member's stream is over before its buffers go */
static void pc_tally_destroy(pc_tally &t)
{
	for (pc_tally_member &m : t.m) {
		if (!m.ctx) continue;
		(void)hipSetDevice(m.ctx->device);
		if (m.ctx->stream) (void)hipStreamSynchronize(m.ctx->stream);
		m = pc_tally_member();
	}
	t.m.clear();
}

inline pc_tally::~pc_tally() { pc_tally_destroy(*this); }

static int pc_tally_hip(hipError_t e, const char *who)
{
	if (e == hipSuccess) return PC_HIP_OK;
	(void)hipGetLastError();
	return pc_fail(e == hipErrorOutOfMemory ? PC_HIP_ERR_MEMORY : PC_HIP_ERR_RUNTIME, std::string(who) + ": " + hipGetErrorString(e));
}

/* `elems` zeroed cells on every context's device; nothing stays allocated when it fails */
static int pc_tally_make(pc_tally &t, const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, size_t elems, const char *who)
{
	const std::string msg = std::string(who) + ": could not allocate the cells";
	t.group = group;
	t.elems = elems;
	for (pc_hip_ctx *c : ctxs) {
		t.m.emplace_back();
		pc_tally_member &m = t.m.back();
		m.ctx = c;
		int st = pc_tally_hip(hipSetDevice(c->device), who);
		if (!st) st = m.d_cells.grow(elems, msg.c_str());
		if (!st) st = pc_tally_hip(hipMemsetAsync(m.d_cells, 0, elems*sizeof(unsigned long long), c->stream), who);
		if (st) { pc_tally_destroy(t); return st; }
	}
	return PC_HIP_OK;
}

/* Turns the tracking of squares on: zeroed pairs beside the cells of every member.  Only while the tally holds no entries; refused
 * (PC_HIP_ERR_INVALID) otherwise, and nothing stays allocated and nothing is changed when it fails. */
static int pc_tally_track_squares(pc_tally &t, const char *who)
{
	const std::string w(who);
	if (t.n_entries[0] | t.n_entries[1] | t.n_entries[2])
		return pc_fail(PC_HIP_ERR_INVALID, w + ": squares can be tracked only while the object holds no entries (before the first add, or after a reset)");
	if (t.squares) return PC_HIP_OK;
	const std::string msg = w + ": could not allocate the square cells";
	int st = PC_HIP_OK;
	for (pc_tally_member &m : t.m) {
		st = pc_tally_hip(hipSetDevice(m.ctx->device), who);
		if (!st) st = m.d_sq.grow(2*t.elems, msg.c_str());
		if (!st) st = pc_tally_hip(hipMemsetAsync(m.d_sq, 0, 2*t.elems*sizeof(unsigned long long), m.ctx->stream), who);
		if (st) break;
	}
	if (st) {
		for (pc_tally_member &m : t.m) {
			(void)hipSetDevice(m.ctx->device);
			(void)hipStreamSynchronize(m.ctx->stream);
			m.d_sq.reset();
		}
		return st;
	}
	t.squares = 1;
	return PC_HIP_OK;
}

/* the energy selection and the plane positions (either may be empty) to every member; as pc_tally_make when it fails */
static int pc_tally_upload(pc_tally &t, const std::vector<int> &sel, const std::vector<double> &zp, const char *who)
{
	const std::string msg = std::string(who) + ": could not allocate the energy selection and the plane positions";
	for (pc_tally_member &m : t.m) {
		int st = pc_tally_hip(hipSetDevice(m.ctx->device), who);
		if (!st) st = m.d_sel.grow(sel.size(), msg.c_str());
		if (!st) st = m.d_zp.grow(zp.size(), msg.c_str());
		if (!st && !sel.empty()) st = pc_tally_hip(hipMemcpy(m.d_sel, sel.data(), sel.size()*sizeof(int), hipMemcpyHostToDevice), who);
		if (!st && !zp.empty()) st = pc_tally_hip(hipMemcpy(m.d_zp, zp.data(), zp.size()*sizeof(double), hipMemcpyHostToDevice), who);
		if (st) { pc_tally_destroy(t); return st; }
	}
	return PC_HIP_OK;
}

/* Every member's source of the entries of `kind` (zeroed for a member of a group that traced nothing), and their count: nothing is
 * launched unless the whole call can be */
static int pc_tally_sources(const std::vector<pc_hip_ctx *> &ctxs, const pc_hip_group *g, int kind, const char *who, std::vector<pc_spot_src> &src,
	long long *n_total)
{
	const std::string w(who);
	if (kind < 0 || kind > 2) return pc_fail(PC_HIP_ERR_INVALID, w + ": kind must be 0 (exit photons), 1 (extleak) or 2 (intleak)");
	if (g && kind == 0 && !g->keep_images)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the last run kept no exit photons (run it with keep_images)");
	if (g && kind > 0 && !g->leak_run)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": leak events need a leak_calc run of the group as the last run");
	src.resize(ctxs.size());
	long long n = 0;
	for (size_t k = 0; k < ctxs.size(); k++) {
		if (g && g->count[k] == 0) { memset(&src[k], 0, sizeof(src[k])); continue; }
		PC_HIP_CHECK(hipSetDevice(ctxs[k]->device));
		const int st = pc_spot_source(ctxs[k], kind, src[k], who);
		if (st) return st;
		n += src[k].n;
	}
	*n_total = n;
	return PC_HIP_OK;
}

/* A selection as an add sees it (pc_select.h): refuses (PC_HIP_ERR_INVALID, nothing changed) a selection of another owner than the
 * tally's, one not applied for `kind`, and a mask that is not of the entries in src; otherwise src[k].mask = member k's mask, passing[k]
 * = how many of its entries pass. */
struct pc_hip_select;
static int pc_select_gate(pc_hip_select *sel, const std::vector<pc_hip_ctx *> &ctxs, const pc_hip_group *g, int kind, const char *who,
	std::vector<pc_spot_src> &src, std::vector<long long> &passing);

/* Adds the entries of `kind` of the last run, through the selection `sel` if there is one: launch(k, src, kind) enqueues member k's
 * non-empty source on its stream (its device is current) and returns a status. */
template <typename Launch>
static int pc_tally_add(pc_tally &t, int kind, const char *who, Launch launch, pc_hip_select *sel = nullptr)
{
	const std::string w(who);
	std::vector<pc_hip_ctx *> ctxs;
	for (const pc_tally_member &m : t.m) ctxs.push_back(m.ctx);
	std::vector<pc_spot_src> src;
	long long n = 0;
	int st = pc_tally_sources(ctxs, t.group, kind, who, src, &n);
	if (st) return st;
	std::vector<long long> passing;          /* per member, with a selection */
	if (sel) {
		st = pc_select_gate(sel, ctxs, t.group, kind, who, src, passing);
		if (st) return st;
		n = 0;
		for (long long p : passing) n += p;
	}
	const long long held = t.shared ? t.n_entries[0] + t.n_entries[1] + t.n_entries[2] : t.n_entries[kind];
	if (held + n > (long long)0xffffffffll)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the cells of a kind take at most 2^32 - 1 entries (their exact sums could wrap beyond)");
	for (size_t k = 0; k < t.m.size(); k++) {
		if (src[k].n == 0 || (sel && passing[k] == 0)) continue;
		PC_HIP_CHECK(hipSetDevice(t.m[k].ctx->device));
		st = launch(k, src[k], kind);
		if (st) return st;
		PC_HIP_CHECK(hipGetLastError());
	}
	t.n_entries[kind] += n;
	return PC_HIP_OK;
}

/* One buffer of n uint64 of every member, summed on the host.  limbs = 1: uint64 cells; 2: (lo, hi) pairs with carry.  Exact either
 * way: the entry cap keeps every sum in range. */
static int pc_tally_sum_of(pc_tally &t, pc_dev_buf<unsigned long long> pc_tally_member::*buf, size_t n, int limbs, std::vector<unsigned long long> &sum)
{
	std::vector<unsigned long long> part(n);
	sum.assign(n, 0ull);
	for (pc_tally_member &m : t.m) {
		PC_HIP_CHECK(hipSetDevice(m.ctx->device));
		const unsigned long long *d = (m.*buf).p;
		PC_HIP_CHECK(hipMemcpyAsync(part.data(), d, n*sizeof(unsigned long long), hipMemcpyDeviceToHost, m.ctx->stream));
		PC_HIP_CHECK(hipStreamSynchronize(m.ctx->stream));
		if (limbs == 2)
			for (size_t k = 0; k < n; k += 2) pc_add128(sum[k], sum[k + 1], part[k], part[k + 1]);
		else
			for (size_t k = 0; k < n; k++) sum[k] += part[k];
	}
	return PC_HIP_OK;
}

/* the members' cells */
static int pc_tally_sum(pc_tally &t, int limbs, std::vector<unsigned long long> &sum)
{
	return pc_tally_sum_of(t, &pc_tally_member::d_cells, t.elems, limbs, sum);
}

/* the summed square pairs of a tally that tracks them; `who` is the call that asks */
static int pc_tally_sum_squares(pc_tally &t, const char *who, std::vector<unsigned long long> &sum)
{
	if (!t.squares)
		return pc_fail(PC_HIP_ERR_INVALID, std::string(who) + ": the object does not track squares (turn it on with its _track_squares call before the first add)");
	return pc_tally_sum_of(t, &pc_tally_member::d_sq, 2*t.elems, 2, sum);
}

static int pc_tally_reset(pc_tally &t)
{
	for (pc_tally_member &m : t.m) {
		PC_HIP_CHECK(hipSetDevice(m.ctx->device));
		PC_HIP_CHECK(hipMemsetAsync(m.d_cells, 0, t.elems*sizeof(unsigned long long), m.ctx->stream));
		if (t.squares) PC_HIP_CHECK(hipMemsetAsync(m.d_sq, 0, 2*t.elems*sizeof(unsigned long long), m.ctx->stream));
	}
	for (int k = 0; k < 3; k++) t.n_entries[k] = 0;
	return PC_HIP_OK;
}

extern "C" {

void pc_hip_tally_stderr(size_t n_cells, const uint64_t *sums, const uint64_t *squares, int64_t n_started, double *out)
{
	pc_tally_stderr(n_cells, sums, squares, n_started, out);
}

void pc_hip_select_transmission(size_t n_energies, const uint64_t *passed_w, const uint64_t *rejected_w, const uint64_t *passed_w2,
	const uint64_t *rejected_w2, double *T, double *T_err)
{
	pc_tally_transmission(n_energies, passed_w, rejected_w, passed_w2, rejected_w2, T, T_err);
}

} /* extern "C" */

#endif /* PC_TALLY_HOST_ONLY */
#endif /* PC_TALLY_H */

/*
 * pc_select.h -- selections: up to eight cuts on per-entry quantities of the last run, ANDed, evaluated once per entry on the device
 * (include/polycap-hip.h, pc_hip_select_*).  A cut is a one-bin histogram axis and a flag negate: the value and the bin are pc_hist.h's
 * (pc_hist_value, pc_hist_bin), "inside" is bin 0.  One streaming pass over the entries a histogram reads (pc_spot_source) leaves one
 * mask byte per entry and the exact totals: how many pass, and per energy the sum of the quantised weights (pc_spot_q) of the passing
 * and of the rejected entries.  Any tally (pc_tally.h) is then filled through the mask: pc_tally_add skips what the mask rejects.
 *
 * A mask belongs to the entries it was made from: the selection remembers the context's entries_epoch per kind, and an add through a
 * mask of other entries is refused (pc_select_gate).
 *
 * The first part (the check of a cut, pc_select_pass, the parser of the public call's variable) compiles for the host as well:
 * -DPC_SELECT_HOST_ONLY stops the header after it.
 */
#ifndef PC_SELECT_H
#define PC_SELECT_H

#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "polycap-hip.h"
#include "pc_hist.h"

#define PC_SELECT_MAX_CUTS 8

/* the cuts as the kernel takes them: ax[k].n_bins = 1, ax[k].zp = z[nmax] + d */
struct pc_select_geo {
	pc_hist_axis_k ax[PC_SELECT_MAX_CUTS];
	int negate[PC_SELECT_MAX_CUTS];
	int nc;
	int need_start, need_travel, need_n;      /* which of the optional fields some cut reads (pc_hist_load) */
};

/* 1 when the entry passes every cut: pass_k = (the entry is in bin 0 of the cut's one-bin axis) XOR negate */
static inline __host__ __device__ int pc_select_pass(const pc_select_geo &g, const pc_hist_entry &e)
{
	for (int k = 0; k < g.nc; k++) {
		const int inside = pc_hist_axis_bin(g.ax[k], e) == 0;
		if (inside == (g.negate[k] != 0)) return 0;
	}
	return 1;
}

/* one cut of a spec: false and the reason in *why (it names the field) when it is refused */
static inline bool pc_select_cut_check(const pc_hip_select_cut &c, std::string *why)
{
	if (!pc_hist_axis_check(c.axis, PC_JOINT_N_QUANTITIES, why)) return false;
	if (c.axis.n_bins != 1)
		*why = "n_bins must be 1 for a cut, got " + std::to_string(c.axis.n_bins);
	else if (c.negate != 0 && c.negate != 1)
		*why = "negate must be 0 or 1, got " + std::to_string(c.negate);
	return why->empty();
}

/* a whole spec: the reason names the cut number and the field */
static inline bool pc_select_spec_check(const pc_hip_select_spec *spec, std::string *why)
{
	if (!spec) { *why = "spec must not be NULL"; return false; }
	if (spec->n_cuts < 1 || spec->n_cuts > PC_SELECT_MAX_CUTS || !spec->cuts) {
		*why = "n_cuts: 1 to 8 cuts are needed, got " + std::to_string(spec->n_cuts);
		return false;
	}
	for (int k = 0; k < spec->n_cuts; k++) {
		std::string w;
		if (!pc_select_cut_check(spec->cuts[k], &w)) {
			*why = "cut " + std::to_string(k) + ": " + w;
			return false;
		}
	}
	return true;
}

/* the cuts of a checked spec for the kernel and for pc_select_pass; zexit = z[nmax] */
static inline pc_select_geo pc_select_make_geo(const pc_hip_select_spec *spec, double zexit)
{
	pc_select_geo g;
	memset(&g, 0, sizeof(g));
	g.nc = spec->n_cuts;
	for (int k = 0; k < g.nc; k++) {
		const pc_hip_hist_axis &x = spec->cuts[k].axis;
		pc_hist_axis_k &a = g.ax[k];
		a.zp = zexit + x.d;          /* once, on the host */
		a.cx = x.cx; a.cy = x.cy; a.lo = x.lo; a.hi = x.hi;
		a.quantity = x.quantity; a.n_bins = 1;
		g.negate[k] = spec->cuts[k].negate;
		if (x.quantity == PC_HIST_N_REFL) g.need_n = 1;
		if (x.quantity == PC_HIST_D_TRAVEL) g.need_travel = 1;
		if (x.quantity == PC_HIST_R_START || x.quantity == PC_JOINT_START_X || x.quantity == PC_JOINT_START_Y) g.need_start = 1;
	}
	return g;
}

/* "A:B" into two doubles */
static inline bool pc_select_parse_pair(const char *v, double *a, double *b)
{
	char *end = nullptr;
	errno = 0;
	*a = strtod(v, &end);
	if (end == v || errno != 0 || *end != ':') return false;
	v = end + 1;
	*b = strtod(v, &end);
	return !(end == v || errno != 0 || *end != '\0');
}

/* one cut: comma-separated key=value parts in the grammar of a POLYCAP_HIST axis without bins, and the word "not" */
static inline const char *pc_select_parse_cut(const std::string &item, pc_hip_select_cut *c)
{
	static const char *names[PC_JOINT_N_QUANTITIES] = { "x", "y", "r", "slope_x", "slope_y", "tan_theta", "nrefl", "dtravel", "r_start", "z", "start_x", "start_y" };
	bool have_axis = false, have_range = false;
	memset(c, 0, sizeof(*c));
	c->axis.n_bins = 1;
	size_t at = 0;
	while (at <= item.size()) {
		size_t comma = item.find(',', at);
		if (comma == std::string::npos) comma = item.size();
		const std::string part = item.substr(at, comma - at);
		at = comma + 1;
		if (part == "not") { c->negate = 1; continue; }
		const size_t eq = part.find('=');
		if (eq == std::string::npos) return "every part of a cut must be key=value or the word not";
		const std::string key = part.substr(0, eq), val = part.substr(eq + 1);
		char *end = nullptr;
		if (key == "axis") {
			c->axis.quantity = -1;
			for (int q = 0; q < PC_JOINT_N_QUANTITIES; q++)
				if (val == names[q]) c->axis.quantity = q;
			if (c->axis.quantity < 0) return "axis must be one of x y r slope_x slope_y tan_theta nrefl dtravel r_start z start_x start_y";
			have_axis = true;
		} else if (key == "d") {
			errno = 0;
			c->axis.d = strtod(val.c_str(), &end);
			if (end == val.c_str() || errno != 0 || *end != '\0') return "d must be a distance in cm";
		} else if (key == "centre") {
			if (!pc_select_parse_pair(val.c_str(), &c->axis.cx, &c->axis.cy)) return "centre must be CX:CY in cm";
		} else if (key == "range") {
			if (!pc_select_parse_pair(val.c_str(), &c->axis.lo, &c->axis.hi)) return "range must be LO:HI";
			have_range = true;
		} else {
			return "unknown key of a cut (axis, d, centre, range, and the word not)";
		}
	}
	return (have_axis && have_range) ? nullptr : "a cut needs axis and range";
}

/* pc_hip_select_parse: a value of POLYCAP_SELECT into cuts [PC_SELECT_MAX_CUTS] and *n_cuts, checked as a spec is; false and the
 * reason (it names the item) in *why otherwise */
static inline bool pc_select_parse(const char *value, pc_hip_select_cut *cuts, int *n_cuts, std::string *why)
{
	*n_cuts = 0;
	if (!value) { *why = "value must not be NULL"; return false; }
	const std::string v(value);
	size_t at = 0;
	int n_item = 0;
	while (at < v.size()) {
		size_t semi = v.find(';', at);
		if (semi == std::string::npos) semi = v.size();
		const std::string item = v.substr(at, semi - at);
		at = semi + 1;
		if (item.empty()) continue;
		const char *bad = nullptr;
		pc_hip_select_cut c;
		if (item.compare(0, 5, "axis=") != 0) bad = "every item must be a cut (axis=NAME,...)";
		else if (*n_cuts >= PC_SELECT_MAX_CUTS) bad = "at most 8 cuts";
		else bad = pc_select_parse_cut(item, &c);
		if (bad) {
			*why = "item " + std::to_string(n_item) + ": " + bad;
			return false;
		}
		cuts[(*n_cuts)++] = c;
		n_item++;
	}
	if (*n_cuts == 0) { *why = "at least one cut is needed"; return false; }
	const pc_hip_select_spec spec = { *n_cuts, cuts };
	return pc_select_spec_check(&spec, why);
}

#ifndef PC_SELECT_HOST_ONLY

/* One lane per entry and wave-sized batches: lane j of a wave evaluates entry base + j, writes its mask byte and the wave shares the
 * 64 verdicts by ballot.  The weights of the batch are then read with the energies across the lanes as in pc_tally_lane_map (gw lanes
 * per entry, 64 / gw entries per step: contiguous 8-byte loads), every lane adding those of its one energy to a passed or a rejected
 * sum in registers for the whole pass.  Workgroup (x, c) does energies [64c, 64c + 64); c = 0 writes the mask and counts.  At the end
 * the lanes of one energy are summed across the wave (shuffles), the waves in LDS, and the workgroup adds its sums with one 64-bit
 * atomic per energy and sum: per workgroup, not per entry -- every entry would hit the same few addresses.
 * Every chunk loads its entries and evaluates the cuts again for the verdicts (a few fields next to the 64 weights per entry it reads).
 * tot: n_pass, a spare word, passed_w [ne], rejected_w [ne].
 * Q: the selection tracks squares.  Every lane also keeps the sums of W*W (pc_tally_sq) of its passing and of its rejected entries as
 * two (lo, hi) pairs in registers, and they take the same way: shuffles and LDS with carry, then one pc_atomic_add128 per workgroup,
 * energy and sum into tot2: passed_w2 [ne][2], rejected_w2 [ne][2].  The build without reads no tot2. */
#define PC_SELECT_BLOCK 256
template <bool Q>
__global__ void __launch_bounds__(PC_SELECT_BLOCK) pc_select_kernel(pc_spot_src s, pc_select_geo g, int ne, unsigned char *mask, unsigned long long *tot,
	unsigned long long *tot2)
{
	constexpr int NRED = 2*64 + 1 + (Q ? 4*64 : 0);
	__shared__ unsigned long long red[NRED];
	unsigned long long *red2 = red + 2*64 + 1;      /* passed [64][2], rejected [64][2], Q only */
	const int e0 = blockIdx.y*64;
	const int en = (ne - e0 < 64) ? ne - e0 : 64;
	for (int k = threadIdx.x; k < NRED; k += blockDim.x) red[k] = 0ull;
	__syncthreads();
	const int gw = pc_tally_gw(en), lane = threadIdx.x & 63, sub = lane & (gw - 1), per = 64 / gw;
	const long long wave = ((long long)blockIdx.x*blockDim.x + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x*blockDim.x) >> 6;
	unsigned long long acc_p = 0ull, acc_r = 0ull, n_pass = 0ull;
	unsigned long long p2_lo = 0ull, p2_hi = 0ull, r2_lo = 0ull, r2_hi = 0ull;
	for (long long base = wave*64; base < s.n; base += n_waves*64) {       /* uniform over the wave */
		const long long i = base + lane;
		int pass = 0;
		if (i < s.n) {
			pc_hist_entry e;
			pc_hist_load(s, i, g.need_start, g.need_travel, g.need_n, e);
			pass = pc_select_pass(g, e);
			if (blockIdx.y == 0) mask[i] = (unsigned char)pass;
		}
		const unsigned long long verdicts = __ballot(pass);
		n_pass += (unsigned long long)__popcll(verdicts);
		if (sub < en)
			for (int t = 0; t < gw; t++) {
				const int j = t*per + lane / gw;
				if (base + j >= s.n) break;
				const unsigned long long q = pc_spot_q(s.w[(base + j)*s.ws + e0 + sub]);
				unsigned long long q2_lo = 0ull, q2_hi = 0ull;
				if (Q) pc_tally_sq(q, q2_lo, q2_hi);
				if ((verdicts >> j) & 1ull) {
					acc_p += q;
					if (Q) pc_add128(p2_lo, p2_hi, q2_lo, q2_hi);
				} else {
					acc_r += q;
					if (Q) pc_add128(r2_lo, r2_hi, q2_lo, q2_hi);
				}
			}
	}
	/* lanes lane ^ gw, lane ^ 2gw, ... have the same energy */
	for (int off = gw; off < 64; off <<= 1) {
		acc_p += __shfl_xor(acc_p, off);
		acc_r += __shfl_xor(acc_r, off);
		if (Q) {
			const unsigned long long a_lo = __shfl_xor(p2_lo, off), a_hi = __shfl_xor(p2_hi, off);
			const unsigned long long b_lo = __shfl_xor(r2_lo, off), b_hi = __shfl_xor(r2_hi, off);
			pc_add128(p2_lo, p2_hi, a_lo, a_hi);
			pc_add128(r2_lo, r2_hi, b_lo, b_hi);
		}
	}
	if (lane < gw && sub < en) {
		if (acc_p) atomicAdd(&red[sub], acc_p);
		if (acc_r) atomicAdd(&red[64 + sub], acc_r);
		if (Q && (p2_lo | p2_hi)) pc_atomic_add128(&red2[2*sub], p2_lo, p2_hi);
		if (Q && (r2_lo | r2_hi)) pc_atomic_add128(&red2[2*64 + 2*sub], r2_lo, r2_hi);
	}
	if (lane == 0 && n_pass) atomicAdd(&red[128], n_pass);
	__syncthreads();
	for (int k = threadIdx.x; k < en; k += blockDim.x) {
		if (red[k]) atomicAdd(tot + 2 + e0 + k, red[k]);
		if (red[64 + k]) atomicAdd(tot + 2 + ne + e0 + k, red[64 + k]);
		if (Q && (red2[2*k] | red2[2*k + 1])) pc_atomic_add128(tot2 + 2*(e0 + k), red2[2*k], red2[2*k + 1]);
		if (Q && (red2[2*64 + 2*k] | red2[2*64 + 2*k + 1])) pc_atomic_add128(tot2 + 2*(ne + e0 + k), red2[2*64 + 2*k], red2[2*64 + 2*k + 1]);
	}
	if (threadIdx.x == 0 && blockIdx.y == 0 && red[128]) atomicAdd(tot, red[128]);
}

/* ---- the object: per member of the group (one member without a group) a mask per kind and the totals of the three kinds */
struct pc_select_member {
	pc_hip_ctx *ctx = nullptr;
	pc_dev_buf<unsigned char> d_mask[3];
	pc_dev_buf<unsigned long long> d_tot;       /* [3][2 + 2 ne] */
	pc_dev_buf<unsigned long long> d_tot2;      /* [3][2][ne][2]: passed_w2, rejected_w2 as (lo, hi) pairs, where the selection tracks squares */
	long long n[3] = {0, 0, 0};                  /* entries the mask of a kind covers */
	long long n_pass[3] = {0, 0, 0};             /* of which pass (once fetched) */
	unsigned long long epoch[3] = {0, 0, 0};     /* ctx->entries_epoch the mask of a kind was made at */
	/* pc_gather.h: the ascending positions of a kind's passing entries [n_pass], built by the first gather after an apply */
	pc_dev_buf<unsigned int> d_idx[3];
	int idx_valid[3] = {0, 0, 0};
	pc_dev_buf<unsigned int> d_tile_cnt, d_tile_off;      /* the compaction's tile counts [tiles] and offsets [tiles + 1] */
	pc_dev_buf<unsigned long long> d_stage;               /* the gathered rows of one chunk */
	/* pc_draw.h: the sums of V over the tiles [tiles] and their scan [tiles + 1] for one (kind, energy, tile), until the next apply */
	pc_dev_buf<unsigned long long> d_draw_sum, d_draw_off;
	pc_dev_buf<unsigned int> d_draw_list;                 /* the local positions of one call's draws */
	int draw_valid = 0, draw_kind = 0, draw_energy = 0;
	long long draw_tile = 0;
	unsigned long long draw_total = 0;                    /* the member's T_j */
};

struct pc_hip_select {
	std::vector<pc_select_member> m;
	pc_hip_group *group = nullptr;
	pc_select_geo geo;
	std::vector<pc_hip_select_cut> cuts;
	int ne = 0;
	int applied[3] = {0, 0, 0};
	int fetched[3] = {0, 0, 0};                  /* the totals of the kind are on the host */
	std::vector<unsigned long long> tot;         /* [3][2 + 2 ne], summed over the members */
	int squares = 0;                             /* every apply also sums W*W (pc_hip_select_track_squares) */
	std::vector<unsigned long long> tot2;        /* [3][2][ne][2], summed over the members with carry */
	~pc_hip_select();
};

/* what was enqueued on a member's stream (the applies, and the gated adds that read the masks) is over before the buffers go */
inline pc_hip_select::~pc_hip_select()
{
	for (pc_select_member &mb : m) {
		if (!mb.ctx) continue;
		(void)hipSetDevice(mb.ctx->device);
		if (mb.ctx->stream) (void)hipStreamSynchronize(mb.ctx->stream);
	}
	m.clear();
}

static int pc_select_make(const std::vector<pc_hip_ctx *> &ctxs, pc_hip_group *group, const pc_hip_select_spec *spec, pc_hip_select **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_create: select must not be NULL");
	*out = nullptr;
	int st = pc_hip_select_validate(spec);
	if (st) return st;
	const pc_hip_ctx *c0 = ctxs[0];
	pc_hip_select *s = new pc_hip_select();
	s->group = group;
	s->ne = c0->host.pm.n_energies;
	s->geo = pc_select_make_geo(spec, c0->host.z[c0->host.pm.nmax]);
	s->cuts.assign(spec->cuts, spec->cuts + spec->n_cuts);
	const size_t per_kind = 2 + 2*(size_t)s->ne;
	s->tot.assign(3*per_kind, 0ull);
	for (pc_hip_ctx *c : ctxs) {
		s->m.emplace_back();
		pc_select_member &mb = s->m.back();
		mb.ctx = c;
		st = pc_tally_hip(hipSetDevice(c->device), "pc_hip_select_create");
		if (!st) st = mb.d_tot.grow(3*per_kind, "pc_hip_select_create: could not allocate the totals");
		if (st) { delete s; return st; }
	}
	*out = s;
	return PC_HIP_OK;
}

/* the totals of `kind` from every member to the host, once per apply (waits for the apply) */
static int pc_select_fetch(pc_hip_select *s, int kind)
{
	if (s->fetched[kind]) return PC_HIP_OK;
	const size_t per_kind = 2 + 2*(size_t)s->ne;
	std::vector<unsigned long long> part(per_kind);
	unsigned long long *sum = s->tot.data() + (size_t)kind*per_kind;
	for (size_t k = 0; k < per_kind; k++) sum[k] = 0ull;
	for (pc_select_member &mb : s->m) {
		mb.n_pass[kind] = 0;
		if (mb.n[kind] == 0) continue;
		PC_HIP_CHECK(hipSetDevice(mb.ctx->device));
		PC_HIP_CHECK(hipMemcpyAsync(part.data(), mb.d_tot + (size_t)kind*per_kind, per_kind*sizeof(unsigned long long), hipMemcpyDeviceToHost, mb.ctx->stream));
		PC_HIP_CHECK(hipStreamSynchronize(mb.ctx->stream));
		mb.n_pass[kind] = (long long)part[0];
		for (size_t k = 0; k < per_kind; k++) sum[k] += part[k];
		sum[1] += (unsigned long long)mb.n[kind];          /* n_seen */
	}
	if (s->squares) {
		const size_t per2 = 4*(size_t)s->ne;
		std::vector<unsigned long long> part2(per2);
		unsigned long long *sum2 = s->tot2.data() + (size_t)kind*per2;
		for (size_t k = 0; k < per2; k++) sum2[k] = 0ull;
		for (pc_select_member &mb : s->m) {
			if (mb.n[kind] == 0) continue;
			PC_HIP_CHECK(hipSetDevice(mb.ctx->device));
			PC_HIP_CHECK(hipMemcpyAsync(part2.data(), mb.d_tot2 + (size_t)kind*per2, per2*sizeof(unsigned long long), hipMemcpyDeviceToHost, mb.ctx->stream));
			PC_HIP_CHECK(hipStreamSynchronize(mb.ctx->stream));
			for (size_t k = 0; k < per2; k += 2) pc_add128(sum2[k], sum2[k + 1], part2[k], part2[k + 1]);
		}
	}
	s->fetched[kind] = 1;
	return PC_HIP_OK;
}

/* declared in pc_tally.h */
static int pc_select_gate(pc_hip_select *sel, const std::vector<pc_hip_ctx *> &ctxs, const pc_hip_group *g, int kind, const char *who,
	std::vector<pc_spot_src> &src, std::vector<long long> &passing)
{
	const std::string w(who);
	bool same = sel->group == g && sel->m.size() == ctxs.size();
	for (size_t k = 0; same && k < ctxs.size(); k++) same = sel->m[k].ctx == ctxs[k];
	if (!same)
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the selection and the tally belong to different owners (make both on the same context or the same group)");
	if (!sel->applied[kind])
		return pc_fail(PC_HIP_ERR_INVALID, w + ": the selection was not applied for kind " + std::to_string(kind) + " (pc_hip_select_apply)");
	for (size_t k = 0; k < ctxs.size(); k++)
		if (sel->m[k].epoch[kind] != ctxs[k]->entries_epoch || sel->m[k].n[kind] != src[k].n)
			return pc_fail(PC_HIP_ERR_INVALID, w + ": the selection's mask is stale: the entries of kind " + std::to_string(kind) + " were replaced after it was applied");
	const int st = pc_select_fetch(sel, kind);
	if (st) return st;
	passing.resize(ctxs.size());
	for (size_t k = 0; k < ctxs.size(); k++) {
		src[k].mask = sel->m[k].d_mask[kind];
		passing[k] = sel->m[k].n_pass[kind];
	}
	return PC_HIP_OK;
}

extern "C" {

int pc_hip_select_validate(const pc_hip_select_spec *spec)
{
	std::string why;
	if (!pc_select_spec_check(spec, &why)) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_validate: " + why);
	return PC_HIP_OK;
}

int pc_hip_select_create(pc_hip_ctx *ctx, const pc_hip_select_spec *spec, pc_hip_select **select)
{
	if (!ctx) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_create: ctx must not be NULL");
	return pc_select_make(std::vector<pc_hip_ctx *>{ctx}, nullptr, spec, select);
}

int pc_hip_group_select_create(pc_hip_group *group, const pc_hip_select_spec *spec, pc_hip_select **select)
{
	if (!group) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_group_select_create: group must not be NULL");
	return pc_select_make(group->ctx, group, spec, select);
}

void pc_hip_select_destroy(pc_hip_select *select)
{
	delete select;
}

int pc_hip_select_apply(pc_hip_select *sel, int kind)
{
	static const char *who = "pc_hip_select_apply";
	if (!sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_apply: select must not be NULL");
	std::vector<pc_hip_ctx *> ctxs;
	for (const pc_select_member &mb : sel->m) ctxs.push_back(mb.ctx);
	std::vector<pc_spot_src> src;
	long long n = 0;
	int st = pc_tally_sources(ctxs, sel->group, kind, who, src, &n);
	if (st) return st;
	if (n > (long long)0xffffffffll)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_apply: a kind of more than 2^32 - 1 entries cannot be applied (the exact sums could wrap beyond)");
	sel->applied[kind] = 0;          /* until every member's mask is enqueued */
	sel->fetched[kind] = 0;
	const size_t per_kind = 2 + 2*(size_t)sel->ne;
	for (size_t k = 0; k < sel->m.size(); k++) {
		pc_select_member &mb = sel->m[k];
		pc_hip_ctx *c = mb.ctx;
		mb.n[kind] = 0;
		mb.idx_valid[kind] = 0;          /* the index list of the old mask (pc_gather.h) */
		if (mb.draw_kind == kind) mb.draw_valid = 0;      /* and its tile sums (pc_draw.h) */
		if (src[k].n == 0) { mb.epoch[kind] = c->entries_epoch; continue; }
		PC_HIP_CHECK(hipSetDevice(c->device));
		/* a gated add of this stream may still read the old mask */
		if (mb.d_mask[kind].cap < (size_t)src[k].n) PC_HIP_CHECK(hipStreamSynchronize(c->stream));
		st = mb.d_mask[kind].grow((size_t)src[k].n, "pc_hip_select_apply: could not allocate the mask");
		if (st) return st;
		unsigned long long *tot = mb.d_tot + (size_t)kind*per_kind;
		unsigned long long *tot2 = sel->squares ? mb.d_tot2 + (size_t)kind*4*(size_t)sel->ne : nullptr;
		PC_HIP_CHECK(hipMemsetAsync(tot, 0, per_kind*sizeof(unsigned long long), c->stream));
		if (tot2) PC_HIP_CHECK(hipMemsetAsync(tot2, 0, 4*(size_t)sel->ne*sizeof(unsigned long long), c->stream));
		const long long chunks = (sel->ne + 63)/64;
		const long long bx = pc_tally_grid_cap((8ll*c->n_cu + chunks - 1)/chunks, src[k].n, PC_SELECT_BLOCK);
		hipLaunchKernelGGL(tot2 ? pc_select_kernel<true> : pc_select_kernel<false>, dim3((unsigned)bx, (unsigned)chunks), dim3(PC_SELECT_BLOCK), 0, c->stream,
		                   src[k], sel->geo, sel->ne, (unsigned char *)mb.d_mask[kind], tot, tot2);
		PC_HIP_CHECK(hipGetLastError());
		mb.n[kind] = src[k].n;
		mb.epoch[kind] = c->entries_epoch;
	}
	sel->applied[kind] = 1;
	return PC_HIP_OK;
}

int pc_hip_select_read(pc_hip_select *sel, int64_t *n_pass, int64_t *n_seen, uint64_t *passed_w, uint64_t *rejected_w)
{
	if (!sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_read: select must not be NULL");
	const size_t ne = (size_t)sel->ne, per_kind = 2 + 2*ne;
	for (int kind = 0; kind < 3; kind++) {
		const unsigned long long *t = sel->tot.data() + (size_t)kind*per_kind;
		if (sel->applied[kind]) {
			const int st = pc_select_fetch(sel, kind);
			if (st) return st;
		}
		const bool have = sel->applied[kind] != 0;
		if (n_pass) n_pass[kind] = have ? (int64_t)t[0] : 0;
		if (n_seen) n_seen[kind] = have ? (int64_t)t[1] : 0;
		for (size_t e = 0; e < ne; e++) {
			if (passed_w) passed_w[kind*ne + e] = have ? t[2 + e] : 0;
			if (rejected_w) rejected_w[kind*ne + e] = have ? t[2 + ne + e] : 0;
		}
	}
	return PC_HIP_OK;
}

int pc_hip_select_track_squares(pc_hip_select *sel)
{
	static const char *who = "pc_hip_select_track_squares";
	if (!sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_track_squares: select must not be NULL");
	if (sel->applied[0] | sel->applied[1] | sel->applied[2])
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_track_squares: squares can be tracked only before the selection is applied for the first time");
	if (sel->squares) return PC_HIP_OK;
	const size_t n = 3*4*(size_t)sel->ne;
	int st = PC_HIP_OK;
	for (pc_select_member &mb : sel->m) {
		st = pc_tally_hip(hipSetDevice(mb.ctx->device), who);
		if (!st) st = mb.d_tot2.grow(n, "pc_hip_select_track_squares: could not allocate the totals of the squares");
		if (st) break;
	}
	if (st) {
		for (pc_select_member &mb : sel->m) {
			(void)hipSetDevice(mb.ctx->device);
			mb.d_tot2.reset();
		}
		return st;
	}
	sel->tot2.assign(n, 0ull);
	sel->squares = 1;
	return PC_HIP_OK;
}

int pc_hip_select_read_squares(pc_hip_select *sel, uint64_t *passed_w2, uint64_t *rejected_w2)
{
	if (!sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_read_squares: select must not be NULL");
	if (!sel->squares)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_read_squares: the selection does not track squares (pc_hip_select_track_squares before the first apply)");
	const size_t ne = (size_t)sel->ne;
	for (int kind = 0; kind < 3; kind++) {
		if (sel->applied[kind]) {
			const int st = pc_select_fetch(sel, kind);
			if (st) return st;
		}
		const bool have = sel->applied[kind] != 0;
		const unsigned long long *t = sel->tot2.data() + (size_t)kind*4*ne;
		for (size_t k = 0; k < 2*ne; k++) {
			if (passed_w2) passed_w2[kind*2*ne + k] = have ? t[k] : 0;
			if (rejected_w2) rejected_w2[kind*2*ne + k] = have ? t[2*ne + k] : 0;
		}
	}
	return PC_HIP_OK;
}

int pc_hip_select_info(const pc_hip_select *sel, int32_t *n_cuts, int32_t *n_energies, pc_hip_select_cut *cuts)
{
	if (!sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_select_info: select must not be NULL");
	if (n_cuts) *n_cuts = (int32_t)sel->cuts.size();
	if (n_energies) *n_energies = sel->ne;
	if (cuts)
		for (size_t k = 0; k < sel->cuts.size(); k++) cuts[k] = sel->cuts[k];
	return PC_HIP_OK;
}

int pc_hip_spot_add_selected(pc_hip_spot *spot, int kind, pc_hip_select *sel)
{
	if (!spot || !sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_spot_add_selected: spot and select must not be NULL");
	return pc_tally_add(*spot, kind, "pc_hip_spot_add_selected",
		[spot](size_t k, const pc_spot_src &s, int) { return pc_spot_launch(spot, spot->m[k], s); }, sel);
}

int pc_hip_beam_add_selected(pc_hip_beam *beam, int kind, pc_hip_select *sel)
{
	if (!beam || !sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_beam_add_selected: beam and select must not be NULL");
	return pc_tally_add(*beam, kind, "pc_hip_beam_add_selected",
		[beam](size_t k, const pc_spot_src &s, int kd) { return pc_beam_launch(beam, beam->m[k], s, kd); }, sel);
}

int pc_hip_hist_add_selected(pc_hip_hist *hist, int kind, pc_hip_select *sel)
{
	if (!hist || !sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_hist_add_selected: hist and select must not be NULL");
	return pc_cells_add<1>(hist, kind, "pc_hip_hist_add_selected", sel);
}

int pc_hip_joint_add_selected(pc_hip_joint *joint, int kind, pc_hip_select *sel)
{
	if (!joint || !sel) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_joint_add_selected: joint and select must not be NULL");
	return pc_cells_add<2>(joint, kind, "pc_hip_joint_add_selected", sel);
}

int pc_hip_select_parse(const char *value, pc_hip_select_cut *cuts, int32_t *n_cuts, char *why, size_t why_len)
{
	pc_hip_select_cut tmp[PC_SELECT_MAX_CUTS];
	int n = 0;
	std::string bad;
	const bool ok = pc_select_parse(value, tmp, &n, &bad);
	if (why && why_len > 0) snprintf(why, why_len, "%s", ok ? "" : bad.c_str());
	if (!ok) return PC_HIP_ERR_INVALID;
	if (cuts) memcpy(cuts, tmp, sizeof(pc_hip_select_cut)*(size_t)n);
	if (n_cuts) *n_cuts = n;
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_SELECT_HOST_ONLY */
#endif /* PC_SELECT_H */

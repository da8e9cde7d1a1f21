/*
 * pc_ctx.h -- the GPU context (pc_hip_ctx) with the owners declared beside it -- relay state, per-lane scratch, scan state, batch
 * store -- and the calls that make and end one.  The image store, the leak run and the sweep certificate come from headers of their
 * own ahead of it.  Included by pc_kernels.hip.
 */
#ifndef PC_CTX_H
#define PC_CTX_H

/* what a context was last asked to do (pc_hip_ctx::last_call) */
enum { PC_CALL_NONE = 0, PC_CALL_RUN, PC_CALL_RUN_LEAK, PC_CALL_EXPLICIT, PC_CALL_SCAN, PC_CALL_RELAY };

/* what the context a relay was traced into keeps of it, and the scratch of relays into it (pc_relay.h, pc_emit.h) */
struct pc_relay_state {
	pc_dev_buf<long long> d_map;           /* position in the first optic's store of every injected photon */
	pc_dev_buf<unsigned long long> d_scan; /* the scratch of the two compactions, then the finish kernel's counters (PC_RELAY_SCAN_WORDS) */
	pc_dev_buf<int> d_emap;                /* emit relays: which of the first optic's energies every energy of this context takes its weight from */
	pc_dev_buf<double> d_mu;               /* slab emits: the sample's attenuation coefficients, mu_in [the first optic's energies] before mu_out [this context's] */
	int acc_lds = 1;                       /* option "relay_acc_lds": 0 = the finish kernel adds to the global sums at once (tests) */
	int64_t counters[8] = {0};
	int64_t lost[3] = {0, 0, 0};           /* photons lost between the optics, at [outcome - PC_RELAY_REJECT]: rejected by the selection, missed
	                                        * the entrance plane (emit: the sample), missed the detector (emit only) */
	int kind = 0;                          /* PC_RELAY_KIND_*: what the relay it holds was */
};

/* Per-lane scratch of a trace launch: the weights of more than 8 energies, and the reflection logs of the logging kernel.  Grown by
 * pc_launch_planned alone.  A context has one for its runs and explicit launches and its scans have another, so that a scan leaves
 * everything of the last run as it was; each owner gives it the words for a refused allocation. */
struct pc_lane_scratch {
	pc_dev_buf<double> d_wscratch, d_rlog;
	const char *no_wscratch, *no_rlog;
	pc_lane_scratch(const char *w, const char *l) : no_wscratch(w), no_rlog(l) {}
	int grow(size_t w_elems, size_t l_elems)
	{
		int st = d_wscratch.grow(w_elems, no_wscratch);
		return st ? st : d_rlog.grow(l_elems, no_rlog);
	}
};

/* scans (pc_scan.h): buffers of their own, so that a scan leaves everything of the last run as it was */
struct pc_scan_state {
	pc_dev_buf<pc_totals> d_totals;        /* work counter and scheduler statistics of the last scan launch */
	pc_dev_buf<unsigned long long> d_tot;  /* per point: 6 counters, 2*ne weight sums, 2*ne squared-weight sums (pc_kargs::sumw of a scan) */
	pc_dev_buf<pc_scan_point> d_pts;
	pc_lane_scratch lanes{"pc_hip_scan_run: could not allocate the per-lane weight scratch", "pc_hip_scan_run: could not allocate the reflection logs"};
	int log = 0;                           /* option "scan_log": scans that can log their reflections do (pc_plan_input::scan_log; kept here
	                                        * because pc_launch_opts is the fixed list tests/plan/plan_host.cpp counts) */
	int kernel = -1;                       /* pc_hip_scan_last_kernel */
	pc_event_handle ev0, ev1;
	long long points = 0;                  /* points of the last scan call (0: none yet) */
	int squares = 0;                       /* the last scan summed the squared weights */
	int pending = 0;                       /* the last scan has not been waited for */
	float ms = 0.f;

	int buffers(size_t ne, int64_t n_points);
};

/* explicit-photon calls (polycap_photon_launch, polycap_source_get_photon): one device buffer and one pinned host
 * buffer, kept between calls, so that a single photon costs two copies and a launch instead of ten copies and
 * as many allocations (pc_batch.h) */
struct pc_batch;
struct pc_batch_store {
	pc_dev_buf<double> d_buf;
	pc_host_buf<double, PC_PIN_OR_PLAIN> h_buf;

	int buffers(size_t elems);
	int layout(size_t ne, int64_t n, bool host, pc_batch &b);
	int upload(hipStream_t stream, const pc_batch &b, const double *start_coords, const double *start_dir, const double *start_elecv);
	int download(hipStream_t stream, const pc_batch &b, const double *start_elecv, int32_t *rc, double *weights, double *exit_coords,
	             double *exit_dir, double *exit_elecv, int64_t *i_refl, double *d_travel, int leak);
};

struct pc_hip_ctx {
	pc_stream_handle stream;               /* first: destroyed after everything that may still be queued on it.  The context's one stream: a launch
	                                        * that goes elsewhere says so in its pc_launch_site */
	int device = 0;
	int n_cu = 256;
	pc_event_handle ev0, ev1;
	pc_host_tables host;
	pc_dev_buf<double> d_tables;           /* z, cap, zh, cap2, hexd, idz, ext: 7 x npts */
	pc_dev_buf<pc_energy_const> d_ec;
	pc_dev_buf<double> d_ec_soa;
	pc_dev_buf<pc_marg4> d_mg;             /* block-certificate records, npts */
	pc_dev_buf<pc_drdev> d_dr;             /* leak path: chord deviations of cap, npts */
	pc_launch_opts opts;                   /* the options that decide a launch (pc_plan.h) */
	pc_sweep_cert cert;                    /* what the logging kernel is told about the energies: made by its first launch (pc_sweep_cert.h) */
	/* the plain run's bookkeeping (pc_run.h; the relay and the explicit launches write some of it) */
	double refl_per_launch = -1.;  /* EVENT visits (reflections, mostly) per launch in the last source run of this context; < 0: not known.
	                                * A big first run is preceded by a probe of 32768 slots (results unused) */
	int last_kernel = -1;          /* pc_hip_last_kernel */
	int last_run_plain = 0;        /* the last run was pc_hip_transmission_run (its counters tell refl_per_launch) */
	int run_squares = 0;           /* the last run did so (pc_hip_transmission_moments) */
	long long run_slots = 0;
	long long run_slot0 = 0;       /* first slot of the last source run: an emission draws on the stream of its photon's slot (pc_emit.h) */
	int run_pending = 0;
	float last_ms = 0.f;
	/* last run */
	pc_dev_buf<pc_totals> d_totals;        /* totals_bytes: the layout of pc_totals.h */
	size_t totals_bytes = 0;
	pc_image_store img;                    /* the exit-photon images of the last run, their options and the way out (pc_images.h) */
	pc_dev_buf<unsigned long long> d_work; /* one work counter per part */
	pc_lane_scratch lanes{"could not allocate the per-lane weight scratch", "could not allocate the reflection logs"};
	pc_batch_store batch;                  /* the buffers of explicit-photon calls */
	pc_leak_run leak;                      /* leak_calc=true runs: buffers, options, the run in flight and its event lists (pc_leak_run.h) */
	unsigned long long entries_epoch = 0;  /* grows with every call that replaces the entries a tally reads (source run, leak run, relay into the
	                                        * context, explicit launch; not a scan): a selection's mask belongs to one value (pc_select.h) */
	pc_scan_state scan;                    /* scans: their buffers, events and what the last one left (pc_scan.h) */
	/* relays (pc_relay.h): what a context did last decides whether its exit photons can be relayed, and the context a relay was
	 * traced into keeps the relay's counters beside what a source run leaves */
	int last_call = PC_CALL_NONE;
	std::vector<double> energies;          /* the problem's energy grid as given: two contexts relay only over bit-equal grids */
	pc_relay_state relay;
	/* gathers of a selection's entries (pc_gather.h) */
	int gather_tile = 0;                   /* option "gather_tile": entries per compaction tile, 0 = automatic */
	long long gather_chunk_rows = 0;       /* option "gather_chunk_rows": rows per staging chunk, 0 = as many as fit in 128 MiB */
};

extern "C" {

int pc_hip_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

const char *pc_hip_last_error(void)
{
	return g_last_error.c_str();
}

void pc_hip_ctx_destroy(pc_hip_ctx *ctx)
{
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	delete ctx;
}

int pc_hip_ctx_create(const pc_hip_problem *problem, int device, pc_hip_ctx **out)
{
	if (!out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_ctx_create: ctx must not be NULL");
	*out = nullptr;
	int ndev = pc_hip_device_count();
	if (ndev <= 0) return pc_fail(PC_HIP_ERR_NO_DEVICE, "pc_hip_ctx_create: no HIP device available (the trace path has no CPU fallback)");
	if (device < 0 || device >= ndev) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_ctx_create: device index out of range");
	pc_hip_ctx *ctx = new pc_hip_ctx();
	ctx->device = device;
	std::string err;
	int rc = pc_build_tables(problem, ctx->host, err);
	if (rc) { delete ctx; return pc_fail(rc, "pc_hip_ctx_create: " + err); }
	ctx->energies.assign(problem->energies, problem->energies + problem->n_energies);
	const size_t npts = (size_t)ctx->host.pm.nmax + 1;
	if (npts > PC_MAX_PITCH) { delete ctx; return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_ctx_create: profile too long for the LDS tables (nmax <= 2047)"); }
#define PC_CTX_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::string m = std::string(#expr) + ": " + hipGetErrorString(_e); pc_hip_ctx_destroy(ctx); return pc_fail(PC_HIP_ERR_RUNTIME, m); } } while (0)
#define PC_CTX_GROW(buf, elems, what) do { int _st = (buf).grow((elems), "pc_hip_ctx_create: could not allocate " what); if (_st) { pc_hip_ctx_destroy(ctx); return _st; } } while (0)
	PC_CTX_CHECK(hipSetDevice(device));
	hipDeviceProp_t prop;
	PC_CTX_CHECK(hipGetDeviceProperties(&prop, device));
	ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	PC_CTX_CHECK(ctx->stream.ensure());
	if (const char *e = getenv("POLYCAP_PRODUCER"))          /* tests: force (1) or forbid (0) the launching-wave kernel */
		if (*e == '0' || *e == '1') ctx->opts.producer = *e - '0';
	PC_CTX_CHECK(ctx->ev0.ensure(hipEventDefault));
	PC_CTX_CHECK(ctx->ev1.ensure(hipEventDefault));
	ctx->img.bind(ctx->host.ec.size(), ctx->stream, ctx->ev1);
	PC_CTX_GROW(ctx->d_tables, 9*npts, "the profile tables");
	const std::vector<double> *src[9] = { &ctx->host.z, &ctx->host.cap, &ctx->host.zh, &ctx->host.cap2, &ctx->host.hexd, &ctx->host.idz, &ctx->host.ext,
	                                      &ctx->host.stp, &ctx->host.istp };
	for (int k = 0; k < 9; k++)
		PC_CTX_CHECK(hipMemcpy(ctx->d_tables + k*npts, src[k]->data(), npts*sizeof(double), hipMemcpyHostToDevice));
	PC_CTX_GROW(ctx->d_mg, npts, "the block certificates");
	PC_CTX_CHECK(hipMemcpy(ctx->d_mg, ctx->host.mg.data(), npts*sizeof(pc_marg4), hipMemcpyHostToDevice));
	PC_CTX_GROW(ctx->d_dr, npts, "the chord deviations");
	PC_CTX_CHECK(hipMemcpy(ctx->d_dr, ctx->host.dr.data(), npts*sizeof(pc_drdev), hipMemcpyHostToDevice));
	{
		/* at least 8 entries: the register-weight kernels read NE constants whatever n_energies is (surplus = copies of the last) */
		std::vector<pc_energy_const> ecp(ctx->host.ec);
		while (ecp.size() < 8) ecp.push_back(ecp.back());
		PC_CTX_GROW(ctx->d_ec, ecp.size(), "the energy constants");
		PC_CTX_CHECK(hipMemcpy(ctx->d_ec, ecp.data(), ecp.size()*sizeof(pc_energy_const), hipMemcpyHostToDevice));
	}
	{
		const size_t ne = ctx->host.ec.size();
		/* field-major constants of the weight sweeps (FORM 3): d2, Re n^2, Im n^2, max((Im n^2)^2, 2^-200), rough_c, valid, rough_c^2 */
		std::vector<double> soa(7*ne);
		for (size_t e = 0; e < ne; e++) {
			const pc_energy_const &c = ctx->host.ec[e];
			soa[e] = c.d2; soa[ne + e] = c.n2_re; soa[2*ne + e] = c.n2_im; soa[3*ne + e] = c.zi2;
			soa[4*ne + e] = c.rough_c; soa[5*ne + e] = c.valid; soa[6*ne + e] = c.rough_k2;
		}
		PC_CTX_GROW(ctx->d_ec_soa, soa.size(), "the energy constants");
		PC_CTX_CHECK(hipMemcpy(ctx->d_ec_soa, soa.data(), soa.size()*sizeof(double), hipMemcpyHostToDevice));
	}
	ctx->leak.opts.max_depth = (int)std::min(65536.0, 2.0*ctx->host.pm.n_shells + 16.0);
	ctx->totals_bytes = PC_TOTALS_BYTES(ctx->host.ec.size());
	PC_CTX_GROW(ctx->d_totals, (ctx->totals_bytes + sizeof(pc_totals) - 1)/sizeof(pc_totals), "the totals");
	PC_CTX_CHECK(hipMemset(ctx->d_totals, 0, ctx->totals_bytes));
#undef PC_CTX_CHECK
#undef PC_CTX_GROW
	*out = ctx;
	return PC_HIP_OK;
}

} /* extern "C" */

#endif /* PC_CTX_H */

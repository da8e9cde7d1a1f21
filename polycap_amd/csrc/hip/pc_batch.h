/*
 * pc_batch.h -- explicit photons: the functions of the batch store (pc_batch_store, held as pc_hip_ctx::batch), the trace over a
 * batch whose inputs are on the device (pc_batch_trace: the public launch and the relay of pc_relay.h share it) and the C calls
 * pc_hip_launch_photons, _leak and pc_hip_sample_photons.  Included by pc_kernels.hip behind the launch code and the leak run.
 */
#ifndef PC_BATCH_H
#define PC_BATCH_H

extern "C" {

/* device + pinned host buffer of at least `elems` doubles for the explicit-photon calls */
int pc_batch_store::buffers(size_t elems)
{
	const size_t want = elems < 4096 ? 4096 : elems + elems/4;
	int st = d_buf.grow(elems, "explicit-photon batch: device allocation failed", want);
	return st ? st : h_buf.grow(elems, "explicit-photon batch: host allocation failed", want);
}

/* An explicit-photon launch in three stages over one device buffer: 3 inputs [3N], rc [N ints padded], weights [N*ne], 3 outputs
 * [3N], irefl [N], dtravel [N].  upload: the caller's inputs through the pinned host buffer, which mirrors the device buffer (one
 * copy in); trace: the kernel over inputs that are on the device -- whoever put them there (pc_relay.h injects them with a
 * kernel); download: everything behind the inputs (one copy out) into the caller's arrays. */
struct pc_batch {
	size_t N = 0, ne = 0, doubles = 0;
	double *d_start = nullptr, *d_dir = nullptr, *d_ev = nullptr;
	int *d_rc = nullptr;
	double *d_w = nullptr, *d_ec = nullptr, *d_ed = nullptr, *d_ee = nullptr;
	long long *d_ir = nullptr;
	double *d_dt = nullptr;
};

/* the buffer(s) for n photons and where everything lies in them; host = false: the device buffer alone */
int pc_batch_store::layout(size_t ne, int64_t n, bool host, pc_batch &b)
{
	const size_t N = (size_t)n;
	b.N = N; b.ne = ne;
	b.doubles = 9*N + N + N*ne + 9*N + N + N;
	int st = host ? buffers(b.doubles)
	              : d_buf.grow(b.doubles, "explicit-photon batch: device allocation failed", b.doubles < 4096 ? 4096 : b.doubles + b.doubles/4);
	if (st) return st;
	double *d = d_buf;
	b.d_start = d; b.d_dir = d + 3*N; b.d_ev = d + 6*N;
	b.d_rc = (int *)(d + 9*N);
	b.d_w = d + 10*N; b.d_ec = b.d_w + N*ne; b.d_ed = b.d_ec + 3*N; b.d_ee = b.d_ed + 3*N;
	b.d_ir = (long long *)(b.d_ee + 3*N);
	b.d_dt = (double *)(b.d_ir + N);
	return PC_HIP_OK;
}

int pc_batch_store::upload(hipStream_t stream, const pc_batch &b, const double *start_coords, const double *start_dir, const double *start_elecv)
{
	const size_t N = b.N;
	double *h = h_buf;
	memcpy(h, start_coords, 3*N*sizeof(double));
	memcpy(h + 3*N, start_dir, 3*N*sizeof(double));
	memcpy(h + 6*N, start_elecv, 3*N*sizeof(double));
	PC_HIP_CHECK(hipMemcpyAsync(d_buf, h, 9*N*sizeof(double), hipMemcpyHostToDevice, stream));
	return PC_HIP_OK;
}

/* clears the totals and traces the N photons whose inputs are in the device buffer; a leak launch has been waited for when it returns */
static int pc_batch_trace(pc_hip_ctx *ctx, const pc_batch &b, int leak)
{
	const int64_t n = (int64_t)b.N;
	PC_HIP_CHECK(hipMemsetAsync(ctx->d_totals, 0, ctx->totals_bytes, ctx->stream));
	ctx->run_squares = 0;          /* explicit launches keep no sums */
	pc_kargs a;
	pc_fill_common(ctx, a);
	a.n_slots = n; a.slot0 = 0; a.max_attempts = 1; a.keep_images = 0;
	a.sumw2 = nullptr;
	a.in_start = b.d_start; a.in_dir = b.d_dir; a.in_elecv = b.d_ev;
	a.out_rc = b.d_rc; a.out_weights = b.d_w; a.out_exit_coords = b.d_ec; a.out_exit_dir = b.d_ed; a.out_exit_elecv = b.d_ee;
	a.out_irefl = b.d_ir; a.out_dtravel = b.d_dt;
	if (!leak) return pc_launch_kernel<PC_MODE_EXPLICIT>(ctx, pc_launch_site{ctx->stream}, a, n);
	/* polycap_photon_launch(..., leak_calc=true): rerun with a larger record buffer until every event fits */
	pc_leak_run &L = ctx->leak;
	L.slot0 = 0;
	L.begin(n, pc_plan_leak_capacity(L.opts.capacity, (int)b.ne, n, 4096));
	int status = L.enqueue<PC_MODE_EXPLICIT>(*ctx, a);
	if (status) return status;
	PC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	return L.run_until_fit(*ctx, &a);
}

int pc_batch_store::download(hipStream_t stream, const pc_batch &b, const double *start_elecv, int32_t *rc, double *weights, double *exit_coords,
                             double *exit_dir, double *exit_elecv, int64_t *i_refl, double *d_travel, int leak)
{
	const size_t N = b.N, ne = b.ne;
	double *d = d_buf, *h = h_buf;
	PC_HIP_CHECK(hipMemcpyAsync(h + 9*N, d + 9*N, (b.doubles - 9*N)*sizeof(double), hipMemcpyDeviceToHost, stream));
	PC_HIP_CHECK(hipStreamSynchronize(stream));
	{
		const double *o = h + 9*N;        /* rc (ints, padded to N doubles), weights, exit coords / dir / elecv, irefl, dtravel */
		memcpy(rc, o, N*sizeof(int)); o += N;
		memcpy(weights, o, N*ne*sizeof(double)); o += N*ne;
		memcpy(exit_coords, o, 3*N*sizeof(double)); o += 3*N;
		memcpy(exit_dir, o, 3*N*sizeof(double)); o += 3*N;
		memcpy(exit_elecv, o, 3*N*sizeof(double)); o += 3*N;
		memcpy(i_refl, o, N*sizeof(long long)); o += N;
		memcpy(d_travel, o, N*sizeof(double));
	}
	/* The kernels work with the normalised electric vector (polycap_refl_polar normalises it in place at the first
	 * reflection, src/polycap-capil.c:492-494); a photon that never reached a reflection keeps the caller's vector */
	for (size_t j = 0; j < N; j++) {
		const bool untouched = (rc[j] == -2) || (!leak && (rc[j] == 2 || (rc[j] == 1 && i_refl[j] == 0)));
		if (untouched)
			for (int c = 0; c < 3; c++) exit_elecv[3*j + c] = start_elecv[3*j + c];
	}
	return PC_HIP_OK;
}

static int pc_launch_photons_impl(pc_hip_ctx *ctx, int64_t n, const double *start_coords, const double *start_dir, const double *start_elecv,
                                  int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
                                  int64_t *i_refl, double *d_travel, int leak)
{
	if (!ctx || n < 0 || !start_coords || !start_dir || !start_elecv || !rc || !weights || !exit_coords || !exit_dir || !exit_elecv || !i_refl || !d_travel)
		return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_launch_photons: NULL argument");
	if (n == 0) return PC_HIP_OK;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	pc_batch b;
	int status = ctx->batch.layout((size_t)ctx->host.pm.n_energies, n, true, b);
	if (status) return status;
	ctx->last_call = PC_CALL_EXPLICIT;
	ctx->entries_epoch++;
	status = ctx->batch.upload(ctx->stream, b, start_coords, start_dir, start_elecv);
	if (!status) status = pc_batch_trace(ctx, b, leak);
	if (!status) status = ctx->batch.download(ctx->stream, b, start_elecv, rc, weights, exit_coords, exit_dir, exit_elecv, i_refl, d_travel, leak);
	ctx->img.valid = 0;
	ctx->leak.events_of_run = 0;
	return status;
}

int pc_hip_launch_photons(pc_hip_ctx *ctx, int64_t n, const double *start_coords, const double *start_dir, const double *start_elecv,
                          int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
                          int64_t *i_refl, double *d_travel)
{
	return pc_launch_photons_impl(ctx, n, start_coords, start_dir, start_elecv, rc, weights, exit_coords, exit_dir, exit_elecv, i_refl, d_travel, 0);
}

int pc_hip_launch_photons_leak(pc_hip_ctx *ctx, int64_t n, const double *start_coords, const double *start_dir, const double *start_elecv,
                               int32_t *rc, double *weights, double *exit_coords, double *exit_dir, double *exit_elecv,
                               int64_t *i_refl, double *d_travel)
{
	return pc_launch_photons_impl(ctx, n, start_coords, start_dir, start_elecv, rc, weights, exit_coords, exit_dir, exit_elecv, i_refl, d_travel, 1);
}

int pc_hip_sample_photons(pc_hip_ctx *ctx, uint64_t seed, int64_t n, const int64_t *slots, const uint32_t *attempts, double *out)
{
	if (!ctx || n < 0 || !slots || !attempts || !out) return pc_fail(PC_HIP_ERR_INVALID, "pc_hip_sample_photons: NULL argument");
	if (n == 0) return PC_HIP_OK;
	PC_HIP_CHECK(hipSetDevice(ctx->device));
	const size_t N = (size_t)n;
	/* layout in the batch buffers: slots [N int64], attempts [N uint32, padded to N/2 + 1 doubles], out [12 N] */
	const size_t off_att = N, off_out = N + N/2 + 1, total = off_out + 12*N;
	{
		int st = ctx->batch.buffers(total);
		if (st) return st;
	}
	double *d = ctx->batch.d_buf, *h = ctx->batch.h_buf;
	memcpy(h, slots, N*sizeof(long long));
	memcpy(h + off_att, attempts, N*sizeof(unsigned int));
	int status = PC_HIP_OK;
	hipError_t e = hipMemcpyAsync(d, h, off_out*sizeof(double), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(pc_sample_kernel, dim3((unsigned)((N + 255)/256)), dim3(256), 0, ctx->stream,
		                   ctx->host.pm, (unsigned long long)seed, (long long)n, (const long long *)d, (const unsigned int *)(d + off_att), d + off_out);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(h + off_out, d + off_out, 12*N*sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) status = pc_fail(PC_HIP_ERR_RUNTIME, std::string("pc_hip_sample_photons: ") + hipGetErrorString(e));
	else memcpy(out, h + off_out, 12*N*sizeof(double));
	return status;
}

} /* extern "C" */

#endif /* PC_BATCH_H */

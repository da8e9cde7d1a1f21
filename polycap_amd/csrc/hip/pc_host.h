/*
 * pc_host.h -- what every host function of the GPU path stands on: the per-thread error text (pc_fail, PC_HIP_CHECK; read by
 * pc_hip_last_error) and the four owners of GPU resources (device buffer, host buffer, stream, event).  Included by pc_kernels.hip.
 */
#ifndef PC_HOST_H
#define PC_HOST_H

static thread_local std::string g_last_error;

static int pc_fail(int code, const std::string &msg)
{
	g_last_error = msg;
	return code;
}

#define PC_HIP_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) \
	return pc_fail(PC_HIP_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

/* Owners of the GPU resources of a context: each frees what it holds when it is reset or destroyed.  None of them switches
 * devices; whoever resets or destroys one has made its device current. */

/* device buffer of `cap` elements */
template <typename T>
struct pc_dev_buf {
	T *p = nullptr;
	size_t cap = 0;
	pc_dev_buf() = default;
	pc_dev_buf(pc_dev_buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	pc_dev_buf &operator=(pc_dev_buf &&o) noexcept
	{
		if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
		return *this;
	}
	~pc_dev_buf() { reset(); }
	operator T *() const { return p; }
	T *operator->() const { return p; }
	void reset()
	{
		if (p) (void)hipFree(p);
		p = nullptr; cap = 0;
	}
	/* at least `elems` elements: unless it has them, the buffer is replaced (contents lost) by one of max(elems, alloc).  A refused
	 * allocation leaves it empty and no HIP error stored, and is PC_HIP_ERR_MEMORY with `msg`. */
	int grow(size_t elems, const char *msg, size_t alloc = 0)
	{
		if (cap >= elems) return PC_HIP_OK;
		T *old = p;
		p = nullptr; cap = 0;
		if (old) PC_HIP_CHECK(hipFree(old));
		const size_t n = std::max(elems, alloc);
		if (hipMalloc(&p, n*sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			p = nullptr;
			return pc_fail(PC_HIP_ERR_MEMORY, msg);
		}
		cap = n;
		return PC_HIP_OK;
	}
};

/* host buffer of `cap` elements in one of three shapes: pinned, or plain memory when pinning is refused (locked-memory limit);
 * pinned only; mapped into the device (coherent if the runtime grants it), with its device address `dev` */
enum pc_pin_kind { PC_PIN_OR_PLAIN, PC_PIN_ONLY, PC_PIN_MAPPED };

template <typename T, pc_pin_kind KIND>
struct pc_host_buf {
	T *p = nullptr;
	T *dev = nullptr;
	size_t cap = 0;
	bool pinned = false;
	pc_host_buf() = default;
	pc_host_buf(const pc_host_buf &) = delete;
	pc_host_buf &operator=(const pc_host_buf &) = delete;
	~pc_host_buf() { reset(); }
	operator T *() const { return p; }
	void reset()
	{
		if (p) { if (pinned) (void)hipHostFree(p); else free(p); }
		p = dev = nullptr; cap = 0; pinned = false;
	}
	/* as pc_dev_buf::grow */
	int grow(size_t elems, const char *msg, size_t alloc = 0)
	{
		if (cap >= elems) return PC_HIP_OK;
		T *old = p;
		const bool old_pinned = pinned;
		p = dev = nullptr; cap = 0; pinned = false;
		if (old && old_pinned) PC_HIP_CHECK(hipHostFree(old));
		else free(old);
		const size_t n = std::max(elems, alloc);
		void *q = nullptr;
		hipError_t e;
		if (KIND == PC_PIN_MAPPED) {
			e = hipHostMalloc(&q, n*sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
			if (e != hipSuccess) { (void)hipGetLastError(); e = hipHostMalloc(&q, n*sizeof(T), hipHostMallocMapped); }
		} else
			e = hipHostMalloc(&q, n*sizeof(T), hipHostMallocDefault);
		pinned = e == hipSuccess;
		if (!pinned) {
			(void)hipGetLastError();
			/* no pinned memory to be had: copies then go through the runtime's own staging, slower but correct */
			q = (KIND == PC_PIN_OR_PLAIN) ? malloc(n*sizeof(T)) : nullptr;
			if (!q) return pc_fail(PC_HIP_ERR_MEMORY, msg);
		}
		p = (T *)q;
		cap = n;
		if (KIND == PC_PIN_MAPPED) {
			e = hipHostGetDevicePointer((void **)&dev, p, 0);
			if (e != hipSuccess) { reset(); return pc_fail(PC_HIP_ERR_RUNTIME, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e)); }
		}
		return PC_HIP_OK;
	}
};

/* stream, created on first use: non-blocking, at the device's greatest priority when `high` and the device has priorities */
struct pc_stream_handle {
	hipStream_t s = nullptr;
	pc_stream_handle() = default;
	pc_stream_handle(const pc_stream_handle &) = delete;
	pc_stream_handle &operator=(const pc_stream_handle &) = delete;
	~pc_stream_handle() { if (s) (void)hipStreamDestroy(s); }
	operator hipStream_t() const { return s; }
	hipError_t ensure(bool high = false)
	{
		if (s) return hipSuccess;
		int least = 0, greatest = 0;
		if (high) {
			if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least
			    && hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) == hipSuccess)
				return hipSuccess;
			(void)hipGetLastError();
		}
		return hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
	}
};

/* event, created on first use */
struct pc_event_handle {
	hipEvent_t e = nullptr;
	pc_event_handle() = default;
	pc_event_handle(const pc_event_handle &) = delete;
	pc_event_handle &operator=(const pc_event_handle &) = delete;
	~pc_event_handle() { if (e) (void)hipEventDestroy(e); }
	operator hipEvent_t() const { return e; }
	hipError_t ensure(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

#endif /* PC_HOST_H */

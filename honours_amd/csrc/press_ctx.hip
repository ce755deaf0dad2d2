// press_ctx.hip - the one context of libpress_hip.so: error text, device and stream control, the libzstd loader and the
// dominant-kernel timing.  The host units that share press_host.h hold NO CPU implementation of any codec: every
// X_press / X_depress runs the HIP kernels and fails (-1 / *nout = 0) when the device is unavailable.  The only
// third-party stage is libzstd for the zstd_* compositions, which the reference itself delegates to it (press.c:1464).

#include <dlfcn.h>
#include <stdarg.h>

#include "press_host.h"

using namespace ph;

// ------------------------------------------------------------------ errors

static thread_local char g_err[256] = "";

extern "C" const char *press_hip_last_error(void) { return g_err; }

int ph::set_error(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof g_err, fmt, ap);
	va_end(ap);
	return code;
}

// ------------------------------------------------------------------ context

namespace ph {

DevBuf *g_bufs = nullptr;
Ctx g;
std::recursive_mutex g_mu;
Zstd zstd_fn;

int ctx_init()
{
	if (g.ready) {
		HIPCHK(hipSetDevice(g.device));
		return 0;
	}
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev == 0)
		return set_error(PRESS_HIP_EHIP, "no HIP device: %s", hipGetErrorString(e));
	if (g.device < 0)
		HIPCHK(hipGetDevice(&g.device));
	HIPCHK(hipSetDevice(g.device));
	HIPCHK(hipStreamCreateWithFlags(&g.own, hipStreamNonBlocking));
	g.ready = true;
	return 0;
}

bool zstd_open()
{
	if (zstd_fn.tried)
		return zstd_fn.compress != nullptr;
	zstd_fn.tried = true;
	// Bind to the libzstd the process already holds, if any: a SECOND copy of the library (another version opened by
	// absolute path) resolves its internal calls through the first one's symbols when that one is in the global
	// scope, and frees what the other allocated - glibc aborts with "free(): invalid pointer" / "munmap_chunk()"
	// (round 2: rocprofv3's tool library links the system's 1.4.8, this opened conda's 1.4.9; RTLD_LOCAL does not
	// prevent it).  So: what is loaded, then the soname, and an absolute path only last and bound to itself.
	struct { const char *name; int flags; } names[] = {
		{ "libzstd.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD },
		{ "libzstd.so.1", RTLD_NOW | RTLD_LOCAL },
		{ "libzstd.so", RTLD_NOW | RTLD_LOCAL },
		{ "/opt/conda/lib/libzstd.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND },
		{ nullptr, 0 } };
	for (int i = 0; names[i].name; i++) {
		void *h = dlopen(names[i].name, names[i].flags);
		if (!h)
			continue;
		zstd_fn.compress = (decltype(zstd_fn.compress)) dlsym(h, "ZSTD_compress");
		zstd_fn.decompress = (decltype(zstd_fn.decompress)) dlsym(h, "ZSTD_decompress");
		zstd_fn.bound = (decltype(zstd_fn.bound)) dlsym(h, "ZSTD_compressBound");
		zstd_fn.is_error = (decltype(zstd_fn.is_error)) dlsym(h, "ZSTD_isError");
		if (zstd_fn.compress && zstd_fn.decompress && zstd_fn.bound && zstd_fn.is_error)
			return true;
		zstd_fn.compress = nullptr;
	}
	return false;
}

uint64_t zstd_bound_(uint64_t n)
{
	if (zstd_open())
		return zstd_fn.bound(n);
	// zstd.h ZSTD_COMPRESSBOUND
	return n + (n >> 8) + (n < (128u << 10) ? (((128u << 10) - n) >> 11) : 0);
}

} // namespace ph

// ------------------------------------------------------------------ dominant-kernel timing

namespace {
constexpr int KT_RING = 128;
struct KTime {
	bool on = false;
	hipEvent_t ev[2][KT_RING][2];
	bool made = false;
	int n[2] = { 0, 0 };
} kt;
} // namespace

namespace ph {
static bool kt_muted = false;
void ktime_mute(bool m) { kt_muted = m; }
void ktime_begin(int which, hipStream_t s)
{
	if (kt.on && !kt_muted && kt.n[which] < KT_RING)
		(void) hipEventRecord(kt.ev[which][kt.n[which]][0], s);
}
void ktime_end(int which, hipStream_t s)
{
	if (kt.on && !kt_muted && kt.n[which] < KT_RING) {
		(void) hipEventRecord(kt.ev[which][kt.n[which]][1], s);
		kt.n[which]++;
	}
}
} // namespace ph

extern "C" int press_hip_kernel_timing(int enable)
{
	API_ENTER;
	if (enable && !kt.made) {
		for (int w = 0; w < 2; w++)
			for (int i = 0; i < KT_RING; i++)
				for (int e = 0; e < 2; e++)
					HIPCHK(hipEventCreate(&kt.ev[w][i][e]));
		kt.made = true;
	}
	kt.on = enable != 0;
	kt.n[0] = kt.n[1] = 0;
	return 0;
}

extern "C" int press_hip_kernel_times(int which, float *ms, int max)
{
	API_LOCK;
	if (which < 0 || which > 1 || !kt.made)
		return 0;
	int n = kt.n[which] < max ? kt.n[which] : max;
	for (int i = 0; i < n; i++) {
		if (hipEventSynchronize(kt.ev[which][i][1]) != hipSuccess ||
		    hipEventElapsedTime(&ms[i], kt.ev[which][i][0], kt.ev[which][i][1]) != hipSuccess)
			return i;
	}
	return n;
}

// ------------------------------------------------------------------ library control

extern "C" int press_hip_set_device(int device)
{
	API_LOCK;
	if (g.ready && device != g.device)
		press_hip_shutdown();
	g.device = device;
	return ctx_init();
}

static int use_stream(hipStream_t user, bool use_user)
{
	API_ENTER;
	g.user = user;
	g.use_user = use_user;
	return 0;
}
extern "C" int press_hip_set_stream(void *stream) { return use_stream((hipStream_t) stream, true); } // nullptr = the default (null) stream
extern "C" int press_hip_reset_stream(void) { return use_stream(nullptr, false); }

extern "C" void *press_hip_get_stream(void)
{
	API_LOCK;
	if (ctx_init())
		return nullptr;
	return (void *) g.stream();
}

extern "C" int press_hip_synchronize(void)
{
	API_ENTER;
	HIPCHK(hipStreamSynchronize(g.stream()));
	return 0;
}

extern "C" void press_hip_shutdown(void)
{
	API_LOCK;
	if (!g.ready)
		return;
	(void) hipSetDevice(g.device);
	(void) hipStreamSynchronize(g.own);
	for (DevBuf *b = g_bufs; b; b = b->next)
		b->release();
	staging_release();
	if (g.zs_pin)
		(void) hipHostFree(g.zs_pin);
	if (g.zs_ev)
		(void) hipEventDestroy(g.zs_ev);
	g.zs_pin = nullptr;
	g.zs_ev = nullptr;
	(void) hipStreamDestroy(g.own);
	g.own = nullptr;
	g.user = nullptr;
	g.use_user = false;
	g.have_table = false;
	g.ready = false;
}

extern "C" uint32_t press_hip_zstd_host_frames(void)
{
	API_LOCK;
	return g.zs_nhost;
}

extern "C" uint32_t press_hip_events_serial_reads(void)
{
	API_LOCK;
	if (!g.ready || hipSetDevice(g.device) != hipSuccess)
		return 0;
	return events_serial_reads(g.stream());
}

extern "C" uint32_t press_hip_scratch_buffers(uint64_t *bytes)
{
	API_LOCK;
	uint32_t nb = 0;
	uint64_t b = 0;
	for (DevBuf *d = g_bufs; d; d = d->next) {
		nb++;
		b += d->cap;
	}
	if (bytes)
		*bytes = b;
	return nb;
}

// Diagnostic: every scratch buffer but the static-Huffman table set to `byte`, in stream order behind the calls already
// enqueued; the page-locked staging buffers behind a synchronisation (the host writes them).  No buffer grows, shrinks
// or moves.
extern "C" int press_hip_scratch_fill(int byte)
{
	API_ENTER;
	const hipStream_t s = g.stream();
	for (DevBuf *d = g_bufs; d; d = d->next)
		if (d->p && d != &g.huff)
			HIPCHK(hipMemsetAsync(d->p, byte & 0xFF, d->cap, s));
	HIPCHK(hipStreamSynchronize(s));
	staging_fill(byte & 0xFF);
	return 0;
}

extern "C" void *press_hip_host_alloc(uint64_t bytes)
{
	API_LOCK;
	if (ctx_init())
		return nullptr;
	void *p = nullptr;
	hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
	if (e != hipSuccess) {
		set_error(PRESS_HIP_EHIP, "hipHostMalloc(%llu): %s", (unsigned long long) bytes, hipGetErrorString(e));
		return nullptr;
	}
	return p;
}

extern "C" void press_hip_host_free(void *p)
{
	API_LOCK;
	if (p)
		(void) hipHostFree(p);
}

// capi.cpp -- the library's runtime behind the C-ABI entry points of include/gmr1_hip.h: the error text, the choice of
// Viterbi decoder, the host burst tables, the per-device state with its shared workspace (dev_state, WsLease,
// dev_workspace), and gmr1_hip_version / _init / _burst_info.  The entry points themselves are in the capi_*.cpp files
// (demodulation batches: capi_demod.cpp; the reference's one-burst calls: capi_one.cpp; the fused BCCH / CCCH launch:
// capi_rx_fused.cpp; layer 1: capi_l1.cpp).  Host code only; every compute step is a HIP kernel.  There is no CPU
// fallback: without a HIP device every call returns -ENODEV.
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "capi_common.h"

namespace gmr1 {

namespace {
thread_local char t_err[256] = "";
std::mutex g_mu;
constexpr int kMaxDevices = 16;
DevState g_dev[kMaxDevices];
bool g_host_types_ready = false;
FcchTables g_fcch_tables;
}  // namespace

DevBurst g_host_types[kNumTypes];
Rx4Ord4 g_host_ord4;

int fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(t_err, sizeof(t_err), fmt, ap);
	va_end(ap);
	return code;
}

const char *last_error() { return t_err; }

int bursts_fit(int n, const uint64_t *offset, int in_len, uint64_t iq_len)
{
	for (int i = 0; i < n; i++)
		if (offset[i] + (uint64_t)in_len > iq_len)
			return fail(-EINVAL, "burst %d runs past the end of iq", i);
	return 0;
}

namespace {
std::atomic<int> g_conv_decoder{-1};       // -1: not chosen yet (the environment decides on first use)
}
int conv_acc()
{
	int v = g_conv_decoder.load(std::memory_order_relaxed);
	if (v < 0) {
		// default: what osmo_conv_decode() of every libosmocore since 0.10 (2017) runs for the K = 5 / 7, N <= 4 codes
		// (INTEGRATION.md "Which Viterbi decoder"); GMR1_HIP_CONV_DECODER=generic selects the older behaviour
		// Accepted spellings, case-insensitive: "generic" / "0", "acc" / "1"; anything else is reported once on stderr and
		// the default stands (a misspelt "Generic" must not silently select the other decoder).
		const char *e = getenv("GMR1_HIP_CONV_DECODER");
		v = GMR1_HIP_CONV_ACC;
		if (e && *e) {
			if (!strcasecmp(e, "generic") || !strcmp(e, "0"))
				v = GMR1_HIP_CONV_GENERIC;
			else if (strcasecmp(e, "acc") && strcmp(e, "1"))
				fprintf(stderr, "libgmr1_hip: GMR1_HIP_CONV_DECODER=\"%s\" is neither generic / 0 nor acc / 1: using acc\n", e);
		}
		int expect = -1;
		if (!g_conv_decoder.compare_exchange_strong(expect, v))
			v = expect;
	}
	return v == GMR1_HIP_CONV_ACC;
}

std::mutex &custom_slots_mutex()
{
	static std::mutex mu;
	return mu;
}

static int host_types_build();

int host_types()
{
	// first use may come from several threads at once (the legacy one-burst calls take no lock)
	static std::once_flag once;
	static int rv_once = 0;
	std::call_once(once, [] { rv_once = host_types_build(); });
	return rv_once;
}

static int host_types_build()
{
	tables_init();
	std::memset(g_host_types, 0, sizeof(g_host_types));
	for (int i = 0; i < GMR1_HIP_N_BURSTS; i++) {
		gmr1_hip_burst_flat f;
		int rv = flatten(kBuiltin[i], &f, kBuiltinName[i]);
		if (rv == 0)
			rv = to_dev(f, &g_host_types[i]);
		if (rv)
			return fail(rv, "built-in burst table %d is inconsistent", i);
	}
	make_ord4(g_host_types, &g_host_ord4);
	fcch_tables_init(&g_fcch_tables);
	g_host_types_ready = true;
	return 0;
}

int dev_state(DevState **out)
{
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0)
		return fail(-ENODEV, "no HIP device available (%s)", hipGetErrorString(e));
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	if (dev < 0 || dev >= kMaxDevices)
		return fail(-EINVAL, "device index %d out of range", dev);
	std::lock_guard<std::mutex> lk(g_mu);
	DevState &s = g_dev[dev];
	if (!s.ready) {
		int rv = host_types();
		if (rv)
			return rv;
		HIP_TRY(upload_types(g_host_types, 0, kNumTypes, nullptr));
		HIP_TRY(upload_rx4_operands(&g_host_ord4, nullptr));
		HIP_TRY(upload_fcch_tables(&g_fcch_tables, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		s.ready = true;
	}
	*out = &s;
	return 0;
}

int WsLease::acquire(DevState *s, hipStream_t st)
{
	s->ws_mu.lock();
	s_ = s;
	st_ = st;
	if (s->ws_depth++ == 0 && s->ws_ev) {
		const hipError_t e = hipStreamWaitEvent(st, s->ws_ev, 0);
		if (e != hipSuccess)
			return fail(-EIO, "workspace lease: hipStreamWaitEvent: %s", hipGetErrorString(e));
	}
	return 0;
}

WsLease::~WsLease()
{
	if (!s_)
		return;
	if (--s_->ws_depth == 0) {
		if (!s_->ws_ev && hipEventCreateWithFlags(&s_->ws_ev, hipEventDisableTiming) != hipSuccess)
			s_->ws_ev = nullptr;
		if (s_->ws_ev)
			(void)hipEventRecord(s_->ws_ev, st_);
	}
	s_->ws_mu.unlock();
}

int dev_workspace(DevState *s, size_t bytes, void **out)
{
	std::lock_guard<std::mutex> lk(g_mu);
	if (s->ws_bytes < bytes) {
		if (s->ws) {
			HIP_TRY(hipDeviceSynchronize());
			HIP_TRY(hipFree(s->ws));
			s->ws = nullptr;
			s->ws_bytes = 0;
		}
		const size_t want = bytes + bytes / 4;
		HIP_TRY(hipMalloc(&s->ws, want));
		s->ws_bytes = want;
	}
	*out = s->ws;
	return 0;
}

}  // namespace gmr1

using namespace gmr1;

extern "C" {

// ---------------------------------------------------------------------------
// library / device
// ---------------------------------------------------------------------------
const char *gmr1_hip_version(void)
{
	// names the Viterbi decoder in force at the time of the call (gmr1_hip_set_conv_decoder)
	return conv_acc() ? "gmr1-hip 0.4 (gfx950; conv decoder: acc)" : "gmr1-hip 0.4 (gfx950; conv decoder: generic)";
}
const char *gmr1_hip_last_error(void) { return last_error(); }

int gmr1_hip_set_conv_decoder(int decoder)
{
	if (decoder != GMR1_HIP_CONV_GENERIC && decoder != GMR1_HIP_CONV_ACC)
		return fail(-EINVAL, "gmr1_hip_set_conv_decoder: %d is neither GMR1_HIP_CONV_GENERIC nor GMR1_HIP_CONV_ACC", decoder);
	g_conv_decoder.store(decoder);
	return 0;
}

int gmr1_hip_get_conv_decoder(void) { return conv_acc() ? GMR1_HIP_CONV_ACC : GMR1_HIP_CONV_GENERIC; }

int gmr1_hip_init(int device)
{
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0)
		return fail(-ENODEV, "no HIP device available (%s)", hipGetErrorString(e));
	if (device < 0 || device >= count)
		return fail(-EINVAL, "device %d not in [0,%d)", device, count);
	HIP_TRY(hipSetDevice(device));
	DevState *s;
	return dev_state(&s);
}

int gmr1_hip_burst_info(int burst_id, struct gmr1_hip_burst_flat *out)
{
	if (burst_id < 0 || burst_id >= GMR1_HIP_N_BURSTS || !out)
		return fail(-EINVAL, "bad burst id %d", burst_id);
	return flatten(kBuiltin[burst_id], out, kBuiltinName[burst_id]);
}

}  // extern "C"

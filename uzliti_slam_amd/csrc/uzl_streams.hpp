// uzl_streams.hpp — the library's long-lived HIP streams: one process-wide pool per device (uzl_streams.hip), and the one way a
// handle with a stream of its own is made, reconfigured and destroyed.
#pragma once
#include "uzl_common.hpp"

namespace uzl {

// A stream from the device's pool that does not stand in the way of any stream of `apart_from` (a pair is measured once per process and
// remembered), of priority `priority` (0 or -1) if one can be had, else of the other one.  The stream is the caller's alone until
// stream_release.  `required`: nullptr when no such stream exists within the pool's budget (the caller falls back to a layout that does
// not need one); otherwise any stream of the pool is better than none and the pair is simply served one behind the other.
hipStream_t stream_lease(int device, int priority, const std::vector<hipStream_t>& apart_from, bool required);
void stream_release(int device, hipStream_t s);

// The stream a handle makes for itself (estimator, gate, places, radius, gist, ...).  It is entered in the pool's books so that the
// pool knows every long-lived stream of the library; `beside_solver`: long launch sequences run on it while a solve is in flight (the
// estimator's), so leases prefer streams that are independent of it too when that costs nothing.
// open sets the device, creates a non-blocking stream and registers it (throws HipError); close synchronises, unregisters and
// destroys it, and is a no-op without a stream.  Kernels and launchers take it as the plain hipStream_t it converts to.
struct HandleStream {
    hipStream_t s = nullptr;
    int device = 0;
    HandleStream() = default;
    HandleStream(const HandleStream&) = delete;
    HandleStream& operator=(const HandleStream&) = delete;
    ~HandleStream() { close(); }
    void open(int device, bool beside_solver);
    void close();
    operator hipStream_t() const { return s; }
};

struct StreamPoolStats { int32_t pooled = 0, leased = 0, registered = 0, pairs_measured = 0, pairs_independent = 0, fallbacks = 0; double probe_ms = 0.; };
StreamPoolStats stream_pool_stats(int device);

// ---- the life of a handle H { cfg (with .device); HandleStream stream; buffers and Events that release themselves }

// The stream is synchronised and closed BEFORE any buffer or event of the handle is released, whatever the order of H's members:
// nothing of the handle's is in flight when it goes.
template <typename H>
void destroy_handle(H* h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    h->stream.close();
    delete h;
}

// uzl_*_create.  The outcomes in their order: null `out`; check(cfg) != UZL_OK -> UZL_ERR_BAD_ARG (with or without a device);
// no such device; out of host memory; an init(h) that throws -> caught_status's code with nothing left allocated.  init runs with
// h->cfg set, the stream open and the device current.
template <typename H, typename Cfg, typename Check, typename Init>
int create_handle(const Cfg* cfg, void (*cfg_default)(Cfg*), H** out, Check&& check, Init&& init, bool beside_solver = false)
{
    if (!out) return UZL_ERR_BAD_ARG;
    *out = nullptr;
    Cfg c;
    if (cfg) c = *cfg; else cfg_default(&c);
    if (check(c) != UZL_OK) return UZL_ERR_BAD_ARG;
    if (check_device(c.device) != UZL_OK) return UZL_ERR_NO_DEVICE;
    H* h = new (std::nothrow) H();
    if (!h) return UZL_ERR_OOM;
    h->cfg = c;
    try {
        h->stream.open(c.device, beside_solver);
        init(h);
    } catch (...) {
        const int code = caught_status(h->last_error);
        destroy_handle(h);
        return code;
    }
    *out = h;
    return UZL_OK;
}

// uzl_*_set_config of a handle whose config is checked as at create and applies from the next call on.
template <typename H, typename Cfg, typename Check>
int set_config_of(H* h, const Cfg* cfg, Check&& check)
{
    UZL_GUARD_BEGIN(h)
    if (!cfg || check(*cfg) != UZL_OK) return fail(h, UZL_ERR_BAD_ARG, "bad config");
    if (cfg->device != h->cfg.device) return fail(h, UZL_ERR_BAD_ARG, "the device of a handle cannot change");
    h->cfg = *cfg;
    return UZL_OK;
    UZL_GUARD_END(h)
}

}  // namespace uzl

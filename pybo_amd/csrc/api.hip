// api.hip -- the C-ABI of libgpx.so (see include/gpx.h for the contract and the pybo call sites each
// entry point stands in for).  Host-side orchestration only: allocation, chunking, launch order,
// HIP-event timers.  No exception leaves this file.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <new>
#include <type_traits>

#include "gpx_internal.h"
#include "gpx_diag.h"
#include "acq_core.h"
#include "ehvi_math.h"
#include "mes_math.h"
#include "kg_math.h"

using namespace gpx;

static thread_local std::string g_create_err;

#define HIPCHK(h, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            char buf_[512];                                                                 \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                     __FILE__, __LINE__);                                                   \
            (h)->err = buf_;                                                                \
            return (e_ == hipErrorOutOfMemory) ? GPX_EOOM : GPX_EHIP;                       \
        }                                                                                   \
    } while (0)

static int fail(gpx_handle* h, int code, const char* msg) {
    h->err = msg;
    return code;
}

// Every extern "C" body runs inside this guard: nothing the C++ runtime throws (bad_alloc from the
// std::vector / std::string used for staging and messages) may cross the C boundary.
template <typename F>
static int guarded(gpx_handle* h, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        if (h) {
            try { h->err = "out of host memory"; } catch (...) {}
        }
        return GPX_EOOM;
    } catch (...) {
        if (h) {
            try { h->err = "unexpected C++ exception inside libgpx"; } catch (...) {}
        }
        return GPX_EHIP;
    }
}

int gpx::ensure_bytes(gpx_handle* h, void** p, int64_t* cap, int64_t need, size_t elem, const char* what) {
    if (need <= *cap && *p) return GPX_OK;
    if (*p && what) hipFree(*p);
    else if (*p) HIPCHK(h, hipFree(*p));
    *p = nullptr, *cap = 0;
    if (!what) HIPCHK(h, hipMalloc(p, (size_t)need * elem));
    else if (hipMalloc(p, (size_t)need * elem) != hipSuccess) return fail(h, GPX_EOOM, (std::string(what) + ": device allocation failed").c_str());
    *cap = need;
    return GPX_OK;
}

// ---- timers -----------------------------------------------------------------------------------
static hipEvent_t ev_get(gpx_handle* h) {
    if (!h->pool.empty()) {
        hipEvent_t e = h->pool.back();
        h->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}
// Recycle finished spans without blocking (callers that never read the timers must not leak events).
static void harvest_finished(gpx_handle* h) {
    size_t keep = 0;
    for (size_t i = 0; i < h->pending.size(); ++i) {
        EventPair p = h->pending[i];
        if (hipEventQuery(p.b) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) h->tacc[p.slot] += ms;
            h->pool.push_back(p.a);
            h->pool.push_back(p.b);
        } else {
            h->pending[keep++] = p;
        }
    }
    h->pending.resize(keep);
}

struct Span {
    gpx_handle* h;
    EventPair p;
    Span(gpx_handle* h_, int slot) : h(h_) {
        if (h->pending.size() >= 256) harvest_finished(h);
        p.a = ev_get(h);
        p.b = ev_get(h);
        p.slot = slot;
        hipEventRecord(p.a, h->stream);
    }
    ~Span() {
        hipEventRecord(p.b, h->stream);
        h->pending.push_back(p);
    }
};
static void harvest(gpx_handle* h) {
    hipStreamSynchronize(h->stream);
    if (h->spec_launched && h->stream3) hipStreamSynchronize(h->stream3);   // its timing events live on that stream
    for (auto& p : h->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) h->tacc[p.slot] += ms;
        h->pool.push_back(p.a);
        h->pool.push_back(p.b);
    }
    h->pending.clear();
}

// ---- options ----------------------------------------------------------------------------------
// One row per option of gpx_set_option: the name; SHIP, or DIAG for the knobs of gpx_diag.h, which a library whose
// gpx_diagnostics() is 0 refuses by name before looking at the value (a consumer of include/gpx.h cannot reach a switch
// that leaves parts of a factorisation out); the accepted range [lo, hi] and the message that refuses a value outside it;
// how an accepted value is stored; and where the range is not all accepted, the test `ok` (refused: `bad_ok`, else `bad`).
enum { SHIP = 0, DIAG = 1 };
struct Option {
    const char* name;
    int diag;
    int64_t lo, hi;
    const char* bad;
    void (*set)(gpx_handle* h, int64_t v);
    bool (*ok)(int64_t v) = nullptr;
    const char* bad_ok = nullptr;
};
template <int gpx_handle::*F>
static void store(gpx_handle* h, int64_t v) { h->*F = (int)v; }
static bool mult128(int64_t v) { return v % 128 == 0; }
static const int64_t BIG = INT64_MAX;
static const char* const TG = "chol_tg*: out of range";
static const char* const TRTRI = "trtri_ahead*: out of range";
static const char* const XBG = "x_bg*: out of range";
static const Option kOptions[] = {
    {"chunk", SHIP, 128, BIG, "chunk must be a positive multiple of 128", [](gpx_handle* h, int64_t v) { h->chunk = v; }, mult128},
    {"super_m", SHIP, 1, 16, "super_m must be 1, 2, 4, 8 or 16", store<&gpx_handle::super_m>, [](int64_t v) { return (v & (v - 1)) == 0; }},
    {"tile_order", SHIP, -1, 31, "tile_order: -1 (by size) or bits 0-1 tile map (0..3), bits 2-4 k-loop schedule (1 .. 7)",
     store<&gpx_handle::tile_order>, [](int64_t v) { return v == -1 || v >= 4; }},
    {"sweep_cache", SHIP, -1, 1, "sweep_cache must be 1, 0 or -1",                                  // -1 also drops a live cache
     [](gpx_handle* h, int64_t v) { h->cache_on = (v == 1); if (v < 0) { h->cache_valid = false; h->npend = 0; } }},
    {"prune", SHIP, -1, 1, "prune must be -1 (by size and gate), 0 (never) or 1 (wherever legal)", store<&gpx_handle::prune>},
    {"prune_keep", DIAG, 0, 1, "prune_keep must be 0 or 1", store<&gpx_handle::prune_keep>},
    {"prune_bound", DIAG, -1, 2, "prune_bound must be -1 (by guard), 0 (generic kernel), 1 (matrix-pipe kernel) or 2 (fp32 matrix-pipe kernel)", store<&gpx_handle::prune_bound>},
    {"bound_fact", DIAG, 0, 1, "bound_fact must be 0 (the fp32 bound kernel never takes its factorised form) or 1 (by its guard)", store<&gpx_handle::bound_fact>},
    {"prune_rows", DIAG, -1, 1000000, "prune_rows must be -1 (by size), 0 (no second bound) or a number of block rows", store<&gpx_handle::prune_rows>},
    {"sweep_cols", SHIP, -1, 128, "sweep_cols must be -1 (by size), 128, 64 or 32", store<&gpx_handle::sweep_cols>,
     [](int64_t v) { return v == -1 || v == 128 || v == 64 || v == 32; }},
    {"sweep_images", SHIP, -1, 2, "sweep_images must be -1 (by size), 1 or 2", store<&gpx_handle::sweep_images>, [](int64_t v) { return v != 0; }},
    {"prune_seeds", DIAG, 0, 1000000, "prune_seeds must be 0 (by the rule) or a number of seeds", store<&gpx_handle::prune_seeds>},
    {"short_map", DIAG, -1, 1, "short_map must be -1 (by size), 0 (never) or 1 (wherever tile map 3 is in use)", store<&gpx_handle::short_map>},
    {"chol_w", SHIP, 0, 8, "chol_w must be 0 (by size) or in [2, 8]", store<&gpx_handle::chol_w>, [](int64_t v) { return v != 1; }},
    {"chol_tg", SHIP, -1, 1000000000, TG, store<&gpx_handle::chol_tg>, [](int64_t v) { return v == 0 || v == 1; }, "chol_tg must be 0 or 1"},
    {"chol_tg_chunks", DIAG, -1, 1000000000, TG, store<&gpx_handle::tg_chunks>},
    {"chol_tg_grid", DIAG, -1, 1000000000, TG, store<&gpx_handle::tg_grid>},
    {"chol_tg_trace", DIAG, -1, 1000000000, TG, store<&gpx_handle::tg_trace>},
    {"chol_tg_isolate", DIAG, -1, 1000000000, TG, store<&gpx_handle::tg_isolate>},
    {"chol_tg_nap", DIAG, -1, 1000000000, TG, [](gpx_handle* h, int64_t v) { h->tg_nap = (int)std::max<int64_t>(0, std::min<int64_t>(127, v)); }},
    {"chol_tg_tmo_ms", SHIP, -1, 1000000000, TG, store<&gpx_handle::tg_tmo_ms>},
    {"chol_tg_min", SHIP, -1, 1000000000, TG, [](gpx_handle* h, int64_t v) { h->tg_min = (int)std::max<int64_t>(1, v); }},
    {"chol_tg_max", SHIP, -1, 1000000000, TG, [](gpx_handle* h, int64_t v) { h->tg_max = (int)std::max<int64_t>(1, v); }},
    {"chol_tg_db", SHIP, -1, 1000000000, TG, [](gpx_handle* h, int64_t v) { h->tg_db = (v < 0) ? -1 : (v != 0 ? 1 : 0); }},
    {"chol_tg_db_max", SHIP, -1, 1000000000, TG, [](gpx_handle* h, int64_t v) { h->tg_db_max = (int)std::max<int64_t>(0, v); }},
    {"chol_tg_fuse", SHIP, -1, 1000000000, TG, [](gpx_handle* h, int64_t v) { h->tg_fuse = (v != 0) ? 1 : 0; }},
    {"trtri_ahead", SHIP, 0, 1000000, TRTRI, [](gpx_handle* h, int64_t v) { h->trtri_ahead = (v != 0) ? 1 : 0; }},
    {"trtri_ahead_min", SHIP, 0, 1000000, TRTRI, [](gpx_handle* h, int64_t v) { h->trtri_ahead_min = (int)std::max<int64_t>(4, v); }},
    {"chol_fuse", SHIP, 0, 1, "chol_fuse must be 0 or 1", store<&gpx_handle::chol_fuse>},
    {"chol_graph", SHIP, 0, 1, "chol_graph must be 0 or 1", store<&gpx_handle::chol_graph>},
    {"chol_merge", SHIP, 0, 100000, "chol_merge: 0 (off) or a minimum number of block rows", store<&gpx_handle::chol_merge>},
    {"chol_rl", SHIP, 0, 1, "chol_rl must be 0 or 1", store<&gpx_handle::chol_rl>},
    {"x_skip", DIAG, 0, 7, "x_skip: bits 0..2", store<&gpx_handle::x_skip>},      // see launch_cholesky
    {"x_bg", DIAG, 0, 10000000, XBG, store<&gpx_handle::x_bg>},
    {"x_bg_lds", DIAG, 0, 10000000, XBG, store<&gpx_handle::x_bg_lds>},
    {"x_bg_iters", DIAG, 0, 10000000, XBG, store<&gpx_handle::x_bg_iters>},
    // A/B of the Thompson sweep kernels: process-wide, not per handle
    {"x_rff", DIAG, 0, 1, "x_rff must be 0 (by size) or 1 (the round-3 kernel)", [](gpx_handle*, int64_t v) { gpx::g_rff_variant = (int)v; }},
    {"grad_form", SHIP, 0, 2, "grad_form must be 0 (auto), 1 (two passes) or 2 (one pass)", store<&gpx_handle::grad_form>},
    {"grad_rb_cs", DIAG, 0, 65536, "grad_rb_cs must be a multiple of 128 (0 = default)", store<&gpx_handle::grad_rb_cs>, mult128},
    {"grad_kernel", SHIP, -1, 1, "grad_kernel must be -1 (auto), 0 or 1", store<&gpx_handle::grad_kernel>},
    {"trtri_left", SHIP, 0, 1, "trtri_left must be 0 or 1", store<&gpx_handle::trtri_left>},
    {"refine_inverse", SHIP, 0, 1, "refine_inverse must be 0 or 1", [](gpx_handle* h, int64_t v) { h->refine_inverse = (v != 0); }},
    {"eager_inverse", SHIP, 0, 1, "eager_inverse must be 0 or 1", [](gpx_handle* h, int64_t v) { h->eager_inverse = (v != 0); }},
};

extern "C" int gpx_set_option(gpx_handle* h, const char* name, int64_t value) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        // any option call, refused ones included, drops the carried gate decisions (prune_hint.h): whoever sets an option before a
        // sweep gets that sweep decided from scratch
        h->prune_hint = h->ens_hint = PruneHint();
        if (!name) return GPX_EARG;
        for (const Option& o : kOptions) {
            if (strcmp(name, o.name)) continue;
            if (o.diag && !gpx_diagnostics())
                return fail(h, GPX_EARG, "diagnostic option: only in a library built with -DGPX_DIAGNOSTICS (libgpx_diag.so)");
            if (value < o.lo || value > o.hi) return fail(h, GPX_EARG, o.bad);
            if (o.ok && !o.ok(value)) return fail(h, GPX_EARG, o.bad_ok ? o.bad_ok : o.bad);
            o.set(h, value);
            return GPX_OK;
        }
        return fail(h, GPX_EARG, "unknown option");
    });
}

// GPX_OPTIONS="name=value,name=value": options every new handle starts with (A/B runs THROUGH the plug-in layer, whose
// handles the caller never sees).  Empty entries are skipped; returns the first entry that is malformed or that
// gpx_set_option refuses, "" when all were applied.
static std::string apply_env_options(gpx_handle* h) {
    const char* env = getenv("GPX_OPTIONS");
    const std::string all(env ? env : "");
    for (size_t pos = 0; pos < all.size();) {
        size_t end = all.find(',', pos);
        if (end == std::string::npos) end = all.size();
        const std::string kv = all.substr(pos, end - pos);
        pos = end + 1;
        if (kv.empty()) continue;
        const size_t eq = kv.find('=');
        char* tail = nullptr;
        const long long v = (eq == std::string::npos) ? 0 : strtoll(kv.c_str() + eq + 1, &tail, 10);
        if (eq == std::string::npos || eq == 0 || !tail || *tail != 0 || tail == kv.c_str() + eq + 1 ||
            gpx_set_option(h, kv.substr(0, eq).c_str(), (int64_t)v) != GPX_OK)
            return kv;
    }
    return "";
}

// ---- lifetime ---------------------------------------------------------------------------------
// gpx_version() = round * 100.  300: gpx_predict_mean, gpx_var_at_obs, gpx_capacity, gpx_append_begin.  400: gpx_chol_trace,
// gpx_chol_tasks, GPX_OPTIONS.  500: timers slot 16.  510: timers slots 17, 18, options trtri_ahead*, chol_tg_fuse.
// 600: gpx_diagnostics, gpx_chol_tasks -> gpx_chol_tasks2 (gpx_diag.h), the diagnostic options only in the diagnostics
// build, tile_order default by size (7 below 32 block rows, 19 from there on).
// 610: option prune (selection-only sweeps), timers slot 19.  620: the ensemble sweep prunes too (the lead's option prune),
// gpx_ensemble_prune_report.  630: the second bound of selection-only sweeps (option prune_rows, gpx_prune_rows, gpx_prune_report's scalars 16 .. 19).
// 640: gpx_sweep_batch, timers slot 20.  650: gpx_ensemble_sweep_batch.
// 660: the gate's decision of a selection-only sweep is carried to the next one (prune_hint.h; any gpx_set_option drops it),
// gpx_prune_report's scalar 19 and gpx_ensemble_prune_report's scalar 10 + n say whether the sweep skipped its gate on it.
// 670: GPX_ACQ_MES = 16 (max-value entropy search: gpx_sweep*, gpx_sweep_update*, gpx_ensemble_sweep*; params = the sampled maxima).
// 680: GPX_ACQ_KG = 32 (knowledge gradient over a support set: gpx_sweep*; params = the support coordinates) and gpx_kg_grad.
// 690: gpx_constrained_sweep[_dev] (EI / PI times the probability of feasibility of up to 16 constraint models), gpx_constrained_prune_report.
// 700: gpx_ehvi_sweep[_dev], gpx_ehvi_fold_dev (expected hypervolume improvement of two objectives over a Pareto front).
// 710: gpx_sweep_batch_fantasy (batch picks with the pending outcomes integrated out over joint fantasies; time in timers slot 20).
// 720: gpx_constrained_sweep_batch (greedy batch picks of the constrained index over the members' live caches; time in timers slot 20).
// 730: gpx_ehvi_sweep_batch (greedy batch picks of the two-objective index; the front follows the picks on the device; timers slot 20).
extern "C" int gpx_version(void) { return 730; }

extern "C" const char* gpx_last_error(const gpx_handle* h) {
    return h ? h->err.c_str() : g_create_err.c_str();
}

static int create_impl(int device, void* stream, gpx_handle** out);

extern "C" int gpx_create(int device, void* stream, gpx_handle** out) {
    try {
        return create_impl(device, stream, out);
    } catch (...) {
        if (out) *out = nullptr;
        return GPX_EOOM;
    }
}

static int create_impl(int device, void* stream, gpx_handle** out) {
    if (!out) { g_create_err = "gpx_create: out is NULL"; return GPX_EARG; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("gpx_create: no HIP device (") + hipGetErrorString(e) + ")";
        return GPX_EHIP;
    }
    if (device < 0 || device >= ndev) { g_create_err = "gpx_create: bad device index"; return GPX_EARG; }
    gpx_handle* h = new (std::nothrow) gpx_handle();
    if (!h) { g_create_err = "gpx_create: out of host memory"; return GPX_EOOM; }
    h->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess) {
        g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        delete h;
        return GPX_EHIP;
    }
    if (stream) {
        h->stream = (hipStream_t)stream;
    } else {
        if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) {
            g_create_err = std::string("hipStreamCreate: ") + hipGetErrorString(e);
            delete h;
            return GPX_EHIP;
        }
        h->own_stream = true;
    }
    // (the factorisation's side streams and events are created on first use: gpx::ensure_side_streams)
    // one allocation for the small per-handle device scalars
    if (hipMalloc((void**)&h->dsmall, 64 + 16 * 8 + DMAX * 8 + 32) != hipSuccess) {
        g_create_err = "gpx_create: device allocation failed";
        delete h;
        return GPX_EOOM;
    }
    if (hipHostMalloc((void**)&h->hinv, (size_t)DMAX * 8, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_inv, hipEventDisableTiming) != hipSuccess) {
        g_create_err = "gpx_create: pinned host allocation failed";
        hipFree(h->dsmall);
        delete h;
        return GPX_EOOM;
    }
    h->dflag = reinterpret_cast<int*>(h->dsmall);
    h->dscal = reinterpret_cast<double*>(h->dsmall + 64);
    h->dinvell = h->dscal + 16;
    h->dclk = reinterpret_cast<unsigned long long*>(h->dinvell + DMAX);
    // (on the handle's own stream: the first use of the NULL stream in a process halves the speed of the stream-scheduled
    //  factorisation -- 6.8 -> 12.6 ms at N = 8192, measured in round 5 after a hipMemset here)
    (void)hipMemsetAsync(h->dclk, 0, 32, h->stream);
    (void)hipStreamSynchronize(h->stream);
    *out = h;
    // an unknown name or a bad value in GPX_OPTIONS fails the creation loudly
    const std::string bad = apply_env_options(h);
    if (!bad.empty()) {
        g_create_err = "gpx_create: GPX_OPTIONS: bad entry '" + bad + "'";
        *out = nullptr;
        gpx_destroy(h);
        return GPX_EARG;
    }
    return GPX_OK;
}

// The blocked factorisation's lookahead streams and events, created when a fit first needs them (more than one
// outer panel): a handle that only ever holds small models -- the members and proposals of the hyper-parameter
// sampler -- never pays for two HSA queues (stream creation dominated gpx_create: ~8 ms per handle).
int gpx::ensure_side_streams(gpx_handle* h) {
    if (h->stream2) return GPX_OK;
    int prio_lo = 0, prio_hi = 0;   // numerically lowest value = highest priority
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    // the side stream carries only off-critical-path work (far trailing updates): lowest priority, so the
    // serial chain on the caller's stream wins the dispatcher whenever both have workgroups pending
    bool ok_ev = true;
    for (auto& e : h->ev_row) ok_ev = ok_ev && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!ok_ev || hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithPriority(&h->stream4, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_chain, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_far, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_rest, hipEventDisableTiming) != hipSuccess)
        return fail(h, GPX_EHIP, "side stream / event creation failed");
    return GPX_OK;
}

extern "C" int gpx_destroy(gpx_handle* h) {
    if (!h) return GPX_OK;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (h->ahead_top != 0 && h->stream2) { hipStreamSynchronize(h->stream2); h->ahead_top = 0; }
    tg_free(h);
    for (auto& p : h->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (auto e : h->pool) hipEventDestroy(e);
    void* ptrs[] = {h->dXs, h->dXraw, h->dy, h->dS, h->dR, h->dT, h->dU, h->da, h->dalpha, h->dsmall, h->dKs, h->dQp, h->dXc, h->dout, h->dblkv, h->dblki,
                    h->dtopv, h->drff, h->drffs, h->dgrad, h->dens, h->dcon, h->dehvi, h->dehvib, h->dprune, h->dkeep, h->dcZ, h->dcq, h->dbatch, h->dhyper, h->dpend, h->drefine, h->dspec, h->dbsel, h->djoint, h->dkg, h->dkgw, h->dfant, h->dpath};  // dPp, dtopi, dcp alias dQp, dtopv, dcq
    for (void* p : ptrs)
        if (p) hipFree(p);
    if (h->hpin) hipHostFree(h->hpin);
    if (h->hinv) hipHostFree(h->hinv);
    if (h->chol_exec) hipGraphExecDestroy(h->chol_exec);
    if (h->ev_inv) hipEventDestroy(h->ev_inv);
    if (h->ev_spec_go) hipEventDestroy(h->ev_spec_go);
    if (h->ev_spec_done) hipEventDestroy(h->ev_spec_done);
    if (h->stream_bg) { hipStreamSynchronize(h->stream_bg); hipStreamDestroy(h->stream_bg); }
    if (h->stream2) { hipStreamSynchronize(h->stream2); hipStreamDestroy(h->stream2); }
    if (h->stream3) { hipStreamSynchronize(h->stream3); hipStreamDestroy(h->stream3); }
    if (h->stream4) { hipStreamSynchronize(h->stream4); hipStreamDestroy(h->stream4); }
    if (h->ev_rest) hipEventDestroy(h->ev_rest);
    for (auto e : h->ev_row)
        if (e) hipEventDestroy(e);
    if (h->ev_chain) hipEventDestroy(h->ev_chain);
    if (h->ev_far) hipEventDestroy(h->ev_far);
    if (h->own_stream) hipStreamDestroy(h->stream);
    delete h;
    return GPX_OK;
}


extern "C" int gpx_sync(gpx_handle* h) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return GPX_OK;
    });
}

extern "C" int64_t gpx_chol_tasks2(int nblocks, int chunks, int16_t* out, int64_t cap, int64_t* counts) {
    if (!counts) return -1;
    try {
        return gpx::tg_tasks_copy(nblocks, chunks, out, cap, counts);
    } catch (...) {
        return -1;
    }
}

extern "C" int64_t gpx_chol_trace(gpx_handle* h, int64_t* out, int64_t n) {
    if (!h || !out || n <= 0) return 0;
    if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "trace words");
    return tg_trace_copy(h, reinterpret_cast<long long*>(out), n);
}

// What gpx_prune_report, gpx_ensemble_prune_report and gpx_constrained_prune_report share, from the records' common head.
// report_begin: the argument checks and the record's state (`what` prefixes every message; `kind` + `whose` name the sweeps the record
// belongs to; `mine`: the record is the caller's; `vectors`: the caller asked for one; `also`: a refusal of the entry's own, reported
// behind the shared ones), then the device, the synchronise and the first eight scalars.  report_vectors: the bound vector with the
// survivor list.
static int report_begin(gpx_handle* h, const char* what, const char* kind, const char* whose, const gpx_handle::SelectRecord& r, bool mine,
                        const double* scal, int nscal, bool vectors, const char* also, double* out) {
    const std::string w(what);
    if (!scal || nscal < 0) return fail(h, GPX_EARG, (w + ": NULL output").c_str());
    if (r.path < 0 || !mine)
        return fail(h, GPX_ESTATE, (w + ": no " + kind + whose + " has completed its argument checks since the record was last cleared").c_str());
    if (vectors && r.path < 2) return fail(h, GPX_ESTATE, (w + ": the last " + kind + " did not reach its bound pass").c_str());
    if (also) return fail(h, GPX_ESTATE, also);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const double head[8] = {(double)r.path, (double)r.M, (double)r.k, (double)r.G, (double)r.Gg, (double)r.done, (double)r.cap, (double)r.nsurv};
    std::copy(head, head + 8, out);
    return GPX_OK;
}
static int report_vectors(gpx_handle* h, const gpx_handle::SelectRecord& r, double* ub, int64_t* idx, int64_t cap_idx) {
    if (ub) HIPCHK(h, hipMemcpy(ub, r.ub, (size_t)r.M * 8, hipMemcpyDeviceToHost));
    const int64_t nidx = std::min(std::min(r.nsurv, r.cap), cap_idx);
    if (idx && nidx > 0) HIPCHK(h, hipMemcpy(idx, r.idx, (size_t)nidx * 8, hipMemcpyDeviceToHost));
    return GPX_OK;
}

extern "C" int gpx_prune_report(gpx_handle* h, double* scal, int nscal, double* ub, int64_t* idx, int64_t cap_idx,
                                double* ub_kept, int64_t* seed_idx, int64_t cap_seed) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        const gpx_handle::PruneRecord& r = h->prune_rec;
        const bool bound = r.path >= 2;
        double out[22];
        int rc;
        if ((rc = report_begin(h, "prune_report", "sweep", "", r, true, scal, nscal, ub || idx || ub_kept || seed_idx,
                               (ub_kept || seed_idx) && !r.kept ? "prune_report: the last sweep ran without the option prune_keep" : nullptr, out)))
            return rc;
        double sc[BM_SC_WORDS];
        int st[4] = {0, 0, 0, 0};
        for (double& v : sc) v = NAN;
        if (bound) {
            HIPCHK(h, hipMemcpy(sc, r.sc, sizeof sc, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(st, r.st, sizeof st, hipMemcpyDeviceToHost));
        }
        // the device chose the bound pass's kernel: sc[8] = guard value, sc[9] = a matrix-pipe kernel ran, sc[12] = the fp32 one, sc[10] = its E
        const bool guarded_bound = bound && r.bound_kernel < 0;
        // (slot 11: the gate's mean s2 as it is, not divided by rho)
        const double tail[12] = {sc[0], sc[1], sc[5], r.gate, bound ? (double)st[2] : NAN, r.kept ? 1.0 : 0.0,
                                 bound ? (guarded_bound ? sc[9] + sc[12] : 0.0) : NAN, guarded_bound ? sc[8] : NAN,
                                 (double)r.nR, (double)r.nsurv2, guarded_bound ? sc[10] : NAN, r.hinted ? 1.0 : 0.0};
        std::copy(tail, tail + 12, out + 8);
        // the fp32 kernel's form (1.0 factorised) and the tile at which its weights change sign; NaN where it did not run
        const bool f32 = guarded_bound && sc[BM_SC_USE32] == 1.0;
        out[20] = f32 ? sc[BM_SC_FACT32] : NAN;
        out[21] = f32 ? sc[BM_SC_TPOS32] : NAN;
        for (int i = 0; i < nscal && i < 22; ++i) scal[i] = out[i];
        if ((rc = report_vectors(h, r, ub, idx, cap_idx))) return rc;
        const KeepWs kw = keep_ws(WsCarver(h->dkeep), r.M, r.G);
        if (ub_kept) HIPCHK(h, hipMemcpy(ub_kept, kw.ub, (size_t)r.M * 8, hipMemcpyDeviceToHost));
        const int64_t nseed = std::min(r.G, cap_seed);
        if (seed_idx && nseed > 0) HIPCHK(h, hipMemcpy(seed_idx, kw.seed, (size_t)nseed * 8, hipMemcpyDeviceToHost));
        return GPX_OK;
    });
}

extern "C" int gpx_prune_rows(gpx_handle* h, double* qR, double* ub2, int64_t* idx2, int64_t cap_idx2) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        const gpx_handle::PruneRecord& r = h->prune_rec;
        if (r.path != 2 || r.nR <= 0) return fail(h, GPX_ESTATE, "prune_rows: the last sweep ran no second bound");
        if (!r.kept) return fail(h, GPX_ESTATE, "prune_rows: the last sweep ran without the option prune_keep");
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (qR) HIPCHK(h, hipMemcpy(qR, r.qR, (size_t)r.nsurv * 8, hipMemcpyDeviceToHost));
        if (ub2) HIPCHK(h, hipMemcpy(ub2, r.ub2, (size_t)r.nsurv * 8, hipMemcpyDeviceToHost));
        const int64_t n2 = std::min(r.nsurv2, cap_idx2);
        if (idx2 && n2 > 0) HIPCHK(h, hipMemcpy(idx2, r.idx2, (size_t)n2 * 8, hipMemcpyDeviceToHost));
        return GPX_OK;
    });
}

extern "C" int gpx_prune_dots(gpx_handle* h, double* dots) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!dots) return fail(h, GPX_EARG, "prune_dots: NULL output");
        const gpx_handle::PruneRecord& r = h->prune_rec;
        if (r.path < 2 || !r.kept) return fail(h, GPX_ESTATE, "prune_dots: the last sweep kept no bound pass (option prune_keep)");
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(dots, keep_ws(WsCarver(h->dkeep), r.M, r.G).dots, (size_t)r.M * 8, hipMemcpyDeviceToHost));
        return GPX_OK;
    });
}

extern "C" int gpx_timers(gpx_handle* h, double* out, int n, int reset) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!out || n < 0) return fail(h, GPX_EARG, "timers: NULL output");
        harvest(h);
        unsigned long long clk[4] = {0, 0, 0, 0};
        (void)hipMemcpyAsync(clk, h->dclk, 32, hipMemcpyDeviceToHost, h->stream);
        (void)hipStreamSynchronize(h->stream);
        h->tacc[T_SCLK] = clk[1] ? 100.0 * (double)clk[0] / (double)clk[1] : 0.0;    // MHz
        h->tacc[T_RFFCLK] = clk[3] ? 100.0 * (double)clk[2] / (double)clk[3] : 0.0;
        const int m = std::min(n, (int)T_COUNT);
        for (int i = 0; i < m; ++i) out[i] = h->tacc[i];
        if (reset) {
            for (int i = 0; i < T_COUNT; ++i) h->tacc[i] = 0;
            (void)hipMemsetAsync(h->dclk, 0, 32, h->stream);
        }
        return m;
    });
}

// An announcement's correction pass may still be reading Xs / the cached candidates on the third stream: whoever is
// about to rewrite those (a refit, a new full sweep with the cache on, the next announcement) orders itself after it.
static void spec_cancel(gpx_handle* h) {
    if (h->spec_launched && h->ev_spec_done) hipStreamWaitEvent(h->stream, h->ev_spec_done, 0);
    h->spec_active = false;
    h->spec_launched = false;
    h->apply_pending = false;        // (callers either flushed first or are discarding the cache)
}

// ---- fit --------------------------------------------------------------------------------------
static int check_fit_args(gpx_handle* h, const void* X, int64_t N, int64_t d, const void* y, int kid,
                          const double* ell, double rho, double sn2) {
    if (!h) return GPX_EARG;
    if (!X || !y || !ell) return fail(h, GPX_EARG, "fit: NULL pointer");
    if (N < 1) return fail(h, GPX_EARG, "fit: N must be >= 1");
    if (d < 1 || d > DMAX) return fail(h, GPX_EARG, "fit: d must be in [1, 1024]");
    if (kid < GPX_KERN_SE_ARD || kid > GPX_KERN_MATERN12) return fail(h, GPX_EARG, "fit: unknown kernel id");
    if (!(rho > 0) || !(sn2 >= 0) || !std::isfinite(rho) || !std::isfinite(sn2))
        return fail(h, GPX_EARG, "fit: need finite rho > 0 and sn2 >= 0");
    for (int64_t k = 0; k < d; ++k)
        if (!(ell[k] > 0) || !std::isfinite(ell[k]))
            return fail(h, GPX_EARG, "fit: length-scales must be positive and finite");
    return GPX_OK;
}

static int alloc_model(gpx_handle* h, int64_t Np, int64_t d) {
    if (Np > h->cap_np || d > h->cap_d) {
        // head-room of at least one block (1/16 of the size beyond that): gpx_append can then grow the factor across
        // a 128-block boundary by re-striding inside the existing buffers, without an allocation
        Np = std::max(Np + std::max<int64_t>(NB, Np / 16 / NB * NB), h->cap_np);
        d = std::max(d, h->cap_d);
        double** mats[] = {&h->dS, &h->dR, &h->dT, &h->dU};
        for (auto m : mats) {
            if (*m) HIPCHK(h, hipFree(*m));
            *m = nullptr;
        }
        double** vecs[] = {&h->dy, &h->da, &h->dalpha, &h->dXs, &h->dXraw};
        for (auto v : vecs) {
            if (*v) HIPCHK(h, hipFree(*v));
            *v = nullptr;
        }
        h->cap_np = 0;
        h->cap_d = 0;
        for (auto m : mats) {
            HIPCHK(h, hipMalloc((void**)m, (size_t)Np * Np * 8));
            // never-written regions (e.g. the upper off-diagonal blocks of T) are never read by a
            // kernel either, but keep them defined for introspection
            HIPCHK(h, hipMemsetAsync(*m, 0, (size_t)Np * Np * 8, h->stream));
        }
        HIPCHK(h, hipMalloc((void**)&h->dy, (size_t)Np * 8));
        HIPCHK(h, hipMalloc((void**)&h->da, (size_t)Np * 8));
        HIPCHK(h, hipMalloc((void**)&h->dalpha, (size_t)Np * 8));
        HIPCHK(h, hipMalloc((void**)&h->dXs, (size_t)Np * d * 8));
        HIPCHK(h, hipMalloc((void**)&h->dXraw, (size_t)Np * d * 8));
        h->cap_np = Np;
        h->cap_d = d;
    }
    return GPX_OK;
}

// The triangular inverse T = R^-T (and U, a, alpha) is formed on FIRST USE, not by the fit: the Thompson path
// (gpx_rff_gram / gpx_rff_sweep, pybo/policies/simple.py:44-48) never reads it, and it is a quarter of a fit
// at N = 16384.  Every entry point that reads T, U, a or alpha calls this first.
// the side stream's share of an inversion that nobody asked for in the end (a new fit, a teardown): wait for it and forget it
static void settle_ahead(gpx_handle* h) {
    if (h->ahead_top == 0) return;
    (void)hipStreamSynchronize(h->stream2);
    h->ahead_top = 0;
}

int gpx::ensure_inverse(gpx_handle* h) {
    if (h->stage >= 3) return GPX_OK;
    if (h->stage < 2) return fail(h, GPX_ESTATE, "model is not fitted");
    HIPCHK(h, hipSetDevice(h->device));
    {
        Span sp(h, T_TRTRI);
        launch_trtri(h);
        if (h->refine_inverse) {
            int rc = ensure(h, h->drefine, h->cap_refine, h->cap_np * h->cap_np);
            if (rc) return rc;
            launch_refine_inverse(h, h->drefine);
        }
    }
    {
        Span sp(h, T_ALPHA);
        launch_alpha(h);
    }
    HIPCHK(h, hipGetLastError());
    h->stage = 3;
    return GPX_OK;
}

// core: dX (N,d), dy (N,) device pointers; stage 1 = stop after Gram, 2 = after Cholesky (what gpx_fit does: the
// model counts as fitted, the inverse follows lazily), 3 = Cholesky + inverse eagerly
static int fit_core(gpx_handle* h, const double* dX, int64_t N, int64_t d, const double* dy, int kid,
                    const double* ell, double rho, double sn2, double bias, int stage) {
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t Np = (N + NB - 1) / NB * NB;
    spec_cancel(h);              // an announced observation belongs to the model that is being replaced
    settle_ahead(h);             // ... and so does an inversion still running ahead on the side stream
    const bool prev_inverse_used = h->stage >= 3;
    ++h->gen;
    h->fitted = false;
    h->stage = 0;
    h->fail_pivot = -1;
    h->last_topn = 0;
    h->cache_valid = false;      // new data / hyper-parameters: the cached sums describe another posterior
    h->npend = 0;
    int rc = alloc_model(h, Np, d);
    if (rc) return rc;
    h->N = N; h->Np = Np; h->d = d; h->kernel_id = kid;
    h->rho = rho; h->sn2 = sn2; h->bias = bias;
    h->ell.assign(ell, ell + d);
    // 1/ell goes through a pinned buffer of the handle (round 2 synchronised the stream here for a stack buffer);
    // the previous fit's copy has long completed -- the event wait returns at once
    if (h->inv_inflight) { HIPCHK(h, hipEventSynchronize(h->ev_inv)); h->inv_inflight = false; }
    for (int64_t k = 0; k < d; ++k) h->hinv[k] = 1.0 / ell[k];
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->dinvell, h->hinv, (size_t)d * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipEventRecord(h->ev_inv, s));
    h->inv_inflight = true;
    HIPCHK(h, hipMemcpyAsync(h->dXraw, dX, (size_t)N * d * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemsetAsync(h->dy, 0, (size_t)Np * 8, s));
    HIPCHK(h, hipMemcpyAsync(h->dy, dy, (size_t)N * 8, hipMemcpyDeviceToDevice, s));
    {
        Span sp(h, T_GRAM);
        launch_scale_x(s, h->dXraw, N, Np, (int)d, h->dinvell, h->dXs);
        launch_gram_sym(s, h->dXs, N, Np, (int)d, kid, rho, sn2, h->dS);
    }
    h->stage = 1;
    if (stage >= 2) {
        {
            Span sp(h, T_CHOL);
            // the persistent task-graph kernel (kernels_chol_tg.hip) unless switched off, diagnosed in parts, or too small
            h->tg_launched = false;
            // the side streams of a model this size (the stream schedule's lookahead; the announced-observation pass of the
            // warm loop runs on the third one) are created HERE, in the cold fit, whichever factorisation runs: created
            // on first use by gpx_append_begin they cost the first warm iteration ~18 ms (three HSA queues)
            if (h->Np / NB > (h->chol_w ? h->chol_w : 4) && (rc = ensure_side_streams(h))) return rc;
            // the inverse's leading part may ride behind the factorisation when the inverse is certain to follow (stage 3,
            // eager_inverse) or likely to (the previous model's was formed: an acquisition loop refits and sweeps)
            h->want_ahead = (stage >= 3 || h->eager_inverse || prev_inverse_used) && !h->refine_inverse;
            const bool tg = h->chol_tg && h->x_skip == 0 && h->x_bg <= 0 && h->Np / NB >= h->tg_min && h->Np / NB <= h->tg_max && launch_cholesky_tg(h);
            if (!tg) launch_cholesky(h);
        }
        int flag2[2] = {0, 0};       // [0] failing pivot + 1, [1] the task-graph kernel's "a spin gave up" (2): one copy for both
        HIPCHK(h, hipMemcpyAsync(flag2, h->dflag, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        int flag = flag2[0];
        if (h->ahead_top != 0 && flag != 0) {      // not positive definite: what the side stream is doing is of no use
            (void)hipStreamSynchronize(h->stream2);
            h->ahead_top = 0;
        }
        if (h->tg_launched && flag == 0 && flag2[1] == 2) {
            // a spin of the persistent kernel gave up (the device is shared with something that kept its workgroups from
            // becoming resident): S is half-consumed -- rebuild it and run the stream schedule.  Loud, and counted.
            ++h->tg_fallbacks;
            h->tacc[T_TGFALL] += 1.0;
            fprintf(stderr, "libgpx: the task-graph factorisation gave up waiting (N = %lld); re-running the stream schedule\n",
                    (long long)N);
            h->tg_launched = false;
            if (h->ahead_top != 0) { (void)hipStreamSynchronize(h->stream2); h->ahead_top = 0; }
            launch_gram_sym(s, h->dXs, N, Np, (int)d, kid, rho, sn2, h->dS);
            if (h->Np / NB > (h->chol_w ? h->chol_w : 4) && (rc = ensure_side_streams(h))) return rc;
            launch_cholesky(h);
            HIPCHK(h, hipMemcpyAsync(&flag, h->dflag, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipStreamSynchronize(s));
        }
        if (flag != 0) {
            h->fail_pivot = (int64_t)flag - 1;
            char buf[160];
            snprintf(buf, sizeof buf, "fit: K + sn2*I is not positive definite (pivot %lld)",
                     (long long)h->fail_pivot);
            return fail(h, GPX_ENOTPD, buf);
        }
        h->stage = 2;
        h->fitted = true;
    }
    HIPCHK(h, hipGetLastError());
    if (stage >= 3 || h->eager_inverse) return (h->stage >= 2) ? ensure_inverse(h) : GPX_OK;
    return GPX_OK;
}

extern "C" int gpx_fit_dev(gpx_handle* h, const double* dX, int64_t N, int64_t d, const double* dy,
                           int kernel_id, const double* ell, double rho, double sn2, double bias) {
    return guarded(h, [&]() -> int {
        int rc = check_fit_args(h, dX, N, d, dy, kernel_id, ell, rho, sn2);
        if (rc) return rc;
        return fit_core(h, dX, N, d, dy, kernel_id, ell, rho, sn2, bias, 2);
    });
}

static int fit_host(gpx_handle* h, const double* X, int64_t N, int64_t d, const double* y, int kid,
                    const double* ell, double rho, double sn2, double bias, int stage) {
    int rc = check_fit_args(h, X, N, d, y, kid, ell, rho, sn2);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    rc = ensure(h, h->dXc, h->cap_xc, N * d + N);
    if (rc) return rc;
    {
        Span sp(h, T_COPY);
        HIPCHK(h, hipMemcpyAsync(h->dXc, X, (size_t)N * d * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->dXc + N * d, y, (size_t)N * 8, hipMemcpyHostToDevice, h->stream));
    }
    return fit_core(h, h->dXc, N, d, h->dXc + N * d, kid, ell, rho, sn2, bias, stage);
}

extern "C" int gpx_fit(gpx_handle* h, const double* X, int64_t N, int64_t d, const double* y, int kernel_id,
                       const double* ell, double rho, double sn2, double bias) {
    return guarded(h, [&]() -> int {
        return fit_host(h, X, N, d, y, kernel_id, ell, rho, sn2, bias, 2);
    });
}

extern "C" int gpx_fit_stage(gpx_handle* h, const double* X, int64_t N, int64_t d, const double* y,
                             int kernel_id, const double* ell, double rho, double sn2, double bias,
                             int stage) {
    return guarded(h, [&]() -> int {
        if (stage < 1 || stage > 3) return h ? fail(h, GPX_EARG, "fit_stage: stage must be 1..3") : GPX_EARG;
        return fit_host(h, X, N, d, y, kernel_id, ell, rho, sn2, bias, stage);
    });
}

extern "C" int gpx_loglik(gpx_handle* h, double* out) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return gpx::loglik_host(h, out);
    });
}

extern "C" int gpx_loglik_grad(gpx_handle* h, double* loglik, double* grad) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return gpx::loglik_grad_host(h, loglik, grad);
    });
}

// Apply the cache corrections of the observations appended since the last flush: ONE pass over the candidates
// (kernels_sweep.hip: k_sweep_rankq).
static int flush_pending(gpx_handle* h) {
    if (h->apply_pending) {
        // an announced observation was appended: its row of V over the cached candidates was computed on the third
        // stream; fold it into the sums now that somebody needs them (not earlier: the caller's stream stays free for
        // the recommender's gradient calls while the pass finishes)
        h->apply_pending = false;
        if (h->cache_valid && h->spec_M == h->cache_M) {
            const SpecBuf sb = spec_layout(h);
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_spec_done, 0));
            h->spec_launched = false;
            Span sp(h, T_RANK1);
            launch_cache_apply(h->stream, sb.v, sb.scal, h->cache_M, h->dcq, h->dcp);
        }
    }
    if (h->npend == 0) return GPX_OK;
    if (h->cache_valid) {
        Span sp(h, T_RANK1);
        const PendWs pw = pend_ws(WsCarver(h->dpend), h->pend_ld);
        launch_sweep_rankq(h->stream, h->dXs, h->N, (int)h->d, pw.rows, h->pend_ld, h->npend, pw.scal, h->dcZ, h->cache_M, h->dinvell,
                           h->kernel_id, h->rho, h->dcq, h->dcp);
        HIPCHK(h, hipGetLastError());
    }
    h->npend = 0;
    return GPX_OK;
}

extern "C" int gpx_loglik_batch(gpx_handle* h, int64_t B, const double* hypers, double* out) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return gpx::loglik_batch_host(h, B, hypers, out);
    });
}

extern "C" int gpx_append_begin(gpx_handle* h, const double* x) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!x) return fail(h, GPX_EARG, "append_begin: NULL point");
        if (!h->fitted) return fail(h, GPX_ESTATE, "append_begin: model is not fitted");
        if (!h->cache_valid) return fail(h, GPX_ESTATE, "append_begin: no live sweep cache (nothing to run ahead)");
        HIPCHK(h, hipSetDevice(h->device));
        int rc;
        if ((rc = ensure_inverse(h))) return rc;
        if ((rc = flush_pending(h))) return rc;                 // earlier appends' corrections: apply them now
        // padding of the last 128-block used up (N = 8192 exactly: the benchmark's first warm iteration): add the block now,
        // as gpx_append would have -- round 3 declined here and that iteration ran its correction pass unhidden (+4.5 ms)
        if ((rc = ensure_side_streams(h))) return rc;
        if (!h->ev_spec_go &&
            (hipEventCreateWithFlags(&h->ev_spec_go, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&h->ev_spec_done, hipEventDisableTiming) != hipSuccess))
            return fail(h, GPX_EHIP, "append_begin: event creation failed");
        spec_cancel(h);                                          // a previous announcement's pass has ended
        if (h->ev_spec_go) HIPCHK(h, hipEventSynchronize(h->ev_spec_go));   // ... and its copy of spec_x too
        // (only now: growing re-strides or re-allocates S / R / T / U and Xs on the main stream, which the previous
        //  announcement's pass on the third stream may still have been reading -- ADVICE round 4)
        if ((rc = grow_factor_if_full(h))) return rc;
        const int64_t d = h->d, M = h->cache_M, ld = h->cap_np;
        if ((rc = ensure(h, h->dspec, h->cap_spec, spec_ws(WsCarver(nullptr), (h->cap_d + 63) / 64 * 64, ld, M).bytes / 8))) return rc;
        h->spec_ld = ld;
        h->spec_M = M;
        const SpecBuf sb = spec_layout(h);
        h->spec_x.assign(x, x + d);
        hipStream_t s = h->stream, s3 = h->stream3;
        int* flag = h->dflag + 12;                               // its own word; a bad pivot surfaces at gpx_append
        HIPCHK(h, hipMemsetAsync(flag, 0, sizeof(int), s));
        HIPCHK(h, hipMemcpyAsync(sb.x, h->spec_x.data(), (size_t)d * 8, hipMemcpyHostToDevice, s));
        launch_append_prepare(h, s, sb.x, sb.ks, sb.g, sb.r, sb.tu, 0.0, sb.scal, flag);
        launch_scale_point(s, sb.x, h->dinvell, (int)d, sb.xs);
        launch_pend_store(s, sb.tu, h->N, ld, sb.scal, sb.row, sb.pscal);
        HIPCHK(h, hipEventRecord(h->ev_spec_go, s));
        HIPCHK(h, hipStreamWaitEvent(s3, h->ev_spec_go, 0));
        {
            EventPair p;                                          // T_RANK1, timed on the stream the pass runs on
            if (h->pending.size() >= 256) harvest_finished(h);
            p.a = ev_get(h);
            p.b = ev_get(h);
            p.slot = T_RANK1;
            hipEventRecord(p.a, s3);
            launch_sweep_rank1_v(s3, h->dXs, h->N + 1, (int)d, sb.row, ld, sb.pscal, h->dcZ, M, h->dinvell, h->kernel_id,
                                 h->rho, sb.xs, sb.v);
            hipEventRecord(p.b, s3);
            h->pending.push_back(p);
        }
        HIPCHK(h, hipEventRecord(h->ev_spec_done, s3));
        HIPCHK(h, hipGetLastError());
        h->spec_active = true;
        h->spec_launched = true;
        h->spec_gen = h->gen;
        return GPX_OK;
    });
}

extern "C" int gpx_append(gpx_handle* h, const double* x, double y) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        const int64_t Nold = h->N;
        int rc;
        {
            Span sp(h, T_APPEND);
            rc = gpx::append_host(h, x, y);
        }
        if (rc != GPX_OK) {
            if (rc != GPX_EARG && rc != GPX_ESTATE) { h->cache_valid = false; h->npend = 0; }
            return rc;
        }
        ++h->gen;
        if (h->cache_valid && h->spec_used && h->spec_M == h->cache_M) {
            // the point was announced: its row of V over the cached candidates is ready (or about to be) on the third
            // stream; what is left is q += v^2, p += v a_new -- O(M)
            const SpecBuf sb = spec_layout(h);
            // keep {d, 1/d, a_new, d^2} beside v (the handle's scalar scratch is rewritten by the next call); the sums
            // are updated by flush_pending when they are next read
            HIPCHK(h, hipMemcpyAsync(sb.scal, h->dscal, 4 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            h->apply_pending = true;
            return GPX_OK;
        }
        if (h->cache_valid) {
            // keep the cached per-candidate sums current: the correction for this observation (one N*M pass
            // instead of the next N^2*M sweep) is queued and applied together with up to PEND_MAX - 1 others --
            // at the next gpx_sweep_update, or here when the queue is full.  (scal / w are the device-side
            // results of the append just done.)
            if (h->npend > 0 && h->N > h->pend_ld) {             // the factor outgrew the rows: apply what is queued
                h->N = Nold;                                     // (the queued rows know nothing of the new point)
                const int rc2 = flush_pending(h);
                h->N = Nold + 1;
                if (rc2) return rc2;
            }
            if (h->npend == 0 && h->cap_np > h->pend_ld) {
                int64_t cap = 0;                                  // (the rows' pitch is the capacity the handle keeps)
                h->pend_ld = 0;
                if ((rc = ensure(h, h->dpend, cap, pend_ws(WsCarver(nullptr), h->cap_np).bytes / 8))) return rc;
                h->pend_ld = h->cap_np;
            }
            const PendWs pw = pend_ws(WsCarver(h->dpend), h->pend_ld);
            launch_pend_store(h->stream, h->app_w, Nold, h->pend_ld, h->dscal, pw.rows + (int64_t)h->npend * h->pend_ld, pw.scal + 2 * h->npend);
            HIPCHK(h, hipGetLastError());
            if (++h->npend == PEND_MAX) return flush_pending(h);
        }
        return GPX_OK;
    });
}

extern "C" int64_t gpx_fail_pivot(const gpx_handle* h) { return h ? h->fail_pivot : -1; }

extern "C" int gpx_get_matrix(gpx_handle* h, int which, double* out) {
    return guarded(h, [&]() -> int {
        if (!h || !out) return GPX_EARG;
        if (which < 0 || which > 2) return fail(h, GPX_EARG, "get_matrix: which must be 0..2");
        if ((which == 2 && h->stage != 1) || (which != 2 && h->stage < 2))
            return fail(h, GPX_ESTATE, "get_matrix: the requested matrix is not available at this stage");
        HIPCHK(h, hipSetDevice(h->device));
        if (which == 1) {
            int rc0 = ensure_inverse(h);
            if (rc0) return rc0;
        }
        const int64_t N = h->N, Np = h->Np;
        int rc = ensure(h, h->dout, h->cap_out, N * N);
        if (rc) return rc;
        if (which == 0) {
            launch_transpose_lower(h->stream, h->dR, Np, h->dout, N);  // L = R^T
            HIPCHK(h, hipMemcpyAsync(out, h->dout, (size_t)N * N * 8, hipMemcpyDeviceToHost, h->stream));
        } else {
            const double* src = (which == 1) ? h->dT : h->dS;
            HIPCHK(h, hipMemcpy2DAsync(out, (size_t)N * 8, src, (size_t)Np * 8, (size_t)N * 8, (size_t)N,
                                       hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (which == 2) {  // only the upper 128-block triangle was built: blank the rest
            for (int64_t i = 0; i < N; ++i)
                for (int64_t j = 0; j < i; ++j) out[i * N + j] = 0.0;
        }
        if (which == 1) {  // T is lower triangular; blocks above the diagonal are never written
            for (int64_t i = 0; i < N; ++i)
                for (int64_t j = i + 1; j < N; ++j) out[i * N + j] = 0.0;
        }
        return GPX_OK;
    });
}

extern "C" int gpx_get_vectors(gpx_handle* h, double* a, double* alpha) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!h->fitted) return fail(h, GPX_ESTATE, "get_vectors: model is not fitted");
        HIPCHK(h, hipSetDevice(h->device));
        {
            int rc0 = ensure_inverse(h);
            if (rc0) return rc0;
        }
        if (a) HIPCHK(h, hipMemcpyAsync(a, h->da, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
        if (alpha) HIPCHK(h, hipMemcpyAsync(alpha, h->dalpha, (size_t)h->N * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return GPX_OK;
    });
}

extern "C" int gpx_mean_at_obs(gpx_handle* h, double* mu_host, double* mu_max) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!h->fitted) return fail(h, GPX_ESTATE, "mean_at_obs: model is not fitted");
        HIPCHK(h, hipSetDevice(h->device));
        {
            int rc0 = ensure_inverse(h);
            if (rc0) return rc0;
        }
        const int64_t N = h->N;
        std::vector<double> al((size_t)N), yy((size_t)N);
        HIPCHK(h, hipMemcpyAsync(al.data(), h->dalpha, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(yy.data(), h->dy, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        // latent posterior mean at the observed inputs: K alpha + bias = y - sn2 * alpha
        double mx = -HUGE_VAL;
        for (int64_t i = 0; i < N; ++i) {
            const double m = yy[i] - h->sn2 * al[i];
            if (mu_host) mu_host[i] = m;
            if (m > mx) mx = m;
        }
        if (mu_max) *mu_max = mx;
        return GPX_OK;
    });
}

extern "C" int gpx_var_at_obs(gpx_handle* h, double* s2_host) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!s2_host) return fail(h, GPX_EARG, "var_at_obs: NULL output");
        if (!h->fitted) return fail(h, GPX_ESTATE, "var_at_obs: model is not fitted");
        HIPCHK(h, hipSetDevice(h->device));
        int rc;
        if ((rc = ensure_inverse(h))) return rc;
        const int64_t N = h->N;
        if ((rc = ensure(h, h->dout, h->cap_out, N))) return rc;
        launch_kinv_diag(h, h->dout);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(s2_host, h->dout, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        // s2_i = sn2 - sn2^2 [K^-1]_ii  (latent variance at observed input i), clipped like the sweep's
        for (int64_t i = 0; i < N; ++i) {
            const double v = h->sn2 * (1.0 - h->sn2 * s2_host[i]);
            s2_host[i] = v > gpx::S2_FLOOR ? v : gpx::S2_FLOOR;
        }
        return GPX_OK;
    });
}

extern "C" int64_t gpx_capacity(const gpx_handle* h) { return h ? h->cap_np : 0; }

// ---- sweep ------------------------------------------------------------------------------------
// top-k of a device vector (value descending, index ascending, NaN last) -> host buffers; synchronises.
static int topk_core(gpx_handle* h, const double* d_vals, int64_t M, int64_t k, double* top_val,
                     int64_t* top_idx) {
    int rc;
    hipStream_t s = h->stream;
    const int64_t nblk = topk_blocks(M);
    if ((rc = ensure(h, h->dblkv, h->cap_blk, nblk * k))) return rc;
    if ((rc = ensure(h, h->dblki, h->cap_blki, nblk * k))) return rc;
    if ((rc = ensure(h, h->dtopv, h->cap_top, (int64_t)TOPK_MAX * 2))) return rc;
    h->dtopi = reinterpret_cast<int64_t*>(h->dtopv + TOPK_MAX);
    {
        Span sp(h, T_ACQ);
        launch_topk(s, d_vals, M, (int)k, h->dblkv, h->dblki, nblk, h->dtopv, h->dtopi);
    }
    h->last_topv = h->dtopv; h->last_topi = h->dtopi; h->last_topn = k;
    HIPCHK(h, hipMemcpyAsync(top_val, h->dtopv, (size_t)k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(top_idx, h->dtopi, (size_t)k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return GPX_OK;
}

// The end of a sweep that leaves its values in d_vals on h's stream: rank them (topk_core synchronises) or synchronise, then report
// whatever a launch left behind.  (sweep_core keeps its own end: with k = 0 it returns without a synchronise.)
static int finish_sweep(gpx_handle* h, const double* d_vals, int64_t M, int64_t k, double* top_val, int64_t* top_idx) {
    if (k > 0) {
        if (int rc = topk_core(h, d_vals, M, k, top_val, top_idx)) return rc;
    } else {
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    HIPCHK(h, hipGetLastError());
    return GPX_OK;
}

// The acquisition arguments of every sweep (`what` prefixes the message): the id and its parameter, then k and the top-k
// outputs (two calls: ensemble_sweep checks its candidates between them).
// One row per acquisition: how many parameters it takes at least (vec: a vector of maximum samples, 1 .. MES_MAX_S per member,
// every entry finite).  Ids without a row -- 4 .. 15 among them -- are unknown.
struct AcqRule { int id, min_params; bool vec; };
static const AcqRule ACQ_RULES[] = {
    {GPX_ACQ_EI, 1, false}, {GPX_ACQ_PI, 1, false}, {GPX_ACQ_UCB, 1, false}, {GPX_ACQ_MEAN, 0, false}, {GPX_ACQ_MES, 1, true},
};
// GPX_ACQ_KG (params = the support set, (m, d) raw coordinates): only where the entry says it takes it (kg_ok: the cold sweep)
static int check_acq(gpx_handle* h, const char* what, int acq_id, const double* params, int nparams, int n_members = 0, bool kg_ok = false) {
    if (acq_id == GPX_ACQ_KG) {
        if (!kg_ok) return fail(h, GPX_EARG, (std::string(what) + ": KG is not supported").c_str());
        bool ok = params && h->d > 0 && nparams >= h->d && nparams % h->d == 0 && nparams / h->d <= KG_MAX_M;
        for (int i = 0; ok && i < nparams; ++i) ok = std::isfinite(params[i]);
        if (!ok) return fail(h, GPX_EARG, (std::string(what) + ": KG takes m * d finite support coordinates, m in [1, 127]").c_str());
        return GPX_OK;
    }
    const AcqRule* rule = nullptr;
    for (const AcqRule& r : ACQ_RULES)
        if (r.id == acq_id) rule = &r;
    if (!rule) return fail(h, GPX_EARG, (std::string(what) + ": unknown acquisition id").c_str());
    if (rule->vec) {
        // n_members > 0: an ensemble entry, member m scores with params[m S .. m S + S)
        if (n_members > 0 && (!params || nparams < n_members || nparams % n_members != 0 || nparams / n_members > MES_MAX_S))
            return fail(h, GPX_EARG, (std::string(what) + ": MES takes n_members * S maximum samples, S in [1, 64]").c_str());
        bool ok = params && nparams >= 1 && (n_members > 0 || nparams <= MES_MAX_S);
        for (int i = 0; ok && i < nparams; ++i) ok = std::isfinite(params[i]);
        if (!ok) return fail(h, GPX_EARG, (std::string(what) + ": MES takes 1 to 64 finite maximum samples").c_str());
        return GPX_OK;
    }
    if (rule->min_params > 0 && (nparams < rule->min_params || !params))
        return fail(h, GPX_EARG, (std::string(what) + ": missing acquisition parameter").c_str());
    return GPX_OK;
}
// the common arguments of the batch entries: the believer rounds are scored by acq_value (kernels_batch.hip), which MES is not part of
static int check_batch(gpx_handle* h, const char* what, int acq_id, const double* params, int nparams, int64_t nb, const double* sel_val,
                       const int64_t* sel_idx) {
    const std::string w(what);
    if (acq_id == GPX_ACQ_MES) return fail(h, GPX_EARG, (w + ": MES is not supported").c_str());
    if (acq_id == GPX_ACQ_KG) return fail(h, GPX_EARG, (w + ": KG is not supported").c_str());
    if (int rc = check_acq(h, what, acq_id, params, nparams)) return rc;
    if (acq_id == GPX_ACQ_MEAN)
        return fail(h, GPX_EARG, (w + ": the posterior mean does not change under hallucinated observations (EI, PI or UCB)").c_str());
    if (nb < 1 || nb > 64) return fail(h, GPX_EARG, (w + ": nb must be in [1, 64]").c_str());
    if (!sel_val || !sel_idx) return fail(h, GPX_EARG, (w + ": NULL sel_val / sel_idx output").c_str());
    return GPX_OK;
}
// the maxima of one sweep as k_acq_mes takes them (checked by check_acq)
static MesArg mes_arg(const double* params, int nparams) {
    MesArg a;
    a.S = nparams;
    for (int i = 0; i < MES_MAX_S; ++i) a.y[i] = i < nparams ? params[i] : 0.0;
    return a;
}

// The prepared support set of the knowledge gradient (kernels_kg.hip; h->dkg: kg_ws); its cross-Gram passes through dKs.
// O(N^2 m), once per support set and model: skipped while the handle holds the bits of this set for this fit (gpx_kg_grad is called
// many times by one refinement).  Enqueued on the handle's stream; the caller has ensured the inverse.
static int kg_prepare(gpx_handle* h, const double* A, int m, KgBuf& b) {
    const int64_t Np = h->Np, d = h->d;
    const int64_t need = kg_ws(WsCarver(nullptr), d, Np, m).bytes / 8;
    if (need > h->cap_kg || !h->dkg) h->kg_A.clear();
    int rc;
    if ((rc = ensure(h, h->dkg, h->cap_kg, need))) return rc;
    if ((rc = ensure(h, h->dKs, h->cap_ks, Np * NB))) return rc;
    b = kg_ws(WsCarver(h->dkg), d, Np, m);
    const size_t na = (size_t)m * d;
    if (h->kg_gen == h->gen && h->kg_Np == Np && h->kg_A.size() == na && memcmp(h->kg_A.data(), A, na * 8) == 0) return GPX_OK;
    h->kg_A.clear();
    hipStream_t s = h->stream;
    {
        Span sp(h, T_COPY);
        HIPCHK(h, hipMemcpyAsync(b.A, A, na * 8, hipMemcpyHostToDevice, s));
    }
    {
        Span sp(h, T_ACQ);
        launch_scale_x(s, b.A, m, NB, (int)d, h->dinvell, b.As);
        launch_cross_gram(s, h->dXs, Np, h->N, (int)d, b.A, 0, m, NB, h->dinvell, h->kernel_id, h->rho, h->dKs, Np);
        launch_cov_trmm(s, h->dU, Np, h->dKs, NB, b.V);
        launch_cov_mu(s, b.V, Np, NB, h->da, h->bias, b.Pp, b.al);
        launch_kg_solve(s, h->dU, Np, h->N, m, b.V, b.B);
        HIPCHK(h, hipGetLastError());
    }
    // (A is pageable host memory: the copy above has read it before it returned)
    h->kg_A.assign(A, A + na);
    h->kg_gen = h->gen;
    h->kg_Np = Np;
    return GPX_OK;
}

static int check_topk(gpx_handle* h, const char* what, int64_t k, const double* top_val, const int64_t* top_idx) {
    if (k < 0 || k > TOPK_MAX) return fail(h, GPX_EARG, (std::string(what) + ": k must be in [0, 4096]").c_str());
    if (k > 0 && (!top_val || !top_idx)) return fail(h, GPX_EARG, (std::string(what) + ": NULL top-k output").c_str());
    return GPX_OK;
}

// The host form of a sweep: stage the candidates, when given, and the outputs in h->dXc (staged_ws), run `core` on the device buffers
// (mu / s2 only where the caller wants them), copy the requested outputs back and synchronise.  `sync_upload`: the core
// reads the candidates from other streams.
template <typename Core>
static int staged_sweep(gpx_handle* h, const double* Xc, int64_t M, bool sync_upload, double* acq_all, double* mu, double* s2,
                        Core&& core) {
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t nx = Xc ? M * h->d : 0;
    int rc;
    if ((rc = ensure(h, h->dXc, h->cap_xc, staged_ws(WsCarver(nullptr), nx, M).bytes / 8))) return rc;
    const StagedWs st = staged_ws(WsCarver(h->dXc), nx, M);
    if (Xc) {
        Span sp(h, T_COPY);
        HIPCHK(h, hipMemcpyAsync(st.X, Xc, (size_t)nx * 8, hipMemcpyHostToDevice, h->stream));
    }
    if (sync_upload) HIPCHK(h, hipStreamSynchronize(h->stream));
    // (no staging vector for an output nobody asked for: a sweep that returns only its top-k may then skip candidates)
    if ((rc = core(st.X, acq_all ? st.acq : nullptr, mu ? st.mu : nullptr, s2 ? st.s2 : nullptr))) return rc;
    {
        Span sp(h, T_COPY);
        if (acq_all) HIPCHK(h, hipMemcpyAsync(acq_all, st.acq, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
        if (mu) HIPCHK(h, hipMemcpyAsync(mu, st.mu, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
        if (s2) HIPCHK(h, hipMemcpyAsync(s2, st.s2, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GPX_OK;
}

// Selection-only sweeps (option "prune" = -1): tried from this many candidates and factor rows on -- below them the N*M bound
// pass and the two extra launch chains are no small part of the sweep they save; abandoned when more than 1 / 4 of the
// candidates survive the bound (the pruned path then costs bound pass + gather + more than a quarter of the plain loop);
// gated by a mean s2 / rho of the first generation of at least 1 / 64.
static const int64_t PRUNE_MIN_M = 32768, PRUNE_MIN_NP = 1024, PRUNE_MAX_SHARE_DIV = 4;
static const double PRUNE_GATE_S2 = 1.0 / 64.0;
// The second bound (option "prune_rows" = -1): the variance bound from the leading nP / 4 block rows
// (measured on the headline workload against nP / 16 and nP / 8: profiles/prune_rows_ab.md),
// tried where the first level left more than one generation of survivors -- an exact launch on wide tiles costs a whole generation
// however few candidates it has, so at or below Gg survivors there is nothing to save (the rule was measured with wide tiles and is
// left as it is: the narrow tiles of sweep_shape_of (sweep_map.h) shorten launches of up to 1024 candidates) -- of at least PRUNE_MIN_M candidates over at least 32
// block rows: below those the prefix pass's launch chain and its sync are no small part of what it saves (the reasoning of
// PRUNE_MIN_M / PRUNE_MIN_NP).  These conditions leave the single-bound accounting untouched at every shape
// tests/test_gpu_prune_bound.py pins (prune = 1: M <= 13288 wherever nP >= 32; its larger M run at nP <= 20).
static const int PRUNE_ROWS_MIN_NP = 32, PRUNE_ROWS_DIV = 4;
// Seeds sized to the chip: where the seeds' exact launch can run on narrow tiles (sweep_map.h, sweep_shape_of:
// the default schedule, option sweep_cols not 128) over at least 48 block rows and M >= PRUNE_MIN_M, G is the column count at which
// the narrowest tile gives every compute unit one workgroup, not a wide generation.  The lower edge is 48 block rows, not the 32 from
// which the default schedule runs: tests/test_gpu_prune_rows.py pins G, the seed list, tau and the launch accounting at N = 4096,
// M = 65536 and at every smaller shape, so the gain at 32 - 47 block rows is left on the table, deliberately.
static const int PRUNE_SEEDS_MIN_NP = SWEEP_NARROW_MIN_NP;
static bool seeds_narrow(const gpx_handle* h) {
    return h->Np / NB >= PRUNE_SEEDS_MIN_NP && (h->tile_order < 0 || h->tile_order == 19) && h->sweep_cols != 128;
}

// Geometry of a selection-only sweep of M candidates for the k best over a factor of nP block rows.
// G: the candidates of one generation of sweep workgroups (512 resident, each a pair of tiles; at most 4096: short
// factors would ask for tens of thousands), at least k.
// narrow: the seeds' launch runs on narrow tiles (seeds_narrow, every member's): G0 = the candidates of 256 workgroups, one per compute
// unit, each a pair of 32-column tiles -- 256 at nP = 64 (profiles/narrow_seeds_ab.md: 0.54 ms against the wide generation's 1.96).
// Gg, cap and the form of the conditions on M do not change.  seeds > 0 (diagnostic option prune_seeds): G0 = that many.
struct PruneGeom { int64_t G, Gg, cap; };
static PruneGeom prune_geom(int nP, int64_t k, int64_t M, bool narrow = false, int64_t seeds = 0) {
    const int64_t gen_tiles = std::max<int64_t>(1, 512 / ((nP + 1) / 2));       // candidate tiles of 512 workgroups
    int64_t G0 = (int64_t)TBH * std::min<int64_t>(32, gen_tiles);
    if (narrow && M >= PRUNE_MIN_M) G0 = 32 * std::max<int64_t>(1, 256 / ((nP + 1) / 2));
    if (seeds > 0) G0 = (seeds + 31) / 32 * 32;
    const int64_t G = std::max<int64_t>(G0, (k + TBH - 1) / TBH * TBH);
    // cap: survivors beyond this: the plain loop is the better path
    // the gate's generation is a FULL one (a launch that fills half the chip takes as long as one that fills it: config B)
    return {G, (int64_t)TBH * gen_tiles, std::max<int64_t>(G, M / PRUNE_MAX_SHARE_DIV)};
}

// The pruning workspace of h (h->dprune: prune_ws_layout), grown where it has to.  The vectors of the ensemble and the constrained record h
// leads lie in it, so this is where they end: both with an allocation that has to grow (they point into the old one); a layout for a
// selection (`owner`: that sweep's record, which lives on; NULL: a member's bound pass) ends the constrained record, and a constrained
// selection's the ensemble record.
static int prune_ws(gpx_handle* h, int64_t M, int64_t cap, int64_t Gg, int64_t extra, PruneWs& w, bool rows = false,
                    const gpx_handle::SelectRecord* owner = nullptr) {
    const int64_t need = prune_ws_layout(WsCarver(nullptr), M, cap, h->d, h->Np, Gg, extra, rows).bytes;
    const bool grows = !h->dprune || need > h->cap_prune;
    if (owner != &h->ens_rec && (grows || owner == &h->con_rec)) h->ens_rec = gpx_handle::EnsPruneRecord();
    if (owner != &h->con_rec && (grows || owner)) h->con_rec = gpx_handle::ConPruneRecord();
    if (int rc = ensure(h, h->dprune, h->cap_prune, need)) return rc;
    w = prune_ws_layout(WsCarver(h->dprune), M, cap, h->d, h->Np, Gg, extra, rows);
    return GPX_OK;
}

// The bound pass's dots: out[n] = alpha2 . k(X, z_n) for the M candidates and w.sc[0 .. 1] = S, delta,
// so that EI((bias + out[n]) + delta, s2 = rho) >= the value the exact chain returns.  bound_mfma: the matrix-pipe form for SE-ARD
// up to d = 18 where its guard allows (decided on the device), in fp32 with its own margin added (out[n] = dot_hi, bound_f32.h) where
// that link's guards allow as well and the pass is long enough to matter (option prune_bound = 2: wherever the kernel exists).
// Returns bound_mfma: the host offered the matrix-pipe kernel (w.sc[9] then says which kernel wrote the dots).
static const int64_t BOUND_F32_MIN_M = 131072;
static bool bound_dots(gpx_handle* h, const double* dXc, int64_t M, const PruneWs& w, double* out) {
    const bool bound_mfma = h->prune_bound != 0 && bound_mfma_ks(h->kernel_id, (int)h->d) > 0;
    hipStream_t s = h->stream;
    launch_prune_alpha(s, h->dU, h->Np, h->da, h->rho, h->bias, w.alpha2, w.sabs, w.sc);
    if (bound_mfma)
        launch_bound_mfma(s, h->dXs, h->N, h->Np, (int)h->d, w.alpha2, h->rho, dXc, M, h->dinvell, h->prune_bound, M >= BOUND_F32_MIN_M, h->bound_fact != 0,
                          w.bws, w.sc, out);
    launch_sweep_rank1_v(s, h->dXs, h->N, (int)h->d, w.alpha2, h->Np, w.sc + 2, dXc, M, h->dinvell, h->kernel_id, h->rho,
                         nullptr, out, bound_mfma ? w.sc + 9 : nullptr);
    return bound_mfma;
}

// candidate columns of one chunk of a sweep of M candidates on h
static int64_t sweep_chunk(const gpx_handle* h, int64_t M) {
    const int64_t chunk_opt = h->chunk > 0 ? h->chunk : (h->Np <= 4096 ? 131072 : 65536);
    return std::min<int64_t>(chunk_opt, (M + TBH - 1) / TBH * TBH);
}

// What the single model's sweep (sweep_core) and the ensemble's (ensemble_core) plug into select_topk_pruned:
//   exact        the path's exact chain for rows [mb, me) of the candidate array X: out[m] (and mu / s2, where given) for every m of the range
//   gate         the first generation [0, Gg) of the sweep's own candidates, exactly, into its output; *value for the record and *go, the
//                decision.  The two gates are NOT the same arithmetic (rho on the right of the comparison / inside the sum) and stay apart
//   bound        ub[n] >= the value `exact` returns for candidate n, for every n >= done
//   after_seeds  (optional) between the seeds' compaction and their exact pass
//   refine       (optional) a second cut of the survivor list: replaces `list` by a list of positions of the first one
struct SelectList { const double* X; int64_t* idx; int64_t n; };
struct SelectOps {
    std::function<int(const double* X, int64_t mb, int64_t me, double* out, double* mu, double* s2)> exact;
    std::function<int(int64_t Gg, double* value, bool* go)> gate;
    std::function<int(double* ub, int64_t done)> bound;
    std::function<int()> after_seeds;
    std::function<int(SelectList& list)> refine;
};

// `exact` for a path whose chain takes (X, cnt, out, a, b): rows [mb, me) of the candidate array (d columns) and of every output given
template <typename Chain>
static std::function<int(const double*, int64_t, int64_t, double*, double*, double*)> exact_rows(Chain& chain, int64_t d) {
    return [&chain, d](const double* X, int64_t mb, int64_t me, double* o, double* a, double* b) -> int {
        return chain(X + mb * d, me - mb, o + mb, a ? a + mb : nullptr, b ? b + mb : nullptr);
    };
}

// `after_seeds` for a path whose other handles read the seeds from their own streams
static std::function<int()> seeds_sync(gpx_handle* L) {
    return [L]() -> int { HIPCHK(L, hipStreamSynchronize(L->stream)); return GPX_OK; };
}

// `gate` of a single model h (the sweep's own, or the objective of a constrained one): the first generation exactly into `out`, its s2
// into w.gs2; mean(s2) >= rho / 64 decides
static int single_gate(gpx_handle* h, const SelectOps& ops, const double* dXc, double* out, const PruneWs& w, int64_t Gg, double* value, bool* go) {
    if (int rc = ops.exact(dXc, 0, Gg, out, nullptr, w.gs2)) return rc;
    hipStream_t s = h->stream;
    launch_prune_mean(s, w.gs2, Gg, w.sc + 4);
    double mean_s2 = 0.0;
    HIPCHK(h, hipMemcpyAsync(&mean_s2, w.sc + 4, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    *go = mean_s2 >= h->rho * PRUNE_GATE_S2;
    *value = mean_s2;
    return GPX_OK;
}

// `bound` of a single model h: its dots -> `dots` (and, where given, a copy as the kernel left them -> keep_dots), then
// ub[n] = EI(bias + alpha . k(X, z_n) + delta, s2 = rho) >= the value the exact chain returns.  *bound_mfma (optional): bound_dots' answer.
static int single_bound(gpx_handle* h, const double* dXc, int64_t M, const PruneWs& w, double p0, double* dots, double* keep_dots, double* ub,
                        int64_t done, bool* bound_mfma = nullptr) {
    Span sp(h, T_BOUND);
    const bool mfma = bound_dots(h, dXc, M, w, dots);
    if (bound_mfma) *bound_mfma = mfma;
    if (keep_dots) HIPCHK(h, hipMemcpyAsync(keep_dots, dots, (size_t)M * 8, hipMemcpyDeviceToDevice, h->stream));
    launch_prune_ub(h->stream, dots, ub, M, done, w.sc, h->rho, h->bias, p0);
    return GPX_OK;
}

// The selection-only sweep of the n members led by L: exact values only where the EI bound
// can reach the top-k.  `legal`: the path's own conditions; the shared ones and the automatic rule are applied here.  On return candidates
// [0, *done) of `out` are final -- exact values, or -inf where the bound rules a candidate out -- and the caller runs the plain loop
// over the rest (plain_rest).  `rec` arrives as its owner started it (the fields behind the common head); the head is filled here.
// `w`: the lead's workspace, laid out here before any callback runs (prune_ws: that layout ends the lead's other records, never `rec`).
// `hint`: read, reset and re-armed by "prune" = -1 sweeps only.
static int select_topk_pruned(gpx_handle* L, bool legal, bool selection_only, int acq_id, int n, int nP, int64_t Np_min, bool narrow,
                              const double* dXc, int64_t M, int64_t k, int64_t ws_extra, bool ws_rows, PruneWs& w, PruneHint& hint,
                              gpx_handle::SelectRecord& rec, double* out, const SelectOps& ops, int64_t* done) {
    const PruneGeom geom = prune_geom(nP, k, M, narrow, L->prune_seeds);
    const int64_t G = geom.G, Gg = geom.Gg, cap = geom.cap;
    rec.path = 0, rec.M = M, rec.k = k, rec.G = G, rec.Gg = Gg, rec.cap = cap, rec.gate = NAN;
    *done = 0;                   // candidates [0, *done) are exactly evaluated already
    legal = legal && selection_only && acq_id == GPX_ACQ_EI && k > 0 && L->prune != 0 && M >= 3 * G;
    bool pruning = legal && (L->prune == 1 || (M >= PRUNE_MIN_M && Np_min >= PRUNE_MIN_NP && M >= Gg + 2 * G));
    if (!pruning) return GPX_OK;
    hipStream_t s = L->stream;
    int rc;
    const int64_t kk = std::min<int64_t>(k, TOPK_PASS);
    if ((rc = ensure(L, L->dblkv, L->cap_blk, topk_blocks(M) * kk))) return rc;
    if ((rc = ensure(L, L->dblki, L->cap_blki, topk_blocks(M) * kk))) return rc;
    if ((rc = ensure(L, L->dtopv, L->cap_top, (int64_t)TOPK_MAX * 2))) return rc;
    L->dtopi = reinterpret_cast<int64_t*>(L->dtopv + TOPK_MAX);
    if ((rc = prune_ws(L, M, cap, Gg, ws_extra, w, ws_rows, &rec))) return rc;
    PruneHint key;
    key.kernel_id = L->kernel_id, key.n = n, key.d = L->d, key.nP = nP, key.Np_min = Np_min, key.M = M, key.k = k;
    const bool automatic = L->prune < 0;       // only these sweeps read or write the carried decision
    if (automatic && prune_hint_matches(hint, key)) {
        // The last sweep of this shape pruned and it paid (prune_hint_after): no gate, on into the bound pass as prune = 1 does
        rec.hinted = true;
    } else if (automatic) {
        // Gate, BEFORE the bound pass: the prior variance is a useful bound only where the data leave variance to explain.
        // The first generation is needed by either path; its mean s2 / rho decides (config B's dense data: declined).
        // A heuristic that only chooses between two correct paths.
        if ((rc = ops.gate(Gg, &rec.gate, &pruning))) return rc;
        *done = Gg;
        rec.path = 1;
    }
    if (automatic) hint = PruneHint();         // re-earned below from this sweep's own outcome, or gone
    if (!pruning) return GPX_OK;
    double *const ub = w.ub, *const vals = w.vals, *const Xg = w.Xg;
    // 1. bound pass
    if ((rc = ops.bound(ub, *done))) return rc;
    {
        // 2. seeds: the G candidates with the largest bound (ties at the threshold: the first by index), exactly
        Span sp(L, T_ACQ);
        launch_sel_threshold(s, ub, M, (int)G, w.hist, w.st);
        launch_sel_compact(s, ub, M, 0, w.st, nullptr, w.blk, G, dXc, (int)L->d, w.idx, Xg);
    }
    if (ops.after_seeds && (rc = ops.after_seeds())) return rc;
    if ((rc = ops.exact(Xg, 0, G, vals, nullptr, nullptr))) return rc;
    int64_t nsurv = 0;
    {
        // tau = the k-th best seed value; 3. survivors: every candidate not yet evaluated whose bound is not below it
        Span sp(L, T_ACQ);
        launch_topk(s, vals, G, (int)k, L->dblkv, L->dblki, topk_blocks(G), L->dtopv, L->dtopi);
        launch_fill_neg_inf(s, out, *done, M);
        launch_sel_scatter(s, w.idx, vals, G, out, ub);
        launch_sel_compact(s, ub, M, 1, w.st, L->dtopv + (k - 1), w.blk, cap, dXc, (int)L->d, w.idx, Xg, w.sc + 5);
        HIPCHK(L, hipMemcpyAsync(&nsurv, w.blk + w.nsel, 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(L, hipStreamSynchronize(s));
    rec.path = nsurv <= cap ? 2 : 3, rec.done = *done, rec.nsurv = nsurv;
    rec.ub = ub, rec.idx = w.idx, rec.sc = w.sc;
    if (automatic) hint = key, hint.armed = prune_hint_after(rec.path, nsurv, cap);
    // 5. too many survivors -- tau = 0, a flat bound: the plain loop over everything not yet evaluated
    if (nsurv > cap) return GPX_OK;
    SelectList list = {Xg, w.idx, nsurv};
    if (ops.refine && (rc = ops.refine(list))) return rc;
    if (list.n > 0) {
        // 4. their exact values to their own positions; everything else stays -inf and the caller's top-k runs as ever
        if ((rc = ops.exact(list.X, 0, list.n, vals, nullptr, nullptr))) return rc;
        Span sp(L, T_ACQ);
        if (list.idx != w.idx) launch_sel_remap(s, w.idx, list.idx, list.n);      // (list positions -> the candidates behind them)
        launch_sel_scatter(s, list.idx, vals, list.n, out, nullptr);
    }
    *done = M;
    return GPX_OK;
}

// What the selection left: after a declined gate the rest of the lead's first chunk, so that every later launch keeps the plain loop's
// boundaries (config B: 1 + 15 full generations instead of 16, where a loop shifted by the gate's candidates would end on a 129th);
// then the plain loop over everything not yet evaluated
static int plain_rest(const SelectOps& ops, const double* dXc, int64_t done, int64_t chunk, int64_t M, double* out, double* mu, double* s2) {
    const int64_t chunk1 = std::min(chunk, M);
    int rc;
    if (done > 0 && done < chunk1) {
        if ((rc = ops.exact(dXc, done, chunk1, out, mu, s2))) return rc;
        done = chunk1;
    }
    return done < M ? ops.exact(dXc, done, M, out, mu, s2) : GPX_OK;
}

// Steps 4a-4c of a single model's selection-only sweep, where the rule says so: s2 <= rho - q_R, q_R the sum of
// V^2 over the leading nR block rows in the exact chain's own bits -- the survivors that EI((bias + dot) + delta, rho - q_R) still lets
// reach tau replace `list` (positions of the first-level list, which select_topk_pruned maps back).  nsurv <= cap of them lie in w.Xg / w.idx.
static int second_bound(gpx_handle* h, const PruneWs& w, int64_t chunk, int sweep_order, double p0, SelectList& list) {
    hipStream_t s = h->stream;
    gpx_handle::PruneRecord& rec = h->prune_rec;
    const int64_t Np = h->Np, M = rec.M, Gg = rec.Gg, cap = rec.cap, nsurv = list.n;
    const int nP = (int)(Np / NB);
    int nR = 0;
    if (h->prune_rows > 0) nR = (int)std::min<int64_t>(std::min<int64_t>(h->prune_rows, nP), h->N / NB);
    else if (h->prune_rows < 0 && M >= PRUNE_MIN_M && nP >= PRUNE_ROWS_MIN_NP && nsurv > Gg) nR = std::max(1, nP / PRUNE_ROWS_DIV);
    if (nR <= 0 || nsurv <= 0) return GPX_OK;
    int64_t nsurv2 = 0;
    {
        Span sp(h, T_BOUND);
        for (int64_t j0 = 0; j0 < nsurv; j0 += chunk) {
            const int64_t valid = std::min(chunk, nsurv - j0);
            const int64_t cols = (valid + TBH - 1) / TBH * TBH;
            // 4a. rows [0, nR 128) of the survivors' cross-Gram panels and the sweep's tiles of those block rows
            launch_cross_gram(s, h->dXs, (int64_t)nR * NB, h->N, (int)h->d, w.Xg, j0, nsurv, cols, h->dinvell, h->kernel_id, h->rho, h->dKs, Np);
            launch_sweep_trmm(s, h->dU, Np, nR, h->dKs, chunk, cols, h->da, h->dQp, h->dPp, chunk, sweep_order, h->super_m, h->dclk, h->short_map,
                              valid, h->sweep_cols, h->sweep_images);
            // 4b. ub2 = EI((bias + dot) + delta, fmax(rho - q_R, S2_FLOOR))
            launch_prune_ub2(s, h->dQp, chunk, nR, j0, valid, w.idx, w.dots, w.sc, h->rho, h->bias, p0, w.ub2, h->prune_keep ? w.qR : nullptr);
        }
    }
    {
        // 4c. the cut of step 3 on ub2 (sc[5]: the tau it cut with): positions of the first-level list, stably
        Span sp(h, T_ACQ);
        launch_sel_compact(s, w.ub2, nsurv, 1, w.st, w.sc + 5, w.blk2, cap, w.Xg, (int)h->d, w.idx2, w.Xg2);
        HIPCHK(h, hipMemcpyAsync(&nsurv2, w.blk2 + sel_blocks(nsurv), 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    rec.nR = nR, rec.nsurv2 = nsurv2;
    rec.ub2 = w.ub2, rec.idx2 = w.idx2, rec.qR = h->prune_keep ? w.qR : nullptr;
    list = {w.Xg2, w.idx2, nsurv2};
    return GPX_OK;
}

static int sweep_core(gpx_handle* h, int acq_id, const double* params, int nparams, const double* dXc,
                      int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* d_acq,
                      double* d_mu, double* d_s2) {
    h->prune_rec = gpx_handle::PruneRecord();      // every sweep entry, refused ones included, ends the previous sweep's record
    if (!h->fitted) return fail(h, GPX_ESTATE, "sweep: model is not fitted");
    if (!dXc || M < 1) return fail(h, GPX_EARG, "sweep: need M >= 1 candidates");
    int rc;
    if ((rc = check_acq(h, "sweep", acq_id, params, nparams, 0, true)) || (rc = check_topk(h, "sweep", k, top_val, top_idx))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = ensure_inverse(h))) return rc;
    hipStream_t s = h->stream;
    const int64_t Np = h->Np;
    const int nP = (int)(Np / NB);
    const int64_t chunk = sweep_chunk(h, M);
    if ((rc = ensure(h, h->dKs, h->cap_ks, Np * chunk))) return rc;
    if ((rc = ensure(h, h->dQp, h->cap_part, (int64_t)nP * chunk * 2))) return rc;
    h->dPp = h->dQp + (int64_t)nP * chunk;
    const bool selection_only = !d_acq && !d_mu && !d_s2;      // the caller reads nothing but the top-k
    if (!d_acq) {
        if ((rc = ensure(h, h->dout, h->cap_out, M))) return rc;
        d_acq = h->dout;
    }
    const bool mes = acq_id == GPX_ACQ_MES;          // its parameters are a vector: k_acq_mes, never pruned
    const MesArg ys = mes_arg(params, mes ? nparams : 0);
    const double p0 = (acq_id == GPX_ACQ_MEAN) ? 0.0 : params[0];
    // the knowledge gradient: its parameters are the support set, prepared once per sweep; k_kg_cross + k_acq_kg per chunk, never pruned
    const bool kg = acq_id == GPX_ACQ_KG;
    KgBuf kb = {};
    if (kg) {
        if ((rc = kg_prepare(h, params, nparams / (int)h->d, kb))) return rc;
        if ((rc = ensure(h, h->dkgw, h->cap_kgw, (int64_t)NB * chunk))) return rc;
    }
    double* cq = nullptr;
    double* cp = nullptr;
    if (h->cache_on) {
        spec_cancel(h);          // (the candidates it reads are about to be replaced)
        h->cache_valid = false;
        h->npend = 0;
        if ((rc = ensure(h, h->dcZ, h->cap_cz, M * h->d))) return rc;
        if ((rc = ensure(h, h->dcq, h->cap_cq, 2 * M))) return rc;
        h->dcp = h->dcq + h->cap_cq / 2;
        cq = h->dcq;
        cp = h->dcp;
        if (dXc != h->dcZ)
            HIPCHK(h, hipMemcpyAsync(h->dcZ, dXc, (size_t)M * h->d * 8, hipMemcpyDeviceToDevice, s));
    }

    // by size: short tiles (fewer than 32 block rows) on the barrier-free loop, long ones on the shared-image loop
    // (crossover measured: profiles/r06_sweep_power_probes.txt, section 6)
    const int sweep_order = h->tile_order >= 0 ? h->tile_order : (Np / NB < 32 ? 7 : 19);

    // The exact chain (cross-Gram -> V = T K* -> moments and value) for rows [mb, me) of the candidate array X, in chunks:
    // out[m] (and mu / s2 / the cache sums, where given) for every m of the range.  A candidate's value depends on its
    // coordinates alone -- not on the chunk, the tile or the column it is computed in (tests/test_gpu_prune.py).
    auto run_chunks = [&](const double* X, int64_t mb, int64_t me, double* out, double* mu, double* s2) -> int {
        for (int64_t m0 = mb; m0 < me; m0 += chunk) {
            const int64_t valid = std::min(chunk, me - m0);
            const int64_t cols = (valid + TBH - 1) / TBH * TBH;
            {
                Span sp(h, T_XGRAM);
                launch_cross_gram(s, h->dXs, Np, h->N, (int)h->d, X, m0, me, cols, h->dinvell, h->kernel_id,
                                  h->rho, h->dKs, Np);
            }
            {
                Span sp(h, T_TRMM);
                launch_sweep_trmm(s, h->dU, Np, nP, h->dKs, chunk, cols, h->da, h->dQp, h->dPp, chunk, sweep_order, h->super_m, h->dclk, h->short_map,
                                  valid, h->sweep_cols, h->sweep_images);
            }
            h->tacc[T_NLAUNCH] += 1.0;
            // ALGORITHMIC work of this launch: N^2 flop per candidate (N^2/2 multiply-adds of the
            // triangular product).  The kernel executes Np*(Np+128) per padded column (identity padding and full
            // diagonal blocks): 1.6 % more at N = 8192 -- not counted.
            h->tacc[T_FLOP] += (double)h->N * (double)h->N * (double)valid;
            {
                Span sp(h, T_ACQ);
                if (kg) {
                    launch_kg_cross(s, kb.B, Np, h->dKs, Np, cols, h->dkgw, chunk);
                    launch_acq_kg(s, h->dQp, h->dPp, chunk, nP, m0, valid, h->rho, h->bias, h->sn2, h->kernel_id, (int)h->d, X, h->dinvell,
                                  kb.As, kb.m, kb.al, h->dkgw, chunk, out, mu, s2, cq, cp);
                } else if (mes) launch_acq_mes(s, h->dQp, h->dPp, chunk, nP, m0, valid, h->rho, h->bias, ys, out, mu, s2, cq, cp);
                else launch_acq(s, h->dQp, h->dPp, chunk, nP, m0, valid, h->rho, h->bias, acq_id, p0, out, mu, s2, cq, cp);
            }
        }
        return GPX_OK;
    };

    // ---- selection-only sweep: select_topk_pruned with this model's exact chain, gate, bound and second bound ----
    gpx_handle::PruneRecord& rec = h->prune_rec;
    PruneWs w;
    KeepWs kw = {};              // (option prune_keep: laid out by the bound pass)
    SelectOps ops;
    ops.exact = run_chunks;
    ops.gate = [&](int64_t Gg, double* value, bool* go) -> int { return single_gate(h, ops, dXc, d_acq, w, Gg, value, go); };
    ops.bound = [&](double* ub, int64_t done) -> int {
        if (h->prune_keep) {
            // diagnostic: the dots as the kernel left them (gpx_prune_dots), behind the two copies below
            if ((rc = ensure(h, h->dkeep, h->cap_keep, keep_ws(WsCarver(nullptr), M, rec.G).bytes))) return rc;
            kw = keep_ws(WsCarver(h->dkeep), M, rec.G);
        }
        // (the dots stay in w.dots: the second bound reads the survivors' again)
        bool bound_mfma = false;
        if ((rc = single_bound(h, dXc, M, w, p0, w.dots, h->prune_keep ? kw.dots : nullptr, ub, done, &bound_mfma))) return rc;
        rec.bound_kernel = bound_mfma ? -1 : 0, rec.st = w.st, rec.kept = h->prune_keep != 0;
        // diagnostic: the bound vector (and after_seeds: the seed list) as they are before the scatter overwrites them
        if (rec.kept) HIPCHK(h, hipMemcpyAsync(kw.ub, ub, (size_t)M * 8, hipMemcpyDeviceToDevice, s));
        return GPX_OK;
    };
    ops.after_seeds = [&]() -> int {
        if (rec.kept) HIPCHK(h, hipMemcpyAsync(kw.seed, w.idx, (size_t)rec.G * 8, hipMemcpyDeviceToDevice, s));
        return GPX_OK;
    };
    ops.refine = [&](SelectList& list) -> int { return second_bound(h, w, chunk, sweep_order, p0, list); };
    int64_t done = 0;
    const bool legal = !h->cache_on && h->rho >= gpx::S2_FLOOR && h->rho < INFINITY;
    if ((rc = select_topk_pruned(h, legal, selection_only, acq_id, 1, nP, Np, seeds_narrow(h), dXc, M, k, 0, true, w, h->prune_hint, rec, d_acq, ops, &done)))
        return rc;
    if ((rc = plain_rest(ops, dXc, done, chunk, M, d_acq, d_mu, d_s2))) return rc;
    if (h->cache_on) {
        h->cache_valid = true;
        h->cache_M = M;
    }
    if (k > 0 && (rc = topk_core(h, d_acq, M, k, top_val, top_idx))) return rc;
    HIPCHK(h, hipGetLastError());
    return GPX_OK;
}

extern "C" int gpx_sweep_dev(gpx_handle* h, int acq_id, const double* params, int nparams, const double* dXc,
                             int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* d_acq_all,
                             double* d_mu, double* d_s2) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return sweep_core(h, acq_id, params, nparams, dXc, M, k, top_val, top_idx, d_acq_all, d_mu, d_s2);
    });
}

extern "C" int gpx_sweep(gpx_handle* h, int acq_id, const double* params, int nparams, const double* Xc,
                         int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* acq_all, double* mu,
                         double* s2) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        h->prune_rec = gpx_handle::PruneRecord();
        if (!h->fitted) return fail(h, GPX_ESTATE, "sweep: model is not fitted");
        if (!Xc || M < 1) return fail(h, GPX_EARG, "sweep: need M >= 1 candidates");
        return staged_sweep(h, Xc, M, false, acq_all, mu, s2, [&](double* dX, double* dacq, double* dmu, double* ds2) {
            return sweep_core(h, acq_id, params, nparams, dX, M, k, top_val, top_idx, dacq, dmu, ds2);
        });
    });
}

// Re-score the cached candidate set: O(M).  The sums were produced by the last full sweep with option
// "sweep_cache" = 1 and have been kept current by every gpx_append since.
static int sweep_update_core(gpx_handle* h, int acq_id, const double* params, int nparams, int64_t k,
                             double* top_val, int64_t* top_idx, double* d_acq, double* d_mu, double* d_s2) {
    h->prune_rec = gpx_handle::PruneRecord();
    if (!h->fitted) return fail(h, GPX_ESTATE, "sweep_update: model is not fitted");
    if (!h->cache_valid)
        return fail(h, GPX_ESTATE, "sweep_update: no valid sweep cache (set option sweep_cache = 1 and run a full "
                                   "sweep; a refit invalidates it)");
    int rc;
    if ((rc = check_acq(h, "sweep_update", acq_id, params, nparams)) || (rc = check_topk(h, "sweep_update", k, top_val, top_idx)))
        return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t M = h->cache_M;
    if ((rc = flush_pending(h))) return rc;
    if (!d_acq) {
        if ((rc = ensure(h, h->dout, h->cap_out, M))) return rc;
        d_acq = h->dout;
    }
    const double p0 = (acq_id == GPX_ACQ_MEAN) ? 0.0 : params[0];
    {
        Span sp(h, T_ACQ);
        if (acq_id == GPX_ACQ_MES)
            launch_acq_mes(h->stream, h->dcq, h->dcp, 0, 0, 0, M, h->rho, h->bias, mes_arg(params, nparams), d_acq, d_mu, d_s2, nullptr,
                           nullptr);
        else
            launch_acq(h->stream, h->dcq, h->dcp, 0, 0, 0, M, h->rho, h->bias, acq_id, p0, d_acq, d_mu, d_s2, nullptr, nullptr);
    }
    if (k > 0 && (rc = topk_core(h, d_acq, M, k, top_val, top_idx))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return GPX_OK;
}

extern "C" int gpx_sweep_update_dev(gpx_handle* h, int acq_id, const double* params, int nparams, int64_t k,
                                    double* top_val, int64_t* top_idx, double* d_acq_all, double* d_mu,
                                    double* d_s2) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return sweep_update_core(h, acq_id, params, nparams, k, top_val, top_idx, d_acq_all, d_mu, d_s2);
    });
}

extern "C" int gpx_sweep_update(gpx_handle* h, int acq_id, const double* params, int nparams, int64_t k,
                                double* top_val, int64_t* top_idx, double* acq_all, double* mu, double* s2) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        h->prune_rec = gpx_handle::PruneRecord();
        if (!h->cache_valid) return fail(h, GPX_ESTATE, "sweep_update: no valid sweep cache");
        return staged_sweep(h, nullptr, h->cache_M, false, acq_all, mu, s2, [&](double*, double* dacq, double* dmu, double* ds2) {
            return sweep_update_core(h, acq_id, params, nparams, k, top_val, top_idx, dacq, dmu, ds2);
        });
    });
}

extern "C" int64_t gpx_sweep_cache_size(const gpx_handle* h) { return (h && h->cache_valid) ? h->cache_M : 0; }

extern "C" int gpx_predict(gpx_handle* h, const double* Xc, int64_t M, double* mu, double* s2, double* dmu,
                           double* ds2) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!mu || !s2) return fail(h, GPX_EARG, "predict: mu and s2 outputs are required");
        if (dmu || ds2) {
            if (!dmu || !ds2) return fail(h, GPX_EARG, "predict: pass both gradient outputs or neither");
            return gpx::predict_grad_host(h, Xc, M, mu, s2, dmu, ds2);
        }
        return gpx_sweep(h, GPX_ACQ_MEAN, nullptr, 0, Xc, M, 0, nullptr, nullptr, nullptr, mu, s2);
    });
}

extern "C" int gpx_predict_mean(gpx_handle* h, const double* Xc, int64_t M, double* mu, double* dmu) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return gpx::predict_mean_host(h, Xc, M, mu, dmu);
    });
}

// ---- joint posterior at a point set (kernels_cov.hip): full covariance, exact draws -------------------------------------
// The chain of both entry points: Ks = k(X, Z) by the sweep's own cross-Gram kernel (into dKs), V = T Ks STORED panel-major,
// mu = bias + V^T a, Kss = k(Z, Z) by the cross-Gram kernel on the scaled points, C = Kss - V^T V; for draws B = C + c I,
// B = R^T R by launch_cholesky_small under a flag word of its own (dflag[10]), out = mu + z R.  One stream, one synchronisation.
// Reads the fit only: no flush of queued corrections, the sweep cache, an announcement and their buffers are not touched.
// Scratch: h->djoint (joint_ws).
static const int64_t JOINT_MAX_M = 4096;

static int joint_core(gpx_handle* h, const char* what, const double* Xc, int64_t M, const double* z, int64_t S, int noisy,
                      double jitter, double* mu, double* cov, double* out) {
    char msg[256];
    const bool draw = out != nullptr;
    if (!h->fitted) {
        snprintf(msg, sizeof msg, "%s: model is not fitted", what);
        return fail(h, GPX_ESTATE, msg);
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure_inverse(h))) return rc;
    hipStream_t s = h->stream;
    const int64_t Np = h->Np, d = h->d, Mp = (M + TBH - 1) / TBH * TBH;
    const int nP = (int)(Np / NB);
    if ((rc = ensure(h, h->dKs, h->cap_ks, Np * Mp))) return rc;
    if ((rc = ensure(h, h->djoint, h->cap_joint, joint_ws(WsCarver(nullptr), M, Mp, d, nP, Np, draw, S).bytes / 8))) return rc;
    const JointWs j = joint_ws(WsCarver(h->djoint), M, Mp, d, nP, Np, draw, S);
    int* flag = h->dflag + 10;                // its own word: the fit's flag, the RFF posterior's and an announcement's stay untouched
    {
        Span sp(h, T_COPY);
        HIPCHK(h, hipMemcpyAsync(j.X, Xc, (size_t)M * d * 8, hipMemcpyHostToDevice, s));
        if (draw) HIPCHK(h, hipMemcpyAsync(j.z, z, (size_t)S * M * 8, hipMemcpyHostToDevice, s));
    }
    {
        Span sp(h, T_JOINT);
        launch_cross_gram(s, h->dXs, Np, h->N, (int)d, j.X, 0, M, Mp, h->dinvell, h->kernel_id, h->rho, h->dKs, Np);
        launch_cov_trmm(s, h->dU, Np, h->dKs, Mp, j.V);
        launch_cov_mu(s, j.V, Np, Mp, h->da, h->bias, j.Pp, j.mu);
        launch_scale_x(s, j.X, M, Mp, (int)d, h->dinvell, j.Zs);
        launch_cross_gram(s, j.Zs, Mp, M, (int)d, j.X, 0, M, Mp, h->dinvell, h->kernel_id, h->rho, j.Kss, Mp);
        launch_cov_syrk(s, j.V, Np, j.Kss, Mp, j.C);
        if (draw) {
            launch_cov_form(s, j.C, M, Mp, (noisy ? h->sn2 : 0.0) + jitter, j.B);
            launch_cholesky_small(s, j.B, j.R, Mp, flag);
            launch_cov_draw(s, j.R, Mp, M, j.z, S, j.mu, flag, j.out);
        }
        HIPCHK(h, hipGetLastError());
    }
    int fl = 0;
    {
        Span sp(h, T_COPY);
        if (mu) HIPCHK(h, hipMemcpyAsync(mu, j.mu, (size_t)M * 8, hipMemcpyDeviceToHost, s));
        if (cov) HIPCHK(h, hipMemcpy2DAsync(cov, (size_t)M * 8, j.C, (size_t)Mp * 8, (size_t)M * 8, (size_t)M, hipMemcpyDeviceToHost, s));
        if (draw) {
            HIPCHK(h, hipMemcpyAsync(out, j.out, (size_t)S * M * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(&fl, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        }
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (fl != 0) {
        snprintf(msg, sizeof msg, "%s: cov + (%s + jitter) I is not positive definite: pivot %d of %lld failed (out is undefined)", what,
                 noisy ? "sn2" : "0", fl - 1, (long long)M);
        return fail(h, GPX_ENOTPD, msg);
    }
    return GPX_OK;
}

extern "C" int gpx_predict_cov(gpx_handle* h, const double* Xc, int64_t M, double* mu, double* cov) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!Xc || !cov) return fail(h, GPX_EARG, "predict_cov: NULL Xc / cov");
        if (M < 1 || M > JOINT_MAX_M) return fail(h, GPX_EARG, "predict_cov: M must be in [1, 4096]");
        return joint_core(h, "predict_cov", Xc, M, nullptr, 0, 0, 0.0, mu, cov, nullptr);
    });
}

extern "C" int gpx_sample_joint(gpx_handle* h, const double* Xc, int64_t M, const double* z, int64_t S, int noisy, double jitter,
                                double* out) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!Xc || !z || !out) return fail(h, GPX_EARG, "sample_joint: NULL Xc / z / out");
        if (M < 1 || M > JOINT_MAX_M) return fail(h, GPX_EARG, "sample_joint: M must be in [1, 4096]");
        if (S < 1) return fail(h, GPX_EARG, "sample_joint: S must be >= 1");
        if (!(jitter >= 0.0) || !std::isfinite(jitter)) return fail(h, GPX_EARG, "sample_joint: jitter must be finite and >= 0");
        return joint_core(h, "sample_joint", Xc, M, z, S, noisy, jitter, nullptr, nullptr, out);
    });
}

// ---- knowledge gradient at a few points: value and gradient (kernels_kg.hip) ---------------------------------------------
// The L-BFGS refinement's `f(x, grad=True)` for policies.KG.  Per panel of 128 points: Ks_z by the cross-Gram kernel (through dKs),
// V_z = T Ks_z, W_z = U V_z, the sums over the observed rows, then lines, value and gradient.  One stream, one synchronisation; reads
// the fit only (the prepared support set is kept in h->dkg for the next call).  Work space: h->dkgw (kg_point_ws).
extern "C" int gpx_kg_grad(gpx_handle* h, const double* A, int64_t m, const double* Xc, int64_t M, double* f, double* g) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!h->fitted) return fail(h, GPX_ESTATE, "kg_grad: model is not fitted");
        if (!A || !Xc || !f || !g) return fail(h, GPX_EARG, "kg_grad: NULL A / Xc / f / g");
        const int64_t d = h->d;
        bool ok = m >= 1 && m <= KG_MAX_M;
        for (int64_t i = 0; ok && i < m * d; ++i) ok = std::isfinite(A[i]);
        if (!ok) return fail(h, GPX_EARG, "kg_grad: KG takes m * d finite support coordinates, m in [1, 127]");
        if (M < 1 || M > JOINT_MAX_M) return fail(h, GPX_EARG, "kg_grad: M must be in [1, 4096]");
        HIPCHK(h, hipSetDevice(h->device));
        int rc;
        if ((rc = ensure_inverse(h))) return rc;
        KgBuf kb;
        if ((rc = kg_prepare(h, A, (int)m, kb))) return rc;
        hipStream_t s = h->stream;
        const int64_t Np = h->Np, Mp = (M + TBH - 1) / TBH * TBH;
        if ((rc = ensure(h, h->dkgw, h->cap_kgw, kg_point_ws(WsCarver(nullptr), Mp, d, Np).bytes / 8))) return rc;
        const KgPointWs pw = kg_point_ws(WsCarver(h->dkgw), Mp, d, Np);
        {
            Span sp(h, T_COPY);
            HIPCHK(h, hipMemcpyAsync(pw.Z, Xc, (size_t)M * d * 8, hipMemcpyHostToDevice, s));
        }
        {
            Span sp(h, T_ACQ);
            for (int64_t p0 = 0; p0 < M; p0 += NB) {
                const int np = (int)std::min<int64_t>(NB, M - p0);
                launch_cross_gram(s, h->dXs, Np, h->N, (int)d, pw.Z, p0, M, NB, h->dinvell, h->kernel_id, h->rho, h->dKs, Np);
                launch_cov_trmm(s, h->dU, Np, h->dKs, NB, pw.Vz);
                launch_kg_solve(s, h->dU, Np, h->N, np, pw.Vz, pw.Wz);
                launch_kg_point_sums(s, h->dXs, h->N, (int)d, pw.Z + p0 * d, np, h->dinvell, h->kernel_id, h->rho, kb.B, h->dalpha, pw.Wz, pw.Vz, pw.S);
                launch_kg_point_final(s, pw.S, np, (int)d, pw.Z + p0 * d, h->dinvell, kb.As, kb.m, kb.al, h->kernel_id, h->rho, h->bias, h->sn2,
                                      pw.L, pw.f + p0, pw.g + p0 * d);
            }
            HIPCHK(h, hipGetLastError());
        }
        {
            Span sp(h, T_COPY);
            HIPCHK(h, hipMemcpyAsync(f, pw.f, (size_t)M * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(g, pw.g, (size_t)M * d * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(h, hipStreamSynchronize(s));
        return GPX_OK;
    });
}

// ---- Thompson / RFF ---------------------------------------------------------------------------
// the host image of the MFMA kernels' draw parameters (rff_sweep_ws): features padded to 128 per tile, k-major tiles
static void rff_retile(const double* W, const double* b, const double* theta, int64_t S, int64_t n, int64_t d, int64_t dp, int64_t nfb,
                       std::vector<double>& stage) {
    const int64_t nW = S * nfb * dp * TBH, nV = S * nfb * TBH;
    stage.assign((size_t)(rff_sweep_ws(WsCarver(nullptr), nW, nV).bytes / 8), 0.0);
    const auto [Wt, bt, tt, nbytes] = rff_sweep_ws(WsCarver(stage.data()), nW, nV);
    for (int64_t q = 0; q < S; ++q)
        for (int64_t j = 0; j < n; ++j) {
            const int64_t fb = j / TBH, c = j % TBH;
            for (int64_t kk = 0; kk < d; ++kk)
                Wt[((q * nfb + fb) * dp + kk) * TBH + c] = W[(q * n + j) * d + kk];
            bt[(q * nfb + fb) * TBH + c] = b[q * n + j];
            tt[(q * nfb + fb) * TBH + c] = theta[q * n + j];
        }
}

// path (gpx_path_sweep*): the weights (S, nv) of the update term that k_path_update adds to the feature part before the top-k
struct PathArg { const double* v; int64_t nv; };

static int rff_core(gpx_handle* h, const double* W, const double* b, const double* theta, int64_t S,
                    int64_t n, int64_t d, double bias, const double* dXc, int64_t M, int64_t k,
                    double* top_val, int64_t* top_idx, double* d_vals, const PathArg* path = nullptr) {
    if (!W || !b || !theta || !dXc) return fail(h, GPX_EARG, "rff_sweep: NULL pointer");
    if (S < 1 || n < 1 || d < 1 || M < 1) return fail(h, GPX_EARG, "rff_sweep: bad sizes");
    if (d > DMAX_RFF) return fail(h, GPX_EARG, "rff_sweep: d must be <= 1024");
    if (k < 0 || k > TOPK_MAX) return fail(h, GPX_EARG, "rff_sweep: k must be in [0, 4096]");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    // re-tile the draw parameters for the MFMA kernel: features padded to 128 per tile, k-major tiles
    const int64_t dp = (d + 3) / 4 * 4;
    const int64_t nfb = (n + TBH - 1) / TBH;
    const int64_t nW = S * nfb * dp * TBH, nV = S * nfb * TBH;
    std::vector<double> stage;      // the host image of the device layout
    rff_retile(W, b, theta, S, n, d, dp, nfb, stage);
    if ((rc = ensure(h, h->drff, h->cap_rff, rff_sweep_ws(WsCarver(nullptr), nW, nV).bytes / 8))) return rc;
    const RffSweepWs rw = rff_sweep_ws(WsCarver(h->drff), nW, nV);
    HIPCHK(h, hipMemcpyAsync(rw.Wt, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));   // `stage` is a local buffer
    if (!d_vals) {
        if ((rc = ensure(h, h->dout, h->cap_out, S * M))) return rc;
        d_vals = h->dout;
    }
    {
        Span sp(h, T_RFF);
        Span sp2(h, T_RFFSWEEP);          // the Thompson sweep kernel alone (bench.py: roofline_rff)
        launch_rff_mfma(s, rw.Wt, rw.bt, rw.tt, (int)S, (int)nfb, (int)n, (int)d, (int)dp, bias, dXc, M, d_vals, h->dclk + 2);
    }
    if (path) {
        // (bias + feature sum) + update: the second term on top of what the kernel above left in d_vals
        const int64_t nv = path->nv;
        if ((rc = ensure(h, h->dpath, h->cap_path, path_sweep_ws(WsCarver(nullptr), S, nv).bytes / 8))) return rc;
        const PathSweepWs pw = path_sweep_ws(WsCarver(h->dpath), S, nv);
        HIPCHK(h, hipMemcpyAsync(pw.v, path->v, (size_t)S * nv * 8, hipMemcpyHostToDevice, s));      // (the caller's buffer: it outlives the call's last wait)
        Span sp(h, T_RFF);
        launch_path_update(s, h->dXs, (int)d, pw.v, nv, S, pw.frag, dXc, M, h->dinvell, h->kernel_id, h->rho, d_vals);
    }
    // algorithmic double-precision lane operations of that launch: per (draw, feature, candidate) d multiply-adds of the
    // projection + 20 instructions of the cosine epilogue (kernels_rff.hip: cos_cw and the weighted sum)
    h->tacc[T_RFFOPS] += (double)S * (double)n * ((double)d + 20.0) * (double)M;
    if (k > 0) {
        const int64_t nblk = topk_blocks(M);
        // all draws ranked by one pair of launches while their block lists fit a modest buffer (k <= 64 per pass, S rows)
        const bool rows = k <= TOPK_PASS && S * nblk * k <= ((int64_t)1 << 24) && S <= 65535;
        const int64_t nlist = rows ? S * nblk * k : nblk * k;
        if ((rc = ensure(h, h->dblkv, h->cap_blk, nlist))) return rc;
        if ((rc = ensure(h, h->dblki, h->cap_blki, nlist))) return rc;
        if ((rc = ensure(h, h->dtopv, h->cap_top, std::max<int64_t>((int64_t)TOPK_MAX * 2, S * k * 2)))) return rc;
        double* tv = h->dtopv;
        int64_t* ti = reinterpret_cast<int64_t*>(h->dtopv + S * k);
        {
            Span sp(h, T_RFF);
            if (rows)
                launch_topk_rows(s, d_vals, M, S, (int)k, h->dblkv, h->dblki, nblk, tv, ti);
            else
                for (int64_t q = 0; q < S; ++q)
                    launch_topk(s, d_vals + q * M, M, (int)k, h->dblkv, h->dblki, nblk, tv + q * k, ti + q * k);
        }
        h->last_topv = tv; h->last_topi = ti; h->last_topn = S * k;
        HIPCHK(h, hipMemcpyAsync(top_val, tv, (size_t)S * k * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(top_idx, ti, (size_t)S * k * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    return GPX_OK;
}

// The host form of gpx_rff_sweep and gpx_path_sweep (`path`), behind the entry's own checks: the candidates staged in h->dXc, the values in
// h->dout, copied back where asked for
static int rff_host(gpx_handle* h, const double* W, const double* b, const double* theta, int64_t S, int64_t n, int64_t d, double bias,
                    const double* Xc, int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* vals_all, const PathArg* path) {
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->dXc, h->cap_xc, M * d))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->dXc, Xc, (size_t)M * d * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = ensure(h, h->dout, h->cap_out, S * M))) return rc;
    if ((rc = rff_core(h, W, b, theta, S, n, d, bias, h->dXc, M, k, top_val, top_idx, h->dout, path))) return rc;
    if (vals_all) {
        HIPCHK(h, hipMemcpyAsync(vals_all, h->dout, (size_t)S * M * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return GPX_OK;
}

extern "C" int gpx_rff_sweep_dev(gpx_handle* h, const double* W, const double* b, const double* theta,
                                 int64_t S, int64_t n, int64_t d, double bias, const double* dXc, int64_t M,
                                 int64_t k, double* top_val, int64_t* top_idx, double* d_vals_all) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return rff_core(h, W, b, theta, S, n, d, bias, dXc, M, k, top_val, top_idx, d_vals_all);
    });
}

extern "C" int gpx_rff_sweep(gpx_handle* h, const double* W, const double* b, const double* theta, int64_t S,
                             int64_t n, int64_t d, double bias, const double* Xc, int64_t M, int64_t k,
                             double* top_val, int64_t* top_idx, double* vals_all) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (!Xc || M < 1 || d < 1) return fail(h, GPX_EARG, "rff_sweep: bad candidates");
        return rff_host(h, W, b, theta, S, n, d, bias, Xc, M, k, top_val, top_idx, vals_all, nullptr);
    });
}

extern "C" int gpx_rff_grad(gpx_handle* h, const double* W, const double* b, const double* theta, int64_t n,
                            int64_t d, double bias, const double* Xc, int64_t M, double* f, double* g) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        return gpx::rff_grad_host(h, W, b, theta, n, d, bias, Xc, M, f, g);
    });
}

// ---- pathwise Thompson draws (kernels_path.hip) --------------------------------------------------------------------------
static int path_check(gpx_handle* h, const char* what, const void* v, int64_t nv, int64_t S, int64_t n, int64_t d) {
    char msg[160];
    if (!h->fitted) {
        snprintf(msg, sizeof msg, "%s: model is not fitted", what);
        return fail(h, GPX_ESTATE, msg);
    }
    const char* bad = !v ? "NULL weights" : d != h->d ? "d must equal the fitted model's" : (nv < 1 || nv > h->N) ? "nv must be in [1, N]"
                      : S < 1 ? "S must be >= 1" : (n < 1 || n > 4096) ? "n must be in [1, 4096]" : nullptr;
    if (!bad) return GPX_OK;
    snprintf(msg, sizeof msg, "%s: %s", what, bad);
    return fail(h, GPX_EARG, msg);
}

extern "C" int gpx_path_sweep_dev(gpx_handle* h, const double* W, const double* b, const double* theta, const double* v, int64_t nv,
                                  int64_t S, int64_t n, int64_t d, double bias, const double* dXc, int64_t M, int64_t k,
                                  double* top_val, int64_t* top_idx, double* d_vals_all) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (int rc = path_check(h, "path_sweep", v, nv, S, n, d)) return rc;
        const PathArg pa = {v, nv};
        return rff_core(h, W, b, theta, S, n, d, bias, dXc, M, k, top_val, top_idx, d_vals_all, &pa);
    });
}

extern "C" int gpx_path_sweep(gpx_handle* h, const double* W, const double* b, const double* theta, const double* v, int64_t nv,
                              int64_t S, int64_t n, int64_t d, double bias, const double* Xc, int64_t M, int64_t k,
                              double* top_val, int64_t* top_idx, double* vals_all) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (int rc0 = path_check(h, "path_sweep", v, nv, S, n, d)) return rc0;
        if (!Xc || M < 1) return fail(h, GPX_EARG, "path_sweep: bad candidates");
        if (k < 0 || k > TOPK_MAX) return fail(h, GPX_EARG, "path_sweep: k must be in [0, 4096]");
        const PathArg pa = {v, nv};
        return rff_host(h, W, b, theta, S, n, d, bias, Xc, M, k, top_val, top_idx, vals_all, &pa);
    });
}

extern "C" int gpx_path_grad(gpx_handle* h, const double* W, const double* b, const double* theta, const double* v, int64_t nv,
                             int64_t n, int64_t d, double bias, const double* Xc, int64_t M, double* f, double* g) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (int rc = path_check(h, "path_grad", v, nv, 1, n, d)) return rc;
        if (!W || !b || !theta || !Xc || !f || !g) return fail(h, GPX_EARG, "path_grad: NULL pointer");
        if (M < 1 || M > JOINT_MAX_M) return fail(h, GPX_EARG, "path_grad: M must be in [1, 4096]");
        return gpx::path_grad_host(h, W, b, theta, v, nv, n, d, bias, Xc, M, f, g);
    });
}

// The weights of S draws.  The prior at the observations is the Thompson sweep kernel's feature sum over the handle's own inputs
// (bias 0), r the right-hand sides as panels of 128 draws, v = U (T r) by the panel products of the joint posterior (k_cov_trmm) and
// the knowledge gradient (k_kg_solve).  Forms the inverse on first use; reads the fit only: no flush of queued corrections, the sweep
// cache, an announcement and their buffers are not touched.  One stream, one synchronisation (the staged host images live until it).
extern "C" int gpx_path_weights(gpx_handle* h, const double* W, const double* b, const double* w, const double* eps, int64_t S,
                                int64_t n, double sc, double* theta, double* v) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (int rc0 = path_check(h, "path_weights", v, 1, S, n, h->d)) return rc0;
        if (!W || !b || !w || !theta) return fail(h, GPX_EARG, "path_weights: NULL pointer");
        if (!std::isfinite(sc)) return fail(h, GPX_EARG, "path_weights: sc must be finite");
        const int64_t d = h->d;
        if (d > DMAX_RFF) return fail(h, GPX_EARG, "path_weights: d must be <= 1024");
        HIPCHK(h, hipSetDevice(h->device));
        int rc;
        if ((rc = ensure_inverse(h))) return rc;
        hipStream_t s = h->stream;
        const int64_t N = h->N, Np = h->Np, Sp = (S + TBH - 1) / TBH * TBH;
        for (int64_t e = 0; e < S * n; ++e) theta[e] = sc * w[e];
        const int64_t dp = (d + 3) / 4 * 4, nfb = (n + TBH - 1) / TBH;
        const int64_t nW = S * nfb * dp * TBH, nV = S * nfb * TBH;
        std::vector<double> stage;
        rff_retile(W, b, theta, S, n, d, dp, nfb, stage);
        if ((rc = ensure(h, h->drff, h->cap_rff, rff_sweep_ws(WsCarver(nullptr), nW, nV).bytes / 8))) return rc;
        if ((rc = ensure(h, h->dpath, h->cap_path, path_weights_ws(WsCarver(nullptr), S, N, Np, Sp, eps != nullptr).bytes / 8))) return rc;
        const RffSweepWs rw = rff_sweep_ws(WsCarver(h->drff), nW, nV);
        const PathWeightsWs pw = path_weights_ws(WsCarver(h->dpath), S, N, Np, Sp, eps != nullptr);
        {
            Span sp(h, T_COPY);
            HIPCHK(h, hipMemcpyAsync(rw.Wt, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, s));
            if (eps) HIPCHK(h, hipMemcpyAsync(pw.eps, eps, (size_t)S * N * 8, hipMemcpyHostToDevice, s));
        }
        {
            Span sp(h, T_RFF);
            launch_rff_mfma(s, rw.Wt, rw.bt, rw.tt, (int)S, (int)nfb, (int)n, (int)d, (int)dp, 0.0, h->dXraw, N, pw.prior, nullptr);
            launch_path_resid(s, h->dy, h->bias, pw.prior, pw.eps, sqrt(h->sn2), S, N, Np, Sp, pw.R);
            launch_cov_trmm(s, h->dU, Np, pw.R, Sp, pw.V);
            for (int64_t p = 0; p < Sp / TBH; ++p)
                launch_kg_solve(s, h->dU, Np, N, (int)std::min<int64_t>(TBH, S - p * TBH), pw.V + p * Np * TBH, pw.W + p * Np * TBH);
            launch_path_gather(s, pw.W, S, N, Np, pw.v);
            HIPCHK(h, hipGetLastError());
        }
        {
            Span sp(h, T_COPY);
            HIPCHK(h, hipMemcpyAsync(v, pw.v, (size_t)S * N * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(h, hipStreamSynchronize(s));
        return GPX_OK;
    });
}

// the wide-feature paths (n >= 128) one draw at a time: W (n,d) and b (n,) of draw q to the device
static int upload_draw(gpx_handle* h, const double* W, const double* b, int64_t q, int64_t n, double* dW, double* db) {
    HIPCHK(h, hipMemcpyAsync(dW, W + q * n * h->d, (size_t)n * h->d * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(db, b + q * n, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    return GPX_OK;
}

// feature Grams of S draws (n < 128 features each) on the device: dA (S,n,n), dv (S,n) inside h->drff, followed by
// `extra` spare doubles (*dextra) for the caller
static int rff_gram_batch_dev(gpx_handle* h, const double* W, const double* b, int64_t S, int64_t n, int64_t extra,
                              double** dA_out, double** dv_out, double** dextra) {
    hipStream_t s = h->stream;
    const int64_t d = h->d, Np = h->Np, N = h->N;
    int rc;
    // batched MFMA path: feature tiles [S][dp][128] k-major, phases [S][128]
    const int64_t dp = (d + 3) / 4 * 4;
    const int64_t nW = S * dp * TBH, nV = S * TBH;
    std::vector<double> stage((size_t)(nW + nV), 0.0);
    for (int64_t q = 0; q < S; ++q)
        for (int64_t j = 0; j < n; ++j) {
            for (int64_t kk = 0; kk < d; ++kk) stage[(size_t)((q * dp + kk) * TBH + j)] = W[(q * n + j) * d + kk];
            stage[(size_t)(nW + q * TBH + j)] = b[q * n + j];
        }
    if ((rc = ensure(h, h->drff, h->cap_rff, rff_gram_ws(WsCarver(nullptr), nW, nV, S, n, extra).bytes / 8))) return rc;
    if ((rc = ensure(h, h->drffs, h->cap_rffs, rff_gram_batch_scratch(S, Np)))) return rc;
    const RffGramWs gw = rff_gram_ws(WsCarver(h->drff), nW, nV, S, n, extra);
    HIPCHK(h, hipMemcpyAsync(gw.Wt, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));   // `stage` is a local buffer
    {
        Span sp(h, T_RFF);
        launch_rff_gram_batch(s, h->dXraw, N, Np, (int)d, (int)dp, gw.Wt, gw.bt, (int)S, (int)n, h->dy, h->bias,
                              h->drffs, gw.A, gw.v);
    }
    HIPCHK(h, hipGetLastError());
    *dA_out = gw.A;
    *dv_out = gw.v;
    if (dextra) *dextra = gw.extra;
    return GPX_OK;
}

extern "C" int gpx_rff_gram_batch(gpx_handle* h, const double* W, const double* b, int64_t S, int64_t n,
                                  double* A, double* v) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (h->stage < 1) return fail(h, GPX_ESTATE, "rff_gram: no data on the device (fit first)");
        if (!W || !b || !A || !v || n < 1 || S < 1) return fail(h, GPX_EARG, "rff_gram: bad arguments");
        HIPCHK(h, hipSetDevice(h->device));
        hipStream_t s = h->stream;
        const int64_t d = h->d, Np = h->Np, N = h->N;
        int rc;
        if (n >= TBH) {
            // wide feature maps: one draw at a time on the generic path
            if ((rc = ensure(h, h->drff, h->cap_rff, rff_wide_ws(WsCarver(nullptr), n, d, 0, Np, false).bytes / 8))) return rc;
            const RffWideWs ww = rff_wide_ws(WsCarver(h->drff), n, d, 0, Np, false);
            for (int64_t q = 0; q < S; ++q) {
                if ((rc = upload_draw(h, W, b, q, n, ww.W, ww.b))) return rc;
                {
                    Span sp(h, T_RFF);
                    launch_rff_gram(s, h->dXraw, ww.Ft, N, (int)d, ww.W, ww.b, (int)n, h->dy, h->bias, ww.A, ww.v);
                }
                HIPCHK(h, hipMemcpyAsync(A + q * n * n, ww.A, (size_t)n * n * 8, hipMemcpyDeviceToHost, s));
                HIPCHK(h, hipMemcpyAsync(v + q * n, ww.v, (size_t)n * 8, hipMemcpyDeviceToHost, s));
                HIPCHK(h, hipStreamSynchronize(s));
            }
            HIPCHK(h, hipGetLastError());
            return GPX_OK;
        }
        double *dA, *dv;
        if ((rc = rff_gram_batch_dev(h, W, b, S, n, 0, &dA, &dv, nullptr))) return rc;
        HIPCHK(h, hipMemcpyAsync(A, dA, (size_t)S * n * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(v, dv, (size_t)S * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        HIPCHK(h, hipGetLastError());
        return GPX_OK;
    });
}

extern "C" int gpx_rff_posterior(gpx_handle* h, const double* W, const double* b, const double* z, int64_t S,
                                 int64_t n, double sc, double* theta) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        if (h->stage < 1) return fail(h, GPX_ESTATE, "rff_posterior: no data on the device (fit first)");
        if (!W || !b || !z || !theta || n < 1 || S < 1) return fail(h, GPX_EARG, "rff_posterior: bad arguments");
        if (n > 4096) return fail(h, GPX_EARG, "rff_posterior: n <= 4096 features");
        if (!(sc > 0.0) || !(h->sn2 > 0.0)) return fail(h, GPX_EARG, "rff_posterior: needs sc > 0 and a noise variance > 0");
        if (n >= TBH) {
            // wide feature maps (n >= 128: the weight posterior no longer fits the LDS-resident kernel): per draw the
            // generic feature Gram, then B = sc^2 A + sn2 I factorised by the blocked Cholesky kernels and two vector
            // substitutions, all on the device -- nothing but theta crosses PCIe
            HIPCHK(h, hipSetDevice(h->device));
            hipStream_t s = h->stream;
            const int64_t d = h->d, Np = h->Np, N = h->N, np = (n + NB - 1) / NB * NB;
            int rc;
            if ((rc = ensure(h, h->drff, h->cap_rff, rff_wide_ws(WsCarver(nullptr), n, d, np, Np, true).bytes / 8))) return rc;
            const RffWideWs ww = rff_wide_ws(WsCarver(h->drff), n, d, np, Np, true);
            int* pflag = h->dflag + 8;
            for (int64_t q = 0; q < S; ++q) {
                if ((rc = upload_draw(h, W, b, q, n, ww.W, ww.b))) return rc;
                HIPCHK(h, hipMemcpyAsync(ww.z, z + q * n, (size_t)n * 8, hipMemcpyHostToDevice, s));
                int flag = 0;
                {
                    Span sp(h, T_RFF);
                    launch_rff_gram(s, h->dXraw, ww.Ft, N, (int)d, ww.W, ww.b, (int)n, h->dy, h->bias, ww.A, ww.v);
                    launch_posterior_wide(s, ww.A, ww.v, ww.z, (int)n, np, sc, h->sn2, ww.B, ww.R, ww.work, pflag, ww.th);
                }
                HIPCHK(h, hipMemcpyAsync(theta + q * n, ww.th, (size_t)n * 8, hipMemcpyDeviceToHost, s));
                HIPCHK(h, hipMemcpyAsync(&flag, pflag, sizeof(int), hipMemcpyDeviceToHost, s));
                HIPCHK(h, hipStreamSynchronize(s));
                HIPCHK(h, hipGetLastError());
                if (flag != 0) return fail(h, GPX_ENOTPD, "rff_posterior: the feature Gram of a draw is not positive definite");
            }
            return GPX_OK;
        }
        HIPCHK(h, hipSetDevice(h->device));
        hipStream_t s = h->stream;
        int rc;
        double *dA, *dv, *dz;
        if ((rc = rff_gram_batch_dev(h, W, b, S, n, 2 * S * n, &dA, &dv, &dz))) return rc;
        double* dth = dz + S * n;
        int* pflag = h->dflag + 8;                    // its own word: the factorisation's flag stays untouched
        HIPCHK(h, hipMemsetAsync(pflag, 0, sizeof(int), s));
        HIPCHK(h, hipMemcpyAsync(dz, z, (size_t)S * n * 8, hipMemcpyHostToDevice, s));
        {
            Span sp(h, T_RFF);
            launch_rff_posterior(s, dA, dv, dz, (int)S, (int)n, sc, h->sn2, dth, pflag);
        }
        int flag = 0;
        HIPCHK(h, hipMemcpyAsync(theta, dth, (size_t)S * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(&flag, pflag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        HIPCHK(h, hipGetLastError());
        if (flag != 0) return fail(h, GPX_ENOTPD, "rff_posterior: the feature Gram of a draw is not positive definite");
        return GPX_OK;
    });
}

extern "C" int gpx_rff_gram(gpx_handle* h, const double* W, const double* b, int64_t n, double* A, double* v) {
    return guarded(h, [&]() -> int {
        return gpx_rff_gram_batch(h, W, b, 1, n, A, v);
    });
}

// ---- sweeps that drive several fitted handles from one lead (ensemble, constrained, two objectives) --------------------------------
// The lead L owns the workspaces, the records and the error text; `role` and `first` are how its messages name handle i of hs
// ("ensemble member 0 ..", "constraint 0 ..", "objective 1 .."); `also`: a handle that takes part without being listed (the objective
// of a constrained sweep), or NULL.
struct Group { gpx_handle* L; gpx_handle* const* hs; int n; const char* role; int first; gpx_handle* also; };

// how messages name handle i (first = -1: the constrained batch lists its objective in front of constraint 0)
static std::string group_name(const Group& g, int i) {
    return g.first + i < 0 ? std::string("objective") : std::string(g.role) + " " + std::to_string(g.first + i);
}

// handle i's failure as the lead reports it
static int group_fail(const Group& g, const gpx_handle* h, int i, int rc) {
    if (h != g.L) g.L->err = group_name(g, i) + ": " + h->err;
    return rc;
}

// The conditions an entry may put on its handles, each with the text (behind the entry's name) of its refusal: GPX_ESTATE for an unfitted
// handle, GPX_EARG otherwise.  group_check applies the rules it is given and no other, in the entry's order: by_handle = every rule on
// handle 0, then on handle 1, .. (the ensemble entries); otherwise rule 0 on every handle, then rule 1, .. (constrained, two objectives).
enum GroupCond { G_NOT_NULL, G_ONCE, G_FITTED, G_SHAPE };
struct GroupRule { GroupCond cond; const char* msg; };
static bool group_holds(const Group& g, int i, GroupCond c) {
    const gpx_handle* h = g.hs[i];
    if (c == G_NOT_NULL) return h != nullptr;
    if (c == G_FITTED) return h->fitted;
    if (c == G_SHAPE) return h->device == g.L->device && h->d == g.L->d;
    return h != g.also && std::find(g.hs, g.hs + i, h) == g.hs + i;      // G_ONCE
}
static int group_check(const Group& g, const char* entry, std::initializer_list<GroupRule> rules, bool by_handle = false) {
    const int nr = (int)rules.size();
    for (int t = 0; t < nr * g.n; ++t) {
        const int i = by_handle ? t / nr : t % g.n;
        const GroupRule& r = rules.begin()[by_handle ? t % nr : t / g.n];
        if (!group_holds(g, i, r.cond)) return fail(g.L, r.cond == G_FITTED ? GPX_ESTATE : GPX_EARG, (std::string(entry) + ": " + r.msg).c_str());
    }
    return GPX_OK;
}

// One member step: sweep_core on handle i of the group for the `cnt` candidates X into the vectors given (no top-k), its failure as the lead
// reports it, then a synchronise of the member's stream -- what follows reads the vectors on the lead's.  s2_mean (optional): the mean of
// d_s2 -> *s2_mean, on the member's stream.
static int member_sweep(const Group& g, int i, int acq_id, const double* params, int nparams, const double* X, int64_t cnt, double* d_acq,
                        double* d_mu, double* d_s2, double* s2_mean = nullptr) {
    gpx_handle* h = g.hs[i];
    if (int rc = sweep_core(h, acq_id, params, nparams, X, cnt, 0, nullptr, nullptr, d_acq, d_mu, d_s2)) return group_fail(g, h, i, rc);
    if (s2_mean) launch_prune_mean(h->stream, d_s2, cnt, s2_mean);
    HIPCHK(g.L, hipStreamSynchronize(h->stream));
    return GPX_OK;
}

// ---- ensemble sweep (hyper-parameter marginalisation; pybo/bayesopt.py:115) ------------------------------
static int ensemble_core(gpx_handle* const* mem, int n, int acq_id, const double* params, int nparams,
                         const double* dXc, int64_t M, int64_t k, double* top_val, int64_t* top_idx,
                         double* d_out, double* d_mu, double* d_s2) {
    gpx_handle* L = mem[0];
    const Group g = {L, mem, n, "ensemble member", 0, nullptr};
    L->ens_rec = gpx_handle::EnsPruneRecord();     // every ensemble sweep entry, refused ones included, ends the previous one's record
    int rc;
    if ((rc = check_acq(L, "ensemble_sweep", acq_id, params, nparams, n))) return rc;
    const int mesS = (acq_id == GPX_ACQ_MES) ? nparams / n : 0;      // MES: member m scores with its own slice of the maxima
    if (!dXc || M < 1) return fail(L, GPX_EARG, "ensemble_sweep: need M >= 1 candidates");
    if ((rc = check_topk(L, "ensemble_sweep", k, top_val, top_idx))) return rc;
    if ((rc = group_check(g, "ensemble_sweep", {{G_FITTED, "a member model is not fitted"}, {G_SHAPE, "members must share the device and the input dimension"}}, true)))
        return rc;
    HIPCHK(L, hipSetDevice(L->device));
    // mixture moments for UCB / mean (mu = mean mu_m, s2 = mean(s2_m + mu_m^2) - mu^2), plain mean for EI / PI
    const int mode = (acq_id == GPX_ACQ_UCB || acq_id == GPX_ACQ_MEAN) ? 1 : 0;
    if ((rc = ensure(L, L->dens, L->cap_ens, ens_ws(WsCarver(nullptr), M).bytes / 8))) return rc;
    const EnsWs ew = ens_ws(WsCarver(L->dens), M);
    double *const acc0 = ew.acc0, *const acc1 = ew.acc1, *const t0 = ew.t0, *const t1 = ew.t1, *const out = d_out ? d_out : ew.out;
    const double beta = (acq_id == GPX_ACQ_UCB) ? params[0] : 0.0;

    // The exact ensemble chain for the `cnt` candidates X: every member's sweep in member order, each folded into the running
    // sums, then one division -> o[c] (and mu / s2, where given).  A candidate's value depends on its coordinates alone.
    // gate_mean (mode 0 only): member m's mean s2 over these candidates -> gate_mean[m] (its s2 vector passes through t1).
    auto members = [&](const double* X, int64_t cnt, double* o, double* o_mu, double* o_s2, double* gate_mean = nullptr) -> int {
        for (int m = 0; m < n; ++m) {
            int rcm = (mode == 0) ? member_sweep(g, m, acq_id, mesS ? params + (size_t)m * mesS : params, mesS ? mesS : nparams, X, cnt, t0, nullptr,
                                                 gate_mean ? t1 : nullptr, gate_mean ? gate_mean + m : nullptr)
                                  : member_sweep(g, m, GPX_ACQ_MEAN, nullptr, 0, X, cnt, nullptr, t0, t1);
            if (rcm) return rcm;
            launch_ens_accum(L->stream, acc0, acc1, t0, t1, cnt, mode, m == 0);
            HIPCHK(L, hipStreamSynchronize(L->stream));    // t0/t1 are reused by the next member
        }
        if (acq_id == GPX_ACQ_MEAN)     // value = mixture mean
            launch_ens_finish(L->stream, acc0, acc1, cnt, 1, (double)n, 0.0, o, o_mu, o_s2);
        else
            launch_ens_finish(L->stream, acc0, acc1, cnt, mode, (double)n, beta, o, o_mu, o_s2);
        return GPX_OK;
    };

    // ---- selection-only ensemble sweep: select_topk_pruned on the MEAN of the members' bounds ----
    // The sum of the members' bounds, accumulated and divided exactly as `members` accumulates and divides their values, is >= the
    // ensemble's value bit for bit (addition and division by n > 0 are monotone).  The lead's option "prune" governs.
    int nPmax = 0;               // (the member with the most block rows: the smallest generation)
    int64_t Np_min = INT64_MAX;
    bool members_ok = true;
    for (int m = 0; m < n; ++m) {
        nPmax = std::max(nPmax, (int)(mem[m]->Np / NB));
        Np_min = std::min(Np_min, mem[m]->Np);
        members_ok = members_ok && !mem[m]->cache_on && mem[m]->rho >= gpx::S2_FLOOR && mem[m]->rho < INFINITY;
    }
    hipStream_t s = L->stream;
    gpx_handle::EnsPruneRecord& rec = L->ens_rec;
    rec.n = n;
    PruneWs w;                   // the lead's: the ensemble bound vector, seeds and survivors; extra = [gate means n][delta n][bound_fact n]
    SelectOps ops;
    ops.exact = exact_rows(members, L->d);
    // the members' mean s2 / rho over the first generation decides
    ops.gate = [&](int64_t Gg, double* value, bool* go) -> int {
        if ((rc = members(dXc, Gg, out, nullptr, nullptr, w.extra))) return rc;
        std::vector<double> gm((size_t)n);
        HIPCHK(L, hipMemcpyAsync(gm.data(), w.extra, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(L, hipStreamSynchronize(s));
        double sum = 0.0;
        for (int m = 0; m < n; ++m) sum += gm[m] / mem[m]->rho;
        *value = sum / (double)n;
        *go = *value >= PRUNE_GATE_S2;
        return GPX_OK;
    };
    // per member in member order: its dots (own factor, weights and workspace) -> t1, its EI bound folded into the running sum ub; then ub / n
    ops.bound = [&](double* ub, int64_t done) -> int {
        double* const delta = w.extra + n;
        for (int m = 0; m < n; ++m) {
            gpx_handle* h = mem[m];
            HIPCHK(L, hipSetDevice(h->device));
            if ((rc = ensure_inverse(h))) return group_fail(g, h, m, rc);
            PruneWs wm = w;
            if (h != L) {
                h->prune_rec = gpx_handle::PruneRecord();      // (the pass overwrites the workspace its last record points into)
                if ((rc = prune_ws(h, 0, 0, 0, 0, wm))) return group_fail(g, h, m, rc);
            }
            {
                Span sp(h, T_BOUND);
                const bool bound_mfma = bound_dots(h, dXc, M, wm, t1);
                launch_prune_ub_fold(h->stream, t1, ub, M, wm.sc, h->rho, h->bias, params[0], m == 0, delta + m,
                                     bound_mfma ? 1 : 0, delta + n + m);
            }
            HIPCHK(L, hipStreamSynchronize(h->stream));      // t1 and ub pass to the next member's stream
        }
        {
            Span sp(L, T_BOUND);
            launch_prune_ub_mean(s, ub, M, done, (double)n);
        }
        rec.delta = delta;
        return GPX_OK;
    };
    ops.after_seeds = seeds_sync(L);
    // (narrow = false: the ensemble keeps the wide generation of seeds.  It has no second bound, so every member evaluates the whole
    //  first-level list, and the list that 256 seeds leave is longer by more than the seeds save: 153.5 against 150.5 ms per step of
    //  bench.py --ensemble 10, profiles/narrow_seeds_ab.md section 2.  The members' short launches are narrow all the same.)
    int64_t done = 0;
    if ((rc = select_topk_pruned(L, members_ok, !d_out && !d_mu && !d_s2, acq_id, n, nPmax, Np_min, false, dXc, M, k, 3 * n, false, w, L->ens_hint, rec,
                                 out, ops, &done)))
        return rc;
    if ((rc = plain_rest(ops, dXc, done, sweep_chunk(L, M), M, out, d_mu, d_s2))) return rc;
    return finish_sweep(L, out, M, k, top_val, top_idx);
}

static int ensemble_check(gpx_handle* const* members, int n) {
    if (!members || n < 1 || !members[0]) return GPX_EARG;
    return group_check({members[0], members, n, "ensemble member", 0, nullptr}, "ensemble_sweep", {{G_NOT_NULL, "NULL member handle"}});
}

extern "C" int gpx_ensemble_predict(gpx_handle* const* members, int n_members, const double* Xc, int64_t M,
                                    double* mu, double* s2, double* dmu, double* ds2) {
    if (ensemble_check(members, n_members)) return GPX_EARG;
    gpx_handle* h = members[0];
    return guarded(h, [&]() -> int {
        if (!mu || !s2 || !dmu || !ds2) return fail(h, GPX_EARG, "ensemble_predict: all four outputs are required");
        return gpx::ensemble_predict_grad_host(members, n_members, Xc, M, mu, s2, dmu, ds2);
    });
}

extern "C" int gpx_ensemble_sweep_dev(gpx_handle* const* members, int n_members, int acq_id, const double* params,
                                      int nparams, const double* dXc, int64_t M, int64_t k, double* top_val,
                                      int64_t* top_idx, double* d_acq_all, double* d_mu, double* d_s2) {
    if (ensemble_check(members, n_members)) return GPX_EARG;
    return guarded(members[0], [&]() -> int {
        return ensemble_core(members, n_members, acq_id, params, nparams, dXc, M, k, top_val, top_idx, d_acq_all,
                             d_mu, d_s2);
    });
}

extern "C" int gpx_ensemble_sweep(gpx_handle* const* members, int n_members, int acq_id, const double* params,
                                  int nparams, const double* Xc, int64_t M, int64_t k, double* top_val,
                                  int64_t* top_idx, double* acq_all, double* mu, double* s2) {
    if (ensemble_check(members, n_members)) return GPX_EARG;
    gpx_handle* h = members[0];
    return guarded(h, [&]() -> int {
        h->ens_rec = gpx_handle::EnsPruneRecord();
        if (!Xc || M < 1) return fail(h, GPX_EARG, "ensemble_sweep: need M >= 1 candidates");
        if ((mu || s2) && acq_id != GPX_ACQ_UCB && acq_id != GPX_ACQ_MEAN)
            return fail(h, GPX_EARG, "ensemble_sweep: mixture moments are only formed for UCB / mean");
        // (true: the members read the candidates from their own streams)
        return staged_sweep(h, Xc, M, true, acq_all, mu, s2, [&](double* dX, double* dacq, double* dmu, double* ds2) {
            return ensemble_core(members, n_members, acq_id, params, nparams, dX, M, k, top_val, top_idx, dacq, dmu, ds2);
        });
    });
}

// ---- constrained sweep: EI or PI of the objective times the probability of feasibility of every constraint ----
static const int CON_MAX = 16;

static gpx_handle* con_lead(gpx_handle* obj, gpx_handle* const* cons, int nc) {
    return obj ? obj : (cons && nc >= 1 ? cons[0] : nullptr);
}

static Group con_group(gpx_handle* obj, gpx_handle* const* cons, int nc) {
    return {con_lead(obj, cons, nc), cons, nc, "constraint", 0, obj};
}

// The refusals every constrained entry shares (`what`: its name), in two parts with the entry's own arguments checked between them:
// the constraints, thresholds and the objective's acquisition ..
static int constrained_check_args(gpx_handle* L, const char* what, gpx_handle* obj, gpx_handle* const* cons, int nc, const double* thr, int acq_id,
                                  const double* params, int nparams) {
    const std::string w(what);
    if (!cons || nc < 1 || nc > CON_MAX) return fail(L, GPX_EARG, (w + ": takes 1 to 16 constraint handles").c_str());
    int rc;
    if ((rc = group_check(con_group(obj, cons, nc), what, {{G_NOT_NULL, "NULL constraint handle"}}))) return rc;
    if (!thr) return fail(L, GPX_EARG, (w + ": NULL thresholds").c_str());
    for (int j = 0; j < nc; ++j)
        if (!std::isfinite(thr[j])) return fail(L, GPX_EARG, (w + ": the thresholds must be finite").c_str());
    if (obj) {
        if (acq_id != GPX_ACQ_EI && acq_id != GPX_ACQ_PI)
            return fail(L, GPX_EARG, (w + ": the objective's acquisition must be EI or PI (non-negative values)").c_str());
        if ((rc = check_acq(L, what, acq_id, params, nparams))) return rc;
    }
    return GPX_OK;
}
// .. and the handles: each once, fitted, on one device with one input dimension
static int constrained_check_handles(gpx_handle* L, const char* what, gpx_handle* obj, gpx_handle* const* cons, int nc) {
    const Group g = con_group(obj, cons, nc);
    if (int rc = group_check(g, what, {{G_ONCE, "a handle appears twice"}})) return rc;
    if (obj && !obj->fitted) return fail(L, GPX_ESTATE, (std::string(what) + ": the objective's model is not fitted").c_str());
    return group_check(g, what, {{G_FITTED, "a constraint's model is not fitted"}, {G_SHAPE, "the handles must share the device and the input dimension"}});
}

// every refusal of gpx_constrained_sweep[_dev], before anything touches a handle's fit, cache or queue
static int constrained_check(gpx_handle* L, gpx_handle* obj, gpx_handle* const* cons, int nc, const double* thr, int acq_id, const double* params,
                             int nparams, const double* Xc, int64_t M, int64_t k, const double* top_val, const int64_t* top_idx) {
    int rc;
    if ((rc = constrained_check_args(L, "constrained_sweep", obj, cons, nc, thr, acq_id, params, nparams))) return rc;
    if (!Xc || M < 1) return fail(L, GPX_EARG, "constrained_sweep: need M >= 1 candidates");
    if ((rc = check_topk(L, "constrained_sweep", k, top_val, top_idx))) return rc;
    return constrained_check_handles(L, "constrained_sweep", obj, cons, nc);
}

// (arguments checked by constrained_check)
static int constrained_core(gpx_handle* obj, gpx_handle* const* cons, int nc, const double* thr, int acq_id, const double* params, int nparams,
                            const double* dXc, int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* d_out, double* d_pof) {
    const Group g = con_group(obj, cons, nc);
    gpx_handle* L = g.L;
    int rc;
    HIPCHK(L, hipSetDevice(L->device));
    if ((rc = ensure(L, L->dcon, L->cap_con, con_ws(WsCarver(nullptr), M).bytes / 8))) return rc;
    const ConWs cw = con_ws(WsCarver(L->dcon), M);
    double *const t0 = cw.t0, *const out = d_out ? d_out : cw.out;
    hipStream_t s = L->stream;

    // The exact chain for the `cnt` candidates X: the objective's value into o, then per constraint in the caller's order its probability
    // of feasibility (its own sweep: the bits of gpx_sweep(GPX_ACQ_PI)) -> t0, folded into o (and into o_pof, the probability of
    // feasibility alone, where given).  Without an objective o is that probability.  o_s2: the objective's s2 (the gate).
    auto chain = [&](const double* X, int64_t cnt, double* o, double* o_pof, double* o_s2) -> int {
        if (obj && (rc = sweep_core(obj, acq_id, params, nparams, X, cnt, 0, nullptr, nullptr, o, nullptr, o_s2))) return rc;
        for (int j = 0; j < nc; ++j) {
            if ((rc = member_sweep(g, j, GPX_ACQ_PI, thr + j, 1, X, cnt, t0, nullptr, nullptr))) return rc;
            launch_con_fold(s, obj ? o : nullptr, obj ? o_pof : o, t0, cnt, j == 0);
            HIPCHK(L, hipStreamSynchronize(s));      // t0 is reused by the next constraint
        }
        if (!obj && o_pof) HIPCHK(L, hipMemcpyAsync(o_pof, o, (size_t)cnt * 8, hipMemcpyDeviceToDevice, s));
        return GPX_OK;
    };

    // ---- selection-only constrained sweep: select_topk_pruned on the OBJECTIVE's EI bound ----
    // Every factor lies in [0, 1] (con_fold's clamp) and fl(a p) <= a for a >= 0, so the single model's bound on EI is a bound on the
    // product bit for bit; the constraints are swept over seeds and survivors only.  The objective's option "prune" governs, the automatic
    // rule included (measured: profiles/constrained_sweep.md).
    int nPmax = (int)(L->Np / NB);
    int64_t Np_min = L->Np;
    bool legal = obj && obj->rho >= gpx::S2_FLOOR && obj->rho < INFINITY && !obj->cache_on;
    for (int j = 0; j < nc; ++j) {
        nPmax = std::max(nPmax, (int)(cons[j]->Np / NB));
        Np_min = std::min(Np_min, cons[j]->Np);
        legal = legal && !cons[j]->cache_on;
    }
    gpx_handle::ConPruneRecord& rec = L->con_rec;
    rec.nc = nc;
    PruneWs w;                   // the lead's: the objective's bound vector, seeds and survivors
    PruneHint hint;              // (local: these sweeps neither read nor arm the decisions the lead carries for its own sweeps)
    SelectOps ops;
    // (plain_rest's mu slot carries the probability of feasibility; selection-only calls pass none)
    ops.exact = exact_rows(chain, L->d);
    // the single model's gate and bound, on the objective (a legal sweep has one, and it leads): no constraint is touched by either
    ops.gate = [&](int64_t Gg, double* value, bool* go) -> int { return single_gate(obj, ops, dXc, out, w, Gg, value, go); };
    ops.bound = [&](double* ub, int64_t done) -> int {
        // (with "prune" = 1 this pass is the first reader of the objective's inverse and `a`: no gate, no sweep_core before it)
        HIPCHK(L, hipSetDevice(obj->device));
        if ((rc = ensure_inverse(obj))) return rc;
        return single_bound(obj, dXc, M, w, params[0], t0, nullptr, ub, done);      // (dots -> t0: no constraint runs during the pass)
    };
    ops.after_seeds = seeds_sync(L);
    int64_t done = 0;
    // (the driver reads and arms nothing but `hint`: the one place that consults prune_hint.h stays the driver itself)
    if ((rc = select_topk_pruned(L, legal, !d_out && !d_pof, obj ? acq_id : -1, 1 + nc, nPmax, Np_min, false, dXc, M, k, 0, false, w, hint, rec, out,
                                 ops, &done)))
        return rc;
    if ((rc = plain_rest(ops, dXc, done, sweep_chunk(L, M), M, out, d_pof, nullptr))) return rc;
    return finish_sweep(L, out, M, k, top_val, top_idx);
}

extern "C" int gpx_constrained_sweep_dev(gpx_handle* obj, gpx_handle* const* cons, int nc, const double* thr, int acq_id, const double* params,
                                         int nparams, const double* dXc, int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* d_acq_all,
                                         double* d_pof_all) {
    gpx_handle* L = con_lead(obj, cons, nc);
    if (!L) return GPX_EARG;
    return guarded(L, [&]() -> int {
        L->con_rec = gpx_handle::ConPruneRecord();     // every constrained sweep entry, refused ones included, ends the previous one's record
        if (int rc = constrained_check(L, obj, cons, nc, thr, acq_id, params, nparams, dXc, M, k, top_val, top_idx)) return rc;
        return constrained_core(obj, cons, nc, thr, acq_id, params, nparams, dXc, M, k, top_val, top_idx, d_acq_all, d_pof_all);
    });
}

extern "C" int gpx_constrained_sweep(gpx_handle* obj, gpx_handle* const* cons, int nc, const double* thr, int acq_id, const double* params,
                                     int nparams, const double* Xc, int64_t M, int64_t k, double* top_val, int64_t* top_idx, double* acq_all,
                                     double* pof_all) {
    gpx_handle* L = con_lead(obj, cons, nc);
    if (!L) return GPX_EARG;
    return guarded(L, [&]() -> int {
        L->con_rec = gpx_handle::ConPruneRecord();
        if (int rc = constrained_check(L, obj, cons, nc, thr, acq_id, params, nparams, Xc, M, k, top_val, top_idx)) return rc;
        // (true: the constraints read the candidates from their own streams; the staging's mu slot carries the probability of feasibility)
        return staged_sweep(L, Xc, M, true, acq_all, pof_all, nullptr, [&](double* dX, double* dacq, double* dpof, double*) {
            return constrained_core(obj, cons, nc, thr, acq_id, params, nparams, dX, M, k, top_val, top_idx, dacq, dpof);
        });
    });
}

extern "C" int gpx_constrained_prune_report(gpx_handle* lead, double* scal, int nscal, double* ub, int64_t* idx, int64_t cap_idx) {
    return guarded(lead, [&]() -> int {
        gpx_handle* h = lead;
        if (!h) return GPX_EARG;
        const gpx_handle::ConPruneRecord& r = h->con_rec;
        double out[11];
        if (int rc = report_begin(h, "constrained_prune_report", "constrained sweep", " led by this handle", r, true, scal, nscal, ub || idx, nullptr, out))
            return rc;
        out[8] = NAN, out[9] = r.gate, out[10] = NAN;
        if (r.path >= 2) {
            HIPCHK(h, hipMemcpy(&out[8], r.sc + 5, 8, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(&out[10], r.sc + 1, 8, hipMemcpyDeviceToHost));
        }
        for (int i = 0; i < nscal && i < 11; ++i) scal[i] = out[i];
        return report_vectors(h, r, ub, idx, cap_idx);
    });
}

// ---- two-objective sweep: expected hypervolume improvement over a Pareto front ----
// The front's part of every refusal, and the strips (ehvi_math.h: a then b, n + 2 doubles each) the fold reads.  Touches no handle but
// the lead's error text.
static int ehvi_front(gpx_handle* L, const char* what, const double* P, int np, const double* ref, std::vector<double>& strips, int& n) {
    const std::string w(what);
    if (!ref || !std::isfinite(ref[0]) || !std::isfinite(ref[1])) return fail(L, GPX_EARG, (w + ": the reference point must be two finite doubles").c_str());
    if (np < 0 || np > EHVI_MAX_RAW) return fail(L, GPX_EARG, (w + ": takes 0 to 4096 raw front points").c_str());
    if (np > 0 && !P) return fail(L, GPX_EARG, (w + ": NULL front").c_str());
    for (int i = 0; i < 2 * np; ++i)
        if (!std::isfinite(P[i])) return fail(L, GPX_EARG, (w + ": the front must be finite").c_str());
    std::vector<double> a((size_t)np + 2), b((size_t)np + 2, 0.0);
    n = ehvi_strips(P, np, ref, a.data(), b.data());
    if (n > EHVI_MAX_FRONT) return fail(L, GPX_EARG, (w + ": more than 1024 non-dominated points above the reference point").c_str());
    strips.assign((size_t)2 * (n + 2), 0.0);
    std::copy(a.begin(), a.begin() + n + 2, strips.begin());
    std::copy(b.begin(), b.begin() + n + 1, strips.begin() + n + 2);
    return GPX_OK;
}

// every refusal of gpx_ehvi_sweep[_dev], before anything touches a handle's fit, cache or queue (f1 is not NULL)
static int ehvi_check(gpx_handle* f1, gpx_handle* f2, const double* P, int np, const double* ref, const double* Xc, int64_t M, int64_t k,
                      const double* top_val, const int64_t* top_idx, std::vector<double>& strips, int& n) {
    gpx_handle* const hs[2] = {f1, f2};
    const Group g = {f1, hs, 2, "objective", 1, nullptr};
    int rc;
    if ((rc = group_check(g, "ehvi_sweep", {{G_NOT_NULL, "NULL handle"}, {G_ONCE, "the two objectives need a handle each"}}))) return rc;
    if ((rc = ehvi_front(f1, "ehvi_sweep", P, np, ref, strips, n))) return rc;
    if (!Xc || M < 1) return fail(f1, GPX_EARG, "ehvi_sweep: need M >= 1 candidates");
    if ((rc = check_topk(f1, "ehvi_sweep", k, top_val, top_idx))) return rc;
    return group_check(g, "ehvi_sweep", {{G_FITTED, "an objective's model is not fitted"}, {G_SHAPE, "the handles must share the device and the input dimension"}});
}

// the lead's workspace for M candidates and a front of n points
static int ehvi_layout(gpx_handle* L, int64_t M, int n, EhviWs& w) {
    if (int rc = ensure(L, L->dehvi, L->cap_ehvi, ehvi_ws(WsCarver(nullptr), M, n).bytes / 8)) return rc;
    w = ehvi_ws(WsCarver(L->dehvi), M, n);
    return GPX_OK;
}

// The fold and the top-k on the lead's stream: mom (4, M) device moments, strips as ehvi_front left them.  Synchronises.
static int ehvi_fold_core(gpx_handle* L, const EhviWs& w, const double* d_mom, int64_t M, const std::vector<double>& strips, int n, int64_t k,
                          double* top_val, int64_t* top_idx, double* d_out) {
    hipStream_t s = L->stream;
    double* const out = d_out ? d_out : w.out;
    {
        Span sp(L, T_COPY);
        // (pageable host memory: the copy has read it before it returns; a and b are adjacent in the walk)
        HIPCHK(L, hipMemcpyAsync(w.a, strips.data(), strips.size() * 8, hipMemcpyHostToDevice, s));
    }
    {
        Span sp(L, T_ACQ);
        launch_ehvi_fold(s, d_mom, M, w.a, n, out);
    }
    return finish_sweep(L, out, M, k, top_val, top_idx);
}

// (arguments checked by ehvi_check)  Each member's plain sweep leaves its moments in HBM -- a live sweep cache is re-seeded exactly as
// gpx_sweep_dev of that member would -- then the fold.  Never pruned: the caller of sweep_core reads mu and s2.
static int ehvi_core(gpx_handle* f1, gpx_handle* f2, const std::vector<double>& strips, int n, const double* dXc, int64_t M, int64_t k,
                     double* top_val, int64_t* top_idx, double* d_out, double* d_mom) {
    gpx_handle* L = f1;
    int rc;
    HIPCHK(L, hipSetDevice(L->device));
    EhviWs w;
    if ((rc = ehvi_layout(L, M, n, w))) return rc;
    double* const mom = d_mom ? d_mom : w.mom;
    gpx_handle* const hs[2] = {f1, f2};
    const Group g = {L, hs, 2, "objective", 1, nullptr};
    for (int j = 0; j < 2; ++j)      // (the fold runs on the lead's stream)
        if ((rc = member_sweep(g, j, GPX_ACQ_MEAN, nullptr, 0, dXc, M, nullptr, mom + (2 * j) * M, mom + (2 * j + 1) * M))) return rc;
    return ehvi_fold_core(L, w, mom, M, strips, n, k, top_val, top_idx, d_out);
}

extern "C" int gpx_ehvi_sweep_dev(gpx_handle* f1, gpx_handle* f2, const double* P, int np, const double* ref, const double* dXc, int64_t M,
                                  int64_t k, double* top_val, int64_t* top_idx, double* d_acq_all, double* d_mom) {
    if (!f1) return GPX_EARG;
    return guarded(f1, [&]() -> int {
        std::vector<double> strips;
        int n = 0;
        if (int rc = ehvi_check(f1, f2, P, np, ref, dXc, M, k, top_val, top_idx, strips, n)) return rc;
        return ehvi_core(f1, f2, strips, n, dXc, M, k, top_val, top_idx, d_acq_all, d_mom);
    });
}

extern "C" int gpx_ehvi_sweep(gpx_handle* f1, gpx_handle* f2, const double* P, int np, const double* ref, const double* Xc, int64_t M, int64_t k,
                              double* top_val, int64_t* top_idx, double* acq_all) {
    if (!f1) return GPX_EARG;
    return guarded(f1, [&]() -> int {
        std::vector<double> strips;
        int n = 0;
        if (int rc = ehvi_check(f1, f2, P, np, ref, Xc, M, k, top_val, top_idx, strips, n)) return rc;
        // (true: the second objective reads the candidates from its own stream)
        return staged_sweep(f1, Xc, M, true, acq_all, nullptr, nullptr, [&](double* dX, double* dacq, double*, double*) {
            return ehvi_core(f1, f2, strips, n, dX, M, k, top_val, top_idx, dacq, nullptr);
        });
    });
}

extern "C" int gpx_ehvi_fold_dev(gpx_handle* lead, const double* d_mom, int64_t M, const double* P, int np, const double* ref, int64_t k,
                                 double* top_val, int64_t* top_idx, double* d_acq_all) {
    if (!lead) return GPX_EARG;
    return guarded(lead, [&]() -> int {
        std::vector<double> strips;
        int n = 0, rc;
        if ((rc = ehvi_front(lead, "ehvi_fold", P, np, ref, strips, n))) return rc;
        if (!d_mom || M < 1) return fail(lead, GPX_EARG, "ehvi_fold: need the moments of M >= 1 candidates");
        if ((rc = check_topk(lead, "ehvi_fold", k, top_val, top_idx))) return rc;
        HIPCHK(lead, hipSetDevice(lead->device));
        EhviWs w;
        if ((rc = ehvi_layout(lead, M, n, w))) return rc;
        return ehvi_fold_core(lead, w, d_mom, M, strips, n, k, top_val, top_idx, d_acq_all);
    });
}

// ---- batch proposals (kernels_batch.hip) --------------------------------------------------------------------------------------------------
// nb greedy picks on the live cache, each conditioned on the earlier ones: at their posterior mean (gpx_sweep_batch), with the pending
// outcomes integrated out over S fantasies (gpx_sweep_batch_fantasy), or by every member of a frozen ensemble at its own posterior mean
// (gpx_ensemble_sweep_batch), or by the objective and every constraint of a constrained index at theirs (gpx_constrained_sweep_batch).
// ONE driver: batch_check, batch_prepare, batch_rounds; an entry keeps its own arguments and what only it needs.
// Per extra pick and member: launch_append_prepare (k(X, x), r = T k, w = U r -- its scalars and flag land in this call's own words and are
// not read: d comes from the CONDITIONED variance), the weight row [w, -1], one rank-1 pass over the cached candidates, then one fold +
// scoring pass for all.  Everything is enqueued on the lead's stream with ONE synchronisation at the end; the picked index never
// leaves the device, so no launch depends on it.  Scratch: every member's h->dbsel (batch_ws); the lead's (n_lead > 0: that many members)
// also holds what they share: taken, the argmax partials, sel_val / sel_idx, the raw x, and behind its V [sel_s2 n nb][descriptors n].
static int batch_layout(gpx_handle* h, int64_t M, int64_t nb, int64_t n_lead, BatchBuf& b) {
    const int64_t xpad = (h->cap_d + 63) / 64 * 64, ld = h->cap_np + NB;      // N + 1 <= ld whatever the padding holds
    const int64_t ndesc = (n_lead * (int64_t)sizeof(BatchMember) + 7) / 8;
    if (int rc = ensure(h, h->dbsel, h->cap_bsel, batch_ws(WsCarver(nullptr), xpad, ld, M, nb, n_lead, ndesc).bytes / 8)) return rc;
    b = batch_ws(WsCarver(h->dbsel), xpad, ld, M, nb, n_lead, ndesc);
    return GPX_OK;
}

// one extra pick's conditioning of member h on the point x (raw) / xs (scaled by h's 1/ell), enqueued on s: row j of V
static void batch_condition(gpx_handle* h, hipStream_t s, const BatchBuf& b, const double* x, const double* Z, int64_t M, int j) {
    launch_append_prepare(h, s, x, b.ks, b.g, b.r, b.tu, 0.0, b.scal_prep, b.flag);
    launch_pend_store(s, b.tu, h->N, b.ld, b.scal, b.row, b.pscal);
    launch_sweep_rank1_v(s, h->dXs, h->N + 1, (int)h->d, b.row, b.ld, b.pscal, Z, M, h->dinvell, h->kernel_id, h->rho, b.xs,
                         b.V + (int64_t)j * M);
}

// member h as the kernels see it: its cached sums and constants, its recurrence in b
static BatchMember batch_member(const gpx_handle* h, const BatchBuf& b) {
    return {h->dcq, h->dcp, h->dinvell, b.qp, b.V, b.cross, b.scal, b.xs, h->rho, h->bias, h->sn2};
}

// one call: the entry's name, its members (g.role: set when refusals name the member), and from batch_check / batch_prepare on M and the scratch
struct BatchCall {
    const char* what;
    Group g;
    int64_t nb, M;
    std::vector<BatchBuf> bufs;
};

// every member holds a live cache, all of one size M >= nb
static int batch_check(BatchCall& c) {
    gpx_handle* L = c.g.L;
    const std::string w(c.what);
    for (int m = 0; m < c.g.n; ++m)
        if (!c.g.hs[m]->fitted || !c.g.hs[m]->cache_valid)
            return fail(L, GPX_ESTATE, ((c.g.role ? group_name(c.g, m) + ": " : std::string()) + w +
                                        ": no live sweep cache (sweep with option sweep_cache = 1 first)").c_str());
    c.M = L->cache_M;
    for (int m = 1; m < c.g.n; ++m)
        if (c.g.hs[m]->cache_M != c.M) return fail(L, GPX_EARG, (w + ": the members' caches differ in size").c_str());
    if (c.nb > c.M) return fail(L, GPX_EARG, (w + ": nb exceeds the number of cached candidates").c_str());
    return GPX_OK;
}

// per member, on its own stream: the inverse, the queued appends (they belong in the sums the picks are scored with), its scratch
static int batch_prepare(BatchCall& c) {
    HIPCHK(c.g.L, hipSetDevice(c.g.L->device));
    c.bufs.assign((size_t)c.g.n, BatchBuf());
    for (int m = 0; m < c.g.n; ++m) {
        gpx_handle* h = c.g.hs[m];
        int rc;
        if ((rc = ensure_inverse(h)) || (rc = flush_pending(h)) || (rc = batch_layout(h, c.M, c.nb, (m == 0 && c.g.role) ? c.g.n : 0, c.bufs[m])))
            return group_fail(c.g, h, m, rc);
    }
    return GPX_OK;
}

// The rounds, on the lead's stream, and the results.  score(j, s2_out) enqueues the scoring pass that folds row j of V (j < 0: round 0;
// s2_out: the variances that score the LAST pick, when asked for), pick(j, last) the pick; unless it was the last, every member is then
// conditioned on the lead's x.  sel_s2: n_s2 words from d_sel_s2; same: the lead's same-grid word (the ensemble); more: what else a form
// brings home (dst NULL: skipped).  The one synchronisation.
struct BatchCopy { void* dst; const void* src; size_t bytes; };
template <class Score, class Pick>
static int batch_rounds(const BatchCall& c, const Score& score, const Pick& pick, double* sel_val, int64_t* sel_idx, double* sel_s2,
                        const double* d_sel_s2, int64_t n_s2, double* s2_all, int* same = nullptr, std::initializer_list<BatchCopy> more = {}) {
    gpx_handle* L = c.g.L;
    const BatchBuf& lb = c.bufs[0];
    hipStream_t s = L->stream;
    {
        Span sp(L, T_BATCH);
        HIPCHK(L, hipMemsetAsync(lb.taken, 0, (size_t)lb.ntaken * 8, s));
        for (const BatchBuf& b : c.bufs) HIPCHK(L, hipMemsetAsync(b.flag, 0, sizeof(int), s));
        for (int j = 0; j < (int)c.nb; ++j) {
            const bool last = j == (int)c.nb - 1;
            score(j - 1, (s2_all && last) ? lb.s2 : nullptr);
            pick(j, last);
            if (last) break;
            for (int m = 0; m < c.g.n; ++m) batch_condition(c.g.hs[m], s, c.bufs[m], lb.x, L->dcZ, c.M, j);
        }
        HIPCHK(L, hipGetLastError());
    }
    HIPCHK(L, hipMemcpyAsync(sel_val, lb.sel_val, (size_t)c.nb * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(L, hipMemcpyAsync(sel_idx, lb.sel_idx, (size_t)c.nb * 8, hipMemcpyDeviceToHost, s));
    if (sel_s2) HIPCHK(L, hipMemcpyAsync(sel_s2, d_sel_s2, (size_t)n_s2 * 8, hipMemcpyDeviceToHost, s));
    if (s2_all) HIPCHK(L, hipMemcpyAsync(s2_all, lb.s2, (size_t)c.M * 8, hipMemcpyDeviceToHost, s));
    if (same) HIPCHK(L, hipMemcpyAsync(same, lb.same, sizeof(int), hipMemcpyDeviceToHost, s));
    for (const BatchCopy& m : more)
        if (m.dst) HIPCHK(L, hipMemcpyAsync(m.dst, m.src, m.bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(L, hipStreamSynchronize(s));
    return GPX_OK;
}

// the rounds of the single-model forms.  f: the fantasised form's arguments on the device (moving: every fantasy's incumbent follows its
// own observations), NULL: the believer's
static int single_rounds(const BatchCall& c, int acq_id, double p0, const FantArg* f, bool moving, double* sel_val, int64_t* sel_idx,
                         double* sel_s2, double* s2_all) {
    gpx_handle* h = c.g.L;
    const BatchBuf& b = c.bufs[0];
    const BatchMember e = batch_member(h, b);
    hipStream_t s = h->stream;
    return batch_rounds(c, [&](int j, double* s2_out) { launch_batch_score(s, j, c.M, e, b, acq_id, p0, f, s2_out); },
                        [&](int j, bool last) { launch_batch_pick(s, j, c.M, (int)h->d, h->dcZ, e, b, f, moving && !last); },
                        sel_val, sel_idx, sel_s2, b.sel_s2, c.nb, s2_all);
}

// The rounds of the forms whose kernels read a table of the members in device memory (the ensemble, the constrained index, two objectives).
// The members' streams are drained; from there on everything runs on the lead's: the table goes up, every member's candidates are compared
// with the lead's (k_ens_same_grid), score(s, j, table, lead's scratch) enqueues a round's scoring pass, pick(s, j, last, table, lead's
// scratch) its pick.  sel_s2: (n, nb) member-major; more: batch_rounds'.
template <class Score, class Pick>
static int table_rounds(const BatchCall& c, const Score& score, const Pick& pick, double* sel_val, int64_t* sel_idx, double* sel_s2,
                        std::initializer_list<BatchCopy> more = {}) {
    gpx_handle* L = c.g.L;
    const int n = c.g.n;
    const int64_t M = c.M, d = L->d;
    L->bsel_desc.resize((size_t)n);
    for (int m = 0; m < n; ++m) {
        HIPCHK(L, hipStreamSynchronize(c.g.hs[m]->stream));
        L->bsel_desc[m] = batch_member(c.g.hs[m], c.bufs[m]);
    }
    const BatchBuf& lb = c.bufs[0];
    BatchMember* ddesc = reinterpret_cast<BatchMember*>(lb.desc);
    hipStream_t s = L->stream;
    int differ = 0;
    {
        Span sp(L, T_BATCH);
        HIPCHK(L, hipMemcpyAsync(ddesc, L->bsel_desc.data(), (size_t)n * sizeof(BatchMember), hipMemcpyHostToDevice, s));
        HIPCHK(L, hipMemsetAsync(lb.same, 0, sizeof(int), s));
        for (int m = 1; m < n; ++m) launch_ens_same_grid(s, L->dcZ, c.g.hs[m]->dcZ, M * d, lb.same);
    }
    if (int rc = batch_rounds(c, [&](int j, double*) { score(s, j, ddesc, lb); }, [&](int j, bool last) { pick(s, j, last, ddesc, lb); },
                              sel_val, sel_idx, sel_s2, lb.ens_s2, n * c.nb, nullptr, &differ, more))
        return rc;
    if (differ) return fail(L, GPX_EARG, (std::string(c.what) + ": the members' caches hold different candidates").c_str());
    return GPX_OK;
}
// .. with the pick the ensemble and the constrained index share (k_ens_batch_pick)
template <class Score>
static int table_rounds(const BatchCall& c, const Score& score, double* sel_val, int64_t* sel_idx, double* sel_s2) {
    return table_rounds(c, score, [&](hipStream_t s, int j, bool, const BatchMember* mem, const BatchBuf& lb) {
        launch_ens_batch_pick(s, j, c.g.n, c.nb, c.M, (int)c.g.L->d, c.g.L->dcZ, mem, lb);
    }, sel_val, sel_idx, sel_s2, {});
}

extern "C" int gpx_sweep_batch(gpx_handle* h, int acq_id, const double* params, int nparams, int64_t nb, double* sel_val,
                               int64_t* sel_idx, double* sel_s2, double* s2_all) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        int rc;
        BatchCall c = {"sweep_batch", {h, &h, 1, nullptr, 0, nullptr}, nb, 0, {}};
        if ((rc = check_batch(h, c.what, acq_id, params, nparams, nb, sel_val, sel_idx)) || (rc = batch_check(c)) || (rc = batch_prepare(c)))
            return rc;
        return single_rounds(c, acq_id, params[0], nullptr, false, sel_val, sel_idx, sel_s2, s2_all);
    });
}

// gpx_sweep_batch with the pending outcomes integrated out over S joint fantasies (kernels_batch.hip: k_fant_score, k_fant_pick).  The
// innovations (re-packed pick-major, zero-padded to the kernel's chunk), the incumbents and the forced rows go up once into h->dfant
// (fant_ws) before the first round.
extern "C" int gpx_sweep_batch_fantasy(gpx_handle* h, int acq_id, const double* params, int nparams, int64_t nb, const double* eps,
                                       int64_t S, int64_t ld_eps, int incumbent, const int64_t* pend_idx, int64_t npend,
                                       double* sel_val, int64_t* sel_idx, double* sel_s2, double* s2_all) {
    return guarded(h, [&]() -> int {
        if (!h) return GPX_EARG;
        int rc;
        BatchCall c = {"sweep_batch_fantasy", {h, &h, 1, nullptr, 0, nullptr}, nb, 0, {}};
        if ((rc = check_batch(h, c.what, acq_id, params, nparams, nb, sel_val, sel_idx))) return rc;
        if (acq_id != GPX_ACQ_EI && acq_id != GPX_ACQ_PI)
            return fail(h, GPX_EARG, "sweep_batch_fantasy: EI or PI (UCB is linear in the mean: its fantasy average is gpx_sweep_batch's value)");
        if (S < 1 || S > FANT_MAX_S) return fail(h, GPX_EARG, "sweep_batch_fantasy: S must be in [1, 64]");
        if (incumbent != 0 && incumbent != 1) return fail(h, GPX_EARG, "sweep_batch_fantasy: incumbent must be 0 or 1");
        if (!eps || ld_eps < std::max<int64_t>(nb - 1, 1)) return fail(h, GPX_EARG, "sweep_batch_fantasy: eps is (S, ld_eps >= max(nb - 1, 1))");
        if (npend < 0 || npend >= nb || (npend > 0 && !pend_idx)) return fail(h, GPX_EARG, "sweep_batch_fantasy: npend must be in [0, nb)");
        if ((rc = batch_check(c))) return rc;
        for (int64_t i = 0; i < npend; ++i) {
            bool ok = pend_idx[i] >= 0 && pend_idx[i] < c.M;
            for (int64_t k = 0; ok && k < i; ++k) ok = pend_idx[k] != pend_idx[i];
            if (!ok) return fail(h, GPX_EARG, "sweep_batch_fantasy: pend_idx must hold distinct rows of the cache");
        }
        const FantWs lay = fant_ws(WsCarver(nullptr), nb, S);
        const int64_t Sp = lay.Sp;
        h->fant_host.assign((size_t)lay.bytes, 0);
        {
            const FantWs hw = fant_ws(WsCarver(h->fant_host.data()), nb, S);
            for (int64_t s = 0; s < S; ++s)
                for (int64_t l = 0; l + 1 < nb; ++l) {
                    const double e = eps[s * ld_eps + l];
                    if (!std::isfinite(e)) return fail(h, GPX_EARG, "sweep_batch_fantasy: eps must be finite");
                    hw.eps[l * Sp + s] = e;
                }
            for (int64_t s = 0; s < Sp; ++s) hw.t[s] = params[0];
            for (int64_t i = 0; i < npend; ++i) hw.pend[i] = pend_idx[i];
        }
        if ((rc = batch_prepare(c)) || (rc = ensure(h, h->dfant, h->cap_fant, lay.bytes / 8))) return rc;
        const FantWs w = fant_ws(WsCarver(h->dfant), nb, S);
        {
            Span sp(h, T_COPY);
            HIPCHK(h, hipMemcpyAsync(w.eps, h->fant_host.data(), (size_t)lay.bytes, hipMemcpyHostToDevice, h->stream));
        }
        const FantArg f = {w.eps, w.t, w.pend, (int)S, (int)Sp, (int)npend};
        return single_rounds(c, acq_id, params[0], &f, incumbent != 0, sel_val, sel_idx, sel_s2, s2_all);
    });
}

// The ensemble: the members frozen, every round scored with ensemble_core's rule.  The members' streams are drained on entry; from there
// on everything runs on the lead's stream.
extern "C" int gpx_ensemble_sweep_batch(gpx_handle* const* members, int n_members, int acq_id, const double* params,
                                        int nparams, int64_t nb, double* sel_val, int64_t* sel_idx, double* sel_s2) {
    if (members && members[0] && (n_members < 1 || n_members > 64)) {
        members[0]->err = "ensemble_sweep_batch: n_members must be in [1, 64]";
        return GPX_EARG;
    }
    if (ensemble_check(members, n_members)) return GPX_EARG;
    gpx_handle* L = members[0];
    return guarded(L, [&]() -> int {
        const int n = n_members;
        BatchCall c = {"ensemble_sweep_batch", {L, members, n, "ensemble member", 0, nullptr}, nb, 0, {}};
        int rc;
        if ((rc = check_batch(L, c.what, acq_id, params, nparams, nb, sel_val, sel_idx))) return rc;
        if ((rc = group_check(c.g, c.what, {{G_FITTED, "a member model is not fitted"},
                                            {G_SHAPE, "members must share the device and the input dimension"},
                                            {G_ONCE, "a handle is listed twice (every member needs its own scratch)"}}, true)))
            return rc;
        if ((rc = batch_check(c)) || (rc = batch_prepare(c))) return rc;
        const double p0 = params[0];
        return table_rounds(c, [&](hipStream_t s, int j, const BatchMember* mem, const BatchBuf& lb) {
            launch_ens_batch_score(s, j, n, c.M, mem, lb, acq_id, p0);
        }, sel_val, sel_idx, sel_s2);
    });
}

// The constrained index in batches: the members are the objective (where there is one) and the constraints in the
// caller's order, target and thresholds frozen, every member conditioned on a pick at its own posterior mean.  The refusals are those of
// gpx_constrained_sweep and gpx_ensemble_sweep_batch, the rounds the ensemble's with k_con_batch_score as the scoring pass.
static_assert(sizeof(ConBatchArg::thr) == CON_MAX * sizeof(double), "ConBatchArg holds CON_MAX thresholds");
extern "C" int gpx_constrained_sweep_batch(gpx_handle* obj, gpx_handle* const* cons, int nc, const double* thr, int acq_id, const double* params,
                                           int nparams, int64_t nb, double* sel_val, int64_t* sel_idx, double* sel_s2) {
    gpx_handle* L = con_lead(obj, cons, nc);
    if (!L) return GPX_EARG;
    return guarded(L, [&]() -> int {
        const char* what = "constrained_sweep_batch";
        int rc;
        if ((rc = constrained_check_args(L, what, obj, cons, nc, thr, acq_id, params, nparams))) return rc;
        // (without an objective acq_id and params are not read: the batch's own arguments are checked beside a constraint's PI)
        if ((rc = obj ? check_batch(L, what, acq_id, params, nparams, nb, sel_val, sel_idx) : check_batch(L, what, GPX_ACQ_PI, thr, 1, nb, sel_val, sel_idx)))
            return rc;
        if ((rc = constrained_check_handles(L, what, obj, cons, nc))) return rc;
        std::vector<gpx_handle*> hs;
        if (obj) hs.push_back(obj);
        hs.insert(hs.end(), cons, cons + nc);
        const int n = (int)hs.size();
        BatchCall c = {what, {L, hs.data(), n, "constraint", obj ? -1 : 0, nullptr}, nb, 0, {}};
        if ((rc = batch_check(c)) || (rc = batch_prepare(c))) return rc;
        ConBatchArg a = {};
        std::copy(thr, thr + nc, a.thr);
        a.target = obj ? params[0] : 0.0;
        a.acq_id = obj ? acq_id : GPX_ACQ_PI;
        a.has_obj = obj ? 1 : 0;
        return table_rounds(c, [&](hipStream_t s, int j, const BatchMember* mem, const BatchBuf& lb) {
            launch_con_batch_score(s, j, n, c.M, mem, lb, a);
        }, sel_val, sel_idx, sel_s2);
    });
}

// Two objectives in batches: both members and the reference point frozen, every round scored by EHVI over the front
// AS IT STANDS, and -- what no other form needs -- the front follows the picks: a pick's believed outcome (the members' own posterior means
// there) is taken into the strips on the device by the pick kernel (ehvi_insert), so the strips go up once, at their capacity, into the
// lead's h->dehvib (ehvi_batch_ws) and the size of the front is a device word the scoring pass reads.  A front of n points may grow to
// n + nb - 1 before the last round: beyond EHVI_MAX_FRONT the call is refused.  The refusals are those of gpx_ehvi_sweep and
// gpx_ensemble_sweep_batch, the rounds table_rounds' with this form's two kernels.
extern "C" int gpx_ehvi_sweep_batch(gpx_handle* f1, gpx_handle* f2, const double* P, int np, const double* ref, int64_t nb, double* sel_val,
                                    int64_t* sel_idx, double* sel_s2, double* sel_y, int64_t* sel_nfront) {
    if (!f1) return GPX_EARG;
    return guarded(f1, [&]() -> int {
        const char* what = "ehvi_sweep_batch";
        gpx_handle* L = f1;
        gpx_handle* const hs[2] = {f1, f2};
        BatchCall c = {what, {L, hs, 2, "objective", 1, nullptr}, nb, 0, {}};
        std::vector<double> strips;
        int n = 0, rc;
        if ((rc = group_check(c.g, what, {{G_NOT_NULL, "NULL handle"}, {G_ONCE, "the two objectives need a handle each"}}))) return rc;
        if ((rc = ehvi_front(L, what, P, np, ref, strips, n))) return rc;
        if ((rc = check_batch(L, what, GPX_ACQ_EI, ref, 1, nb, sel_val, sel_idx))) return rc;      // (nb and the outputs: every EI here is over a strip's edge)
        if (n + nb - 1 > EHVI_MAX_FRONT)
            return fail(L, GPX_EARG, (std::string(what) + ": the front may grow by a point per pick: n + nb - 1 must not exceed 1024").c_str());
        if ((rc = group_check(c.g, what, {{G_FITTED, "an objective's model is not fitted"}, {G_SHAPE, "the handles must share the device and the input dimension"}})))
            return rc;
        if ((rc = batch_check(c)) || (rc = batch_prepare(c))) return rc;
        if ((rc = ensure(L, L->dehvib, L->cap_ehvib, ehvi_batch_ws(WsCarver(nullptr), EHVI_STRIP_LD).bytes / 8))) return rc;
        const EhviBatchWs w = ehvi_batch_ws(WsCarver(L->dehvib), EHVI_STRIP_LD);
        // ehvi_front's strips (a then b, n + 2 each) at the device's pitch; the words behind them are never read before they are written
        std::vector<double> up((size_t)2 * EHVI_STRIP_LD, 0.0);
        std::copy(strips.begin(), strips.begin() + n + 2, up.begin());
        std::copy(strips.begin() + n + 2, strips.end(), up.begin() + EHVI_STRIP_LD);
        {
            Span sp(L, T_COPY);
            // (pageable host memory: each copy has read it before it returns; a and b are adjacent in the walk)
            HIPCHK(L, hipMemcpyAsync(w.a, up.data(), up.size() * 8, hipMemcpyHostToDevice, L->stream));
            HIPCHK(L, hipMemcpyAsync(w.n, &n, sizeof(int), hipMemcpyHostToDevice, L->stream));
        }
        return table_rounds(c, [&](hipStream_t s, int j, const BatchMember* mem, const BatchBuf& lb) { launch_ehvi_batch_score(s, j, c.M, mem, lb, w); },
                            [&](hipStream_t s, int j, bool last, const BatchMember* mem, const BatchBuf& lb) {
                                launch_ehvi_batch_pick(s, j, nb, c.M, (int)L->d, L->dcZ, mem, lb, w, last);
                            }, sel_val, sel_idx, sel_s2,
                            {{sel_y, w.y, (size_t)nb * 16}, {sel_nfront, w.nfront, (size_t)nb * 8}});
    });
}

extern "C" int gpx_ensemble_prune_report(gpx_handle* const* members, int n_members, double* scal, int nscal, double* ub,
                                         int64_t* idx, int64_t cap_idx) {
    if (ensemble_check(members, n_members)) return GPX_EARG;
    gpx_handle* h = members[0];
    return guarded(h, [&]() -> int {
        const gpx_handle::EnsPruneRecord& r = h->ens_rec;
        double head[8];
        if (int rc = report_begin(h, "ensemble_prune_report", "ensemble sweep", " of these members", r, r.n == n_members, scal, nscal, ub || idx, nullptr, head))
            return rc;
        std::vector<double> out((size_t)(11 + 2 * n_members), NAN);      // (behind gate_hint: the members' bound_fact)
        std::copy(head, head + 8, out.begin());
        out[10 + n_members] = r.hinted ? 1.0 : 0.0;      // behind the deltas: head[8] is tau, and callers built against 10 + n read on as before
        out[9] = r.gate;
        if (r.path >= 2) {
            HIPCHK(h, hipMemcpy(&out[8], r.sc + 5, 8, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(&out[10], r.delta, (size_t)n_members * 8, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(&out[11 + n_members], r.delta + n_members, (size_t)n_members * 8, hipMemcpyDeviceToHost));
        }
        for (int i = 0; i < nscal && i < 11 + 2 * n_members; ++i) scal[i] = out[i];
        return report_vectors(h, r, ub, idx, cap_idx);
    });
}

// ---- candidate grids resident in HBM (pybo/solvers/lbfgs.py:45; pybo/inits/methods.py) -------------------
struct gpx_grid {
    int device = 0;
    int64_t M = 0, d = 0;
    double* dX = nullptr;
    hipStream_t s = nullptr;        // the grid's own (non-blocking) stream: nothing in this library touches the NULL stream -- its
                                    // first use in a process halves the speed of multi-stream schedules (see gpx_create)
};

#define GRIDCHK(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            g_create_err = std::string(#call) + " failed: " + hipGetErrorString(e_);               \
            return (e_ == hipErrorOutOfMemory) ? GPX_EOOM : GPX_EHIP;                              \
        }                                                                                          \
    } while (0)

static int grid_create_impl(int device, int kind, const double* bounds, int64_t M, int64_t d, uint64_t seed,
                            int64_t first, const uint32_t* sv, int bits, gpx_grid** out) {
    if (!out) return GPX_EARG;
    *out = nullptr;
    if (!bounds || M < 1 || d < 1 || d > DMAX) { g_create_err = "grid_create: bad sizes or NULL bounds"; return GPX_EARG; }
    if (kind != GPX_GRID_UNIFORM && kind != GPX_GRID_SOBOL) { g_create_err = "grid_create: unknown grid kind"; return GPX_EARG; }
    if (first < 0) { g_create_err = "grid_create: first must be >= 0"; return GPX_EARG; }
    if (kind == GPX_GRID_SOBOL && (!sv || bits < 1 || bits > 32 || first < 0 ||
                                   (bits < 63 && (uint64_t)(first + M) > (1ull << bits)))) {
        g_create_err = "grid_create: Sobol needs direction numbers (d, bits), 1 <= bits <= 32, first + M <= 2^bits";
        return GPX_EARG;
    }
    GRIDCHK(hipSetDevice(device));
    gpx_grid* g = new gpx_grid();
    g->device = device; g->M = M; g->d = d;
    double* dB = nullptr;
    uint32_t* dsv = nullptr;
    auto cleanup = [&]() { if (dB) hipFree(dB); if (dsv) hipFree(dsv); };
    auto bail = [&](int rc) { cleanup(); if (g->dX) hipFree(g->dX); if (g->s) hipStreamDestroy(g->s); delete g; return rc; };
#define GRIDTRY(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            g_create_err = std::string(#call) + " failed: " + hipGetErrorString(e_);               \
            return bail((e_ == hipErrorOutOfMemory) ? GPX_EOOM : GPX_EHIP);                        \
        }                                                                                          \
    } while (0)
    GRIDTRY(hipStreamCreateWithFlags(&g->s, hipStreamNonBlocking));
    GRIDTRY(hipMalloc((void**)&g->dX, (size_t)M * d * 8));
    GRIDTRY(hipMalloc((void**)&dB, (size_t)d * 2 * 8));
    GRIDTRY(hipMemcpyAsync(dB, bounds, (size_t)d * 2 * 8, hipMemcpyHostToDevice, g->s));
    if (kind == GPX_GRID_SOBOL) {
        GRIDTRY(hipMalloc((void**)&dsv, (size_t)d * bits * 4));
        GRIDTRY(hipMemcpyAsync(dsv, sv, (size_t)d * bits * 4, hipMemcpyHostToDevice, g->s));
        launch_grid_sobol(g->s, dsv, bits, first, M, (int)d, dB, g->dX);
    } else {
        launch_grid_uniform(g->s, seed, first, M, (int)d, dB, g->dX);
    }
    GRIDTRY(hipGetLastError());
    GRIDTRY(hipStreamSynchronize(g->s));             // the grid is complete when this call returns: any stream may read it
    cleanup();
    *out = g;
    return GPX_OK;
}

extern "C" int gpx_grid_create(int device, int kind, const double* bounds, int64_t M, int64_t d, uint64_t seed,
                               int64_t first, const uint32_t* sv, int bits, gpx_grid** out) {
    try {
        return grid_create_impl(device, kind, bounds, M, d, seed, first, sv, bits, out);
    } catch (...) {
        if (out) *out = nullptr;
        return GPX_EOOM;
    }
}

extern "C" const double* gpx_grid_data(const gpx_grid* g) { return g ? g->dX : nullptr; }

extern "C" int gpx_grid_rows(gpx_grid* g, const int64_t* idx, int64_t k, double* out) {
    try {
        if (!g || !out) { g_create_err = "grid_rows: NULL pointer"; return GPX_EARG; }
        GRIDCHK(hipSetDevice(g->device));
        if (!idx) {                                   // the whole grid
            GRIDCHK(hipMemcpyAsync(out, g->dX, (size_t)g->M * g->d * 8, hipMemcpyDeviceToHost, g->s));
            GRIDCHK(hipStreamSynchronize(g->s));
            return GPX_OK;
        }
        if (k < 1) return GPX_OK;
        for (int64_t i = 0; i < k; ++i)
            if (idx[i] < 0 || idx[i] >= g->M) { g_create_err = "grid_rows: index out of range"; return GPX_EARG; }
        for (int64_t i = 0; i < k;) {                 // one copy per run of consecutive rows
            int64_t j = i + 1;
            while (j < k && idx[j] == idx[j - 1] + 1) ++j;
            GRIDCHK(hipMemcpyAsync(out + i * g->d, g->dX + idx[i] * g->d, (size_t)(j - i) * g->d * 8, hipMemcpyDeviceToHost, g->s));
            i = j;
        }
        GRIDCHK(hipStreamSynchronize(g->s));
        return GPX_OK;
    } catch (...) {
        return GPX_EOOM;
    }
}

extern "C" int gpx_grid_destroy(gpx_grid* g) {
    if (!g) return GPX_OK;
    hipSetDevice(g->device);
    if (g->dX) hipFree(g->dX);
    if (g->s) hipStreamDestroy(g->s);
    delete g;
    return GPX_OK;
}

// bssm_api.hip -- C-ABI implementation (include/bayesssm_amd.h) over the kernels.
//
// Host-side sequencing of the reference's loops:
//   bssm_pf_run      = .particle_filter_core's T-loop       R/particle_filter_core.R:123-246
//   bssm_pmmh_chain  = chain_result's MH loop               R/pmmh.R:403-415,422-500
// One context = one GPU + one stream; device memory is owned by the context.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>
#include <algorithm>
#include "kernels.hip.h"
#include "fused.hip.h"
#include "mv.hip.h"
#include "rnet.hip.h"
#include "multi.hip.h"
#include "smooth.hip.h"
#include <atomic>
#include "../../include/bayesssm_amd.h"

using namespace bssm;

static thread_local std::string g_err;

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess) {                                                          \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e__);                   \
            return BSSM_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

#define ARGFAIL(msg) do { g_err = (msg); return BSSM_ERR_ARG; } while (0)

struct ProfEntry { double ms = 0; long long launches = 0; };
// bssm_pf_run_smooth in flight on a context: what the caller's own cfg asked to have copied to the host, K, and where the trace's outputs go
struct SmoothReq { int host_particles, host_ancestors, K; bssm_smooth_result* out; };

struct bssm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    long long cap = 0;          // particles
    int max_dim = 1;
    int maxB = 0;
    // particle state
    double *x0 = nullptr, *x1 = nullptr, *lw = nullptr, *w = nullptr, *auxlw = nullptr, *auxg = nullptr, *cum = nullptr;
    // scan workspace
    double *pm = nullptr, *ps = nullptr, *pq = nullptr, *bsum = nullptr, *bsq = nullptr, *ain_w = nullptr, *ain_p = nullptr;
    BlockRec *brec = nullptr, *brec_p = nullptr;      // block records of the sum(w) pass / of the cumsum(w / total) pass
    SideList *side = nullptr, *side_p = nullptr;
    uint64_t* cin = nullptr;
    DevState* st = nullptr;
    unsigned long long* gmax_cur = nullptr;   // slot of the grid-wide max(log-weights) of the weight evaluation in flight
    int sh_boff = 0, sh_nloc = 0;  // particle-block sharding (bssm_pf_run_sharded): this rank's first block / block count; 0 = whole grid
    // per-context options (bssm_ctx_set_option): test aids and A/B switches -- no process-global state
    int opt_window = 0;            // > 0: override the validity window of the scan records (ulps); a tiny window drives the literal fallbacks
    int opt_batch_lit_max = 384;   // largest N that takes the in-order exact sums in k_pf_batch
    int opt_stage = 1;             // LDS staging of k_apply's particle stores
    int opt_inkernel_resolve = 1;  // grids of <= 2 NT blocks: resolve inside the consuming kernels instead of k_resolve launches
    int opt_renormalize = 1;       // filters: 1 = the resampler divides the normalised weights by their exact sum again (src/resampling.cpp:24,51),
                                   // 0 = that division (by 1 +- a few 1e-14) is folded away: one exact pass instead of two
    int opt_recompute_lw = 1;      // bootstrap filters on the Gaussian-observation models: log-weights re-evaluated in k_weights instead of stored by k_step
    int opt_fuse_step = 0;         // SISR bootstrap filters: the next observation's transition + weight inside the expansion kernel
                                   // (off: measured slower -- 7 generator pairs per lane at 2 waves per SIMD cost the expansion kernel 7.7 us,
                                   //  the k_step launch they replace costs 11.2 us but the per-block partials still need a 5.4 us launch)
    int opt_debug_stop = 0;        // DEV builds: stage stamps (99 typical block, 98 head block, 97 batched kernel)
    int opt_fused_prefetch = 0;    // fused path: the next observation's transition normals are drawn while the workgroups wait for the resolver
    int opt_fused_early_max = 1;   // fused path: the global max of the log-weights is broadcast ahead of the sum, the workers' exp runs in the wait for the sum
    int opt_force_fallback = 0;    // test aid: the resolvers take their exact fallbacks (FF_* bits; mirrored in DevState::force_fallback, FusedArgs)
    int opt_mv_y_missing = 0;      // multivariate family: 1 = a NaN in y is a component that was not observed (mv.hip.h, mv_observed); 0 = refused
    int opt_rn_leaps = 0;          // reaction networks: K >= 1 = the transition is K tau-leaps per unit of time (rnet.hip.h); 0 = Gillespie's direct method
    int opt_rn_noise = 0;          // reaction networks: 1 = the Euler-multinomial leaps (opt_rn_method = 1) draw gamma white noise on the rates and the block carries lead[R], sigma[R] (rnet.hip.h)
    int opt_rn_method = 0;         // reaction networks: 0 = opt_rn_leaps decides (0 Gillespie, K tau-leaping); 1 = Euler-multinomial leaps, opt_rn_leaps = K >= 1 of them
    int opt_fused = 1;             // bootstrap filters on the scalar Gaussian-observation models, N <= 2^20: one launch per observation (fused.hip.h)
    // fused path: workspace of the tagged records, launch counter (the tags), what happened
    FusedWs* fz = nullptr; uint32_t fz_tag = 0; bool fz_ok = false;
    long long fz_launches = 0, fz_runs = 0, fz_bails = 0, fz_timeouts = 0;
    long long multi_lockstep = 0, multi_sequential = 0;      // bssm_pf_run_multi calls with this context as ctxs[0]: lock-step kernels / one filter after the other
    // growable buffers
    std::map<std::string, std::pair<void*, size_t>> pool;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void* h_stage = nullptr; size_t h_stage_bytes = 0;      // pinned host staging (batched filters: one upload, one download)
    // profiling
    bool profile = false;
    std::map<std::string, ProfEntry> prof;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    int last_device_status = 0;
    const SmoothReq* smooth = nullptr;     // set for the span of a bssm_pf_run_smooth call: the run keeps its histories for the trace (smooth.hip.h)
};

// One fused run at a time per device (in this process): all workgroups of a fused launch must be resident together, and two
// such launches from two contexts could each hold half of the chip.  A run that does not get the token takes the multi-launch path.
static std::atomic<int> g_fused_busy[64];
// ... and a fused launch fills every residency slot of the chip, which starves the kernels of other contexts running at the same
// time (measured: two / four filter runs in flight 20.0 / 26.3 G particle-steps/s with one of them fused against 29.8 / 33 G all
// multi-launch).  So: runs in flight per device are counted, and after any overlap the next FZ_QUIET runs of the device stay multi-launch.
static std::atomic<int> g_runs_active[64];
static std::atomic<long long> g_run_serial[64], g_last_overlap[64];
static std::atomic<long long> g_fused_hold[64], g_fused_span[64];       // back-off after a time-out: no fused run before serial `hold`; `span` doubles while they keep coming
constexpr long long FZ_QUIET = 16;

static int pool_get(bssm_ctx* c, const char* name, size_t bytes, void** out)
{
    auto& e = c->pool[name];
    if (e.second < bytes) {
        if (e.first) HIPCHK(hipFree(e.first));
        e.first = nullptr; e.second = 0;
        const size_t want = bytes + bytes / 4 + 256;
        HIPCHK(hipMalloc(&e.first, want));
        e.second = want;
    }
    *out = e.first;
    return BSSM_OK;
}
template <class P>
static int pool_get(bssm_ctx* c, const char* name, size_t bytes, P** out) { void* v = nullptr; const int rc = pool_get(c, name, bytes, &v); *out = (P*)v; return rc; }
// a pool buffer that holds a copy of a host array (the copy is asynchronous: src stays alive until the stream has been synchronised)
template <class P>
static int pool_put(bssm_ctx* c, const char* name, const void* src, size_t bytes, P** out)
{
    if (int rc = pool_get(c, name, bytes, out)) return rc;
    HIPCHK(hipMemcpyAsync((void*)*out, src, bytes, hipMemcpyHostToDevice, c->stream));
    return BSSM_OK;
}

static int host_stage(bssm_ctx* c, size_t bytes)
{
    if (c->h_stage_bytes >= bytes) return BSSM_OK;
    if (c->h_stage) HIPCHK(hipHostFree(c->h_stage));
    c->h_stage = nullptr; c->h_stage_bytes = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    HIPCHK(hipHostMalloc(&c->h_stage, want, hipHostMallocDefault));
    c->h_stage_bytes = want;
    return BSSM_OK;
}

extern "C" const char* bssm_last_error(void) { return g_err.c_str(); }

extern "C" const char* bssm_status_string(int status)
{
    switch (status) {
        case BSSM_OK: return "ok";
        case BSSM_ERR_NEGATIVE_WEIGHT: return "Weights must be non-negative";
        case BSSM_ERR_ZERO_SUM: return "Sum of weights must be greater than 0";
        case BSSM_ERR_LENGTH: return "Number of particles must match the length of weights";
        case BSSM_ERR_ARG: return "invalid argument";
        case BSSM_ERR_HIP: return "HIP runtime error";
        case BSSM_ERR_CAPACITY: return "problem exceeds context capacity";
        default: return "unknown status";
    }
}

extern "C" int bssm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int bssm_ctx_create(int device, long long max_particles, int max_dim, bssm_ctx** out)
{
    if (!out) ARGFAIL("bssm_ctx_create: out is NULL");
    *out = nullptr;
    if (max_particles <= 0) ARGFAIL("bssm_ctx_create: max_particles must be positive");
    if (max_dim < 1 || max_dim > MVD) ARGFAIL("bssm_ctx_create: max_dim must be 1 .. 8");
    const long long B = (max_particles + EB - 1) / EB;
    if (B > MAXB) { g_err = "bssm_ctx_create: max_particles exceeds 2^22 (scan workspace limit of this build)"; return BSSM_ERR_CAPACITY; }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) { g_err = "no HIP device visible: this library has no CPU path"; return BSSM_ERR_HIP; }
    if (device < 0 || device >= ndev) ARGFAIL("bssm_ctx_create: device index out of range");
    HIPCHK(hipSetDevice(device));
    bssm_ctx* c = new bssm_ctx();
    c->device = device; c->cap = max_particles; c->max_dim = max_dim; c->maxB = (int)B;
    const size_t npad = (size_t)B * EB;
    hipError_t e = hipSuccess;
    // zero-fill ON THE CONTEXT'S STREAM: the stream is non-blocking, so a hipMemset on the null stream is not ordered with the
    // context's first kernels and could land after them (seen once as wrong weights in the first call of a fresh 2^20 context)
    auto A = [&](void** p, size_t bytes) { if (e == hipSuccess) { e = hipMalloc(p, bytes); if (e == hipSuccess) e = hipMemsetAsync(*p, 0, bytes, c->stream); } };
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    A((void**)&c->x0, npad * 8 * max_dim); A((void**)&c->x1, npad * 8 * max_dim);
    A((void**)&c->lw, npad * 8); A((void**)&c->w, npad * 8); A((void**)&c->auxlw, npad * 8); A((void**)&c->auxg, npad * 8);
    A((void**)&c->cum, npad * 8);
    A((void**)&c->pm, MAXB * 8); A((void**)&c->ps, MAXB * 8); A((void**)&c->pq, MAXB * 8); A((void**)&c->bsum, MAXB * 8); A((void**)&c->bsq, MAXB * 8);
    A((void**)&c->ain_w, MAXB * 8); A((void**)&c->ain_p, MAXB * 8);
    A((void**)&c->brec, MAXB * sizeof(BlockRec)); A((void**)&c->brec_p, MAXB * sizeof(BlockRec)); A((void**)&c->cin, MAXB * 8);
    A((void**)&c->side, (size_t)B * sizeof(SideList)); A((void**)&c->side_p, (size_t)B * sizeof(SideList));
    A((void**)&c->st, sizeof(DevState));
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_resolve<MODE_W>), hipFuncAttributeMaxDynamicSharedMemorySize, MAXB * (int)sizeof(BlockRec));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_resolve<MODE_P>), hipFuncAttributeMaxDynamicSharedMemorySize, MAXB * (int)sizeof(BlockRec));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply<0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply<0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    for (const void* fnp : {reinterpret_cast<const void*>(&k_apply<0, true, true>), reinterpret_cast<const void*>(&k_apply<0, false, true>),
                            reinterpret_cast<const void*>(&k_apply<1, true, true>), reinterpret_cast<const void*>(&k_apply<1, false, true>)})
        if (e == hipSuccess) e = hipFuncSetAttribute(fnp, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    static_assert(sizeof(ResolveSmem) <= 3 * CAPX * sizeof(double), "the in-kernel resolve borrows k_apply's staging area");
    for (const void* fnp : {reinterpret_cast<const void*>(&k_apply_multi<0>), reinterpret_cast<const void*>(&k_apply_multi<1>)})
        if (e == hipSuccess) e = hipFuncSetAttribute(fnp, hipFuncAttributeMaxDynamicSharedMemorySize, 3 * CAPX * (int)sizeof(double));
    if (e == hipSuccess) {
        // fused path: workspace (zeroed once: the tags only grow), dynamic LDS, and the residency it rests on -- two workgroups
        // per CU, every block of the largest grid resident at once
        e = hipMalloc((void**)&c->fz, sizeof(FusedWs));
        if (e == hipSuccess) e = hipMemsetAsync(c->fz, 0, sizeof(FusedWs), c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        int per_cu = 8, ncu = 0;
        for (const void* fnp : {reinterpret_cast<const void*>(&k_obs<0, 0>), reinterpret_cast<const void*>(&k_obs<0, 1>),
                                reinterpret_cast<const void*>(&k_obs<1, 0>), reinterpret_cast<const void*>(&k_obs<1, 1>)}) {
            if (e == hipSuccess) e = hipFuncSetAttribute(fnp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FZ_DYN_LDS);
            int nb = 0;
            if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fnp, NT, FZ_DYN_LDS);
            per_cu = std::min(per_cu, nb);
        }
        if (e == hipSuccess) e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        c->fz_ok = (e == hipSuccess) && per_cu >= 1 && (long long)per_cu * ncu >= FZ_MAXB;
    }
    if (e != hipSuccess) {
        g_err = std::string("bssm_ctx_create: ") + hipGetErrorString(e);
        bssm_ctx_destroy(c);
        return BSSM_ERR_HIP;
    }
    *out = c;
    return BSSM_OK;
}

extern "C" void bssm_ctx_destroy(bssm_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void* ptrs[] = {c->x0, c->x1, c->lw, c->w, c->auxlw, c->auxg, c->cum, c->pm, c->ps, c->pq, c->bsum, c->bsq,
                    c->ain_w, c->ain_p, c->brec, c->brec_p, c->side, c->side_p, c->cin, c->st, c->fz};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (auto& kv : c->pool) if (kv.second.first) (void)hipFree(kv.second.first);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (auto ev : c->ev_pool) (void)hipEventDestroy(ev);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int bssm_ctx_synchronize(bssm_ctx* c)
{
    if (!c) ARGFAIL("ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

extern "C" void* bssm_ctx_stream(bssm_ctx* c) { return c ? (void*)c->stream : nullptr; }

extern "C" int bssm_ctx_set_option(bssm_ctx* c, int option, int value)
{
    // (a check of the value alone, in front of the one of ctx: it can be exercised where no device is)
    if (option == BSSM_OPT_RN_LEAPS && (value < 0 || value > RN_MAX_LEAPS)) ARGFAIL("bssm_ctx_set_option: rn_leaps takes 0 (Gillespie's direct method) or a number of leaps 1 .. 1024");
    if (option == BSSM_OPT_RN_METHOD && value != 0 && value != 1) ARGFAIL("bssm_ctx_set_option: rn_method takes 0 (rn_leaps decides: Gillespie's direct method or tau-leaping) or 1 (Euler-multinomial leaps)");
    if (option == BSSM_OPT_RN_NOISE && value != 0 && value != 1) ARGFAIL("bssm_ctx_set_option: rn_noise takes 0 or 1 (gamma white noise on the rates of the Euler-multinomial leaps)");
    if (!c) ARGFAIL("ctx is NULL");
    switch (option) {
        case BSSM_OPT_RN_NOISE: c->opt_rn_noise = value; break;
        case BSSM_OPT_RN_LEAPS: c->opt_rn_leaps = value; break;
        case BSSM_OPT_RN_METHOD: c->opt_rn_method = value; break;
        case BSSM_OPT_RECORD_WINDOW: c->opt_window = value; break;
        case BSSM_OPT_BATCH_LITERAL_MAX: c->opt_batch_lit_max = value; break;
        case BSSM_OPT_STAGE_EXPANSION: c->opt_stage = value; break;
        case BSSM_OPT_INKERNEL_RESOLVE: c->opt_inkernel_resolve = value; break;
        case BSSM_OPT_DEBUG_STOP: c->opt_debug_stop = value; break;
        case BSSM_OPT_FUSE_STEP: c->opt_fuse_step = value; break;
        case BSSM_OPT_RECOMPUTE_LW: c->opt_recompute_lw = value ? 1 : 0; break;
        case BSSM_OPT_RENORMALIZE: c->opt_renormalize = value ? 1 : 0; break;
        case BSSM_OPT_FUSED: c->opt_fused = value < 0 ? 0 : (value > 2 ? 2 : value); break;
        case BSSM_OPT_FUSED_PREFETCH: c->opt_fused_prefetch = value ? 1 : 0; break;
        case BSSM_OPT_FUSED_EARLY_MAX: c->opt_fused_early_max = value ? 1 : 0; break;
        case BSSM_OPT_MV_Y_MISSING: c->opt_mv_y_missing = value ? 1 : 0; break;
        case BSSM_OPT_FORCE_FALLBACK: {
            if (value < 0 || value > (FF_SERIAL_WALK | FF_GENERAL_LINK | FF_SUM_PASS_ONLY)) ARGFAIL("bssm_ctx_set_option: force_fallback takes the bits 1 | 2 | 4");
            // (a word of the run state that k_reset_state leaves alone: every path that resolves on this context sees it)
            const int32_t v = value;
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipMemcpyAsync(&c->st->force_fallback, &v, sizeof(v), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            c->opt_force_fallback = value;
            break;
        }
        case BSSM_OPT_FUSED_TAG: {
            // the next fused launch carries tag value + 1 (uint32: -3 starts 3 launches before the wrap); the workspace is zeroed, so
            // that no granule of an earlier launch can carry one of the coming tags
            if (!c->fz) ARGFAIL("bssm_ctx_set_option: this context has no fused workspace");
            HIPCHK(hipSetDevice(c->device));
            HIPCHK(hipMemsetAsync(c->fz, 0, sizeof(FusedWs), c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            c->fz_tag = (uint32_t)value;
            break;
        }
        default: ARGFAIL("bssm_ctx_set_option: unknown option");
    }
    return BSSM_OK;
}
__global__ void k_set_debug(DevState* st, int v) { st->debug_stop = v; }
__global__ void k_set_calls(DevState* st, int v) { st->res_calls = v; }       // the next resample call draws the generator's stream `v`
extern "C" int bssm_ctx_get_stamps(bssm_ctx* c, long long* out /* [4][16] */)
{   // DEV builds (make DEV=1): the clock64() stage stamps of the last run; zeros otherwise
    if (!c || !out) ARGFAIL("bssm_ctx_get_stamps: NULL argument");
    DevState h;
    HIPCHK(hipMemcpy(&h, c->st, sizeof(h), hipMemcpyDeviceToHost));
    memcpy(out, h.stamps, sizeof(h.stamps));
    return BSSM_OK;
}

extern "C" int bssm_ctx_set_profile(bssm_ctx* c, int enable)
{
    if (!c) ARGFAIL("ctx is NULL");
    c->profile = enable != 0;
    c->prof.clear();
    return BSSM_OK;
}

extern "C" int bssm_ctx_get_profile(bssm_ctx* c, int max_entries, const char** names, double* total_ms, long long* launches)
{
    if (!c) return 0;
    int k = 0;
    for (auto& kv : c->prof) {
        if (k >= max_entries) break;
        names[k] = kv.first.c_str(); total_ms[k] = kv.second.ms; launches[k] = kv.second.launches; k++;
    }
    return k;
}

// ---- launch helper: optional per-kernel-class timing ------------------------------------------
// Profile mode hands the launch a start and a stop event (hipExtLaunchKernelGGL): they receive the begin / end
// timestamps of the kernel's own dispatch, i.e. the duration rocprofv3 --kernel-trace reports.  (A pair of
// hipEventRecord calls around the launch would also time the dispatch of the launch, ~2.5 us here.)
static hipEvent_t prof_event(bssm_ctx* c)
{
    hipEvent_t e = nullptr;
    if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else (void)hipEventCreate(&e);
    return e;
}
#define LAUNCH(c, name, kern, grid, block, shmem, ...)                                                              \
    do {                                                                                                              \
        if ((c)->profile) {                                                                                           \
            hipEvent_t ea__ = prof_event(c), eb__ = prof_event(c);                                                    \
            hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), shmem, (c)->stream, ea__, eb__, 0, __VA_ARGS__);     \
            (c)->prof_pending.push_back({name, {ea__, eb__}});                                                        \
        } else hipLaunchKernelGGL(kern, dim3(grid), dim3(block), shmem, (c)->stream, __VA_ARGS__);                    \
    } while (0)

static void prof_collect(bssm_ctx* c)
{
    for (auto& p : c->prof_pending) {
        float ms = 0;
        (void)hipEventSynchronize(p.second.second);
        (void)hipEventElapsedTime(&ms, p.second.first, p.second.second);
        auto& e = c->prof[p.first]; e.ms += ms; e.launches++;
        c->ev_pool.push_back(p.second.first); c->ev_pool.push_back(p.second.second);
    }
    c->prof_pending.clear();
}
static PhiloxKey make_key(unsigned long long seed, unsigned long long stream)
{
    PhiloxKey k; k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32);
    k.stream = (uint32_t)stream ^ (uint32_t)((stream >> 32) * 0x9E3779B9u);
    return k;
}
static NoiseSrc noise_src(const double* arr, const PhiloxKey& key, uint32_t purpose, int call)
{
    NoiseSrc ns; ns.arr = arr; ns.key = key; ns.purpose = purpose; ns.call = (uint32_t)call;
    return ns;
}
// validity window of the scan records (ulps): the option's, or the one that fits N terms
static int rec_lim(const bssm_ctx* c, long long N) { return c->opt_window > 0 ? c->opt_window : rec_window(N); }

// ---- the argument blocks of the scan and expansion kernels, each filled in ONE place: launch_scan_and_apply, fused_obs,
// bssm_pf_run_multi and bssm_pf_run_sharded start from these and set only what their path does differently, stated where they do.
// As built: the log-weights are stored (xw: re-evaluated), no grid-max slot, no folding; lead / publishing block from the shard.
static FromLw from_lw(const bssm_ctx* c, const double* lw, double* w_out, long long N, int B, int plan, int obs_i,
                      int resample_algorithm, double threshold, double* ess, double* llh, int* resampled)
{
    FromLw f;
    f.lw = lw; f.w_out = w_out; f.pm = c->pm; f.ps = c->ps; f.pq = c->pq; f.nb = B;
    f.xw = nullptr; f.yw = 0; f.syw = 1; f.lsyw = 0; f.gmax = nullptr; f.fold = 0;
    f.lead = c->sh_boff; f.pub = c->sh_nloc ? c->sh_boff + c->sh_nloc / 2 : B / 2;
    f.ain_out = c->ain_w; f.plan = plan; f.N = N; f.obs_i = obs_i; f.resample_algorithm = resample_algorithm; f.threshold = threshold;
    f.ess_out = ess; f.llh_out = llh; f.resampled_out = resampled;
    return f;
}
// As built: prefixes from the cumsum pass, no exact cum_sum out, nothing auxiliary carried, no transition riding along (only the
// STEP kernels read step_*), one LDS staging array per particle array when the particles are stored and the ancestors are not.
static ApplyArgs apply_args(const bssm_ctx* c, const double* w, long long nw, int n, int B, const double* u, long long u_stride,
                            const PhiloxKey& key, int* anc, long long anc_stride, const double* xsrc, double* xdst, int dim,
                            long long xstride, double* se_part)
{
    ApplyArgs a;
    a.w = w; a.nw = nw; a.ain_p = c->ain_p; a.cin = c->cin; a.lim = rec_lim(c, nw); a.n = n;
    a.u_base = u; a.u_stride = u_stride; a.key = key; a.anc_out = anc; a.anc_stride = anc_stride; a.cum_out = nullptr;
    a.xsrc = xsrc; a.xdst = xdst; a.dim = dim; a.xstride = xstride; a.auxsrc = nullptr; a.auxdst = nullptr; a.se_part = se_part;
    a.nstage = (c->opt_stage && xdst && !anc) ? (dim > 1 ? 2 : 1) : 0;
    a.lead = c->sh_boff; a.last = c->sh_boff + (c->sh_nloc ? c->sh_nloc : B) - 1;
    a.step_model = -1; memset(&a.step_par, 0, sizeof(a.step_par)); a.step_y = 0; a.step_ns = noise_src(nullptr, key, 0, 0); a.step_lw = nullptr;
    return a;
}

// ---- the exact resampling pipeline on weights already in HBM ---------------------
// resample_*_cpp: total = sum(w); prob = w/total; cum = cumsum(prob); walk.   src/resampling.cpp:16-66
struct ResampleLaunch {
    // filter path: weights are produced from log-weights inside the first scan kernel
    const double* d_lw = nullptr; int plan = PLAN_RESAMPLE_ONLY; int check_degenerate = 0;
    const double* xw = nullptr; double yw = 0, syw = 1, lsyw = 0;      // log-weights not stored: dnorm(yw, xw[j], syw) re-evaluated by the normalising kernel
    int obs_i = 0; int resample_algorithm = 1; double threshold = 0; double* d_ess = nullptr; double* d_llh = nullptr; int* d_resampled = nullptr;
    const double* d_w; long long nw; int n; int kind;
    const double* d_u; long long u_stride; PhiloxKey key;
    int* d_anc; long long anc_stride; double* d_cum;
    const double* xsrc = nullptr; double* xdst = nullptr; int dim = 1; long long xstride = 0;      // as built: ancestors only, nothing gathered
    const double* auxsrc = nullptr; double* auxdst = nullptr; double* se_part = nullptr;
    // the next observation's transition + weight fused into the expansion (k_apply<.., STEP>): model id or -1
    int step_model = -1; ModelPar step_par; double step_y = 0; NoiseSrc step_ns;
};

static void launch_scan_and_apply(bssm_ctx* c, const ResampleLaunch& r)
{
    const int B = (int)((r.nw + EB - 1) / EB);
    const int lim = rec_lim(c, r.nw);
    const size_t shm = (size_t)B * sizeof(BlockRec);
    const int boff = c->sh_boff, G = c->sh_nloc ? c->sh_nloc : B;        // launch grid: all blocks, or this rank's (sharded)
    const int Bg = c->sh_nloc ? B : 0;                                   // global block count handed to the kernels when sharded
    FromLw f = from_lw(c, r.d_lw, const_cast<double*>(r.d_w), r.nw, B, r.plan, r.obs_i, r.resample_algorithm, r.threshold, r.d_ess, r.d_llh, r.d_resampled);
    f.xw = r.xw; f.yw = r.yw; f.syw = r.syw; f.lsyw = r.lsyw;      // (xw set: the caller's k_step did not store the log-weights)
    const bool fold = r.d_lw && !c->opt_renormalize && !c->sh_nloc && r.kind != BSSM_MULTINOMIAL_R;
    f.fold = fold ? 1 : 0;
    f.gmax = (r.d_lw && !c->sh_nloc) ? c->gmax_cur : nullptr;       // (sharded: the partial maxima of other ranks are not in this rank's slots)
    if (r.kind == BSSM_MULTINOMIAL_R) {
        // parity mode: Rcpp::sample's own algorithm on the injected unif_rand() stream; no exact scan involved
        if (r.d_lw) LAUNCH(c, "k_weights(normalize+local<W>)", (k_local<MODE_W, true>), G, NT, 0, r.d_w, r.nw, c->ain_w, lim, c->brec, c->side, c->st, f, nullptr, nullptr, nullptr, boff, Bg);
        void *dq, *da, *dh, *danc = r.d_anc;
        if (pool_get(c, "mr_q", (size_t)r.nw * 8, &dq) || pool_get(c, "mr_a", (size_t)r.nw * 4, &da) || pool_get(c, "mr_hl", (size_t)r.nw * 4, &dh)) return;
        long long astride = r.anc_stride;
        if (!danc) { if (pool_get(c, "mr_anc", (size_t)r.n * 4, &danc)) return; astride = 0; }
        LAUNCH(c, "k_multinomial_r", k_multinomial_r, 1, NTM, 0, r.d_w, r.n, r.d_u, r.u_stride, (int*)danc, astride, (double*)dq, (int*)da, (int*)dh, c->st);
        if (r.xdst || r.auxdst) {
            const int Bo = (int)(((long long)r.n + EB - 1) / EB);
            LAUNCH(c, "k_gather_anc", k_gather_anc, Bo, NT, 0, (const int*)danc, astride, r.n, r.xsrc, r.xdst, r.dim, r.xstride, r.auxsrc, r.auxdst, r.se_part, c->st);
        }
        return;
    }
    // B <= 2 NT: the consuming kernels resolve the pass before them in every workgroup (resolve_in_block); larger grids
    // keep the single-workgroup k_resolve launches (a thread would have to hold more than two block records)
    const bool inres = c->opt_inkernel_resolve && B <= 2 * NT;
    if (r.d_lw) LAUNCH(c, "k_weights(normalize+local<W>)", (k_local<MODE_W, true>), G, NT, 0, r.d_w, r.nw, c->ain_w, lim, c->brec, c->side, c->st, f, nullptr, nullptr, nullptr, boff, Bg);
    else LAUNCH(c, "k_local<W>", (k_local<MODE_W, false>), G, NT, 0, r.d_w, r.nw, c->ain_w, lim, c->brec, c->side, c->st, f, nullptr, nullptr, nullptr, boff, Bg);
    // grids of more than 2 NT blocks: one workgroup of NTR threads runs the block-wide resolve and emits every block's state
    // (k_resolve_all); k_resolve (the round-1 resolver) remains for inkernel_resolve = 0 on small grids
    const bool rall = c->opt_inkernel_resolve && !inres && B <= 2 * NTR;
    if (fold) {
        // the W records are the records of cumsum(prob) (total == 1): the expansion resolves them directly
        if (rall) LAUNCH(c, "k_resolve_all<P>", k_resolve_all<MODE_P>, 1, NTR, 0, r.d_w, r.nw, B, c->brec, c->side, c->cin, c->ain_w, c->ain_p, c->st);
        else if (!inres) LAUNCH(c, "k_resolve<P>", k_resolve<MODE_P>, 1, NTR, shm, r.d_w, r.nw, B, c->brec, c->side, c->cin, c->ain_w, c->ain_p, c->st);
    } else if (rall) {
        LAUNCH(c, "k_resolve_all<W>", k_resolve_all<MODE_W>, 1, NTR, 0, r.d_w, r.nw, B, c->brec, c->side, c->cin, c->ain_w, c->ain_p, c->st);
        LAUNCH(c, "k_local<P>", (k_local<MODE_P, false>), G, NT, 0, r.d_w, r.nw, c->ain_p, lim, c->brec_p, c->side_p, c->st, f, nullptr, nullptr, nullptr, boff, Bg);
        LAUNCH(c, "k_resolve_all<P>", k_resolve_all<MODE_P>, 1, NTR, 0, r.d_w, r.nw, B, c->brec_p, c->side_p, c->cin, c->ain_w, c->ain_p, c->st);
    } else if (inres) {
        LAUNCH(c, "k_local<P>(+resolve<W>)", (k_local<MODE_P, false, true>), G, NT, 0, r.d_w, r.nw, c->ain_w, lim, c->brec_p, c->side_p, c->st, f, c->brec, c->side, c->ain_p, boff, Bg);
    } else {
        LAUNCH(c, "k_resolve<W>", k_resolve<MODE_W>, 1, NTR, shm, r.d_w, r.nw, B, c->brec, c->side, c->cin, c->ain_w, c->ain_p, c->st);
        LAUNCH(c, "k_local<P>", (k_local<MODE_P, false>), G, NT, 0, r.d_w, r.nw, c->ain_p, lim, c->brec_p, c->side_p, c->st, f, nullptr, nullptr, nullptr, boff, Bg);
        LAUNCH(c, "k_resolve<P>", k_resolve<MODE_P>, 1, NTR, shm, r.d_w, r.nw, B, c->brec_p, c->side_p, c->cin, c->ain_w, c->ain_p, c->st);
    }
    const BlockRec* pb = inres ? (fold ? c->brec : c->brec_p) : nullptr;
    const SideList* psd = inres ? (fold ? c->side : c->side_p) : nullptr;
    ApplyArgs a = apply_args(c, r.d_w, r.nw, r.n, B, r.d_u, r.u_stride, r.key, r.d_anc, r.anc_stride, r.xsrc, r.xdst, r.dim, r.xstride, r.se_part);
    if (fold) a.ain_p = c->ain_w;
    a.cum_out = (r.kind == BSSM_MULTINOMIAL) ? (r.d_cum ? r.d_cum : c->cum) : r.d_cum;
    a.auxsrc = r.auxsrc; a.auxdst = r.auxdst;
    // LDS staging for the coalesced particle store: one array per thing carried to the outputs (the multinomial walk stores for itself)
    if (r.kind == BSSM_MULTINOMIAL) a.nstage = 0; else if (a.nstage && r.auxdst) a.nstage++;
    const bool step = r.step_model >= 0;
    if (step) { a.step_model = r.step_model; a.step_par = r.step_par; a.step_y = r.step_y; a.step_ns = r.step_ns; a.step_lw = c->lw; }
    // several rounds of workgroups per CU (more than 2 NT blocks), scalar state, nothing else to carry: the lean expansion
    // (fewer registers, a smaller staging area: four workgroups per CU instead of three)
    const bool lean = !inres && !step && B > 2 * NT && r.dim == 1 && !r.auxdst && !r.d_anc && a.nstage == 1;
    const size_t xshm = lean ? (size_t)CAP_LEAN * sizeof(double)
                             : std::max((size_t)a.nstage * CAPX * sizeof(double), inres ? sizeof(ResolveSmem) : (size_t)0);
#define APPLY(K, NAME) do { \
        if (lean) LAUNCH(c, "k_apply<" NAME ",lean>", (k_apply<K, false, false, true>), G, NT, xshm, a, c->st, pb, psd, boff, Bg); \
        else if (inres && step) LAUNCH(c, "k_apply+step<" NAME ">(+resolve<P>)", (k_apply<K, true, true>), G, NT, xshm, a, c->st, pb, psd, boff, Bg); \
        else if (inres) LAUNCH(c, "k_apply<" NAME ">(+resolve<P>)", (k_apply<K, true, false>), G, NT, xshm, a, c->st, pb, psd, boff, Bg); \
        else if (step) LAUNCH(c, "k_apply+step<" NAME ">", (k_apply<K, false, true>), G, NT, xshm, a, c->st, pb, psd, boff, Bg); \
        else LAUNCH(c, "k_apply<" NAME ">", (k_apply<K, false, false>), G, NT, xshm, a, c->st, pb, psd, boff, Bg); } while (0)
    if (r.kind == BSSM_SYSTEMATIC) APPLY(1, "systematic");
    else if (r.kind == BSSM_STRATIFIED) APPLY(0, "stratified");
#undef APPLY
    else {
        if (inres) LAUNCH(c, "k_apply<cum>(+resolve<P>)", (k_apply<2, true>), G, NT, xshm, a, c->st, pb, psd, boff, Bg); else LAUNCH(c, "k_apply<cum>", (k_apply<2, false>), G, NT, xshm, a, c->st, pb, psd, boff, Bg);
        const int Bo = (int)(((long long)r.n + EB - 1) / EB);
        LAUNCH(c, "k_multinomial", k_multinomial, Bo, NT, 0, a.cum_out, r.nw, r.n, a, c->st);
    }
}

static int flags_to_status(uint32_t f)
{
    f &= ~(FLAG_FUSED_BAIL | FLAG_FUSED_TIMEOUT);      // (not errors: the run is repeated on the multi-launch path)
    if (f & FLAG_NEGATIVE) return BSSM_ERR_NEGATIVE_WEIGHT;     // checked first, as the reference does
    if (f & FLAG_NONFINITE) { g_err = "weights contain NaN/Inf"; return BSSM_ERR_ARG; }
    if (f & FLAG_ZERO_SUM) return BSSM_ERR_ZERO_SUM;
    return BSSM_OK;
}

static int resample_common_device(bssm_ctx* c, int kind, int n, const double* d_w, int nw, const double* d_u,
                                  int* d_idx, double* d_cum)
{
    const int B = (nw + EB - 1) / EB;
    LAUNCH(c, "k_reset_state", k_reset_state, 1, 1, 0, c->st);
    if (c->opt_debug_stop) hipLaunchKernelGGL(k_set_debug, dim3(1), dim3(1), 0, c->stream, c->st, c->opt_debug_stop);
    LAUNCH(c, "k_bsum", k_bsum, B, NT, 0, d_w, (long long)nw, c->bsum, c->st);
    LAUNCH(c, "k_plan", k_plan, 1, NT, 0, c->bsum, B, c->ain_w, c->st);
    ResampleLaunch r;
    r.d_w = d_w; r.nw = nw; r.n = n; r.kind = kind; r.d_u = d_u; r.u_stride = (kind == BSSM_SYSTEMATIC) ? 1 : n;
    r.key = make_key(0, 0); r.d_anc = d_idx; r.anc_stride = 0; r.d_cum = d_cum;
    launch_scan_and_apply(c, r);
    return BSSM_OK;
}

extern "C" int bssm_resample_device(bssm_ctx* c, int kind, int n, const double* d_w, int nw, double U_scalar,
                                    const double* d_U, int* d_idx, double* d_cum)
{
    if (!c) ARGFAIL("ctx is NULL");
    if (n <= 0 || nw <= 0) ARGFAIL("bssm_resample_device: n and nw must be positive");
    if (kind < 0 || kind > 3) ARGFAIL("bssm_resample_device: unknown resampler kind");
    if ((long long)nw > c->cap || (long long)n > c->cap) { g_err = "bssm_resample_device: size exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    const double* du = d_U;
    if (kind == BSSM_SYSTEMATIC && !d_U) {
        void* p; int rc = pool_put(c, "u_scalar", &U_scalar, 8, &p); if (rc) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));   // U_scalar lives on the caller's stack
        du = (const double*)p;
    }
    if (!du) ARGFAIL("bssm_resample_device: d_U is required for stratified/multinomial");
    return resample_common_device(c, kind, n, d_w, nw, du, d_idx, d_cum);
}

extern "C" int bssm_resample_device_status(bssm_ctx* c)
{
    if (!c) ARGFAIL("ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    DevState h;
    HIPCHK(hipMemcpyAsync(&h, c->st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    return flags_to_status(h.flags);
}

extern "C" int bssm_resample_ex(bssm_ctx* c, int kind, int n, const double* w, int nw, const double* U,
                                int* idx_out, double* cum_out, long long* stats)
{
    if (!c) ARGFAIL("ctx is NULL");
    if (!w || !idx_out || !U) ARGFAIL("bssm_resample: NULL pointer argument");
    if (kind < 0 || kind > 3) ARGFAIL("bssm_resample: unknown resampler kind");
    if (kind == BSSM_MULTINOMIAL_R && n != nw) ARGFAIL("probs.size() != n!");      // Rcpp::sample's own check
    if (n <= 0 || nw <= 0) ARGFAIL("bssm_resample: n and nw must be positive");
    if ((long long)nw > c->cap || (long long)n > c->cap) { g_err = "bssm_resample: size exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    void *dw, *du, *di, *dc = nullptr;
    int rc;
    const size_t nu = (kind == BSSM_SYSTEMATIC) ? 1 : (size_t)n;
    if ((rc = pool_put(c, "rs_w", w, (size_t)nw * 8, &dw))) return rc;
    if ((rc = pool_put(c, "rs_u", U, nu * 8, &du))) return rc;
    if ((rc = pool_get(c, "rs_idx", (size_t)n * 4, &di))) return rc;
    if (cum_out || kind == BSSM_MULTINOMIAL) { if ((rc = pool_get(c, "rs_cum", (size_t)nw * 8, &dc))) return rc; }
    rc = resample_common_device(c, kind, n, (const double*)dw, nw, (const double*)du, (int*)di, (double*)dc);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    DevState h;
    HIPCHK(hipMemcpyAsync(&h, c->st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (stats) { stats[0] = h.stat_hard_blocks; stats[1] = h.stat_serial_walks; stats[2] = h.stat_literal_terms; stats[3] = (nw + EB - 1) / EB; }
    const int st = flags_to_status(h.flags);
    if (st) { if (st != BSSM_ERR_ARG) g_err = bssm_status_string(st); return st; }
    HIPCHK(hipMemcpy(idx_out, di, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (cum_out) HIPCHK(hipMemcpy(cum_out, dc, (size_t)nw * 8, hipMemcpyDeviceToHost));
    return BSSM_OK;
}

extern "C" int bssm_resample_systematic(bssm_ctx* c, int n, const double* w, int nw, double U, int* out)
{
    return bssm_resample_ex(c, BSSM_SYSTEMATIC, n, w, nw, &U, out, nullptr, nullptr);
}
extern "C" int bssm_resample_stratified(bssm_ctx* c, int n, const double* w, int nw, const double* U, int* out)
{
    return bssm_resample_ex(c, BSSM_STRATIFIED, n, w, nw, U, out, nullptr, nullptr);
}
extern "C" int bssm_resample_multinomial(bssm_ctx* c, int n, const double* w, int nw, const double* U, int* out)
{
    return bssm_resample_ex(c, BSSM_MULTINOMIAL, n, w, nw, U, out, nullptr, nullptr);
}

extern "C" int bssm_resample_multinomial_r(bssm_ctx* c, int n, const double* w, int nw, const double* U, int* out)
{
    return bssm_resample_ex(c, BSSM_MULTINOMIAL_R, n, w, nw, U, out, nullptr, nullptr);
}

// ---- generator dumps ---------------------------------------------------------------
extern "C" int bssm_dump_normals(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int purpose, int call,
                                 long long n, double* out)
{
    if (!c || !out || n <= 0) ARGFAIL("bssm_dump_normals: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void* d; int rc = pool_get(c, "dump", (size_t)n * 8, &d); if (rc) return rc;
    const long long pairs = (n + 1) / 2;
    hipLaunchKernelGGL(k_dump_normals, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, c->stream,
                       make_key(seed, stream), (uint32_t)purpose, (uint32_t)call, n, (double*)d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}
extern "C" int bssm_dump_move_draws(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int call, long long n,
                                    double* z_out, double* u_out)
{
    if (!c || !z_out || !u_out || n <= 0) ARGFAIL("bssm_dump_move_draws: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void *dz, *du; int rc;
    if ((rc = pool_get(c, "dump", (size_t)n * 8, &dz))) return rc;
    if ((rc = pool_get(c, "dump2", (size_t)n * 8, &du))) return rc;
    hipLaunchKernelGGL(k_dump_move, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, make_key(seed, stream), (uint32_t)call, n, (double*)dz, (double*)du);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(z_out, dz, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(u_out, du, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}
extern "C" int bssm_dump_uniforms(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int call, long long n, double* out)
{
    if (!c || !out || n <= 0) ARGFAIL("bssm_dump_uniforms: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void* d; int rc = pool_get(c, "dump", (size_t)n * 8, &d); if (rc) return rc;
    hipLaunchKernelGGL(k_dump_uniforms, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       make_key(seed, stream), (uint32_t)call, n, (double*)d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

// ---- particle filter ---------------------------------------------------------------
extern "C" int bssm_pf_noise_shape(int algorithm, int T, const int* obs_times, int* max_trans, int* max_res)
{
    if (T < 0 || !max_trans || !max_res) ARGFAIL("bssm_pf_noise_shape: bad argument");
    const int last = (T > 0) ? (obs_times ? obs_times[T - 1] : T) : 0;
    *max_trans = last + ((algorithm == BSSM_APF) ? T : 0);
    *max_res = T * ((algorithm == BSSM_APF) ? 2 : 1);
    return BSSM_OK;
}

template <int MODEL>
static void launch_step(bssm_ctx* c, bool trans, int weight, bool subaux, double* x, long long N, int B,
                        const ModelPar& par, double y, const NoiseSrc& ns, bool store_lw = true)
{
    if (c->sh_nloc) B = c->sh_nloc;                  // sharded: this rank's blocks only (k_step adds the block offset)
    double* lw_out = store_lw ? c->lw : nullptr;     // nullptr: the normalising kernel re-evaluates the log-weights (FromLw::xw)
#define STEP_ARGS x, x, lw_out, c->auxg, N, par, y, ns, c->pm, c->ps, c->pq, c->st, c->gmax_cur, c->sh_boff
    if (trans && weight == 1 && !subaux) LAUNCH(c, "k_step<trans+weight>", (k_step<MODEL, true, 1, false>), B, NTS, 0, STEP_ARGS);
    else if (trans && weight == 1 && subaux) LAUNCH(c, "k_step<trans+weight-aux>", (k_step<MODEL, true, 1, true>), B, NTS, 0, STEP_ARGS);
    else if (trans && weight == 0) LAUNCH(c, "k_step<trans>", (k_step<MODEL, true, 0, false>), B, NTS, 0, STEP_ARGS);
    else if (!trans && weight == 2) {
        LAUNCH(c, "k_step<aux-weight>", (k_step<MODEL, false, 2, false>), B, NTS, 0, x, x, c->auxlw, c->auxg, N, par, y, ns, c->pm, c->ps, c->pq, c->st, c->gmax_cur, c->sh_boff);
    } else if (!trans && weight == 1) LAUNCH(c, "k_step<weight>", (k_step<MODEL, false, 1, false>), B, NTS, 0, STEP_ARGS);   // obs_times repeats a time
#undef STEP_ARGS
}

static void launch_step_sir(bssm_ctx* c, bool trans, int weight, bool subaux, double* x, long long N, int B,
                            const ModelPar& par, double y, const NoiseSrc& ns)
{
#define SIR_ARGS(LW) x, x, LW, c->auxg, N, par, y, ns, c->pm, c->ps, c->pq, c->gmax_cur
    if (trans && weight == 1 && !subaux) LAUNCH(c, "k_step_sir<trans+weight>", (k_step_sir<true, 1, false>), B, NTS, 0, SIR_ARGS(c->lw));
    else if (trans && weight == 1 && subaux) LAUNCH(c, "k_step_sir<trans+weight-aux>", (k_step_sir<true, 1, true>), B, NTS, 0, SIR_ARGS(c->lw));
    else if (trans && weight == 0) LAUNCH(c, "k_step_sir<trans>", (k_step_sir<true, 0, false>), B, NTS, 0, SIR_ARGS(c->lw));
    else if (!trans && weight == 2) LAUNCH(c, "k_step_sir<aux-weight>", (k_step_sir<false, 2, false>), B, NTS, 0, SIR_ARGS(c->auxlw));
    else if (!trans && weight == 1) LAUNCH(c, "k_step_sir<weight>", (k_step_sir<false, 1, false>), B, NTS, 0, SIR_ARGS(c->lw));
#undef SIR_ARGS
}

static void launch_step_model(bssm_ctx* c, int model, bool trans, int weight, bool subaux, double* x, long long N, int B,
                              const ModelPar& par, double y, const NoiseSrc& ns, bool store_lw = true)
{
    if (model == BSSM_MODEL_LG) launch_step<0>(c, trans, weight, subaux, x, N, B, par, y, ns, store_lw);
    else if (model == BSSM_MODEL_AR1SIN) launch_step<1>(c, trans, weight, subaux, x, N, B, par, y, ns, store_lw);
    else launch_step_sir(c, trans, weight, subaux, x, N, B, par, y, ns);
}

// ---- what the runners share: two argument rules, the record of a run with its set-up, and the read-back ------------------------
static int obs_times_check(const int* obs_times, int T)                 // assert_integerish(lower = 1, sorted = TRUE) :73
{
    int prev = 1;
    for (int i = 0; obs_times && i < T; i++) { if (obs_times[i] < prev) ARGFAIL("Assertion on 'obs_times' failed: Must be sorted and >= 1"); prev = obs_times[i]; }
    return BSSM_OK;
}
// NaN: NULL => the algorithm's own (:44-50); an explicit value, negative included, is kept
static double threshold_or_auto(int resample_algorithm, double threshold, double dN)
{
    if (!isnan(threshold)) return threshold;
    return (resample_algorithm == BSSM_SIS) ? INFINITY : (resample_algorithm == BSSM_SISR) ? dN : dN / 2;
}

// One filter run on one context: what every kernel launch of it is told, and the per-run device outputs (pool buffers)
struct PfRun {
    long long N; int T, B, dim; double dN;
    int resample_algorithm; double threshold;
    int max_trans, max_res; long long u_stride, anc_stride; PhiloxKey key;
    double *ess, *llh, *se, *separt, *ph, *wh; int *resampled, *anc; const double* ur;
    int *call_obs, *noted;      // smoother only (else nullptr): the observation of every ancestor row, and how many rows are labelled
};

// The clock of the T-loop (:123-124): observation i's time, the transitions since the previous one (0: obs_times repeats a time) and up
// to the next one (0: there is none); ktrans numbers the transition calls, which is what keys their draws.
struct ObsClock {
    const int* times; int T;
    int ot = 0, gap = 0, prev_t = 0, ktrans = 0;
    ObsClock(const int* obs_times, int T_) : times(obs_times), T(T_) {}
    int at(int i) const { return times ? times[i - 1] : i; }
    void advance(int i) { ot = at(i); gap = ot - prev_t; prev_t = ot; }
    int gap_after(int i) const { return i < T ? at(i + 1) - at(i) : 0; }
};

// theta of the scalar models: (phi, sigma_x, sigma_y), or the SIR model's (lambda, gamma, n_total, s0, i0)
static ModelPar scalar_par(int model, const double* theta)
{
    ModelPar par; memset(&par, 0, sizeof(par));
    par.phi = theta[0]; par.sx = theta[1]; par.sy = theta[2]; par.log_sy = log(theta[2]);
    if (model == BSSM_MODEL_SIR) { par.n_total = theta[2]; par.s0 = theta[3]; par.i0 = theta[4]; }
    return par;
}
// the draws of transition call k of a scalar-state run: row k of the injected z_trans, or the generator
static NoiseSrc trans_noise(const PfRun& r, const double* zt, int k) { return noise_src(zt ? zt + (size_t)k * r.N : nullptr, r.key, DRAW_TRANS, k); }

// The grid-max slots of a run: one per weight evaluation, zeroed (key 0 lies below every double's key); next() stays on the last one
struct GmaxSlots {
    unsigned long long* base = nullptr; size_t n = 0, used = 0;
    static constexpr size_t WORDS = (size_t)GM_SLOTS * GM_STRIDE;
    int take(bssm_ctx* c, size_t n_slots, hipStream_t zero_on)
    {
        n = n_slots;
        if (int rc = pool_get(c, "gmax", n * WORDS * 8, &base)) return rc;
        HIPCHK(hipMemsetAsync(base, 0, n * WORDS * 8, zero_on));
        return BSSM_OK;
    }
    unsigned long long* next() { const size_t k = used < n ? used : n - 1; used++; return base + k * WORDS; }
};

// A run for the smoother records its histories and ancestor rows whatever the caller's cfg says (bssm_pf_run_smooth sets both flags
// in its copy); they are copied to the host only where the caller's own cfg asked for them
static bool host_wants_particles(const bssm_ctx* c, const bssm_pf_config* cfg) { return cfg->return_particles && (!c->smooth || c->smooth->host_particles); }
static bool host_wants_ancestors(const bssm_ctx* c, const bssm_pf_config* cfg) { return cfg->return_ancestors && (!c->smooth || c->smooth->host_ancestors); }
// (smoother) the resample calls observation i made get its index, on the device, behind the launches that made them
static void note_calls(bssm_ctx* c, const PfRun& r, int i)
{
    if (r.call_obs) LAUNCH(c, "k_note_calls", k_note_calls, 1, 1, 0, (const DevState*)c->st, r.call_obs, r.noted, i, std::max(r.max_res, 1));
}

// Fills the record, takes the buffers, zeroes them and uploads u_res.  dim: doubles per particle.  anc_always: the family's gather
// reads the ancestors of the call in flight, so there is always a buffer -- N of them reused by every call (stride 0), or one row
// per call when they are returned; without it (scalar models) the buffer exists only when they are returned, zeroed, stride N.
// zero_on: the stream the zeroing is ordered on when it is not the context's own (the lock-step runner's one stream for all filters).
static int pf_run_setup(bssm_ctx* c, const bssm_pf_config* cfg, const bssm_pf_result* res, int dim, bool anc_always, PfRun& r, hipStream_t zero_on = nullptr)
{
    if (!zero_on) zero_on = c->stream;
    const bool rmpf = cfg->algorithm == BSSM_RMPF;        // forces SISR and the automatic threshold (R/resample_move_filter.R:229)
    r.N = cfg->num_particles; r.T = cfg->T; r.B = (int)((r.N + EB - 1) / EB); r.dim = dim; r.dN = (double)r.N;
    r.resample_algorithm = rmpf ? BSSM_SISR : cfg->resample_algorithm;
    r.threshold = threshold_or_auto(r.resample_algorithm, rmpf ? (double)NAN : cfg->threshold, r.dN);
    bssm_pf_noise_shape(cfg->algorithm, r.T, cfg->obs_times, &r.max_trans, &r.max_res);
    r.u_stride = (cfg->resample_fn == BSSM_SYSTEMATIC) ? 1 : r.N;
    r.anc_stride = (anc_always && !cfg->return_ancestors) ? 0 : r.N;
    r.key = make_key(cfg->seed, cfg->stream);
    r.anc = nullptr; r.ph = r.wh = nullptr; r.ur = nullptr; r.call_obs = r.noted = nullptr;
    const size_t T1 = (size_t)r.T + 1, n_separt = T1 * r.B * dim * 8, n_anc = (size_t)(cfg->return_ancestors ? std::max(r.max_res, 1) : 1) * r.N * 4;
    int rc;
    if ((rc = pool_get(c, "ess", T1 * 8, &r.ess))) return rc;
    if ((rc = pool_get(c, "llh", T1 * 8, &r.llh))) return rc;
    if ((rc = pool_get(c, "se", T1 * dim * 8, &r.se))) return rc;
    if ((rc = pool_get(c, "separt", n_separt, &r.separt))) return rc;
    if ((rc = pool_get(c, "resampled", T1 * 4, &r.resampled))) return rc;
    if (host_wants_ancestors(c, cfg) && !res->ancestors) ARGFAIL("bssm_pf_run: ancestors buffer missing");
    if (c->smooth) {
        // the histories stay on the device for the trace: they have to fit what the device has free (what the pool already holds counts)
        const size_t n_ph = T1 * r.N * dim * 8, n_wh = T1 * r.N * 8, n_seen = T1 * (size_t)((r.N + 31) / 32) * 4, n_part = T1 * (size_t)((r.N + NT - 1) / NT) * dim * 8;
        const size_t need = n_ph + n_wh + n_anc + n_seen + n_part;
        size_t grow = 0, mfree = 0, mtotal = 0;
        const std::pair<const char*, size_t> bufs[] = {{"ph", n_ph}, {"wh", n_wh}, {"anc", n_anc}, {"sm_seen", n_seen}, {"sm_part", n_part}};
        for (const auto& b : bufs) { const auto it = c->pool.find(b.first); const size_t have = it == c->pool.end() ? 0 : it->second.second; if (have < b.second) grow += b.second + b.second / 4 + 256 - have; }
        HIPCHK(hipMemGetInfo(&mfree, &mtotal));
        if (grow > mfree) {
            g_err = "bssm_pf_run_smooth: the histories, ancestor rows and trace workspace need " + std::to_string((unsigned long long)need) + " bytes of device memory (" +
                    std::to_string((unsigned long long)grow) + " more than this context holds, " + std::to_string((unsigned long long)mfree) + " free)";
            return BSSM_ERR_CAPACITY;
        }
        if ((rc = pool_get(c, "sm_call_obs", ((size_t)std::max(r.max_res, 1) + 1) * 4, &r.call_obs))) return rc;
        r.noted = r.call_obs + std::max(r.max_res, 1);
        HIPCHK(hipMemsetAsync(r.call_obs, 0, ((size_t)std::max(r.max_res, 1) + 1) * 4, zero_on));
    }
    if ((anc_always || cfg->return_ancestors) && (rc = pool_get(c, "anc", n_anc, &r.anc))) return rc;
    if (cfg->return_particles) {
        if (host_wants_particles(c, cfg) && (!res->particles_history || !res->weights_history)) ARGFAIL("bssm_pf_run: history buffers missing");
        if ((rc = pool_get(c, "ph", T1 * r.N * dim * 8, &r.ph))) return rc;
        if ((rc = pool_get(c, "wh", T1 * r.N * 8, &r.wh))) return rc;
    }
    HIPCHK(hipMemsetAsync(r.separt, 0, n_separt, zero_on));
    HIPCHK(hipMemsetAsync(r.ess, 0, T1 * 8, zero_on));
    HIPCHK(hipMemsetAsync(r.llh, 0, T1 * 8, zero_on));
    HIPCHK(hipMemsetAsync(r.resampled, 0, T1 * 4, zero_on));
    if (r.anc && !anc_always) HIPCHK(hipMemsetAsync(r.anc, 0, n_anc, zero_on));
    if (cfg->u_res && r.max_res > 0 && (rc = pool_put(c, "ur", cfg->u_res, (size_t)r.max_res * r.u_stride * 8, &r.ur))) return rc;
    return BSSM_OK;
}

// history row 0: the initial particles, and weights = rep(1/N, N) (do_resample is 0 after reset, so from a constant fill)
static int pf_run_seed_history(bssm_ctx* c, const PfRun& r, const double* X0)
{
    std::vector<double> w0((size_t)r.N, 1.0 / r.dN);
    HIPCHK(hipMemcpyAsync(r.wh, w0.data(), (size_t)r.N * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpyAsync(r.ph, X0, (size_t)r.N * r.dim * 8, hipMemcpyDeviceToDevice, c->stream));
    return BSSM_OK;
}

// The end of a run, first half: the run state and the per-observation outputs come back, the stream is drained.  Nothing but
// the arrays of res is written yet: the scalar runner decides on h whether the run stands (a fused run that stood down is repeated).
static int pf_run_read_back(bssm_ctx* c, const PfRun& r, bssm_pf_result* res, DevState& h)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, c->st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(res->state_est, r.se, (size_t)(r.T + 1) * r.dim * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(res->ess, r.ess, (size_t)(r.T + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (r.T > 0) HIPCHK(hipMemcpyAsync(res->loglike_history, r.llh, (size_t)r.T * 8, hipMemcpyDeviceToHost, c->stream));
    if (res->resampled && r.T > 0) HIPCHK(hipMemcpyAsync(res->resampled, r.resampled, (size_t)r.T * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    return BSSM_OK;
}
// ... of a run on one GPU: the state estimates are reduced and the timed span closed first
static int pf_run_finish(bssm_ctx* c, const PfRun& r, bssm_pf_result* res, DevState& h)
{
    LAUNCH(c, "k_reduce_state_est", k_reduce_state_est, r.T + 1, NT, 0, r.separt, r.B, r.dim, r.se);
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    return pf_run_read_back(c, r, res, h);
}
// The genealogy smoother (smooth.hip.h) on the histories and ancestor rows the run left in r.ph, r.wh, r.anc: the trace, the sum of
// its block partials (k_reduce_state_est, as the filter's state estimates), and for K > 0 the terminal draw -- the multinomial leg
// of the resampler on W with K outputs -- and the K paths.  A run that returned early is not traced.
static int smooth_trace(bssm_ctx* c, const PfRun& r, const DevState& h)
{
    bssm_smooth_result* o = c->smooth->out;
    const int K = c->smooth->K, T = r.T, d = r.dim, n_calls = h.res_calls;
    const long long N = r.N;
    if (o->smooth_ms) *o->smooth_ms = 0.0;
    if (o->call_obs && n_calls > 0) HIPCHK(hipMemcpy(o->call_obs, r.call_obs, (size_t)n_calls * 4, hipMemcpyDeviceToHost));
    if (h.dead) return BSSM_OK;
    const size_t T1 = (size_t)T + 1;
    const int Bt = (int)((N + NT - 1) / NT);
    const long long words = (N + 31) / 32;
    double *part, *sm, *traj = nullptr, *du = nullptr; int *nlin, *didx = nullptr; unsigned int* seen;
    int rc;
    if ((rc = pool_get(c, "sm_part", T1 * Bt * d * 8, &part))) return rc;
    if ((rc = pool_get(c, "sm_seen", T1 * (size_t)words * 4, &seen))) return rc;
    if ((rc = pool_get(c, "sm_se", T1 * d * 8, &sm))) return rc;
    if ((rc = pool_get(c, "sm_nlin", T1 * 4, &nlin))) return rc;
    if (K > 0) {
        if ((rc = pool_get(c, "sm_traj", (size_t)K * T1 * d * 8, &traj))) return rc;
        if ((rc = pool_get(c, "sm_u", (size_t)K * 8, &du))) return rc;
        if ((rc = pool_get(c, "sm_idx", (size_t)K * 4, &didx))) return rc;
    }
    const double* W = r.wh + (size_t)T * N;
    hipEvent_t ea = prof_event(c), eb = prof_event(c);
    HIPCHK(hipEventRecord(ea, c->stream));
    HIPCHK(hipMemsetAsync(seen, 0, T1 * (size_t)words * 4, c->stream));
    HIPCHK(hipMemsetAsync(nlin, 0, T1 * 4, c->stream));
    LAUNCH(c, "k_trace", k_trace, Bt, NT, 0, (const double*)r.ph, W, (const int*)r.anc, (const int*)r.call_obs, n_calls, N, d, T, part, nlin, seen, words);
    LAUNCH(c, "k_reduce_state_est", k_reduce_state_est, (int)T1, NT, 0, (const double*)part, Bt, d, sm);
    if (K > 0) {
        LAUNCH(c, "k_traj_uniforms", k_traj_uniforms, (K + 255) / 256, 256, 0, r.key, K, du);
        if ((rc = resample_common_device(c, BSSM_MULTINOMIAL, K, W, (int)N, du, didx, nullptr))) return rc;
        LAUNCH(c, "k_trace_paths", k_trace_paths, (K + 255) / 256, 256, 0, (const double*)r.ph, (const int*)r.anc, (const int*)r.call_obs, n_calls, N, d, T, (const int*)didx, K, traj);
    }
    HIPCHK(hipEventRecord(eb, c->stream));
    HIPCHK(hipGetLastError());
    DevState hs;
    HIPCHK(hipMemcpyAsync(&hs, c->st, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->smoothed, sm, T1 * d * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->n_lineages, nlin, T1 * 4, hipMemcpyDeviceToHost, c->stream));
    if (K > 0) {
        HIPCHK(hipMemcpyAsync(o->trajectories, traj, (size_t)K * T1 * d * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(o->trajectory_u, du, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(o->trajectory_index, didx, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ea, eb));
    c->ev_pool.push_back(ea); c->ev_pool.push_back(eb);
    if (o->smooth_ms) *o->smooth_ms = ms;
    if (K > 0 && hs.flags) { const int st = flags_to_status(hs.flags); if (st != BSSM_ERR_ARG) g_err = bssm_status_string(st); return st; }      // (the terminal draw's weights: W of a run that stood)
    return BSSM_OK;
}

// Second half: the scalars, the rows a run that returned early never reached, the status, the ancestors and the histories.
// timed: ev0 .. ev1 span the run (the sharded runner's collectives go through the host: it reports 0)
static int pf_run_results(bssm_ctx* c, const bssm_pf_config* cfg, const PfRun& r, const DevState& h, bool timed, bssm_pf_result* res)
{
    const int T = r.T, dim = r.dim;
    if (res->device_ms) { float ms = 0; if (timed) HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1)); *res->device_ms = ms; }
    res->ess[0] = 1.0 / (r.dN * ((1.0 / r.dN) * (1.0 / r.dN)));       // ess[1] = 1 / sum(rep(1/N, N)^2)   (:106-107)
    *res->loglike = h.loglike;
    if (res->early_return_step) *res->early_return_step = h.dead;
    if (res->n_res_calls) *res->n_res_calls = h.res_calls;
    if (res->scan_stats) { res->scan_stats[0] = h.stat_hard_blocks; res->scan_stats[1] = h.stat_serial_walks; res->scan_stats[2] = h.stat_literal_terms; }
    if (h.dead) {   // the reference returns at once (:189-202): later rows keep their initial values -- numeric(out_steps) = 0 for a scalar
                    // state, matrix(NA, out_steps, d) for d > 1 (:90-97); NaN stands for NA_real_ at the C ABI
        const double se_init = (dim > 1) ? (double)NAN : 0.0;
        for (int i = h.dead; i <= T; i++) { res->ess[i] = 0.0; for (int k = 0; k < dim; k++) res->state_est[(size_t)i * dim + k] = se_init; }
        for (int i = h.dead; i < T; i++) res->loglike_history[i] = 0.0;
    }
    if (h.flags) { const int st = flags_to_status(h.flags); if (st != BSSM_ERR_ARG) g_err = bssm_status_string(st); return st; }
    if (host_wants_ancestors(c, cfg) && h.res_calls > 0) HIPCHK(hipMemcpy(res->ancestors, r.anc, (size_t)h.res_calls * r.N * 4, hipMemcpyDeviceToHost));
    if (host_wants_particles(c, cfg)) {
        const int rows = h.dead ? h.dead : T + 1;
        HIPCHK(hipMemcpy(res->particles_history, r.ph, (size_t)rows * r.N * dim * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(res->weights_history, r.wh, (size_t)rows * r.N * 8, hipMemcpyDeviceToHost));
    }
    return c->smooth ? smooth_trace(c, r, h) : BSSM_OK;
}

static constexpr int BSSM_RETRY_UNFUSED = -1000;     // internal: a fused run stood down, repeat it on the multi-launch path

// the scalar runner's argument rules, in the order the reference makes its assertions
static int pf_run_check(const bssm_ctx* c, const bssm_pf_config* cfg, const bssm_pf_result* res)
{
    if (!c || !cfg || !res) ARGFAIL("bssm_pf_run: NULL argument");
    const long long N = cfg->num_particles;
    const int T = cfg->T;
    if (N <= 0) ARGFAIL("num_particles must be a positive count");                    // assert_count(..., positive = TRUE) :33
    if (T < 0) ARGFAIL("bssm_pf_run: T must be >= 0");
    if (N > c->cap) { g_err = "bssm_pf_run: num_particles exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    if (cfg->model != BSSM_MODEL_LG && cfg->model != BSSM_MODEL_AR1SIN && cfg->model != BSSM_MODEL_SIR) ARGFAIL("bssm_pf_run: unknown model");
    const bool sir = cfg->model == BSSM_MODEL_SIR;
    if (sir && (cfg->z_init || cfg->z_trans)) ARGFAIL("bssm_pf_run: the SIR model draws a data-dependent number of variates; injected z_* are not supported");
    if (sir && cfg->n_theta < 5) ARGFAIL("bssm_pf_run: SIR theta must hold (lambda, gamma, n_total, s0, i0)");
    if (sir && c->max_dim < 2) { g_err = "bssm_pf_run: the SIR model needs a context created with max_dim = 2"; return BSSM_ERR_CAPACITY; }
    if (cfg->algorithm != BSSM_BPF && cfg->algorithm != BSSM_APF && cfg->algorithm != BSSM_RMPF) ARGFAIL("bssm_pf_run: unknown algorithm");
    const bool rmpf = cfg->algorithm == BSSM_RMPF;
    if (rmpf && cfg->model == BSSM_MODEL_SIR) ARGFAIL("bssm_pf_run: the built-in move step is defined for the scalar Gaussian-observation models only");
    if (rmpf && !(cfg->move_sd > 0)) ARGFAIL("bssm_pf_run: RMPF needs move_sd > 0");
    if (rmpf && ((cfg->z_move == nullptr) != (cfg->u_move == nullptr))) ARGFAIL("bssm_pf_run: z_move and u_move must be given together");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL("bssm_pf_run: unknown resample_algorithm");
    if (cfg->resample_fn < 0 || cfg->resample_fn > 3) ARGFAIL("bssm_pf_run: unknown resample_fn");
    if (cfg->resample_fn == BSSM_MULTINOMIAL_R && !cfg->u_res) ARGFAIL("bssm_pf_run: BSSM_MULTINOMIAL_R replays R's unif_rand() stream: u_res is required");
    if (!cfg->theta || cfg->n_theta < 3) ARGFAIL("bssm_pf_run: theta must hold (phi, sigma_x, sigma_y) or (lambda, gamma, n_total, s0, i0)");
    if (T > 0 && !cfg->y) ARGFAIL("bssm_pf_run: y is NULL");
    if (!res->state_est || !res->ess || !res->loglike || (T > 0 && !res->loglike_history)) ARGFAIL("bssm_pf_run: result buffers missing");
    for (int i = 0; i < T; i++) if (!isfinite(cfg->y[i])) ARGFAIL("Assertion on 'y' failed: Contains missing values");  // assert_numeric(y, any.missing = FALSE) :69
    return obs_times_check(cfg->obs_times, T);
}

// One observation of the fused path (fused.hip.h): the gap's transitions but the last in launches of their own, then k_obs -- the
// last transition, the weights, the resolves and the expansion of X0 into X1 in one launch.  z_ready: the normals of the coming
// fused transition when the previous launch drew them (fused_prefetch), taken and, for the next launch, set here.
static int fused_obs(bssm_ctx* c, const bssm_pf_config* cfg, const PfRun& run, ObsClock& clk, int i, const ModelPar& par,
                     const double* zt, const double*& z_ready, double* X0, double* X1, double* se_row)
{
    const long long N = run.N;
    const double yi = cfg->y[i - 1];
    for (int step = 1; step < clk.gap; step++) launch_step_model(c, cfg->model, true, 0, false, X0, N, run.B, par, yi, trans_noise(run, zt, clk.ktrans++));
    FusedArgs g;
    g.xin = X0; g.N = N; g.nblk = run.B; g.par = par; g.y = yi; g.trans = (clk.gap >= 1) ? 1 : 0; g.ns = trans_noise(run, zt, clk.gap >= 1 ? clk.ktrans : 0);
    if (clk.gap >= 1) clk.ktrans++;
    g.obs_i = i; g.resample_algorithm = run.resample_algorithm; g.threshold = run.threshold;
    g.ess_out = run.ess; g.llh_out = run.llh; g.resampled_out = run.resampled;
    g.w_out = cfg->return_particles ? c->w : nullptr;
    g.lim = rec_lim(c, N);
    g.force_fallback = c->opt_force_fallback; g.early_max = c->opt_fused_early_max;
    // the expansion as built: this path resamples stratified / systematic only and carries nothing auxiliary, so nstage is 1 or 0
    g.a = apply_args(c, c->w, N, (int)N, run.B, run.ur, run.u_stride, run.key, run.anc, run.anc_stride, X0, X1, 1, N, se_row);
    g.ws = c->fz; g.tag = ++c->fz_tag;
    if (g.tag == 0) {
        // the launch counter wrapped: tag 0 is what every never-written granule carries, and the granules of the launches 2^32
        // ago would validate as this run's -- zero the workspace (stream-ordered behind the launches before) and count from 1
        HIPCHK(hipMemsetAsync(c->fz, 0, sizeof(FusedWs), c->stream));
        g.tag = c->fz_tag = 1;
    }
    // the normals of the NEXT fused transition are drawn inside this launch, in the time its workgroups wait for the resolver
    // (device generator only; injected draws are arrays already); two buffers alternate (this launch reads one, fills the other)
    g.znext = nullptr; g.znext_call = 0;
    if (z_ready) { g.ns.arr = z_ready; z_ready = nullptr; }
    if (!zt && c->opt_fused_prefetch && clk.gap_after(i) >= 1) {
        g.znext = (i & 1) ? c->auxlw : c->auxg; g.znext_call = (uint32_t)(clk.ktrans + clk.gap_after(i) - 1);
        z_ready = g.znext;
    }
    c->fz_launches++;
    const bool sysk = cfg->resample_fn == BSSM_SYSTEMATIC;
    if (cfg->model == BSSM_MODEL_LG) { if (sysk) LAUNCH(c, "k_obs<systematic>", (k_obs<0, 1>), run.B, NT, FZ_DYN_LDS, g, c->st); else LAUNCH(c, "k_obs<stratified>", (k_obs<0, 0>), run.B, NT, FZ_DYN_LDS, g, c->st); }
    else { if (sysk) LAUNCH(c, "k_obs<systematic>", (k_obs<1, 1>), run.B, NT, FZ_DYN_LDS, g, c->st); else LAUNCH(c, "k_obs<stratified>", (k_obs<1, 0>), run.B, NT, FZ_DYN_LDS, g, c->st); }
    return BSSM_OK;
}

static int pf_run_impl(bssm_ctx* c, const bssm_pf_config* cfg, bssm_pf_result* res, bool allow_fused)
{
    int rc;
    if ((rc = pf_run_check(c, cfg, res))) return rc;
    HIPCHK(hipSetDevice(c->device));
    const long long N = cfg->num_particles;
    const int T = cfg->T;
    const bool sir = cfg->model == BSSM_MODEL_SIR, apf = cfg->algorithm == BSSM_APF, rmpf = cfg->algorithm == BSSM_RMPF;
    const int dim = sir ? 2 : 1;
    PfRun run;
    if ((rc = pf_run_setup(c, cfg, res, dim, false, run))) return rc;
    const int B = run.B;
    const double *d_zi = nullptr, *d_zt = nullptr, *d_zmv = nullptr, *d_umv = nullptr;
    if (cfg->z_init && (rc = pool_put(c, "zi", cfg->z_init, (size_t)N * 8, &d_zi))) return rc;
    if (cfg->z_trans && run.max_trans > 0 && (rc = pool_put(c, "zt", cfg->z_trans, (size_t)run.max_trans * N * 8, &d_zt))) return rc;
    if (rmpf && cfg->z_move && T > 0) {
        if ((rc = pool_put(c, "zmv", cfg->z_move, (size_t)T * N * 8, &d_zmv))) return rc;
        if ((rc = pool_put(c, "umv", cfg->u_move, (size_t)T * N * 8, &d_umv))) return rc;
    }
    GmaxSlots gm;                                        // (two weight evaluations per observation in the auxiliary filter)
    if ((rc = gm.take(c, (size_t)2 * T + 2, c->stream))) return rc;
    auto next_gmax = [&]() { c->gmax_cur = gm.next(); };

    ModelPar par = scalar_par(cfg->model, cfg->theta);
    double* X0 = c->x0; double* X1 = c->x1;

    HIPCHK(hipEventRecord(c->ev0, c->stream));
    LAUNCH(c, "k_reset_state", k_reset_state, 1, 1, 0, c->st);
    if (c->opt_debug_stop) hipLaunchKernelGGL(k_set_debug, dim3(1), dim3(1), 0, c->stream, c->st, c->opt_debug_stop);
    // t = 0  (:76-116)
    LAUNCH(c, "k_init", k_init, B, NT, 0, X0, N, noise_src(d_zi, run.key, DRAW_INIT, 0), run.separt, cfg->model, par, 0);
    if (cfg->return_particles && (rc = pf_run_seed_history(c, run, X0))) return rc;
    ObsClock clk(cfg->obs_times, T);
    bool stepped_ahead = false;
    const double* z_ready = nullptr;      // fused path: the normals of the coming fused transition, drawn by the previous launch
    // bootstrap / resample-move filter on the Gaussian-observation models: k_step does not store the log-weights, k_weights
    // re-evaluates dnorm(y, x) on the particles (8 MB less written per observation at N = 2^20, the same 8 MB read)
    const bool relw = c->opt_recompute_lw && !apf && !sir && !c->opt_fuse_step;
    // one launch per observation (fused.hip.h): bootstrap / resample-move filter, scalar Gaussian-observation model, stratified or
    // systematic resampling, at most 512 blocks; the A/B and test switches that select other kernels keep the multi-launch path
    // (grids of at most FZ_MINB blocks -- one workgroup per CU -- stay on the multi-launch path unless the option is 2: the fused launch's three
    //  in-launch hand-offs cost the same whatever N is, the multi-launch kernels shrink with N: 46.9 vs 43.2 us per observation at 256 blocks,
    //  44.1 vs 47.8 at 320: tools/diag_fused_threshold.py)
    const bool fused = allow_fused && c->fz_ok && c->opt_fused && (B > FZ_MINB || c->opt_fused >= 2) && !apf && !sir && B <= FZ_MAXB && !c->sh_nloc && c->opt_renormalize &&
                       !c->opt_fuse_step && c->opt_inkernel_resolve &&
                       (cfg->resample_fn == BSSM_STRATIFIED || cfg->resample_fn == BSSM_SYSTEMATIC);
    if (fused) c->fz_runs++;
    for (int i = 1; i <= T; i++) {                                                        // :123
        clk.advance(i);
        const int gap = clk.gap;                                                          // :124
        const double yi = cfg->y[i - 1];
        if (sir) par.lgy = lgamma(yi + 1.0);
        double* se_row = run.separt + (size_t)i * B * dim;
        auto move_and_record = [&]() {   // (RMPF) move every particle, then take the state estimate (:226-241); the history row
            const double* zm = d_zmv ? d_zmv + (size_t)(i - 1) * N : nullptr;
            const double* um = d_umv ? d_umv + (size_t)(i - 1) * N : nullptr;
            if (rmpf && cfg->model == BSSM_MODEL_LG) LAUNCH(c, "k_move", k_move<0>, B, NT, 0, X0, N, par, yi, cfg->move_sd, zm, um, run.key, (uint32_t)i, se_row, c->st);
            else if (rmpf) LAUNCH(c, "k_move", k_move<1>, B, NT, 0, X0, N, par, yi, cfg->move_sd, zm, um, run.key, (uint32_t)i, se_row, c->st);
            if (cfg->return_particles)
                LAUNCH(c, "k_record_history", k_record_history, (unsigned)((N + 255) / 256), 256, 0, X0, c->w, N, dim,
                       run.ph + (size_t)i * N * dim, run.wh + (size_t)i * N, c->st);
        };
        if (fused) {
            if ((rc = fused_obs(c, cfg, run, clk, i, par, d_zt, z_ready, X0, X1, se_row))) return rc;
            std::swap(X0, X1);
            move_and_record();
            note_calls(c, run, i);
            continue;
        }
        ResampleLaunch r;
        r.d_w = c->w; r.nw = N; r.n = (int)N; r.kind = cfg->resample_fn; r.d_u = run.ur; r.u_stride = run.u_stride; r.key = run.key;
        r.d_anc = run.anc; r.anc_stride = N; r.d_cum = nullptr; r.dim = dim; r.xstride = N;
        // gap transitions; the last one is fused with the weight evaluation unless APF  (:125-136)
        if (stepped_ahead) {
            // this observation's (single) transition and its log-weights were computed inside the previous observation's
            // expansion kernel; what is left of k_step are the per-block log-sum-exp partials
            next_gmax();
            LAUNCH(c, "k_lw_partials", k_lw_partials, B, NTS, 0, c->lw, N, c->pm, c->ps, c->pq, c->gmax_cur);
            clk.ktrans++;
        } else for (int step = 1; step <= gap; step++) {
            const bool fuse_w = (!apf && step == gap);
            if (fuse_w) next_gmax();
            launch_step_model(c, cfg->model, true, fuse_w ? 1 : 0, false, X0, N, B, par, yi, trans_noise(run, d_zt, clk.ktrans++), !relw);
        }
        // can the NEXT observation's transition + weight ride along with this observation's expansion?  (bootstrap filter
        // that resamples at every observation, a single transition to the next observation, nothing that needs the
        // resampled particles themselves in HBM)
        stepped_ahead = c->opt_fuse_step && !apf && !rmpf && !sir && run.resample_algorithm == BSSM_SISR && !cfg->return_particles &&
                        !cfg->return_ancestors && (cfg->resample_fn == BSSM_STRATIFIED || cfg->resample_fn == BSSM_SYSTEMATIC) && clk.gap_after(i) == 1;
        if (apf) {                                                                        // :140-175
            next_gmax();
            launch_step_model(c, cfg->model, false, 2, false, X0, N, B, par, yi, trans_noise(run, d_zt, 0));
            r.d_lw = c->auxlw; r.plan = PLAN_AUX; r.check_degenerate = 0; r.obs_i = i;
            r.xsrc = X0; r.xdst = X1; r.auxsrc = c->auxlw; r.auxdst = c->auxg; r.se_part = nullptr;
            launch_scan_and_apply(c, r);
            std::swap(X0, X1);
            next_gmax();
            launch_step_model(c, cfg->model, true, 1, true, X0, N, B, par, yi, trans_noise(run, d_zt, clk.ktrans++));   // :159-175
        } else if (gap <= 0) {
            // obs_times repeats a time: no transition, weights on the current particles
            next_gmax();
            launch_step_model(c, cfg->model, false, 1, false, X0, N, B, par, yi, trans_noise(run, d_zt, 0), !relw);
        }
        // normalise (:204-207) + loglik/ESS/decision (:208-218) + resample (:220-224), fused into the scan kernels
        r.d_lw = c->lw; r.plan = PLAN_PF; r.check_degenerate = 1; r.obs_i = i; r.resample_algorithm = run.resample_algorithm;
        if (relw) { r.xw = X0; r.yw = yi; r.syw = par.sy; r.lsyw = par.log_sy; }
        r.threshold = run.threshold; r.d_ess = run.ess; r.d_llh = run.llh; r.d_resampled = run.resampled;
        r.xsrc = X0; r.xdst = X1; r.auxsrc = nullptr; r.auxdst = nullptr; r.se_part = se_row;
        if (stepped_ahead) { r.step_model = cfg->model; r.step_par = par; r.step_y = cfg->y[i]; r.step_ns = trans_noise(run, d_zt, clk.ktrans); }
        launch_scan_and_apply(c, r);
        if (run.resample_algorithm != BSSM_SISR)
            LAUNCH(c, "k_carry", k_carry, B, NT, 0, X0, X1, c->w, N, dim, se_row, c->st, 0);
        std::swap(X0, X1);
        move_and_record();
        note_calls(c, run, i);
    }
    DevState h;
    if ((rc = pf_run_finish(c, run, res, h))) return rc;
    if (fused && (h.flags & (FLAG_FUSED_BAIL | FLAG_FUSED_TIMEOUT))) {      // (before the first scalar of res is written)
        if (h.flags & FLAG_FUSED_BAIL) c->fz_bails++; else c->fz_timeouts++;
        return BSSM_RETRY_UNFUSED;
    }
    return pf_run_results(c, cfg, run, h, true, res);
}


// ---- multivariate linear-Gaussian family (mv.hip.h): bootstrap, auxiliary and resample-move filters, d <= 8 -----------------
// cfg->theta: the packed block  d, p, m0[d], L0[d d], A[d d], b[d], L[d d], c0, H[p d], h0[p], sd[p];  cfg->y: [T][p] row-major
// (unused when p == 0);  injected draws: z_init [d][N], z_trans [calls][d][N] (component-major), u_res as for the scalar models,
// z_move [T][d][N] and u_move [T][N] (RMPF).  The loop (pf_run_family, shared with the reaction networks) follows pf_run_impl's
// multi-launch path call for call: the same transition-call and resample-call numbering, so the draws of a run are keyed exactly
// as the scalar models' are.  Set-up and read-back are the scalar runner's (pf_run_setup, pf_run_finish, pf_run_results).
// bssm_mv_tv of a run with T observations of a (d, p) model: n_times covers the last observation time, finite values, no
// observation pieces without observations.  (obs_times has been checked: sorted, >= 1.)  who: the entry point, for the message.
// The same for the array sets of bssm_mv_tv_batch (F filters): every set is checked; a stride is 0 (one shared array) or a set's
// full size; the set indices lie in [0, n_sets).  mv_tv_check is the one-set case.
static int mv_tvb_check(const char* who, const bssm_pf_config* cfg, int d, int p, int F, const bssm_mv_tv_batch* tv)
{
    const int T = cfg->T;
    const std::string W = std::string(who) + ": mv_tv: ";
    if (p == 0 && (tv->h0_t || tv->H_t)) ARGFAIL(W + "h0_t / H_t given for a model without observation components (p == 0)");
    const int G = tv->n_sets;
    if (G < 1) ARGFAIL(W + "n_sets must be >= 1");
    if (tv->set_of) { for (int f = 0; f < F; f++) if (tv->set_of[f] < 0 || tv->set_of[f] >= G) ARGFAIL(W + "set_of holds an index outside [0, n_sets)"); }
    else if (G != 1 && G != F) ARGFAIL(W + "without set_of, n_sets must be n_filters (filter f uses set f) or 1");
    const size_t n_b = (size_t)std::max(tv->n_times, 0) * d, n_h0 = (size_t)T * p, n_H = (size_t)T * p * d;
    if ((tv->b_t && tv->b_stride != 0 && tv->b_stride != (long long)n_b) || (tv->h0_t && tv->h0_stride != 0 && tv->h0_stride != (long long)n_h0) ||
        (tv->H_t && tv->H_stride != 0 && tv->H_stride != (long long)n_H))
        ARGFAIL(W + "a stride must be 0 (one shared array) or the full size of one set");
    if (tv->b_t) {
        const int last = T > 0 ? (cfg->obs_times ? cfg->obs_times[T - 1] : T) : 0;
        if (tv->n_times < last) ARGFAIL(W + "n_times must cover the last observation time");
        for (size_t i = 0; i < n_b * (tv->b_stride ? G : 1); i++) if (!isfinite(tv->b_t[i])) ARGFAIL(W + "b_t contains non-finite values");
    }
    if (tv->h0_t) for (size_t i = 0; i < n_h0 * (tv->h0_stride ? G : 1); i++) if (!isfinite(tv->h0_t[i])) ARGFAIL(W + "h0_t contains non-finite values");
    if (tv->H_t) for (size_t i = 0; i < n_H * (tv->H_stride ? G : 1); i++) if (!isfinite(tv->H_t[i])) ARGFAIL(W + "H_t contains non-finite values");
    return BSSM_OK;
}

static bssm_mv_tv_batch mv_tv_as_batch(const bssm_mv_tv* tv)
{
    bssm_mv_tv_batch b;
    b.n_times = tv->n_times; b.n_sets = 1; b.set_of = nullptr;
    b.b_t = tv->b_t; b.b_stride = 0; b.h0_t = tv->h0_t; b.h0_stride = 0; b.H_t = tv->H_t; b.H_stride = 0;
    return b;
}

static int mv_tv_check(const char* who, const bssm_pf_config* cfg, int d, int p)
{
    if (!cfg->mv_tv) return BSSM_OK;
    const bssm_mv_tv_batch one = mv_tv_as_batch(cfg->mv_tv);
    return mv_tvb_check(who, cfg, d, p, 1, &one);
}

// the observation family of a multivariate model id (-1: another model)
static int mv_obs_of(int model)
{
    return model == BSSM_MODEL_LGMV ? MV_OBS_GAUSS : model == BSSM_MODEL_LGMV_POIS ? MV_OBS_POIS : model == BSSM_MODEL_LGMV_LOGVAR ? MV_OBS_LOGVAR : -1;
}
// y [T][p] of the family holds no missing value; with the context option mv_y_missing a NaN is a component that was not observed
// (skip) and only +-inf is refused
static int mv_y_check(const double* y, int n, bool skip)
{
    for (int i = 0; i < n; i++) if (!isfinite(y[i]) && !(skip && isnan(y[i]))) ARGFAIL("Assertion on 'y' failed: Contains missing values");
    return BSSM_OK;
}
// what the non-Gaussian families ask of (p, y) beyond the family's common checks: p >= 1; Poisson counts (finite, >= 0, integral);
// skip: the entries that were not observed (NaN, let through by mv_y_check) are no counts
static int mv_obs_check(const std::string& W, int obs, int p, const double* y, int T, bool skip)
{
    if (obs == MV_OBS_GAUSS) return BSSM_OK;
    if (p < 1) ARGFAIL(W + "multivariate model: the Poisson / log-variance observation families need p >= 1");
    if (obs == MV_OBS_POIS)
        for (int i = 0; i < T * p; i++) {
            if (skip && isnan(y[i])) continue;
            if (!isfinite(y[i]) || y[i] < 0.0 || y[i] != floor(y[i])) ARGFAIL(W + "multivariate model: Poisson observations must be finite non-negative integers");
        }
    return BSSM_OK;
}
// the Poisson family's table entry: lgamma(y + 1), 0.0 where y was not observed (never read: mv_observed)
static double mv_lgy(double y) { return isnan(y) ? 0.0 : lgamma(y + 1.0); }
// the device's parameter block of one filter: the caller's packed block, then log(sd)[p] taken on the host (like log(sigma_y) of the
// scalar models) for the Gaussian family; the other families read neither sd nor log(sd), whose slots are then 0.  dst: mp.size() doubles.
static void mv_fill_block(double* dst, const double* theta, const MvPar& mp, int obs)
{
    memcpy(dst, theta, (size_t)mp.o_lsd() * 8);
    for (int k = 0; k < mp.p; k++) dst[mp.o_lsd() + k] = obs == MV_OBS_GAUSS ? log(theta[mp.o_sd() + k]) : 0.0;
}

// The observation loop of the multivariate and the reaction-network families (R/particle_filter_core.R:123-241).  FAM (MvFamily,
// RnFamily) launches its own kernels under its own profile names: row(i) takes the data rows of observation i, then the five steps
// (call: the transition's number, first: the first one since the previous observation, tau: the time it reaches or the
// observation's), the gather along the ancestors of the resample call in flight (aux: the first stage's, which carries the
// auxiliary log-weights along) and the move (RMPF; a family without one is never asked).
template <class FAM>
static void pf_run_family(bssm_ctx* c, const bssm_pf_config* cfg, const PfRun& run, FAM& fam)
{
    const long long N = run.N;
    const int T = run.T, B = run.B, d = run.dim;
    const bool apf = cfg->algorithm == BSSM_APF, rmpf = cfg->algorithm == BSSM_RMPF;
    double* X0 = c->x0; double* X1 = c->x1;
    ObsClock clk(cfg->obs_times, T);
    for (int i = 1; i <= T; i++) {                                                        // :123
        clk.advance(i);
        const int ot = clk.ot, gap = clk.gap;                                             // :124
        fam.row(i);
        auto resample = [&](const double* lw, int plan) {                                // ancestors only; the gather follows
            ResampleLaunch r;
            r.d_lw = lw; r.plan = plan; r.check_degenerate = plan == PLAN_PF ? 1 : 0; r.obs_i = i; r.resample_algorithm = run.resample_algorithm; r.threshold = run.threshold;
            r.d_ess = run.ess; r.d_llh = run.llh; r.d_resampled = run.resampled;
            r.d_w = c->w; r.nw = N; r.n = (int)N; r.kind = cfg->resample_fn; r.d_u = run.ur; r.u_stride = run.u_stride; r.key = run.key;
            r.d_anc = run.anc; r.anc_stride = run.anc_stride; r.d_cum = nullptr;
            launch_scan_and_apply(c, r);
        };
        for (int step = 1; step <= gap; step++) {                                         // :125-136, the last one fused with weight_fn (:177-183) unless APF
            const int tau = ot - gap + step;                                              // the transition to prev_t + step
            if (step == gap && !apf) fam.trans_weight(X0, clk.ktrans++, step == 1, tau);
            else fam.trans(X0, clk.ktrans++, step == 1, tau);
        }
        if (apf) {                                                                        // :140-175
            fam.aux_weight(X0, ot);
            resample(c->auxlw, PLAN_AUX);                                                 // :152-155
            fam.gather(true, X0, X1, nullptr);                                            // :157, aux_log_weights[indices]
            std::swap(X0, X1);
            fam.trans_weight_aux(X0, clk.ktrans++, ot);                                   // :159-175
        } else if (gap <= 0) fam.weight(X0, ot);
        double* se_row = run.separt + (size_t)i * B * d;
        resample(c->lw, PLAN_PF);                                                         // :204-224
        fam.gather(false, X0, X1, se_row);                                                // particles[indices, ]
        if (run.resample_algorithm != BSSM_SISR) LAUNCH(c, "k_carry_mv", k_carry_mv, B, NT, 0, X0, X1, c->w, N, d, se_row, c->st);
        std::swap(X0, X1);
        if (rmpf) fam.move(X0, ot, se_row);                                           // move every particle, then take the state estimate (:226-241)
        if (cfg->return_particles)
            LAUNCH(c, "k_record_history", k_record_history, (unsigned)((N + 255) / 256), 256, 0, X0, c->w, N, d,
                   run.ph + (size_t)i * N * d, run.wh + (size_t)i * N, c->st);
        note_calls(c, run, i);
    }
}

// (device copies; nullptr: not given.  tv_at: the rows of this observation -- h0 / H by observation row, b by the absolute time the
//  transition reaches)
template <int OBS>
struct MvFamily {
    bssm_ctx* c; const PfRun& run; MvPar mp; double move_sd;
    const double *y, *lgy, *bt, *h0t, *Ht, *zt, *zmv, *umv;
    int i = 0; const double *yrow = nullptr, *lgyrow = nullptr;
    void row(int i_) { i = i_; yrow = mp.p > 0 ? y + (size_t)(i - 1) * mp.p : nullptr; lgyrow = lgy ? lgy + (size_t)(i - 1) * mp.p : nullptr; }
    MvTv tv_at(int tau) const
    {
        MvTv tv;
        tv.b = (bt && tau >= 1) ? bt + (size_t)(tau - 1) * mp.d : nullptr;
        tv.h0 = h0t ? h0t + (size_t)(i - 1) * mp.p : nullptr;
        tv.H = Ht ? Ht + (size_t)(i - 1) * mp.p * mp.d : nullptr;
        return tv;
    }
    MvNoise noise(int k) const { MvNoise ns; ns.arr = zt ? zt + (size_t)k * run.N * mp.d : nullptr; ns.key = run.key; ns.purpose = DRAW_TRANS; ns.call = (uint32_t)k; return ns; }
#define STEP_MV(NAME, TR, WT, SA, LW, TAU, CALL) \
        LAUNCH(c, NAME, (k_step_mv<TR, WT, SA, OBS>), run.B, NTS, 0, X0, LW, c->auxg, run.N, mp, tv_at(TAU), yrow, lgyrow, noise(CALL), c->pm, c->ps, c->pq, (unsigned long long*)nullptr)
    void trans(double* X0, int call, bool, int tau) { STEP_MV("k_step_mv<trans>", true, 0, false, c->lw, tau, call); }
    void trans_weight(double* X0, int call, bool, int tau) { STEP_MV("k_step_mv<trans+weight>", true, 1, false, c->lw, tau, call); }
    void aux_weight(double* X0, int ot) { STEP_MV("k_step_mv<aux-weight>", false, 2, false, c->auxlw, ot, 0); }
    void trans_weight_aux(double* X0, int call, int ot) { STEP_MV("k_step_mv<trans+weight-aux>", true, 1, true, c->lw, ot, call); }
    void weight(double* X0, int ot) { STEP_MV("k_step_mv<weight>", false, 1, false, c->lw, ot, 0); }
#undef STEP_MV
    void gather(bool aux, const double* X0, double* X1, double* se_row)
    {
        if (aux) LAUNCH(c, "k_gather_mv<aux>", k_gather_mv, run.B, NT, 0, (const int*)run.anc, run.anc_stride, run.N, mp.d, X0, X1, (double*)nullptr, c->st, (const double*)c->auxlw, c->auxg);
        else LAUNCH(c, "k_gather_mv", k_gather_mv, run.B, NT, 0, (const int*)run.anc, run.anc_stride, run.N, mp.d, X0, X1, se_row, c->st, (const double*)nullptr, (double*)nullptr);
    }
    void move(double* X0, int ot, double* se_row)
    {
        const double* zm = zmv ? zmv + (size_t)(i - 1) * mp.d * run.N : nullptr;
        const double* um = umv ? umv + (size_t)(i - 1) * run.N : nullptr;
        LAUNCH(c, "k_move_mv", k_move_mv<OBS>, run.B, NT, 0, X0, run.N, mp, tv_at(ot), yrow, lgyrow, move_sd, zm, um, run.key, (uint32_t)i, se_row, (const DevState*)c->st);
    }
};

template <int OBS>
static int pf_run_mv(bssm_ctx* c, const bssm_pf_config* cfg, bssm_pf_result* res)
{
    const long long N = cfg->num_particles;
    const int T = cfg->T;
    if (N <= 0) ARGFAIL("num_particles must be a positive count");
    if (T < 0) ARGFAIL("bssm_pf_run: T must be >= 0");
    if (N > c->cap) { g_err = "bssm_pf_run: num_particles exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    if (!cfg->theta || cfg->n_theta < 2) ARGFAIL("bssm_pf_run: the multivariate model needs its packed parameter block");
    MvPar mp; mp.P = nullptr; mp.d = (int)cfg->theta[0]; mp.p = (int)cfg->theta[1];
    const int d = mp.d, p = mp.p;
    if (d < 1 || d > MVD || p < 0 || p > MVD) ARGFAIL("bssm_pf_run: multivariate model: 1 <= d <= 8, 0 <= p <= 8");
    if (cfg->n_theta != mp.o_lsd()) ARGFAIL("bssm_pf_run: multivariate model: parameter block has the wrong length");
    if (d > c->max_dim) { g_err = "bssm_pf_run: the context was created with a smaller max_dim than this model's state dimension"; return BSSM_ERR_CAPACITY; }
    if (cfg->algorithm != BSSM_BPF && cfg->algorithm != BSSM_APF && cfg->algorithm != BSSM_RMPF) ARGFAIL("bssm_pf_run: unknown algorithm");
    const bool rmpf = cfg->algorithm == BSSM_RMPF;
    if (rmpf && !(cfg->move_sd > 0)) ARGFAIL("bssm_pf_run: RMPF needs move_sd > 0");
    if (rmpf && ((cfg->z_move == nullptr) != (cfg->u_move == nullptr))) ARGFAIL("bssm_pf_run: z_move and u_move must be given together");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL("bssm_pf_run: unknown resample_algorithm");
    if (cfg->resample_fn != BSSM_STRATIFIED && cfg->resample_fn != BSSM_SYSTEMATIC) ARGFAIL("bssm_pf_run: the multivariate family resamples stratified / systematic");
    if (T > 0 && p > 0 && !cfg->y) ARGFAIL("bssm_pf_run: y is NULL");
    if (!res->state_est || !res->ess || !res->loglike || (T > 0 && !res->loglike_history)) ARGFAIL("bssm_pf_run: result buffers missing");
    const bool skip = c->opt_mv_y_missing != 0;
    { const int rc_y = mv_y_check(cfg->y, T * p, skip); if (rc_y) return rc_y; }
    if (OBS == MV_OBS_GAUSS) for (int k = 0; k < p; k++) if (!(cfg->theta[mp.o_sd() + k] > 0)) ARGFAIL("bssm_pf_run: multivariate model: observation sd must be positive");
    { const int rc_obs = mv_obs_check("bssm_pf_run: ", OBS, p, cfg->y, T, skip); if (rc_obs) return rc_obs; }
    if (int rc_o = obs_times_check(cfg->obs_times, T)) return rc_o;
    { const int rc_tv = mv_tv_check("bssm_pf_run", cfg, d, p); if (rc_tv) return rc_tv; }
    HIPCHK(hipSetDevice(c->device));
    PfRun run;
    int rc;
    if ((rc = pf_run_setup(c, cfg, res, d, true, run))) return rc;
    MvFamily<OBS> fam{c, run, mp, cfg->move_sd, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<double> hp((size_t)mp.size());
    mv_fill_block(hp.data(), cfg->theta, mp, OBS);
    if ((rc = pool_put(c, "mv_par", hp.data(), hp.size() * 8, &fam.mp.P))) return rc;
    if (p > 0 && T > 0 && (rc = pool_put(c, "mv_y", cfg->y, (size_t)T * p * 8, &fam.y))) return rc;
    std::vector<double> hlgy;                                                    // Poisson: lgamma(y + 1) per (t, k), taken on the host as the SIR model's
    if (OBS == MV_OBS_POIS && T > 0) {
        hlgy.resize((size_t)T * p);
        for (size_t i = 0; i < hlgy.size(); i++) hlgy[i] = mv_lgy(cfg->y[i]);
        if ((rc = pool_put(c, "mv_lgy", hlgy.data(), hlgy.size() * 8, &fam.lgy))) return rc;
    }
    if (cfg->mv_tv && T > 0) {                                                   // time-varying pieces: data, uploaded like y
        const bssm_mv_tv* tv = cfg->mv_tv;
        if (tv->b_t && tv->n_times > 0 && (rc = pool_put(c, "mv_bt", tv->b_t, (size_t)tv->n_times * d * 8, &fam.bt))) return rc;
        if (tv->h0_t && (rc = pool_put(c, "mv_h0t", tv->h0_t, (size_t)T * p * 8, &fam.h0t))) return rc;
        if (tv->H_t && (rc = pool_put(c, "mv_Ht", tv->H_t, (size_t)T * p * d * 8, &fam.Ht))) return rc;
    }
    const double* d_zi = nullptr;
    if (cfg->z_init && (rc = pool_put(c, "zi", cfg->z_init, (size_t)N * d * 8, &d_zi))) return rc;
    if (cfg->z_trans && run.max_trans > 0 && (rc = pool_put(c, "zt", cfg->z_trans, (size_t)run.max_trans * N * d * 8, &fam.zt))) return rc;
    if (rmpf && cfg->z_move && T > 0) {
        if ((rc = pool_put(c, "zmv", cfg->z_move, (size_t)T * d * N * 8, &fam.zmv))) return rc;
        if ((rc = pool_put(c, "umv", cfg->u_move, (size_t)T * N * 8, &fam.umv))) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));                 // (hp and hlgy live on this stack frame)
    c->gmax_cur = nullptr;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    LAUNCH(c, "k_reset_state", k_reset_state, 1, 1, 0, c->st);
    {
        MvNoise ns; ns.arr = d_zi; ns.key = run.key; ns.purpose = DRAW_INIT; ns.call = 0;
        LAUNCH(c, "k_init_mv", k_init_mv, run.B, NT, 0, c->x0, N, fam.mp, ns, run.separt);
        if (cfg->return_particles && (rc = pf_run_seed_history(c, run, c->x0))) return rc;
    }
    pf_run_family(c, cfg, run, fam);
    DevState h;
    if ((rc = pf_run_finish(c, run, res, h))) return rc;
    return pf_run_results(c, cfg, run, h, true, res);
}

// ---- mass-action reaction networks (rnet.hip.h): bootstrap and auxiliary filters, d <= 8 species, R <= 8 reactions, p <= 8 ----------
// cfg->theta: the packed block  d, R, p, x0[d], k[R], s1[R], s2[R], nu[R][d], G[p][d], then optionally reset[d] of 0.0 / 1.0 (the
// counter species, rnet.hip.h), then optionally n_times, M[n_times][R] (the rate schedule, rnet.hip.h; only after reset[d]);  cfg->y: [T][p] counts, with the context option mv_y_missing NaN where a component was not observed;
// u_res as for the other models.  The loop is pf_run_family, the multivariate family's too: one transition-call and resample-call numbering for both.
// BSSM_MODEL_RNET_NB (nb): the same block with size[p] directly after G[p][d], in front of the tails; every length below moves by p.
// The block of one filter, checked (who: the entry point with ": ", for the message); rp gets d, R, p, nsz, tail and n_times.
// gwn: the context option rn_noise -- the block carries lead[R], sigma[R] directly after size[nsz] (rnet.hip.h); every length below moves by 2 R.
static int rn_block_check(const std::string& W, const double* th, int n_theta, RnPar& rp, bool nb, bool gwn)
{
    if (!th || n_theta < 3) ARGFAIL(W + "the reaction-network model needs its packed parameter block");
    rp.P = nullptr; rp.d = rp.R = rp.p = rp.tail = rp.n_times = rp.nsz = rp.nnz = 0;
    // (the header is compared as doubles: a NaN or a huge value must not reach a conversion to int)
    if (!(th[0] >= 1 && th[0] <= MVD && th[1] >= 1 && th[1] <= RNR && th[2] >= 1 && th[2] <= MVD) || th[0] != floor(th[0]) || th[1] != floor(th[1]) || th[2] != floor(th[2]))
        ARGFAIL(W + "reaction network: 1 <= d <= 8 species, 1 <= R <= 8 reactions, 1 <= p <= 8 observation components");
    rp.d = (int)th[0]; rp.R = (int)th[1]; rp.p = (int)th[2];
    rp.nsz = nb ? rp.p : 0;
    rp.nnz = gwn ? 2 * rp.R : 0;
    const int d = rp.d, R = rp.R;
    if (n_theta > rp.size_tail() + 1) {                                          // the rate schedule: n_times, M[n_times][R] after reset[d]
        const double nt = th[rp.size_tail()];
        if (!(nt >= 1) || nt != floor(nt) || nt > (double)(n_theta - rp.size_tail() - 1) || (long long)nt * R != (long long)(n_theta - rp.size_tail() - 1))
            ARGFAIL(W + "reaction network: parameter block has the wrong length (the rate schedule's n_times entry and the block's length disagree)");
        rp.n_times = (int)nt;
    }
    else if (n_theta != rp.size() && n_theta != rp.size_tail()) ARGFAIL(W + "reaction network: parameter block has the wrong length");
    rp.tail = n_theta != rp.size() ? 1 : 0;
    for (int k = 0; k < rp.nsz; k++)
        if (!isfinite(th[rp.o_size() + k]) || !(th[rp.o_size() + k] > 0)) ARGFAIL(W + "reaction network: the negative-binomial sizes size[p] must be finite and > 0");
    for (int r = 0; r < rp.nnz / 2; r++) {                                       // (in front of the general finiteness test: a NaN sigma gets its own message)
        const double g = th[rp.o_lead() + r], sg = th[rp.o_sigma() + r];
        if (g != floor(g) || g < -1 || g >= R) ARGFAIL(W + "reaction network: a noise group's leader lead[r] must be -1 (no noise) or a reaction index 0 .. R-1");
        if (g < 0) continue;
        if (g > r || th[rp.o_lead() + (int)g] != g) ARGFAIL(W + "reaction network: a noise group's leader must be the lowest reaction index of its group (lead[g] == g, lead[r] <= r)");
        if (!isfinite(sg) || !(sg > 0)) ARGFAIL(W + "reaction network: a noise group's sigma must be finite and > 0");
        if (sg != th[rp.o_sigma() + (int)g]) ARGFAIL(W + "reaction network: the reactions of one noise group carry one sigma");
    }
    for (int i = 3; i < n_theta; i++) if (!isfinite(th[i])) ARGFAIL(W + "reaction network: the parameter block contains non-finite values");
    for (int r = 0; r < R; r++) {
        const double s1 = th[rp.o_s1() + r], s2 = th[rp.o_s2() + r];
        if (s1 != floor(s1) || s2 != floor(s2) || s1 < -1 || s1 >= d || s2 < -1 || s2 >= d) ARGFAIL(W + "reaction network: a reactant index must be -1 (none) or a species 0 .. d-1");
        if (s1 < 0 && s2 >= 0) ARGFAIL(W + "reaction network: a first-order reaction names its reactant in s1 (s2 = -1)");
        if (s1 >= 0 && s1 == s2) ARGFAIL(W + "reaction network: s1 == s2 (dimerisation) is not supported");
        if (th[rp.o_k() + r] < 0) ARGFAIL(W + "reaction network: rate constants must be >= 0");
    }
    if (rp.tail) for (int c = 0; c < d; c++) {
        const double f = th[rp.o_reset() + c];
        if (f != 0.0 && f != 1.0) ARGFAIL(W + "reaction network: the counter flags reset[d] must be 0 or 1");
        if (f != 0.0) for (int r = 0; r < R; r++)
            if (th[rp.o_s1() + r] == c || th[rp.o_s2() + r] == c) ARGFAIL(W + "reaction network: a counter species may not be a reactant (the reset would change the dynamics)");
    }
    for (int i = 0; i < rp.n_times * R; i++)
        if (th[rp.o_sched() + i] < 0) ARGFAIL(W + "reaction network: the rate schedule's multipliers must be >= 0");
    return BSSM_OK;
}

// The Euler-multinomial method (rnet.hip.h, context option rn_method = 1): it needs rn_leaps = K >= 1, and every reaction of the block
// either has a source -- one reactant with nu == -1, the other reactant (if any) with nu >= 0 -- or is sourceless (no species with nu < 0)
static int rn_em_check(const std::string& W, const double* th, const RnPar& rp, int leaps)
{
    if (leaps < 1) ARGFAIL(W + "reaction network: rn_method = 1 (Euler-multinomial leaps) needs rn_leaps = K in 1 .. 1024");
    if (rp.nnz) {                                        // (rn_noise = 1: at least one group, or the option has nothing to say)
        bool any = false;
        for (int r = 0; r < rp.R; r++) any = any || th[rp.o_lead() + r] >= 0;
        if (!any) ARGFAIL(W + "reaction network: rn_noise = 1 (gamma white noise on the rates) with no noise group in the block (every lead[r] is -1)");
    }
    for (int r = 0; r < rp.R; r++) {
        const int s1 = (int)th[rp.o_s1() + r], s2 = (int)th[rp.o_s2() + r];
        const double* nu = th + rp.o_nu() + r * rp.d;
        const double n1 = s1 >= 0 ? nu[s1] : 0.0, n2 = s2 >= 0 ? nu[s2] : 0.0;
        if (n1 < 0.0 && n2 < 0.0)
            ARGFAIL(W + "reaction network: a reaction consumes both of its reactants (A + B -> C); the Euler-multinomial method splits the leavers of ONE compartment over its exits -- use tau-leaping (rn_method = 0 with rn_leaps = K) for such a network");
        if ((n1 < 0.0 && n1 != -1.0) || (n2 < 0.0 && n2 != -1.0))
            ARGFAIL(W + "reaction network: under the Euler-multinomial method a consumed reactant has nu == -1 (one individual leaves per firing)");
        for (int c = 0; c < rp.d; c++)
            if (c != s1 && c != s2 && nu[c] < 0.0) ARGFAIL(W + "reaction network: under the Euler-multinomial method only a reactant may have nu < 0");
    }
    return BSSM_OK;
}

// the schedule must reach the last observation time (T without obs_times)
static int rn_sched_check(const std::string& W, const RnPar& rp, int T, const int* obs_times)
{
    const int last = T > 0 ? (obs_times ? obs_times[T - 1] : T) : 0;
    if (rp.n_times && rp.n_times < last) ARGFAIL(W + "reaction network: the rate schedule's n_times is short of the last observation time");
    return BSSM_OK;
}

// the device copy of a block with a schedule: M[tau][r] becomes the product k_r * M[tau][r] (fp64, one rounding, what the kernel's own
// multiplication would give), so that a row is the rate vector of its moment (rnet.hip.h)
static void rn_sched_products(const RnPar& rp, double* blk)
{
    for (int t = 0; t < rp.n_times; t++)
        for (int r = 0; r < rp.R; r++) blk[rp.o_sched() + t * rp.R + r] = blk[rp.o_k() + r] * blk[rp.o_sched() + t * rp.R + r];
}

// the negative-binomial family's table entry (rnet.hip.h): c(t, k) = (lgamma(y + r) - lgamma(r)) - lgamma(y + 1), 0.0 where y was not
// observed (never read: mv_observed)
static double rn_nb_c(double y, double r) { return isnan(y) ? 0.0 : (lgamma(y + r) - lgamma(r)) - lgamma(y + 1.0); }

// the tables of F filters on one y [T][p]: out [F][T][p], filter f with the sizes at sizes + f * size_stride.  lgamma(r) and
// lgamma(y + 1) are taken once per (f, k) and per (t, k); the entries are rn_nb_c's bit for bit.  Exported for tools/bench_rnet_nb.py,
// which times the host's share of a batched call with it.
extern "C" int bssm_rn_nb_tables(const double* y, int T, int p, int n_filters, const double* sizes, long long size_stride, double* out)
{
    if (T < 0 || p < 1 || p > MVD || n_filters < 0 || ((T > 0 && n_filters > 0) && (!y || !sizes || !out))) ARGFAIL("bssm_rn_nb_tables: bad argument");
    if (T == 0 || n_filters == 0) return BSSM_OK;
    std::vector<double> lgy1((size_t)T * p);
    for (size_t i = 0; i < lgy1.size(); i++) lgy1[i] = isnan(y[i]) ? 0.0 : lgamma(y[i] + 1.0);
    for (int f = 0; f < n_filters; f++) {
        const double* r = sizes + (long long)f * size_stride;
        double lgr[MVD];
        for (int k = 0; k < p; k++) lgr[k] = lgamma(r[k]);
        double* o = out + (size_t)f * T * p;
        for (int t = 0; t < T; t++)
            for (int k = 0; k < p; k++) { const double yk = y[(size_t)t * p + k]; o[(size_t)t * p + k] = isnan(yk) ? 0.0 : (lgamma(yk + r[k]) - lgr[k]) - lgy1[(size_t)t * p + k]; }
    }
    return BSSM_OK;
}

// The family's kernels for pf_run_family.  y / lgy: the device copies of y [T][p] and of the table lgamma(y + 1) (nb: c(t, k)).
struct RnFamily {
    bssm_ctx* c; const PfRun& run; RnPar rp; bool nb, em, gwn; int leaps;
    const double *y, *lgy;
    const double *yrow = nullptr, *lgyrow = nullptr;
    void row(int i) { yrow = y + (size_t)(i - 1) * rp.p; lgyrow = lgy + (size_t)(i - 1) * rp.p; }
    // (SC: the instantiation that reads the schedule's row of the device copy; only the kernels that take propensities have one.
    //  OB: the observation family; only the kernels that take weights have a negative-binomial instantiation)
    //  MT: the transition method; only the kernels with a transition have a tau-leap instantiation (the context option rn_leaps, read
    //  once per run: leaps = K >= 1, or 0 for Gillespie's direct method; with the option rn_method = 1 (em) the K leaps are Euler-multinomial)
#define STEP_RN_MT(NAME, DM_, TR, WT, SA, SC, OB, MT, LW, CALL, FIRST, KROW) \
        LAUNCH(c, NAME, (k_step_rn<DM_, TR, WT, SA, SC, OB, MT>), run.B, NTS, 0, X0, LW, c->auxg, run.N, rp, yrow, lgyrow, run.key, (uint32_t)(CALL), (int)(FIRST), c->pm, c->ps, c->pq, (unsigned long long*)nullptr, KROW, leaps)
#define STEP_RN_DM(NAME, DM_, TR, WT, SA, SC, OB, LW, CALL, FIRST, KROW) do { \
        if (em && gwn && (TR)) STEP_RN_MT(NAME, DM_, TR, WT, SA, SC, OB, ((TR) ? RN_EULER_MULTINOM_GWN : RN_GILLESPIE), LW, CALL, FIRST, KROW); \
        else if (em && (TR)) STEP_RN_MT(NAME, DM_, TR, WT, SA, SC, OB, ((TR) ? RN_EULER_MULTINOM : RN_GILLESPIE), LW, CALL, FIRST, KROW); \
        else if (leaps > 0 && (TR)) STEP_RN_MT(NAME, DM_, TR, WT, SA, SC, OB, ((TR) ? RN_TAU_LEAP : RN_GILLESPIE), LW, CALL, FIRST, KROW); \
        else STEP_RN_MT(NAME, DM_, TR, WT, SA, SC, OB, RN_GILLESPIE, LW, CALL, FIRST, KROW); } while (0)
#define STEP_RN_OB(NAME, TR, WT, SA, SC, OB, LW, CALL, FIRST, KROW) do { \
        if (rp.d <= 2) STEP_RN_DM(NAME, 2, TR, WT, SA, SC, OB, LW, CALL, FIRST, KROW); \
        else if (rp.d <= 4) STEP_RN_DM(NAME, 4, TR, WT, SA, SC, OB, LW, CALL, FIRST, KROW); \
        else STEP_RN_DM(NAME, 8, TR, WT, SA, SC, OB, LW, CALL, FIRST, KROW); } while (0)
#define STEP_RN_SC(NAME, TR, WT, SA, SC, LW, CALL, FIRST, KROW) do { \
        if (nb && (WT) != 0) STEP_RN_OB(NAME, TR, WT, SA, SC, ((WT) != 0 ? RN_OBS_NB : RN_OBS_POIS), LW, CALL, FIRST, KROW); \
        else STEP_RN_OB(NAME, TR, WT, SA, SC, RN_OBS_POIS, LW, CALL, FIRST, KROW); } while (0)
#define STEP_RN(NAME, TR, WT, SA, LW, CALL, FIRST, TAU) do { \
        if (rp.n_times && ((TR) || (WT) == 2)) STEP_RN_SC(NAME, TR, WT, SA, ((TR) || (WT) == 2), LW, CALL, FIRST, rp.rates_row(TAU)); \
        else STEP_RN_SC(NAME, TR, WT, SA, false, LW, CALL, FIRST, (const double*)nullptr); } while (0)
    void trans(double* X0, int call, bool first, int tau) { STEP_RN("k_step_rn<trans>", true, 0, false, c->lw, call, first, tau); }     // (first: the counters start at 0.0)
    void trans_weight(double* X0, int call, bool first, int tau) { STEP_RN("k_step_rn<trans+weight>", true, 1, false, c->lw, call, first, tau); }
    void aux_weight(double* X0, int ot) { STEP_RN("k_step_rn<aux-weight>", false, 2, false, c->auxlw, 0, 0, ot); }     // (the Euler mean's propensities at the observation's time)
    void trans_weight_aux(double* X0, int call, int ot) { STEP_RN("k_step_rn<trans+weight-aux>", true, 1, true, c->lw, call, 0, ot); }     // (the second stage never resets)
    void weight(double* X0, int) { STEP_RN("k_step_rn<weight>", false, 1, false, c->lw, 0, 0, 1); }     // (reads no propensity)
#undef STEP_RN
#undef STEP_RN_SC
#undef STEP_RN_OB
#undef STEP_RN_DM
#undef STEP_RN_MT
    void gather(bool aux, const double* X0, double* X1, double* se_row)      // (groups the state estimate as the built-in SIR's expansion does)
    {
        if (aux) LAUNCH(c, "k_gather_rn<aux>", k_gather_rn, run.B, NT, 0, (const int*)run.anc, run.anc_stride, run.N, rp.d, X0, X1, (double*)nullptr, c->st, (const double*)c->auxlw, c->auxg);
        else LAUNCH(c, "k_gather_rn", k_gather_rn, run.B, NT, 0, (const int*)run.anc, run.anc_stride, run.N, rp.d, X0, X1, se_row, c->st, (const double*)nullptr, (double*)nullptr);
    }
    void move(double*, int, double*) {}      // (no move step: RMPF is refused)
};

// nb: BSSM_MODEL_RNET_NB -- the weight kernels are the negative-binomial instantiations and the table holds c(t, k)
static int pf_run_rn(bssm_ctx* c, const bssm_pf_config* cfg, bssm_pf_result* res, bool nb)
{
    const long long N = cfg->num_particles;
    const int T = cfg->T;
    if (N <= 0) ARGFAIL("num_particles must be a positive count");
    if (T < 0) ARGFAIL("bssm_pf_run: T must be >= 0");
    if (N > c->cap) { g_err = "bssm_pf_run: num_particles exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    RnPar rp;
    // (the context option rn_noise qualifies rn_method = 1: asked for under any other method it is refused here, before the block is read)
    if (c->opt_rn_noise && c->opt_rn_method != 1) ARGFAIL("bssm_pf_run: reaction network: rn_noise = 1 (gamma white noise on the rates) needs rn_method = 1 (Euler-multinomial leaps)");
    const bool gwn = c->opt_rn_noise != 0;
    { const int rc_b = rn_block_check("bssm_pf_run: ", cfg->theta, cfg->n_theta, rp, nb, gwn); if (rc_b) return rc_b; }
    const int d = rp.d, p = rp.p;
    if (d > c->max_dim) { g_err = "bssm_pf_run: the context was created with a smaller max_dim than this model's state dimension"; return BSSM_ERR_CAPACITY; }
    if (cfg->algorithm == BSSM_RMPF) ARGFAIL("bssm_pf_run: the reaction-network family has no move step (RMPF): a move on integer states is not defined");
    if (cfg->algorithm != BSSM_BPF && cfg->algorithm != BSSM_APF) ARGFAIL("bssm_pf_run: unknown algorithm");
    if (cfg->z_init || cfg->z_trans) ARGFAIL("bssm_pf_run: a reaction network draws a data-dependent number of variates; injected z_* are not supported");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL("bssm_pf_run: unknown resample_algorithm");
    if (cfg->resample_fn != BSSM_STRATIFIED && cfg->resample_fn != BSSM_SYSTEMATIC) ARGFAIL("bssm_pf_run: the reaction-network family resamples stratified / systematic");
    if (T > 0 && !cfg->y) ARGFAIL("bssm_pf_run: y is NULL");
    if (!res->state_est || !res->ess || !res->loglike || (T > 0 && !res->loglike_history)) ARGFAIL("bssm_pf_run: result buffers missing");
    const bool skip = c->opt_mv_y_missing != 0;
    { const int rc_y = mv_y_check(cfg->y, T * p, skip); if (rc_y) return rc_y; }
    { const int rc_obs = mv_obs_check("bssm_pf_run: ", MV_OBS_POIS, p, cfg->y, T, skip); if (rc_obs) return rc_obs; }
    if (int rc_o = obs_times_check(cfg->obs_times, T)) return rc_o;
    { const int rc_s = rn_sched_check("bssm_pf_run: ", rp, T, cfg->obs_times); if (rc_s) return rc_s; }
    const bool em = c->opt_rn_method == 1;               // (the context option rn_method: Euler-multinomial leaps, rn_leaps of them)
    if (em) { const int rc_e = rn_em_check("bssm_pf_run: ", cfg->theta, rp, c->opt_rn_leaps); if (rc_e) return rc_e; }
    HIPCHK(hipSetDevice(c->device));
    PfRun run;
    int rc;
    if ((rc = pf_run_setup(c, cfg, res, d, true, run))) return rc;
    RnFamily fam{c, run, rp, nb, em, gwn, c->opt_rn_leaps, nullptr, nullptr};
    std::vector<double> hblk;                                                    // (with a schedule: the copy that holds the products)
    if (rp.n_times) { hblk.assign(cfg->theta, cfg->theta + cfg->n_theta); rn_sched_products(rp, hblk.data()); }
    if ((rc = pool_put(c, "rn_par", rp.n_times ? hblk.data() : cfg->theta, (size_t)cfg->n_theta * 8, &fam.rp.P))) return rc;     // (with the tails, if any)
    std::vector<double> hlgy;                                                    // lgamma(y + 1) per (t, k), taken on the host as the SIR model's (nb: c(t, k))
    if (T > 0) {
        if ((rc = pool_put(c, "mv_y", cfg->y, (size_t)T * p * 8, &fam.y))) return rc;
        hlgy.resize((size_t)T * p);
        for (size_t i = 0; i < hlgy.size(); i++) hlgy[i] = nb ? rn_nb_c(cfg->y[i], cfg->theta[rp.o_size() + (int)(i % (size_t)p)]) : mv_lgy(cfg->y[i]);
        if ((rc = pool_put(c, "mv_lgy", hlgy.data(), hlgy.size() * 8, &fam.lgy))) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));                 // (hlgy and hblk live on this stack frame)
    c->gmax_cur = nullptr;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    LAUNCH(c, "k_reset_state", k_reset_state, 1, 1, 0, c->st);
    LAUNCH(c, "k_init_rn", k_init_rn, run.B, NT, 0, c->x0, N, fam.rp, run.separt);
    if (cfg->return_particles && (rc = pf_run_seed_history(c, run, c->x0))) return rc;
    pf_run_family(c, cfg, run, fam);
    DevState h;
    if ((rc = pf_run_finish(c, run, res, h))) return rc;
    return pf_run_results(c, cfg, run, h, true, res);
}

extern "C" int bssm_dump_rpois(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int call, int leap, int r, long long n,
                               const double* lam, double* out)
{
    if (!c || !lam || !out || n <= 0 || call < 0 || leap < 0 || leap >= RN_MAX_LEAPS || r < 0 || r >= RNR) ARGFAIL("bssm_dump_rpois: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void *dl, *d_; int rc;
    if ((rc = pool_get(c, "dump", (size_t)n * 8, &d_))) return rc;
    if ((rc = pool_put(c, "dump2", lam, (size_t)n * 8, &dl))) return rc;
    hipLaunchKernelGGL(k_dump_rpois, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, make_key(seed, stream), (uint32_t)call,
                       (uint32_t)(leap * RNR + r), n, (const double*)dl, (double*)d_);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

extern "C" int bssm_dump_rgamma(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int call, int leap, int g, long long n,
                                const double* shape, double* out)
{
    if (!c || !shape || !out || n <= 0 || call < 0 || leap < 0 || leap >= RN_MAX_LEAPS || g < 0 || g >= RNR) ARGFAIL("bssm_dump_rgamma: bad argument");
    for (long long i = 0; i < n; i++) if (!isfinite(shape[i]) || !(shape[i] > 0)) ARGFAIL("bssm_dump_rgamma: a shape must be finite and > 0");
    HIPCHK(hipSetDevice(c->device));
    void *ds, *d_; int rc;
    if ((rc = pool_get(c, "dump", (size_t)n * 8, &d_))) return rc;
    if ((rc = pool_put(c, "dump2", shape, (size_t)n * 8, &ds))) return rc;
    hipLaunchKernelGGL(k_dump_rgamma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, make_key(seed, stream), (uint32_t)call,
                       (uint32_t)(leap * RNR + g), n, (const double*)ds, (double*)d_);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

extern "C" int bssm_dump_rbinom(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int call, int leap, int r, long long n_draws,
                                const double* n, const double* q, double* out)
{
    if (!c || !n || !q || !out || n_draws <= 0 || call < 0 || leap < 0 || leap >= RN_MAX_LEAPS || r < 0 || r >= RNR) ARGFAIL("bssm_dump_rbinom: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void *dn, *dq, *d_; int rc;
    if ((rc = pool_get(c, "dump", (size_t)n_draws * 8, &d_))) return rc;
    if ((rc = pool_put(c, "dump2", n, (size_t)n_draws * 8, &dn))) return rc;
    if ((rc = pool_put(c, "dump3", q, (size_t)n_draws * 8, &dq))) return rc;
    hipLaunchKernelGGL(k_dump_rbinom, dim3((unsigned)((n_draws + 255) / 256)), dim3(256), 0, c->stream, make_key(seed, stream), (uint32_t)call,
                       (uint32_t)(leap * RNR + r), n_draws, (const double*)dn, (const double*)dq, (double*)d_);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_, (size_t)n_draws * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

extern "C" int bssm_dump_normals_mv(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int purpose, int call,
                                    long long N, int d, double* out /* [d][N] */)
{
    if (!c || !out || N <= 0 || d < 1 || d > MVD) ARGFAIL("bssm_dump_normals_mv: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void* dd; int rc = pool_get(c, "dump", (size_t)N * d * 8, &dd); if (rc) return rc;
    const long long pairs = (N + 1) / 2;
    hipLaunchKernelGGL(k_dump_normals_mv, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, c->stream, make_key(seed, stream), (uint32_t)purpose, (uint32_t)call, N, d, (double*)dd);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dd, (size_t)N * d * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

extern "C" int bssm_dump_move_draws_mv(bssm_ctx* c, unsigned long long seed, unsigned long long stream, int call, long long N, int d,
                                       double* z_out /* [d][N] */, double* u_out /* [N] */)
{
    if (!c || !z_out || !u_out || N <= 0 || d < 1 || d > MVD) ARGFAIL("bssm_dump_move_draws_mv: bad argument");
    HIPCHK(hipSetDevice(c->device));
    void *dz, *du; int rc;
    if ((rc = pool_get(c, "dump", (size_t)N * d * 8, &dz))) return rc;
    if ((rc = pool_get(c, "dump2", (size_t)N * 8, &du))) return rc;
    hipLaunchKernelGGL(k_dump_move_draws_mv, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, make_key(seed, stream), (uint32_t)call, N, d, (double*)dz, (double*)du);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(z_out, dz, (size_t)N * d * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(u_out, du, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return BSSM_OK;
}

extern "C" int bssm_pf_run(bssm_ctx* c, const bssm_pf_config* cfg, bssm_pf_result* res)
{
    if (!c) ARGFAIL("bssm_pf_run: NULL argument");
    if (cfg && res && cfg->model == BSSM_MODEL_LGMV) return pf_run_mv<MV_OBS_GAUSS>(c, cfg, res);
    if (cfg && res && cfg->model == BSSM_MODEL_LGMV_POIS) return pf_run_mv<MV_OBS_POIS>(c, cfg, res);
    if (cfg && res && cfg->model == BSSM_MODEL_LGMV_LOGVAR) return pf_run_mv<MV_OBS_LOGVAR>(c, cfg, res);
    if (cfg && res && (cfg->model == BSSM_MODEL_RNET || cfg->model == BSSM_MODEL_RNET_NB)) return pf_run_rn(c, cfg, res, cfg->model == BSSM_MODEL_RNET_NB);
    // the fused path needs the device's token (one fused run at a time); without it the run takes the multi-launch path
    const int dev = c->device & 63;
    const long long serial = ++g_run_serial[dev];
    const bool alone = (++g_runs_active[dev] == 1);
    if (!alone) g_last_overlap[dev].store(serial);
    const bool quiet = alone && (g_last_overlap[dev].load() == 0 || serial - g_last_overlap[dev].load() > FZ_QUIET) && serial > g_fused_hold[dev].load();
    int expected = 0;
    const bool token = quiet && c->opt_fused && c->fz_ok && g_fused_busy[dev].compare_exchange_strong(expected, 1);
    const long long timeouts0 = c->fz_timeouts;
    int rc = pf_run_impl(c, cfg, res, token);
    if (token) g_fused_busy[dev].store(0);
    // a time-out means the launch's workgroups were not all resident: the GPU is shared with work this process cannot see (another
    // process, another library).  Each costs 20 ms before the run is repeated, so the device backs off: 256 runs without a fused attempt
    // after the first time-out, doubling up to 65 536 while they keep coming
    if (c->fz_timeouts != timeouts0) {
        const long long last = g_fused_span[dev].load();
        const long long span = last > 0 ? (last * 2 > 65536 ? 65536 : last * 2) : 256;
        g_fused_span[dev].store(span);
        g_fused_hold[dev].store(serial + span);
    } else if (token && rc == BSSM_OK) g_fused_span[dev].store(0);
    if (rc == BSSM_RETRY_UNFUSED) rc = pf_run_impl(c, cfg, res, false);      // deterministic: the same draws, the other kernels
    --g_runs_active[dev];
    return rc;
}

// The smoother's entry point: bssm_pf_run on a copy of cfg that records histories and ancestors, with the context told what the
// caller's own cfg wants on the host; pf_run_results ends such a run with the trace (smooth_trace).
extern "C" int bssm_pf_run_smooth(bssm_ctx* c, const bssm_pf_config* cfg, bssm_pf_result* res, const bssm_smooth_config* scfg, bssm_smooth_result* sres)
{
    if (!c || !cfg || !res) ARGFAIL("bssm_pf_run_smooth: NULL argument");
    if (!scfg || !sres) ARGFAIL("bssm_pf_run_smooth: the smoother's config and result structs are required");
    const int K = scfg->n_trajectories;
    if (K < 0 || K > 4096) ARGFAIL("bssm_pf_run_smooth: n_trajectories must be 0 .. 4096");
    if (!sres->smoothed || !sres->n_lineages) ARGFAIL("bssm_pf_run_smooth: smoothed / n_lineages buffers missing");
    if (K > 0 && (!sres->trajectories || !sres->trajectory_u || !sres->trajectory_index)) ARGFAIL("bssm_pf_run_smooth: trajectory buffers missing");
    if (c->sh_nloc) ARGFAIL("bssm_pf_run_smooth: a sharded context holds a part of the particles only");
    bssm_pf_config run_cfg = *cfg;
    run_cfg.return_particles = 1; run_cfg.return_ancestors = 1;
    const SmoothReq req{cfg->return_particles, cfg->return_ancestors, K, sres};
    c->smooth = &req;
    const int rc = bssm_pf_run(c, &run_cfg, res);
    c->smooth = nullptr;
    return rc;
}

extern "C" int bssm_ctx_fused_stamps(bssm_ctx* c, long long* out /* [2][24] */)
{   // DEV builds (make DEV=1): clock64() stage stamps of the last fused launch (typical worker, resolver); zeros otherwise
    if (!c || !out || !c->fz) ARGFAIL("bssm_ctx_fused_stamps: NULL argument");
    HIPCHK(hipMemcpy(out, c->fz->stamps, sizeof(c->fz->stamps), hipMemcpyDeviceToHost));
    return BSSM_OK;
}

extern "C" int bssm_ctx_fused_endt(bssm_ctx* c, long long* out /* [2][512]: end, start */)
{
    if (!c || !out || !c->fz) ARGFAIL("bssm_ctx_fused_endt: NULL argument");
    HIPCHK(hipMemcpy(out, c->fz->endt, sizeof(c->fz->endt), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + FZ_MAXB, c->fz->startt, sizeof(c->fz->startt), hipMemcpyDeviceToHost));
    return BSSM_OK;
}

extern "C" int bssm_ctx_fused_pubt(bssm_ctx* c, long long* out /* [4][512] */)
{
    if (!c || !out || !c->fz) ARGFAIL("bssm_ctx_fused_pubt: NULL argument");
    HIPCHK(hipMemcpy(out, c->fz->pubt, sizeof(c->fz->pubt), hipMemcpyDeviceToHost));
    return BSSM_OK;
}

extern "C" int bssm_ctx_fused_waket(bssm_ctx* c, long long* out /* [5][512]: the three answers, M seen, S seen (early_max) */)
{
    if (!c || !out || !c->fz) ARGFAIL("bssm_ctx_fused_waket: NULL argument");
    HIPCHK(hipMemcpy(out, c->fz->waket, sizeof(c->fz->waket), hipMemcpyDeviceToHost));
    return BSSM_OK;
}

extern "C" int bssm_ctx_fused_stats(bssm_ctx* c, long long* out /* [4]: runs, launches, stand-downs (unsupported record), time-outs */)
{
    if (!c || !out) ARGFAIL("bssm_ctx_fused_stats: NULL argument");
    out[0] = c->fz_runs; out[1] = c->fz_launches; out[2] = c->fz_bails; out[3] = c->fz_timeouts;
    return BSSM_OK;
}

extern "C" int bssm_ctx_multi_stats(bssm_ctx* c, long long* out /* [2]: bssm_pf_run_multi calls with c as ctxs[0] that took the lock-step kernels, that ran one filter after the other */)
{
    if (!c || !out) ARGFAIL("bssm_ctx_multi_stats: NULL argument");
    out[0] = c->multi_lockstep; out[1] = c->multi_sequential;
    return BSSM_OK;
}

// ---- K independent large filters in lock-step on ONE stream (multi.hip.h) -------------------------------------------------
// ctxs[k] holds filter k's buffers; every launch carries all K argument sets (blockIdx.y = filter).  Shared: data, N, T, model,
// resampling settings; per filter: theta, seed, stream.  Each filter's outputs are bit-identical to bssm_pf_run's.  Configurations
// outside the lock-step kernels' reach (APF / RMPF, SIR, multinomial, more than 2^20 particles, histories, injected draws) run
// one after the other through bssm_pf_run.  Either way a filter writes into its rows of the batch result and ends as a run of its own.
// batch_rows: the bssm_pf_result of filter k (d state components): its rows, or one shared set of scratch rows for those not asked for
struct RowScratch { std::vector<double> se, ess, llh; RowScratch(int T, int d) : se((size_t)(T + 1) * d), ess((size_t)T + 1), llh((size_t)std::max(T, 1)) {} };
static bssm_pf_result batch_rows(const bssm_pf_batch_result* res, int k, int T, int d, RowScratch& s)
{
    const size_t T1 = (size_t)T + 1;
    bssm_pf_result r; memset(&r, 0, sizeof(r));
    r.state_est = res->state_est ? res->state_est + (size_t)k * T1 * d : s.se.data();
    r.ess = res->ess ? res->ess + (size_t)k * T1 : s.ess.data();
    r.loglike_history = res->loglike_history ? res->loglike_history + (size_t)k * T : s.llh.data();
    r.loglike = res->loglike + k;
    r.early_return_step = res->early_return_step ? res->early_return_step + k : nullptr;
    r.n_res_calls = res->n_res_calls ? res->n_res_calls + k : nullptr;
    return r;
}

extern "C" int bssm_pf_run_multi(bssm_ctx* const* ctxs, int n_filters, const bssm_pf_config* cfg, const double* thetas,
                                 const unsigned long long* seeds, const unsigned long long* streams, bssm_pf_batch_result* res)
{
    if (!ctxs || !cfg || !res || !thetas || !seeds || !streams) ARGFAIL("bssm_pf_run_multi: NULL argument");
    const int F = n_filters;
    if (F < 1 || F > MULTI_MAX) ARGFAIL("bssm_pf_run_multi: 1 .. 4 filters per call");
    for (int k = 0; k < F; k++) { if (!ctxs[k]) ARGFAIL("bssm_pf_run_multi: NULL context"); for (int j = 0; j < k; j++) if (ctxs[j] == ctxs[k]) ARGFAIL("bssm_pf_run_multi: every filter needs a context of its own"); }
    const long long N = cfg->num_particles;
    const int T = cfg->T, nth = cfg->n_theta;
    if (N <= 0) ARGFAIL("num_particles must be a positive count");
    if (T < 0 || nth < 3) ARGFAIL("bssm_pf_run_multi: bad filter configuration");
    if (!res->loglike) ARGFAIL("bssm_pf_run_multi: result buffers missing");
    const int B = (int)((N + EB - 1) / EB);
    bssm_ctx* c0 = ctxs[0];
    bool lock = (cfg->model == BSSM_MODEL_LG || cfg->model == BSSM_MODEL_AR1SIN) && cfg->algorithm == BSSM_BPF && B <= 2 * NT &&
                (cfg->resample_fn == BSSM_STRATIFIED || cfg->resample_fn == BSSM_SYSTEMATIC) && !cfg->return_particles && !cfg->return_ancestors &&
                !cfg->z_init && !cfg->z_trans && !cfg->u_res && F > 1;
    for (int k = 0; k < F && lock; k++) {
        const bssm_ctx* c = ctxs[k];
        lock = c->device == c0->device && N <= c->cap && c->opt_inkernel_resolve && c->opt_renormalize && c->opt_recompute_lw && !c->opt_fuse_step &&
               !c->opt_debug_stop && c->opt_window == c0->opt_window && c->opt_stage == c0->opt_stage && c->opt_force_fallback == c0->opt_force_fallback &&
               !c->profile;
    }
    const int dim = (cfg->model == BSSM_MODEL_SIR) ? 2 : 1;
    RowScratch scratch(T, dim);
    if (!lock) {      // one after the other, each into its rows of the result
        c0->multi_sequential++;
        double ms_total = 0;
        int first_bad = BSSM_OK;
        for (int k = 0; k < F; k++) {
            bssm_pf_config q = *cfg;
            q.theta = thetas + (size_t)k * nth; q.seed = seeds[k]; q.stream = streams[k];
            bssm_pf_result r = batch_rows(res, k, T, dim, scratch);
            double ms = 0; r.device_ms = &ms;
            *r.loglike = 0; if (r.early_return_step) *r.early_return_step = 0; if (r.n_res_calls) *r.n_res_calls = 0;      // (a refused run writes none of them)
            const int rc = bssm_pf_run(ctxs[k], &q, &r);
            if (res->status) res->status[k] = rc;
            if (rc && !first_bad) first_bad = rc;
            ms_total += ms;
        }
        if (res->device_ms) *res->device_ms = ms_total;
        return res->status ? BSSM_OK : first_bad;
    }
    for (int i = 0; i < T; i++) if (!isfinite(cfg->y[i])) ARGFAIL("Assertion on 'y' failed: Contains missing values");
    if (int rc_o = obs_times_check(cfg->obs_times, T)) return rc_o;
    HIPCHK(hipSetDevice(c0->device));
    hipStream_t stream = c0->stream;
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL("bssm_pf_run_multi: unknown resample_algorithm");
    c0->multi_lockstep++;
    // per filter: its configuration, the run record and buffers of pf_run_setup (zeroed on the one stream), its grid-max slots
    struct Per { bssm_pf_config q; bssm_pf_result rows; PfRun run; GmaxSlots gm; unsigned long long* gslot; ModelPar par; double *X0, *X1; };
    std::vector<Per> P((size_t)F);
    int rc;
    for (int k = 0; k < F; k++) {
        bssm_ctx* c = ctxs[k];
        Per& p = P[k];
        HIPCHK(hipStreamSynchronize(c->stream));                     // (its buffers may still be in use by its own stream)
        p.q = *cfg; p.q.theta = thetas + (size_t)k * nth; p.q.seed = seeds[k]; p.q.stream = streams[k];
        p.rows = batch_rows(res, k, T, 1, scratch);
        if ((rc = pf_run_setup(c, &p.q, &p.rows, 1, false, p.run, stream))) return rc;
        if ((rc = p.gm.take(c, (size_t)T + 2, stream))) return rc;
        p.par = scalar_par(cfg->model, p.q.theta);
        p.X0 = c->x0; p.X1 = c->x1;
    }
    HIPCHK(hipEventRecord(c0->ev0, stream));
    for (int k = 0; k < F; k++) {
        hipLaunchKernelGGL(k_reset_state, dim3(1), dim3(1), 0, stream, ctxs[k]->st);
        hipLaunchKernelGGL(k_init, dim3(B), dim3(NT), 0, stream, P[k].X0, N, noise_src(nullptr, P[k].run.key, DRAW_INIT, 0), P[k].run.separt, cfg->model, P[k].par, 0);
    }
    const bool sysk = cfg->resample_fn == BSSM_SYSTEMATIC;
    const dim3 grid(B, F);
    ObsClock clk(cfg->obs_times, T);
    for (int i = 1; i <= T; i++) {                                                        // R/particle_filter_core.R:123
        clk.advance(i);
        const int gap = clk.gap;
        const double yi = cfg->y[i - 1];
        for (int k = 0; k < F; k++) P[k].gslot = P[k].gm.next();
        StepMulti sm; LocalMulti lw_, lp_; ApplyMulti am;
        for (int step = 1; step <= std::max(gap, 1); step++) {
            const bool last = (step >= gap), trans = gap >= 1;
            for (int k = 0; k < F; k++) {
                StepArgs& a = sm.a[k];
                a.xin = P[k].X0; a.xout = P[k].X0; a.lw = nullptr; a.N = N; a.par = P[k].par; a.y = yi;
                a.ns = noise_src(nullptr, P[k].run.key, DRAW_TRANS, clk.ktrans);
                a.pm = ctxs[k]->pm; a.ps = ctxs[k]->ps; a.pq = ctxs[k]->pq; a.st = ctxs[k]->st; a.gmax = P[k].gslot;
            }
            if (cfg->model == BSSM_MODEL_LG) {
                if (trans && last) hipLaunchKernelGGL((k_step_multi<0, true, 1>), grid, dim3(NTS), 0, stream, sm);
                else if (trans) hipLaunchKernelGGL((k_step_multi<0, true, 0>), grid, dim3(NTS), 0, stream, sm);
                else hipLaunchKernelGGL((k_step_multi<0, false, 1>), grid, dim3(NTS), 0, stream, sm);
            } else {
                if (trans && last) hipLaunchKernelGGL((k_step_multi<1, true, 1>), grid, dim3(NTS), 0, stream, sm);
                else if (trans) hipLaunchKernelGGL((k_step_multi<1, true, 0>), grid, dim3(NTS), 0, stream, sm);
                else hipLaunchKernelGGL((k_step_multi<1, false, 1>), grid, dim3(NTS), 0, stream, sm);
            }
            if (trans) clk.ktrans++;
        }
        for (int k = 0; k < F; k++) {
            bssm_ctx* c = ctxs[k];
            const Per& p = P[k];
            double* se_row = p.run.separt + (size_t)i * B;
            // the log-weights are never stored here (recompute_lw is a condition of this path), and the filter's own slot holds the grid max
            FromLw f = from_lw(c, c->lw, c->w, N, B, PLAN_PF, i, p.run.resample_algorithm, p.run.threshold, p.run.ess, p.run.llh, p.run.resampled);
            f.xw = p.X0; f.yw = yi; f.syw = p.par.sy; f.lsyw = p.par.log_sy; f.gmax = p.gslot;
            LocalArgs& w_ = lw_.a[k];
            w_.w = c->w; w_.nw = N; w_.ain = c->ain_w; w_.lim = rec_lim(c, N); w_.brec = c->brec; w_.side = c->side; w_.st = c->st; w_.f = f; w_.prev_brec = nullptr; w_.prev_side = nullptr; w_.ain_p_out = nullptr;
            LocalArgs& p_ = lp_.a[k];
            p_ = w_; p_.brec = c->brec_p; p_.side = c->side_p; p_.prev_brec = c->brec; p_.prev_side = c->side; p_.ain_p_out = c->ain_p;
            // the expansion as built, on the generator's uniforms and without ancestors (injected draws and histories take the other path)
            ApplyOne& q = am.a[k];
            q.a = apply_args(c, c->w, N, (int)N, B, nullptr, p.run.u_stride, p.run.key, nullptr, 0, p.X0, p.X1, 1, N, se_row);
            q.st = c->st; q.prev_brec = c->brec_p; q.prev_side = c->side_p;
        }
        hipLaunchKernelGGL(k_weights_multi, grid, dim3(NT), 0, stream, lw_);
        hipLaunchKernelGGL(k_localp_multi, grid, dim3(NT), 0, stream, lp_);
        const size_t xshm = std::max((size_t)(c0->opt_stage ? 1 : 0) * CAPX * sizeof(double), sizeof(ResolveSmem));
        if (sysk) hipLaunchKernelGGL((k_apply_multi<1>), grid, dim3(NT), xshm, stream, am);
        else hipLaunchKernelGGL((k_apply_multi<0>), grid, dim3(NT), xshm, stream, am);
        for (int k = 0; k < F; k++) {
            if (cfg->resample_algorithm != BSSM_SISR)
                hipLaunchKernelGGL(k_carry, dim3(B), dim3(NT), 0, stream, P[k].X0, P[k].X1, ctxs[k]->w, N, 1, P[k].run.separt + (size_t)i * B, ctxs[k]->st, 0);
            std::swap(P[k].X0, P[k].X1);
        }
    }
    for (int k = 0; k < F; k++)
        hipLaunchKernelGGL(k_reduce_state_est, dim3(T + 1), dim3(NT), 0, stream, P[k].run.separt, B, 1, P[k].run.se);
    HIPCHK(hipEventRecord(c0->ev1, stream));
    HIPCHK(hipStreamSynchronize(stream));
    // each filter ends as a run of its own does: read-back (on its context's stream, behind the drained one), scalars, dead rows, status
    int first_bad = BSSM_OK;
    std::string first_err;
    for (int k = 0; k < F; k++) {
        DevState h;
        if ((rc = pf_run_read_back(ctxs[k], P[k].run, &P[k].rows, h))) return rc;
        const int st = pf_run_results(ctxs[k], &P[k].q, P[k].run, h, false, &P[k].rows);
        if (res->status) res->status[k] = st;
        if (st && !first_bad) { first_bad = st; first_err = g_err; }
    }
    if (first_bad) g_err = first_err;
    if (res->device_ms) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c0->ev0, c0->ev1)); *res->device_ms = ms; }
    return res->status ? BSSM_OK : first_bad;
}

// ---- closure mode: normalise, decide, resample for host-evaluated log-weights -------------------------------------
extern "C" int bssm_pf_weigh_resample(bssm_ctx* c, long long n, const double* lw, int always, int resample_algorithm,
                                      double threshold, int resample_fn, const double* U, unsigned long long seed,
                                      unsigned long long stream, int call, double* weights_out, int* ancestors_out,
                                      double* scalars_out, int* flags_out)
{
    if (!c || !lw || !scalars_out || !flags_out) ARGFAIL("bssm_pf_weigh_resample: NULL argument");
    if (n <= 0) ARGFAIL("num_particles must be a positive count");
    if (n > c->cap) { g_err = "bssm_pf_weigh_resample: num_particles exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    if (resample_algorithm < 0 || resample_algorithm > 2) ARGFAIL("bssm_pf_weigh_resample: unknown resample_algorithm");
    if (resample_fn < 0 || resample_fn > 3) ARGFAIL("bssm_pf_weigh_resample: unknown resample_fn");
    if (resample_fn == BSSM_MULTINOMIAL_R && !U) ARGFAIL("bssm_pf_weigh_resample: BSSM_MULTINOMIAL_R replays R's unif_rand() stream: U is required");
    if (call < 0) ARGFAIL("bssm_pf_weigh_resample: call must be >= 0");
    HIPCHK(hipSetDevice(c->device));
    const int B = (int)((n + EB - 1) / EB);
    threshold = threshold_or_auto(resample_algorithm, threshold, (double)n);
    const long long nu = (resample_fn == BSSM_SYSTEMATIC) ? 1 : n;
    void *d_small, *d_anc, *d_u = nullptr;
    int rc;
    if ((rc = pool_get(c, "wr_small", 64, &d_small))) return rc;          // ess_out[2], llh_out[1], resampled[1]
    if ((rc = pool_get(c, "wr_anc", (size_t)n * 4, &d_anc))) return rc;
    HIPCHK(hipMemcpyAsync(c->lw, lw, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    if (U && (rc = pool_put(c, "wr_u", U, (size_t)nu * 8, &d_u))) return rc;
    HIPCHK(hipMemsetAsync(d_small, 0, 64, c->stream));
    LAUNCH(c, "k_reset_state", k_reset_state, 1, 1, 0, c->st);
    LAUNCH(c, "k_lw_partials", k_lw_partials, B, NTS, 0, c->lw, n, c->pm, c->ps, c->pq, (unsigned long long*)nullptr);
    c->gmax_cur = nullptr;
    ResampleLaunch r;
    r.d_lw = c->lw; r.plan = always ? PLAN_AUX : PLAN_PF; r.check_degenerate = always ? 0 : 1; r.obs_i = 1;
    r.resample_algorithm = resample_algorithm; r.threshold = threshold;
    r.d_ess = (double*)d_small; r.d_llh = (double*)d_small + 2; r.d_resampled = (int*)((double*)d_small + 4);
    r.d_w = c->w; r.nw = n; r.n = (int)n; r.kind = resample_fn;
    // the generator's resample draws are indexed by call: place the injected draws so that call 0 reads them
    r.d_u = (const double*)d_u; r.u_stride = 0; r.key = make_key(seed, stream);
    r.d_anc = (int*)d_anc; r.anc_stride = 0; r.d_cum = nullptr;
    if (!U && call > 0) hipLaunchKernelGGL(k_set_calls, dim3(1), dim3(1), 0, c->stream, c->st, call);
    launch_scan_and_apply(c, r);
    HIPCHK(hipGetLastError());
    DevState h;
    HIPCHK(hipMemcpyAsync(&h, c->st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    flags_out[0] = 0; flags_out[1] = h.dead ? 1 : 0;
    scalars_out[0] = h.loglike; scalars_out[1] = h.ess; scalars_out[2] = h.lse_max; scalars_out[3] = h.lse_sum;
    if (h.dead) return BSSM_OK;
    if (h.flags) { const int st = flags_to_status(h.flags); if (st != BSSM_ERR_ARG) g_err = bssm_status_string(st); return st; }
    if (weights_out) HIPCHK(hipMemcpy(weights_out, c->w, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (h.do_resample) {
        if (!ancestors_out) ARGFAIL("bssm_pf_weigh_resample: ancestors_out is required when the observation resamples");
        HIPCHK(hipMemcpy(ancestors_out, d_anc, (size_t)n * 4, hipMemcpyDeviceToHost));
        flags_out[0] = 1;
    }
    return BSSM_OK;
}

// ---- one filter, particle blocks sharded over ranks (prototype) -------------------------------------------------
// The same kernels on this rank's blocks of the global numbering (block offset), host-staged collectives at the four
// points where a step needs the other ranks' blocks; every rank resolves the exact sums itself (resolve_in_block), so no
// rank waits for a "resolver" and the result does not depend on the number of ranks.
struct ShardScope {      // the context runs sharded only inside bssm_pf_run_sharded
    bssm_ctx* c;
    ShardScope(bssm_ctx* c_, int boff, int nloc) : c(c_) { c->sh_boff = boff; c->sh_nloc = nloc; }
    ~ShardScope() { c->sh_boff = 0; c->sh_nloc = 0; }
};

extern "C" int bssm_pf_run_sharded(bssm_ctx* c, const bssm_pf_config* cfg, const bssm_shard* sh, bssm_pf_result* res)
{
    if (!c || !cfg || !sh || !res) ARGFAIL("bssm_pf_run_sharded: NULL argument");
    if (!sh->all_gather || !sh->exchange || sh->world < 1 || sh->rank < 0 || sh->rank >= sh->world) ARGFAIL("bssm_pf_run_sharded: bad shard description");
    const long long N = cfg->num_particles;
    const int T = cfg->T, W = sh->world;
    if (cfg->model != BSSM_MODEL_LG && cfg->model != BSSM_MODEL_AR1SIN) ARGFAIL("bssm_pf_run_sharded: scalar-state Gaussian models only");
    if (cfg->algorithm != BSSM_BPF) ARGFAIL("bssm_pf_run_sharded: bootstrap filter only");
    if (cfg->resample_fn != BSSM_STRATIFIED && cfg->resample_fn != BSSM_SYSTEMATIC) ARGFAIL("bssm_pf_run_sharded: stratified / systematic resampling only");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL("bssm_pf_run_sharded: unknown resample_algorithm");
    if (cfg->return_particles || cfg->return_ancestors) ARGFAIL("bssm_pf_run_sharded: histories are not available");
    if (N <= 0 || N % ((long long)W * EB) != 0) ARGFAIL("bssm_pf_run_sharded: num_particles must be a multiple of world x 2048");
    const int B = (int)(N / EB), nloc = B / W, boff = sh->rank * nloc;
    if (B > MAXB) { g_err = "bssm_pf_run_sharded: at most 2^22 particles in all (the block-record workspace of this build; every rank resolves the records of all blocks itself)"; return BSSM_ERR_CAPACITY; }
    // up to 2 NT blocks every workgroup resolves the records itself (as on one GPU); above, one 1024-thread workgroup per rank does (k_resolve_all)
    const bool inres = B <= 2 * NT;
    if (N > c->cap) { g_err = "bssm_pf_run_sharded: num_particles exceeds context capacity"; return BSSM_ERR_CAPACITY; }
    if (T < 0 || (T > 0 && !cfg->y) || !cfg->theta || cfg->n_theta < 3) ARGFAIL("bssm_pf_run_sharded: bad filter configuration");
    if (!res->state_est || !res->ess || !res->loglike || (T > 0 && !res->loglike_history)) ARGFAIL("bssm_pf_run_sharded: result buffers missing");
    HIPCHK(hipSetDevice(c->device));
    ShardScope scope(c, boff, nloc);
    const long long lo = (long long)boff * EB, cnt = (long long)nloc * EB;        // this rank's particles
    PfRun run;                                                                    // (B = N / EB; no histories: refused above)
    int rc;
    if ((rc = pf_run_setup(c, cfg, res, 1, false, run))) return rc;
    const double *d_zi = nullptr, *d_zt = nullptr;
    if (cfg->z_init && (rc = pool_put(c, "zi", cfg->z_init, (size_t)N * 8, &d_zi))) return rc;
    if (cfg->z_trans && run.max_trans > 0 && (rc = pool_put(c, "zt", cfg->z_trans, (size_t)run.max_trans * N * 8, &d_zt))) return rc;
    // host staging for the collectives
    const size_t rec_bytes = (size_t)nloc * sizeof(BlockRec), side_bytes = (size_t)nloc * sizeof(SideList);
    std::vector<char> hsend(std::max<size_t>({rec_bytes + side_bytes, (size_t)3 * nloc * 8, (size_t)(T + 1) * nloc * 8, (size_t)64})), hrecv(hsend.size() * W);
    std::vector<double> xsend((size_t)std::min<long long>(N, 2 * cnt + (long long)CAPX)), xrecv((size_t)cnt);
    auto sync = [&]() -> int { HIPCHK(hipStreamSynchronize(c->stream)); return BSSM_OK; };
#define SHCHK(expr) do { if ((expr) != 0) { g_err = "bssm_pf_run_sharded: a collective callback failed"; return BSSM_ERR_ARG; } } while (0)
    // all_gather of one per-block device array slice [boff, boff + nloc) x item bytes, written back to the full device array
    const bool devbuf = sh->device_buffers != 0;
    // device-buffer collectives of HOST data (the ranks' output ranges + status; at the end the state-estimate partials): staged
    // through a device send area and, 64-byte aligned behind it, the receive area
    auto gather_host = [&](const void* send, void* recv, size_t bytes) -> int {
        if (!devbuf) { SHCHK(sh->all_gather(sh->user, send, recv, (long long)bytes)); return BSSM_OK; }
        const size_t at = (bytes + 63) & ~(size_t)63;
        char* ds;
        if (int r2 = pool_get(c, "sh_stage", at + bytes * W, &ds)) return r2;
        char* dr = ds + at;
        HIPCHK(hipMemcpyAsync(ds, send, bytes, hipMemcpyHostToDevice, c->stream));
        if (int r2 = sync()) return r2;
        SHCHK(sh->all_gather(sh->user, ds, dr, (long long)bytes));
        if (int r2 = sync()) return r2;
        HIPCHK(hipMemcpy(recv, dr, bytes * W, hipMemcpyDeviceToHost));
        return BSSM_OK;
    };
    auto gather_blocks = [&](void* d_arr, size_t item) -> int {
        if (devbuf) {      // in place on the device array: rank r's slice sits at r x nloc x item already
            if (int r2 = sync()) return r2;
            SHCHK(sh->all_gather(sh->user, (char*)d_arr + (size_t)boff * item, d_arr, (long long)((size_t)nloc * item)));
            return sync();
        }
        HIPCHK(hipMemcpyAsync(hsend.data(), (char*)d_arr + (size_t)boff * item, (size_t)nloc * item, hipMemcpyDeviceToHost, c->stream));
        if (int r2 = sync()) return r2;
        SHCHK(sh->all_gather(sh->user, hsend.data(), hrecv.data(), (long long)((size_t)nloc * item)));
        HIPCHK(hipMemcpyAsync(d_arr, hrecv.data(), (size_t)B * item, hipMemcpyHostToDevice, c->stream));      // rank order == block order
        return sync();            // (hrecv is reused by the next gather)
    };
    const ModelPar par = scalar_par(cfg->model, cfg->theta);
    double* X0 = c->x0; double* X1 = c->x1;
    const int lim = rec_lim(c, N);
    LAUNCH(c, "k_reset_state", k_reset_state, 1, 1, 0, c->st);
    LAUNCH(c, "k_init", k_init, nloc, NT, 0, X0, N, noise_src(d_zi, run.key, DRAW_INIT, 0), run.separt, cfg->model, par, boff);
    DevState h; memset(&h, 0, sizeof(h));
    ObsClock clk(cfg->obs_times, T);
    for (int i = 1; i <= T; i++) {                                                        // R/particle_filter_core.R:123
        clk.advance(i);
        const double yi = cfg->y[i - 1];
        c->gmax_cur = nullptr;      // (no slot: the partial maxima of other ranks are not in this rank's; launch_step takes the shard off the context)
        for (int step = 1; step <= clk.gap; step++)
            launch_step_model(c, cfg->model, true, (step == clk.gap) ? 1 : 0, false, X0, N, B, par, yi, trans_noise(run, d_zt, clk.ktrans++));
        if (clk.gap <= 0) launch_step_model(c, cfg->model, false, 1, false, X0, N, B, par, yi, trans_noise(run, d_zt, 0));      // obs_times repeats a time
        // (1) the log-sum-exp partials of every block
        if ((rc = gather_blocks(c->pm, 8)) || (rc = gather_blocks(c->ps, 8)) || (rc = gather_blocks(c->pq, 8))) return rc;
        double* se_row = run.separt + (size_t)i * B;
        // as built: stored log-weights, no slot, no folding, this rank's lead and publishing blocks
        FromLw f = from_lw(c, c->lw, c->w, N, B, PLAN_PF, i, run.resample_algorithm, run.threshold, run.ess, run.llh, run.resampled);
        LAUNCH(c, "k_weights(normalize+local<W>)", (k_local<MODE_W, true>), nloc, NT, 0, c->w, N, c->ain_w, lim, c->brec, c->side, c->st, f, nullptr, nullptr, nullptr, boff, B);
        HIPCHK(hipMemcpyAsync(&h, c->st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        if ((rc = sync())) return rc;
        if (h.dead || h.flags) break;                                                     // identical on every rank: all leave together
        if (h.do_resample) {
            // (2) the records of sum(w), (3) the records of cumsum(w / total): every rank resolves them itself
            for (int q = 0; q < 4; q++) if ((rc = gather_blocks((char*)c->brec + (size_t)q * BREC_STRIDE * 16, 16))) return rc;      // (the records live in four planes)
            if ((rc = gather_blocks(c->side, sizeof(SideList)))) return rc;
            if (inres) LAUNCH(c, "k_local<P>(+resolve<W>)", (k_local<MODE_P, false, true>), nloc, NT, 0, c->w, N, c->ain_w, lim, c->brec_p, c->side_p, c->st, f, c->brec, c->side, c->ain_p, boff, B);
            else {
                // (ain_w holds the approximate prefix of EVERY block on every rank: the publishing block of k_weights derives them all from the gathered partials)
                LAUNCH(c, "k_resolve_all<W>", k_resolve_all<MODE_W>, 1, NTR, 0, c->w, N, B, c->brec, c->side, c->cin, c->ain_w, c->ain_p, c->st);
                LAUNCH(c, "k_local<P>", (k_local<MODE_P, false>), nloc, NT, 0, c->w, N, c->ain_p, lim, c->brec_p, c->side_p, c->st, f, nullptr, nullptr, nullptr, boff, B);
            }
            for (int q = 0; q < 4; q++) if ((rc = gather_blocks((char*)c->brec_p + (size_t)q * BREC_STRIDE * 16, 16))) return rc;
            if ((rc = gather_blocks(c->side_p, sizeof(SideList)))) return rc;
            // as built, without ancestors (histories are refused above); lead / last are this rank's first and last block
            ApplyArgs a = apply_args(c, c->w, N, (int)N, B, run.ur, run.u_stride, run.key, nullptr, 0, X0, X1, 1, N, se_row);
            const size_t xshm = std::max((size_t)a.nstage * CAPX * sizeof(double), inres ? sizeof(ResolveSmem) : (size_t)0);
            if (inres) {
                if (cfg->resample_fn == BSSM_SYSTEMATIC) LAUNCH(c, "k_apply<systematic>(+resolve<P>)", (k_apply<1, true>), nloc, NT, xshm, a, c->st, c->brec_p, c->side_p, boff, B);
                else LAUNCH(c, "k_apply<stratified>(+resolve<P>)", (k_apply<0, true>), nloc, NT, xshm, a, c->st, c->brec_p, c->side_p, boff, B);
            } else {
                LAUNCH(c, "k_resolve_all<P>", k_resolve_all<MODE_P>, 1, NTR, 0, c->w, N, B, c->brec_p, c->side_p, c->cin, c->ain_w, c->ain_p, c->st);
                if (cfg->resample_fn == BSSM_SYSTEMATIC) LAUNCH(c, "k_apply<systematic>", (k_apply<1, false>), nloc, NT, xshm, a, c->st, nullptr, nullptr, boff, B);
                else LAUNCH(c, "k_apply<stratified>", (k_apply<0, false>), nloc, NT, xshm, a, c->st, nullptr, nullptr, boff, B);
            }
            HIPCHK(hipMemcpyAsync(&h, c->st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
            if ((rc = sync())) return rc;
            // (4) the resampled particles: this rank produced the outputs [out_lo, out_hi); owners are cut at multiples of N / world
            // ... with this rank's status riding along: a rank that failed (its run state carries an error flag, its kernels returned
            // early) is seen by every rank HERE, and all of them leave the loop together instead of one returning while the others
            // wait in the next collective.  The tiling check is made on the gathered ranges, so every rank reaches the same verdict.
            long long mine[3] = {h.out_lo, h.out_hi, (long long)(h.flags | (h.dead ? 0x100u : 0u))};
            std::vector<long long> all((size_t)3 * W), scnt((size_t)W), rcnt((size_t)W);
            if ((rc = gather_host(mine, all.data(), 24))) return rc;
            auto overlap = [](long long a0, long long a1, long long b0, long long b1) { const long long l = std::max(a0, b0), r = std::min(a1, b1); return r > l ? r - l : 0LL; };
            bool any_fail = false, tiles = true;
            long long edge = 0;
            for (int r2 = 0; r2 < W; r2++) {
                any_fail = any_fail || all[3 * r2 + 2] != 0;
                tiles = tiles && all[3 * r2] == edge && all[3 * r2 + 1] >= edge;      // rank r2's outputs start where rank r2 - 1's ended
                edge = all[3 * r2 + 1];
                scnt[r2] = overlap(mine[0], mine[1], (long long)r2 * cnt, (long long)(r2 + 1) * cnt);
                rcnt[r2] = overlap(all[3 * r2], all[3 * r2 + 1], lo, lo + cnt);
            }
            if (any_fail) { for (int r2 = 0; r2 < W; r2++) h.flags |= (uint32_t)(all[3 * r2 + 2] & 0xff); break; }      // every rank: same decision
            if (!tiles || edge != N) { g_err = "bssm_pf_run_sharded: the ranks' output ranges do not tile the particles"; return BSSM_ERR_ARG; }
            const long long nsend = mine[1] - mine[0];
            if (devbuf) {
                // straight from the resampled particles on this GPU into a device staging area (the send and receive ranges of X1 overlap),
                // then into this rank's slice
                double* stage = c->auxlw;
                if ((rc = sync())) return rc;
                SHCHK(sh->exchange(sh->user, X1 + mine[0], scnt.data(), stage, rcnt.data()));
                if ((rc = sync())) return rc;
                HIPCHK(hipMemcpyAsync(X1 + lo, stage, (size_t)cnt * 8, hipMemcpyDeviceToDevice, c->stream));
            } else {
                if ((long long)xsend.size() < nsend) xsend.resize((size_t)nsend);
                if (nsend > 0) HIPCHK(hipMemcpyAsync(xsend.data(), X1 + mine[0], (size_t)nsend * 8, hipMemcpyDeviceToHost, c->stream));
                if ((rc = sync())) return rc;
                SHCHK(sh->exchange(sh->user, xsend.data(), scnt.data(), xrecv.data(), rcnt.data()));
                HIPCHK(hipMemcpyAsync(X1 + lo, xrecv.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, c->stream));
            }
            if ((rc = sync())) return rc;
        } else {
            LAUNCH(c, "k_carry", k_carry, nloc, NT, 0, X0, X1, c->w, N, 1, se_row, c->st, boff);
        }
        std::swap(X0, X1);
    }
#undef SHCHK
    // state estimates: every rank's per-block partials, then the same reduction kernel as the single-GPU run
    {
        HIPCHK(hipMemcpy2DAsync(hsend.data(), (size_t)nloc * 8, run.separt + boff, (size_t)B * 8, (size_t)nloc * 8, (size_t)(T + 1), hipMemcpyDeviceToHost, c->stream));
        if ((rc = sync())) return rc;
        if ((rc = gather_host(hsend.data(), hrecv.data(), (size_t)(T + 1) * nloc * 8))) return rc;
        std::vector<double> full((size_t)(T + 1) * B);
        const double* rv = (const double*)hrecv.data();
        for (int r2 = 0; r2 < W; r2++) for (int i = 0; i <= T; i++)
            memcpy(&full[(size_t)i * B + (size_t)r2 * nloc], rv + ((size_t)r2 * (T + 1) + i) * nloc, (size_t)nloc * 8);
        HIPCHK(hipMemcpyAsync(run.separt, full.data(), full.size() * 8, hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, "k_reduce_state_est", k_reduce_state_est, T + 1, NT, 0, run.separt, B, 1, run.se);
        if ((rc = sync())) return rc;
    }
    if ((rc = pf_run_read_back(c, run, res, h))) return rc;
    return pf_run_results(c, cfg, run, h, false, res);
}

// ---- many small filters per launch (one workgroup = one whole filter) -------------------------
extern "C" int bssm_pf_batch_max_particles(void) { return EB; }
extern "C" int bssm_pf_batch_max_particles_mv(int d) { return mv_batch_max_particles(d); }

// What the three batch runners share.  Each checks its own arguments in its own order, then: batch_layout (the packed inputs and
// outputs of the call), batch_stage (pinned staging + the pool buffers b_in / b_out), batch_fill (keys, y, obs_times and the kernel
// arguments every family sets alike) next to the family's own pieces, batch_upload, the family's launch between ev0 and ev1,
// batch_download and batch_read_back.  One packed upload and one packed download per call: at T = 20 the filter itself takes
// ~0.3 ms, a dozen separate small copies and memsets would double that.
struct BatchRun {
    int F, T, dim; long long N; double dN;
    size_t ny;                                                                  // doubles of y: T, or T * p
    size_t o_keys, o_y, o_mid, o_ot, o_tail, in_bytes;                          // inputs: [pre: thetas at 0, ...] keys, y, [mid], obs_times, [tail]
    size_t q_ll, q_se, q_ess, q_llh, q_dead, q_flags, q_res, out_bytes, rowsT1, rowsSe;
    char *hs, *di, *dq;                                                         // pinned staging, b_in, b_out
};
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
// pre / mid / tail: the bytes a family puts in front of the keys (its thetas first), between y and obs_times, behind obs_times --
// each piece rounded with up16 by the family, which also knows the pieces' offsets (from 0, o_mid, o_tail)
static void batch_layout(BatchRun& r, int F, long long N, int T, int dim, size_t ny, size_t pre, size_t mid, size_t tail)
{
    r.F = F; r.N = N; r.dN = (double)N; r.T = T; r.dim = dim; r.ny = ny;
    const size_t Tn = (size_t)std::max(T, 1);
    r.o_keys = pre; r.o_y = r.o_keys + up16((size_t)F * sizeof(PhiloxKey)); r.o_mid = r.o_y + up16(std::max(ny, (size_t)1) * 8);
    r.o_ot = r.o_mid + mid; r.o_tail = r.o_ot + up16(Tn * 4); r.in_bytes = r.o_tail + tail;
    r.rowsT1 = (size_t)F * (T + 1) * 8; r.rowsSe = r.rowsT1 * dim;
    r.q_ll = 0; r.q_se = r.q_ll + up16((size_t)F * 8); r.q_ess = r.q_se + up16(r.rowsSe); r.q_llh = r.q_ess + up16(r.rowsT1);
    r.q_dead = r.q_llh + up16((size_t)F * Tn * 8); r.q_flags = r.q_dead + up16((size_t)F * 4); r.q_res = r.q_flags + up16((size_t)F * 4);
    r.out_bytes = r.q_res + up16((size_t)F * 4);
}
// who_sets: the entry point of a call whose time-varying array sets make the inputs large (else nullptr): its own capacity message
static int batch_stage(bssm_ctx* c, BatchRun& r, const char* who_sets = nullptr)
{
    int rc;
    void *d_in, *d_out;
    if ((rc = host_stage(c, std::max(r.in_bytes, r.out_bytes))) || (rc = pool_get(c, "b_in", r.in_bytes, &d_in))) {
        if (!who_sets) return rc;
        (void)hipGetLastError();
        g_err = std::string(who_sets) + ": the time-varying array sets do not fit the staging buffers (fewer filters or sets per call)";
        return BSSM_ERR_CAPACITY;
    }
    if ((rc = pool_get(c, "b_out", r.out_bytes, &d_out))) return rc;
    r.hs = (char*)c->h_stage; r.di = (char*)d_in; r.dq = (char*)d_out;
    return BSSM_OK;
}
// the family then sets what differs: theta_stride, log_sy, lgy, lgy_stride, move_sd (and the resampling rule where RMPF forces SISR)
static void batch_fill(const bssm_ctx* c, const bssm_pf_config* cfg, const BatchRun& r, const unsigned long long* seeds,
                       const unsigned long long* streams, BatchArgs& g)
{
    for (int f = 0; f < r.F; f++) ((PhiloxKey*)(r.hs + r.o_keys))[f] = make_key(seeds[f], streams[f]);
    if (r.ny) memcpy(r.hs + r.o_y, cfg->y, r.ny * 8);
    if (cfg->obs_times && r.T > 0) memcpy(r.hs + r.o_ot, cfg->obs_times, (size_t)r.T * 4);
    g.N = (int)r.N; g.T = r.T; g.resample_algorithm = cfg->resample_algorithm; g.resample_fn = cfg->resample_fn;
    g.lim = rec_lim(c, r.N);
    g.lit_max = c->opt_batch_lit_max; g.move_sd = 0.0; g.fold = c->opt_renormalize ? 0 : 1;
    g.threshold = threshold_or_auto(cfg->resample_algorithm, cfg->threshold, r.dN);
    g.y = (const double*)(r.di + r.o_y); g.obs_times = cfg->obs_times ? (const int*)(r.di + r.o_ot) : nullptr; g.lgy = nullptr;
    g.theta = (const double*)r.di; g.log_sy = nullptr; g.keys = (const PhiloxKey*)(r.di + r.o_keys);
    g.loglike = (double*)(r.dq + r.q_ll); g.state_est = (double*)(r.dq + r.q_se); g.ess = (double*)(r.dq + r.q_ess); g.llh = (double*)(r.dq + r.q_llh);
    g.dead = (int*)(r.dq + r.q_dead); g.flags = (uint32_t*)(r.dq + r.q_flags); g.res_calls = (int*)(r.dq + r.q_res);
    g.phase_cycles = nullptr;
}
static int batch_upload(bssm_ctx* c, const BatchRun& r)
{
    HIPCHK(hipMemcpyAsync(r.di, r.hs, r.in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(r.dq, 0, r.out_bytes, c->stream));
    return BSSM_OK;
}
// behind the launch: the end of the timed bracket, the launch's error, the download
static int batch_download(bssm_ctx* c, const BatchRun& r)
{
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(r.hs, r.dq, r.out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    return BSSM_OK;
}
static int batch_read_back(bssm_ctx* c, const BatchRun& r, bssm_pf_batch_result* res)
{
    const int F = r.F, T = r.T, dim = r.dim;
    if (res->device_ms) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1)); *res->device_ms = ms; }
    memcpy(res->loglike, r.hs + r.q_ll, (size_t)F * 8);
    if (res->state_est) memcpy(res->state_est, r.hs + r.q_se, r.rowsSe);
    if (res->ess) memcpy(res->ess, r.hs + r.q_ess, r.rowsT1);
    if (res->loglike_history && T > 0) memcpy(res->loglike_history, r.hs + r.q_llh, (size_t)F * T * 8);
    const int* dead = (const int*)(r.hs + r.q_dead); const int* nres = (const int*)(r.hs + r.q_res);
    const uint32_t* flags = (const uint32_t*)(r.hs + r.q_flags);
    int first_bad = BSSM_OK;
    for (int f = 0; f < F; f++) {
        if (res->ess) res->ess[(size_t)f * (T + 1)] = 1.0 / (r.dN * ((1.0 / r.dN) * (1.0 / r.dN)));       // :106-107
        if (res->early_return_step) res->early_return_step[f] = dead[f];
        if (res->n_res_calls) res->n_res_calls[f] = nres[f];
        if (dead[f]) {                                // the reference returns at once: later rows keep their initial values (:90-97)
            for (int i = dead[f]; i <= T; i++) {
                if (res->ess) res->ess[(size_t)f * (T + 1) + i] = 0.0;
                if (res->state_est) for (int d = 0; d < dim; d++) res->state_est[((size_t)f * (T + 1) + i) * dim + d] = (dim > 1) ? (double)NAN : 0.0;   // matrix(NA) for d > 1 (:90-95)
            }
            if (res->loglike_history) for (int i = dead[f]; i < T; i++) res->loglike_history[(size_t)f * T + i] = 0.0;
        }
        const int stf = flags[f] ? flags_to_status(flags[f]) : BSSM_OK;
        if (res->status) res->status[f] = stf;
        if (stf && !first_bad) first_bad = stf;
    }
    if (first_bad && !res->status) { g_err = bssm_status_string(first_bad); return first_bad; }
    return BSSM_OK;
}

// ---- bssm_pf_run_batch_smooth: the batched launch leaves its histories (batch_record, mv.hip.h) and one more launch traces them
// (k_trace_batch, smooth.hip.h).  The two family runners take the request; nullptr is the plain call.
struct BatchSmoothReq { int K; bssm_smooth_batch_result* out; };
struct BatchHist { BatchRec rec; size_t n_hist, n_anc, n_co, n_w; };
static const char* const BSM = "bssm_pf_run_batch_smooth";
// The histories of F filters: F ((T+1) d N 8 + cap N 4 + cap 4 + N 8) bytes, cap = max(T, 1), and the trace's outputs.  They have to fit
// what the device has free (what the pool already holds counts), and that is settled here, before anything else of the call is
// staged or launched; 128-bit arithmetic, since F T N is the caller's.
static int batch_hist_take(bssm_ctx* c, const BatchSmoothReq& q, int F, long long N, int T, int d, BatchHist& h)
{
    typedef unsigned __int128 u128;
    const u128 T1 = (u128)T + 1, cap = (u128)std::max(T, 1), K = (u128)q.K;
    const u128 b_hist = (u128)F * T1 * d * N * 8, b_anc = (u128)F * cap * N * 4, b_co = (u128)F * cap * 4, b_w = (u128)F * N * 8;
    const u128 b_out = (u128)F * (T1 * d * 8 + T1 * 4 + K * T1 * d * 8 + K * 12 + 4) + 128;
    const std::pair<const char*, u128> bufs[] = {{"bs_hist", b_hist}, {"bs_anc", b_anc}, {"bs_co", b_co}, {"bs_w", b_w}, {"bs_out", b_out}};
    u128 need = 0, grow = 0;
    for (const auto& b : bufs) {
        need += b.second;
        const auto it = c->pool.find(b.first);
        const u128 have = it == c->pool.end() ? 0 : it->second.second;
        if (have < b.second) grow += b.second + b.second / 4 + 256 - have;
    }
    size_t mfree = 0, mtotal = 0;
    HIPCHK(hipMemGetInfo(&mfree, &mtotal));
    if (grow > (u128)mfree) {
        const auto str = [](u128 v) { return v > (u128)UINT64_MAX ? std::string("more than 2^64") : std::to_string((unsigned long long)v); };
        g_err = std::string(BSM) + ": the histories, ancestor rows and trace outputs of " + std::to_string(F) + " filters need " + str(need) +
                " bytes of device memory (" + str(grow) + " more than this context holds, " + std::to_string((unsigned long long)mfree) +
                " free); fewer filters per call";
        return BSSM_ERR_CAPACITY;
    }
    h.n_hist = (size_t)b_hist; h.n_anc = (size_t)b_anc; h.n_co = (size_t)b_co; h.n_w = (size_t)b_w;
    int rc;
    if ((rc = pool_get(c, "bs_hist", h.n_hist, &h.rec.hist))) return rc;
    if ((rc = pool_get(c, "bs_anc", h.n_anc, &h.rec.anc))) return rc;
    if ((rc = pool_get(c, "bs_co", h.n_co, &h.rec.call_obs))) return rc;
    if ((rc = pool_get(c, "bs_w", h.n_w, &h.rec.W))) return rc;
    h.rec.cap = std::max(T, 1);
    return BSSM_OK;
}
// behind batch_download (the stream is drained, the filters' own outputs are in the staging buffer): the trace and its outputs.
// g: the launch's arguments -- res_calls, dead, flags and the keys are still on the device
static int batch_trace(bssm_ctx* c, const BatchRun& r, const BatchArgs& g, const BatchSmoothReq& q, const BatchHist& h)
{
    bssm_smooth_batch_result* o = q.out;
    const int F = r.F, T = r.T, d = r.dim, K = q.K;
    const size_t T1 = (size_t)T + 1;
    const size_t n_sm = up16((size_t)F * T1 * d * 8), n_nl = up16((size_t)F * T1 * 4), n_tr = up16((size_t)F * K * T1 * d * 8), n_u = up16((size_t)F * K * 8),
                 n_ix = up16((size_t)F * K * 4), n_td = up16((size_t)F * 4);
    char* dout; int rc;
    if ((rc = pool_get(c, "bs_out", n_sm + n_nl + n_tr + n_u + n_ix + n_td, &dout))) return rc;
    TraceBatchArgs a;
    a.hist = h.rec.hist; a.W = h.rec.W; a.anc = h.rec.anc; a.call_obs = h.rec.call_obs; a.cap = h.rec.cap;
    a.res_calls = g.res_calls; a.dead = g.dead; a.flags = g.flags; a.keys = g.keys;
    a.N = (int)r.N; a.T = T; a.d = d; a.K = K;
    a.smoothed = (double*)dout; a.nlin = (int*)(dout + n_sm); a.traj = (double*)(dout + n_sm + n_nl); a.u = (double*)(dout + n_sm + n_nl + n_tr);
    a.idx = (int*)(dout + n_sm + n_nl + n_tr + n_u); a.traced = (int*)(dout + n_sm + n_nl + n_tr + n_u + n_ix);
    hipEvent_t ea = prof_event(c), eb = prof_event(c);
    HIPCHK(hipEventRecord(ea, c->stream));
    LAUNCH(c, "k_trace_batch", k_trace_batch, F, NT, 0, a);
    HIPCHK(hipEventRecord(eb, c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(o->smoothed, a.smoothed, (size_t)F * T1 * d * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->n_lineages, a.nlin, (size_t)F * T1 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->traced, a.traced, (size_t)F * 4, hipMemcpyDeviceToHost, c->stream));
    if (K > 0) {
        HIPCHK(hipMemcpyAsync(o->trajectories, a.traj, (size_t)F * K * T1 * d * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(o->trajectory_u, a.u, (size_t)F * K * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(o->trajectory_index, a.idx, (size_t)F * K * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ea, eb));
    c->ev_pool.push_back(ea); c->ev_pool.push_back(eb);
    if (o->smooth_ms) *o->smooth_ms = ms;
    return BSSM_OK;
}

// bssm_pf_run_batch / bssm_pf_run_batch_tv for the multivariate linear-Gaussian family (k_pf_batch_mv): thetas [F][n_theta]
// packed blocks as bssm_pf_run takes them (without log(sd)), all of one (d, p); cfg->y [T][p]; state_est [F][T+1][d].
// tvb: the array sets of bssm_pf_run_batch_tv, or nullptr: cfg->mv_tv, one array per piece shared by the filters.
// who: the entry point, for the messages.
static int pf_run_batch_mv(bssm_ctx* c, const bssm_pf_config* cfg, int F, const double* thetas, const unsigned long long* seeds,
                           const unsigned long long* streams, bssm_pf_batch_result* res, const bssm_mv_tv_batch* tvb, const char* who,
                           const BatchSmoothReq* smq = nullptr)
{
    const std::string W = std::string(who) + ": ";
    const long long N = cfg->num_particles;
    const int T = cfg->T, nth = cfg->n_theta;
    const int obs = mv_obs_of(cfg->model);                          // (the callers dispatched on it)
    if (T < 0) ARGFAIL(W + "T must be >= 0");
    if (cfg->algorithm != BSSM_BPF) ARGFAIL(W + "the multivariate family runs the bootstrap filter");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL(W + "unknown resample_algorithm");
    if (cfg->resample_fn != BSSM_STRATIFIED && cfg->resample_fn != BSSM_SYSTEMATIC) ARGFAIL(W + "the multivariate family resamples stratified / systematic");
    if (cfg->z_init || cfg->z_trans || cfg->u_res || cfg->return_particles || cfg->return_ancestors)
        ARGFAIL(W + "injected draws and histories are not available in the batched path");
    if (nth < 2) ARGFAIL(W + "the multivariate model needs its packed parameter blocks");
    MvPar mp; mp.P = nullptr; mp.d = (int)thetas[0]; mp.p = (int)thetas[1];
    const int d = mp.d, p = mp.p;
    if (d < 1 || d > MVD || p < 0 || p > MVD || thetas[0] != (double)d || thetas[1] != (double)p) ARGFAIL(W + "multivariate model: 1 <= d <= 8, 0 <= p <= 8");
    if (nth != mp.o_lsd()) ARGFAIL(W + "multivariate model: parameter block has the wrong length");
    for (int f = 0; f < F; f++) {
        const double* th = thetas + (size_t)f * nth;
        if (th[0] != thetas[0] || th[1] != thetas[1]) ARGFAIL(W + "multivariate model: every block of one call must have the same (d, p)");
        if (obs == MV_OBS_GAUSS) for (int k = 0; k < p; k++) if (!(th[mp.o_sd() + k] > 0)) ARGFAIL(W + "multivariate model: observation sd must be positive");
    }
    if (N > mv_batch_max_particles(d)) {
        g_err = W + "a batched filter of the multivariate family holds at most bssm_pf_batch_max_particles_mv(d) particles; use bssm_pf_run";
        return BSSM_ERR_CAPACITY;
    }
    if (T > 0 && p > 0 && !cfg->y) ARGFAIL(W + "y is NULL");
    if (!res->loglike) ARGFAIL(W + "loglike buffer missing");
    const bool skip = c->opt_mv_y_missing != 0;
    { const int rc_y = mv_y_check(cfg->y, T * p, skip); if (rc_y) return rc_y; }
    { const int rc_obs = mv_obs_check(W, obs, p, cfg->y, T, skip); if (rc_obs) return rc_obs; }
    if (int rc_o = obs_times_check(cfg->obs_times, T)) return rc_o;
    bssm_mv_tv_batch one;
    if (!tvb && cfg->mv_tv) { one = mv_tv_as_batch(cfg->mv_tv); tvb = &one; }
    if (tvb) { const int rc_tv = mv_tvb_check(who, cfg, d, p, F, tvb); if (rc_tv) return rc_tv; }
    const bssm_mv_tv_batch* tv = T > 0 ? tvb : nullptr;
    // doubles of one set of each piece, and how many sets of it travel (1: the one shared array)
    const size_t n_bt = (tv && tv->b_t && tv->n_times > 0) ? (size_t)tv->n_times * d : 0, n_h0t = (tv && tv->h0_t) ? (size_t)T * p : 0,
                 n_Ht = (tv && tv->H_t) ? (size_t)T * p * d : 0;
    const size_t g_bt = (n_bt && tv->b_stride) ? (size_t)tv->n_sets : 1, g_h0t = (n_h0t && tv->h0_stride) ? (size_t)tv->n_sets : 1,
                 g_Ht = (n_Ht && tv->H_stride) ? (size_t)tv->n_sets : 1;
    const bool sets = g_bt > 1 || g_h0t > 1 || g_Ht > 1;             // some piece has more than one set: the filters' set indices travel too
    HIPCHK(hipSetDevice(c->device));
    const int psz = mp.size();                                      // the device block: + log(sd)
    int rc;
    BatchHist bh;
    if (smq && (rc = batch_hist_take(c, *smq, F, N, T, d, bh))) return rc;
    // behind obs_times: the array sets, the filters' set indices (shared arrays only: the same bytes as before the sets), and for
    // Poisson lgamma(y + 1), [T][p]
    const size_t s_bt = up16(n_bt * g_bt * 8), s_h0t = up16(n_h0t * g_h0t * 8), s_Ht = up16(n_Ht * g_Ht * 8), s_set = sets ? up16((size_t)F * 4) : 0,
                 s_lgy = (obs == MV_OBS_POIS && T > 0) ? up16((size_t)std::max(T * p, 1) * 8) : 0;
    BatchRun r;
    batch_layout(r, F, N, T, d, (size_t)T * p, up16((size_t)F * psz * 8), 0, s_bt + s_h0t + s_Ht + s_set + s_lgy);
    const size_t o_bt = r.o_tail, o_h0t = o_bt + s_bt, o_Ht = o_h0t + s_h0t, o_set = o_Ht + s_Ht, o_lgy = o_set + s_set;
    if ((rc = batch_stage(c, r, sets ? who : nullptr))) return rc;
    BatchArgs g;
    batch_fill(c, cfg, r, seeds, streams, g);
    for (int f = 0; f < F; f++) mv_fill_block((double*)r.hs + (size_t)f * psz, thetas + (size_t)f * nth, mp, obs);      // as pf_run_mv
    if (obs == MV_OBS_POIS) for (int i = 0; i < T * p; i++) ((double*)(r.hs + o_lgy))[i] = mv_lgy(cfg->y[i]);      // as pf_run_mv
    if (n_bt) memcpy(r.hs + o_bt, tv->b_t, n_bt * g_bt * 8);
    if (n_h0t) memcpy(r.hs + o_h0t, tv->h0_t, n_h0t * g_h0t * 8);
    if (n_Ht) memcpy(r.hs + o_Ht, tv->H_t, n_Ht * g_Ht * 8);
    if (sets) for (int f = 0; f < F; f++) ((int*)(r.hs + o_set))[f] = tv->set_of ? tv->set_of[f] : f;      // (checked: without set_of, n_sets == F)
    if ((rc = batch_upload(c, r))) return rc;
    MvTvBatch gt;
    gt.b = n_bt ? (const double*)(r.di + o_bt) : nullptr; gt.h0 = n_h0t ? (const double*)(r.di + o_h0t) : nullptr;
    gt.H = n_Ht ? (const double*)(r.di + o_Ht) : nullptr; gt.n_times = n_bt ? tv->n_times : 0;
    gt.set_of = sets ? (const int*)(r.di + o_set) : nullptr;
    gt.sb = g_bt > 1 ? (long long)n_bt : 0; gt.sh0 = g_h0t > 1 ? (long long)n_h0t : 0; gt.sH = g_Ht > 1 ? (long long)n_Ht : 0;
    g.theta_stride = psz;
    if (s_lgy) g.lgy = (const double*)(r.di + o_lgy);
    const size_t dyn = mv_batch_dyn_lds(d, N);
    HIPCHK(hipEventRecord(c->ev0, c->stream));
#define BATCH_MV_R(DM, OBS, REC, rec) do { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pf_batch_mv<DM, OBS, REC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn)); \
                               LAUNCH(c, "k_pf_batch_mv", (k_pf_batch_mv<DM, OBS, REC>), F, NT, dyn, g, d, p, gt, rec); } while (0)
#define BATCH_MV(DM, OBS) do { if (smq) BATCH_MV_R(DM, OBS, BatchRec, bh.rec); else BATCH_MV_R(DM, OBS, BatchNoRec, BatchNoRec()); } while (0)
#define BATCH_MV_D(OBS) do { if (d <= 2) BATCH_MV(2, OBS); else if (d <= 4) BATCH_MV(4, OBS); else BATCH_MV(8, OBS); } while (0)
    if (obs == MV_OBS_POIS) BATCH_MV_D(MV_OBS_POIS); else if (obs == MV_OBS_LOGVAR) BATCH_MV_D(MV_OBS_LOGVAR); else BATCH_MV_D(MV_OBS_GAUSS);
#undef BATCH_MV_D
#undef BATCH_MV
#undef BATCH_MV_R
    if ((rc = batch_download(c, r))) return rc;
    if (smq && (rc = batch_trace(c, r, g, *smq, bh))) return rc;
    return batch_read_back(c, r, res);
}

// bssm_pf_run_batch for the reaction-network family (k_pf_batch_rn): thetas [F][n_theta] packed blocks as bssm_pf_run takes them,
// all of one (d, R, p) and one length (with or without the counters' tail and the rate schedule, one schedule per filter); cfg->y [T][p]; state_est [F][T+1][d].
extern "C" int bssm_pf_batch_max_particles_rn(int d) { return rn_batch_max_particles(d); }

// nb: BSSM_MODEL_RNET_NB -- the blocks carry size[p], and the table c(t, k) is the filter's own: [F][T][p], filled here on the host
static int pf_run_batch_rn(bssm_ctx* c, const bssm_pf_config* cfg, int F, const double* thetas, const unsigned long long* seeds,
                           const unsigned long long* streams, bssm_pf_batch_result* res, bool nb, const char* who = "bssm_pf_run_batch",
                           const BatchSmoothReq* smq = nullptr)
{
    const std::string W = std::string(who) + ": ";
    const long long N = cfg->num_particles;
    const int T = cfg->T, nth = cfg->n_theta;
    if (T < 0) ARGFAIL(W + "T must be >= 0");
    if (cfg->algorithm != BSSM_BPF) ARGFAIL(W + "the reaction-network family runs the bootstrap filter in the batched path");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL(W + "unknown resample_algorithm");
    if (cfg->resample_fn != BSSM_STRATIFIED && cfg->resample_fn != BSSM_SYSTEMATIC) ARGFAIL(W + "the reaction-network family resamples stratified / systematic");
    if (cfg->z_init || cfg->z_trans || cfg->u_res || cfg->return_particles || cfg->return_ancestors)
        ARGFAIL(W + "injected draws and histories are not available in the batched path");
    RnPar rp;
    if (c->opt_rn_noise && c->opt_rn_method != 1) ARGFAIL(W + "reaction network: rn_noise = 1 (gamma white noise on the rates) needs rn_method = 1 (Euler-multinomial leaps)");      // (as pf_run_rn)
    const bool gwn = c->opt_rn_noise != 0;
    for (int f = 0; f < F; f++) {
        RnPar rf;
        const int rc_b = rn_block_check(W, thetas + (size_t)f * nth, nth, rf, nb, gwn); if (rc_b) return rc_b;
        if (f == 0) rp = rf;
        else if (rf.d != rp.d || rf.R != rp.R || rf.p != rp.p) ARGFAIL(W + "reaction network: every block of one call must have the same (d, R, p)");
    }
    const int d = rp.d, p = rp.p;
    if (N > rn_batch_max_particles(d)) {
        g_err = W + "a batched filter of the reaction-network family holds at most bssm_pf_batch_max_particles_rn(d) particles; use bssm_pf_run";
        return BSSM_ERR_CAPACITY;
    }
    if (T > 0 && !cfg->y) ARGFAIL(W + "y is NULL");
    if (!res->loglike) ARGFAIL(W + "loglike buffer missing");
    const bool skip = c->opt_mv_y_missing != 0;
    { const int rc_y = mv_y_check(cfg->y, T * p, skip); if (rc_y) return rc_y; }
    { const int rc_obs = mv_obs_check(W, MV_OBS_POIS, p, cfg->y, T, skip); if (rc_obs) return rc_obs; }
    if (int rc_o = obs_times_check(cfg->obs_times, T)) return rc_o;
    { const int rc_s = rn_sched_check(W, rp, T, cfg->obs_times); if (rc_s) return rc_s; }       // (one length, hence one n_times for every block)
    const bool em = c->opt_rn_method == 1;               // (as pf_run_rn)
    if (em) for (int f = 0; f < F; f++) { const int rc_e = rn_em_check(W, thetas + (size_t)f * nth, rp, c->opt_rn_leaps); if (rc_e) return rc_e; }
    HIPCHK(hipSetDevice(c->device));
    int rc;
    BatchHist bh;
    if (smq && (rc = batch_hist_take(c, *smq, F, N, T, d, bh))) return rc;
    BatchRun r;                                          // behind obs_times: the table lgy, one per filter for negative-binomial counts
    batch_layout(r, F, N, T, d, (size_t)T * p, up16((size_t)F * nth * 8), 0, up16((nb ? (size_t)F : 1) * (size_t)std::max(T * p, 1) * 8));
    if ((rc = batch_stage(c, r))) return rc;
    BatchArgs g;
    batch_fill(c, cfg, r, seeds, streams, g);
    memcpy(r.hs, thetas, (size_t)F * nth * 8);
    if (rp.n_times) for (int f = 0; f < F; f++) rn_sched_products(rp, (double*)r.hs + (size_t)f * nth);   // as pf_run_rn
    if (nb) { const int rc_t = bssm_rn_nb_tables(cfg->y, T, p, F, thetas + rp.o_size(), nth, (double*)(r.hs + r.o_tail)); if (rc_t) return rc_t; }   // as pf_run_rn, per filter
    else for (int i = 0; i < T * p; i++) ((double*)(r.hs + r.o_tail))[i] = mv_lgy(cfg->y[i]);       // as pf_run_rn
    if ((rc = batch_upload(c, r))) return rc;
    g.theta_stride = nth; g.lgy = (const double*)(r.di + r.o_tail); g.lgy_stride = nb ? (long long)T * p : 0;
    const size_t dyn = mv_batch_dyn_lds(d, N);
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    const int leaps = c->opt_rn_leaps;                      // (the context option rn_leaps, as pf_run_rn reads it)
#define BATCH_RN_R(DM, OB, MT, REC, rec) do { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pf_batch_rn<DM, OB, MT, REC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn)); \
                          LAUNCH(c, "k_pf_batch_rn", (k_pf_batch_rn<DM, OB, MT, REC>), F, NT, dyn, g, d, rp.R, p, leaps, rec); } while (0)
#define BATCH_RN_MT(DM, OB, MT) do { if (smq) BATCH_RN_R(DM, OB, MT, BatchRec, bh.rec); else BATCH_RN_R(DM, OB, MT, BatchNoRec, BatchNoRec()); } while (0)
#define BATCH_RN_OB(DM, OB) do { if (em && gwn) BATCH_RN_MT(DM, OB, RN_EULER_MULTINOM_GWN); else if (em) BATCH_RN_MT(DM, OB, RN_EULER_MULTINOM); else if (leaps > 0) BATCH_RN_MT(DM, OB, RN_TAU_LEAP); else BATCH_RN_MT(DM, OB, RN_GILLESPIE); } while (0)
#define BATCH_RN(DM) do { if (nb) BATCH_RN_OB(DM, RN_OBS_NB); else BATCH_RN_OB(DM, RN_OBS_POIS); } while (0)
    if (d <= 2) BATCH_RN(2); else if (d <= 4) BATCH_RN(4); else BATCH_RN(8);
#undef BATCH_RN
#undef BATCH_RN_OB
#undef BATCH_RN_MT
#undef BATCH_RN_R
    if ((rc = batch_download(c, r))) return rc;
    if (smq && (rc = batch_trace(c, r, g, *smq, bh))) return rc;
    return batch_read_back(c, r, res);
}

extern "C" int bssm_pf_run_batch_tv(bssm_ctx* c, const bssm_pf_config* cfg, int n_filters, const double* thetas, const unsigned long long* seeds,
                                    const unsigned long long* streams, const bssm_mv_tv_batch* tv, bssm_pf_batch_result* res)
{
    if (!c || !cfg || !res || !thetas || !seeds || !streams || !tv) ARGFAIL("bssm_pf_run_batch_tv: NULL argument");
    if (n_filters <= 0) ARGFAIL("bssm_pf_run_batch_tv: n_filters must be positive");
    if (cfg->num_particles <= 0) ARGFAIL("num_particles must be a positive count");
    if (mv_obs_of(cfg->model) < 0) ARGFAIL("bssm_pf_run_batch_tv: the multivariate linear-Gaussian family (BSSM_MODEL_LGMV, BSSM_MODEL_LGMV_POIS, BSSM_MODEL_LGMV_LOGVAR) only");
    if (cfg->mv_tv) ARGFAIL("bssm_pf_run_batch_tv: mv_tv: cfg->mv_tv must be NULL (the arrays come in the bssm_mv_tv_batch)");
    return pf_run_batch_mv(c, cfg, n_filters, thetas, seeds, streams, res, tv, "bssm_pf_run_batch_tv");
}

// The batched smoother's entry point: bssm_pf_run_batch / bssm_pf_run_batch_tv with the recording form of the family's kernel, then
// the trace of every filter in one launch.
extern "C" int bssm_pf_run_batch_smooth(bssm_ctx* c, const bssm_pf_config* cfg, int n_filters, const double* thetas, const unsigned long long* seeds,
                                        const unsigned long long* streams, const bssm_mv_tv_batch* tv, bssm_pf_batch_result* res,
                                        const bssm_smooth_config* scfg, bssm_smooth_batch_result* sres)
{
    const std::string W = std::string(BSM) + ": ";
    if (!c || !cfg || !res || !thetas || !seeds || !streams) ARGFAIL(W + "NULL argument");
    if (!scfg || !sres) ARGFAIL(W + "the smoother's config and result structs are required");
    const int K = scfg->n_trajectories;
    if (K < 0 || K > TRACE_MAX_K) ARGFAIL(W + "n_trajectories must be 0 .. 4096");
    if (!sres->smoothed || !sres->n_lineages || !sres->traced) ARGFAIL(W + "smoothed / n_lineages / traced buffers missing");
    if (K > 0 && (!sres->trajectories || !sres->trajectory_u || !sres->trajectory_index)) ARGFAIL(W + "trajectory buffers missing");
    if (n_filters <= 0) ARGFAIL(W + "n_filters must be positive");
    if (cfg->num_particles <= 0) ARGFAIL("num_particles must be a positive count");
    const bool mv = mv_obs_of(cfg->model) >= 0, rn = cfg->model == BSSM_MODEL_RNET || cfg->model == BSSM_MODEL_RNET_NB;
    const char* const covers = "covers the bootstrap filter of the multivariate linear-Gaussian family (BSSM_MODEL_LGMV*) and of the reaction networks "
                               "(BSSM_MODEL_RNET, BSSM_MODEL_RNET_NB) with stratified / systematic resampling";
    if (!mv && !rn) ARGFAIL(W + "the scalar models run on a batched kernel that keeps no history; this entry point " + covers);
    if (cfg->algorithm != BSSM_BPF) ARGFAIL(W + "no batched APF / RMPF exists for these families; this entry point " + covers);
    if (cfg->resample_fn != BSSM_STRATIFIED && cfg->resample_fn != BSSM_SYSTEMATIC) ARGFAIL(W + "multinomial resampling is not available; this entry point " + covers);
    if (tv && !mv) ARGFAIL(W + "mv_tv: the array sets belong to the multivariate linear-Gaussian family");
    if (tv && cfg->mv_tv) ARGFAIL(W + "mv_tv: cfg->mv_tv must be NULL (the arrays come in the bssm_mv_tv_batch)");
    const BatchSmoothReq q{K, sres};
    if (sres->smooth_ms) *sres->smooth_ms = 0.0;
    if (mv) return pf_run_batch_mv(c, cfg, n_filters, thetas, seeds, streams, res, tv, BSM, &q);
    return pf_run_batch_rn(c, cfg, n_filters, thetas, seeds, streams, res, cfg->model == BSSM_MODEL_RNET_NB, BSM, &q);
}

extern "C" int bssm_pf_run_batch(bssm_ctx* c, const bssm_pf_config* cfg, int n_filters, const double* thetas,
                                 const unsigned long long* seeds, const unsigned long long* streams, bssm_pf_batch_result* res)
{
    if (!c || !cfg || !res || !thetas || !seeds || !streams) ARGFAIL("bssm_pf_run_batch: NULL argument");
    const long long N = cfg->num_particles;
    const int T = cfg->T, F = n_filters;
    if (F <= 0) ARGFAIL("bssm_pf_run_batch: n_filters must be positive");
    if (N <= 0) ARGFAIL("num_particles must be a positive count");
    if (mv_obs_of(cfg->model) >= 0) return pf_run_batch_mv(c, cfg, F, thetas, seeds, streams, res, nullptr, "bssm_pf_run_batch");
    if (cfg->model == BSSM_MODEL_RNET || cfg->model == BSSM_MODEL_RNET_NB) return pf_run_batch_rn(c, cfg, F, thetas, seeds, streams, res, cfg->model == BSSM_MODEL_RNET_NB);
    if (N > EB) { g_err = "bssm_pf_run_batch: a batched filter holds at most 2048 particles (one workgroup); use bssm_pf_run"; return BSSM_ERR_CAPACITY; }
    if (T < 0) ARGFAIL("bssm_pf_run_batch: T must be >= 0");
    if (cfg->model != BSSM_MODEL_LG && cfg->model != BSSM_MODEL_AR1SIN && cfg->model != BSSM_MODEL_SIR) ARGFAIL("bssm_pf_run_batch: unknown model");
    const bool sir = cfg->model == BSSM_MODEL_SIR;
    const int dim = sir ? 2 : 1;
    if (cfg->algorithm != BSSM_BPF && cfg->algorithm != BSSM_APF && cfg->algorithm != BSSM_RMPF) ARGFAIL("bssm_pf_run_batch: unknown algorithm");
    const bool apf = cfg->algorithm == BSSM_APF, rmpf = cfg->algorithm == BSSM_RMPF;
    if (rmpf && cfg->model == BSSM_MODEL_SIR) ARGFAIL("bssm_pf_run_batch: the built-in move step is defined for the scalar Gaussian-observation models only");
    if (rmpf && !(cfg->move_sd > 0)) ARGFAIL("bssm_pf_run_batch: RMPF needs move_sd > 0");
    if (rmpf && (cfg->z_move || cfg->u_move)) ARGFAIL("bssm_pf_run_batch: injected draws are not available in the batched path");
    if (cfg->resample_algorithm < 0 || cfg->resample_algorithm > 2) ARGFAIL("bssm_pf_run_batch: unknown resample_algorithm");
    if (cfg->resample_fn < 0 || cfg->resample_fn > 2) ARGFAIL("bssm_pf_run_batch: unknown resample_fn");
    if (cfg->z_init || cfg->z_trans || cfg->u_res || cfg->return_particles || cfg->return_ancestors)
        ARGFAIL("bssm_pf_run_batch: injected draws and histories are not available in the batched path");
    if (cfg->n_theta < (sir ? 5 : 3)) ARGFAIL("bssm_pf_run_batch: theta rows must hold (phi, sigma_x, sigma_y) or (lambda, gamma, n_total, s0, i0)");
    if (T > 0 && !cfg->y) ARGFAIL("bssm_pf_run_batch: y is NULL");
    if (!res->loglike) ARGFAIL("bssm_pf_run_batch: loglike buffer missing");
    for (int i = 0; i < T; i++) if (!isfinite(cfg->y[i])) ARGFAIL("Assertion on 'y' failed: Contains missing values");
    if (int rc_o = obs_times_check(cfg->obs_times, T)) return rc_o;
    HIPCHK(hipSetDevice(c->device));
    const int nth = cfg->n_theta;
    int rc;
    const size_t o_lsy = up16((size_t)F * nth * 8), s_lgy = up16((size_t)std::max(T, 1) * 8);       // log(sigma_y) [F] behind the thetas; lgy [T] behind y
    BatchRun r;
    batch_layout(r, F, N, T, dim, (size_t)T, o_lsy + up16((size_t)F * 8), s_lgy, 0);
    if ((rc = batch_stage(c, r))) return rc;
    BatchArgs g;
    batch_fill(c, cfg, r, seeds, streams, g);
    memcpy(r.hs, thetas, (size_t)F * nth * 8);
    for (int f = 0; f < F; f++) ((double*)(r.hs + o_lsy))[f] = log(thetas[(size_t)f * nth + 2]);                      // as bssm_pf_run: log(sigma_y) on the host
    for (int i = 0; i < T; i++) ((double*)(r.hs + r.o_mid))[i] = sir ? lgamma(cfg->y[i] + 1.0) : 0.0;   // as bssm_pf_run: lgamma(y + 1) on the host
    if ((rc = batch_upload(c, r))) return rc;
    g.theta_stride = nth; g.log_sy = (const double*)(r.di + o_lsy); g.move_sd = cfg->move_sd;
    if (sir) g.lgy = (const double*)(r.di + r.o_mid);
    if (rmpf) { g.resample_algorithm = BSSM_SISR; g.threshold = threshold_or_auto(BSSM_SISR, (double)NAN, r.dN); }      // RMPF forces SISR (R/resample_move_filter.R:229)
    void* d_ph = nullptr;
    if (c->opt_debug_stop == 97) { if ((rc = pool_get(c, "b_ph", 40 * 8, &d_ph))) return rc; HIPCHK(hipMemsetAsync(d_ph, 0, 40 * 8, c->stream)); g.phase_cycles = (long long*)d_ph; }
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    const int alg = apf ? 1 : rmpf ? 2 : 0;
    const size_t bshm = (cfg->resample_fn == BSSM_MULTINOMIAL) ? (size_t)EB * sizeof(double) : 0;     // the exact cum_sum for the inverse-CDF search
#define BATCH(M, A) do { if (bshm) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pf_batch<M, A>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bshm)); \
                         LAUNCH(c, "k_pf_batch", (k_pf_batch<M, A>), F, NT, bshm, g); } while (0)
    if (cfg->model == BSSM_MODEL_LG) { if (alg == 0) BATCH(0, 0); else if (alg == 1) BATCH(0, 1); else BATCH(0, 2); }
    else if (cfg->model == BSSM_MODEL_AR1SIN) { if (alg == 0) BATCH(1, 0); else if (alg == 1) BATCH(1, 1); else BATCH(1, 2); }
    else { if (alg == 0) BATCH(2, 0); else BATCH(2, 1); }
#undef BATCH
    if ((rc = batch_download(c, r))) return rc;
    if (d_ph) { long long h[40]; HIPCHK(hipMemcpy(h, d_ph, 40 * 8, hipMemcpyDeviceToHost));
        const long long* w2 = h + 8; const long long* a3 = h + 24;
        fprintf(stderr, "   last observation, weights block: start->prologue %lld, ->weights %lld, ->terms ready %lld;  apply block: start->loaded %lld, ->in-order/resolve %lld, ->counts %lld, ->expanded %lld, ->state est %lld\n",
                w2[8] - w2[4], w2[9] - w2[8], w2[1] - w2[9], a3[1] - a3[0], a3[3] - a3[1], a3[4] - a3[3], a3[5] - a3[4], a3[6] - a3[5]); fprintf(stderr, "k_pf_batch filter 0 cycles/observation: step %lld, weights+scan<W> %lld, apply %lld, carry/store %lld\n", h[0] / std::max(T, 1), h[1] / std::max(T, 1), h[2] / std::max(T, 1), h[3] / std::max(T, 1)); }
    return batch_read_back(c, r, res);
}

// ---- PMMH: one chain --------------------------------------------------------------------
// Chain-level draws (proposal normals, acceptance uniform) come from the same
// counter-based generator, keyed by the chain seed: results do not depend on
// which GPU runs the chain.
static double host_normal(const PhiloxKey& key, uint32_t iter, uint32_t j)
{
    u32x4 cn; cn.x = j; cn.y = iter; cn.z = DRAW_PROPOSAL; cn.w = key.stream;
    const u32x4 r = philox4x32_10(cn, key.k0, key.k1);
    return qnorm_as241(u01_from_bits(r.x, r.y));
}
static double host_uniform(const PhiloxKey& key, uint32_t iter)
{
    u32x4 cn; cn.x = 0; cn.y = iter; cn.z = DRAW_ACCEPT; cn.w = key.stream;
    const u32x4 r = philox4x32_10(cn, key.k0, key.k1);
    return u01_from_bits(r.x, r.y);
}
static double log_prior(int kind, double a, double b, double x)
{
    switch (kind) {
        case BSSM_PRIOR_NORMAL: { const double z = (x - a) / b; return -(BSSM_LN_SQRT_2PI + 0.5 * z * z + log(b)); }   // dnorm(log=TRUE)
        case BSSM_PRIOR_EXP: return (x < 0) ? -INFINITY : (log(a) - a * x);                                         // dexp(rate, log=TRUE)
        case BSSM_PRIOR_UNIFORM: return (x >= a && x <= b) ? -log(b - a) : -INFINITY;                               // dunif(log=TRUE)
        case BSSM_PRIOR_HALFNORMAL: { if (x < 0) return -INFINITY; const double z = x / a;                          // extraDistr::dhnorm(x, sigma = a, log = TRUE)
                                      return log(2.0) - (BSSM_LN_SQRT_2PI + 0.5 * z * z + log(a)); }
        default: return 0.0;
    }
}
static double tr_fwd(int tr, double x) { return tr == BSSM_TR_LOG ? log(x) : tr == BSSM_TR_LOGIT ? log(x / (1 - x)) : x; }          // R/utils.R:102-112
static double tr_back(int tr, double z) { return tr == BSSM_TR_LOG ? exp(z) : tr == BSSM_TR_LOGIT ? 1 / (1 + exp(-z)) : z; }        // R/utils.R:122-132
static double tr_logjac(int tr, double x) { return tr == BSSM_TR_LOG ? log(x) : tr == BSSM_TR_LOGIT ? log(1 / (x * (1 - x))) : 0.0; }  // R/utils.R:142-152

// fac = V diag(sqrt(max(ev, 0))) of the symmetric matrix S (row-major p x p)
static int eigen_factor(int p, const double* S, double* fac)
{
    std::vector<double> A((size_t)p * p), V((size_t)p * p);
    for (int a = 0; a < p; a++) for (int b = 0; b < p; b++) { A[a * p + b] = 0.5 * (S[a * p + b] + S[b * p + a]); V[a * p + b] = (a == b); }
    for (int sweep = 0; sweep < 100; sweep++) {
        double off = 0.0;
        for (int a = 0; a < p; a++) for (int b = a + 1; b < p; b++) off += A[a * p + b] * A[a * p + b];
        if (off == 0.0) break;
        for (int a = 0; a < p - 1; a++) for (int b = a + 1; b < p; b++) {
            const double apq = A[a * p + b];
            if (apq == 0.0) continue;
            const double th = (A[b * p + b] - A[a * p + a]) / (2.0 * apq);
            const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
            for (int k = 0; k < p; k++) {
                const double aka = A[k * p + a], akb = A[k * p + b];
                A[k * p + a] = c * aka - sn * akb; A[k * p + b] = sn * aka + c * akb;
                const double vka = V[k * p + a], vkb = V[k * p + b];
                V[k * p + a] = c * vka - sn * vkb; V[k * p + b] = sn * vka + c * vkb;
            }
            for (int k = 0; k < p; k++) {
                const double aak = A[a * p + k], abk = A[b * p + k];
                A[a * p + k] = c * aak - sn * abk; A[b * p + k] = sn * aak + c * abk;
            }
        }
    }
    std::vector<int> order(p);
    for (int k = 0; k < p; k++) order[k] = k;
    for (int i = 1; i < p; i++) {
        const int o = order[i]; int j = i - 1;
        while (j >= 0 && A[order[j] * p + order[j]] < A[o * p + o]) { order[j + 1] = order[j]; j--; }
        order[j + 1] = o;
    }
    const double ev0 = A[order[0] * p + order[0]];
    for (int k = 0; k < p; k++) {
        const int o = order[k];
        const double ev = A[o * p + o];
        if (!(ev >= -1e-6 * fabs(ev0))) ARGFAIL("'Sigma' is not positive definite");
        int big = 0;
        for (int a = 1; a < p; a++) if (fabs(V[a * p + o]) > fabs(V[big * p + o])) big = a;
        const double sg = (V[big * p + o] < 0) ? -1.0 : 1.0;
        for (int a = 0; a < p; a++) fac[a * p + k] = (sg * V[a * p + o]) * sqrt(ev > 0 ? ev : 0.0);
    }
    return BSSM_OK;
}

// One chain's Metropolis-Hastings state: everything of R/pmmh.R:345-505 except the filter run itself, so that the
// same code drives one chain over bssm_pf_run and many chains in lock-step over bssm_pf_run_batch.
struct ChainState {
    const bssm_pmmh_config* cfg; bssm_pmmh_result* res;
    int p, m, T, dim, n_full;
    std::vector<double> L, cur, prop, lp_prop, th_full, se_cur, se_prop;
    PhiloxKey ckey;
    double cur_ll; int accepted;

    int init(const bssm_pmmh_config* cfg_, bssm_pmmh_result* res_)
    {
        cfg = cfg_; res = res_;
        if (!cfg || !res) ARGFAIL("bssm_pmmh_chain: NULL argument");
        p = cfg->n_params; m = cfg->m; T = cfg->pf.T;
        if (p < 1 || p > 16) ARGFAIL("bssm_pmmh_chain: n_params out of range");
        if (m < 1) ARGFAIL("Assertion on 'm' failed: Must be >= 1");                         // assert_int(m, lower = 1) R/pmmh.R:264
        if (!cfg->init_theta || !cfg->proposal_cov || !cfg->transform || !cfg->prior_kind || !cfg->prior_a || !cfg->prior_b)
            ARGFAIL("bssm_pmmh_chain: NULL configuration array");
        if (!res->theta_chain) ARGFAIL("bssm_pmmh_chain: theta_chain buffer missing");
        // proposal covariance on the transformed scale: J Sigma J, J = diag(dz/dtheta at init_theta)   R/pmmh.R:378-389
        std::vector<double> scale(p), cov((size_t)p * p);
        L.assign((size_t)p * p, 0.0);
        for (int j = 0; j < p; j++) {
            const double th = cfg->init_theta[j];
            scale[j] = cfg->transform[j] == BSSM_TR_LOG ? 1 / th : cfg->transform[j] == BSSM_TR_LOGIT ? 1 / (th * (1 - th)) : 1.0;
        }
        for (int a = 0; a < p; a++) for (int b = 0; b < p; b++) cov[a * p + b] = scale[a] * cfg->proposal_cov[a * p + b] * scale[b];
        // MASS::mvrnorm(1, mu, Sigma) (R/pmmh.R:425-428):  mu + V diag(sqrt(pmax(ev, 0))) z  with eigen(Sigma, symmetric = TRUE),
        // "'Sigma' is not positive definite" only when an eigenvalue is below -1e-6 |ev[1]| -- a positive SEMI-definite pilot
        // covariance (a parameter that never moved in the pilot's second half) is accepted, the chain just does not move in
        // the null directions.  Eigen-solver: cyclic Jacobi (p <= 16), eigenvalues decreasing, each eigenvector's largest
        // component positive (LAPACK's sign choice is build-dependent; same law either way).
        if (int rc = eigen_factor(p, cov.data(), L.data())) return rc;
        ckey = make_key(cfg->seed, 0x50000000ull + (unsigned long long)cfg->chain_index);
        cur.assign(cfg->init_theta, cfg->init_theta + p); prop.assign(p, 0.0); lp_prop.assign(p, 0.0);
        dim = (cfg->pf.model == BSSM_MODEL_SIR) ? 2 : 1;
        n_full = std::max(cfg->pf.n_theta, p);               // sampled parameters first, then fixed model constants
        th_full.assign((size_t)n_full, 0.0);
        for (int j = p; j < n_full; j++) th_full[j] = cfg->pf.theta ? cfg->pf.theta[j] : 0.0;
        se_cur.assign(((size_t)T + 1) * dim, 0.0); se_prop.assign(((size_t)T + 1) * dim, 0.0);
        cur_ll = 0; accepted = 0;
        return BSSM_OK;
    }
    // the filter's theta / stream for iteration `iter` with parameters `th`
    const double* full_theta(const std::vector<double>& th) { for (int j = 0; j < p; j++) th_full[j] = th[j]; return th_full.data(); }
    unsigned long long stream_of(unsigned iter) const { return ((unsigned long long)cfg->chain_index << 32) | iter; }
    void store(int i)
    {
        for (int j = 0; j < p; j++) res->theta_chain[(size_t)i * p + j] = cur[j];
        if (res->loglike_chain) res->loglike_chain[i] = cur_ll;
        if (res->state_est_chain) memcpy(res->state_est_chain + (size_t)i * (T + 1) * dim, se_cur.data(), sizeof(double) * (T + 1) * dim);
    }
    void start(double ll0) { cur_ll = ll0; store(0); }                                       // R/pmmh.R:403-417 (se_cur filled by the caller)
    // draw the proposal of iteration i (:424-432); false = a prior is -Inf, the chain stays put and no filter runs (:435-442)
    bool propose(int i)
    {
        std::vector<double> z(p), ztr(p);
        for (int j = 0; j < p; j++) {
            ztr[j] = tr_fwd(cfg->transform[j], cur[j]);
            z[j] = cfg->z_prop ? cfg->z_prop[(size_t)i * p + j] : host_normal(ckey, (uint32_t)i, (uint32_t)j);       // rnorm(p) of mvrnorm
        }
        for (int a = 0; a < p; a++) { double s = 0.0; for (int k = 0; k < p; k++) s += L[a * p + k] * z[k]; prop[a] = tr_back(cfg->transform[a], ztr[a] + s); }
        bool finite = true;
        for (int j = 0; j < p; j++) { lp_prop[j] = log_prior(cfg->prior_kind[j], cfg->prior_a[j], cfg->prior_b[j], prop[j]); if (!isfinite(lp_prop[j])) finite = false; }
        if (!finite) store(i);
        return finite;
    }
    // accept / reject with the proposal's log-likelihood (se_prop filled by the caller)   :461-496
    void finish(int i, double prop_ll)
    {
        long double lj_prop = 0, lj_cur = 0, slp_prop = 0, slp_cur = 0;                  // R's sum() accumulates in long double
        for (int j = 0; j < p; j++) {
            lj_prop += tr_logjac(cfg->transform[j], prop[j]); lj_cur += tr_logjac(cfg->transform[j], cur[j]);   // :461-469
            slp_prop += lp_prop[j]; slp_cur += log_prior(cfg->prior_kind[j], cfg->prior_a[j], cfg->prior_b[j], cur[j]);
        }
        const double num = prop_ll + (double)slp_prop + (double)lj_prop;                 // :475-478
        const double den = cur_ll + (double)slp_cur + (double)lj_cur;                    // :480-483
        double lar = num - den;                                                          // :485
        if (isnan(lar)) lar = -INFINITY;                                                 // :488-490
        const double u = cfg->u_accept ? cfg->u_accept[i] : host_uniform(ckey, (uint32_t)i);
        if (log(u) < lar) { cur = prop; cur_ll = prop_ll; se_cur = se_prop; accepted++; }   // :492-496
        store(i);
    }
};

extern "C" int bssm_pmmh_chain_draws(unsigned long long seed, int chain_index, int m, int n_params, double* z_prop_out, double* u_accept_out)
{
    if (m < 1 || n_params < 1 || !z_prop_out || !u_accept_out) ARGFAIL("bssm_pmmh_chain_draws: bad argument");
    const PhiloxKey ckey = make_key(seed, 0x50000000ull + (unsigned long long)chain_index);
    for (int i = 0; i < m; i++) {
        for (int j = 0; j < n_params; j++) z_prop_out[(size_t)i * n_params + j] = host_normal(ckey, (uint32_t)i, (uint32_t)j);
        u_accept_out[i] = host_uniform(ckey, (uint32_t)i);
    }
    return BSSM_OK;
}

extern "C" int bssm_pmmh_chain(bssm_ctx* c, const bssm_pmmh_config* cfg, bssm_pmmh_result* res)
{
    if (!c) ARGFAIL("bssm_pmmh_chain: NULL argument");
    ChainState ch;
    int rc = ch.init(cfg, res);
    if (rc) return rc;
    const int T = ch.T, m = ch.m;
    std::vector<double> ess((size_t)T + 1), llh((size_t)std::max(T, 1));
    double ll = 0, ms = 0, ms_total = 0;
    int ers = 0, nres = 0;
    bssm_pf_config pf = cfg->pf;
    pf.n_theta = ch.n_full; pf.return_particles = 0; pf.return_ancestors = 0; pf.z_init = pf.z_trans = pf.u_res = nullptr;
    pf.seed = cfg->seed;
    bssm_pf_result pr; memset(&pr, 0, sizeof(pr));
    pr.scan_stats = nullptr; pr.ess = ess.data(); pr.loglike_history = llh.data(); pr.loglike = &ll; pr.early_return_step = &ers; pr.n_res_calls = &nres; pr.device_ms = &ms;
    auto run_pf = [&](const std::vector<double>& th, std::vector<double>& se, unsigned iter) -> int {
        pf.theta = ch.full_theta(th); pr.state_est = se.data();
        pf.stream = ch.stream_of(iter);
        const int rc2 = bssm_pf_run(c, &pf, &pr);
        ms_total += ms;
        return rc2;
    };
    rc = run_pf(ch.cur, ch.se_cur, 0);                                                   // R/pmmh.R:403-417
    if (rc) return rc;
    ch.start(ll);
    for (int i = 1; i < m; i++) {                                                        // for (i in 2:m)  R/pmmh.R:422
        if (!ch.propose(i)) continue;
        rc = run_pf(ch.prop, ch.se_prop, (unsigned)i);                                   // :445-457
        if (rc) return rc;
        ch.finish(i, ll);
    }
    if (res->accepted) *res->accepted = ch.accepted;
    if (res->device_ms) *res->device_ms = ms_total;
    return BSSM_OK;
}

// Chains in lock-step: iteration i of every chain proposes on the host, ONE call of run_filters(pf, F, who, thetas, seeds, streams, br)
// runs the filters of the F chains who[0 .. F) whose proposal has a finite prior, every chain accepts or rejects (R/pmmh.R:422-500).
// entry: the entry point, for the message.  Chain draws are keyed by (seed, chain_index), so with filters that are bit-identical to
// bssm_pf_run chain k's result is exactly bssm_pmmh_chain's for cfgs[k].
template <class RunFilters>
static int pmmh_chains_lockstep(const char* entry, int n_chains, const bssm_pmmh_config* cfgs, bssm_pmmh_result* ress, RunFilters run_filters)
{
    std::vector<ChainState> ch((size_t)n_chains);
    for (int k = 0; k < n_chains; k++) { const int rc = ch[k].init(&cfgs[k], &ress[k]); if (rc) return rc; }
    const bssm_pf_config& pf0 = cfgs[0].pf;
    const int T = ch[0].T, m = ch[0].m, nth = ch[0].n_full;
    for (int k = 1; k < n_chains; k++) {
        const bssm_pf_config& q = cfgs[k].pf;
        if (ch[k].m != m || ch[k].T != T || ch[k].n_full != nth || q.model != pf0.model || q.algorithm != pf0.algorithm ||
            q.num_particles != pf0.num_particles || q.resample_algorithm != pf0.resample_algorithm || q.resample_fn != pf0.resample_fn ||
            !(q.threshold == pf0.threshold || (isnan(q.threshold) && isnan(pf0.threshold))) || q.y != pf0.y || q.obs_times != pf0.obs_times)
            ARGFAIL(std::string(entry) + ": the chains must share the data, the filter settings and m");
    }
    bssm_pf_config pf = pf0;
    pf.n_theta = nth; pf.theta = nullptr; pf.return_particles = 0; pf.return_ancestors = 0; pf.z_init = pf.z_trans = pf.u_res = nullptr;
    const int dim = ch[0].dim;
    std::vector<double> thetas((size_t)n_chains * nth), ll((size_t)n_chains), se((size_t)n_chains * (T + 1) * dim);
    std::vector<unsigned long long> seeds((size_t)n_chains), streams((size_t)n_chains);
    std::vector<int> who((size_t)n_chains);
    double ms = 0, ms_total = 0;
    bssm_pf_batch_result br; memset(&br, 0, sizeof(br));
    br.loglike = ll.data(); br.state_est = se.data(); br.device_ms = &ms;
    for (int i = 0; i < m; i++) {
        int F = 0;
        for (int k = 0; k < n_chains; k++) {
            const bool run = (i == 0) ? true : ch[k].propose(i);
            if (!run) continue;
            const double* th = ch[k].full_theta(i == 0 ? ch[k].cur : ch[k].prop);
            for (int j = 0; j < nth; j++) thetas[(size_t)F * nth + j] = th[j];
            seeds[F] = cfgs[k].seed; streams[F] = ch[k].stream_of((unsigned)i); who[F] = k; F++;
        }
        if (F == 0) continue;
        const int rc = run_filters(&pf, F, who.data(), thetas.data(), seeds.data(), streams.data(), &br);
        if (rc) return rc;
        ms_total += ms;
        for (int f = 0; f < F; f++) {
            ChainState& s = ch[who[f]];
            std::vector<double>& dst = (i == 0) ? s.se_cur : s.se_prop;
            memcpy(dst.data(), se.data() + (size_t)f * (T + 1) * dim, sizeof(double) * (T + 1) * dim);
            if (i == 0) s.start(ll[f]); else s.finish(i, ll[f]);
        }
    }
    for (int k = 0; k < n_chains; k++) {
        if (ress[k].accepted) *ress[k].accepted = ch[k].accepted;
        if (ress[k].device_ms) *ress[k].device_ms = ms_total / n_chains;
    }
    return BSSM_OK;
}

// Many small filters: ONE batched launch (bssm_pf_run_batch, one workgroup per filter) runs all the proposals' filters of an iteration.
extern "C" int bssm_pmmh_chains_batch(bssm_ctx* c, int n_chains, const bssm_pmmh_config* cfgs, bssm_pmmh_result* ress)
{
    if (!c || !cfgs || !ress) ARGFAIL("bssm_pmmh_chains_batch: NULL argument");
    if (n_chains < 1) ARGFAIL("bssm_pmmh_chains_batch: n_chains must be positive");
    return pmmh_chains_lockstep("bssm_pmmh_chains_batch", n_chains, cfgs, ress,
        [c](const bssm_pf_config* pf, int F, const int*, const double* thetas, const unsigned long long* seeds, const unsigned long long* streams,
            bssm_pf_batch_result* br) { return bssm_pf_run_batch(c, pf, F, thetas, seeds, streams, br); });
}

// The same loop for LARGE filters: ONE run of bssm_pf_run_multi (the kernels of bssm_pf_run, one argument set per chain) filters all the
// proposals of an iteration.  ctxs: one context per chain (at most 4); the chains that run an iteration bring theirs.
extern "C" int bssm_pmmh_chains_multi(bssm_ctx* const* ctxs, int n_chains, const bssm_pmmh_config* cfgs, bssm_pmmh_result* ress)
{
    if (!ctxs || !cfgs || !ress) ARGFAIL("bssm_pmmh_chains_multi: NULL argument");
    if (n_chains < 1 || n_chains > MULTI_MAX) ARGFAIL("bssm_pmmh_chains_multi: 1 .. 4 chains per call");
    return pmmh_chains_lockstep("bssm_pmmh_chains_multi", n_chains, cfgs, ress,
        [ctxs](const bssm_pf_config* pf, int F, const int* who, const double* thetas, const unsigned long long* seeds, const unsigned long long* streams,
               bssm_pf_batch_result* br) {
            bssm_ctx* cx[MULTI_MAX];
            for (int f = 0; f < F; f++) cx[f] = ctxs[who[f]];
            return bssm_pf_run_multi(cx, F, pf, thetas, seeds, streams, br);
        });
}

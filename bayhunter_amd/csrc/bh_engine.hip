// bayhunter_amd/csrc/bh_engine.hip -- the engine itself, of the host side of the C ABI declared in include/bh_engine.h: the experiment
// switches (bh_tuning.h), the handle's life, its settings, its timing and debug read-outs, and the helpers the other engine units
// (bh_engine_impl.h) stand on -- the last error, the buffers the engine owns and grows, the staging of a BH_HOST call's models and
// the events of a timed call.  There is no CPU code path in here: if no HIP device is usable, bh_engine_create fails.
#include "bh_engine_impl.h"

#include <mutex>

using namespace bheng;

// ---- the experiment switches (bh_tuning.h) ----
namespace {
BhTuning g_tuning;
std::once_flag g_tuning_once;
int tuning_value(const char *env, const char *txt, int dflt)
{
    if (!txt) return dflt;
    if (!std::strcmp(env, "BH_SWD_SEARCH")) return (txt[0] == 'f' || txt[0] == '1') ? ((std::strstr(txt, "ray") || txt[0] == '2') ? BH_SEARCH_FAST_RAYLEIGH : BH_SEARCH_FAST) : (txt[0] == '2' ? BH_SEARCH_FAST_RAYLEIGH : BH_SEARCH_REFERENCE);
    if (!std::strcmp(env, "BH_SWD_ARITH")) return (txt[0] == 'e' || txt[0] == '0') ? BH_ARITH_EXACT : BH_ARITH_FAST;
    if (!std::strcmp(env, "BH_SWD_SCAN")) return (txt[0] == 's' || txt[0] == '0') ? BH_SCAN_STEPS : ((txt[0] == 'c' || txt[0] == '1') ? BH_SCAN_COUNTED : BH_SCAN_AUTO);
    char *end = nullptr;
    const long v = std::strtol(txt, &end, 10);
    if (end == txt) return 1; // a flag set to some text
    return (int)v;
}
// bounds: a switch can cost time, never memory safety (after the environment is parsed and after every bh_tuning_set)
void tuning_clamp()
{
    if (g_tuning.rf_lds_gated < 0 || g_tuning.rf_lds_gated > 160 * 1024) g_tuning.rf_lds_gated = 0;
    if (g_tuning.rf_lds_beside > 160 * 1024) g_tuning.rf_lds_beside = -1;
    if (g_tuning.swd_love_inlook < 0 || g_tuning.swd_love_inlook > 4) g_tuning.swd_love_inlook = 0;
    if (g_tuning.swd_gsplit < 0 || g_tuning.swd_gsplit > (1 << 24)) g_tuning.swd_gsplit = 0; // (the launch's entry index is an int)
}
void tuning_parse()
{
#ifndef BH_NO_EXPERIMENTS
#define X(field, env, dflt, doc) g_tuning.field = tuning_value(env, std::getenv(env), dflt);
    BH_TUNING_TABLE(X)
#undef X
    tuning_clamp();
#endif
    g_tuning.under_pmc = std::getenv("ROCPROF_COUNTER_COLLECTION") != nullptr ? 1 : 0;
}
} // namespace
const BhTuning &bh_tuning()
{
    std::call_once(g_tuning_once, tuning_parse);
    return g_tuning;
}
int bh_tuning_set(const char *name, int value)
{
#ifdef BH_NO_EXPERIMENTS
    (void)name; (void)value;
    return -1;
#else
    (void)bh_tuning();
    if (!name) return -1;
#define X(field, env, dflt, doc) if (!std::strcmp(name, #field)) { g_tuning.field = value; tuning_clamp(); return 0; }
    BH_TUNING_TABLE(X)
#undef X
    return -1;
#endif
}
int bh_tuning_get(const char *name, int *value)
{
    const BhTuning &t = bh_tuning();
    if (!name || !value) return -1;
#define X(field, env, dflt, doc) if (!std::strcmp(name, #field)) { *value = t.field; return 0; }
    BH_TUNING_TABLE(X)
#undef X
    return -1;
}

namespace bheng {

int fail(bh_engine *e, int code, const char *what, hipError_t he)
{
    if (e) {
        e->err = what;
        if (he != hipSuccess) {
            e->err += ": ";
            e->err += hipGetErrorString(he);
        }
    }
    return code;
}

int ensure(bh_engine *e, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return BH_OK;
    if (b.p) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->aux) HIPCHK(e, hipStreamSynchronize(e->aux));
        if (e->aux2) HIPCHK(e, hipStreamSynchronize(e->aux2));
        HIPCHK(e, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 4 + 256;
    hipError_t he = hipMalloc(&b.p, want);
    if (he != hipSuccess) return fail(e, BH_ENOMEM, "hipMalloc", he);
    b.cap = want;
    return BH_OK;
}

int check_models(bh_engine *e, const ModelBatch &m)
{
    if (!e) return BH_EINVAL;
    if (m.B < 0 || m.Lmax < 1 || m.Lmax > BH_MAX_LAYERS) return fail(e, BH_EINVAL, "bad B or Lmax (1..100)");
    if (m.sl <= 0 || m.sb <= 0) return fail(e, BH_EINVAL, "strides must be positive");
    return BH_OK;
}

// Copy the model arrays of a BH_HOST call into the engine's device buffers: m's host pointers become device pointers
// (rho, qp and qs may be null and stay so).
int stage_models(bh_engine *e, ModelBatch &m)
{
    const int B = m.B;
    const size_t bytes = span_elems(m) * sizeof(double);
    {   // mean layer count, rounded up: what the lanes-per-model choice should be sized for
        long sum = 0;
        for (int b = 0; b < B; ++b) sum += m.nlay[b];
        m.typ_layers = B > 0 ? (int)((sum + B - 1) / B) : 0;
    }
    int rc;
    if ((rc = ensure(e, e->nlay, (size_t)B * sizeof(int32_t)))) return rc;
    HIPCHK(e, hipMemcpyAsync(e->nlay.p, m.nlay, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    m.nlay = (const int32_t *)e->nlay.p;
    const double **arr[6] = {&m.h, &m.vp, &m.vs, &m.rho, &m.qp, &m.qs};
    DevBuf *buf[6] = {&e->h, &e->vp, &e->vs, &e->rho, &e->qp, &e->qs};
    for (int k = 0; k < 6; ++k) {
        if (!*arr[k]) continue;
        if ((rc = ensure(e, *buf[k], bytes))) return rc;
        HIPCHK(e, hipMemcpyAsync(buf[k]->p, *arr[k], bytes, hipMemcpyHostToDevice, e->stream));
        *arr[k] = (const double *)buf[k]->p;
    }
    return BH_OK;
}

} // namespace bheng

namespace {
bh_engine::EventSet *cur_set(bh_engine *e)
{
    return (e->timing && e->ncalls > 0) ? &e->evsets[e->ncalls - 1] : nullptr;
}
} // namespace

namespace bheng {

void ev_begin(bh_engine *e, int fam, hipStream_t st)
{
    bh_engine::EventSet *s = cur_set(e);
    if (!s) return;
    if (!s->used[fam]) { // first launch of this family in the call
        (void)hipEventRecord(s->ev[2 * fam], st);
        s->used[fam] = true;
    }
}
void ev_end(bh_engine *e, int fam, hipStream_t st)
{
    bh_engine::EventSet *s = cur_set(e);
    if (s) (void)hipEventRecord(s->ev[2 * fam + 1], st);
}
void call_begin(bh_engine *e, hipStream_t st)
{
    e->neval_pending = false;
    if (!e->timing) return;
    if (e->ncalls == e->evsets.size()) {
        bh_engine::EventSet s{};
        for (auto &ev : s.ev)
            if (hipEventCreate(&ev) != hipSuccess) return; // timing silently unavailable
        e->evsets.push_back(s);
    }
    bh_engine::EventSet &s = e->evsets[e->ncalls++];
    for (bool &u : s.used) u = false;
    (void)hipEventRecord(s.ev[6], st);
    s.used[3] = true;
}
void call_end(bh_engine *e, hipStream_t st)
{
    bh_engine::EventSet *s = cur_set(e);
    if (s) (void)hipEventRecord(s->ev[7], st);
}

} // namespace bheng

extern "C" {

int bh_abi_version(void) { return BH_ABI_VERSION; }

int bh_engine_create(int device, bh_engine **out)
{
    if (!out) return BH_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BH_EHIP;
    if (device < 0 || device >= ndev) return BH_EINVAL;
    bh_engine *e = new (std::nothrow) bh_engine;
    if (!e) return BH_ENOMEM;
    e->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&e->stream) != hipSuccess ||
        hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&e->aux2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fork2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_join2, hipEventDisableTiming) != hipSuccess) {
        delete e;
        return BH_EHIP;
    }
    const BhTuning &tun = bh_tuning(); // (the experiment switches: parsed once per process, bh_tuning.h)
    if (tun.no_overlap) e->overlap_rf = false;
    if (tun.rf_lds_beside >= 0) e->rf_lds_beside_swd = tun.rf_lds_beside;
    {
        hipDeviceProp_t prop;
        e->pairwork.ncu = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 0;
    }
    if (tun.swd_prio_low >= 0) e->swd_prio_low = tun.swd_prio_low != 0 ? 1 : 0;
    {   // the counter the dispersion kernel's workgroups bump at start; hipStreamWaitValue32 polls it from the RF stream
        int can = 0;
        (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device);
        if (tun.no_started) can = 0;
        // rocprofv3 --pmc (counter collection) runs the dispatches of ALL queues one at a time; the RF stream's wait
        // packet then never sees the dispersion kernel start (measured: bench.py --workload c3 hangs under --pmc, runs
        // under --kernel-trace).  The gate is a scheduling aid only: off in that mode.
        if (tun.under_pmc) can = 0;
        // plain device memory: the wait packet polls it just as well, and atomics on signal memory
        // (hipMallocSignalMemory) cost the dispersion kernel 1 ms per launch (976 workgroups, one atomic each)
        if (can && hipMalloc((void **)&e->started, 8) != hipSuccess) e->started = nullptr;
        if (e->started && hipMemset(e->started, 0, 8) != hipSuccess) {
            (void)hipFree(e->started);
            e->started = nullptr;
        }
        (void)hipGetLastError();
    }
    e->force_group = tun.swd_group;
    e->force_look = tun.swd_lookahead;
    if (tun.swd_search >= 0) e->swd_search = tun.swd_search;
    if (tun.swd_arith >= 0) e->swd_arith = tun.swd_arith != 0 ? BH_ARITH_FAST : BH_ARITH_EXACT;
    if (tun.swd_scan >= 0) e->swd_scan = tun.swd_scan;
    if (tun.no_mfma) e->no_mfma = true;
    *out = e;
    return BH_OK;
}

int bh_engine_set_typical_layers(bh_engine *e, int nlay)
{
    if (!e) return BH_EINVAL;
    if (nlay < 0 || nlay > BH_MAX_LAYERS) return fail(e, BH_EINVAL, "typical layer count must be 0 (unknown) or 1..100");
    e->hint_layers = nlay;
    return BH_OK;
}

int bh_engine_set_model_order(bh_engine *e, int sort_by_depth)
{
    if (!e) return BH_EINVAL;
    e->as_given = (sort_by_depth == 0);
    return BH_OK;
}

int bh_engine_set_swd_search(bh_engine *e, int search)
{
    if (!e) return BH_EINVAL;
    if (search != BH_SEARCH_REFERENCE && search != BH_SEARCH_FAST && search != BH_SEARCH_FAST_RAYLEIGH)
        return fail(e, BH_EINVAL, "search must be BH_SEARCH_REFERENCE (0), BH_SEARCH_FAST (1) or BH_SEARCH_FAST_RAYLEIGH (2)");
    e->swd_search = search;
    return BH_OK;
}

int bh_engine_get_swd_search(const bh_engine *e) { return e ? e->swd_search : 0; }

int bh_engine_set_swd_scan(bh_engine *e, int scan)
{
    if (!e) return BH_EINVAL;
    if (scan != BH_SCAN_STEPS && scan != BH_SCAN_COUNTED && scan != BH_SCAN_AUTO) return fail(e, BH_EINVAL, "scan must be BH_SCAN_STEPS, BH_SCAN_COUNTED or BH_SCAN_AUTO");
    e->swd_scan = scan;
    return BH_OK;
}
int bh_engine_get_swd_scan(const bh_engine *e) { return e ? e->swd_scan : 0; }

int bh_engine_set_tuning(bh_engine *e, const char *name, int value)
{
    if (!e) return BH_EINVAL;
    if (bh_tuning_set(name, value) != 0) return fail(e, BH_EINVAL, "unknown experiment switch (csrc/bh_tuning.h), or a build with BH_NO_EXPERIMENTS");
    return BH_OK;
}
int bh_engine_get_tuning(bh_engine *e, const char *name, int *value)
{
    if (!e) return BH_EINVAL;
    if (bh_tuning_get(name, value) != 0) return fail(e, BH_EINVAL, "unknown experiment switch (csrc/bh_tuning.h)");
    return BH_OK;
}

int bh_engine_set_swd_arith(bh_engine *e, int arith)
{
    if (!e) return BH_EINVAL;
    if (arith != BH_ARITH_EXACT && arith != BH_ARITH_FAST) return fail(e, BH_EINVAL, "arith must be BH_ARITH_EXACT (0) or BH_ARITH_FAST (1)");
    e->swd_arith = arith;
    return BH_OK;
}
int bh_engine_get_swd_arith(const bh_engine *e) { return e ? e->swd_arith : 0; }
int bh_engine_last_swd_kernel(const bh_engine *e) { return e ? e->last_swd_kernel : -1; }
int bh_engine_last_swd_perm(bh_engine *e, int target, int32_t *out, int n)
{
    if (!e || !out || target < 0 || target > 1 || n < 0) return BH_EINVAL;
    if (e->last_swd_perm[target] == nullptr) return 0;
    if (n < e->last_swd_perm_n) return BH_EINVAL;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, e->last_swd_perm[target], (size_t)e->last_swd_perm_n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return e->last_swd_perm_n;
}
int bh_engine_last_swd_order(const bh_engine *e, int *workgroups, int *fills)
{
    if (workgroups) *workgroups = e ? e->last_swd_order[1] : 0;
    if (fills) *fills = e ? e->last_swd_order[2] : 0;
    return e ? e->last_swd_order[0] : -1;
}
int bh_engine_last_swd_launches(const bh_engine *e, bh_swd_launch *out, int max, int *n)
{
    if (!e || !n || max < 0 || (max > 0 && !out)) return BH_EINVAL;
    const int m = e->n_swd_launches < max ? e->n_swd_launches : max;
    for (int i = 0; i < m; ++i) out[i] = e->swd_launches[i];
    *n = m;
    return BH_OK;
}
int bh_engine_set_swd_trials(bh_engine *e, int trials)
{
    if (!e) return BH_EINVAL;
    if (trials != 0 && trials != 4 && trials != 8 && trials != 16 && trials != 32 && trials != 64)
        return fail(e, BH_EINVAL, "trials must be 0 (by the call's shape), 4, 8, 16, 32 or 64");
    e->swd_trials = trials;
    return BH_OK;
}
int bh_engine_get_swd_trials(const bh_engine *e) { return e ? e->swd_trials : 0; }
int bh_engine_guard_stats(bh_engine *e, int32_t *counts, uint64_t *rerun_launches, uint64_t *total)
{
    if (!e) return BH_EINVAL;
    if (rerun_launches) *rerun_launches = e->rerun_launches;
    if (counts || total) {
        int32_t w[3 * BH_MAX_TARGETS] = {0};
        if (e->guard.p && !e->guard_fresh) {
            HIPCHK(e, hipDeviceSynchronize()); // (the last call may have run on a caller's stream)
            HIPCHK(e, hipMemcpy(w, e->guard.p, sizeof(w), hipMemcpyDeviceToHost));
        }
        if (counts)
            for (int t = 0; t < BH_MAX_TARGETS; ++t) counts[t] = e->guard_last ? w[t] + w[BH_MAX_TARGETS + t] : 0;
        if (total)
            for (int t = 0; t < BH_MAX_TARGETS; ++t) total[t] = e->guard_total[t] + (uint64_t)(uint32_t)w[2 * BH_MAX_TARGETS + t];
    }
    return BH_OK;
}

int bh_engine_set_swd_lookahead(bh_engine *e, int trials_per_round)
{
    if (!e) return BH_EINVAL;
    if (trials_per_round < 0 || trials_per_round > 16)
        return fail(e, BH_EINVAL, "look-ahead must be 0 (auto) or 1..16 trial velocities per round");
    e->force_look = trials_per_round;
    return BH_OK;
}

int bh_engine_set_swd_group(bh_engine *e, int lanes_per_model)
{
    if (!e) return BH_EINVAL;
    if (lanes_per_model < 0 || lanes_per_model > 32)
        return fail(e, BH_EINVAL, "lanes per model must be 0 (auto) or 1..32");
    e->force_group = lanes_per_model;
    return BH_OK;
}

void bh_engine_destroy(bh_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (DevBuf *b : {&e->nlay, &e->h, &e->vp, &e->vs, &e->rho, &e->qp, &e->qs, &e->periods, &e->vel,
                      &e->errb, &e->rf, &e->coef, &e->ymod, &e->noise, &e->logL, &e->misfits,
                      &e->err_t, &e->probe_in, &e->probe_out, &e->counter, &e->sph, &e->perm, &e->board, &e->nevhi, &e->guard, &e->rfz, &e->gfirst, &e->nevhi2})
        release(*b);
    for (auto &t : e->targets) release_target(t);
    e->sites.drop(PART_COUNTS);
    release(e->sites.class_work);
    for (auto &s : e->evsets)
        for (auto &ev : s.ev)
            if (ev) (void)hipEventDestroy(ev);
    if (e->started) (void)hipFree(e->started);
    for (int t = 0; t < 2; ++t) {
        if (e->pairwork.perm[t]) (void)hipFree(e->pairwork.perm[t]);
        if (e->pairwork.slot_rank[t]) (void)hipFree(e->pairwork.slot_rank[t]);
    }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->aux) (void)hipStreamDestroy(e->aux);
    if (e->ev_fork2) (void)hipEventDestroy(e->ev_fork2);
    if (e->ev_join2) (void)hipEventDestroy(e->ev_join2);
    if (e->aux2) (void)hipStreamDestroy(e->aux2);
    (void)hipStreamDestroy(e->stream);
    delete e;
}

const char *bh_engine_last_error(const bh_engine *e) { return e ? e->err.c_str() : "null engine"; }

} // extern "C"

int bh_engine_fail_internal(bh_engine *e, int code, const char *what) { return fail(e, code, what); }
int bh_engine_device_internal(const bh_engine *e) { return e->device; }

extern "C" {
void *bh_engine_stream(bh_engine *e) { return e ? (void *)e->stream : nullptr; }

int bh_engine_synchronize(bh_engine *e)
{
    if (!e) return BH_EINVAL;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BH_OK;
}

int bh_engine_set_instrumentation(bh_engine *e, int timing, int counting)
{
    if (!e) return BH_EINVAL;
    e->timing = timing != 0;
    e->counting = counting != 0;
    return BH_OK;
}

int bh_timing_reset(bh_engine *e)
{
    if (!e) return BH_EINVAL;
    e->ncalls = 0;
    return BH_OK;
}

int bh_timing_collect(bh_engine *e, int *ncalls, double *total_ms, double family_ms[3])
{
    if (!e) return BH_EINVAL;
    double tot = 0.0, fam[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < e->ncalls; ++i) {
        bh_engine::EventSet &s = e->evsets[i];
        HIPCHK(e, hipEventSynchronize(s.ev[7]));
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, s.ev[6], s.ev[7]));
        tot += ms;
        for (int f = 0; f < 3; ++f) {
            if (!s.used[f]) continue;
            float fm = 0.f;
            HIPCHK(e, hipEventElapsedTime(&fm, s.ev[2 * f], s.ev[2 * f + 1]));
            fam[f] += fm;
        }
    }
    if (ncalls) *ncalls = (int)e->ncalls;
    if (total_ms) *total_ms = tot;
    if (family_ms)
        for (int f = 0; f < 3; ++f) family_ms[f] = fam[f];
    return BH_OK;
}

int bh_timing_steps(bh_engine *e, int max, double *step_ms, int *n)
{
    if (!e || !step_ms || !n || max < 0) return BH_EINVAL;
    int k = 0;
    for (size_t i = 0; i < e->ncalls && k < max; ++i, ++k) {
        bh_engine::EventSet &s = e->evsets[i];
        HIPCHK(e, hipEventSynchronize(s.ev[7]));
        float ms = 0.f;
        if (i + 1 < e->ncalls) HIPCHK(e, hipEventElapsedTime(&ms, s.ev[6], e->evsets[i + 1].ev[6]));
        else HIPCHK(e, hipEventElapsedTime(&ms, s.ev[6], s.ev[7]));
        step_ms[k] = ms;
    }
    *n = k;
    return BH_OK;
}

int bh_debug_counters(bh_engine *e, uint64_t out[16])
{
    if (!e || !out) return BH_EINVAL;
    if (!e->counter.p) return fail(e, BH_EINVAL, "counting was never enabled");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, e->counter.p, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_debug_trace(bh_engine *e, uint64_t *out, int nwaves)
{
    if (!e || !out || nwaves < 0 || nwaves > BH_TRACE_WAVES) return BH_EINVAL;
    if (!e->counter.p) return fail(e, BH_EINVAL, "counting was never enabled");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, (uint64_t *)e->counter.p + BH_COUNTER_WORDS, (size_t)4 * nwaves * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return BH_OK;
}

int bh_debug_guard_list(bh_engine *e, int target, int B, int32_t *out, int max, int *n)
{
    if (!e || !n || target < 0 || target >= BH_MAX_TARGETS || B < 0 || max < 0 || (max > 0 && !out)) return BH_EINVAL;
    *n = 0;
    if (!e->guard.p || e->guard_fresh || !e->guard_last) return BH_OK;
    if (((size_t)GUARD_HEAD + (size_t)(target + 1) * (size_t)(B + 4)) * sizeof(int32_t) > e->guard.cap) return fail(e, BH_EINVAL, "not the last call's batch size");
    int32_t cnt = 0;
    HIPCHK(e, hipDeviceSynchronize()); // (the last call may have run on a caller's stream)
    HIPCHK(e, hipMemcpy(&cnt, (int32_t *)e->guard.p + target, sizeof(cnt), hipMemcpyDeviceToHost));
    if (cnt < 0 || cnt > B) return fail(e, BH_EINVAL, "not the last call's batch size");
    const int m = cnt < max ? cnt : max;
    if (m > 0) HIPCHK(e, hipMemcpy(out, (int32_t *)e->guard.p + GUARD_HEAD + (size_t)target * (size_t)(B + 4), (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n = m;
    return BH_OK;
}

int bh_last_neval(bh_engine *e, uint64_t *neval)
{
    if (!e || !neval) return BH_EINVAL;
    if (e->neval_pending) {
        unsigned long long v = 0;
        HIPCHK(e, hipMemcpy(&v, e->counter.p, sizeof(v), hipMemcpyDeviceToHost));
        e->last_neval = v;
        e->neval_pending = false;
    }
    *neval = e->last_neval;
    return BH_OK;
}

} // extern "C"

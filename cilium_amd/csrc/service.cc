// The resident services' host side (product code; kernels/service.h, mailbox
// kernels/service_types.h): a synchronous drop-in call (one Allowed(), one
// OnData) posted to a polling workgroup instead of launched.
#include <cstring>

#include "engine_state.h"

// Stops a service's workgroup and waits for it to leave (v.mu held): its
// launch arguments (tables, connections) are about to change, or the engine
// goes away.
static hipError_t ServiceStop(Service &v) {
    if (!v.launched) return hipSuccess;
    __atomic_store_n(&v.box->stop, 1u, __ATOMIC_SEQ_CST);
    v.launched = false;
    return hipStreamSynchronize(v.s);  // (it leaves at its next poll; a fault is reported here)
}
void StopServices(l7g_engine *e) {
    for (Service &v : e->svc) {
        std::lock_guard<std::mutex> g(v.mu);  // (waits for a call in flight)
        ServiceStop(v);
    }
}
// A launch that wants every CU (a persistent grid) asks the services to leave
// without waiting; the next synchronous call starts them again.
void ReleaseServiceCUs(l7g_engine *e) {
    for (Service &v : e->svc) {
        SvcBox *b = __atomic_load_n(&v.box_ready, __ATOMIC_ACQUIRE);  // (set once; v.mu not taken here)
        if (b && __atomic_load_n(&b->state, __ATOMIC_ACQUIRE) != kSvcStopped) __atomic_store_n(&b->stop, 1u, __ATOMIC_SEQ_CST);
    }
}

// The service's box, staging and stream (v.mu held), on its first call.
static hipError_t ServiceAlloc(Service &v) {
    if (v.s) return hipSuccess;
    hipError_t rc;
    void *p = nullptr;
    if ((rc = hipHostMalloc(&p, sizeof(SvcBox), hipHostMallocCoherent)) != hipSuccess) return rc;
    v.box = (SvcBox *)p;
    memset(v.box, 0, sizeof(SvcBox));
    if ((rc = hipHostGetDevicePointer((void **)&v.box_dev, v.box, 0)) != hipSuccess ||
        (rc = hipHostMalloc((void **)&v.pin_in, kSvcInBytes, hipHostMallocDefault)) != hipSuccess ||
        (rc = hipHostMalloc((void **)&v.pin_out, kSvcOutBytes, hipHostMallocDefault)) != hipSuccess ||
        (rc = hipHostGetDevicePointer((void **)&v.pin_in_dev, v.pin_in, 0)) != hipSuccess ||
        (rc = hipHostGetDevicePointer((void **)&v.pin_out_dev, v.pin_out, 0)) != hipSuccess ||
        (rc = hipMalloc((void **)&v.dev_in, kSvcInBytes)) != hipSuccess)
        return rc;
    if ((rc = hipStreamCreateWithFlags(&v.s, hipStreamNonBlocking)) != hipSuccess) return rc;  // (v.s: allocated)
    __atomic_store_n(&v.box_ready, v.box, __ATOMIC_RELEASE);
    return hipSuccess;
}

// Posts a call to service v (e->mu and v.mu held; the inputs are in
// v.pin_in): the job's words, then req_seq, then the state read that decides
// whether a workgroup must be launched (a new service, one that has left, or
// one whose launch arguments are stale).
static hipError_t ServicePost(l7g_engine *e, Service &v, int kind, uint32_t n, uint64_t arena_len, uint32_t flags,
                              uint32_t *seq_out) {
    hipError_t rc = hipSuccess;
    const uint32_t nconns = (uint32_t)e->conns.size();
    const bool same = kind == 0 ? memcmp(&v.ht, &e->ht, sizeof v.ht) == 0 : memcmp(&v.mt, &e->mt, sizeof v.mt) == 0;
    if (v.launched && !(same && v.conns == e->d_conns && v.nconns == nconns) && (rc = ServiceStop(v)) != hipSuccess)
        return rc;
    SvcBox *b = v.box;
    __atomic_store_n(&b->n, n, __ATOMIC_RELAXED);  // (the line's other words: stored before req_seq)
    __atomic_store_n(&b->arena_len, (uint32_t)arena_len, __ATOMIC_RELAXED);
    __atomic_store_n(&b->flags, flags, __ATOMIC_RELAXED);
    __atomic_store_n(&b->stop, 0u, __ATOMIC_RELAXED);
    std::atomic_thread_fence(std::memory_order_release);
    const uint32_t seq = NextSeq(v.seq);
    __atomic_store_n(&b->req_seq, seq, __ATOMIC_SEQ_CST);  // (after the inputs and the job's words)
    // the workgroup's exit handshake writes EXITING, fences, reads req_seq:
    // either it sees this call, or this read sees it leaving
    uint32_t st = __atomic_load_n(&b->state, __ATOMIC_SEQ_CST);
    bool start = !v.launched;
    if (v.launched && st != kSvcRunning) {
        const auto t0 = std::chrono::steady_clock::now();
        while ((st = __atomic_load_n(&b->state, __ATOMIC_SEQ_CST)) == kSvcExiting &&
               std::chrono::steady_clock::now() - t0 < std::chrono::seconds(1))
            __builtin_ia32_pause();
        start = st != kSvcRunning;
        if (start && (rc = hipStreamSynchronize(v.s)) != hipSuccess) return rc;  // (the old workgroup has left)
    }
    if (start) {
        __atomic_store_n(&b->state, (uint32_t)kSvcRunning, __ATOMIC_SEQ_CST);
        const SvcStatic S{v.pin_in_dev, v.dev_in, v.pin_out_dev, e->d_conns, nconns, 0};
        rc = kind == 0 ? LaunchHttpService(v.box_dev, S, e->ht, seq - 1, kSvcIdleCycles, v.s)
                       : LaunchMemcacheService(v.box_dev, S, e->mt, seq - 1, kSvcIdleCycles, v.s);
        if (rc != hipSuccess) return rc;
        v.ht = e->ht;
        v.mt = e->mt;
        v.conns = e->d_conns;
        v.nconns = nconns;
        v.launched = true;
        v.launches++;
    }
    v.calls++;
    *seq_out = seq;
    return hipSuccess;
}

// A synchronous call a service can take: the HTTP (at most kSvcHttpMax) or the
// memcached (at most kSvcMcMax) requests of one small call whose inputs lie in
// one piece of pinned memory, with the selection Classify makes for such a
// call from the same ScanConns (only that protocol's kernel, unpartitioned,
// answering the requests no parser owns) and nothing else to run (no
// NFA-fallback matchers, no proxy statistics).  Returns false when the call
// takes the launched path; true when it was answered (or failed: *rc_out).
bool ServiceTry(l7g_engine *e, uint32_t n, uint64_t arena_len, const HostIn &in, uint8_t *verdict, int32_t *rule,
                uint32_t *consumed, hipError_t *rc_out) {
    if (!e->svc_on || n == 0 || n > kSvcMcMax || arena_len > kZeroCopyMaxBytes) return false;
    if (!(in.nseg == 0 || (in.nseg == 1 && in.seg[0].rows <= 1 && in.seg[0].width == arena_len))) return false;
    if (in.nseg == 0 && arena_len) return false;
    Service *v = nullptr;
    uint32_t seq = 0;
    {
        std::lock_guard<std::mutex> g(e->mu);
        if (e->device < 0 || hipSetDevice(e->device) != hipSuccess || Upload(e) != hipSuccess) return false;
        if (e->flow_stats && !e->skey_list.empty()) return false;
        const ConnScan scan = ScanConns(e, in.conn, n);
        int kind = -1;
        uint32_t flags = kSvcAnswerOther;
        if (scan.http_only && n <= kSvcHttpMax && !e->ht.nfa_pool) {
            kind = 0;
            const bool hot = e->ht.hot_ruleset >= 0;
            flags |= (hot ? kSvcHttpHot : 0u) | (!hot || scan.any_cold ? kSvcHttpGeneral : 0u);
        } else if (scan.mc_only && !e->mt.nfa_pool) {
            kind = 1;
        }
        if (kind < 0) return false;
        v = &e->svc[kind];
        if (!v->mu.try_lock()) return false;  // (another thread's call is in the service: launch this one)
        // the inputs, in the service's layout (packed: kernels/call_layout.h; n > 0)
        hipError_t rc = ServiceAlloc(*v);
        if (rc == hipSuccess) {
            memcpy(v->pin_in, in.off, (size_t)n * 8);
            memcpy(v->pin_in + CallLenOff(n), in.len, (size_t)n * 4);
            memcpy(v->pin_in + CallConnOff(n), in.conn, (size_t)n * 4);
            if (arena_len) memcpy(v->pin_in + CallArenaOff(n), in.seg[0].p, arena_len);
            rc = ServicePost(e, *v, kind, n, arena_len, flags, &seq);
        }
        if (rc != hipSuccess) {
            v->mu.unlock();
            *rc_out = rc;
            return true;
        }
    }
    // the answers: the done word, then pinned memory (no stream wait: a fault
    // shows as a done word that never comes, and the service's stream reports it)
    hipError_t rc = hipSuccess;
    const bool done = SpinUntil([&] { return __atomic_load_n(&v->box->done, __ATOMIC_ACQUIRE); }, seq,
                                std::chrono::milliseconds(1000));
    if (!done) {  // (v->mu held: the service's own fields only, no engine lock)
        rc = hipStreamQuery(v->s);
        if (rc == hipSuccess || rc == hipErrorNotReady) rc = hipErrorLaunchTimeOut;
        const hipError_t r2 = ServiceStop(*v);
        if (rc == hipErrorLaunchTimeOut && r2 != hipSuccess) rc = r2;
    } else {
        const uint8_t *po = v->pin_out;
        memcpy(verdict, po, n);
        memcpy(rule, po + CallRuleOff(n), (size_t)n * 4);
        memcpy(consumed, po + CallConsumedOff(n), (size_t)n * 4);
    }
    v->mu.unlock();
    *rc_out = rc;
    return true;
}

extern "C" {

int l7g_service_enable(l7g_engine *e, int on) {
    if (!e) return 0;
    std::lock_guard<std::mutex> g(e->mu);
    const int was = e->svc_on.exchange(on != 0) ? 1 : 0;
    if (!on && e->device >= 0) StopServices(e);
    return was;
}

void l7g_service_stats(l7g_engine *e, uint64_t out[4]) {
    if (!e) {
        memset(out, 0, 4 * sizeof *out);
        return;
    }
    for (int k = 0; k < 2; k++) {
        std::lock_guard<std::mutex> g(e->svc[k].mu);
        out[2 * k] = e->svc[k].calls;
        out[2 * k + 1] = e->svc[k].launches;
    }
}

}  // extern "C"

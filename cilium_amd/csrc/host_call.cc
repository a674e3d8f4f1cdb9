// l7g_classify_host's per-thread path (product code), in three steps: stage,
// fill, run (the batcher's flushers fill the staging in place and skip the
// copy).  The staging's layout is kernels/call_layout.h.  The host-buffer twins
// of the other calls follow: each starts with HostStage, sends the staging
// over with UploadStaged, calls its device-pointer entry on the views
// (CallViews, OutViews) and fills the caller's arrays (UnpackOut); what the
// call layout has no place for travels in a StagePair of the thread's HostCtx
// (engine_state.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine_state.h"
#include "wire.h"

// grow-only staging for the inputs and the outputs of a call
static hipError_t HostGrow(HostCtx *H, uint32_t n, uint64_t arena_len) {
    const size_t need_in = CallInCap(n, arena_len);
    const size_t need_out = CallOutCap(n);
    if (need_in <= H->in_cap && need_out <= H->out_cap) return hipSuccess;
    // (the previous call of this thread has its answers; its kernels may still be
    // retiring after storing the done word)
    if (H->s) hipStreamSynchronize(H->s);
    if (H->dev) hipFree(H->dev);
    if (H->pin_in) hipHostFree(H->pin_in);
    if (H->pin_out) hipHostFree(H->pin_out);
    H->dev = H->pin_in = H->pin_out = H->pin_in_dev = H->pin_out_dev = nullptr;
    H->in_cap = std::max(need_in + need_in / 4, (size_t)1 << 16);  // (some slack: batches vary)
    H->out_cap = std::max(need_out + need_out / 4, (size_t)1 << 14);
    hipError_t rc;
    if ((rc = hipMalloc(&H->dev, H->in_cap + H->out_cap)) != hipSuccess) { H->in_cap = H->out_cap = 0; return rc; }
    if ((rc = hipHostMalloc(&H->pin_in, H->in_cap, hipHostMallocDefault)) != hipSuccess ||
        (rc = hipHostMalloc(&H->pin_out, H->out_cap, hipHostMallocDefault)) != hipSuccess ||
        (rc = hipHostGetDevicePointer((void **)&H->pin_in_dev, H->pin_in, 0)) != hipSuccess ||
        (rc = hipHostGetDevicePointer((void **)&H->pin_out_dev, H->pin_out, 0)) != hipSuccess) {
        H->in_cap = H->out_cap = 0;
        return rc;
    }
    if (!H->pin_done) {
        if ((rc = hipHostMalloc((void **)&H->pin_done, 64, hipHostMallocDefault)) != hipSuccess) return rc;
        *(volatile uint32_t *)H->pin_done = 0;
        H->seq = 0;
        if ((rc = hipHostGetDevicePointer((void **)&H->pin_done_dev, H->pin_done, 0)) != hipSuccess) return rc;
    }
    return hipSuccess;
}

// The calling thread's stream and staging on the engine's device (the engine
// lock is held only while l7g_classify enqueues, so threads' copies and
// kernels overlap); grow: the staging sized for n requests over arena_len bytes.
static hipError_t HostEnter(l7g_engine *e, HostCtx **H, bool grow = false, uint32_t n = 0, uint64_t arena_len = 0) {
    if (e->device < 0) return hipErrorNoDevice;
    hipError_t rc = hipSetDevice(e->device);
    if (rc != hipSuccess) return rc;
    {
        std::lock_guard<std::mutex> g(e->hmu);
        auto &slot = e->hctx[std::this_thread::get_id()];
        if (!slot) {
            auto h = std::make_unique<HostCtx>();
            if ((rc = hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking)) != hipSuccess) return rc;
            slot = std::move(h);
        }
        *H = slot.get();
    }
    return grow ? HostGrow(*H, n, arena_len) : hipSuccess;
}

// What every host-buffer twin starts with: the thread's context entered (once),
// its staging grown, the caller's arrays and arena (`host`: host pointers)
// copied into the pinned staging.  *dev: the views of the device staging that
// UploadStaged fills from it.
static hipError_t HostStage(l7g_engine *e, const DevIn &host, HostCtx **Hout, DevIn *dev) {
    HostCtx *H = nullptr;
    const hipError_t rc = HostEnter(e, &H, true, host.n, host.arena_len);
    if (rc != hipSuccess) return rc;
    const size_t nn = CallNn(host.n), n = host.n;
    if (n) {
        memcpy(H->pin_in, host.off, n * 8);
        memcpy(H->pin_in + CallLenOff(nn), host.len, n * 4);
        memcpy(H->pin_in + CallConnOff(nn), host.conn, n * 4);
    }
    if (host.arena_len) memcpy(H->pin_in + CallArenaOff(nn), host.arena, host.arena_len);
    *Hout = H;
    *dev = CallViews(H->dev, nn, host.arena_len, host.n);
    return hipSuccess;
}
// the staged inputs to the device: one copy of the whole layout
static hipError_t UploadStaged(HostCtx *H, const DevIn &dev) {
    return hipMemcpyAsync(H->dev, H->pin_in, CallInBytes(CallNn(dev.n), dev.arena_len), hipMemcpyHostToDevice, H->s);
}

// A call's outputs (call_layout.h) at d_out, and the caller's arrays filled
// from the pinned ones (rule null: a call without rules).
static DevOut OutViews(uint8_t *d_out, uint32_t n) {
    return {d_out, (int32_t *)(d_out + CallRuleOff(n)), (uint32_t *)(d_out + CallConsumedOff(n)), nullptr};
}
static void UnpackOut(const HostCtx *H, uint32_t n, uint8_t *verdict, int32_t *rule, uint32_t *consumed) {
    memcpy(verdict, H->pin_out, n);
    if (rule) memcpy(rule, H->pin_out + CallRuleOff(n), (size_t)n * 4);
    memcpy(consumed, H->pin_out + CallConsumedOff(n), (size_t)n * 4);
}

// classify a call whose inputs are in pinned host memory, wait for it, copy
// the answers out
static hipError_t HostRun(l7g_engine *e, HostCtx *H, uint32_t n, uint64_t arena_len, const HostIn &in,
                          uint8_t *verdict, int32_t *rule, uint32_t *consumed, bool try_service = true) {
    hipError_t rc = hipSuccess;
    if (try_service && ServiceTry(e, n, arena_len, in, verdict, rule, consumed, &rc)) return rc;
    const size_t nn = CallNn(n);
    const size_t a_off = CallArenaOff(nn);
    // A small call (the Envoy adapter's Allowed(), one OnData, a light batch)
    // is latency, not bandwidth: the kernels read the inputs from and write the
    // verdicts to the pinned memory in place (zero-copy, over PCIe), so the
    // call is one launch and a wait instead of copy, launch, copy, wait.
    static const bool zc_on = [] {
        const char *v = getenv("L7G_SYNC_ZEROCOPY");
        return !(v && v[0] == '0');
    }();
    const bool zc = zc_on && (in.nseg == 0 || (in.nseg == 1 && in.seg[0].rows <= 1)) && n <= kZeroCopyMaxRequests &&
                    a_off + arena_len <= kZeroCopyMaxBytes;
    hipStream_t s = H->s;
    DevIn dv;  // the inputs where the kernels read them
    uint8_t *d_out = H->dev + H->in_cap;
    CopyIn pre{};  // zero-copy: the inputs' copy into HBM, done by the call's first kernel
    if (zc) {
        // The inputs are copied into HBM (one PCIe round trip per 64 KiB, every
        // load in flight before the first store: by the call's first kernel when
        // it is one workgroup, else by copy_in_kernel) and classified there: read
        // in place, every dependent read of a framer was a PCIe round trip.  The
        // verdicts are still written to the pinned memory in place.
        d_out = H->pin_out_dev;
        uint8_t *d_in = H->dev;
        CopyIn ci{};
        const size_t a_at = in.nseg ? (size_t)((const uint8_t *)in.seg[0].p - H->pin_in) : 0;
        if (in.off == (const uint64_t *)H->pin_in && in.len == (const uint32_t *)(H->pin_in + CallLenOff(nn)) &&
            in.conn == (const uint32_t *)(H->pin_in + CallConnOff(nn)) && a_at <= a_off && a_at % 16 == 0) {
            // the thread's staging (packed): one piece
            ci.p[0] = {H->pin_in_dev, d_in, (uint64_t)CallInBytes(nn, arena_len)};
            ci.n = 1;
            dv = CallViews(d_in, nn, arena_len, n);
            dv.arena = d_in + a_at;
        } else {
            // a batcher slot: four pieces into [off | len | conn | arena], the arrays
            // nn4 entries long so each starts 16-byte aligned (call_layout.h)
            void *dp = nullptr;
            auto dev_ptr = [&](const void *h) -> const uint8_t * {
                if (rc == hipSuccess) rc = hipHostGetDevicePointer(&dp, const_cast<void *>(h), 0);
                return (const uint8_t *)dp;
            };
            const uint8_t *h_o = dev_ptr(in.off), *h_l = dev_ptr(in.len), *h_c = dev_ptr(in.conn);
            const uint8_t *h_a = in.nseg ? dev_ptr(in.seg[0].p) : h_o;
            if (rc != hipSuccess) return rc;
            auto al16 = [](const void *p) { return ((uintptr_t)p & 15) == 0; };
            if (!(al16(h_o) && al16(h_l) && al16(h_c) && al16(h_a))) return hipErrorInvalidValue;  // (slots are)
            const size_t nn4 = CallNn4(n);
            ci.p[0] = {h_o, d_in, (uint64_t)nn * 8};
            ci.p[1] = {h_l, d_in + CallLenOff(nn4), (uint64_t)nn * 4};
            ci.p[2] = {h_c, d_in + CallConnOff(nn4), (uint64_t)nn * 4};
            ci.p[3] = {h_a, d_in + a_off, in.nseg ? arena_len : 0};
            ci.n = 4;
            dv = CallViews(d_in, nn4, arena_len, n);
            dv.arena = in.nseg ? d_in + a_off : d_in;
        }
        pre = ci;
        pre.done = H->pin_done_dev;
        pre.seq = NextSeq(H->seq);
    } else {
        uint8_t *d_in = H->dev;
        const bool staging = in.off == (const uint64_t *)H->pin_in;
        const size_t st = staging ? nn : in.stride ? in.stride : nn;
        dv = CallViews(d_in, st, arena_len, n);
        uint8_t *d_a = d_in + CallArenaOff(st);
        if (staging) {  // the thread's staging: one copy of the whole layout
            rc = hipMemcpyAsync(d_in, H->pin_in, CallInBytes(nn, arena_len), hipMemcpyHostToDevice, s);
        } else {
            if (in.stride) {  // the three arrays in one copy
                rc = hipMemcpyAsync(d_in, in.off, CallConnOff(st) + (size_t)n * 4, hipMemcpyHostToDevice, s);
            } else {
                rc = hipMemcpyAsync((void *)dv.off, in.off, (size_t)n * 8, hipMemcpyHostToDevice, s);
                if (rc == hipSuccess) rc = hipMemcpyAsync((void *)dv.len, in.len, (size_t)n * 4, hipMemcpyHostToDevice, s);
                if (rc == hipSuccess) rc = hipMemcpyAsync((void *)dv.conn, in.conn, (size_t)n * 4, hipMemcpyHostToDevice, s);
            }
            uint64_t at = 0;
            for (int k = 0; k < in.nseg && rc == hipSuccess; k++) {
                const l7g_host_seg &g = in.seg[k];
                if (!g.width || !g.rows) continue;
                if (g.rows == 1)
                    rc = hipMemcpyAsync(d_a + at, g.p, g.width, hipMemcpyHostToDevice, s);
                else
                    rc = hipMemcpy2DAsync(d_a + at, g.width, g.p, g.pitch, g.width, g.rows, hipMemcpyHostToDevice, s);
                at += g.width * g.rows;
            }
        }
    }
    bool signaled = false;
    ClassifyOpts o;
    o.host_conn = in.conn;
    o.pre = pre.n ? &pre : nullptr;
    o.signaled = &signaled;
    if (rc == hipSuccess) rc = (hipError_t)Classify(e, dv, OutViews(d_out, n), s, o);
    if (rc == hipSuccess && n && !zc)
        rc = hipMemcpyAsync(H->pin_out, d_out, CallOutBytes(n), hipMemcpyDeviceToHost, s);
    // One workgroup answered the call: its done word says the answers are in
    // pinned memory (a spin on that word is some microseconds shorter than the
    // stream's completion signal); past 2 ms, or otherwise, wait on the stream,
    // which also reports a kernel's failure.
    bool done = false;
    if (rc == hipSuccess && signaled) {
        done = SpinUntil([&] { return *(volatile uint32_t *)H->pin_done; }, pre.seq, std::chrono::milliseconds(2));
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (rc == hipSuccess && !done) rc = hipStreamSynchronize(s);
    if (rc == hipSuccess && n) UnpackOut(H, n, verdict, rule, consumed);
    return rc;
}

int l7g_host_stage(l7g_engine *e, uint32_t n, uint64_t arena_len, uint8_t **arena, uint64_t **off, uint32_t **len,
                   uint32_t **conn) {
    HostCtx *H = nullptr;
    const hipError_t rc = HostEnter(e, &H, true, n, arena_len);
    if (rc != hipSuccess) return (int)rc;
    const DevIn p = CallViews(H->pin_in, CallNn(n), arena_len, n);
    *off = (uint64_t *)p.off;
    *len = (uint32_t *)p.len;
    *conn = (uint32_t *)p.conn;
    *arena = (uint8_t *)p.arena;
    return 0;
}

// HostRun over the thread's filled staging
static hipError_t HostRunStaged(l7g_engine *e, HostCtx *H, uint32_t n, uint64_t arena_len, uint8_t *verdict,
                                int32_t *rule, uint32_t *consumed, bool try_service) {
    const size_t nn = CallNn(n);
    const DevIn p = CallViews(H->pin_in, nn, arena_len, n);
    const l7g_host_seg seg{p.arena, arena_len, arena_len, 1};
    const HostIn in{p.off, p.len, p.conn, nn, &seg, 1};
    return HostRun(e, H, n, arena_len, in, verdict, rule, consumed, try_service);
}

int l7g_host_run(l7g_engine *e, uint32_t n, uint64_t arena_len, uint8_t *verdict, int32_t *rule, uint32_t *consumed) {
    HostCtx *H = nullptr;
    hipError_t rc = HostEnter(e, &H);
    if (rc == hipSuccess) rc = HostRunStaged(e, H, n, arena_len, verdict, rule, consumed, true);
    return (int)rc;
}
int l7g_host_run_pinned(l7g_engine *e, uint32_t n, const uint64_t *off, size_t stride, const l7g_host_seg *seg,
                        int nseg, uint8_t *verdict, int32_t *rule, uint32_t *consumed) {
    HostCtx *H = nullptr;
    uint64_t arena_len = 0;
    for (int k = 0; k < nseg; k++) arena_len += seg[k].width * seg[k].rows;
    const uint32_t st = (uint32_t)std::max<size_t>(stride, n);
    // device staging for `st` entries' arrays and the arena, pinned outputs for n
    hipError_t rc = HostEnter(e, &H, true, st, arena_len);
    if (rc == hipSuccess) {
        const DevIn p = CallViews((const uint8_t *)off, stride, arena_len, n);
        const HostIn in{off, p.len, p.conn, stride, seg, nseg};
        rc = HostRun(e, H, n, arena_len, in, verdict, rule, consumed);
    }
    return (int)rc;
}

int l7g_host_reserve(l7g_engine *e, uint32_t n, uint64_t arena_len) {
    HostCtx *H = nullptr;
    return (int)HostEnter(e, &H, true, n, arena_len);
}

int l7g_engine_has_device(const l7g_engine *e) { return e && e->device >= 0 ? 1 : 0; }

void *l7g_pinned_alloc(size_t bytes) {
    void *p = nullptr;
    return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void l7g_pinned_free(void *p) {
    if (p) hipHostFree(p);
}

extern "C" {

int l7g_classify_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                      const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule, uint32_t *consumed) {
    {  // a call a service takes goes from the caller's buffers straight into the service's staging
        const l7g_host_seg seg{arena, arena_len, arena_len, 1};
        const HostIn in{off, len, conn, 0, &seg, 1};
        hipError_t rc = hipSuccess;
        if (e->device >= 0 && ServiceTry(e, n, arena_len, in, verdict, rule, consumed, &rc)) return (int)rc;
    }
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, off, len, conn, n}, &H, &dev);
    if (rc == hipSuccess) rc = HostRunStaged(e, H, n, arena_len, verdict, rule, consumed, false);
    return (int)rc;
}

// l7g_classify_host with the access-log outputs (the body of both logged
// twins; all: l7g_classify_logged_all's plan, the text rows with it): the
// calling thread's stream and staging, one copy in, the launch plan of
// Classify with the log outputs (always launched: no resident service, no
// zero-copy), the outputs and the log staging, laid out [records | span rows |
// text rows], copied out, a wait.  The caller's span and text rows go in
// first, so that what no kernel writes (rows of other protocols, bytes past a
// row's written prefix) comes back as it was.
static int ClassifyLoggedHost(l7g_engine *e, const DevIn &host, uint8_t *verdict, int32_t *rule, uint32_t *consumed,
                              const l7g_log_all_out_t &log, bool all) {
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, host, &H, &dev);
    const uint32_t n = host.n;
    if (rc != hipSuccess || n == 0) return (int)rc;
    const size_t rec_b = (size_t)n * sizeof(l7g_logrec_t);
    const size_t span_b = (size_t)n * log.span_stride * sizeof(l7g_span_t);
    const size_t text_b = (size_t)n * log.text_stride;
    const size_t all_b = rec_b + span_b + text_b;
    if ((rc = H->log.Grow(H->s, all_b)) != hipSuccess) return (int)rc;
    uint8_t *d_log = H->log.dev, *p_log = H->log.pin, *d_out = H->dev + H->in_cap;
    const LogOut lo{(LogRec *)d_log, span_b ? (LogSpan *)(d_log + rec_b) : nullptr, log.span_stride};
    const LogText tx{text_b ? d_log + rec_b + span_b : nullptr, log.text_stride};
    ClassifyOpts o;
    o.host_conn = (const uint32_t *)(H->pin_in + CallConnOff(CallNn(n)));
    o.log = &lo;
    o.text = all ? &tx : nullptr;  // (Classify's plan differs on it)
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess && span_b + text_b) {
        if (span_b) memcpy(p_log + rec_b, log.spans, span_b);
        if (text_b) memcpy(p_log + rec_b + span_b, log.text, text_b);
        rc = hipMemcpyAsync(d_log + rec_b, p_log + rec_b, span_b + text_b, hipMemcpyHostToDevice, H->s);
    }
    if (rc == hipSuccess) rc = (hipError_t)Classify(e, dev, OutViews(d_out, n), H->s, o);
    if (rc == hipSuccess) rc = hipMemcpyAsync(H->pin_out, d_out, CallOutBytes(n), hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipMemcpyAsync(p_log, d_log, all_b, hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc == hipSuccess) {
        UnpackOut(H, n, verdict, rule, consumed);
        memcpy(log.rec, p_log, rec_b);
        if (span_b) memcpy(log.spans, p_log + rec_b, span_b);
        if (text_b) memcpy(log.text, p_log + rec_b + span_b, text_b);
    }
    return (int)rc;
}

int l7g_classify_logged_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                             const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                             uint32_t *consumed, const l7g_log_out_t *log) {
    if (!log || !log->rec || (log->topic_stride && !log->topics)) return (int)hipErrorInvalidValue;
    return ClassifyLoggedHost(e, {arena, arena_len, off, len, conn, n}, verdict, rule, consumed,
                              {log->rec, log->topics, log->topic_stride, nullptr, 0}, false);
}

int l7g_classify_logged_all_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                                 const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict,
                                 int32_t *rule, uint32_t *consumed, const l7g_log_all_out_t *log) {
    if (!log || !log->rec || (log->span_stride && !log->spans) || (log->text_stride && !log->text))
        return (int)hipErrorInvalidValue;
    return ClassifyLoggedHost(e, {arena, arena_len, off, len, conn, n}, verdict, rule, consumed, *log, true);
}

// l7g_deny_replies with host buffers, over the calling thread's stream and
// staging: the inputs and the verdicts copied in, the reply kernels, the
// sizes copied out and waited for, then the bytes that were written.  The
// replies that fit under cap are a prefix of the batch (off[] is a prefix
// sum), so what the device wrote is one piece, buf[0, W) with W the last
// fitting reply's end: only that is copied to the caller's buffer.  The reply
// staging is [verdict | off | len | total | cap reply bytes], on the device and
// pinned, grow-only per calling thread.
int l7g_deny_replies_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                          const uint32_t *len, const uint32_t *conn, uint32_t n, const uint8_t *verdict,
                          const l7g_reply_out_t *out) {
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (!out || !out->off || !out->len || !out->total || (!out->buf && out->cap)) return (int)hipErrorInvalidValue;
    if (n && (!off || !len || !conn || !verdict)) return (int)hipErrorInvalidValue;
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, off, len, conn, n}, &H, &dev);
    if (rc != hipSuccess) return (int)rc;
    const size_t o_off = ((size_t)n + 15) & ~(size_t)15, o_len = o_off + (size_t)n * 8;
    const size_t o_tot = (o_len + (size_t)n * 4 + 15) & ~(size_t)15, o_buf = o_tot + 16;
    if ((rc = H->reply.Grow(H->s, o_buf + out->cap)) != hipSuccess) return (int)rc;
    uint8_t *d_r = H->reply.dev, *p_r = H->reply.pin;
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess && n) {
        memcpy(p_r, verdict, n);
        rc = hipMemcpyAsync(d_r, p_r, n, hipMemcpyHostToDevice, H->s);
    }
    const l7g_reply_out_t dout{out->cap ? d_r + o_buf : nullptr, out->cap, (uint64_t *)(d_r + o_off),
                               (uint32_t *)(d_r + o_len), (uint64_t *)(d_r + o_tot)};
    if (rc == hipSuccess) rc = (hipError_t)DenyReplies(e, dev, d_r, &dout, H->s);
    if (rc == hipSuccess)
        rc = hipMemcpyAsync(p_r + o_off, d_r + o_off, o_buf - o_off, hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc != hipSuccess) return (int)rc;
    const uint64_t *h_off = (const uint64_t *)(p_r + o_off);
    const uint32_t *h_len = (const uint32_t *)(p_r + o_len);
    // the last reply that fits: off + len never decreases
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (h_off[m] + h_len[m] <= out->cap) lo = m + 1; else hi = m;
    }
    const uint64_t W = lo ? h_off[lo - 1] + h_len[lo - 1] : 0;
    if (W) {
        rc = hipMemcpyAsync(p_r + o_buf, d_r + o_buf, W, hipMemcpyDeviceToHost, H->s);
        if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
        if (rc != hipSuccess) return (int)rc;
        memcpy(out->buf, p_r + o_buf, W);
    }
    if (n) {
        memcpy(out->off, h_off, (size_t)n * 8);
        memcpy(out->len, h_len, (size_t)n * 4);
    }
    memcpy(out->total, p_r + o_tot, 16);
    return 0;
}

// l7g_cass_replies with host buffers, over the calling thread's stream and
// staging: one copy in, the reply kernels, one copy out, a wait.
int l7g_cass_replies_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                          const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, uint32_t *consumed) {
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, off, len, conn, n}, &H, &dev);
    if (rc != hipSuccess) return (int)rc;
    uint8_t *d_out = H->dev + H->in_cap;
    const DevOut o = OutViews(d_out, n);
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess) rc = (hipError_t)CassReplies(e, dev, o.verdict, o.consumed, H->s);
    if (rc == hipSuccess && n) rc = hipMemcpyAsync(H->pin_out, d_out, CallOutBytes(n), hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc == hipSuccess && n) UnpackOut(H, n, verdict, nullptr, consumed);
    return (int)rc;
}

// l7g_kafka_forward with host buffers, over the calling thread's stream and
// staging: the inputs, the verdicts and the tags copied in, the forward
// kernels, fwd and new_id copied out and waited for.  The arena is not copied
// back: the caller's frames are patched from new_id, four bytes per forwarded
// request.  The session staging is [verdict | tag | fwd | new_id].
int l7g_kafka_forward_host(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                           const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag, uint32_t n,
                           uint64_t now_ms, uint8_t *fwd, uint32_t *new_id) {
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (n && (!off || !len || !conn || !verdict || !fwd || !new_id)) return (int)hipErrorInvalidValue;
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, off, len, conn, n}, &H, &dev);
    if (rc != hipSuccess) return (int)rc;
    const size_t o_tag = ((size_t)n + 15) & ~(size_t)15, o_fwd = o_tag + (size_t)n * 8;
    const size_t o_id = (o_fwd + n + 15) & ~(size_t)15, end = o_id + (size_t)n * 4;
    if ((rc = H->ksess.Grow(H->s, end + 16)) != hipSuccess) return (int)rc;
    uint8_t *d_k = H->ksess.dev, *p_k = H->ksess.pin;
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess && n) {
        memcpy(p_k, verdict, n);
        if (tag) memcpy(p_k + o_tag, tag, (size_t)n * 8);
        rc = hipMemcpyAsync(d_k, p_k, o_fwd, hipMemcpyHostToDevice, H->s);
    }
    if (rc == hipSuccess)
        rc = (hipError_t)l7g_kafka_forward(e, (uint8_t *)dev.arena, arena_len, dev.off, dev.len, dev.conn, d_k,
                                           tag ? (const uint64_t *)(d_k + o_tag) : nullptr, n, now_ms, d_k + o_fwd,
                                           (uint32_t *)(d_k + o_id), H->s);
    if (rc == hipSuccess && n) rc = hipMemcpyAsync(p_k + o_fwd, d_k + o_fwd, end - o_fwd, hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc != hipSuccess || n == 0) return (int)rc;
    memcpy(fwd, p_k + o_fwd, n);
    memcpy(new_id, p_k + o_id, (size_t)n * 4);
    for (uint32_t i = 0; i < n; i++)
        if (fwd[i] == 1 && len[i] >= 12) PutBE32(arena + off[i] + 8, new_id[i]);
    return 0;
}

// l7g_kafka_responses with host buffers, likewise: the inputs copied in, the
// response kernels, the outputs copied out ([tag | orig_id | api_key |
// api_version | found] in the session staging), the caller's frames patched
// from orig_id, four bytes per hit.
int l7g_kafka_responses_host(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                             const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *found, uint32_t *orig_id,
                             int16_t *api_key, int16_t *api_version, uint64_t *tag) {
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (n && (!off || !len || !conn || !found || !orig_id || !api_key || !api_version || !tag))
        return (int)hipErrorInvalidValue;
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, off, len, conn, n}, &H, &dev);
    if (rc != hipSuccess) return (int)rc;
    const size_t o_orig = (size_t)n * 8, o_key = o_orig + (size_t)n * 4, o_ver = o_key + (size_t)n * 2;
    const size_t o_found = o_ver + (size_t)n * 2, end = o_found + n;
    if ((rc = H->ksess.Grow(H->s, end + 16)) != hipSuccess) return (int)rc;
    uint8_t *d_k = H->ksess.dev, *p_k = H->ksess.pin;
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess)
        rc = (hipError_t)l7g_kafka_responses(e, (uint8_t *)dev.arena, arena_len, dev.off, dev.len, dev.conn, n,
                                             d_k + o_found, (uint32_t *)(d_k + o_orig), (int16_t *)(d_k + o_key),
                                             (int16_t *)(d_k + o_ver), (uint64_t *)d_k, H->s);
    if (rc == hipSuccess && n) rc = hipMemcpyAsync(p_k, d_k, end, hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc != hipSuccess || n == 0) return (int)rc;
    memcpy(tag, p_k, (size_t)n * 8);
    memcpy(orig_id, p_k + o_orig, (size_t)n * 4);
    memcpy(api_key, p_k + o_key, (size_t)n * 2);
    memcpy(api_version, p_k + o_ver, (size_t)n * 2);
    memcpy(found, p_k + o_found, n);
    for (uint32_t i = 0; i < n; i++)
        if (found[i] && len[i] >= 8) PutBE32(arena + off[i] + 4, orig_id[i]);
    return 0;
}

// l7g_mc_forward with host buffers, over the calling thread's stream and
// staging: the inputs, the verdicts and the tags copied in, the forward
// kernels, act copied out and waited for.  The session staging is
// [verdict | tag | act].
int l7g_mc_forward_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                        const uint32_t *len, const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag,
                        uint32_t n, uint8_t *act) {
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (n && (!off || !len || !conn || !verdict || !act)) return (int)hipErrorInvalidValue;
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, off, len, conn, n}, &H, &dev);
    if (rc != hipSuccess) return (int)rc;
    const size_t o_tag = ((size_t)n + 15) & ~(size_t)15, o_act = o_tag + (size_t)n * 8, end = o_act + n;
    if ((rc = H->mcsess.Grow(H->s, end + 16)) != hipSuccess) return (int)rc;
    uint8_t *d_m = H->mcsess.dev, *p_m = H->mcsess.pin;
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess && n) {
        memcpy(p_m, verdict, n);
        if (tag) memcpy(p_m + o_tag, tag, (size_t)n * 8);
        rc = hipMemcpyAsync(d_m, p_m, o_act, hipMemcpyHostToDevice, H->s);
    }
    if (rc == hipSuccess)
        rc = (hipError_t)l7g_mc_forward(e, dev.arena, arena_len, dev.off, dev.len, dev.conn, d_m,
                                        tag ? (const uint64_t *)(d_m + o_tag) : nullptr, n, d_m + o_act, H->s);
    if (rc == hipSuccess && n) rc = hipMemcpyAsync(p_m + o_act, d_m + o_act, n, hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc == hipSuccess && n) memcpy(act, p_m + o_act, n);
    return (int)rc;
}

// l7g_mc_replies with host buffers, likewise: the streams copied in, the reply
// kernel, the outputs copied out ([taken | op_aux | op_n | nops | op_kind |
// result] in the session staging).
int l7g_mc_replies_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                        const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_ops, uint8_t *op_kind,
                        uint32_t *op_n, uint64_t *op_aux, uint32_t *nops, uint8_t *result, uint64_t *taken) {
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (n && (!s_off || !s_len || !s_conn || !nops || !result || !taken || (max_ops && (!op_kind || !op_n))))
        return (int)hipErrorInvalidValue;
    HostCtx *H = nullptr;
    DevIn dev;
    hipError_t rc = HostStage(e, {arena, arena_len, s_off, s_len, s_conn, n}, &H, &dev);
    if (rc != hipSuccess) return (int)rc;
    const size_t slots = (size_t)n * max_ops;
    const size_t o_aux = (size_t)n * 8, o_n = o_aux + slots * 8, o_nops = o_n + slots * 4, o_kind = o_nops + (size_t)n * 4;
    const size_t o_res = o_kind + slots, end = o_res + n;
    if ((rc = H->mcsess.Grow(H->s, end + 16)) != hipSuccess) return (int)rc;
    uint8_t *d_m = H->mcsess.dev, *p_m = H->mcsess.pin;
    rc = UploadStaged(H, dev);
    if (rc == hipSuccess && n) rc = hipMemsetAsync(d_m, 0, end, H->s);  // (op slots past nops come back as zeros)
    if (rc == hipSuccess)
        rc = (hipError_t)l7g_mc_replies(e, dev.arena, arena_len, dev.off, dev.len, dev.conn, n, max_ops, d_m + o_kind,
                                        (uint32_t *)(d_m + o_n), (uint64_t *)(d_m + o_aux), (uint32_t *)(d_m + o_nops),
                                        d_m + o_res, (uint64_t *)d_m, H->s);
    if (rc == hipSuccess && n) rc = hipMemcpyAsync(p_m, d_m, end, hipMemcpyDeviceToHost, H->s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(H->s);
    if (rc != hipSuccess || n == 0) return (int)rc;
    memcpy(taken, p_m, (size_t)n * 8);
    if (op_aux) memcpy(op_aux, p_m + o_aux, slots * 8);
    if (slots) memcpy(op_n, p_m + o_n, slots * 4);
    memcpy(nops, p_m + o_nops, (size_t)n * 4);
    if (slots) memcpy(op_kind, p_m + o_kind, slots);
    memcpy(result, p_m + o_res, n);
    return 0;
}

}  // extern "C"

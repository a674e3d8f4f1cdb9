// Memcached sessions behind the C-ABI (product code): the lifetime of the
// device state (kernels/memcached_session.hip) and the calls over device
// pointers, l7g_mc_forward and l7g_mc_replies, each on the caller's stream
// with that stream's scratch.  Nothing of l7g_classify's plan is involved.
// The slot sync and the frame of the entries are sessions.h's, as for every
// protocol's sessions; the ring grows beside the slots here.  The host-buffer
// twins are in host_call.cc.
#include "deny_templates.h"
#include "sessions.h"

namespace {

constexpr uint32_t kMaxRing = 1u << 16;  // ring entries per connection at most (1 MiB of intents)
constexpr size_t kStatBytes = (MSS_WORDS + 2) * sizeof(unsigned long long);

static_assert(sizeof(l7::kMcDeniedText) - 1 == kMcDeniedTextLen && sizeof(l7::kMcDeniedBinary) == kMcDeniedBinaryLen,
              "the denied messages and the INJECT counts of the reply kernel");

size_t RingBytes(const McSessions &S, uint32_t slots) { return (size_t)slots * S.cap * sizeof(McSessIntent); }

bool On(const l7g_engine *e) { return e->mcsess.stats != nullptr; }

}  // namespace

void McSessionsFree(l7g_engine *e) {
    for (void *p : {(void *)e->mcsess.slots, (void *)e->mcsess.ring, (void *)e->mcsess.stats})
        if (p) hipFree(p);
    e->mcsess = McSessions{};
    e->mcsess_ring_slots = 0;
    e->mcsess_reset.Clear();
}

hipError_t McSessionsSync(l7g_engine *e) {
    McSessions &S = e->mcsess;
    if (!S.stats) return hipSuccess;
    // (a zeroed slot queues nothing: the ring's bytes need no reset)
    hipError_t rc = SlotsSync(
        e, S.slots, S.nslots, e->mcsess_reset, [] { return hipSuccess; },
        [&](const uint32_t *conn, uint32_t n) { return LaunchMcSessReset(S, conn, n, nullptr); });
    if (rc != hipSuccess || S.nslots <= e->mcsess_ring_slots) return rc;
    // the ring beside the slots: connection c's entries stay at c * cap
    McSessIntent *d = nullptr;
    if ((rc = hipMalloc(&d, RingBytes(S, S.nslots))) != hipSuccess) return rc;
    rc = Quiet(e, [&] {
        hipError_t r = hipMemsetAsync(d, 0, RingBytes(S, S.nslots), nullptr);
        if (r == hipSuccess && e->mcsess_ring_slots)
            r = hipMemcpyAsync(d, S.ring, RingBytes(S, e->mcsess_ring_slots), hipMemcpyDeviceToDevice, nullptr);
        return r;
    });
    if (rc != hipSuccess) { hipFree(d); return rc; }
    if (S.ring) hipFree(S.ring);
    S.ring = d;
    e->mcsess_ring_slots = S.nslots;
    return hipSuccess;
}

extern "C" {

int l7g_mc_sessions_enable(l7g_engine *e, uint32_t max_pending, char *err, size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = EnableBegin(e, err, errlen);
    if (rc != hipSuccess) return (int)rc;
    McSessionsFree(e);
    if (max_pending == 0) return 0;
    if (max_pending > kMaxRing) { set_err(err, errlen, "max_pending exceeds 65536"); return (int)hipErrorInvalidValue; }
    McSessions S{};
    S.cap = 1;
    while (S.cap < max_pending) S.cap <<= 1;
    rc = hipMalloc(&S.stats, kStatBytes);
    if (rc == hipSuccess) rc = hipMemsetAsync(S.stats, 0, kStatBytes, nullptr);
    e->mcsess = S;  // (the slots and the ring come with the first call: McSessionsSync)
    return EnableEnd(e, rc, McSessionsFree, err, errlen);
}

int l7g_mc_forward(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                   const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag, uint32_t n, uint8_t *act,
                   void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = Enter(e, On(e), kSyncMc);
    if (rc != hipSuccess || n == 0) return (int)rc;
    if (!off || !len || !conn || !verdict || !act) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    if ((rc = GetScratch(e, s, &S)) != hipSuccess) return (int)rc;
    const uint32_t nconns = (uint32_t)e->conns.size();
    const size_t need = McSessForwardScratchBytes(n, nconns);
    if (need == 0) return (int)hipErrorInvalidValue;
    if ((rc = S->Grow(&S->d_mcsess, &S->mcsess_cap, need, need)) != hipSuccess) return (int)rc;
    const McSessBatch B{arena, arena_len, off, len, conn, e->d_conns, n, nconns};
    rc = LaunchMcSessForward(B, e->mcsess, verdict, tag, act, S->d_mcsess, S->mcsess_cap, s);
    return (int)CallEnd(S, s, rc);
}

int l7g_mc_replies(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                   const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_ops, uint8_t *op_kind,
                   uint32_t *op_n, uint64_t *op_aux, uint32_t *nops, uint8_t *result, uint64_t *taken, void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = Enter(e, On(e), kSyncMc);
    if (rc != hipSuccess || n == 0) return (int)rc;
    if (!s_off || !s_len || !s_conn || !nops || !result || !taken || (max_ops && (!op_kind || !op_n)))
        return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    if ((rc = GetScratch(e, s, &S)) != hipSuccess) return (int)rc;
    const McSessBatch B{arena, arena_len, s_off, s_len, s_conn, e->d_conns, n, (uint32_t)e->conns.size()};
    rc = LaunchMcSessReplies(B, e->mcsess, McReplyOut{op_kind, op_n, op_aux, nops, result, taken, max_ops}, s);
    return (int)CallEnd(S, s, rc);
}

int l7g_mc_session_reset(l7g_engine *e, const uint32_t *conn, uint32_t n) {
    std::lock_guard<std::mutex> g(e->mu);
    return SessionReset(e, On(e), e->mcsess_reset, conn, n, McSessionsSync);
}

void l7g_mc_session_stats(l7g_engine *e, uint64_t out[8]) {
    std::lock_guard<std::mutex> g(e->mu);
    for (int k = 0; k < 8; k++) out[k] = 0;
    unsigned long long h[MSS_WORDS + 2] = {};
    if (!SessionStats(e, On(e), McSessionsSync, e->mcsess.stats, MSS_WORDS, h,
                      [&](unsigned long long *out2) { return LaunchMcSessLive(e->mcsess, out2, nullptr); }))
        return;
    out[0] = h[MSS_WORDS];
    out[1] = h[MSS_WORDS + 1];
    for (int k = 0; k < MSS_WORDS; k++) out[2 + k] = h[k];
}

const uint8_t *l7g_mc_denied_message(int binary, size_t *len) {
    if (len) *len = binary ? l7::kMcDeniedBinaryLen : l7::kMcDeniedTextLen;
    return binary ? l7::kMcDeniedBinary : (const uint8_t *)l7::kMcDeniedText;
}

}  // extern "C"

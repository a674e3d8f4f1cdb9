// Kafka sessions behind the C-ABI (product code): the lifetime of the device
// tables (kernels/kafka_session.hip) and the calls over device pointers,
// l7g_kafka_forward and l7g_kafka_responses, each on the caller's stream with
// that stream's scratch.  Nothing of l7g_classify's plan is involved.  The
// slot sync and the frame of the entries are sessions.h's, as for every
// protocol's sessions; the host-buffer twins are in host_call.cc.
#include "sessions.h"

namespace {

size_t TableBytes(const KafkaSessions &S) { return ((size_t)S.mask + 1) * sizeof(KafkaSessEntry); }
constexpr size_t kStatBytes = (KSS_WORDS + 2) * sizeof(unsigned long long);

bool On(const l7g_engine *e) { return e->ksess.tab != nullptr; }

}  // namespace

void KafkaSessionsFree(l7g_engine *e) {
    for (void *p : {(void *)e->ksess.slots, (void *)e->ksess.tab, (void *)e->ksess.spare, (void *)e->ksess.stats})
        if (p) hipFree(p);
    e->ksess = KafkaSessions{};
    e->ksess_reset.Clear();
    e->ksess_expired = 0;
}

hipError_t KafkaSessionsSync(l7g_engine *e) {
    KafkaSessions &S = e->ksess;
    if (!S.tab) return hipSuccess;
    return SlotsSync(
        e, S.slots, S.nslots, e->ksess_reset,
        [&] { return hipMemsetAsync(S.tab, 0, TableBytes(S), nullptr); },
        [&](const uint32_t *conn, uint32_t n) { return LaunchKafkaSessReset(S, conn, n, nullptr); });
}

extern "C" {

int l7g_kafka_sessions_enable(l7g_engine *e, uint32_t max_inflight, char *err, size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = EnableBegin(e, err, errlen);
    if (rc != hipSuccess) return (int)rc;
    KafkaSessionsFree(e);
    if (max_inflight == 0) return 0;
    if (max_inflight > (1u << 28)) { set_err(err, errlen, "max_inflight exceeds 2^28"); return (int)hipErrorInvalidValue; }
    // open addressing: the power of two that holds twice the requests in flight
    uint32_t cap = 2;
    while (cap < 2 * max_inflight) cap <<= 1;
    KafkaSessions S{};
    S.mask = cap - 1;
    const size_t tab = TableBytes(S);
    rc = hipMalloc(&S.tab, tab);
    if (rc == hipSuccess) rc = hipMalloc(&S.spare, tab);
    if (rc == hipSuccess) rc = hipMalloc(&S.stats, kStatBytes);
    if (rc == hipSuccess) rc = hipMemsetAsync(S.tab, 0, tab, nullptr);
    if (rc == hipSuccess) rc = hipMemsetAsync(S.stats, 0, kStatBytes, nullptr);
    e->ksess = S;  // (the slots come with the first call: KafkaSessionsSync)
    return EnableEnd(e, rc, KafkaSessionsFree, err, errlen);
}

int l7g_kafka_forward(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                      const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag, uint32_t n, uint64_t now_ms,
                      uint8_t *fwd, uint32_t *new_id, void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = Enter(e, On(e), kSyncKafka);
    if (rc != hipSuccess || n == 0) return (int)rc;
    if (!off || !len || !conn || !verdict || !fwd || !new_id) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    if ((rc = GetScratch(e, s, &S)) != hipSuccess) return (int)rc;
    const uint32_t nconns = (uint32_t)e->conns.size();
    const size_t need = KafkaSessForwardScratchBytes(n, nconns);
    if (need == 0) return (int)hipErrorInvalidValue;
    if ((rc = S->Grow(&S->d_ksess, &S->ksess_cap, need, need)) != hipSuccess) return (int)rc;
    const KafkaSessBatch B{arena, arena_len, off, len, conn, e->d_conns, n, nconns};
    rc = LaunchKafkaSessForward(B, e->ksess, verdict, tag, now_ms, fwd, new_id, S->d_ksess, S->ksess_cap, s);
    return (int)CallEnd(S, s, rc);
}

int l7g_kafka_responses(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                        const uint32_t *conn, uint32_t n, uint8_t *found, uint32_t *orig_id, int16_t *api_key,
                        int16_t *api_version, uint64_t *tag, void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = Enter(e, On(e), kSyncKafka);
    if (rc != hipSuccess || n == 0) return (int)rc;
    if (!off || !len || !conn || !found || !orig_id || !api_key || !api_version || !tag) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    if ((rc = GetScratch(e, s, &S)) != hipSuccess) return (int)rc;
    const size_t need = KafkaSessResponsesScratchBytes(n);
    if ((rc = S->Grow(&S->d_ksess, &S->ksess_cap, need, need)) != hipSuccess) return (int)rc;
    const KafkaSessBatch B{arena, arena_len, off, len, conn, e->d_conns, n, (uint32_t)e->conns.size()};
    rc = LaunchKafkaSessResponses(B, e->ksess, found, orig_id, api_key, api_version, tag, S->d_ksess, S->ksess_cap, s);
    return (int)CallEnd(S, s, rc);
}

int l7g_kafka_session_gc(l7g_engine *e, uint64_t now_ms, uint64_t lifetime_ms, uint64_t *expired) {
    std::lock_guard<std::mutex> g(e->mu);
    if (expired) *expired = 0;
    hipError_t rc = Enter(e, On(e), kSyncKafka);
    if (rc != hipSuccess) return (int)rc;
    KafkaSessions &S = e->ksess;
    unsigned long long gone = 0;
    rc = Quiet(e, [&] {
        hipError_t r = hipMemsetAsync(S.spare, 0, TableBytes(S), nullptr);
        if (r == hipSuccess) r = hipMemsetAsync(S.stats + KSS_EXPIRED, 0, sizeof gone, nullptr);
        if (r == hipSuccess) r = LaunchKafkaSessGc(S, now_ms, lifetime_ms, S.stats + KSS_EXPIRED, nullptr);
        if (r == hipSuccess) r = hipMemcpyAsync(&gone, S.stats + KSS_EXPIRED, sizeof gone, hipMemcpyDeviceToHost, nullptr);
        return r;
    });
    if (rc != hipSuccess) return (int)rc;
    std::swap(S.tab, S.spare);
    e->ksess_expired += gone;
    if (expired) *expired = gone;
    return 0;
}

int l7g_kafka_session_reset(l7g_engine *e, const uint32_t *conn, uint32_t n) {
    std::lock_guard<std::mutex> g(e->mu);
    return SessionReset(e, On(e), e->ksess_reset, conn, n, KafkaSessionsSync);
}

void l7g_kafka_session_stats(l7g_engine *e, uint64_t out[7]) {
    std::lock_guard<std::mutex> g(e->mu);
    for (int k = 0; k < 7; k++) out[k] = 0;
    unsigned long long h[KSS_WORDS + 2] = {};
    if (!SessionStats(e, On(e), KafkaSessionsSync, e->ksess.stats, KSS_WORDS, h,
                      [&](unsigned long long *out2) { return LaunchKafkaSessLive(e->ksess, out2, nullptr); }))
        return;
    out[0] = h[KSS_WORDS];
    out[1] = h[KSS_WORDS + 1];
    out[2] = h[KSS_DROPPED];
    out[3] = h[KSS_FORWARDED];
    out[4] = h[KSS_FOUND];
    out[5] = h[KSS_MISSED];
    out[6] = e->ksess_expired;
}

}  // extern "C"

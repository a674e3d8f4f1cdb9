// Cassandra sessions behind the C-ABI (product code): the lifetime of the
// device tables (kernels/cassandra_session.hip) and l7g_cass_replies, the call
// over device pointers that binds into them, on the caller's stream with that
// stream's cassandra scratch.  l7g_classify reads and commits them in its own
// plan (classify.cc).  The slot sync and the frame of the entries are
// sessions.h's; the host-buffer twin is in host_call.cc.
#include "sessions.h"

static size_t TableBytes(const CassSessions &S) { return ((size_t)S.mask + 1) * sizeof(CassEntry); }
constexpr size_t kStatBytes = (CSS_WORDS + 2) * sizeof(unsigned long long);

void SessionsFree(l7g_engine *e) {
    for (void *p : {(void *)e->sess.slots, (void *)e->sess.by_stream, (void *)e->sess.by_id, (void *)e->sess.stats})
        if (p) hipFree(p);
    e->sess = CassSessions{};
    e->sess_reset.Clear();
}

hipError_t SessionsSync(l7g_engine *e) {
    CassSessions &S = e->sess;
    if (!S.by_id) return hipSuccess;
    return SlotsSync(
        e, S.slots, S.nslots, e->sess_reset,
        [&] {
            hipError_t r = hipMemsetAsync(S.by_stream, 0, TableBytes(S), nullptr);
            if (r == hipSuccess) r = hipMemsetAsync(S.by_id, 0, TableBytes(S), nullptr);
            return r;
        },
        [&](const uint32_t *conn, uint32_t n) { return LaunchCassandraSessionReset(S, conn, n, nullptr); });
}

// l7g_cass_replies: the replies framed, the RESULT/prepared ones bound
int CassReplies(l7g_engine *e, const DevIn &in, uint8_t *verdict, uint32_t *consumed, void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = Enter(e, e->sess.by_id != nullptr, kSyncCass);  // (sessions off: nothing to bind into)
    if (rc != hipSuccess || in.n == 0) return (int)rc;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    if ((rc = GetScratch(e, s, &S)) != hipSuccess) return (int)rc;
    const size_t need = CassandraScratchBytes(in.n);
    if (need == 0) return (int)hipErrorInvalidValue;
    rc = S->Grow(&S->d_use, &S->use_cap, need, need);
    const Batch B{in.arena, in.arena_len, in.off, in.len, in.conn, e->d_conns, verdict, nullptr, consumed, in.n,
                  (uint32_t)e->conns.size()};
    if (rc == hipSuccess) rc = LaunchCassandraReplies(B, e->sess, S->d_use, S->use_cap, s);
    return (int)CallEnd(S, s, rc);
}

extern "C" {

int l7g_cass_sessions_enable(l7g_engine *e, uint32_t max_statements, char *err, size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    hipError_t rc = EnableBegin(e, err, errlen);
    if (rc != hipSuccess) return (int)rc;
    SessionsFree(e);
    if (max_statements == 0) return 0;
    // open addressing: twice the statements, so that probe chains stay short when all are held
    if (max_statements > (1u << 24)) { set_err(err, errlen, "max_statements exceeds 2^24"); return (int)hipErrorInvalidValue; }
    uint32_t cap = 16;
    while (cap < 2 * max_statements) cap <<= 1;
    CassSessions S{};
    S.mask = cap - 1;
    const size_t tab = TableBytes(S);
    rc = hipMalloc(&S.by_stream, tab);
    if (rc == hipSuccess) rc = hipMalloc(&S.by_id, tab);
    if (rc == hipSuccess) rc = hipMalloc(&S.stats, kStatBytes);
    if (rc == hipSuccess) rc = hipMemsetAsync(S.by_stream, 0, tab, nullptr);
    if (rc == hipSuccess) rc = hipMemsetAsync(S.by_id, 0, tab, nullptr);
    if (rc == hipSuccess) rc = hipMemsetAsync(S.stats, 0, kStatBytes, nullptr);
    e->sess = S;  // (the slots come with the first launch: SessionsSync)
    return EnableEnd(e, rc, SessionsFree, err, errlen);
}

int l7g_cass_replies(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                     const uint32_t *conn, uint32_t n, uint8_t *verdict, uint32_t *consumed, void *stream) {
    return CassReplies(e, {arena, arena_len, off, len, conn, n}, verdict, consumed, stream);
}

int l7g_cass_session_reset(l7g_engine *e, const uint32_t *conn, uint32_t n) {
    std::lock_guard<std::mutex> g(e->mu);
    return SessionReset(e, e->sess.by_id != nullptr, e->sess_reset, conn, n, SessionsSync);
}

void l7g_cass_session_stats(l7g_engine *e, uint64_t out[6]) {
    std::lock_guard<std::mutex> g(e->mu);
    for (int k = 0; k < 6; k++) out[k] = 0;
    unsigned long long h[CSS_WORDS + 2] = {};
    if (!SessionStats(e, e->sess.by_id != nullptr, SessionsSync, e->sess.stats, CSS_WORDS, h,
                      [&](unsigned long long *out2) { return LaunchCassandraSessionLive(e->sess, out2, nullptr); }))
        return;
    out[0] = h[CSS_WORDS];
    out[1] = h[CSS_WORDS + 1];
    out[2] = h[CSS_DROPPED];
    out[3] = h[CSS_OVERFLOW];
    out[4] = h[CSS_RESOLVED];
    out[5] = h[CSS_UNPREPARED];
}

}  // extern "C"

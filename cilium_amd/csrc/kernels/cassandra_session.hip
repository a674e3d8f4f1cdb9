// Cassandra sessions on gfx950 (product code): what proxylib's parser keeps
// per connection (cassandraparser.go:146-160) -- the keyspace of the last USE,
// preparedPathByStreamID (written by PREPARE requests, :471-581) and
// preparedPathByPreparedID (written by RESULT/prepared replies, :605-642, read
// by EXECUTE) -- resident in HBM (device_tables.h CassSlot / CassEntry), so
// that l7g_classify gives the reference's answers across batches.
//
// Nothing here runs while a classifier reads the tables.  A request batch is
// classified first (cassandra_session_classify_kernel, read-only) and
// committed after it, in batch order per connection:
//   cass_commit_prepares_kernel  the sorted PREPARE marks, one lane per
//     connection segment: each statement's action and parts[3] (the keyspace in
//     force at its position joined: the last USE before it in the batch, else
//     the slot's keyspace as it stood before the batch) is upserted under
//     (connection, stream id); the last one in batch order wins;
//   cass_commit_keyspace_kernel  the last USE of every connection goes to its
//     slot (after the PREPAREs, which read the slot's previous keyspace).
// A reply batch is framed by cass_replies_kernel (ref_cass_reply's outcomes),
// its RESULT/prepared frames are sorted by (connection, index), and
// cass_commit_binds_kernel copies each one's stream entry under (connection,
// id), again one lane per connection, the last reply winning.
//
// A connection with many PREPAREs (or prepared replies) in one batch is walked
// by one lane: these are rare operations, and the single walker is what makes
// "last in batch order wins" and the full-key compare exact without any
// protocol between lanes.  Lanes of different connections meet only in the
// CAS that claims a slot (kernels/cass_session.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../device_tables.h"
#include "cass_parse.h"
#include "cass_session.h"
#include "launch.h"

namespace l7 {

namespace {

constexpr int kBlock = 256;

// parts[3] as bytes into a statement's entry; n counts on past the cap
struct PathSink {
    uint8_t *out;
    uint32_t n;
    __device__ void raw(uint32_t c) {
        if (n < kCassPathMax) out[n] = (uint8_t)c;
        n++;
    }
    __device__ void rune(uint32_t r) {
        uint8_t e[4];
        const uint32_t k = cass_encode(r, e);
        for (uint32_t j = 0; j < k; j++) raw(e[j]);
    }
};

}  // namespace

__global__ __launch_bounds__(kBlock) void cass_commit_prepares_kernel(Batch B, CassTables T, CassSessions S,
                                                                      const uint64_t *__restrict__ use_sorted,
                                                                      const uint64_t *__restrict__ prep_sorted) {
    uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= B.n || prep_sorted[j] == ~0ull || !segment_head(prep_sorted, j)) return;
    const uint32_t ci = key_conn(prep_sorted[j]);
    if (ci >= S.nslots) return;
    CassSlot *slot = &S.slots[ci];
    const unsigned long long mine = sess_claim_of(ci, slot->gen);
    for (; j < B.n && prep_sorted[j] != ~0ull && key_conn(prep_sorted[j]) == ci; j++) {
        const uint32_t i = key_index(prep_sorted[j]);
        // (a complete PREPARE frame whose query parses: cassandra_marks_kernel)
        const uint8_t *b = B.arena + B.offs[i];
        const CassQuery Q = cass_parse_query(b + 13, cass_be32(b + 9), T.lower, T.nlower);
        const uint8_t *ks = nullptr;
        CassQuery K{};
        bool over = false;
        if (Q.seg3 == S3_KS_TABLE) {
            const int64_t best = cass_last_before(use_sorted, B.n, ci, i);
            if (best >= 0) {
                const uint8_t *bj = B.arena + B.offs[best];
                K = cass_parse_query(bj + 13, cass_be32(bj + 9), T.lower, T.nlower);
                ks = bj + 13;
            } else if (slot->ks_len == kCassOver) {
                over = true;
            } else {
                ks = slot->ks;
                K.te = slot->ks_len;
                K.fc = slot->ks_fc;
            }
        }
        CassEntry *e = cass_upsert(S.by_stream, S.mask, S.slots, S.nslots, mine, ci, b + 2, 2);
        if (!e) {  // full: the statement is not kept; its binding must not resolve to an older one
            slot->dropped = 1;
            atomicAdd(&S.stats[CSS_DROPPED], 1ull);
            continue;
        }
        PathSink sink{e->path, 0};
        if (!over) cass_seg3(Q, b + 13, ks, K.ts, K.te, K.fc, T.lower, T.nlower, sink);
        over = over || sink.n > kCassPathMax;
        if (over) atomicAdd(&S.stats[CSS_OVERFLOW], 1ull);
        e->action = Q.action;
        e->path_len = over ? kCassOver : sink.n;
    }
}

__global__ __launch_bounds__(kBlock) void cass_commit_keyspace_kernel(Batch B, CassTables T, CassSessions S,
                                                                      const uint64_t *__restrict__ use_sorted) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= B.n || use_sorted[j] == ~0ull) return;
    const uint32_t ci = key_conn(use_sorted[j]);
    // the connection's last USE of the batch only
    if (j + 1 < B.n && use_sorted[j + 1] != ~0ull && key_conn(use_sorted[j + 1]) == ci) return;
    if (ci >= S.nslots) return;
    const uint32_t i = key_index(use_sorted[j]);
    const uint8_t *q = B.arena + B.offs[i] + 13;
    const CassQuery Q = cass_parse_query(q, cass_be32(q - 4), T.lower, T.nlower);
    CassSlot *slot = &S.slots[ci];
    const uint32_t n = Q.te - Q.ts;
    if (n > kCassKsMax) {
        slot->ks_len = kCassOver;
        atomicAdd(&S.stats[CSS_OVERFLOW], 1ull);
        return;
    }
    for (uint32_t k = 0; k < n; k++) slot->ks[k] = q[Q.ts + k];
    slot->ks_len = n;
    slot->ks_fc = Q.fc == ~0u ? ~0u : Q.fc > Q.ts ? Q.fc - Q.ts : 0u;
}

// One lane per reply (ref_cass_reply, oracle/cassandra_ref.c): framing as for
// requests, cassandraParseReply's slices bounded by the buffer handed in;
// keys[i] = (connection << 32 | i) for a RESULT/prepared reply to bind, else ~0.
__global__ __launch_bounds__(kBlock) void cass_replies_kernel(Batch B, uint64_t *__restrict__ keys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= B.n) return;
    keys[i] = ~0ull;
    const uint32_t ci = B.conn_ids[i];
    uint8_t verdict = V_UNSUPPORTED;
    uint32_t consumed = 0;
    const uint64_t off = B.offs[i];
    const uint32_t len = B.lens[i];
    if (ci < B.nconns && B.conns[ci].proto == PROTO_CASSANDRA && l7_in_arena(off, len, B.arena_len)) {
        const uint8_t *d = B.arena + off;
        const uint32_t rl = len >= 9 ? cass_be32(d + 5) : 0;
        if (len < 9) {
            verdict = V_INCOMPLETE;
            consumed = 9 - len;
        } else if (rl > kCassMaxLen) {
            verdict = V_PARSE_ERROR;
            consumed = 3;
        } else if (9 + rl > len) {
            verdict = V_INCOMPLETE;
            consumed = 9 + rl - len;
        } else {
            verdict = V_ALLOW;
            consumed = 9 + rl;
            if ((d[0] & 0x80) && !(d[1] & 0x01) && d[4] == 0x08) {
                if (len < 13) {
                    verdict = V_PARSE_ERROR;  // data[9:13] panics
                } else if (cass_be32(d + 9) == 4) {
                    if (len < 15 || 15u + cass_be16(d + 13) > len) verdict = V_PARSE_ERROR;  // the id's slices panic
                    else keys[i] = sess_key(ci, i);
                }
                if (verdict == V_PARSE_ERROR) consumed = 0;
            }
        }
    }
    B.verdict[i] = verdict;
    B.consumed[i] = consumed;
}

__global__ __launch_bounds__(kBlock) void cass_commit_binds_kernel(Batch B, CassSessions S,
                                                                   const uint64_t *__restrict__ sorted) {
    uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= B.n || sorted[j] == ~0ull || !segment_head(sorted, j)) return;
    const uint32_t ci = key_conn(sorted[j]);
    if (ci >= S.nslots) return;
    const CassSlot *slot = &S.slots[ci];
    const unsigned long long mine = sess_claim_of(ci, slot->gen);
    for (; j < B.n && sorted[j] != ~0ull && key_conn(sorted[j]) == ci; j++) {
        const uint8_t *d = B.arena + B.offs[key_index(sorted[j])];
        const uint32_t il = cass_be16(d + 13);
        const uint8_t *id = d + 15;
        const CassEntry *st = cass_find(S.by_stream, S.mask, mine, ci, d + 2, 2);
        if (!st) {
            // no statement under this stream id: nothing is bound -- unless a PREPARE
            // of this connection was dropped, when the reply may have been its
            // answer and an older binding of the id must stop resolving
            if (slot->dropped && il <= kCassIdMax) {
                CassEntry *old = cass_find(S.by_id, S.mask, mine, ci, id, il);
                if (old) old->action = kCassTomb;
            }
            continue;
        }
        if (il > kCassIdMax) {  // not bound: its EXECUTE answers unprepared
            atomicAdd(&S.stats[CSS_OVERFLOW], 1ull);
            continue;
        }
        CassEntry *e = cass_upsert(S.by_id, S.mask, S.slots, S.nslots, mine, ci, id, il);
        if (!e) {
            atomicAdd(&S.stats[CSS_DROPPED], 1ull);
            continue;
        }
        const uint32_t pn = st->path_len;
        for (uint32_t k = 0; k < pn && pn != kCassOver; k++) e->path[k] = st->path[k];
        e->action = st->action;
        e->path_len = pn;
    }
}

// New-connection events: the slots' generation moves on (their statements stop
// resolving at once and their table slots become reusable), the keyspace is "".
__global__ __launch_bounds__(kBlock) void cass_reset_kernel(CassSessions S, const uint32_t *__restrict__ conn,
                                                            uint32_t n) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n || conn[k] >= S.nslots) return;
    CassSlot *slot = &S.slots[conn[k]];
    // (an index named twice is bumped by either lane or both: any new generation serves)
    atomicAdd(&slot->gen, 1u);
    slot->ks_len = 0;
    slot->ks_fc = ~0u;
    slot->dropped = 0;
}

// out[0] / out[1]: statements by stream / by id that still resolve
__global__ __launch_bounds__(kBlock) void cass_live_kernel(CassSessions S, unsigned long long *__restrict__ out) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p > S.mask) return;
    const CassEntry *tabs[2] = {S.by_stream, S.by_id};
    for (int t = 0; t < 2; t++) {
        const CassEntry *e = &tabs[t][p];
        const unsigned long long c = e->claim;
        if (c == 0 || e->action == kCassTomb) continue;
        if (sess_claim_live(S.slots, S.nslots, c)) atomicAdd(&out[t], 1ull);
    }
}

hipError_t LaunchCassandraCommit(const Batch &B, const CassTables &T, const CassSessions &S,
                                 const uint64_t *use_sorted, const uint64_t *prep_sorted, hipStream_t stream) {
    const dim3 grid((B.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(cass_commit_prepares_kernel, grid, dim3(kBlock), 0, stream, B, T, S, use_sorted, prep_sorted);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(cass_commit_keyspace_kernel, grid, dim3(kBlock), 0, stream, B, T, S, use_sorted);
    return hipGetLastError();
}

// scratch: CassandraScratchBytes(B.n) bytes; B.rule is not written
hipError_t LaunchCassandraReplies(const Batch &B, const CassSessions &S, void *scratch, size_t scratch_bytes,
                                  hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const CassandraScratch L = CassandraLayout(B.n, false, 0);
    if (scratch_bytes < L.temp) return hipErrorInvalidValue;
    uint8_t *base = (uint8_t *)scratch;
    uint64_t *keys = (uint64_t *)(base + L.keys), *sorted = (uint64_t *)(base + L.sorted);
    void *temp = base + L.temp;
    size_t temp_bytes = scratch_bytes - L.temp;
    const dim3 grid((B.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(cass_replies_kernel, grid, dim3(kBlock), 0, stream, B, keys);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    rc = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, sorted, (int)B.n, 0, 64, stream);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(cass_commit_binds_kernel, grid, dim3(kBlock), 0, stream, B, S, sorted);
    return hipGetLastError();
}

hipError_t LaunchCassandraSessionReset(const CassSessions &S, const uint32_t *conn, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cass_reset_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, S, conn, n);
    return hipGetLastError();
}

hipError_t LaunchCassandraSessionLive(const CassSessions &S, unsigned long long *out2, hipStream_t stream) {
    hipLaunchKernelGGL(cass_live_kernel, dim3(S.mask / kBlock + 1), dim3(kBlock), 0, stream, S, out2);
    return hipGetLastError();
}

}  // namespace l7

// proxylib cassandra request classification on gfx950 (product code).
//
// proxylib/cassandra/cassandraparser.go, one lane per request (a frame at the
// start of the request's bytes):
//   framing (OnData :171-210): < 9 bytes => INCOMPLETE, consumed = the missing
//     header bytes (MORE); body length > 256 MB => PARSE_ERROR, consumed 3
//     (ERROR_INVALID_FRAME_LENGTH); missing body bytes => INCOMPLETE with their
//     count; reply direction bit or compression flag => PARSE_ERROR, consumed
//     2 (ERROR_INVALID_FRAME_TYPE);
//   cassandraParseRequest (:471-581): QUERY / PREPARE => parseQuery
//     (kernels/cass_parse.h; a short body or a trailing FROM is a Go panic =>
//     PARSE_ERROR, consumed 0; an unparsable query => PARSE_ERROR 2); BATCH
//     always panics (:519); EXECUTE => PARSE_ERROR 2 without sessions, since a
//     batch carries no prepared statements (the proxylib shim answers EXECUTE
//     from its PREPARE cache), and with sessions the verdict of the statement
//     its id is bound to; any other opcode => a two-part path every rule matches;
//   Connection.Matches over the rule set's image: query_action row AND the
//     query_table automata over parts[3] of the path, which is produced as a
//     stream of lowered bytes straight from the request (and, for an undotted
//     table, from the USE request that set the keyspace).
//
// Keyspace: a batch's requests on one connection are read in batch order, as
// proxylib's OnData reads a connection's frames, so the keyspace of request i
// is the one set by the last USE (a QUERY or PREPARE "use x") before i on the
// same connection; none => "" (with sessions: the keyspace the connection's
// slot holds).  cassandra_use_kernel writes one key per
// request, (connection << 32 | index) for a USE request and ~0 otherwise; the
// keys are radix-sorted (hipcub), and a lane whose table needs the keyspace
// finds the last USE on its connection before it by one binary search over
// them: O(n log n) per batch however many USE requests it holds (a scan of an
// unordered USE list per lane was O(n x #USE), quadratic on a USE-heavy batch).
//
// Sessions (l7g_cass_sessions_enable) are a second instantiation of the
// classifier: it only reads the session tables (slot keyspace, statements by
// id); the batch's USE and PREPARE requests are committed to them by the
// launches that follow it (kernels/cassandra_session.hip).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../device_tables.h"
#include "cass_parse.h"
#include "cass_session.h"
#include "launch.h"

namespace l7 {

namespace {

constexpr int kBlock = 256;

struct CountSink {
    uint32_t n = 0;
    __device__ void raw(uint32_t) { n++; }
    __device__ void rune(uint32_t) { n++; }
};
struct DfaSink {
    const uint8_t *img;
    DevDfa D;
    uint32_t st;
    __device__ void raw(uint32_t c) {
        if (st) st = ((const uint16_t *)(img + D.trans_off))[st * D.ncls + img[D.cls_off + c]];
    }
    __device__ void rune(uint32_t r) {
        uint8_t e[4];
        const uint32_t n = cass_encode(r, e);
        for (uint32_t k = 0; k < n; k++) raw(e[k]);
    }
};
struct NfaSink {
    const uint8_t *pool;
    uint64_t off;
    NfaRun R;
    __device__ void raw(uint32_t c) { nfa_step(pool, off, R, 0xFFFD, c); }
    __device__ void rune(uint32_t r) {
        uint8_t e[4];
        cass_encode(r, e);
        nfa_step(pool, off, R, r, e[0]);
    }
};

// Where parts[3] of a path comes from: a query's token spans (and its keyspace) ...
struct QuerySrc {
    const CassQuery &Q;
    const uint8_t *q, *ks;
    const CassQuery &K;
    const uint32_t *lower;
    uint32_t nlower;
    template <class Sink>
    __device__ __forceinline__ void emit(Sink &s) const {
        cass_seg3(Q, q, ks, K.ts, K.te, K.fc, lower, nlower, s);
    }
};
// ... or the bytes a PREPARE emitted (CassEntry::path), decoded again: an
// invalid byte goes to raw(), everything else to rune(), as cass_emit fed them
// (the NFA sink tells a kept invalid byte from an encoded U+FFFD).
struct StoredSrc {
    const uint8_t *p;
    uint32_t n;
    template <class Sink>
    __device__ __forceinline__ void emit(Sink &s) const {
        for (uint32_t i = 0; i < n;) {
            uint32_t w;
            const uint32_t r = nfa_decode(p, i, n, &w);
            if (w == 1 && r == 0xFFFD) s.raw(p[i]);
            else s.rune(r);
            i += w;
        }
    }
};

// Connection.Matches of the path (action, parts[3] from src) over the rule
// set's image: the first rule that holds => ALLOW with its id, else the
// image's terminal verdict.
template <class Src>
__device__ __forceinline__ void cass_match(const uint8_t *img, const CassImgHeader *H, const CassTables &T,
                                           int32_t action, const Src &src, uint64_t *scratch, uint8_t *verdict,
                                           int32_t *rule) {
    const uint32_t nch = H->nchunks;
    const int32_t *ids = (const int32_t *)(img + H->rule_off);
    CountSink cnt;
    src.emit(cnt);
    uint64_t ok[kCassMaxChunks];
    const uint64_t *act = (const uint64_t *)(img + H->act_off) + (size_t)(action >= 0 ? action : kCassActions) * nch;
    const uint64_t *notab = (const uint64_t *)(img + H->notab_off);
#pragma unroll
    for (int c = 0; c < kCassMaxChunks; c++) ok[c] = (uint32_t)c < nch ? (cnt.n ? notab[c] : ~0ull) : 0;
    if (cnt.n) {  // parts[3] non-empty: the table regexes decide
        const DevDfa *dd = (const DevDfa *)(img + H->dfa_off);
        for (uint32_t d = 0; d < H->ndfa; d++) {
            DfaSink S{img, dd[d], dd[d].start};
            src.emit(S);
            const uint64_t *m = (const uint64_t *)(img + S.D.mask_off) + (size_t)S.st * nch;
#pragma unroll
            for (int c = 0; c < kCassMaxChunks; c++)
                if ((uint32_t)c < nch) ok[c] |= m[c];
        }
        const DevNfaRef *refs = (const DevNfaRef *)(img + H->nfa_off);
        for (uint32_t k = 0; k < H->nnfa; k++) {
            const DevNfaRef r = refs[k];
            NfaSink S{T.nfa_pool, r.nfa, {}};
            nfa_begin(S.R, scratch);
            src.emit(S);
            if (!nfa_end(T.nfa_pool, r.nfa, S.R)) continue;
            const uint64_t *own = (const uint64_t *)(img + r.mask_off);
#pragma unroll
            for (int c = 0; c < kCassMaxChunks; c++)
                if ((uint32_t)c < nch) ok[c] |= own[c];
        }
    }
    *verdict = H->terminal;
#pragma unroll
    for (int c = 0; c < kCassMaxChunks; c++) {
        if ((uint32_t)c >= nch) break;
        const uint64_t hit = ok[c] & act[c];
        if (hit) {
            *verdict = V_ALLOW;
            *rule = ids[c * 64 + __builtin_ctzll(hit)];
            break;
        }
    }
}

// A QUERY / PREPARE frame's query at b (len bytes of buffer), or false.
__device__ __forceinline__ bool cass_request_query(const Batch &B, uint32_t i, uint32_t *ci_out, const uint8_t **b_out,
                                                   uint8_t *op, uint32_t *qn) {
    const uint32_t ci = B.conn_ids[i];
    if (ci >= B.nconns || B.conns[ci].proto != PROTO_CASSANDRA) return false;
    const uint64_t off = B.offs[i];
    const uint32_t len = B.lens[i];
    if (!l7_in_arena(off, len, B.arena_len)) return false;
    const uint8_t *b = B.arena + off;
    CassFrame F;
    if (!cass_frame_of(b, len, &F) || (F.op != 0x07 && F.op != 0x09) || !cass_query_of(b, len, qn)) return false;
    *ci_out = ci;
    *b_out = b;
    *op = F.op;
    return true;
}

// cheap pre-check of a USE: the first token must be "use" (ASCII only: no other rune lowers to u, s or e)
__device__ __forceinline__ bool cass_starts_use(const uint8_t *b, uint32_t qn) {
    uint32_t p = 0;
    while (p < qn) {
        uint32_t w;
        const uint32_t r = nfa_decode(b + 13, p, qn, &w);
        if (!cass_space(r)) break;
        p += w;
    }
    return !(p + 3 > qn || (b[13 + p] | 0x20) != 'u' || (b[14 + p] | 0x20) != 's' || (b[15 + p] | 0x20) != 'e');
}

}  // namespace

// One key per request: (connection << 32 | index) for a USE request, ~0 otherwise.
__global__ __launch_bounds__(kBlock) void cassandra_use_kernel(Batch B, CassTables T, uint64_t *__restrict__ keys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= B.n) return;
    keys[i] = ~0ull;
    uint32_t ci, qn;
    const uint8_t *b;
    uint8_t op;
    if (!cass_request_query(B, i, &ci, &b, &op, &qn) || !cass_starts_use(b, qn)) return;
    const CassQuery Q = cass_parse_query(b + 13, qn, T.lower, T.nlower);
    if (Q.status == CQ_OK && Q.is_use) keys[i] = (uint64_t)ci << 32 | i;
}

// Sessions: the USE keys as above, and in pkeys the same key for every PREPARE
// whose query parses (the statements the commit stashes, whatever their verdict).
__global__ __launch_bounds__(kBlock) void cassandra_marks_kernel(Batch B, CassTables T, uint64_t *__restrict__ keys,
                                                                 uint64_t *__restrict__ pkeys) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= B.n) return;
    keys[i] = ~0ull;
    pkeys[i] = ~0ull;
    uint32_t ci, qn;
    const uint8_t *b;
    uint8_t op;
    if (!cass_request_query(B, i, &ci, &b, &op, &qn)) return;
    if (op != 0x09 && !cass_starts_use(b, qn)) return;
    const CassQuery Q = cass_parse_query(b + 13, qn, T.lower, T.nlower);
    if (Q.status != CQ_OK) return;
    if (Q.is_use) keys[i] = (uint64_t)ci << 32 | i;
    if (op == 0x09) pkeys[i] = (uint64_t)ci << 32 | i;
}

// kSess: SS's tables are read (never written); returns CSS_RESOLVED / CSS_UNPREPARED for an EXECUTE, else -1.
template <bool kSess>
__device__ __forceinline__ int cassandra_one(const Batch &B, const CassTables &T, const uint64_t *__restrict__ use_keys,
                                             uint32_t answer_other, uint32_t i, uint64_t *scratch,
                                             const CassSessions &SS) {
    const uint32_t ci = B.conn_ids[i];
    const DevConn conn = L7_BATCH_CONN(B, ci);
    if (conn.proto != PROTO_CASSANDRA || conn.ruleset < 0 || (uint32_t)conn.ruleset >= T.nrulesets) {
        if (answer_other && !L7_PROTO_OWNED(conn.proto)) {  // no parser: UNSUPPORTED
            B.verdict[i] = V_UNSUPPORTED;
            B.rule[i] = -1;
            B.consumed[i] = 0;
        }
        return -1;
    }
    const uint64_t off = B.offs[i];
    const uint32_t len = B.lens[i];
    uint8_t verdict = V_UNSUPPORTED;
    int32_t rule = -1;
    uint32_t consumed = 0;
    int stat = -1;
    if (l7_in_arena(off, len, B.arena_len)) {
        const uint8_t *b = B.arena + off;
        const uint8_t *img = T.images + T.rulesets[conn.ruleset].image_off;
        const CassImgHeader *H = (const CassImgHeader *)img;
        const int32_t *ids = (const int32_t *)(img + H->rule_off);
        CassFrame F;
        bool query_like = false;
        CassQuery Q{};
        uint32_t qn = 0;
        if (!cass_frame_of(b, len, &F)) {
            verdict = F.verdict;
            consumed = F.consumed;
        } else if (F.op == 0x07 || F.op == 0x09) {
            if (!cass_query_of(b, len, &qn)) {
                verdict = V_PARSE_ERROR;  // slice bounds panic
            } else {
                Q = cass_parse_query(b + 13, qn, T.lower, T.nlower);
                if (Q.status == CQ_PANIC) verdict = V_PARSE_ERROR;
                else if (Q.status == CQ_INVALID) { verdict = V_PARSE_ERROR; consumed = 2; }
                else query_like = true;
            }
        } else if (F.op == 0x0D) {
            verdict = V_PARSE_ERROR;  // Uint16(data[10:11]) panics
        } else if (F.op == 0x0A) {
            if (len < 11 || 11u + cass_be16(b + 9) > len) {
                verdict = V_PARSE_ERROR;  // panic (capacity-bounded, as above)
            } else {
                verdict = V_PARSE_ERROR;  // no prepared statement under this id
                consumed = 2;
                if constexpr (kSess) {
                    stat = CSS_UNPREPARED;
                    const uint32_t il = cass_be16(b + 9);
                    const CassEntry *e = nullptr;
                    if (il <= kCassIdMax && ci < SS.nslots)  // (a longer id is never bound)
                        e = cass_find(SS.by_id, SS.mask, sess_claim_of(ci, SS.slots[ci].gen), ci, b + 11, il);
                    if (e && e->action != kCassTomb) {
                        stat = CSS_RESOLVED;
                        consumed = 0;
                        if (e->path_len == kCassOver) {
                            verdict = V_UNSUPPORTED;  // the statement's table did not fit its entry
                        } else {
                            cass_match(img, H, T, e->action, StoredSrc{e->path, e->path_len}, scratch, &verdict, &rule);
                            consumed = F.fl;
                        }
                    }
                }
            }
        } else {  // "/" + opcode name: every rule matches
            verdict = H->nrules ? V_ALLOW : H->terminal;
            rule = H->nrules ? ids[0] : -1;
            consumed = F.fl;
        }
        if (query_like) {
            // keyspace: the last USE on this connection before request i
            const uint8_t *ks = nullptr;
            CassQuery K{};
            bool ks_over = false;
            if (Q.seg3 == S3_KS_TABLE) {
                const int64_t best = cass_last_before(use_keys, B.n, ci, i);
                if (best >= 0) {
                    const uint8_t *bj = B.arena + B.offs[best];
                    const uint32_t qj = cass_be32(bj + 9);
                    K = cass_parse_query(bj + 13, qj, T.lower, T.nlower);
                    ks = bj + 13;
                } else if constexpr (kSess) {  // none in this batch: the one the session holds
                    if (ci < SS.nslots) {
                        const CassSlot *sl = &SS.slots[ci];
                        ks_over = sl->ks_len == kCassOver;
                        if (!ks_over) {
                            ks = sl->ks;
                            K.te = sl->ks_len;
                            K.fc = sl->ks_fc;
                        }
                    }
                }
            }
            if (!ks_over) {
                cass_match(img, H, T, Q.action, QuerySrc{Q, b + 13, ks, K, T.lower, T.nlower}, scratch, &verdict, &rule);
                consumed = F.fl;
            }
        }
    }
    B.verdict[i] = verdict;
    B.rule[i] = rule;
    B.consumed[i] = consumed;
    return stat;
}

// grid-stride: a launch with large NFAs has as many lanes as it has scratch for
__global__ __launch_bounds__(kBlock) void cassandra_classify_kernel(Batch B, CassTables T,
                                                                    const uint64_t *__restrict__ use_keys,
                                                                    uint32_t answer_other) {
    uint64_t *scratch = l7_nfa_lane_scratch(T.nfa_scratch, T.nfa_lane_words);
    const CassSessions none{};
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < B.n; i += gridDim.x * kBlock)
        cassandra_one<false>(B, T, use_keys, answer_other, i, scratch, none);
}

// The same with sessions; the EXECUTEs resolved and refused are counted per
// wave (one atomic each per wave and launch).
__global__ __launch_bounds__(kBlock) void cassandra_session_classify_kernel(Batch B, CassTables T,
                                                                            const uint64_t *__restrict__ use_keys,
                                                                            uint32_t answer_other, CassSessions SS) {
    uint64_t *scratch = l7_nfa_lane_scratch(T.nfa_scratch, T.nfa_lane_words);
    uint32_t resolved = 0, unprepared = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < B.n; i += gridDim.x * kBlock) {
        const int st = cassandra_one<true>(B, T, use_keys, answer_other, i, scratch, SS);
        resolved += st == CSS_RESOLVED;
        unprepared += st == CSS_UNPREPARED;
    }
    for (int d = 32; d > 0; d >>= 1) {
        resolved += __shfl_xor(resolved, d);
        unprepared += __shfl_xor(unprepared, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (resolved) atomicAdd(&SS.stats[CSS_RESOLVED], (unsigned long long)resolved);
        if (unprepared) atomicAdd(&SS.stats[CSS_UNPREPARED], (unsigned long long)unprepared);
    }
}

// Scratch bytes LaunchCassandraClassify needs for a batch of n requests
// (sessions: two more key arrays, the PREPARE marks and their sorted copy).
size_t CassandraScratchBytes(uint32_t n, bool sessions) {
    size_t temp = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, temp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, 64) !=
        hipSuccess)
        return 0;
    return CassandraLayout(n, sessions, temp).total;
}

// scratch: CassandraScratchBytes(B.n) bytes (256-byte aligned)
// nfa_lanes: lanes T.nfa_scratch holds (when it is set)
hipError_t LaunchCassandraClassify(const Batch &B, const CassTables &T, void *scratch, size_t scratch_bytes,
                                   bool answer_other, uint32_t nfa_lanes, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const CassandraScratch L = CassandraLayout(B.n, false, 0);
    if (scratch_bytes < L.temp) return hipErrorInvalidValue;
    uint8_t *base = (uint8_t *)scratch;
    uint64_t *keys = (uint64_t *)(base + L.keys), *sorted = (uint64_t *)(base + L.sorted);
    void *temp = base + L.temp;
    size_t temp_bytes = scratch_bytes - L.temp;
    const dim3 grid((B.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(cassandra_use_kernel, grid, dim3(kBlock), 0, stream, B, T, keys);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    // connection ids are < 2^32 and request indices < 2^32: all 64 bits
    rc = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, sorted, (int)B.n, 0, 64, stream);
    if (rc != hipSuccess) return rc;
    dim3 cgrid = grid;
    if (T.nfa_scratch) cgrid.x = max(1u, min(cgrid.x, nfa_lanes / kBlock));
    hipLaunchKernelGGL(cassandra_classify_kernel, cgrid, dim3(kBlock), 0, stream, B, T, sorted, answer_other ? 1u : 0u);
    return hipGetLastError();
}

// With sessions: marks, both sorts, the read-only classifier, then the commit
// of the batch's PREPAREs and keyspaces (separate launches: the kernel
// boundaries order the tables' readers and writers).
// scratch: CassandraScratchBytes(B.n, true) bytes
// commit: false leaves the commit launches to the caller (the logged sequence below)
static hipError_t SessionClassify(const Batch &B, const CassTables &T, const CassSessions &SS, void *scratch,
                                  size_t scratch_bytes, bool answer_other, uint32_t nfa_lanes, hipStream_t stream,
                                  bool commit) {
    if (B.n == 0) return hipSuccess;
    const CassandraScratch L = CassandraLayout(B.n, true, 0);
    if (scratch_bytes < L.temp) return hipErrorInvalidValue;
    uint8_t *base = (uint8_t *)scratch;
    uint64_t *keys = (uint64_t *)(base + L.keys), *sorted = (uint64_t *)(base + L.sorted);
    uint64_t *pkeys = (uint64_t *)(base + L.pkeys), *psorted = (uint64_t *)(base + L.psorted);
    void *temp = base + L.temp;
    size_t temp_bytes = scratch_bytes - L.temp;
    const dim3 grid((B.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(cassandra_marks_kernel, grid, dim3(kBlock), 0, stream, B, T, keys, pkeys);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    rc = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, sorted, (int)B.n, 0, 64, stream);
    if (rc != hipSuccess) return rc;
    rc = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, pkeys, psorted, (int)B.n, 0, 64, stream);
    if (rc != hipSuccess) return rc;
    dim3 cgrid = grid;
    if (T.nfa_scratch) cgrid.x = max(1u, min(cgrid.x, nfa_lanes / kBlock));
    hipLaunchKernelGGL(cassandra_session_classify_kernel, cgrid, dim3(kBlock), 0, stream, B, T, sorted,
                       answer_other ? 1u : 0u, SS);
    rc = hipGetLastError();
    if (rc != hipSuccess || !commit) return rc;
    return LaunchCassandraCommit(B, T, SS, sorted, psorted, stream);
}

hipError_t LaunchCassandraSessionClassify(const Batch &B, const CassTables &T, const CassSessions &SS, void *scratch,
                                          size_t scratch_bytes, bool answer_other, uint32_t nfa_lanes,
                                          hipStream_t stream) {
    return SessionClassify(B, T, SS, scratch, scratch_bytes, answer_other, nfa_lanes, stream, true);
}

// l7g_classify_logged_all's sequence: the same launches, with the access-log
// post-pass between the read-only classifier and the commit, where the session
// tables still stand as the classifier read them.
hipError_t LaunchCassandraSessionClassifyLogged(const Batch &B, const CassTables &T, const CassSessions &SS,
                                                void *scratch, size_t scratch_bytes, bool answer_other,
                                                uint32_t nfa_lanes, const LogOut &L, const LogText &X,
                                                hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    hipError_t rc = SessionClassify(B, T, SS, scratch, scratch_bytes, answer_other, nfa_lanes, stream, false);
    if (rc != hipSuccess) return rc;
    const CassandraScratch at = CassandraLayout(B.n, true, 0);
    const uint64_t *sorted = (const uint64_t *)((uint8_t *)scratch + at.sorted);
    const uint64_t *psorted = (const uint64_t *)((uint8_t *)scratch + at.psorted);
    rc = LaunchGenericLog(B, L, X, T, sorted, SS, stream);
    if (rc != hipSuccess) return rc;
    return LaunchCassandraCommit(B, T, SS, sorted, psorted, stream);
}

// The sorted USE keys the launchers above left in `scratch` for a batch of n requests.
const uint64_t *CassandraSortedUseKeys(const void *scratch, uint32_t n) {
    // (the sorted USE keys lie at one offset with sessions and without)
    return (const uint64_t *)((const uint8_t *)scratch + CassandraLayout(n, false, 0).sorted);
}

}  // namespace l7

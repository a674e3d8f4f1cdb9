// Access-log records of memcached, r2d2 and cassandra requests on gfx950
// (product code): the post-pass of l7g_classify_logged_all, launched once per
// call on the call's stream, after http_log_kernel (which gives every request
// that is neither HTTP nor Kafka kind 0) and after the classifiers -- with
// cassandra sessions on, between the session classifier and that call's
// commit launches, so that an EXECUTE and the slot's keyspace are read as the
// classifier read them.
//
// It reads verdict[] and handles only the requests of those three protocols
// that a classifier answered ALLOW or DENY: their framing is known to hold (a
// memcached or r2d2 first line ends in "\r\n" inside the request, a memcached
// command has the tokens its key set needs, a binary header is complete, a
// cassandra frame is whole and its query parses), so nothing is validated
// again.  The fields are those of the LogEntry_GenericL7 the proxylib parsers
// log (include/l7gpu.h has the layout and the reference lines).
//
// One lane per request, as in the three classifiers: the first line of a
// memcached or r2d2 request is tens of bytes (one to four 16-byte chunks), so
// a lane team per request would leave most of its lanes without a chunk; a
// lane walks its line once through a 16-byte aligned register window
// (global_load_dwordx4), never outside [first byte & ~15, (last byte + 16) &
// ~15).  A cassandra lane parses its query with kernels/cass_parse.h, byte
// loads inside its request (and, for an undotted table, inside the USE request
// that set the keyspace, as the classifier reads it), and streams the lowered
// table into its text row, a dword at a time where the row's address allows.
// Plain vector stores, no atomics, no LDS, no scratch of its own: the sorted
// USE keys are the ones the cassandra classifier has just built.
#include <hip/hip_runtime.h>

#include "../device_tables.h"
#include "cass_parse.h"
#include "cass_session.h"
#include "gmem.h"
#include "launch.h"
#include "text_bytes.h"

namespace l7 {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNoTok = ~0u;

struct Rec {
    uint32_t w[8];
};

#define GL_CMD(lit) (clen == sizeof(lit) - 1 && c0 == pk4(lit, sizeof(lit) - 1, 0) && c1 == pk4(lit, sizeof(lit) - 1, 1))

// memcached text (text/parser.go:98-171): tokens of bytes.Fields(first line),
// the command and the key tokens its class takes.
__device__ __forceinline__ void mc_text_log(const uint8_t *b, uint32_t len, uint32_t i, const LogOut &L, Rec &R) {
    Reader W{b, ~0ull, 0, 0, 0, 0};
    uint32_t nt = 0, start = 0, cmd_off = 0, cmd_len = 0;
    uint32_t first = kNoTok, maxk = 0;  // key tokens: [first, first + maxk) of the line's
    bool in_tok = false, found = false;
    for (uint32_t p = 0; p < len;) {
        const uint32_t c = rd(W, p);
        const bool end = c == '\r' && p + 1 < len && rd(W, p + 1) == '\n';
        // a separator (text_bytes.h): the bytes after a lead byte are read where the request holds them
        uint32_t sw = 0;
        if (c < 0x80) sw = ws_rune_len(c, 0, 0, 1);
        else if (ws_lead_len(c) == 2) {
            if (p + 1 < len) sw = ws_rune_len(c, rd(W, p + 1), 0, 2);
        } else if (ws_lead_len(c) == 3 && p + 2 < len) {
            const uint32_t c1 = rd(W, p + 1), c2 = rd(W, p + 2);
            sw = ws_rune_len(c, c1, c2, 3);
        }
        const uint32_t w = sw ? sw : 1u;
        const bool sp = end || sw;
        if (sp && in_tok) {  // token nt is [start, p)
            in_tok = false;
            const uint32_t k = nt++;
            if (k == 0) {
                cmd_off = start;
                const uint32_t clen = cmd_len = p - start;
                uint32_t c0 = 0, c1 = 0;
                for (uint32_t j = 0; j < clen && j < 8; j++) {
                    const uint32_t x = rd(W, start + j);
                    if (j < 4) c0 |= x << (8 * j);
                    else c1 |= x << (8 * (j - 4));
                }
                const uint32_t pre = c0 & 0xFFFFFFu;
                if (clen >= 3 && pre == pk4("get", 3, 0)) { first = 1; maxk = ~0u; }
                else if (clen >= 3 && pre == pk4("gat", 3, 0)) { first = 2; maxk = ~0u; }
                else if (GL_CMD("set") || GL_CMD("add") || GL_CMD("replace") || GL_CMD("append") || GL_CMD("prepend") ||
                         GL_CMD("cas") || GL_CMD("delete") || GL_CMD("incr") || GL_CMD("decr") || GL_CMD("touch")) {
                    first = 1;
                    maxk = 1;
                }
            } else if (k >= first && k - first < maxk && k - first < L.stride) {
                L.topics[(size_t)i * L.stride + (k - first)] = LogSpan{start, p - start};
            }
        } else if (!sp && !in_tok) {
            in_tok = true;
            start = p;
        }
        if (end) { found = true; break; }
        p += w;
    }
    if (!found || nt == 0) return;  // (no classifier answers such a request ALLOW or DENY)
    uint32_t nkeys = first != kNoTok && nt > first ? nt - first : 0;
    if (nkeys > maxk) nkeys = maxk;
    R.w[0] = LOG_MC_TEXT | (nkeys > L.stride ? 1u << 8 : 0u);
    R.w[1] = cmd_off;
    R.w[2] = cmd_len;
    R.w[3] = nkeys;
}
#undef GL_CMD

// memcached binary (binary/parser.go:78-105): the header alone
__device__ __forceinline__ void mc_binary_log(const uint8_t *b, uint32_t len, Rec &R) {
    if (len < 24) return;
    Reader W{b, ~0ull, 0, 0, 0, 0};
    const uint32_t opcode = rd(W, 1);
    const uint32_t keylen = rd(W, 2) << 8 | rd(W, 3);
    const uint32_t extras = rd(W, 4);
    R.w[0] = LOG_MC_BINARY | opcode << 16;
    R.w[1] = keylen ? 24 + extras : 0;
    R.w[2] = keylen;
}

// r2d2 (r2d2parser.go:165-205): the line up to the first "\r\n", split on single spaces
__device__ __forceinline__ void r2d2_log(const uint8_t *b, uint32_t len, Rec &R) {
    Reader W{b, ~0ull, 0, 0, 0, 0};
    uint32_t lf = 0, sp1 = 0, nsp = 0, prev = 0x100;
    bool found = false;
    for (uint32_t p = 0; p < len; p++) {
        const uint32_t c = rd(W, p);
        if (prev == '\r' && c == '\n') { lf = p - 1; found = true; break; }
        if (prev == ' ') { if (nsp++ == 0) sp1 = p - 1; }
        prev = c;
    }
    if (!found) return;
    R.w[0] = LOG_R2D2;
    R.w[1] = nsp ? sp1 : lf;
    R.w[2] = nsp == 1 ? sp1 + 1 : 0;
    R.w[3] = nsp == 1 ? lf - sp1 - 1 : 0;
    R.w[4] = nsp + 1;
}

// parts[3] of a path into a text row: n counts every byte, the first `cap` are
// stored -- four at a time where they fill an aligned dword of the row.
struct TextSink {
    uint8_t *row;
    uint32_t cap, n, acc, cnt;
    __device__ __forceinline__ void flush(uint32_t end) {  // the cnt pending bytes are row[end - cnt, end)
        if (cnt == 4) {
            *reinterpret_cast<uint32_t *>(row + end - 4) = acc;  // (flushed at every aligned end: the start is aligned)
        } else {
            for (uint32_t k = 0; k < cnt; k++) row[end - cnt + k] = (uint8_t)(acc >> (8 * k));
        }
        acc = 0;
        cnt = 0;
    }
    __device__ __forceinline__ void raw(uint32_t c) {
        if (n < cap) {
            acc |= (c & 0xFFu) << (8 * cnt);
            cnt++;
            if ((((uintptr_t)row + n + 1) & 3) == 0) flush(n + 1);
        }
        n++;
    }
    __device__ __forceinline__ void rune(uint32_t r) {
        uint8_t e[4];
        const uint32_t k = cass_encode(r, e);
        for (uint32_t j = 0; j < k; j++) raw(e[j]);
    }
    __device__ __forceinline__ void finish() {
        if (cnt) flush(n < cap ? n : cap);
    }
};

// cassandra (cassandraparser.go:212-244, parseQuery :368-469)
__device__ __forceinline__ void cass_log(const Batch &B, const uint8_t *b, uint32_t len, uint32_t i, uint32_t ci,
                                         const LogText &X, const CassTables &T, const uint64_t *__restrict__ use_keys,
                                         const CassSessions &SS, Rec &R) {
    CassFrame F;
    if (!cass_frame_of(b, len, &F)) return;
    TextSink sink{X.text + (size_t)i * X.stride, X.stride, 0, 0, 0};
    int32_t action = -1;
    uint32_t flags = 0, keyword = 0, word_off = 0, word_len = 0;
    if (F.op == 0x07 || F.op == 0x09) {
        uint32_t qn = 0;
        if (!cass_query_of(b, len, &qn)) return;
        const uint8_t *q = b + 13;
        const CassQuery Q = cass_parse_query(q, qn, T.lower, T.nlower);
        if (Q.status != CQ_OK) return;
        action = Q.action;
        if (action < 0) {  // "<kw>-<fields[1]>", outside queryActionMap: the caller spells it
            keyword = Q.kw == CW_ALTER ? 0 : Q.kw == CW_CREATE ? 1 : Q.kw == CW_DROP ? 2 : Q.kw == CW_TRUNCATE ? 3 : 4;
            word_off = 13 + Q.f1s;
            word_len = Q.f1e - Q.f1s;
        }
        // a '/' in fields[1] (S3_F1) always leaves a path of five or more parts: no entry
        bool slash = Q.seg3 == S3_F1;
        if (Q.seg3 == S3_TABLE) {
            slash = cass_emit(q, Q.ts, Q.te, Q.fc, T.lower, T.nlower, sink);
        } else if (Q.seg3 == S3_KS_TABLE) {
            // the keyspace: the last USE on this connection before request i, else the session's
            const int64_t best = cass_last_before(use_keys, B.n, ci, i);
            if (best >= 0) {
                const uint8_t *bj = B.arena + B.offs[best];
                const CassQuery K = cass_parse_query(bj + 13, cass_be32(bj + 9), T.lower, T.nlower);
                slash = cass_emit(bj + 13, K.ts, K.te, K.fc, T.lower, T.nlower, sink);
            } else if (SS.slots && ci < SS.nslots) {
                const CassSlot *sl = &SS.slots[ci];
                if (sl->ks_len == kCassOver) return;  // (answered UNSUPPORTED)
                slash = cass_emit(sl->ks, 0, sl->ks_len, sl->ks_fc, T.lower, T.nlower, sink);
            }
            if (!slash) {
                sink.raw('.');
                slash = cass_emit(q, Q.ts, Q.te, Q.fc, T.lower, T.nlower, sink);
            }
        }
        if (!slash) flags |= 2;
    } else if (F.op == 0x0A && SS.by_id) {  // EXECUTE: the statement its id was bound to before this call
        if (len < 11) return;
        const uint32_t il = cass_be16(b + 9);
        if (il > kCassIdMax || 11u + il > len || ci >= SS.nslots) return;
        const CassEntry *e = cass_find(SS.by_id, SS.mask, sess_claim_of(ci, SS.slots[ci].gen), ci, b + 11, il);
        if (!e || e->action == kCassTomb || e->path_len == kCassOver) return;
        action = e->action;
        if (action < 0) flags |= 4;  // a statement keeps no action word
        for (uint32_t k = 0; k < e->path_len; k++) sink.raw(e->path[k]);
        flags |= 2;
    }
    sink.finish();
    if (sink.n > X.stride) flags |= 1;
    R.w[0] = LOG_CASSANDRA | flags << 8 | ((uint32_t)action & 0xFFFFu) << 16;
    R.w[1] = sink.n;
    R.w[2] = keyword;
    R.w[3] = word_off;
    R.w[4] = word_len;
}

}  // namespace

// use_keys: the batch's sorted USE keys (null: no cassandra classifier ran; its requests have no ALLOW / DENY)
__global__ __launch_bounds__(kBlock) void generic_log_kernel(Batch B, LogOut L, LogText X, CassTables T,
                                                             const uint64_t *__restrict__ use_keys, CassSessions SS) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= B.n) return;
    const uint32_t i = (uint32_t)gi;
    const uint32_t ci = B.conn_ids[i];
    if (ci >= B.nconns) return;
    const DevConn conn = B.conns[ci];
    if (conn.proto != PROTO_MEMCACHE && conn.proto != PROTO_R2D2 && conn.proto != PROTO_CASSANDRA) return;
    const uint8_t v = B.verdict[i];
    if (v != V_ALLOW && v != V_DENY) return;
    const uint64_t off = B.offs[i];
    const uint32_t len = B.lens[i];
    if (len == 0 || !l7_in_arena(off, len, B.arena_len)) return;
    const uint8_t *b = B.arena + off;
    Rec R{};
    if (conn.proto == PROTO_MEMCACHE) {
        // the parser, as the classifier picks it: the connection's flags, else the first byte
        uint32_t mode = conn.flags & 3;
        if (mode == 0) mode = b[0] >= 0x80 ? 2 : 1;
        if (mode == 2) mc_binary_log(b, len, R);
        else mc_text_log(b, len, i, L, R);
    } else if (conn.proto == PROTO_R2D2) {
        r2d2_log(b, len, R);
    } else if (use_keys) {
        cass_log(B, b, len, i, ci, X, T, use_keys, SS, R);
    }
    if (R.w[0] == LOG_NONE) return;  // (kind 0 stands, from http_log_kernel)
    uint4 *o = reinterpret_cast<uint4 *>(L.rec + i);
    o[0] = make_uint4(R.w[0], R.w[1], R.w[2], R.w[3]);
    o[1] = make_uint4(R.w[4], 0, 0, 0);
}

hipError_t LaunchGenericLog(const Batch &B, const LogOut &L, const LogText &X, const CassTables &T,
                            const uint64_t *use_keys, const CassSessions &SS, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)B.n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(generic_log_kernel, dim3(blocks), dim3(kBlock), 0, stream, B, L, X, T, use_keys, SS);
    return hipGetLastError();
}

}  // namespace l7

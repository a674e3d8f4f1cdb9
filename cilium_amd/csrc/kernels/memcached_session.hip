// Memcached sessions on gfx950 (product code): the reply queue of
// proxylib/memcached/text/parser.go and the request / reply counters and
// inject queue of proxylib/memcached/binary/parser.go for a batch, resident in
// HBM (device_tables.h McSessSlot / McSessIntent).
//
// l7g_mc_forward (the request direction, after l7g_classify), on the caller's
// stream:
//   mcsess_keys_kernel     one key (connection << 32 | index) per participating
//     request, a key past every connection for the others; the same lane walks
//     its request's first line once and leaves the request's info byte;
//   a hipcub radix sort    (bits 0 .. 32 + those of a connection index);
//   mcsess_heads_kernel    the first key of every connection's segment finds
//     the segment's end (a binary search) and the parser in force: the slot's,
//     else that of this first request;
//   mcsess_elems_kernel    one scan element per sorted request (mc_session.h);
//   a hipcub inclusive scan whose operator composes adjacent spans and forgets
//     at a segment's first request;
//   mcsess_resolve_kernel  one lane per sorted request: its act, and its ring
//     entry at (head + count + rank) & (cap - 1);
//   mcsess_advance_kernel  one lane per connection advances the slot once, from
//     the scan's value at the segment's end.
// l7g_mc_replies (the reply direction): mcsess_replies_kernel, one wave per
// stream, runs the op loop of proxylib/proxylib/connection.go:118-174 over its
// stream: the lanes find a line's "\r\n" and a retrieval's "\r\nEND\r\n" 64
// bytes at a step by ballot, walk the line's first token and the queue head in
// step, and lane 0 writes the ops.  A binary stream is a hop over 24-byte
// headers, the lanes in step.
//
// The slot and the ring are read by resolve and written by advance (the slot)
// and resolve (ring entries past the queued ones): kernel boundaries on the
// caller's stream are the only ordering, there is no flag between workgroups.
// Every grid is capped at kSessMaxBlocks workgroups and strides above that; loops
// are uniform per wave so that the statistics take one atomic per wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "launch.h"
#include "mc_session.h"
#include "sess_common.h"

namespace l7 {

namespace {

constexpr int kBlock = kSessBlock;

struct McSeg {
    uint32_t start, end, kind, pad;
};
static_assert(sizeof(McSeg) == kMcSegBytes && sizeof(McScan) == kMcScanBytes,
              "seg[], el[] and sc[] as sess_scratch.h lays them out");

// replies - requests of a binary slot; the immediate injects of a segment are
// the DENYs from position g + 1 (1-based) up to the next ALLOW, none for g < 0
__device__ __forceinline__ int64_t mc_gap(const McSessSlot &sl) { return (int64_t)(int32_t)(sl.replies - sl.requests); }

}  // namespace

__global__ __launch_bounds__(kBlock) void mcsess_keys_kernel(McSessBatch B, McSessions S,
                                                             const uint8_t *__restrict__ verdict,
                                                             uint64_t *__restrict__ keys, uint8_t *__restrict__ info,
                                                             uint8_t *__restrict__ act) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < B.n; i += (uint64_t)gridDim.x * kBlock) {
        const uint8_t v = verdict[i];
        uint32_t bits = 0;
        if ((v == V_ALLOW || v == V_DENY) && B.lens[i] != 0 && sess_item(B, S.nslots, PROTO_MEMCACHE, (uint32_t)i)) {
            const uint8_t *b = B.arena + B.offs[i];
            McReader W{b, ~0ull, 0, 0};
            // the parser, as the classifier picks it: the connection's flags, else the first byte
            uint32_t mode = B.conns[B.conn_ids[i]].flags & 3;
            if (mode == 0) mode = mcs_rd(W, 0) >= 0x80 ? MCK_BINARY : MCK_TEXT;
            if (mode == MCK_BINARY) bits = MCI_VALID | MCI_BINARY;
            else bits = mcs_text_request(mcs_line(W, 0, B.lens[i]));
            if (bits && v == V_DENY) bits |= MCI_DENY;
        }
        keys[i] = sess_key(bits ? B.conn_ids[i] : B.nconns, (uint32_t)i);
        info[i] = (uint8_t)bits;
        if (!bits) act[i] = 0;
    }
}

// seg[connection] = (segment start and end in sorted, the parser in force)
__global__ __launch_bounds__(kBlock) void mcsess_heads_kernel(McSessBatch B, McSessions S,
                                                              const uint64_t *__restrict__ sorted,
                                                              const uint8_t *__restrict__ info,
                                                              McSeg *__restrict__ seg) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < B.n; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t ci = key_conn(sorted[j]);
        if (ci >= B.nconns || !segment_head(sorted, j)) continue;
        const uint64_t end = segment_end(sorted, j, B.n, ci);
        uint32_t kind = S.slots[ci].kind;
        if (kind == MCK_NONE) kind = (info[key_index(sorted[j])] & MCI_BINARY) ? MCK_BINARY : MCK_TEXT;
        seg[ci] = McSeg{(uint32_t)j, (uint32_t)end, kind, 0};
    }
}

__global__ __launch_bounds__(kBlock) void mcsess_elems_kernel(McSessBatch B, const uint64_t *__restrict__ sorted,
                                                              const uint8_t *__restrict__ info,
                                                              const McSeg *__restrict__ seg, McScan *__restrict__ el) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < B.n; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t ci = key_conn(sorted[j]);
        McScan x{MCS_HEAD, 0, 0, 0};
        if (ci < B.nconns) {
            const McSeg sg = seg[ci];
            const uint32_t in = info[key_index(sorted[j])];
            const bool bin = sg.kind == MCK_BINARY, deny = (in & MCI_DENY) != 0;
            x.f = ((uint32_t)j == sg.start ? MCS_HEAD : 0u) | (bin ? MCS_BIN : 0u);
            if (bin == ((in & MCI_BINARY) != 0)) {  // (a request of the other parser changes nothing)
                if (bin) {
                    x.c = 1;
                    x.a = deny ? 0 : 1;
                    x.d = deny ? 1 : 0;
                } else {
                    if (in & MCI_WATCH) x.f |= MCS_WATCH;
                    if (!(in & MCI_NOREPLY)) {
                        x.c = 1;
                        if (deny) x.a = 1; else x.f |= MCS_E;
                    }
                }
            }
        }
        el[j] = x;
    }
}

__global__ __launch_bounds__(kBlock) void mcsess_resolve_kernel(McSessBatch B, McSessions S,
                                                                const uint64_t *__restrict__ sorted,
                                                                const uint8_t *__restrict__ info,
                                                                const McSeg *__restrict__ seg,
                                                                const McScan *__restrict__ sc,
                                                                const uint64_t *__restrict__ tag,
                                                                uint8_t *__restrict__ act) {
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < B.n; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t j = base + threadIdx.x;
        const uint32_t ci = j < B.n ? key_conn(sorted[j]) : B.nconns;
        bool full = false, mismatch = false, now = false;
        if (ci < B.nconns) {
            const uint32_t i = key_index(sorted[j]);
            const uint32_t in = info[i];
            const McSeg sg = seg[ci];
            const McSessSlot sl = S.slots[ci];
            const bool bin = sg.kind == MCK_BINARY, deny = (in & MCI_DENY) != 0;
            const McScan inc = sc[j];
            const McScan ex = (uint32_t)j == sg.start ? McScan{0, 0, 0, 0} : sc[j - 1];
            uint8_t a;
            if (bin != ((in & MCI_BINARY) != 0)) {
                a = 7;
                mismatch = true;
            } else if (bin) {
                const int64_t g = mc_gap(sl);
                now = deny && g >= 0 && (int64_t)inc.c > g && (int64_t)inc.a <= g;
                a = !deny ? 1 : now ? 3 : 4;
            } else if (in & MCI_NOREPLY) {
                a = deny ? 5 : 2;
            } else {
                // the queue is not empty here: it was not before the call, or an earlier ALLOW of the call pushed
                const bool queued = sl.count > 0 || (ex.f & MCS_E);
                if (deny && !queued) {
                    a = 3;
                    now = true;
                } else {
                    // the pushes before this one: every reply owed (from the first ALLOW on, on an empty queue)
                    const uint32_t rank = sl.count > 0 ? ex.c : (ex.f & MCS_E) ? ex.c - ex.a : 0u;
                    if ((uint64_t)sl.count + rank < S.cap) {
                        McSessIntent *q = &S.ring[(size_t)ci * S.cap + ((sl.head + sl.count + rank) & (S.cap - 1))];
                        // one 16-byte store: the tag, then class and denied bit
                        *reinterpret_cast<uint4 *>(q) =
                            make_uint4((uint32_t)(tag ? tag[i] : 0), (uint32_t)((tag ? tag[i] : 0) >> 32),
                                       (in & MCI_CLS) | (deny ? 1u << 8 : 0u), 0);
                        a = deny ? 4 : 1;
                    } else {
                        a = 6;
                        full = true;
                    }
                }
            }
            act[i] = a;
        }
        wave_count(&S.stats[MSS_FULL], full);
        wave_count(&S.stats[MSS_MISMATCH], mismatch);
        wave_count(&S.stats[MSS_INJECT_NOW], now);
    }
}

// The slot after the segment, once per connection.
__global__ __launch_bounds__(kBlock) void mcsess_advance_kernel(McSessBatch B, McSessions S,
                                                                const uint64_t *__restrict__ sorted,
                                                                const McSeg *__restrict__ seg,
                                                                const McScan *__restrict__ sc) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < B.n; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t ci = key_conn(sorted[j]);
        if (ci >= B.nconns || !segment_head(sorted, j, ci)) continue;
        const McSeg sg = seg[ci];
        const McScan tot = sc[sg.end - 1];
        McSessSlot sl = S.slots[ci];
        sl.kind = (uint8_t)sg.kind;
        if (sg.kind == MCK_TEXT) {
            const uint32_t pushes = sl.count > 0 ? tot.c : (tot.f & MCS_E) ? tot.c - tot.a : 0u;
            const uint32_t room = S.cap - sl.count;
            sl.count += pushes < room ? pushes : room;
            if (tot.f & MCS_WATCH) sl.watching = 1;
        } else {
            const int64_t g = mc_gap(sl);
            // the ALLOW that ends the run of immediate injects: the first position whose last ALLOW is past g
            uint32_t lo = sg.start, hi = sg.end;
            while (lo < hi) {
                const uint32_t m = lo + (hi - lo) / 2;
                if ((int64_t)sc[m].a > g) hi = m; else lo = m + 1;
            }
            const int64_t stop = lo < sg.end ? (int64_t)sc[lo].a : (int64_t)tot.c + 1;
            const int64_t imm = g >= 0 && stop - 1 > g ? stop - 1 - g : 0;
            if (sl.bstate == MCB_EMPTY && tot.d) {
                // the first DENY of the connection's life heads injectQueue from now on
                lo = sg.start, hi = sg.end;
                while (lo < hi) {
                    const uint32_t m = lo + (hi - lo) / 2;
                    if (sc[m].d) hi = m; else lo = m + 1;
                }
                const uint32_t i = key_index(sorted[lo]);
                const bool now = g >= 0 && (int64_t)tot.d > g && (int64_t)sc[lo].a <= g;
                sl.bstate = now ? MCB_BLOCKED : MCB_ARMED;
                sl.armed_id = sl.requests + tot.d;
                sl.armed_magic = (uint8_t)(B.arena[B.offs[i]] | 0x81);
            }
            sl.requests += tot.c;
            sl.replies += (uint32_t)imm;
        }
        S.slots[ci] = sl;
    }
}

namespace {

// One stream's run; every lane of its wave holds the same values.
struct ReplyRun {
    uint32_t nops, result;
    uint64_t taken;
    uint32_t inj, passed;
};

__device__ __forceinline__ void put_op(const McReplyOut &O, uint64_t s, ReplyRun &R, uint32_t kind, uint32_t n,
                                       uint64_t aux) {
    const uint64_t at = s * O.max_ops + R.nops++;
    if (__lane_id() == 0) {
        O.op_kind[at] = (uint8_t)kind;
        O.op_n[at] = n;
        if (O.op_aux) O.op_aux[at] = aux;
    }
}

enum : uint32_t { OP_MORE = 0, OP_PASS = 1, OP_INJECT = 3, OP_ERROR = 4 };  // FILTEROP_*

// text/parser.go OnData(reply) under the op loop
__device__ __forceinline__ void text_replies(const McSessions &S, uint32_t ci, McSessSlot &sl, const uint8_t *b,
                                             uint64_t len, const McReplyOut &O, uint64_t s, ReplyRun &R) {
    const McSessIntent *ring = S.ring + (size_t)ci * S.cap;
    const uint32_t mask = S.cap - 1;
    McReader W{b, ~0ull, 0, 0};
    uint64_t pos = 0;
    while (R.nops < O.max_ops) {
        uint32_t k = 0;  // injectFromQueue: the denied intents at the head
        while (k < sl.count && ring[(sl.head + k) & mask].denied) k++;
        if (k) {
            sl.head = (sl.head + k) & mask;
            sl.count -= k;
            R.inj += k;
            put_op(O, s, R, OP_INJECT, k * kMcDeniedTextLen, 0);
            continue;
        }
        if (pos >= len) return;  // NOP
        const uint64_t lf = mcs_wave_crlf(b, pos, len);
        if (lf == len) {
            put_op(O, s, R, OP_MORE, b[len - 1] == '\r' ? 1 : 2, 0);
            return;
        }
        if (sl.count == 0) { R.result = 1; return; }  // replyQueue[0] of an empty queue
        const uint32_t line = (uint32_t)(lf - pos) + 2;
        if (sl.watching) {
            put_op(O, s, R, OP_PASS, line, 0);
            R.taken += line;
            pos += line;
            continue;
        }
        const McTok t = mcs_first_token(W, pos, lf);
        if (t.len == 0) { R.result = 1; return; }  // tokens[0] of a blank line
        const McSessIntent *q = &ring[sl.head & mask];
        const uint32_t cls = q->cls;
        bool one = MCS_IS(t, "ERROR") || MCS_IS(t, "CLIENT_ERROR") || MCS_IS(t, "SERVER_ERROR") || cls == MCC_LINE;
        if (!one && cls == MCC_CRAWLER) one = MCS_IS(t, "OK") || MCS_IS(t, "BUSY") || MCS_IS(t, "BADCLASS");
        uint32_t n = line;
        if (!one) {
            if (cls == MCC_OTHER) { R.result = 1; return; }  // ERROR, 0
            // (no hit starts before the first "\r\n", and one at the frame's start has no token before it)
            const uint64_t e = mcs_wave_end(b, lf, len);
            if (e == len) {
                put_op(O, s, R, OP_MORE, 1, 0);
                return;
            }
            n = (uint32_t)(e - pos) + 7;
        }
        put_op(O, s, R, OP_PASS, n, q->tag);
        sl.head = (sl.head + 1) & mask;
        sl.count--;
        R.passed++;
        R.taken += n;
        pos += n;
    }
}

// binary/parser.go OnData(reply) under the op loop: a hop over 24-byte headers, the lanes in step
__device__ __forceinline__ void binary_replies(McSessSlot &sl, const uint8_t *b, uint64_t len, const McReplyOut &O,
                                               uint64_t s, ReplyRun &R) {
    McReader W{b, ~0ull, 0, 0};
    uint64_t pos = 0;
    while (R.nops < O.max_ops) {
        if (sl.bstate == MCB_ARMED && sl.armed_id == sl.replies + 1u) {
            sl.replies++;
            sl.bstate = MCB_BLOCKED;  // (its second copy heads the queue now and never fires)
            R.inj++;
            put_op(O, s, R, OP_INJECT, kMcDeniedBinaryLen, sl.armed_magic);
            continue;
        }
        if (pos >= len) return;  // NOP
        const uint64_t rem = len - pos;
        if (rem < 24) {
            put_op(O, s, R, OP_MORE, (uint32_t)(24 - rem), 0);
            return;
        }
        const uint32_t keylen = mcs_rd(W, pos + 2) << 8 | mcs_rd(W, pos + 3), extras = mcs_rd(W, pos + 4);
        if (keylen > 0 && 24u + keylen + extras > rem) {
            put_op(O, s, R, OP_MORE, (uint32_t)(24u + keylen + extras - rem), 0);
            return;
        }
        if (!(mcs_rd(W, pos) & 0x80)) {  // ERROR_INVALID_FRAME_TYPE: neither advances nor ends the loop
            put_op(O, s, R, OP_ERROR, 2, 0);
            continue;
        }
        const uint32_t body = mcs_rd(W, pos + 8) << 24 | mcs_rd(W, pos + 9) << 16 | mcs_rd(W, pos + 10) << 8 |
                              mcs_rd(W, pos + 11);
        sl.replies++;
        const uint32_t n = body + 24u;  // (uint32, as the reference adds)
        if (n == 0) { R.result = 1; return; }
        put_op(O, s, R, OP_PASS, n, 0);
        R.passed++;
        R.taken += n;
        pos = n < len - pos ? pos + n : len;
    }
}

}  // namespace

// One wave per stream: the lanes find line ends and END together
// (mc_session.h) and carry the queue head in step; lane 0 writes.
__global__ __launch_bounds__(kBlock) void mcsess_replies_kernel(McSessBatch B, McSessions S, McReplyOut O) {
    constexpr uint32_t kWaves = kBlock / 64;
    for (uint64_t s = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); s < B.n; s += (uint64_t)gridDim.x * kWaves) {
        ReplyRun R{0, 0, 0, 0, 0};
        McSessSlot sl{};
        uint32_t ci = 0;
        if (!sess_item(B, S.nslots, PROTO_MEMCACHE, (uint32_t)s)) {
            R.result = 2;
        } else {
            ci = B.conn_ids[s];
            const uint64_t len = B.lens[s];
            const uint8_t *b = B.arena + B.offs[s];
            sl = S.slots[ci];
            if (sl.kind == MCK_NONE) {
                // memcached/parser.go:186-202: no parser yet, the first byte makes one
                const uint32_t mode = B.conns[ci].flags & 3;
                if (len == 0) R.result = 3;
                else sl.kind = (uint8_t)(mode ? mode : b[0] >= 0x80 ? MCK_BINARY : MCK_TEXT);
            }
            if (sl.kind == MCK_TEXT) text_replies(S, ci, sl, b, len, O, s, R);
            else if (sl.kind == MCK_BINARY) binary_replies(sl, b, len, O, s, R);
        }
        if (__lane_id() == 0) {
            if (sl.kind != MCK_NONE) S.slots[ci] = sl;
            O.nops[s] = R.nops;
            O.result[s] = (uint8_t)R.result;
            O.taken[s] = R.taken;
            if (R.inj) atomicAdd(&S.stats[MSS_INJECT_QUEUED], (unsigned long long)R.inj);
            if (R.passed) atomicAdd(&S.stats[MSS_PASSED], (unsigned long long)R.passed);
            if (R.result == 1) atomicAdd(&S.stats[MSS_ERRORS], 1ull);
        }
    }
}

// New-connection events: the slot is a new connection's again.
__global__ __launch_bounds__(kBlock) void mcsess_reset_kernel(McSessions S, const uint32_t *__restrict__ conn,
                                                              uint32_t n) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n || conn[k] >= S.nslots) return;
    // (an index named twice is zeroed by either lane or both)
    *reinterpret_cast<uint4 *>(&S.slots[conn[k]]) = make_uint4(0, 0, 0, 0);
    *(reinterpret_cast<uint4 *>(&S.slots[conn[k]]) + 1) = make_uint4(0, 0, 0, 0);
}

// out[0]: intents queued; out[1]: connections whose parser is locked
__global__ __launch_bounds__(kBlock) void mcsess_live_kernel(McSessions S, unsigned long long *__restrict__ out) {
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < S.nslots; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t p = base + threadIdx.x;
        const uint32_t count = p < S.nslots && S.slots[p].kind == MCK_TEXT ? S.slots[p].count : 0;
        if (count) atomicAdd(&out[0], (unsigned long long)count);
        wave_count(&out[1], p < S.nslots && S.slots[p].kind != MCK_NONE);
    }
}

size_t McSessForwardScratchBytes(uint32_t n, uint32_t nconns) {
    size_t sort_temp = 0, scan_temp = 0;
    if (n > 0x7FFFFFFFu ||
        hipcub::DeviceRadixSort::SortKeys(nullptr, sort_temp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0,
                                          32 + ConnBits(nconns)) != hipSuccess ||
        hipcub::DeviceScan::InclusiveScan(nullptr, scan_temp, (const McScan *)nullptr, (McScan *)nullptr, McScanOp{},
                                          (int)n) != hipSuccess)
        return 0;
    return McForwardLayout(n, nconns, std::max(sort_temp, scan_temp)).total;
}

hipError_t LaunchMcSessForward(const McSessBatch &B, const McSessions &S, const uint8_t *verdict, const uint64_t *tag,
                               uint8_t *act, void *scratch, size_t scratch_bytes, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const McForwardScratch L = McForwardLayout(B.n, B.nconns, 0);
    if (scratch_bytes < L.temp) return hipErrorInvalidValue;
    uint8_t *base = (uint8_t *)scratch;
    uint64_t *keys = (uint64_t *)(base + L.keys), *sorted = (uint64_t *)(base + L.sorted);
    uint8_t *info = base + L.info;
    McScan *el = (McScan *)(base + L.el), *sc = (McScan *)(base + L.sc);
    McSeg *seg = (McSeg *)(base + L.seg);
    void *temp = base + L.temp;
    size_t temp_bytes = scratch_bytes - L.temp;
    const dim3 grid = GridFor(B.n), block(kBlock);
    hipLaunchKernelGGL(mcsess_keys_kernel, grid, block, 0, stream, B, S, verdict, keys, info, act);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    // (the index is part of the key: batch order inside a connection does not lean on a stable sort)
    rc = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, sorted, (int)B.n, 0, 32 + ConnBits(B.nconns), stream);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(mcsess_heads_kernel, grid, block, 0, stream, B, S, (const uint64_t *)sorted,
                       (const uint8_t *)info, seg);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    hipLaunchKernelGGL(mcsess_elems_kernel, grid, block, 0, stream, B, (const uint64_t *)sorted, (const uint8_t *)info,
                       (const McSeg *)seg, el);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    rc = hipcub::DeviceScan::InclusiveScan(temp, temp_bytes, (const McScan *)el, sc, McScanOp{}, (int)B.n, stream);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(mcsess_resolve_kernel, grid, block, 0, stream, B, S, (const uint64_t *)sorted,
                       (const uint8_t *)info, (const McSeg *)seg, (const McScan *)sc, tag, act);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    hipLaunchKernelGGL(mcsess_advance_kernel, grid, block, 0, stream, B, S, (const uint64_t *)sorted, (const McSeg *)seg,
                       (const McScan *)sc);
    return hipGetLastError();
}

hipError_t LaunchMcSessReplies(const McSessBatch &B, const McSessions &S, const McReplyOut &O, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    // a wave per stream: kBlock / 64 streams per workgroup
    hipLaunchKernelGGL(mcsess_replies_kernel, GridFor((uint64_t)B.n * 64), dim3(kBlock), 0, stream, B, S, O);
    return hipGetLastError();
}

hipError_t LaunchMcSessReset(const McSessions &S, const uint32_t *conn, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mcsess_reset_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, S, conn, n);
    return hipGetLastError();
}

hipError_t LaunchMcSessLive(const McSessions &S, unsigned long long *out2, hipStream_t stream) {
    hipLaunchKernelGGL(mcsess_live_kernel, GridFor(S.nslots), dim3(kBlock), 0, stream, S, out2);
    return hipGetLastError();
}

}  // namespace l7

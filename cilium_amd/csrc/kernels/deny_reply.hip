// Deny replies on gfx950 (product code): l7g_deny_replies, a post-pass over a
// classified batch that writes what each enforcement point of the reference
// sends back for a DENY, packed in request order.
//
//   Kafka       req.CreateResponse(ErrTopicAuthorizationFailed), every topic and
//               partition of the request echoed (pkg/proxy/kafka.go:249-261,
//               pkg/kafka/response.go:81-315): byte for byte what
//               l7g_kafka_deny_response (proxylib/kafka_response.cc) writes
//   HTTP        Envoy's 403 local reply (envoy/cilium_l7policy.cc:90-96,171-177)
//   cassandra   the unauthorized frame (cassandraparser.go:269-278)
//   r2d2        "ERROR\r\n"
//   (the three templates: deny_templates.h; memcached is answered nothing here,
//   see include/l7gpu.h)
//
// Three steps on the caller's stream:
// 1. deny_select_kernel: one coalesced pass over verdict and conn.  The fixed
//    replies get their length; denied Kafka requests are appended to an index
//    list (ballot + prefix; one atomic per workgroup step), so that the walks
//    below run in full waves and not in one lane of 64.
// 2. deny_kafka_kernel<false>: one lane per list entry decodes its request as
//    kafka_response.cc's Decode does (kresp::Decode restated on the wire
//    decoder and message set of kafka_wire.h over the device's byte cursor,
//    CRC included: a mismatch stops a message set without draining it, and
//    the next partition id is then read from inside the set)
//    and counts the reply's bytes; any decode error gives length 0.  Then an
//    exclusive sum of len[] into off[] (hipcub::DeviceScan).
// 3. deny_fixed_write_kernel writes the templates and the two totals; the
//    write instantiation of deny_kafka_kernel walks the list entries again,
//    now emitting (a request whose message sets the size pass read to their
//    ends steps over them: no second CRC).  Reply i is written only if
//    off[i] + len[i] <= cap.
// The same walk template serves both passes (a counting and a writing
// emitter), so the bytes written are exactly the bytes counted.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../deny_templates.h"
#include "../device_tables.h"
#include "kafka_wire.h"
#include "launch.h"

namespace l7 {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMaxBlocks = 4096;  // every grid's ceiling; grid-stride above it
constexpr int16_t kErrTopicAuthorizationFailed = 29;  // proto/errors.go:37
// time.Time{}.UnixNano() / int64(time.Millisecond) under Go 1.10's int64
// wrap-around: the ListOffsets v1+ timestamp (messages.go:1996)
constexpr int64_t kZeroTimeMillis = -6795364578871LL;

// The request decoder is kafka_wire.h's KD over the chunk cursor (CurRd), which
// reads as kafka_response.cc's Dec does: short reads are errors, errors are
// sticky.  A message set is read for its effect on the position and on errors,
// as kafka_response.cc's SkipMessageSet (kd_message_set): a compressed message
// needs no inflate, since its inner set changes nothing the reply echoes, and
// the walk leaves the set there.
struct DenySetHooks : CurCrc {
    static constexpr bool kLeaveAtPacked = true;
};

// ---------------- the reply emitters ----------------
// what the size pass runs the walk with: the bytes, counted
struct CountEmit {
    uint32_t n;
    __device__ __forceinline__ void put(uint64_t, uint32_t k) { n += k; }
    __device__ __forceinline__ void zeros(uint32_t k) { n += k; }
    __device__ __forceinline__ void copy(const uint8_t *, uint32_t k) { n += k; }
};
// and the write pass: plain vector stores at any byte alignment, byte stores
// at the ragged ends and dword stores in between
struct WriteEmit {
    uint8_t *p;
    // k (1..8) bytes, the low k of m in memory order
    __device__ __forceinline__ void store(uint64_t m, uint32_t k) {
        while (k) {
            if (k >= 4 && ((uintptr_t)p & 3) == 0) {
                *reinterpret_cast<uint32_t *>(p) = (uint32_t)m;
                p += 4; m >>= 32; k -= 4;
            } else {
                *p = (uint8_t)m;
                p += 1; m >>= 8; k -= 1;
            }
        }
    }
    // the low k (1..8) bytes of v, big-endian
    __device__ __forceinline__ void put(uint64_t v, uint32_t k) { store(__builtin_bswap64(v) >> (64 - 8 * k), k); }
    __device__ __forceinline__ void zeros(uint32_t k) {
        for (; k >= 8; k -= 8) store(0, 8);
        if (k) store(0, k);
    }
    // k bytes from s: source and destination both at any alignment
    __device__ __forceinline__ void copy(const uint8_t *s, uint32_t k) {
        while (k && ((uintptr_t)p & 3)) { *p++ = *s++; k--; }
        for (; k >= 4; k -= 4) {
            uint32_t w;
            __builtin_memcpy(&w, s, 4);  // (as the target loads an unaligned dword)
            *reinterpret_cast<uint32_t *>(p) = w;
            p += 4; s += 4;
        }
        while (k) { *p++ = *s++; k--; }
    }
};

// One partition of the reply (the Encode switch of kafka_response.cc:280-393).
template <class E>
__device__ __forceinline__ void emit_partition(E &e, int kind, int16_t v, int32_t id) {
    e.put((uint32_t)id, 4);
    switch (kind) {
    case 0:  // ProduceResp: errno, Offset, v2+ LogAppendTime
        e.put(kErrTopicAuthorizationFailed, 2);
        e.zeros(v >= 2 ? 16 : 8);
        break;
    case 1:  // FetchResp: errno, TipOffset, v4+ LastStableOffset, v5+ LogStartOffset, v4+ nil aborted array, set size
        e.put(kErrTopicAuthorizationFailed, 2);
        e.zeros(8);
        if (v >= 4) {
            e.zeros(v >= 5 ? 16 : 8);
            e.put(0xFFFFFFFFu, 4);
        }
        e.zeros(4);
        break;
    case 2:  // OffsetResp: errno, v1+ timestamp, empty Offsets
        e.put(kErrTopicAuthorizationFailed, 2);
        if (v >= 1) e.put((uint64_t)kZeroTimeMillis, 8);
        e.zeros(4);
        break;
    case 8:  // OffsetCommitResp: errno
        e.put(kErrTopicAuthorizationFailed, 2);
        break;
    default:  // 9, OffsetFetchResp: Offset, Metadata "", errno
        e.zeros(10);
        e.put(kErrTopicAuthorizationFailed, 2);
        break;
    }
}

// kafka.ReadRequest + the typed decoder + the response encoder, in one pass:
// the reply's fields follow the request's in wire order, so each is emitted as
// its source is read.  false = no response (untyped kind, framing or decode
// error): whatever was emitted until then is void -- the size pass answers
// length 0, and the write pass only walks requests the size pass accepted.
// `total`: the reply's length (its size word is total - 4; the size pass gives 0).
// whole: cleared when the walk leaves a message set before its end (a CRC
// mismatch, a compressed or short message).  skip: the size pass found every
// set of this request read to its end, so the write pass steps over them, CRCs
// unread.
template <class E>
__device__ __forceinline__ bool reply_walk(const uint8_t *b, uint32_t len, const uint32_t *crctab, uint32_t total,
                                           E &e, bool &whole, bool skip) {
    if (len < 12) return false;
    Cur cur;
    cur.line = ~(uintptr_t)0;
    CurRd r{b, &cur};
    const int32_t size = (int32_t)r.be(0, 4);
    if (size <= 0 || (uint64_t)(uint32_t)size + 4 > len || (uint64_t)(uint32_t)size + 4 > kMaxParseBuf ||
        (uint32_t)size + 4 < 12)
        return false;
    KD<CurRd> d{&r, 4, (uint32_t)size + 4, -1, 0};
    const int kind = (int16_t)kd_int(d, 2);
    const int16_t v = (int16_t)kd_int(d, 2);
    const uint32_t corr = (uint32_t)kd_int(d, 4);
    if (!(kind == 0 || kind == 1 || kind == 2 || kind == 3 || kind == 8 || kind == 9 || kind == 10))
        return false;  // request == nil: "unsupported request API key"
    uint32_t o, l;
    kd_string(d, o, l);  // ClientID
    e.put(total - 4, 4);
    e.put(corr, 4);
    bool bad = false, packed = false;  // (packed: kd_message_set's zflag, not used here)
    DenySetHooks h{{crctab, r}};
    int32_t nt = 0, np = 0;
    switch (kind) {
    case 0:  // Produce (messages.go:1591-1647) -> ProduceResp.Bytes (:1716)
        if (v >= 3) kd_string(d, o, l);
        kd_skip(d, 6);
        nt = kd_arraylen(d, false, bad);
        if (bad) return false;
        e.put((uint32_t)nt, 4);
        for (int32_t t = 0; t < nt; t++) {
            kd_string(d, o, l);
            if (d.err) return false;
            np = kd_arraylen(d, false, bad);
            if (bad) return false;
            e.put(l, 2);
            e.copy(b + o, l);
            e.put((uint32_t)np, 4);
            for (int32_t p = 0; p < np; p++) {
                const int32_t id = (int32_t)kd_int(d, 4);
                const int32_t ss = (int32_t)kd_int(d, 4);
                if (d.err) return false;
                if (ss > (int32_t)kMaxParseBuf) return false;
                // the set's bytes: min(size, room); read whole when the walk advances by exactly that
                const uint32_t room = d.end - d.pos, at = d.pos;
                const uint32_t want = ss < 0 ? 0u : (uint32_t)ss < room ? (uint32_t)ss : room;
                if (skip) {
                    d.pos += want;
                } else {
                    if (kd_message_set(r, d.pos, d.end, ss, v, packed, h) < 0) return false;
                    whole = whole && d.pos - at == want;
                }
                emit_partition(e, 0, v, id);
            }
        }
        if (v >= 1) e.zeros(4);  // ThrottleTime
        break;
    case 1:  // Fetch (:767-824) -> FetchResp.Bytes (:911)
    case 2:  // ListOffsets (:1810-1858) -> OffsetResp.Bytes (:1975)
    case 8:  // OffsetCommit (:1173-1228) -> OffsetCommitResp.Bytes (:1342)
    case 9:  // OffsetFetch (:1389-1430) -> OffsetFetchResp.Bytes (:1531)
        if (kind == 1) {
            kd_skip(d, 12);
            if (v >= 3) kd_skip(d, 4);
            if (v >= 4) kd_skip(d, 1);
            if (v >= 1) e.zeros(4);
        } else if (kind == 2) {
            kd_skip(d, 4);
            if (v >= 2) { kd_skip(d, 1); e.zeros(4); }
        } else if (kind == 8) {
            kd_string(d, o, l);
            if (v >= 1) { kd_skip(d, 4); kd_string(d, o, l); }
            if (v >= 2) kd_skip(d, 8);
            if (v >= 3) e.zeros(4);
        } else {
            kd_string(d, o, l);
            if (v >= 3) e.zeros(4);
        }
        nt = kd_arraylen(d, kind == 9, bad);
        if (bad) return false;
        e.put((uint32_t)nt, 4);  // (a null OffsetFetch array: -1)
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            np = kd_arraylen(d, false, bad);
            if (bad) return false;
            e.put(l, 2);
            e.copy(b + o, l);
            e.put((uint32_t)np, 4);
            for (int32_t p = 0; p < np && !d.err; p++) {
                const int32_t id = (int32_t)kd_int(d, 4);
                if (kind == 1) {
                    kd_skip(d, v >= 5 ? 20 : 12);
                } else if (kind == 2) {
                    kd_skip(d, v == 0 ? 12 : 8);
                } else if (kind == 8) {
                    kd_skip(d, v == 1 ? 16 : 8);
                    uint32_t o2, l2;
                    kd_string(d, o2, l2);
                }
                emit_partition(e, kind, v, id);
            }
        }
        if (kind == 9 && v >= 2) e.zeros(2);  // Err: nil
        break;
    case 3:  // Metadata (:504-537) -> MetadataResp.Bytes (:610)
        if (v >= 3) e.zeros(4);
        e.zeros(4);              // Brokers: empty, not nil
        if (v >= 2) e.zeros(2);  // ClusterID
        if (v >= 1) e.zeros(4);  // ControllerID
        nt = kd_arraylen(d, true, bad);
        if (bad) return false;
        e.put((uint32_t)nt, 4);
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            e.put(kErrTopicAuthorizationFailed, 2);
            e.put(l, 2);
            e.copy(b + o, l);
            e.zeros(v >= 1 ? 5 : 4);  // v1+ IsInternal; Partitions: empty, not nil
        }
        if (v >= 4) kd_skip(d, 1);
        break;
    default:  // 10: ConsumerMetadata (:1033-1054) -> ConsumerMetadataResp.Bytes (:1117)
        kd_string(d, o, l);
        if (v >= 1) kd_skip(d, 1);
        if (v >= 1) e.zeros(4);
        e.put(kErrTopicAuthorizationFailed, 2);
        e.zeros(v >= 1 ? 12 : 10);  // v1+ ErrMsg; CoordinatorID, CoordinatorHost, CoordinatorPort
        break;
    }
    return !d.err;
}

// the protocol that answers request i's DENY, PROTO_NONE if nothing does (not
// DENY, connection outside the table, bytes outside the arena)
__device__ __forceinline__ uint8_t reply_proto(const Batch &B, uint32_t i) {
    if (B.verdict[i] != V_DENY) return PROTO_NONE;
    const uint32_t ci = B.conn_ids[i];
    if (ci >= B.nconns) return PROTO_NONE;
    if (!l7_in_arena(B.offs[i], B.lens[i], B.arena_len)) return PROTO_NONE;
    return B.conns[ci].proto;
}

// ctl: [0] Kafka list entries, [1] replies with len > 0 (zeroed by the launcher)
// One atomic per workgroup and step: a wave takes kSelSteps x 64 consecutive
// requests (coalesced), counts its Kafka entries by ballot, the workgroup's
// four counts meet in LDS, and each lane's place is the workgroup's base + the
// waves before its own + the lanes before it.  (One atomic per wave: 15.6k
// adds on one address per 1M requests, 70-180 us; this: 1k.)
constexpr int kSelSteps = 4;
constexpr uint32_t kSelPerBlock = kBlock * kSelSteps;
__global__ __launch_bounds__(kBlock) void deny_select_kernel(Batch B, uint32_t *__restrict__ rlen,
                                                             uint32_t *__restrict__ klist, uint32_t *__restrict__ ctl) {
    __shared__ uint32_t wcnt[kBlock / 64], wnz[kBlock / 64], wbase;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    uint32_t nz = 0;  // (wave-uniform) fixed replies of this wave
    // (whole workgroups take each step: the ballots and barriers below are over converged lanes)
    for (uint64_t base = (uint64_t)blockIdx.x * kSelPerBlock; base < B.n; base += (uint64_t)gridDim.x * kSelPerBlock) {
        unsigned long long km[kSelSteps];
        uint32_t cnt = 0;
#pragma unroll
        for (int s = 0; s < kSelSteps; s++) {
            const uint64_t i64 = base + wv * (64 * kSelSteps) + s * 64 + lane;
            const bool in = i64 < B.n;
            const uint32_t i = (uint32_t)i64;
            const uint8_t proto = in ? reply_proto(B, i) : (uint8_t)PROTO_NONE;
            uint32_t l = 0;
            if (proto == PROTO_HTTP) l = kDenied403Len;
            else if (proto == PROTO_R2D2) l = kR2ErrorLen;
            else if (proto == PROTO_CASSANDRA) l = B.lens[i] >= 4 ? kCassUnauthLen : 0u;
            if (in) rlen[i] = l;  // (a Kafka request's: by the size pass)
            km[s] = __ballot(proto == PROTO_KAFKA);
            cnt += (uint32_t)__popcll(km[s]);
            nz += (uint32_t)__popcll(__ballot(l > 0));
        }
        if (lane == 0) wcnt[wv] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < kBlock / 64; w++) t += wcnt[w];
            wbase = t ? atomicAdd(&ctl[0], t) : 0u;
        }
        __syncthreads();
        uint32_t at = wbase;
        for (uint32_t w = 0; w < wv; w++) at += wcnt[w];
#pragma unroll
        for (int s = 0; s < kSelSteps; s++) {
            if ((km[s] >> lane) & 1)
                klist[at + (uint32_t)__popcll(km[s] & below)] = (uint32_t)(base + wv * (64 * kSelSteps) + s * 64 + lane);
            at += (uint32_t)__popcll(km[s]);
        }
        __syncthreads();  // (wcnt and wbase are rewritten by the next step)
    }
    if (lane == 0) wnz[wv] = nz;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kBlock / 64; w++) t += wnz[w];
        if (t) atomicAdd(&ctl[1], t);
    }
}

// kWrite false: the size pass (rlen[i] = the reply's bytes, 0 = none; bit 31 of
// the list entry set when every message set of the request was read to its
// end); true: the write pass (reply i to buf + roff[i] when it fits under cap)
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void deny_kafka_kernel(Batch B, uint32_t *__restrict__ rlen,
                                                            const uint64_t *__restrict__ roff,
                                                            uint32_t *__restrict__ klist,
                                                            uint32_t *__restrict__ ctl, uint8_t *__restrict__ buf,
                                                            uint64_t cap) {
    __shared__ uint32_t crctab[kCrcTables * 256];
    __shared__ uint32_t wnz[kBlock / 64];
    const uint32_t m = ctl[0];
    if ((uint64_t)blockIdx.x * kBlock >= m) return;  // (the whole workgroup: before the tables' barriers)
    crc_tables_init<kBlock>(crctab, threadIdx.x);
    uint32_t nz = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t ent = klist[j];
        const uint32_t i = ent & 0x7FFFFFFFu;
        bool whole = true;
        // (reply_proto admitted it: the bytes lie inside the arena)
        const uint8_t *b = B.arena + B.offs[i];
        const uint32_t len = B.lens[i];
        if constexpr (kWrite) {
            const uint32_t total = rlen[i];
            const uint64_t at = roff[i];
            if (total == 0 || at > cap || total > cap - at) continue;
            WriteEmit e{buf + at};
            reply_walk(b, len, crctab, total, e, whole, (ent >> 31) != 0);
        } else {
            CountEmit e{0};
            const uint32_t total = reply_walk(b, len, crctab, 0, e, whole, false) ? e.n : 0u;
            rlen[i] = total;
            nz += total > 0;
            if (total && whole) klist[j] = ent | 0x80000000u;
        }
    }
    if constexpr (!kWrite) {
        // the workgroup's replies in one add (every thread is here: the early return above is the workgroup's)
        for (int d = 32; d > 0; d >>= 1) nz += (uint32_t)__shfl_down((int)nz, d, 64);
        if ((threadIdx.x & 63) == 0) wnz[threadIdx.x >> 6] = nz;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < kBlock / 64; w++) t += wnz[w];
            if (t) atomicAdd(&ctl[1], t);
        }
    }
}

// the fixed replies, and the call's two totals
__global__ __launch_bounds__(kBlock) void deny_fixed_write_kernel(Batch B, const uint32_t *__restrict__ rlen,
                                                                  const uint64_t *__restrict__ roff,
                                                                  const uint32_t *__restrict__ ctl,
                                                                  uint8_t *__restrict__ buf, uint64_t cap,
                                                                  uint64_t *__restrict__ total) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        total[0] = B.n ? roff[B.n - 1] + rlen[B.n - 1] : 0;
        total[1] = ctl[1];
    }
    for (uint64_t i64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i64 < B.n; i64 += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)i64;
        const uint32_t l = rlen[i];
        if (l == 0) continue;
        const uint64_t at = roff[i];
        if (at > cap || l > cap - at) continue;
        const uint8_t proto = reply_proto(B, i);
        WriteEmit e{buf + at};
        if (proto == PROTO_HTTP) {
            e.copy(reinterpret_cast<const uint8_t *>(kDenied403), kDenied403Len);
        } else if (proto == PROTO_R2D2) {
            e.copy(reinterpret_cast<const uint8_t *>(kR2Error), kR2ErrorLen);
        } else if (proto == PROTO_CASSANDRA) {
            const uint8_t *q = B.arena + B.offs[i];  // (len >= 4: the select pass gave it a reply)
            e.put(0x80u | (q[0] & 7u), 1);
            e.put(kCassUnauth[1], 1);
            e.put(q[2], 1);
            e.put(q[3], 1);
            e.copy(kCassUnauth + 4, kCassUnauthLen - 4);
        }
    }
}

struct U32ToU64 {
    __host__ __device__ __forceinline__ uint64_t operator()(uint32_t x) const { return x; }
};
using LenIter = hipcub::TransformInputIterator<uint64_t, U32ToU64, const uint32_t *>;

constexpr size_t kCtlBytes = 256;  // the two counters, and the list 256-byte aligned behind them
size_t ListBytes(uint32_t n) { return ((size_t)n * sizeof(uint32_t) + 255) & ~(size_t)255; }
uint32_t Blocks(uint32_t n) {
    const uint64_t b = ((uint64_t)n + kBlock - 1) / kBlock;
    return (uint32_t)(b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b);
}

}  // namespace

// Scratch bytes LaunchDenyReplies needs for n requests: 256 (counters) + 4 n
// (the Kafka index list, rounded up to 256) + the scan's temporary storage.
size_t DenyRepliesScratchBytes(uint32_t n) {
    size_t temp = 0;
    if (hipcub::DeviceScan::ExclusiveScan(nullptr, temp, LenIter(nullptr, U32ToU64()), (uint64_t *)nullptr, hipcub::Sum(),
                                          (uint64_t)0, (int)n) != hipSuccess)
        return 0;
    return kCtlBytes + ListBytes(n) + ((temp + 255) & ~(size_t)255);
}

// B.verdict is read, not written; B.rule and B.consumed are not used.
// scratch: DenyRepliesScratchBytes(B.n) bytes, 256-byte aligned.
hipError_t LaunchDenyReplies(const Batch &B, uint8_t *buf, uint64_t cap, uint64_t *roff, uint32_t *rlen,
                             uint64_t *total, void *scratch, size_t scratch_bytes, hipStream_t stream) {
    if (B.n > 0x7FFFFFFFu) return hipErrorInvalidValue;  // (the scan counts in int)
    if (scratch_bytes < kCtlBytes + ListBytes(B.n)) return hipErrorInvalidValue;
    uint32_t *ctl = (uint32_t *)scratch;
    uint32_t *klist = (uint32_t *)((uint8_t *)scratch + kCtlBytes);
    void *temp = (uint8_t *)scratch + kCtlBytes + ListBytes(B.n);
    size_t temp_bytes = scratch_bytes - kCtlBytes - ListBytes(B.n);
    hipError_t rc = hipMemsetAsync(ctl, 0, 2 * sizeof(uint32_t), stream);
    if (rc != hipSuccess) return rc;
    const dim3 grid(Blocks(B.n)), block(kBlock);
    if (B.n) {
        const dim3 sgrid(Blocks((uint32_t)(((uint64_t)B.n + kSelSteps - 1) / kSelSteps)));
        hipLaunchKernelGGL(deny_select_kernel, sgrid, block, 0, stream, B, rlen, klist, ctl);
        if ((rc = hipGetLastError()) != hipSuccess) return rc;
        hipLaunchKernelGGL(deny_kafka_kernel<false>, grid, block, 0, stream, B, rlen, (const uint64_t *)nullptr, klist, ctl,
                           (uint8_t *)nullptr, (uint64_t)0);
        if ((rc = hipGetLastError()) != hipSuccess) return rc;
        rc = hipcub::DeviceScan::ExclusiveScan(temp, temp_bytes, LenIter(rlen, U32ToU64()), roff, hipcub::Sum(),
                                               (uint64_t)0, (int)B.n, stream);
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(deny_fixed_write_kernel, grid, block, 0, stream, B, (const uint32_t *)rlen,
                       (const uint64_t *)roff, (const uint32_t *)ctl, buf, cap, total);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    if (B.n && cap) {
        hipLaunchKernelGGL(deny_kafka_kernel<true>, grid, block, 0, stream, B, rlen, (const uint64_t *)roff, klist, ctl, buf,
                           cap);
        rc = hipGetLastError();
    }
    return rc;
}

}  // namespace l7

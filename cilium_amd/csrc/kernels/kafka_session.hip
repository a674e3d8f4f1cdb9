// Kafka sessions on gfx950 (product code): the correlation cache of the
// in-agent Kafka proxy (pkg/kafka/correlation_cache.go:97-213) for a batch,
// resident in HBM (device_tables.h KafkaSessSlot / KafkaSessEntry).
//
// l7g_kafka_forward (HandleRequest, :116-147), on the caller's stream:
//   ksess_keys_kernel    one key (connection << 32 | index) per forwarded
//     request, a key past every connection for the others;
//   a hipcub radix sort  (bits 0 .. 32 + those of a connection index);
//   ksess_heads_kernel   the first key of every connection's segment finds the
//     segment's end (a binary search), keeps (segment start, the slot's
//     sequence number before the batch) for its connection and advances the
//     slot by the segment's length -- once per connection;
//   ksess_insert_kernel  one lane per sorted key: rank = position - segment
//     start, new id = sequence number + 1 + rank; the lane claims a table slot
//     (kernels/kafka_session.h), fills it and rewrites the frame's id.
// l7g_kafka_responses (CorrelateResponse, :158-178):
//   ksess_probe_kernel   each response finds the entry of (connection, id) and
//     atomicMins its batch index into the entry's taker word;
//   ksess_take_kernel    the response the taker word names restores the id,
//     reports the entry and deletes it; every other one is a miss.  So of
//     several responses with one id the earliest in batch order is the hit,
//     as in the reference's loop.
// l7g_kafka_session_gc: ksess_gc_kernel re-inserts every live, unexpired entry
// of the table into the spare one (zeroed first); the host swaps the two.
//
// Every grid is capped at kSessMaxBlocks workgroups and strides above that; loops
// are uniform per wave so that the statistics take one atomic per wave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "kafka_session.h"
#include "launch.h"

namespace l7 {

namespace {

constexpr int kBlock = kSessBlock;
static_assert(sizeof(uint2) == kKafkaSegBytes, "seg[] as sess_scratch.h lays it out");

__device__ __forceinline__ uint32_t be_bytes(const uint8_t *p, int k) {
    uint32_t v = 0;
    for (int j = 0; j < k; j++) v = v << 8 | p[j];
    return v;
}

// v big-endian to p at any alignment: one dword store, or four byte stores
__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v) {
    if (((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uint32_t *>(p) = __builtin_bswap32(v);
    } else {
        p[0] = (uint8_t)(v >> 24);
        p[1] = (uint8_t)(v >> 16);
        p[2] = (uint8_t)(v >> 8);
        p[3] = (uint8_t)v;
    }
}

}  // namespace

__global__ __launch_bounds__(kBlock) void ksess_keys_kernel(KafkaSessBatch B, KafkaSessions S,
                                                            const uint8_t *__restrict__ verdict,
                                                            uint64_t *__restrict__ keys, uint8_t *__restrict__ fwd,
                                                            uint32_t *__restrict__ new_id) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < B.n; i += (uint64_t)gridDim.x * kBlock) {
        const bool go = verdict[i] == V_ALLOW && sess_item(B, S.nslots, PROTO_KAFKA, (uint32_t)i);
        keys[i] = sess_key(go ? B.conn_ids[i] : B.nconns, (uint32_t)i);
        if (!go) {
            fwd[i] = 0;
            new_id[i] = 0;
        }
    }
}

// seg[connection] = (segment start in sorted, sequence numbers spent before the batch)
__global__ __launch_bounds__(kBlock) void ksess_heads_kernel(KafkaSessBatch B, KafkaSessions S,
                                                             const uint64_t *__restrict__ sorted,
                                                             uint2 *__restrict__ seg) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < B.n; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t ci = key_conn(sorted[j]);
        if (ci >= B.nconns || !segment_head(sorted, j)) continue;
        const uint64_t end = segment_end(sorted, j, B.n, ci);
        KafkaSessSlot *slot = &S.slots[ci];
        seg[ci] = make_uint2((uint32_t)j, slot->seq);
        slot->seq += (uint32_t)(end - j);
    }
}

__global__ __launch_bounds__(kBlock) void ksess_insert_kernel(KafkaSessBatch B, KafkaSessions S,
                                                              const uint64_t *__restrict__ sorted,
                                                              const uint2 *__restrict__ seg,
                                                              const uint64_t *__restrict__ tag, uint64_t now_ms,
                                                              uint8_t *__restrict__ fwd, uint32_t *__restrict__ new_id) {
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < B.n; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t j = base + threadIdx.x;
        const uint32_t ci = j < B.n ? key_conn(sorted[j]) : B.nconns;
        bool kept = false, dropped = false;
        if (ci < B.nconns) {
            const uint32_t i = key_index(sorted[j]);
            const uint2 sg = seg[ci];
            const uint32_t id = sg.y + 1u + ((uint32_t)j - sg.x);
            uint8_t *r = B.arena + B.offs[i];
            const uint32_t len = B.lens[i];
            KafkaSessEntry *e = ksess_claim(S, S.tab, sess_claim_of(ci, S.slots[ci].gen), ci, id);
            if (e) {
                e->id = id;
                e->orig = len >= 12 ? be_bytes(r + 8, 4) : 0;
                e->api_key = len >= 6 ? (int16_t)be_bytes(r + 4, 2) : (int16_t)0;
                e->api_version = len >= 8 ? (int16_t)be_bytes(r + 6, 2) : (int16_t)0;
                e->taker = kKafkaSessNoTaker;
                e->tag = tag ? tag[i] : 0;
                e->created_ms = now_ms;
                if (len >= 12) put_be32(r + 8, id);
            }
            kept = e != nullptr;
            dropped = !kept;
            fwd[i] = kept ? 1 : 2;
            new_id[i] = kept ? id : 0;
        }
        wave_count(&S.stats[KSS_FORWARDED], kept);
        wave_count(&S.stats[KSS_DROPPED], dropped);
    }
}

// where[i] = the table position of response i's entry, ~0u without one
__global__ __launch_bounds__(kBlock) void ksess_probe_kernel(KafkaSessBatch B, KafkaSessions S,
                                                             uint32_t *__restrict__ where) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < B.n; i += (uint64_t)gridDim.x * kBlock) {
        uint32_t at = ~0u;
        if (sess_item(B, S.nslots, PROTO_KAFKA, (uint32_t)i)) {
            const uint32_t ci = B.conn_ids[i];
            const uint32_t id = B.lens[i] >= 8 ? be_bytes(B.arena + B.offs[i] + 4, 4) : 0;
            KafkaSessEntry *e = ksess_find(S.tab, S.mask, sess_claim_of(ci, S.slots[ci].gen), ci, id);
            if (e) {
                at = (uint32_t)(e - S.tab);
                atomicMin(&e->taker, (uint32_t)i);
            }
        }
        where[i] = at;
    }
}

__global__ __launch_bounds__(kBlock) void ksess_take_kernel(KafkaSessBatch B, KafkaSessions S,
                                                            const uint32_t *__restrict__ where,
                                                            uint8_t *__restrict__ found, uint32_t *__restrict__ orig_id,
                                                            int16_t *__restrict__ api_key,
                                                            int16_t *__restrict__ api_version,
                                                            uint64_t *__restrict__ tag) {
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < B.n; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = base + threadIdx.x;
        bool hit = false;
        if (i < B.n) {
            const uint32_t at = where[i];
            KafkaSessEntry *e = at != ~0u ? &S.tab[at] : nullptr;
            hit = e && e->taker == (uint32_t)i;
            if (hit && B.lens[i] >= 8) put_be32(B.arena + B.offs[i] + 4, e->orig);
            found[i] = hit ? 1 : 0;
            orig_id[i] = hit ? e->orig : 0;
            api_key[i] = hit ? e->api_key : (int16_t)0;
            api_version[i] = hit ? e->api_version : (int16_t)0;
            tag[i] = hit ? e->tag : 0;
            if (hit) ksess_delete(e);  // (the other responses on this entry read its taker word only)
        }
        wave_count(&S.stats[KSS_FOUND], hit);
        wave_count(&S.stats[KSS_MISSED], i < B.n && !hit);
    }
}

// S.spare is zeroed: every entry of S.tab that still resolves and is younger
// than lifetime_ms moves over; *expired counts the live ones that were not.
__global__ __launch_bounds__(kBlock) void ksess_gc_kernel(KafkaSessions S, uint64_t now_ms, uint64_t lifetime_ms,
                                                          unsigned long long *__restrict__ expired) {
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base <= S.mask; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t p = base + threadIdx.x;
        bool old = false;
        if (p <= S.mask) {
            const KafkaSessEntry *e = &S.tab[p];
            const unsigned long long c = e->claim;
            if (c != 0 && sess_claim_live(S.slots, S.nslots, c)) {
                const uint64_t age = now_ms > e->created_ms ? now_ms - e->created_ms : 0;
                old = age >= lifetime_ms;
                if (!old) {
                    // (the spare table has the capacity of this one: a slot is always found)
                    KafkaSessEntry *d = ksess_claim(S, S.spare, c, (uint32_t)(c >> 32) - 1u, e->id);
                    if (d) {
                        d->id = e->id;
                        d->orig = e->orig;
                        d->api_key = e->api_key;
                        d->api_version = e->api_version;
                        d->taker = kKafkaSessNoTaker;
                        d->tag = e->tag;
                        d->created_ms = e->created_ms;
                    }
                }
            }
        }
        wave_count(expired, old);
    }
}

// New-connection events: the slot's generation moves on (its entries stop
// resolving at once and become claimable), its numbering restarts at 1.
__global__ __launch_bounds__(kBlock) void ksess_reset_kernel(KafkaSessions S, const uint32_t *__restrict__ conn,
                                                             uint32_t n) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n || conn[k] >= S.nslots) return;
    // (an index named twice is bumped by either lane or both: any new generation serves)
    atomicAdd(&S.slots[conn[k]].gen, 1u);
    S.slots[conn[k]].seq = 0;
}

// out[0]: entries that still resolve; out[1]: slots that are not never-used
__global__ __launch_bounds__(kBlock) void ksess_live_kernel(KafkaSessions S, unsigned long long *__restrict__ out) {
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base <= S.mask; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t p = base + threadIdx.x;
        const unsigned long long c = p <= S.mask ? S.tab[p].claim : 0;
        wave_count(&out[0], c != 0 && sess_claim_live(S.slots, S.nslots, c));
        wave_count(&out[1], c != 0);
    }
}

size_t KafkaSessForwardScratchBytes(uint32_t n, uint32_t nconns) {
    size_t temp = 0;
    if (n > 0x7FFFFFFFu ||
        hipcub::DeviceRadixSort::SortKeys(nullptr, temp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0,
                                          32 + ConnBits(nconns)) != hipSuccess)
        return 0;
    return KafkaForwardLayout(n, nconns, temp).total;
}

hipError_t LaunchKafkaSessForward(const KafkaSessBatch &B, const KafkaSessions &S, const uint8_t *verdict,
                                  const uint64_t *tag, uint64_t now_ms, uint8_t *fwd, uint32_t *new_id, void *scratch,
                                  size_t scratch_bytes, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const KafkaForwardScratch L = KafkaForwardLayout(B.n, B.nconns, 0);
    if (scratch_bytes < L.temp) return hipErrorInvalidValue;
    uint8_t *base = (uint8_t *)scratch;
    uint64_t *keys = (uint64_t *)(base + L.keys), *sorted = (uint64_t *)(base + L.sorted);
    uint2 *seg = (uint2 *)(base + L.seg);
    void *temp = base + L.temp;
    size_t temp_bytes = scratch_bytes - L.temp;
    const dim3 grid = GridFor(B.n), block(kBlock);
    hipLaunchKernelGGL(ksess_keys_kernel, grid, block, 0, stream, B, S, verdict, keys, fwd, new_id);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    // (the index is part of the key: batch order inside a connection does not lean on a stable sort)
    rc = hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, keys, sorted, (int)B.n, 0, 32 + ConnBits(B.nconns), stream);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(ksess_heads_kernel, grid, block, 0, stream, B, S, (const uint64_t *)sorted, seg);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    hipLaunchKernelGGL(ksess_insert_kernel, grid, block, 0, stream, B, S, (const uint64_t *)sorted, (const uint2 *)seg,
                       tag, now_ms, fwd, new_id);
    return hipGetLastError();
}

size_t KafkaSessResponsesScratchBytes(uint32_t n) { return KafkaResponsesLayout(n).total; }

hipError_t LaunchKafkaSessResponses(const KafkaSessBatch &B, const KafkaSessions &S, uint8_t *found, uint32_t *orig_id,
                                    int16_t *api_key, int16_t *api_version, uint64_t *tag, void *scratch,
                                    size_t scratch_bytes, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const KafkaResponsesScratch L = KafkaResponsesLayout(B.n);
    if (scratch_bytes < L.total) return hipErrorInvalidValue;
    uint32_t *where = (uint32_t *)((uint8_t *)scratch + L.where);
    const dim3 grid = GridFor(B.n), block(kBlock);
    hipLaunchKernelGGL(ksess_probe_kernel, grid, block, 0, stream, B, S, where);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(ksess_take_kernel, grid, block, 0, stream, B, S, (const uint32_t *)where, found, orig_id, api_key,
                       api_version, tag);
    return hipGetLastError();
}

hipError_t LaunchKafkaSessGc(const KafkaSessions &S, uint64_t now_ms, uint64_t lifetime_ms, unsigned long long *expired,
                             hipStream_t stream) {
    hipLaunchKernelGGL(ksess_gc_kernel, GridFor((uint64_t)S.mask + 1), dim3(kBlock), 0, stream, S, now_ms, lifetime_ms,
                       expired);
    return hipGetLastError();
}

hipError_t LaunchKafkaSessReset(const KafkaSessions &S, const uint32_t *conn, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ksess_reset_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, S, conn, n);
    return hipGetLastError();
}

hipError_t LaunchKafkaSessLive(const KafkaSessions &S, unsigned long long *out2, hipStream_t stream) {
    hipLaunchKernelGGL(ksess_live_kernel, GridFor((uint64_t)S.mask + 1), dim3(kBlock), 0, stream, S, out2);
    return hipGetLastError();
}

}  // namespace l7

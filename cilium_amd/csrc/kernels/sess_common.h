// What the session kernels of every protocol share on the device
// (kafka_session.hip, memcached_session.hip, cassandra_session.hip and the
// probes in kafka_session.h / cass_session.h): the launch geometry, the
// per-wave statistics add, the sorted (connection, index) keys and their
// segments, the claim word of the open-addressing tables and the batch
// predicate.  A protocol's file keeps its own logic: what takes part, what a
// segment's head does, how its table is probed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../device_tables.h"
#include "sess_scratch.h"

namespace l7 {

constexpr int kSessBlock = 256;
constexpr uint32_t kSessMaxBlocks = 4096;  // every capped grid's ceiling; grid-stride above it

inline dim3 GridFor(uint64_t n) {
    return dim3((uint32_t)std::min<uint64_t>((n + kSessBlock - 1) / kSessBlock, kSessMaxBlocks));
}

// bits of a connection index, the value nconns (the keys of items that take no part) included
inline int ConnBits(uint32_t nconns) {
    int b = 1;
    while (b < 32 && (nconns >> b)) b++;
    return b;
}

// *w += the lanes of the wave with pred set (every lane of the wave calls it)
__device__ __forceinline__ void wave_count(unsigned long long *w, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m && __lane_id() == (unsigned)__ffsll((long long)m) - 1u) atomicAdd(w, (unsigned long long)__popcll(m));
}

// Sorted keys.  An item that takes part has the key (connection << 32 | index):
// a radix sort leaves every connection's items adjacent (its segment) and in
// batch order, without leaning on a stable sort.  The others get a key past
// every segment, by one of two conventions, each with its sort bit range:
//   Kafka, memcached: nconns << 32 | index   (bits 0 .. 32 + ConnBits(nconns))
//   cassandra:        ~0                     (all 64 bits)
// so a walker tests key_conn(k) < nconns, or k != ~0, before it takes k for a segment's.
__device__ __forceinline__ uint64_t sess_key(uint32_t ci, uint32_t i) { return (uint64_t)ci << 32 | i; }
__device__ __forceinline__ uint32_t key_conn(uint64_t k) { return (uint32_t)(k >> 32); }
__device__ __forceinline__ uint32_t key_index(uint64_t k) { return (uint32_t)k; }

// Is sorted[j] the first key of its connection?  (ci: that connection, from a caller that holds it)
__device__ __forceinline__ bool segment_head(const uint64_t *__restrict__ sorted, uint64_t j, uint32_t ci) {
    return j == 0 || key_conn(sorted[j - 1]) != ci;
}
__device__ __forceinline__ bool segment_head(const uint64_t *__restrict__ sorted, uint64_t j) {
    return segment_head(sorted, j, key_conn(sorted[j]));
}

// The first position past the keys of connection ci, whose segment holds sorted[j] (j < n)
__device__ __forceinline__ uint64_t segment_end(const uint64_t *__restrict__ sorted, uint64_t j, uint64_t n,
                                                uint32_t ci) {
    uint64_t lo = j + 1, hi = n;
    while (lo < hi) {
        const uint64_t m = lo + (hi - lo) / 2;
        if (key_conn(sorted[m]) == ci) lo = m + 1; else hi = m;
    }
    return lo;
}

// The claim word of a table entry: (connection + 1) << 32 | the generation of
// the connection's slot when the entry was claimed; 0 = never used.  A word
// whose generation is no longer its slot's has stopped resolving (the
// connection was reset) and its entry may be claimed again.
__device__ __forceinline__ unsigned long long sess_claim_of(uint32_t ci, uint32_t gen) {
    return (unsigned long long)(ci + 1ull) << 32 | gen;
}
// (of an entry another lane may be claiming: an agent-scope relaxed load)
template <class Entry>
__device__ __forceinline__ unsigned long long sess_claim_load(const Entry *e) {
    return __hip_atomic_load(&e->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Does claim word c (not 0) still resolve?  A value that names no connection (a
// protocol's deleted marker) reads as stale, like a claim of a connection that moved on.
template <class Slot>
__device__ __forceinline__ bool sess_claim_live(const Slot *slots, uint32_t nslots, unsigned long long c) {
    const uint32_t cj = (uint32_t)(c >> 32) - 1u;
    return cj < nslots && slots[cj].gen == (uint32_t)c;
}

// item i of a batch (device_tables.h SessBatchT): on a connection of `proto` that has a slot, its bytes inside the arena
template <class Byte>
__device__ __forceinline__ bool sess_item(const SessBatchT<Byte> &B, uint32_t nslots, uint32_t proto, uint32_t i) {
    const uint32_t ci = B.conn_ids[i];
    return ci < B.nconns && ci < nslots && B.conns[ci].proto == proto && l7_in_arena(B.offs[i], B.lens[i], B.arena_len);
}

}  // namespace l7

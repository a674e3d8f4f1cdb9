// The in-flight table of the Kafka sessions (device_tables.h KafkaSessEntry):
// the probe, the claim and the delete that kernels/kafka_session.hip shares
// between its forward, response and collection kernels.
//
// Who writes what: an entry is claimed by a CAS on its claim word, and its
// payload is written by the lane that won that CAS, in the same kernel, and by
// no other.  A lane that probes past an entry it did not claim reads of it
// only the claim word (an agent-scope atomic load); payloads are read by
// later kernels alone.  Kernel boundaries on the caller's stream are the only
// ordering between the two.  The claim word itself is sess_common.h's; the
// deleted value (kKafkaSessDeleted) names no connection, so it reads as stale.
#pragma once
#include "sess_common.h"

namespace l7 {

__device__ __forceinline__ uint32_t ksess_hash(uint32_t ci, uint32_t id) {
    // (sequence numbers of one connection are consecutive: the multiply spreads
    // them, the connection moves the whole run; the table index is the low bits)
    uint32_t h = id * 0x9E3779B1u + ci * 0x85EBCA6Bu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 13;
    return h;
}

// The entry of (mine, id) in tab, or null.  Only a never-used slot ends the chain.
__device__ inline KafkaSessEntry *ksess_find(KafkaSessEntry *tab, uint32_t mask, unsigned long long mine, uint32_t ci,
                                             uint32_t id) {
    uint32_t p = ksess_hash(ci, id) & mask;
    for (uint32_t k = 0; k <= mask; k++, p = (p + 1) & mask) {
        const unsigned long long c = sess_claim_load(&tab[p]);
        if (c == 0) return nullptr;
        if (c == mine && tab[p].id == id) return &tab[p];
    }
    return nullptr;
}

// Claims the first claimable slot of (ci, id)'s chain for `mine`: a never-used
// one, a deleted one, or one of a stale generation.  The ids a connection
// inserts are distinct, so the chain is not searched for the key first.  A lane
// that loses the CAS lost it to a live claim and moves on.  Null: no slot.
__device__ inline KafkaSessEntry *ksess_claim(const KafkaSessions &S, KafkaSessEntry *tab, unsigned long long mine,
                                              uint32_t ci, uint32_t id) {
    uint32_t p = ksess_hash(ci, id) & S.mask;
    for (uint32_t k = 0; k <= S.mask; k++, p = (p + 1) & S.mask) {
        const unsigned long long c = sess_claim_load(&tab[p]);
        if (c != 0 && sess_claim_live(S.slots, S.nslots, c)) continue;
        if (atomicCAS(&tab[p].claim, c, mine) == c) return &tab[p];
    }
    return nullptr;
}

__device__ __forceinline__ void ksess_delete(KafkaSessEntry *e) {
    __hip_atomic_store(&e->claim, kKafkaSessDeleted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace l7

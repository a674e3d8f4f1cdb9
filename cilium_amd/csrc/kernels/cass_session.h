// The statement tables of the cassandra sessions (device_tables.h CassEntry):
// the probe shared by the classifier's EXECUTE lookup (read-only) and the
// commit kernels' upserts (kernels/cassandra_session.hip).
//
// Who writes what: an entry is claimed by a CAS on its claim word, which
// carries the connection, and from then on only lanes of that connection's
// commit walk touch it -- one lane per connection and kernel.  So a lane reads
// its own connection's entries with plain loads, and of every other entry only
// the claim word (an agent-scope atomic load).  Tables are never written while
// a kernel looks statements up for verdicts: kernel boundaries on the caller's
// stream are the only ordering between the two.  The claim word itself is
// sess_common.h's.
#pragma once
#include "cass_frame.h"
#include "sess_common.h"

namespace l7 {

__device__ __forceinline__ uint32_t cass_key_hash(uint32_t ci, const uint8_t *key, uint32_t n) {
    uint32_t h = kFnvBasis;
    for (int k = 0; k < 4; k++) h = (h ^ ((ci >> (8 * k)) & 0xFF)) * 16777619u;
    for (uint32_t k = 0; k < n; k++) h = (h ^ key[k]) * 16777619u;
    h ^= h >> 16;  // (the table index is the low bits)
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    return h;
}

__device__ __forceinline__ bool cass_key_eq(const CassEntry *e, const uint8_t *key, uint32_t n) {
    if (e->key_len != n) return false;
    for (uint32_t k = 0; k < n; k++)
        if (e->key[k] != key[k]) return false;  // the whole key, never the hash alone
    return true;
}

// The entry of (mine, key), or null.  A never-used slot ends the chain.
__device__ inline CassEntry *cass_find(CassEntry *tab, uint32_t mask, unsigned long long mine, uint32_t ci,
                                       const uint8_t *key, uint32_t n) {
    uint32_t p = cass_key_hash(ci, key, n) & mask;
    for (uint32_t k = 0; k <= mask; k++, p = (p + 1) & mask) {
        const unsigned long long c = sess_claim_load(&tab[p]);
        if (c == 0) return nullptr;
        if (c == mine && cass_key_eq(&tab[p], key, n)) return &tab[p];
    }
    return nullptr;
}

// The entry of (mine, key) for its connection's lane to fill: the one that
// exists, else (the whole chain searched first, so a key never lies twice) a
// claimed slot -- the first never-used one or one whose connection has moved
// to another generation -- with the key stored; null = the table is full.
__device__ inline CassEntry *cass_upsert(CassEntry *tab, uint32_t mask, const CassSlot *slots, uint32_t nslots,
                                         unsigned long long mine, uint32_t ci, const uint8_t *key, uint32_t n) {
    const uint32_t h = cass_key_hash(ci, key, n) & mask;
    for (;;) {
        uint32_t p = h;
        bool have = false;
        uint32_t cand = 0;
        unsigned long long cand_claim = 0;
        for (uint32_t k = 0; k <= mask; k++, p = (p + 1) & mask) {
            const unsigned long long c = sess_claim_load(&tab[p]);
            if (c == mine) {
                if (cass_key_eq(&tab[p], key, n)) return &tab[p];
                continue;
            }
            if (c == 0) {
                if (!have) { have = true; cand = p; cand_claim = 0; }
                break;
            }
            if (!have) {
                if (!sess_claim_live(slots, nslots, c)) { have = true; cand = p; cand_claim = c; }
            }
        }
        if (!have) return nullptr;
        if (atomicCAS(&tab[cand].claim, cand_claim, mine) == cand_claim) {
            CassEntry *e = &tab[cand];
            e->key_len = n;
            for (uint32_t k = 0; k < n; k++) e->key[k] = key[k];
            return e;
        }
        // another connection's lane claimed it first: search again
    }
}

}  // namespace l7

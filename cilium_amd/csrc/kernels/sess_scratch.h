// The scratch layouts of the session calls, each stated once: the
// ...ScratchBytes function that sizes a call's buffer and the launcher that
// carves it both ask the layout function here, so a region cannot be added to
// one and not the other.  Plain C++ (no HIP header): the host test of the
// layouts (tests/native/sess_scratch_main.cc) compiles it alone.
//
// Every region starts 256-byte aligned; the arrays indexed by a request carry
// 256 bytes of slack, the per-connection ones an entry for the value nconns.
// `temp` is where the library's temp storage (the sort's, the scan's) starts,
// which is also the least a launcher needs; `total` adds Align256(temp_bytes).
#pragma once
#include <cstddef>
#include <cstdint>

namespace l7 {

inline size_t Align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Regions off the front of a buffer, in the order they are taken.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t off = at;
        at += Align256(bytes);
        return off;
    }
};
inline size_t PerRequest(uint32_t n, size_t elem) { return (size_t)n * elem + 256; }

// element sizes the layouts assume (the kernels' files assert them)
constexpr size_t kKafkaSegBytes = 8, kMcScanBytes = 16, kMcSegBytes = 16;  // uint2, McScan, McSeg

// (braced lists evaluate left to right: the members are carved in the order they are declared)

// l7g_kafka_forward: keys[n], sorted[n], seg[nconns + 1], the sort's temp
struct KafkaForwardScratch { size_t keys, sorted, seg, temp, total; };
inline KafkaForwardScratch KafkaForwardLayout(uint32_t n, uint32_t nconns, size_t temp_bytes) {
    Carve c;
    return {c.take(PerRequest(n, 8)), c.take(PerRequest(n, 8)), c.take(((size_t)nconns + 1) * kKafkaSegBytes),
            c.take(temp_bytes), c.at};
}

// l7g_mc_forward: keys[n], sorted[n], info[n], el[n], sc[n], seg[nconns + 1], the larger temp of sort and scan
struct McForwardScratch { size_t keys, sorted, info, el, sc, seg, temp, total; };
inline McForwardScratch McForwardLayout(uint32_t n, uint32_t nconns, size_t temp_bytes) {
    Carve c;
    return {c.take(PerRequest(n, 8)), c.take(PerRequest(n, 8)), c.take(PerRequest(n, 1)),
            c.take(PerRequest(n, kMcScanBytes)), c.take(PerRequest(n, kMcScanBytes)),
            c.take(((size_t)nconns + 1) * kMcSegBytes), c.take(temp_bytes), c.at};
}

// l7g_kafka_responses: where[n]
struct KafkaResponsesScratch { size_t where, total; };
inline KafkaResponsesScratch KafkaResponsesLayout(uint32_t n) {
    Carve c;
    return {c.take(PerRequest(n, 4)), c.at};
}

// The cassandra classifier and l7g_cass_replies: keys[n], sorted[n], the sort's temp; with sessions the PREPARE
// marks and their sorted copy lie between (without: pkeys = psorted = temp, no regions).
struct CassandraScratch { size_t keys, sorted, pkeys, psorted, temp, total; };
inline CassandraScratch CassandraLayout(uint32_t n, bool sessions, size_t temp_bytes) {
    Carve c;
    return {c.take(PerRequest(n, 8)), c.take(PerRequest(n, 8)), sessions ? c.take(PerRequest(n, 8)) : c.at,
            sessions ? c.take(PerRequest(n, 8)) : c.at, c.take(temp_bytes), c.at};
}

}  // namespace l7

// cassandra frame helpers shared by the request classifier
// (cassandra_classify.hip) and the session kernels (cassandra_session.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../device_tables.h"

namespace l7 {

constexpr uint32_t kCassMaxLen = 268435456u;  // cassMaxLen (cassandraparser.go:56)

__device__ __forceinline__ uint32_t cass_be32(const uint8_t *b) {
    return (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
}
__device__ __forceinline__ uint32_t cass_be16(const uint8_t *b) { return (uint32_t)b[0] << 8 | b[1]; }

// The frame at b (len bytes of buffer): true for a complete request-direction
// frame (op / fl set), else false with the framing outcome in verdict / consumed.
struct CassFrame {
    uint8_t verdict;     // V_* when not a request frame
    uint32_t consumed;
    uint32_t fl;         // frame length
    uint8_t op;
};
__device__ __forceinline__ bool cass_frame_of(const uint8_t *b, uint32_t len, CassFrame *F) {
    F->consumed = 0;
    F->fl = 0;
    F->op = 0;
    if (len < 9) { F->verdict = V_INCOMPLETE; F->consumed = 9 - len; return false; }
    const uint32_t rl = cass_be32(b + 5);
    if (rl > kCassMaxLen) { F->verdict = V_PARSE_ERROR; F->consumed = 3; return false; }
    const uint32_t fl = 9 + rl;
    if (fl > len) { F->verdict = V_INCOMPLETE; F->consumed = fl - len; return false; }
    F->fl = fl;
    if ((b[0] & 0x80) || (b[1] & 0x01)) { F->verdict = V_PARSE_ERROR; F->consumed = 2; return false; }
    F->op = b[4];
    return true;
}

// QUERY / PREPARE: the long string at 9; false = the slice expressions panic.
// The frame is data[0:fl] of the bytes.Join buffer (cassandraparser.go:174,
// :211); Go bounds data[9:13] and data[13:13+ql] by the slice's capacity, so
// they read on into the bytes after the frame and panic only past the
// buffer's end (cap = the request's buffer length; a single-slice join's
// allocator slack is not restated: parity unpinned, oracle/cassandra_ref.c).
__device__ __forceinline__ bool cass_query_of(const uint8_t *b, uint32_t cap, uint32_t *qn) {
    if (cap < 13) return false;
    const uint32_t ql = cass_be32(b + 9);
    const uint32_t end = 13u + ql;  // uint32 arithmetic, as in Go
    if (end < 13u || end > cap) return false;
    *qn = ql;
    return true;
}

// The last key of connection ci below (ci << 32 | i) among the n sorted keys
// (connection << 32 | request index; ~0 = none): that request's index, or -1.
__device__ __forceinline__ int64_t cass_last_before(const uint64_t *__restrict__ keys, uint32_t n, uint32_t ci,
                                                    uint32_t i) {
    const uint64_t probe = (uint64_t)ci << 32 | i;
    uint32_t lo = 0, hi = n;  // first key >= probe
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < probe) lo = mid + 1; else hi = mid;
    }
    if (lo > 0 && (keys[lo - 1] >> 32) == ci) return (int64_t)(keys[lo - 1] & 0xFFFFFFFFu);
    return -1;
}

}  // namespace l7

// Access-log records of HTTP requests on gfx950 (product code): the post-pass
// of the logged calls (l7g_classify_logged), launched after the classifiers on
// the same stream.
//
// It reads verdict[] and handles only the requests of HTTP connections that a
// classifier answered ALLOW or DENY.  Their heads are known to satisfy the
// framing contract: no CR, LF or other CTL inside a token or a
// value, so every CR before the empty line ends a line, the first two SPs are
// the request line's, and a header name runs up to its ':'.  The kernel
// therefore validates nothing.  It locates the two SPs, the CRs, the empty
// line and the first line named "host", and writes the record (LogRec,
// device_tables.h).  Requests of every other connection but Kafka's (whose
// records kafka_classify_kernel<., true> writes) and HTTP requests with any
// other verdict get kind 0.
//
// A team of 16 lanes per request: each lane loads one aligned 16-byte chunk of
// a 256-byte window and makes 16-bit CR / SP masks of it; the team merges what
// it needs with width-16 shuffles (the first SPs, the first CR that follows a
// CR two bytes before, the CRs counted) and takes further windows until the
// empty line is found, so only the head is fetched, not the body.  Lanes whose
// chunk holds a line's CR test the next line's name with byte loads (bytes the
// team has just fetched).  No lane fetches a chunk outside
// [first byte & ~15, (last byte + 16) & ~15): the arena is only readable to
// the next 16-byte boundary.  Plain vector stores, no atomics, no LDS.
#include <hip/hip_runtime.h>

#include "../device_tables.h"
#include "gmem.h"
#include "launch.h"

namespace l7 {

namespace {

constexpr int kBlock = 256;
constexpr int kTeam = 16;             // lanes per request
constexpr uint32_t kWin = 16 * kTeam;  // bytes per window
constexpr uint32_t kNone = ~0u;
// positions are 32-bit offsets from the first chunk; a head reaching past this is not looked for
constexpr uint64_t kMaxScan = 0x7FFFFF00ull;

// bit k = byte k of the word equals the byte replicated in rep
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t rep) {
    const uint32_t x = w ^ rep;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where the byte is 0
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
__device__ __forceinline__ uint32_t eq16(const uint4 &w, uint32_t c) {
    const uint32_t rep = c * 0x01010101u;
    return eq4(w.x, rep) | (eq4(w.y, rep) << 4) | (eq4(w.z, rep) << 8) | (eq4(w.w, rep) << 12);
}
__device__ __forceinline__ uint32_t team_min(uint32_t v) {
#pragma unroll
    for (int m = kTeam / 2; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, kTeam);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t team_sum(uint32_t v) {
#pragma unroll
    for (int m = kTeam / 2; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, kTeam);
    return v;
}
// the chunk's mask bits at positions after p (cq: the chunk's first position)
__device__ __forceinline__ uint32_t after(uint32_t m, uint32_t cq, uint32_t p) {
    if (p < cq) return m;
    if (p - cq >= 15) return 0;
    return m & ~((2u << (p - cq)) - 1u);
}
__device__ __forceinline__ uint32_t first_pos(uint32_t m, uint32_t cq) {
    return m ? cq + (uint32_t)__builtin_ctz(m) : kNone;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void http_log_kernel(Batch B, LogRec *__restrict__ rec) {
    const uint32_t t = threadIdx.x & (kTeam - 1);
    const uint64_t team = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) / kTeam;
    if (team >= B.n) return;
    const uint32_t i = (uint32_t)team;
    const uint32_t ci = B.conn_ids[i];
    const uint8_t proto = ci < B.nconns ? B.conns[ci].proto : (uint8_t)PROTO_NONE;
    if (proto == PROTO_KAFKA) return;  // the Kafka classifier's record
    uint4 r0 = make_uint4(LOG_NONE, 0, 0, 0), r1 = make_uint4(0, 0, 0, 0);
    const uint8_t v = B.verdict[i];
    const uint64_t off = B.offs[i];
    const uint32_t len = B.lens[i];
    if (proto == PROTO_HTTP && (v == V_ALLOW || v == V_DENY) && len && l7_in_arena(off, len, B.arena_len)) {
        const uint64_t a0 = (uint64_t)(uintptr_t)B.arena + off;
        const uint64_t base = a0 & ~15ull;
        const uint32_t lead = (uint32_t)(a0 & 15);  // position of the request's first byte
        const uint64_t qe = (uint64_t)lead + len;   // position past its last byte
        const uint32_t qend = (uint32_t)(qe < kMaxScan ? qe : kMaxScan);
        const uint8_t *b = B.arena + off - lead;    // b[q]: the byte at position q (read for lead <= q < qend only)
        uint32_t sp1 = kNone, sp2 = kNone, endcr = kNone, host_s = kNone, host_cr = kNone, ncr = 0;
        uint32_t carry = 0;  // the CR mask of the chunk before this window
        for (uint32_t wq = 0; wq < qend && endcr == kNone; wq += kWin) {
            const uint32_t cq = wq + 16 * t;
            uint4 w = make_uint4(0, 0, 0, 0);
            uint32_t vm = 0;  // bytes of this chunk inside the request
            if (cq < qend) {
                w = gload16(base + cq);
                const uint32_t lo = cq >= lead ? 0u : lead - cq;
                const uint32_t hi = qend - cq >= 16 ? 16u : qend - cq;
                vm = (0xFFFFu << lo) & (0xFFFFu >> (16 - hi));
            }
            const uint32_t cr = eq16(w, '\r') & vm, sp = eq16(w, ' ') & vm;
            // the empty line: a CR two bytes after a CR (bits 14, 15 of the chunk before carry over)
            uint32_t prev = (uint32_t)__shfl_up((int)cr, 1, kTeam);
            if (t == 0) prev = carry;
            const uint32_t two_back = ((cr << 2) | (prev >> 14)) & 0xFFFFu;
            endcr = team_min(first_pos(cr & two_back, cq));
            // the lines' CRs up to the empty line's
            const uint32_t crs = endcr == kNone ? cr : cr & ~after(cr, cq, endcr);
            ncr += team_sum((uint32_t)__builtin_popcount(crs));
            if (sp2 == kNone) {
                if (sp1 == kNone) sp1 = team_min(first_pos(sp, cq));
                if (sp1 != kNone) sp2 = team_min(first_pos(after(sp, cq, sp1), cq));
            }
            if (host_s == kNone) {
                // the lines that start two bytes after one of this chunk's CRs (not the empty line's)
                uint32_t m = endcr == kNone ? crs : crs & ~after(crs, cq, endcr - 1);
                uint32_t cand = kNone;
                while (m && cand == kNone) {
                    const uint32_t s = cq + (uint32_t)__builtin_ctz(m) + 2;
                    m &= m - 1;
                    if (s + 5 <= qend && (b[s] | 0x20) == 'h' && (b[s + 1] | 0x20) == 'o' && (b[s + 2] | 0x20) == 's' &&
                        (b[s + 3] | 0x20) == 't' && b[s + 4] == ':')
                        cand = s;
                }
                host_s = team_min(cand);
            }
            if (host_s != kNone && host_cr == kNone) host_cr = team_min(first_pos(after(cr, cq, host_s), cq));
            carry = (uint32_t)__shfl((int)cr, kTeam - 1, kTeam);
        }
        if (t == 0 && endcr != kNone && sp2 != kNone && sp2 + 9 <= qend && ncr >= 2) {
            uint32_t flags = 0, ho = 0, hl = 0;
            if (host_s != kNone && host_cr != kNone) {
                uint32_t vs = host_s + 5, ve = host_cr;
                while (vs < ve && (b[vs] == ' ' || b[vs] == '\t')) vs++;
                while (ve > vs && (b[ve - 1] == ' ' || b[ve - 1] == '\t')) ve--;
                flags = 1;
                ho = vs - lead;
                hl = ve - vs;
            }
            // "HTTP/x.y" follows the second SP
            const uint32_t ver = (((uint32_t)b[sp2 + 6] - '0') << 4) | (((uint32_t)b[sp2 + 8] - '0') & 15u);
            r0 = make_uint4(LOG_HTTP | (flags << 8) | ((ver & 0xFFu) << 16), sp1 - lead, sp2 - sp1 - 1, ho);
            r1 = make_uint4(hl, endcr + 2 - lead, ncr - 2, 0);
        }
    }
    if (t == 0) {
        uint4 *o = reinterpret_cast<uint4 *>(rec + i);
        o[0] = r0;
        o[1] = r1;
    }
}

hipError_t LaunchHttpLog(const Batch &B, LogRec *rec, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const uint32_t per_block = kBlock / kTeam;
    const uint32_t blocks = (B.n + per_block - 1) / per_block;  // (n = 2^32 - 1: 2^28 workgroups)
    hipLaunchKernelGGL(http_log_kernel, dim3(blocks), dim3(kBlock), 0, stream, B, rec);
    return hipGetLastError();
}

}  // namespace l7

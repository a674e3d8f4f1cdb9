// What the kernels of the memcached sessions share (kernels/memcached_session.hip):
// the 16-byte window a lane reads a request or a reply's first token through,
// the walk of a text request's first line (text/parser.go:87-162), a wave's
// search for a reply line's "\r\n" and for "\r\nEND\r\n" (:203-273), and the
// element of the forward call's segmented scan.
//
// The window reads as text_bytes.h's Reader does (aligned 16-byte loads, never
// outside [first byte & ~15, (last byte + 16) & ~15) of what the lane walks)
// and holds the 16 bytes as two 64-bit halves: see mcs_rd.
#pragma once
#include "../device_tables.h"
#include "gmem.h"
#include "text_bytes.h"

namespace l7 {

constexpr uint32_t kMcSessWindow = 16;  // bytes a lane holds in registers
constexpr uint32_t kMcSessStep = 64;    // bytes a wave of the reply kernel looks at per step (cilium_amd/_lib.py mirrors it)

// One request of l7g_mc_forward as the keys kernel leaves it (0: takes no part)
enum : uint8_t {
    MCI_CLS = 3,        // MCC_*
    MCI_NOREPLY = 4,
    MCI_WATCH = 8,
    MCI_BINARY = 16,    // the parser l7g_classify used
    MCI_DENY = 32,      // the verdict (else ALLOW)
    MCI_VALID = 64,
};

// An element of the forward call's scan over the sorted requests, and the
// operator that composes two adjacent spans.  A span that contains a segment's
// first request (MCS_HEAD) forgets what came before it.
//   text:   c = requests that owe a reply; MCS_E: one of them is an ALLOW;
//           a = the DENYs among them before the first such ALLOW
//   binary: c = requests; a = position (1-based, in the span) of the last
//           ALLOW, 0 = none; d = position of the first DENY, 0 = none
enum : uint32_t { MCS_HEAD = 1, MCS_E = 2, MCS_WATCH = 4, MCS_BIN = 8 };
struct __attribute__((aligned(16))) McScan {
    uint32_t f, c, a, d;
};
struct McScanOp {
    __host__ __device__ __forceinline__ McScan operator()(const McScan &x, const McScan &y) const {
        if (y.f & MCS_HEAD) return y;
        McScan r;
        r.f = x.f | y.f;
        r.c = x.c + y.c;
        if (x.f & MCS_BIN) {
            r.a = y.a ? x.c + y.a : x.a;
            r.d = x.d ? x.d : (y.d ? x.c + y.d : 0u);
        } else {
            r.a = (x.f & MCS_E) ? x.a : x.a + y.a;
            r.d = 0;
        }
        return r;
    }
};

#if defined(__HIPCC__)

struct McReader {
    const uint8_t *b;
    uint64_t base;
    uint64_t lo, hi;  // the window's bytes 0..7 and 8..15
};
__device__ __forceinline__ uint32_t mcs_rd(McReader &r, uint64_t i) {
    const uint64_t a = (uint64_t)(r.b + i);
    const uint64_t base = a & ~(uint64_t)(kMcSessWindow - 1);
    if (base != r.base) {
        const uint4 v = gload16(base);
        r.lo = (uint64_t)v.y << 32 | v.x;
        r.hi = (uint64_t)v.w << 32 | v.z;
        r.base = base;
    }
    // (two shifts, not a choice among four words: that one the compiler keeps as an array in scratch)
    return (uint32_t)(((a & 8) ? r.hi : r.lo) >> ((a & 7) * 8)) & 0xFF;
}

// the first 16 bytes of a token, packed little-endian, and its length
struct McTok {
    uint32_t t0, t1, t2, t3, len;
};
__device__ __forceinline__ void mcs_tok_add(McTok &t, uint32_t x) {
    const uint32_t j = t.len++, v = x << ((j & 3) * 8);
    if (j < 4) t.t0 |= v;
    else if (j < 8) t.t1 |= v;
    else if (j < 12) t.t2 |= v;
    else if (j < 16) t.t3 |= v;
}
#define MCS_IS(t, lit)                                                                               \
    ((t).len == sizeof(lit) - 1 && (t).t0 == pk4(lit, sizeof(lit) - 1, 0) &&                         \
     (t).t1 == pk4(lit, sizeof(lit) - 1, 1) && (t).t2 == pk4(lit, sizeof(lit) - 1, 2) &&             \
     (t).t3 == pk4(lit, sizeof(lit) - 1, 3))

// The width of the Unicode White_Space rune at [p, end) whose first byte is c
// (text_bytes.h), 0 = none; the bytes after a lead byte are read where [p, end) holds them.
__device__ __forceinline__ uint32_t mcs_space(McReader &W, uint32_t c, uint64_t p, uint64_t end) {
    if (c < 0x80) return ws_rune_len(c, 0, 0, 1);
    if (ws_lead_len(c) == 2) {
        if (p + 1 < end) return ws_rune_len(c, mcs_rd(W, p + 1), 0, 2);
    } else if (ws_lead_len(c) == 3 && p + 2 < end) {
        const uint32_t c1 = mcs_rd(W, p + 1), c2 = mcs_rd(W, p + 2);
        return ws_rune_len(c, c1, c2, 3);
    }
    return 0;
}

// The first line of [from, end) of what W reads: lf = the position of its
// "\r\n" (end: none), first = its first token, last = its last one, ntok =
// how many it has.  last_cr: the byte at end - 1 is '\r'.
struct McLine {
    uint64_t lf;
    uint32_t ntok;
    bool found, last_cr;
    McTok first, last;
};
__device__ __forceinline__ McLine mcs_line(McReader &W, uint64_t from, uint64_t end) {
    McLine L{end, 0, false, false, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
    McTok cur{0, 0, 0, 0, 0};
    bool in_tok = false;
    uint32_t c = 0;
    for (uint64_t p = from; p < end;) {
        c = mcs_rd(W, p);
        const bool eol = c == '\r' && p + 1 < end && mcs_rd(W, p + 1) == '\n';
        const uint32_t w = eol ? 1u : mcs_space(W, c, p, end);
        if (w) {
            if (in_tok) {
                if (L.ntok++ == 0) L.first = cur;
                L.last = cur;
                in_tok = false;
            }
            if (eol) { L.lf = p; L.found = true; return L; }
            p += w;
        } else {
            if (!in_tok) { in_tok = true; cur = McTok{0, 0, 0, 0, 0}; }
            mcs_tok_add(cur, c);
            p++;
        }
    }
    L.last_cr = end > from && c == '\r';
    return L;
}

// A text request's info byte from its first line (text/parser.go:108-162):
// the reply class of its command, whether it has noreply, whether it is watch.
__device__ __forceinline__ uint32_t mcs_text_request(const McLine &L) {
    if (!L.found || L.ntok == 0) return 0;  // (no classifier answers such a request ALLOW or DENY)
    const McTok &t = L.first;
    const uint32_t pre = t.t0 & 0xFFFFFFu, nt = L.ntok;
    uint32_t cls = MCC_OTHER;
    bool noreply = false, watch = false;
    if (t.len >= 3 && (pre == pk4("get", 3, 0) || pre == pk4("gat", 3, 0))) {
        cls = MCC_END;
    } else if (MCS_IS(t, "set") || MCS_IS(t, "add") || MCS_IS(t, "replace") || MCS_IS(t, "append") ||
               MCS_IS(t, "prepend")) {
        cls = MCC_LINE;
        noreply = nt == 6;
    } else if (MCS_IS(t, "cas")) {
        cls = MCC_LINE;
        noreply = nt == 7;
    } else if (MCS_IS(t, "delete")) {
        cls = MCC_LINE;
        noreply = nt == 3;
    } else if (MCS_IS(t, "incr") || MCS_IS(t, "decr") || MCS_IS(t, "touch")) {
        cls = MCC_LINE;
        noreply = nt == 4;
    } else if (MCS_IS(t, "slabs") || MCS_IS(t, "lru") || MCS_IS(t, "version") || MCS_IS(t, "misbehave")) {
        cls = MCC_LINE;
    } else if (MCS_IS(t, "lru_crawler")) {
        cls = MCC_CRAWLER;
    } else if (MCS_IS(t, "stats")) {
        cls = MCC_END;
    } else if (MCS_IS(t, "flush_all") || MCS_IS(t, "cache_memlimit")) {
        cls = MCC_LINE;
        noreply = MCS_IS(L.last, "noreply");
    } else if (MCS_IS(t, "quit")) {
        noreply = true;
    } else if (MCS_IS(t, "watch")) {
        watch = true;
    }
    return MCI_VALID | cls | (noreply ? MCI_NOREPLY : 0u) | (watch ? MCI_WATCH : 0u);
}

// ---- one wave per reply stream: every lane of the wave calls these with the
// same arguments and gets the same answer.  Lane l looks at byte p + l of a
// 64-byte step (byte loads inside [from, end), coalesced); a ballot finds the
// first hit.

// the first "\r\n" of b[from, end); end = none
__device__ __forceinline__ uint64_t mcs_wave_crlf(const uint8_t *b, uint64_t from, uint64_t end) {
    for (uint64_t p = from; p < end; p += kMcSessStep) {
        const uint64_t q = p + __lane_id();
        const bool hit = q + 1 < end && b[q] == '\r' && b[q + 1] == '\n';
        const unsigned long long m = __ballot(hit);
        if (m) return p + (uint64_t)(__ffsll((long long)m) - 1);
    }
    return end;
}

// bytes.Index(b[from:end], "\r\nEND\r\n") as a position in b; end = none
__device__ __forceinline__ uint64_t mcs_wave_end(const uint8_t *b, uint64_t from, uint64_t end) {
    for (uint64_t p = from; p + 7 <= end; p += kMcSessStep) {
        const uint64_t q = p + __lane_id();
        bool hit = q + 7 <= end && b[q] == '\r';
        if (hit)
            hit = b[q + 1] == '\n' && b[q + 2] == 'E' && b[q + 3] == 'N' && b[q + 4] == 'D' && b[q + 5] == '\r' &&
                  b[q + 6] == '\n';
        const unsigned long long m = __ballot(hit);
        if (m) return p + (uint64_t)(__ffsll((long long)m) - 1);
    }
    return end;
}

// tokens[0] of bytes.Fields(line [from, lf)); len 0 = the line has no token.
// A reply's first token is a few bytes at the line's start: the lanes walk it
// in step, each through its own window.
__device__ __forceinline__ McTok mcs_first_token(McReader &W, uint64_t from, uint64_t lf) {
    McTok t{0, 0, 0, 0, 0};
    uint64_t p = from;
    while (p < lf) {
        const uint32_t w = mcs_space(W, mcs_rd(W, p), p, lf);
        if (!w) break;
        p += w;
    }
    while (p < lf) {
        const uint32_t c = mcs_rd(W, p);
        if (mcs_space(W, c, p, lf)) break;
        mcs_tok_add(t, c);
        p++;
    }
    return t;
}

#endif  // __HIPCC__

}  // namespace l7

// What the memcached / r2d2 text kernels share byte by byte (frame.hip,
// memcache_classify.hip, generic_log.hip, mc_session.h) and, for the separator
// rule, the host scan of proxylib/shim.cc: the Unicode White_Space rune that
// bytes.Fields splits on, a command literal packed into words, the 16-byte
// register window a lane reads a request through, and the per-byte masks of a
// 16-byte chunk.  Nothing here loads on its own account but rd(): a call site
// fetches the bytes it hands to ws_rune_len, inside the range it may read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"

namespace l7 {

// Unicode White_Space (unicode.IsSpace, the runes bytes.Fields splits on), in
// UTF-8: U+0009..000D, U+0020 | U+0085, U+00A0 (C2 85, C2 A0) | U+1680 (E1 9A
// 80) | U+2000..200A, U+2028, U+2029, U+202F (E2 80 80..8A / A8 / A9 / AF) |
// U+205F (E2 81 9F) | U+3000 (E3 80 80).  A multi-byte one starts with a lead
// byte, which never continues another rune, so it is judged on its own bytes.
//
// ws_lead_len: the width a White_Space rune that starts with c0 has (2 or 3),
// 0 if c0 starts no multi-byte one: the bytes after c0 that a site fetches
// before it asks ws_rune_len, where that many lie in its range.
L7_HD inline uint32_t ws_lead_len(uint32_t c0) { return c0 == 0xC2 ? 2u : (c0 >= 0xE1 && c0 <= 0xE3) ? 3u : 0u; }

// The width of the White_Space rune c0 [c1 [c2]] of which `avail` >= 1 bytes
// exist (the line or request ends after them), 0 = none.  c1 is looked at only
// if c0 is a lead byte and avail >= 2, c2 only if c0 is 0xE1..0xE3 and avail >= 3.
L7_HD inline uint32_t ws_rune_len(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t avail) {
    if (c0 < 0x80) return (c0 - 9u < 5u || c0 == ' ') ? 1u : 0u;
    if (c0 == 0xC2) return (avail >= 2 && (c1 == 0x85 || c1 == 0xA0)) ? 2u : 0u;
    if (avail < 3) return 0;
    if ((c0 == 0xE1 && c1 == 0x9A && c2 == 0x80) || (c0 == 0xE3 && c1 == 0x80 && c2 == 0x80) ||
        (c0 == 0xE2 && ((c1 == 0x80 && ((c2 >= 0x80 && c2 <= 0x8A) || c2 == 0xA8 || c2 == 0xA9 || c2 == 0xAF)) ||
                        (c1 == 0x81 && c2 == 0x9F))))
        return 3;
    return 0;
}

// bytes [4w, 4w + 4) of the n-byte literal s packed little-endian (compile-time;
// bytes past n are 0), as a token's first bytes are kept
L7_HD constexpr uint32_t pk4(const char *s, uint32_t n, uint32_t w) {
    return (4 * w + 0 < n ? (uint32_t)(uint8_t)s[4 * w + 0] : 0u) | (4 * w + 1 < n ? (uint32_t)(uint8_t)s[4 * w + 1] << 8 : 0u) |
           (4 * w + 2 < n ? (uint32_t)(uint8_t)s[4 * w + 2] << 16 : 0u) |
           (4 * w + 3 < n ? (uint32_t)(uint8_t)s[4 * w + 3] << 24 : 0u);
}

}  // namespace l7

#if defined(__HIPCC__)
#include "gmem.h"

namespace l7 {

// 16-byte aligned register window over one request: aligned 16-byte loads,
// never outside [first byte & ~15, (last byte + 16) & ~15) of what the lane
// walks (the arena is readable up to the 16-byte boundary after its last byte;
// see include/l7gpu.h).
struct Reader {
    const uint8_t *b;
    uint64_t base;
    uint32_t w0, w1, w2, w3;
};
__device__ __forceinline__ uint32_t rd(Reader &r, uint32_t i) {
    const uint64_t a = (uint64_t)(r.b + i);
    const uint64_t base = a & ~(uint64_t)15;
    if (base != r.base) {
        const uint4 v = gload16(base);  // global, not flat (gmem.h)
        r.w0 = v.x; r.w1 = v.y; r.w2 = v.z; r.w3 = v.w;
        r.base = base;
    }
    const uint32_t k = (uint32_t)(a >> 2) & 3;
    const uint32_t w = k == 0 ? r.w0 : k == 1 ? r.w1 : k == 2 ? r.w2 : r.w3;
    return (w >> ((a & 3) * 8)) & 0xFF;
}

// bit i (0..15) set iff byte i of the chunk equals b (SWAR compare per word,
// the four byte flags of a word gathered by one multiply)
__device__ __forceinline__ uint32_t eq_mask(uint4 w, uint32_t b) {
    const uint32_t bb = b * 0x01010101u;
    auto e = [bb](uint32_t x) {
        const uint32_t t = x ^ bb;
        return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    };
    auto nib = [](uint32_t s) { return __builtin_amdgcn_ubfe((s >> 7) * 0x204081u, 21, 4); };
    return nib(e(w.x)) | nib(e(w.y)) << 4 | nib(e(w.z)) << 8 | nib(e(w.w)) << 12;
}
// bit i set iff byte i is an ASCII white space (0x09..0x0D or 0x20: unicode.IsSpace below 0x80)
__device__ __forceinline__ uint32_t ascii_space_mask(uint4 w) {
    auto sp = [](uint32_t x) {
        const uint32_t t = x & 0x7F7F7F7Fu;
        // 0x09..0x0D: t - 0x09 < 5 per byte (no borrow across bytes: t >= 0 and the high bit is clear)
        const uint32_t ge9 = (t + 0x77777777u) & 0x80808080u;   // t >= 0x09
        const uint32_t ge14 = (t + 0x72727272u) & 0x80808080u;  // t >= 0x0E
        const uint32_t tt = t ^ 0x20202020u;
        const uint32_t is20 = ~(((tt & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | tt) & 0x80808080u;
        return ((ge9 & ~ge14) | is20) & ~x & 0x80808080u;  // high bit of the byte clear
    };
    auto nib = [](uint32_t s) { return __builtin_amdgcn_ubfe((s >> 7) * 0x204081u, 21, 4); };
    return nib(sp(w.x)) | nib(sp(w.y)) << 4 | nib(sp(w.z)) << 8 | nib(sp(w.w)) << 12;
}
// byte q (0..15) of the chunk
__device__ __forceinline__ uint32_t chunk_byte(uint4 w, uint32_t q) {
    const bool upper = (q & 8) != 0;
    const uint32_t lo = upper ? w.z : w.x, hi = upper ? w.w : w.y;
    return __builtin_amdgcn_perm(hi, lo, (q & 7) | 0x0C0C0C00u);
}

}  // namespace l7
#endif

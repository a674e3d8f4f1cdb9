// HTTP classifier, layer 1: byte-class predicates, one byte at a time and SWAR
// over a 16-byte chunk (16-bit masks, bit i = byte i).  Needs nothing below it.
#pragma once
#include <hip/hip_runtime.h>

namespace l7 {

namespace {

__device__ __forceinline__ bool is_tchar(uint32_t c) {
    // tchar = "!#$%&'*+-.^_`|~" / DIGIT / ALPHA  (bitmap over 0x20..0x7F)
    const uint32_t m1 = 0x03FF6CFAu;  // 0x20-0x3F
    const uint32_t m2 = 0xC7FFFFFEu;  // 0x40-0x5F
    const uint32_t m3 = 0x57FFFFFFu;  // 0x60-0x7F
    const uint32_t w = c < 0x40 ? m1 : (c < 0x60 ? m2 : m3);
    return (c - 0x20u < 0x60u) & ((w >> (c & 31)) & 1);
}

// a byte that ends a header value: a CTL other than HT, or DEL (branch-free)
__device__ __forceinline__ bool value_stop(uint32_t c) { return ((c < 0x20) & (c != '\t')) | (c == 0x7F); }

// Per-dword SWAR: bit 7 of byte i set iff byte i < 0x20 or == 0x7F (exact).
__device__ __forceinline__ uint32_t stop_bits(uint32_t x) {
    const uint32_t t = x & 0x7F7F7F7Fu;
    return (~(t + 0x60606060u) | (t + 0x01010101u)) & ~x & 0x80808080u;
}
// bit 7 of each byte -> 4-bit nibble
__device__ __forceinline__ uint32_t nib(uint32_t s) { return __builtin_amdgcn_ubfe((s >> 7) * 0x204081u, 21, 4); }
// 16-bit mask of the stop bytes of a chunk
__device__ __forceinline__ uint32_t stop_mask(uint4 w) {
    return nib(stop_bits(w.x)) | nib(stop_bits(w.y)) << 4 | nib(stop_bits(w.z)) << 8 | nib(stop_bits(w.w)) << 12;
}
// bit 7 of byte i set iff byte i <= 0x20 or == 0x7F (ends a request target)
__device__ __forceinline__ uint32_t tstop_bits(uint32_t x) {
    const uint32_t t = x & 0x7F7F7F7Fu;
    return (~(t + 0x5F5F5F5Fu) | (t + 0x01010101u)) & ~x & 0x80808080u;
}
// bit 7 of byte i set iff byte i ends a header value: < 0x20 other than HT, or DEL
__device__ __forceinline__ uint32_t vstop_bits(uint32_t x) {
    const uint32_t t = x ^ 0x09090909u;  // HT -> 0
    const uint32_t ht = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    return stop_bits(x) & ~ht;
}
// nonzero iff some byte of the chunk is < 0x20 or DEL (HT included: a superset
// of the value stops, for the tile map)
__device__ __forceinline__ uint32_t stop_any(uint4 w) {
    const uint32_t a = w.x & 0x7F7F7F7Fu, b = w.y & 0x7F7F7F7Fu, c = w.z & 0x7F7F7F7Fu, d = w.w & 0x7F7F7F7Fu;
    const uint32_t s = ((~(a + 0x60606060u) | (a + 0x01010101u)) & ~w.x) | ((~(b + 0x60606060u) | (b + 0x01010101u)) & ~w.y) |
                       ((~(c + 0x60606060u) | (c + 0x01010101u)) & ~w.z) | ((~(d + 0x60606060u) | (d + 0x01010101u)) & ~w.w);
    return s & 0x80808080u;
}
// bit 7 of byte i set iff byte i is one of [0-9A-Za-z-] (a subset of tchar)
__device__ __forceinline__ uint32_t alnum_bits(uint32_t x) {
    const uint32_t h = x | 0x80808080u;
    const uint32_t l = x | 0xA0A0A0A0u;  // letters folded to lower case, bit 7 set
    const uint32_t dig = (h - 0x30303030u) & ~(h - 0x3A3A3A3Au);
    const uint32_t let = (l - 0x61616161u) & ~(l - 0x7B7B7B7Bu);
    const uint32_t t = x ^ 0x2D2D2D2Du;  // '-' -> 0
    const uint32_t dash = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t);
    return (dig | let | dash) & ~x & 0x80808080u;
}
// 16-bit mask of the bytes of a chunk that are not [0-9A-Za-z-]
__device__ __forceinline__ uint32_t nonalnum_mask(uint4 w) {
    return (nib(~alnum_bits(w.x) & 0x80808080u) | nib(~alnum_bits(w.y) & 0x80808080u) << 4 |
            nib(~alnum_bits(w.z) & 0x80808080u) << 8 | nib(~alnum_bits(w.w) & 0x80808080u) << 12);
}
__device__ __forceinline__ uint32_t tstop_mask(uint4 w) {
    return nib(tstop_bits(w.x)) | nib(tstop_bits(w.y)) << 4 | nib(tstop_bits(w.z)) << 8 | nib(tstop_bits(w.w)) << 12;
}
__device__ __forceinline__ uint32_t vstop_mask(uint4 w) {
    return nib(vstop_bits(w.x)) | nib(vstop_bits(w.y)) << 4 | nib(vstop_bits(w.z)) << 8 | nib(vstop_bits(w.w)) << 12;
}
__device__ __forceinline__ uint32_t byte_of(uint4 w, uint32_t q) {
    // two selects + v_perm_b32 (an indexed select would be lowered to scratch)
    const bool upper = (q & 8) != 0;
    const uint32_t lo = upper ? w.z : w.x, hi = upper ? w.w : w.y;
    return __builtin_amdgcn_perm(hi, lo, (q & 7) | 0x0C0C0C00u);
}

// bit i (0..15) set iff byte i of the 16 bytes is SP or HT
__device__ __forceinline__ uint32_t ws_mask(uint4 w) {
    auto eq = [](uint32_t x, uint32_t b) {  // bit 7 of byte i set iff byte i == b
        const uint32_t t = x ^ b;
        return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    };
    return nib(eq(w.x, 0x20202020u) | eq(w.x, 0x09090909u)) | nib(eq(w.y, 0x20202020u) | eq(w.y, 0x09090909u)) << 4 |
           nib(eq(w.z, 0x20202020u) | eq(w.z, 0x09090909u)) << 8 | nib(eq(w.w, 0x20202020u) | eq(w.w, 0x09090909u)) << 12;
}

// bit i (0..15) set iff byte i of the chunk is CR
__device__ __forceinline__ uint32_t cr_mask(uint4 w) {
    auto eq = [](uint32_t x) {
        const uint32_t t = x ^ 0x0D0D0D0Du;
        return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    };
    return nib(eq(w.x)) | nib(eq(w.y)) << 4 | nib(eq(w.z)) << 8 | nib(eq(w.w)) << 12;
}

// bit i (0..15) set iff byte i of the chunk is b
__device__ __forceinline__ uint32_t byte_mask(uint4 w, uint32_t b) {
    const uint32_t bb = b * 0x01010101u;
    auto eq = [bb](uint32_t x) {
        const uint32_t t = x ^ bb;
        return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
    };
    return nib(eq(w.x)) | nib(eq(w.y)) << 4 | nib(eq(w.z)) << 8 | nib(eq(w.w)) << 12;
}
// bytes the fast path refuses anywhere in a header block: < 0x20 other than
// HT / CR / LF, or DEL
__device__ __forceinline__ uint32_t fast_bad_mask(uint4 w) {
    return stop_mask(w) & ~(byte_mask(w, '\t') | byte_mask(w, '\r') | byte_mask(w, '\n'));
}

}  // namespace

}  // namespace l7

// The block schedule of kafka_classify_kernel's window-path CRC and the span
// rule of its staging slot, as plain integer code: the kernel runs it
// (kafka_dec.h, kafka_classify.hip) and a host program can include it
// (tests/native_sched/kafka_block_schedule.cc).  Product code.
//
// Positions are "slot-relative": byte offsets from the 16-byte aligned address
// at or below the request's first byte, so request byte pos is
// pos + (request address & 15) and a multiple of 16 is a chunk boundary in
// memory.  The lane's staging slot holds 64 bytes, four chunks, and `sb` names
// them: the slot holds [sb, sb + 64), or nothing usable when sb == kNoSpan.
//
// A message at [s, e) read through its 36-byte window has its CRC over
// [s + 16, e).  Its window block is [wb, wb + 64), wb <= s, already in the slot.
// The blocks after it are [wb + 64 k, +64), each staged while the one before is
// hashed; the last one holds e - 1 and is hashed where it lies, up to e.  It is
// left in the slot, and so is known to hold [keep_base, keep_base + 64): when
// the next message's window, or the header that follows the set, lies in it,
// the walk reads it there and not from memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define L7_KSCHED_FN __host__ __device__ __forceinline__
#else
#define L7_KSCHED_FN inline
#endif

namespace l7 {
namespace ksched {

constexpr uint32_t kNoSpan = 0x80000000u;  // no position is within 64 bytes above it
constexpr uint32_t kWindow = 36;           // bytes of a message the walk reads at once

// [pos, pos + n) lies in the slot (n <= 64): its offset there is pos - sb
L7_KSCHED_FN bool in_span(uint32_t sb, uint32_t pos, uint32_t n) { return pos - sb <= 64u - n; }
// the window block of a message at s: the slot's when its window lies in it, else staged from s's chunk
L7_KSCHED_FN uint32_t window_base(uint32_t sb, uint32_t s) { return in_span(sb, s, kWindow) ? sb : s & ~15u; }
// what the slot holds after the CRC of a message ending at e whose window block was wb: the block of byte e - 1
L7_KSCHED_FN uint32_t keep_base(uint32_t wb, uint32_t e) { return wb + ((e - wb - 1u) & ~63u); }

// The CRC of [p, e) (p = s + 16, wb <= s, p < wb + 64, p < e), step by step on v:
//   v.head(p, h)           h < 16 bytes up to the first chunk boundary, from the cursor's chunk
//   v.slot(base, lo, hi)   bytes [lo, hi) of the block at base, hashed where they lie in the slot
//   v.window(wb, lo, next) bytes [lo, 64) of the window block, read out of the slot; next is staged
//   v.block(a, next)       the 64 bytes of the block staged at a; next (kNoSpan: none) is staged meanwhile
template <class V>
L7_KSCHED_FN void crc_schedule(uint32_t wb, uint32_t p, uint32_t e, V &v) {
    uint32_t h = (16u - (p & 15u)) & 15u;
    if (h > e - p) h = e - p;
    if (h) v.head(p, h);
    const uint32_t i = p + h;
    if (i >= e) return;
    if (e <= wb + 64u) {  // the message ends in its window block: nothing is staged
        v.slot(wb, i - wb, e - wb);
        return;
    }
    uint32_t a = wb + 64u;
    v.window(wb, i - wb, a);
    while (e - a >= 64u) {
        v.block(a, e - a > 64u ? a + 64u : kNoSpan);
        a += 64u;
    }
    if (a < e) v.slot(a, 0u, e - a);
}

}  // namespace ksched
}  // namespace l7

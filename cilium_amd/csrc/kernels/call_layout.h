// The staging layout of one synchronous call (product code), the same text for
// the host path (host_call.cc, batcher.cc), the resident services' staging
// (service.cc) and the service kernels (kernels/service.h).
// Inputs of a call of n requests over arena_len bytes, nn = max(n, 1):
//   [off u64[st] | len u32[st] | conn u32[st] | arena at CallArenaOff(st)]
// where st, the arrays' length in entries, is nn (packed: a thread's staging,
// a service's), a batcher slot's stride, or CallNn4(n) (a slot's arrays copied
// as four pieces, each starting 16-byte aligned); CallArenaOff(st), a multiple
// of 256 at least 16 st, is past the arrays in every form.
// Outputs: [verdict u8[nn], padded to 4 | rule i32[nn] | consumed u32[nn]].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"

namespace l7 {

L7_HD constexpr size_t CallNn(uint32_t n) { return n ? n : 1; }
L7_HD constexpr size_t CallNn4(uint32_t n) { return (CallNn(n) + 3) & ~(size_t)3; }

// inputs: byte offsets of the arrays st entries long (off is at 0), and of the arena
L7_HD constexpr size_t CallLenOff(size_t st) { return st * 8; }
L7_HD constexpr size_t CallConnOff(size_t st) { return st * 12; }
L7_HD constexpr size_t CallArenaOff(size_t st) { return ((st ? st : 1) * 16 + 255) & ~(size_t)255; }
L7_HD constexpr size_t CallInBytes(size_t st, uint64_t arena_len) { return CallArenaOff(st) + arena_len; }

// outputs
L7_HD constexpr size_t CallRuleOff(uint32_t n) { return CallNn4(n); }
L7_HD constexpr size_t CallConsumedOff(uint32_t n) { return CallNn4(n) + CallNn(n) * 4; }
L7_HD constexpr size_t CallOutBytes(uint32_t n) { return CallNn4(n) + CallNn(n) * 8; }

// capacities of buffers that hold them: 64 bytes more, so that aligned 16-byte reads past the last
// request stay inside (the outputs' 9 bytes per request and the slack cover the verdicts' padding)
constexpr size_t kCallSlack = 64;
L7_HD constexpr size_t CallInCap(size_t st, uint64_t arena_len) { return CallInBytes(st, arena_len) + kCallSlack; }
L7_HD constexpr size_t CallOutCap(uint32_t n) { return CallNn(n) * 9 + kCallSlack; }

static_assert(CallArenaOff(0) == 256 && CallArenaOff(1) == 256 && CallArenaOff(16) == 256 && CallArenaOff(17) == 512,
              "arena offset");
static_assert(CallArenaOff(17) >= CallConnOff(CallNn4(17)) + CallNn4(17) * 4, "the arrays end before the arena");
static_assert(CallOutBytes(1) == 12 && CallOutBytes(5) == 8 + 5 * 8, "output bytes");
static_assert(CallOutCap(1) >= CallOutBytes(1) && CallOutCap(5) >= CallOutBytes(5), "the slack covers the padding");
static_assert(CallOutCap(64) == 64 * 9 + 64, "a service's outputs (kSvcOutBytes)");
static_assert(CallInCap(64, 256 * 1024) == 1024 + 256 * 1024 + 64, "a service's inputs (kSvcInBytes)");

}  // namespace l7

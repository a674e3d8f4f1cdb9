// HTTP classifier, layer 0: the workgroup's geometry (waves, windows, the LDS
// layout, the window swizzle) and the optional phase-timing macros.  Like the
// layers above it, included by http_classify.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include "../device_tables.h"

// OCKL's DPP wave reductions (64-bit forms are not declared by hip_runtime.h)
extern "C" __device__ __attribute__((const)) unsigned long long __ockl_wfred_min_u64(unsigned long long);
extern "C" __device__ __attribute__((const)) unsigned long long __ockl_wfred_max_u64(unsigned long long);
extern "C" __device__ __attribute__((const)) unsigned long long __ockl_wfred_and_u64(unsigned long long);

namespace l7 {

namespace {

// (Round 6: 16 waves with 128-byte windows, 128 VGPRs, 4 waves per SIMD:
// 22.8 ms on cfg5 against 17.0 -- the spills and twice the window rounds cost
// more than the occupancy gains; 12 waves 23.2 ms; profiles/r6/ab6d_*.)
constexpr int kWaves = 8;
constexpr int kBlock = 64 * kWaves;
constexpr uint32_t kWin = 256;                 // bytes per lane window
constexpr uint32_t kWinChunks = kWin / 16;
constexpr uint32_t kWaveLds = 64 * kWin;       // 16 KiB per wave
constexpr uint32_t kOffImg = kWaves * kWaveLds;
constexpr uint32_t kLdsBytes = kOffImg + kLdsImageBytes;
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");
constexpr uint32_t kLanesPerWin = kWinChunks;  // DMA: one lane per 16-byte chunk of a window
constexpr uint32_t kWinPerInst = 64 / kLanesPerWin;
static_assert(kWinChunks == 8 || kWinChunks == 16, "window size");
// Chunk swizzle of lane t's slot, chosen so that the 16 lanes of each
// ds_read_b128 bank group reading "their chunk k" cover all 64 banks.
__device__ __forceinline__ uint32_t win_swizzle(uint32_t t) {
    return kWinChunks == 16 ? (t & 15) : ((t >> 1) & 7);
}

// Optional per-phase cycle accounting (debug builds with -DL7G_PHASE_TIMING:
// libl7gpu_timing.so, used by tools/exp_http.py).  Slots: 0 dma, 1 parse,
// 2 tile map + skips, 3 emit/other, 4 rounds, 5 skips, 6 tiles.
#ifdef L7G_PHASE_TIMING
__device__ unsigned long long g_phase[16];
#define PH_DECL uint64_t ph_t = __builtin_amdgcn_s_memtime(); uint64_t ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PH_MARK(slot) do { const uint64_t ph_n = __builtin_amdgcn_s_memtime(); ph_acc[slot] += ph_n - ph_t; ph_t = ph_n; } while (0)
#define PH_COUNT(slot, v) (ph_acc[slot] += (v))
#define PH_FLUSH(lane) do { if ((lane) == 0) for (int ph_i = 0; ph_i < 8; ph_i++) atomicAdd(&g_phase[ph_i], (unsigned long long)ph_acc[ph_i]); } while (0)
#else
#define PH_DECL
#define PH_MARK(slot) do {} while (0)
#define PH_COUNT(slot, v) do {} while (0)
#define PH_FLUSH(lane) do {} while (0)
#endif
// latency path: cycles of a section, added to g_phase[slot] by lane 0
#ifdef L7G_PHASE_TIMING
#define LAT_T0 uint64_t lat_t = __builtin_amdgcn_s_memtime();
#define LAT_T(slot) do { const uint64_t lat_n = __builtin_amdgcn_s_memtime(); if ((threadIdx.x & 63) == 0) atomicAdd(&g_phase[slot], (unsigned long long)(lat_n - lat_t)); lat_t = lat_n; } while (0)
#define LAT_N(slot) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_phase[slot], 1ull); } while (0)
#else
#define LAT_T0
#define LAT_T(slot) do {} while (0)
#define LAT_N(slot) do {} while (0)
#endif

}  // namespace

}  // namespace l7

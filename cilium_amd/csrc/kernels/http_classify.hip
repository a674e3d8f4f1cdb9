// HTTP/1 request classification on gfx950 (product code), v4.
//
// One wave owns a tile of 64 consecutive requests, one lane per request.
// Work proceeds in rounds, each made of three wave-wide steps:
//
//   1. window DMA: for every lane that needs bytes, the wave copies the next
//      256-byte window of the lane's request (16-byte aligned, clipped to the
//      request) into the lane's LDS slot with global_load_lds_dwordx4.
//      Sixteen lanes cooperate per window (one wave-instruction moves four
//      windows); chunk c of lane t's window is stored at position c ^ (t & 15)
//      so the lanes' later ds_read_b128 of "their chunk k" hit 64 distinct
//      banks.
//   2. parse: each lane runs the resumable framer over its window: request
//      line, header names (name DFA), header values of slots the rule set
//      constrains (slot DFAs; end-state rule masks AND-ed into u64
//      accumulators), Content-Length digits.  Bytes come from a two-chunk
//      register cursor (16-byte LDS reads, next chunk prefetched); tchar and
//      CTL tests are ALU; on the long tokens the DFA class of the next byte is
//      fetched while the current transition is in flight, so a byte costs one
//      dependent LDS round trip.  Values nobody constrains are skipped 16
//      bytes a step (SWAR CTL/DEL test).
//   3. skip: before its first window the wave streams its tile's byte span
//      once (coalesced LDS-DMA, 16 pieces of 1 KiB in flight) and keeps a
//      bit per 16-byte chunk holding a value-stop byte (< 0x20 other than HT,
//      or DEL) in registers.  A lane whose unconstrained value runs past its
//      window finds the first marked chunk after it by ds_bpermute and reads
//      just that chunk; when the stop is the CR of "\r\n\r\n" the request
//      finishes there, otherwise the next window starts at the stop.
//
// For the benchmark stream a tile takes the span stream, one window per
// request (the head) and one map lookup (the long pad header); constrained
// values stop being walked once their DFA state is absorbing.
//
// One 512-thread workgroup per CU: 8 waves x 16 KiB windows + the hot rule
// set's image (<= 32 KiB) = 160 KiB of LDS.
//
// Grammar, error precedence and policy semantics: Envoy's HTTP/1 codec +
// cilium.l7policy (envoy/cilium_l7policy.cc:127-182,
// envoy/cilium_network_policy.h:50-237); the oracle is
// oracle/http_ref.c.  Rule sets larger than kChunksPerPass chunks x
// kDfasPerPass DFAs per slot are evaluated in several framing passes.
//
// This file holds the kernels and their launchers; the layers under them, one
// header each, included here only: http_geom.h, http_bytes.h, http_lane.h,
// http_framer.h, http_tile.h, http_lat.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "../device_tables.h"
#include "copy_in.h"
#include "http_lat.h"
#include "launch.h"
#include "service.h"

namespace l7 {

// kHot = true : requests whose connection uses the hot rule set (image in LDS),
//               plus entries on connections without an HTTP parser.
// kHot = false: every other HTTP request (images read through L2); all of
//               them when no hot kernel runs (T.hot_ruleset < 0).
// answer_other: also answer the entries no classifier owns (unknown connection,
// no parser) UNSUPPORTED; false when partition_kernel has answered them.
// sel: the HTTP requests of a mixed batch (partition_kernel), tiles of 64
// list entries; null: the whole batch, tiles of 64 consecutive requests.
// An entry (ListEnt, device_tables.h) carries the request's length, offset
// and rule set, so a lane sets itself up from one coalesced 16-byte load;
// conn_ids, offs, lens and conns are read only for kEntByIndex entries, which
// take the steps of a request without a list.
// kGrab: tiles taken from the counter per atomic (1, or 4 for short requests;
// the launcher's note).  Separate instantiations keep kGrab == 1 the round-4
// code (+1-2 % on cfg2 when the grab size was a runtime value).
template <bool kHot, uint32_t kGrab = 1>
__global__ __launch_bounds__(kBlock) void http_classify_kernel(Batch B, HttpTables T, const uint4 *__restrict__ sel,
                                                               const uint32_t *__restrict__ sel_count,
                                                               uint32_t answer_other, uint32_t *__restrict__ tile_ctr) {
    const uint8_t *__restrict__ arena = B.arena;
    const uint32_t n = B.n;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    uint8_t *s_img = lds + kOffImg;

    const bool hot_ok = hot_ruleset_ok(T);
    if (kHot && !hot_ok) return;
#ifdef L7G_PHASE_TIMING
    const uint64_t ph_k0 = __builtin_amdgcn_s_memtime();
#endif
    if (kHot) stage_image<kLdsImageBytes>(s_img, T, (uint32_t)T.hot_ruleset);
    __syncthreads();
#ifdef L7G_PHASE_TIMING
    if (tid == 0) atomicAdd(&g_phase[7], (unsigned long long)(__builtin_amdgcn_s_memtime() - ph_k0));
#endif

    const Out O{B.verdict, B.rule, B.consumed, T.nfa_bits};
    uint8_t *wave_lds = lds + wave * kWaveLds;
    const uint32_t m = sel ? *sel_count : n;
    const uint32_t ntiles = (m + 63) / 64;
    // Tiles: the first by position, the rest (when the launcher passes a zeroed
    // counter) taken one at a time by whichever wave is free, so the waves of
    // the persistent grid finish together whatever their tiles cost; else a
    // fixed stride.
    const uint32_t stride = gridDim.x * kWaves;
    uint32_t grab_next = 0, grab_left = 0;  // tiles taken from the counter, not started yet (wave-uniform)
    for (uint32_t tile = blockIdx.x * kWaves + wave, next; tile < ntiles; tile = next) {
        next = tile + stride;
        Lane L;
        const uint32_t slot = tile * 64 + lane;
        uint4 e = make_uint4(slot, 0, 0, kEntByIndex);
        if (sel) e = slot < m ? sel[slot] : make_uint4(n, 0, 0, kEntByIndex);
        L.idx = e.x;
        lane_idle(L);
        const uint8_t *img = kHot ? s_img : nullptr;
        if (L.idx < n) {
            // a packed entry is an HTTP request on rule set w >> 12 (the partition's reading of its connection)
            DevConn conn{(int32_t)(e.w >> 12), PROTO_HTTP, 0, 0xFFFF};
            if (e.w == kEntByIndex) {
                const uint32_t ci = B.conn_ids[L.idx];
                conn = L7_BATCH_CONN(B, ci);
            }
            const int32_t rs = lane_ruleset<kHot>(L, conn, T, hot_ok, answer_other);
            if (rs >= 0) {
                uint64_t off = l7_ent_off(e.z, e.w);
                uint32_t len = e.y;
                if (e.w == kEntByIndex) {
                    off = B.offs[L.idx];
                    len = B.lens[L.idx];
                }
                if (lane_place(L, arena, off, len, B.arena_len) && !kHot) img = T.images + T.rulesets[rs].image_off;
            }
        }
        run_tile<kHot>(L, img, wave_lds, lane, O);
        if (tile_ctr) {  // taken at the tile's end: a wave asks for work only when it is free
            if (kGrab == 1) {
                uint32_t t = 0;
                if (lane == 0) t = atomicAdd(tile_ctr, 1u);
                next = stride + __builtin_amdgcn_readfirstlane(t);
            } else {
                if (grab_left == 0) {
                    uint32_t t = 0;
                    if (lane == 0) t = atomicAdd(tile_ctr, kGrab);
                    grab_next = stride + __builtin_amdgcn_readfirstlane(t);
                    grab_left = kGrab;
                }
                next = grab_next++;
                grab_left--;
            }
        }
    }
}


// One request per wave (lat_request, http_lat.h) for small calls; the image
// staging, the request's checks and the answers for entries no parser owns are
// the tile kernel's.  stage: copy the hot rule set's image into LDS (the
// resident service stages it once for its lifetime).  Ends with a barrier.
template <bool kHot>
__device__ __forceinline__ void lat_body(const Batch &B, const HttpTables &T, const uint4 *__restrict__ sel,
                                         const uint32_t *__restrict__ sel_count, uint32_t answer_other, uint8_t *lds,
                                         bool stage) {
    const uint8_t *__restrict__ arena = B.arena;
    const uint32_t n = B.n;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    uint8_t *s_img = lds + kOffImg;
#ifdef L7G_PHASE_TIMING
    const uint64_t ph_k0 = __builtin_amdgcn_s_memtime();
#endif
    const bool hot_ok = hot_ruleset_ok(T);
    if (kHot && !hot_ok) return;
    if (kHot && stage) stage_image<kLdsImageBytes>(s_img, T, (uint32_t)T.hot_ruleset);
    __syncthreads();
#ifdef L7G_PHASE_TIMING
    if (tid == 0) atomicAdd(&g_phase[7], (unsigned long long)(__builtin_amdgcn_s_memtime() - ph_k0));
#endif
    const Out O{B.verdict, B.rule, B.consumed, T.nfa_bits};
    uint8_t *wave_lds = lds + wave * kWaveLds;
    const uint32_t m = sel ? *sel_count : n;
    for (uint32_t r = blockIdx.x * kWaves + wave; r < m; r += gridDim.x * kWaves) {
        LAT_T0
        Lane L;
        L.idx = sel ? sel[r].x : r;  // (a small call: the entry's index, the rest as without a list)
        lane_idle(L);
        const uint8_t *img = kHot ? s_img : nullptr;
        if (L.idx < n) {
            const uint32_t ci = B.conn_ids[L.idx];
            const DevConn conn = L7_BATCH_CONN(B, ci);
            const int32_t rs = lane_ruleset<kHot>(L, conn, T, hot_ok, answer_other);
            if (rs >= 0 && lane_place(L, arena, B.offs[L.idx], B.lens[L.idx], B.arena_len) && !kHot)
                img = T.images + T.rulesets[rs].image_off;
        }
        LAT_T(8);
        LAT_N(12);
        if (!L.done) {
            if (!lat_fast<kHot>(L, img, wave_lds, lane, O)) lat_request<kHot>(L, img, wave_lds, lane, O);
        } else if (L.owed && lane == 0) {
            emit(L, O);
        }
    }
    __syncthreads();
}

template <bool kHot>
// ci: the call's inputs to copy first (a one-workgroup launch), or none.
__global__ __launch_bounds__(kBlock) void http_latency_kernel(Batch B, HttpTables T, const uint4 *__restrict__ sel,
                                                              const uint32_t *__restrict__ sel_count,
                                                              uint32_t answer_other, CopyIn ci) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    copy_in_block(ci);
    lat_body<kHot>(B, T, sel, sel_count, answer_other, lds, true);
    signal_done_block(ci);
}

// The resident service (kernels/service.h): one workgroup serves the
// synchronous HTTP calls (one Envoy Allowed(), a few requests) the host posts
// to the box, each as the launched path would run it -- the inputs copied
// into HBM, the hot pass and / or the general pass of lat_body, the answers to
// pinned memory, then the done word -- with the hot rule set's image staged
// in LDS once for the service's lifetime.  The box's first word holds the
// poll's result (wave 0's window area: free between calls).
__global__ __launch_bounds__(kBlock) void http_service_kernel(SvcBox *box, SvcStatic S, HttpTables T, uint32_t seen0,
                                                              uint64_t idle) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    uint32_t *word = reinterpret_cast<uint32_t *>(lds);
    uint32_t seen = seen0;
    uint64_t t_last = __builtin_amdgcn_s_memtime();
    bool staged = false;
    if (threadIdx.x == 0) svc_store(&box->state, kSvcRunning);
    for (;;) {
        const SvcCall c = svc_next(box, seen, t_last, idle, word);
        if (!c.seq) break;
        const Batch B = svc_batch(S, c);
        const CopyIn ci = svc_copy(S, box, c);
        copy_in_block(ci);
        const uint32_t other = (c.flags & kSvcAnswerOther) ? 1u : 0u;
        if (c.flags & kSvcHttpHot) {
            lat_body<true>(B, T, nullptr, nullptr, other, lds, !staged);
            staged = true;
        }
        if (c.flags & kSvcHttpGeneral) lat_body<false>(B, T, nullptr, nullptr, other, lds, false);
        signal_done_block(ci);
        __syncthreads();
        t_last = __builtin_amdgcn_s_memtime();
    }
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        svc_store(&box->state, kSvcStopped);
    }
}

// Requests grouped by rule set (http_group.hip): a workgroup takes one segment
// of the grouped list at a time (all of it on one rule set), stages that rule
// set's image in LDS, and its waves take the segment's tiles of 64 entries
// from a counter in LDS; the image-in-LDS framer runs them (a tile never mixes
// rule sets, so image-derived values are wave-uniform as in the hot kernel).
// ctl: [0] segments, [1] the segment counter (zeroed by the launcher).
__global__ __launch_bounds__(kBlock) void http_grouped_kernel(Batch B, HttpTables T, const uint32_t *__restrict__ gsel,
                                                              const uint32_t *__restrict__ segs,
                                                              uint32_t *__restrict__ ctl) {
    const uint8_t *__restrict__ arena = B.arena;
    const uint32_t n = B.n;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    uint8_t *s_img = lds + kOffImg;
    uint32_t *s_ctl = reinterpret_cast<uint32_t *>(lds + kOffImg + kGroupImageBytes);  // segment, tile counter
    const Out O{B.verdict, B.rule, B.consumed, T.nfa_bits};
    uint8_t *wave_lds = lds + wave * kWaveLds;
    const uint32_t nsegs = ctl[0];
    for (;;) {
        if (tid == 0) {
            s_ctl[0] = atomicAdd(&ctl[1], 1u);
            s_ctl[1] = 0;
        }
        __syncthreads();
        const uint32_t sg = s_ctl[0];
        if (sg >= nsegs) break;
        const uint32_t rs = segs[3 * sg], e0 = segs[3 * sg + 1], cnt = segs[3 * sg + 2];
        stage_image<kGroupImageBytes>(s_img, T, rs);
        __syncthreads();
        for (;;) {
            uint32_t tile = 0;
            if (lane == 0) tile = atomicAdd(&s_ctl[1], 1u);
            tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile);
            if (tile * 64 >= cnt) break;
            Lane L;
            const uint32_t slot = tile * 64 + lane;
            L.idx = slot < cnt ? gsel[e0 + slot] : n;
            lane_idle(L);
            // (every grouped entry is an HTTP request on rule set rs)
            if (L.idx < n) lane_place(L, arena, B.offs[L.idx], B.lens[L.idx], B.arena_len);
            run_tile<true>(L, s_img, wave_lds, lane, O);
        }
        __syncthreads();  // every wave is done with the image before the next segment's
    }
}

// Host-side launcher (called from the C-ABI): persistent grids of one
// 512-thread workgroup per CU; the hot-rule-set kernel, then (only if some
// HTTP connection uses another rule set) the general one.
// latency: a small call, one request per wave (http_latency_kernel)
// (ci: latency only, with one workgroup: copied by the first kernel launched)
hipError_t LaunchHttpClassify(const Batch &B, const HttpTables &T, const ListEnt *ents, const uint32_t *sel_count,
                              bool any_cold, bool answer_other, uint32_t *tile_ctr, bool latency, const CopyIn *ci,
                              hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const uint4 *sel = reinterpret_cast<const uint4 *>(ents);
    const int num_cus = DeviceCuCount();
    const bool hot = T.hot_ruleset >= 0;
    const uint32_t other = answer_other ? 1u : 0u;
    if (latency) {
        const uint32_t lblocks = min((B.n + kWaves - 1) / kWaves, (uint32_t)num_cus);
        if (ci && lblocks != 1) return hipErrorInvalidValue;
        // the copy in the first kernel, the done word from the last
        const bool gen = !hot || any_cold;
        CopyIn first = ci ? *ci : CopyIn{};
        if (hot) {
            CopyIn k = first;
            if (gen) k.done = nullptr;
            hipLaunchKernelGGL(http_latency_kernel<true>, dim3(lblocks), dim3(kBlock), 0, stream, B, T, sel, sel_count,
                               other, k);
            first.n = 0;
        }
        if (gen)
            hipLaunchKernelGGL(http_latency_kernel<false>, dim3(lblocks), dim3(kBlock), 0, stream, B, T, sel, sel_count,
                               other, first);
        return hipGetLastError();
    }
    if (ci) return hipErrorInvalidValue;
    const uint32_t ntiles = (B.n + 63) / 64;
    uint32_t blocks = (ntiles + kWaves - 1) / kWaves;
    blocks = min(blocks, (uint32_t)num_cus);
    // tile_ctr: two zeroed counters (hot, general launch) or null (fixed stride).
    // Tiles taken from a counter one at a time serialise on its atomic when
    // they are quick (short requests: 4M 34-byte requests 0.74 ms, taken four at
    // a time 0.36 ms), and cost a longer tail when they are not (cfg2's 1.1 KB
    // requests: 1.59 vs 1.63 ms), so a batch of short requests takes four.
    // A wave with many tiles to run (a long batch: cfg5's 50M HTTP requests are
    // ~380 tiles per wave) also takes two per atomic: the tail grows by half a
    // tile, the counter's queue shrinks (cfg5 HTTP 16.94 -> 16.87 ms, profiles/r5/ab5e_work_grab.log).
    const uint32_t per_wave = ntiles / (blocks * kWaves);
    const uint32_t grab = B.arena_len / B.n < 512 ? 4u : per_wave >= 64 ? 2u : 1u;
    using Kern = void (*)(Batch, HttpTables, const uint4 *, const uint32_t *, uint32_t, uint32_t *);
    const Kern kHot = grab == 4 ? http_classify_kernel<true, 4> : grab == 2 ? http_classify_kernel<true, 2>
                                                                         : http_classify_kernel<true, 1>;
    const Kern kGen = grab == 4 ? http_classify_kernel<false, 4> : grab == 2 ? http_classify_kernel<false, 2>
                                                                          : http_classify_kernel<false, 1>;
    if (hot)
        hipLaunchKernelGGL(kHot, dim3(blocks), dim3(kBlock), 0, stream, B, T, sel, sel_count, other, tile_ctr);
    if (!hot || any_cold)
        hipLaunchKernelGGL(kGen, dim3(blocks), dim3(kBlock), 0, stream, B, T, sel, sel_count, other,
                           tile_ctr ? tile_ctr + 1 : nullptr);
    return hipGetLastError();
}

// The grouped list (LaunchHttpGroup's outputs): the grouped kernel over the
// segments, then the general kernel over the entries on rule sets whose image
// exceeds the LDS budget (gbig, ctl[2] of them; ctl[3] its tile counter).
hipError_t LaunchHttpGrouped(const Batch &B, const HttpTables &T, const uint32_t *gsel, const uint32_t *segs,
                             const ListEnt *gbig, uint32_t *ctl, bool any_big, hipStream_t stream) {
    if (B.n == 0) return hipSuccess;
    const int num_cus = DeviceCuCount();
    const uint32_t ntiles = (B.n + 63) / 64;
    const uint32_t blocks = min((ntiles + kWaves - 1) / kWaves, (uint32_t)num_cus);
    hipLaunchKernelGGL(http_grouped_kernel, dim3(blocks), dim3(kBlock), 0, stream, B, T, gsel, segs, ctl);
    if (any_big)
        hipLaunchKernelGGL(http_classify_kernel<false>, dim3(blocks), dim3(kBlock), 0, stream, B, T,
                           reinterpret_cast<const uint4 *>(gbig), ctl + 2, 0u,
                           ctl + 3);
    return hipGetLastError();
}

// The HTTP service: one workgroup on `stream` until it leaves (idle cycles
// without a call, or stop).
hipError_t LaunchHttpService(SvcBox *box, const SvcStatic &S, const HttpTables &T, uint32_t seen0, uint64_t idle,
                             hipStream_t stream) {
    hipLaunchKernelGGL(http_service_kernel, dim3(1), dim3(kBlock), 0, stream, box, S, T, seen0, idle);
    return hipGetLastError();
}

#ifdef L7G_PHASE_TIMING
hipError_t HttpPhaseTimes(uint64_t *out, bool reset) {
    hipError_t rc = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 16);
    if (rc == hipSuccess && reset) {
        static const unsigned long long z[16] = {};
        rc = hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z);
    }
    return rc;
}
#else
hipError_t HttpPhaseTimes(uint64_t *, bool) { return hipErrorNotSupported; }
#endif

}  // namespace l7

// HTTP classifier, layer 4: a tile of 64 requests -- the window DMA, the
// value-stop map and its skips, and all rounds of the tile (run_tile).  Needs
// the framer and gmem.h.
#pragma once
#include "gmem.h"
#include "http_framer.h"

namespace l7 {

namespace {

// ---------------------------------------------------------------- window DMA
// For every lane t with a window to load: chunks [0, hi] of the 256-byte
// window at address `win` into LDS slot t (chunk c stored at position
// c ^ (t & 15)).  packed = window address | hi (addresses are 16-byte aligned;
// 0 = nothing to load).
__device__ __forceinline__ void dma_windows_issue(uint8_t *wave_lds, uint64_t packed, uint32_t lane) {
    const uint32_t plo = (uint32_t)packed, phi = (uint32_t)(packed >> 32);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's earlier LDS reads have landed
    // every window address first, one wait, then the loads: issued one per
    // load, the compiler waits on each ds_bpermute in turn (16 serial LDS
    // round trips per round)
    uint32_t tlo[kWinChunks], thi[kWinChunks];
#pragma unroll
    for (int j = 0; j < (int)kWinChunks; j++) {
        const int t = (int)(kWinPerInst * j + lane / kLanesPerWin);
        tlo[j] = __shfl(plo, t);
        thi[j] = __shfl(phi, t);
    }
#pragma unroll
    for (int j = 0; j < (int)kWinChunks; j++) {
        const uint32_t t = kWinPerInst * j + lane / kLanesPerWin;
        const uint32_t c = (lane % kLanesPerWin) ^ win_swizzle(t);
        if ((tlo[j] | thi[j]) && c <= (tlo[j] & 15)) {
            const uint8_t *src = (const uint8_t *)((((uint64_t)thi[j]) << 32) | (tlo[j] & ~15u)) + 16 * c;
            __builtin_amdgcn_global_load_lds((const void *)src,
                                             (__attribute__((address_space(3))) void *)(wave_lds + j * 1024), 16, 0, 0);
        }
    }
}
__device__ __forceinline__ void dma_windows(uint8_t *wave_lds, uint64_t packed, uint32_t lane) {
    dma_windows_issue(wave_lds, packed, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// the DMA word of a lane's next window (0: nothing to load)
__device__ __forceinline__ uint64_t window_packed(Lane &L) {
    if (L.done) return 0;
    L.w = L.pa & ~15u;
    const uint32_t hi = min(L.lena - 1 - L.w, kWin - 1) >> 4;
    return (L.base + L.w) | hi;
}

// ---------------------------------------------------------------- value-stop map of a tile
// A value nobody constrains ends at its first "value stop" byte (< 0x20 other
// than HT, or DEL: CR normally, anything else is an error).  Before its first
// window the wave streams its tile's bytes, and each lane keeps, for its own
// request, one bit per 16-byte chunk -- "holds a value stop" -- in registers.
// A step moves 128 bytes of every request of the tile into VGPRs: load q of
// step j covers requests 8q..8q+7, lane l reading chunk 8j + (l & 7) of
// request 8q + (l >> 3), so one load instruction touches 8 full lines; a
// ballot per load hands each lane its request's eight bits; three steps are in
// flight.  (Four lanes per request and 64-byte steps: 2.42 -> 2.18 ms on 4M
// mixed-stream HTTP requests against one line per lane; eight lanes and VGPRs
// instead of an LDS ring went further, DESIGN.md.)  So every 16-byte chunk of
// a request is read once, whatever lies between the tile's requests (packed
// streams, the HTTP list of a mixed batch, scattered offsets), and a lane
// searches only its own bits.  A long value is then skipped by finding the
// lane's first marked chunk at or after L.pa and reading only that chunk and
// the next.  Chunks past the mapped range (kMapChunks, 3 KiB) continue window
// by window.  The head windows' DMA is issued before the map, into the window
// area, so it overlaps the map's stream.
//
// The bits enter a per-lane shift register eight at a time (one step), so
// after smax8 steps (the tile's longest request) chunk c sits at bit
// c + T.off with T.off = kMapChunks - 8 smax8, the same for every lane.
//
// Packed tiles (the 64 requests side by side, their span at most 9/8 of their
// own chunks) take the span mode instead: the span streams as coalesced 1 KiB
// pieces (lane l loads the piece's chunk l), a ballot gives every lane the
// piece's 64 stop bits, and each lane keeps the (at most four) pieces that
// overlap its request and finally shifts its own chunks into place (T.off = 0).
// One 1 KiB piece is 8 full cache lines per load instruction where the
// per-lane steps touch 64 lines: 0.48 vs 0.64 ms on cfg2's packed 1M stream;
// on the mixed stream's HTTP list the per-lane steps win (2.35 vs 2.61 ms per
// 4M requests) since no foreign byte is read.
constexpr uint32_t kMapWords = 6;
constexpr uint32_t kMapChunks = kMapWords * 32;             // chunks mapped per request
constexpr int kRing = (int)(kWaveLds / 1024);               // span mode: 1 KiB pieces in flight
constexpr uint64_t kSpanChunksMax = 256 * 64;               // span mode: at most 256 KiB

// Lane mode leaves out each request's first kWin bytes: map_skip only ever
// searches from the end of a window (a value still open there), so the first
// window's chunks are never looked up, and the head window reads them anyway.
constexpr uint32_t kSkipSteps = kWin / 64;

struct TileMap {
    uint32_t off;              // bit position of chunk 0 (uniform)
    uint32_t from;             // first chunk the map holds (uniform)
    uint32_t m[kMapWords];     // this lane's request: chunk bits (shift register)
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ uint4 u4(gm_u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); }

__device__ __forceinline__ uint32_t byte_at32(uint4 a, uint4 b, uint32_t i) {
    // byte i (0..31) of the 32 bytes a, b (little endian)
    const uint32_t d = i < 16 ? (i < 8 ? (i < 4 ? a.x : a.y) : (i < 12 ? a.z : a.w))
                              : (i < 24 ? (i < 20 ? b.x : b.y) : (i < 28 ? b.z : b.w));
    return (d >> (8 * (i & 3))) & 0xFF;
}

// a lane's chunk count (lanes without a request or with an empty one: 0)
__device__ __forceinline__ uint32_t map_nch(const Lane &L) { return L.lena > L.a0 ? (L.lena + 15u) >> 4 : 0u; }

// Span mode (packed tiles): see above.  The lane's request covers span chunks
// [vs, vs + nch); pieces j0..j0+3 (j0 = vs / 64) hold them.
__device__ __forceinline__ void map_span(TileMap &T, const Lane &L, uint32_t lane, uint8_t *wave_lds, uint64_t lo,
                                         uint32_t vtot, uint32_t nch) {
    const uint32_t npieces = (vtot + 63) >> 6;
    const uint32_t vs = nch ? (uint32_t)((L.base - lo) >> 4) : 0u;
    const uint32_t j0 = vs >> 6;
    uint32_t pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // pieces j0..j0+3, 2 words each
    // piece j -> slot j % kRing; an idle slot still issues its load (at the span
    // start), so a slot is examined with exactly kRing-1 loads behind it
#define MAP_PIECE(s, j)                                                                                   \
    do {                                                                                                  \
        const uint64_t a_ = lo + ((uint64_t)(j) << 10) + 16 * lane;                                       \
        __builtin_amdgcn_global_load_lds((const void *)((j) < npieces && ((j) << 6) + lane < vtot ? a_ : lo), \
                                         (__attribute__((address_space(3))) void *)(wave_lds + (s) * 1024), \
                                         16, 0, 0);                                                       \
    } while (0)
#pragma unroll
    for (int s = 0; s < kRing; s++) MAP_PIECE(s, (uint32_t)s);
    for (uint32_t jb = 0; jb < npieces; jb += kRing) {
#pragma unroll
        for (int s = 0; s < kRing; s++) {
            const uint32_t j = jb + s;
            wait_vmcnt<kRing - 1>();
            if (j < npieces) {
                // inline asm: a plain LDS read here would make hipcc drain every
                // in-flight LDS-DMA first (vmcnt(0)), serialising the ring
                uint4 v;
                asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)"
                             : "=v"(v)
                             : "v"((uint32_t)(uintptr_t)(wave_lds + s * 1024 + 16 * lane))
                             : "memory");
                const bool ok = (j << 6) + lane < vtot;
                const uint64_t M = __ballot(ok && stop_any(v) != 0);  // HT marks too: map_skip sorts it out
                const uint32_t q = j - j0;  // which of the lane's pieces (>= 4 or wrapped: none)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (q == (uint32_t)t) {
                        pc[2 * t] = (uint32_t)M;
                        pc[2 * t + 1] = (uint32_t)(M >> 32);
                    }
            }
            MAP_PIECE(s, j + kRing);
        }
    }
    wait_vmcnt<0>();
#undef MAP_PIECE
    // own chunk c = bit (vs & 63) + c of pc[]: shift right by vs & 63
    const uint32_t sh = vs & 63, wsh = sh >> 5, bsh = sh & 31;
#pragma unroll
    for (int w = 0; w < (int)kMapWords; w++) {
        const uint32_t a0 = wsh ? pc[w + 1] : pc[w];
        const uint32_t a1 = wsh ? (w + 2 < 8 ? pc[w + 2] : 0u) : pc[w + 1];
        T.m[w] = __builtin_amdgcn_alignbit(a1, a0, bsh);
    }
    T.off = 0;
}

// Returns true when the lane-mode map also DMA'd the tile's first head
// windows (window_packed of every lane) into the window area.
template <int kMapDepth>
__device__ __forceinline__ bool build_tile_map(TileMap &T, Lane &L, uint32_t lane, uint8_t *wave_lds) {
#pragma unroll
    for (int q = 0; q < (int)kMapWords; q++) T.m[q] = 0;
    T.off = kMapChunks;
    T.from = 0;
    const uint32_t nch = min(map_nch(L), kMapChunks);
    const uint32_t nseg = (nch + 3) >> 2;  // 64-byte steps of this lane
    // wave reductions by DPP (__ockl_wfred_*): no LDS round trips
    const uint32_t smax = (uint32_t)__builtin_amdgcn_readfirstlane((int)__ockl_wfred_max_u32(nseg));
    if (smax == 0) return false;
    const uint64_t act = __ballot(nch > 0);
    const uint64_t dummy = (uint64_t)__shfl((unsigned long long)L.base, (int)__builtin_ctzll(act));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // earlier LDS reads of the window area have landed
    {
        uint64_t lo = __ockl_wfred_min_u64(nch ? L.base : ~0ull);
        uint64_t hi = __ockl_wfred_max_u64(nch ? L.base + ((uint64_t)nch << 4) : 0ull);
        uint32_t own = __ockl_wfred_add_u32(nch);
        lo = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(lo >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)lo);
        hi = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(hi >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hi);
        own = (uint32_t)__builtin_amdgcn_readfirstlane((int)own);
        const uint64_t span = (hi - lo) >> 4;
        if (span <= kSpanChunksMax && span <= (uint64_t)own + (own >> 3)) {
            map_span(T, L, lane, wave_lds, lo, (uint32_t)span, nch);
            return false;
        }
    }
    T.off = kMapChunks - 4 * smax;
    T.from = 4 * kSkipSteps;
    if (smax <= kSkipSteps) return false;  // every request fits its head window
    // Lanes with nothing (more) to load still issue theirs, at a chunk of the
    // tile, so every step is eight loads and vmcnt counts stay exact.  Eight
    // lanes per request: a step is 128 bytes (a whole line) per request, load q
    // of step j covers requests 8q..8q+7, lane l reading chunk 8j + (l & 7) of
    // request 8q + (l >> 3), so every load instruction touches 8 full lines.
    // The head windows go into the window area now (the map does not use it),
    // so their DMA overlaps the map stream; the map's steps land in VGPRs,
    // kMapDepth of them in flight.  Loads and waits are written out (inline
    // asm): the compiler's own wait placement drains every load at the loop
    // head (vmcnt(0)), which leaves one memory latency per kMapDepth steps.
    {
        dma_windows_issue(wave_lds, window_packed(L), lane);
        const uint32_t smax8 = (smax + 1) >> 1, skip8 = kWin / 128;
        T.off = kMapChunks - 8 * smax8;
        const uint32_t sub8 = lane & 7, grp8 = lane >> 3;
        uint64_t qb8[8];
        uint32_t qn8[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            qb8[q] = (uint64_t)__shfl((unsigned long long)L.base, 8 * q + (int)grp8);
            qn8[q] = (uint32_t)__shfl((int)nch, 8 * q + (int)grp8);
        }
        gm_u32x4 buf[kMapDepth][8];
#define MAP_LOAD8(s, j)                                                                                        \
    do {                                                                                                       \
        _Pragma("unroll") for (int q_ = 0; q_ < 8; q_++) {                                                     \
            const uint32_t c_ = 8 * (uint32_t)(j) + sub8;                                                      \
            const uint64_t a_ = c_ < qn8[q_] ? qb8[q_] + ((uint64_t)c_ << 4) : dummy;                          \
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(buf[s][q_]) : "v"(a_) : "memory");           \
        }                                                                                                      \
    } while (0)
#pragma unroll
        for (int s = 0; s < kMapDepth; s++) MAP_LOAD8(s, skip8 + (uint32_t)s);
        for (uint32_t j0 = skip8; j0 < smax8; j0 += kMapDepth) {
#pragma unroll
            for (int s = 0; s < kMapDepth; s++) {
                const uint32_t j = j0 + s;
                asm volatile("s_waitcnt vmcnt(%8)"
                             : "+v"(buf[s][0]), "+v"(buf[s][1]), "+v"(buf[s][2]), "+v"(buf[s][3]), "+v"(buf[s][4]),
                               "+v"(buf[s][5]), "+v"(buf[s][6]), "+v"(buf[s][7])
                             : "n"(8 * (kMapDepth - 1)));
                // block q, bit l: request 8q + (l >> 3), chunk 8j + (l & 7)
                uint64_t M[8];
#pragma unroll
                for (int q = 0; q < 8; q++) M[q] = __ballot(stop_any(u4(buf[s][q])) != 0);
                MAP_LOAD8(s, j + kMapDepth);
                if (j < smax8) {
                    const uint32_t qo = lane >> 3;
                    uint64_t Mq = M[0];
#pragma unroll
                    for (int q = 1; q < 8; q++) Mq = qo == (uint32_t)q ? M[q] : Mq;
                    uint32_t nb = (uint32_t)(Mq >> (8 * (lane & 7))) & 0xFFu;
                    if (8 * j >= nch) nb = 0;
#pragma unroll
                    for (int q = 0; q < (int)kMapWords - 1; q++) T.m[q] = __builtin_amdgcn_alignbit(T.m[q + 1], T.m[q], 8);
                    T.m[kMapWords - 1] = (T.m[kMapWords - 1] >> 8) | (nb << 24);
                }
            }
        }
#undef MAP_LOAD8
        wait_vmcnt<0>();
        return true;
    }
}

// Lanes with L.scan set: skip the rest of the value with the lane's map.
__device__ __forceinline__ void map_skip(Lane &L, const TileMap &T) {
    if (!__any(L.scan)) return;
    if (!L.scan) return;
    const uint32_t nch = map_nch(L);
    const uint32_t mapped = min(nch, kMapChunks);
    for (;;) {
        const uint32_t k = L.pa >> 4;
        if (k < T.from) {  // (not reached: a scan starts at a window's end) window by window
            L.scan = false;
            return;
        }
        // first marked chunk in [k, mapped): bit positions [k + off, mapped + off)
        uint32_t found = 0xFFFFFFFFu;
        if (k < mapped) {
            const uint32_t p0 = k + T.off, p1 = mapped + T.off;
#pragma unroll
            for (int w = (int)kMapWords - 1; w >= 0; w--) {
                const uint32_t lo = 32u * (uint32_t)w;
                uint32_t bits = T.m[w];
                if (p0 > lo) bits = p0 - lo >= 32 ? 0u : bits & (0xFFFFFFFFu << (p0 - lo));
                if (p1 < lo + 32) bits = p1 <= lo ? 0u : bits & (0xFFFFFFFFu >> (lo + 32 - p1));
                if (bits) found = lo + (uint32_t)__builtin_ctz(bits) - T.off;
            }
        }
        if (found == 0xFFFFFFFFu) {
            if (mapped < nch) {  // no stop in the mapped chunks: on window by window after them
                L.pa = max(L.pa, mapped << 4);
                L.scan = false;
            } else {             // no value stop before the request's end
                L.pa = L.lena;
                finish(L, V_INCOMPLETE);
            }
            return;
        }
        const uint32_t cpos = found << 4;  // the marked chunk, request-relative
        const uint64_t ca = L.base + cpos;
        const uint4 w0 = gload16(ca);  // global, not flat (gmem.h)
        const uint4 w1 = cpos + 16 < L.lena ? gload16(ca + 16) : make_uint4(0, 0, 0, 0);
        const uint32_t lo_b = L.pa > cpos ? L.pa - cpos : 0;
        const uint32_t hi_b = min(L.lena - cpos, 16u);
        const uint32_t m = vstop_mask(w0) & (0xFFFFu << lo_b) & ((1u << hi_b) - 1u);
        if (m) {
            const uint32_t b = (uint32_t)__builtin_ctz(m);
            L.pa = cpos + b;
            L.scan = false;
            // "\r\n\r\n" here ends the header block: no window needed for it
            if (L.pa + 4 <= L.lena) {
                const uint32_t t4 = byte_at32(w0, w1, b) | byte_at32(w0, w1, b + 1) << 8 |
                                    byte_at32(w0, w1, b + 2) << 16 | byte_at32(w0, w1, b + 3) << 24;
                L.tail = t4 == 0x0A0D0A0Du;
            }
            return;
        }
        // the chunk's stops lie before pa (or are HT): search on
        L.pa = cpos + 16;
        if (L.pa >= L.lena) {
            L.pa = L.lena;
            finish(L, V_INCOMPLETE);
            return;
        }
    }
}

// The skipped value ended at the CR of "\r\n\r\n": what parse_window does for
// those four bytes (M_SKIP -> M_LF -> line_done -> M_LINE -> M_ENDLF ->
// headers_done), without another window.
template <bool kLds>
__device__ __forceinline__ void finish_tail(const Img<kLds> &I, Lane &L, const uint64_t *nfa_bits) {
    L.tail = false;
    L.pa += 4;
    if (line_done(I, L)) {
        L.mode = M_LINE;
        headers_done(I, L, nfa_bits);
    } else {
        finish(L, V_PARSE_ERROR);
    }
}

// All rounds of one tile.
// kInit = false: the lanes' framing state is set up by the caller (latency path).
// pre: the tile's map, already built (latency path); null: built here.
template <bool kLds, bool kFlush = true, bool kInit = true, int kMapDepth = 3>
__device__ __forceinline__ void run_tile(Lane &L, const uint8_t *img, uint8_t *wave_lds, uint32_t lane, const Out &O,
                                         const TileMap *pre = nullptr) {
    const Img<kLds> I{img};
    L.scan = false;
    L.tail = false;
    if (kInit && !L.done) {
        L.cg = 0;
        L.dg = 0;
        acc_init(I, L);
        frame_reset(I, L);
        if (L.lena == L.a0) finish(L, V_INCOMPLETE);
    }
    PH_DECL
    TileMap TM;
    bool loaded = false;  // true: the first windows are in
    if (pre) TM = *pre;
    else loaded = build_tile_map<kMapDepth>(TM, L, lane, wave_lds);
    PH_MARK(2);
    Cursor C;
    C.slot = wave_lds + lane * kWin;
    C.swz = win_swizzle(lane) << 4;
    while (__any(!L.done)) {
        const uint64_t packed = window_packed(L);
        PH_MARK(3);
        if (!loaded) dma_windows(wave_lds, packed, lane);
        loaded = false;
        PH_MARK(0);
        if (!L.done) {
            parse_window(I, L, C, O.nfa_bits);
            if (!L.done && !L.scan && L.pa >= L.lena) finish(L, V_INCOMPLETE);
        }
        PH_MARK(1);
        PH_COUNT(5, __builtin_popcountll(__ballot(L.scan)));
        map_skip(L, TM);
        if (L.tail) finish_tail(I, L, O.nfa_bits);
        PH_MARK(2);
        if (L.done && L.owed) {
            emit(L, O);
            L.owed = false;
        }
        PH_COUNT(4, 1);
    }
    if (L.done && L.owed) {  // answered before any round
        emit(L, O);
        L.owed = false;
    }
    PH_MARK(3);
    PH_COUNT(6, 1);
    if (kFlush) PH_FLUSH(lane);
}

}  // namespace

}  // namespace l7

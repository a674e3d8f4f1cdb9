// HTTP classifier, layer 2: a lane's request and framing state, the rule-set
// image accessor and its staging in LDS, how an entry becomes a lane's request,
// the slot DFAs, the end of a header line / header block, and the answer's way
// out.  Needs device_tables.h and the geometry (kBlock).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../device_tables.h"
#include "http_geom.h"

namespace l7 {

namespace {

enum : uint32_t {
    M_METHOD, M_TARGET, M_VERSION, M_LINE, M_NAME, M_OWS, M_VALUE, M_SKIP, M_LF, M_ENDLF, M_DONE,
    // chunked body (Transfer-Encoding: chunked), after the verdict is known
    M_CHSIZE, M_CHEXT, M_CHLF, M_CHDATA, M_CHDCR, M_CHDLF, M_TRL, M_TRLSCAN, M_TRLLF, M_TRLEND
};
constexpr uint32_t kNoSlot = 0xFF;

// Rule-set image accessor: LDS (hot rule set) or global memory.
template <bool kLds>
struct Img {
    const uint8_t *p;
    __device__ __forceinline__ uint32_t u8(uint32_t o) const { return p[o]; }
    __device__ __forceinline__ uint32_t u16(uint32_t o) const { return *(const uint16_t *)(p + o); }
    __device__ __forceinline__ uint32_t u32(uint32_t o) const { return *(const uint32_t *)(p + o); }
    __device__ __forceinline__ uint64_t u64(uint32_t o) const { return *(const uint64_t *)(p + o); }
    __device__ __forceinline__ uint4 u128(uint32_t o) const { return *(const uint4 *)(p + o); }  // o 16-byte aligned
};
template <bool kLds>
__device__ __forceinline__ uint32_t uni(uint32_t v) {
    return kLds ? (uint32_t)__builtin_amdgcn_readfirstlane((int)v) : v;
}
#define HDR_U32(I, field) uni<kLds>((I).u32(offsetof(ImgHeader, field)))
#define HDR_U16(I, field) uni<kLds>((I).u16(offsetof(ImgHeader, field)))
#define HDR_U8(I, field) uni<kLds>((I).u8(offsetof(ImgHeader, field)))

// ---------------------------------------------------------------- lane state
struct Lane {
    uint64_t base;      // request start rounded down to 16 B (absolute address)
    uint32_t a0;        // position of request byte 0 relative to base
    uint32_t lena;      // a0 + len
    uint32_t pa;        // next position to look at
    uint32_t w;         // position of the window held in the lane's LDS slot
    uint32_t mode;
    uint32_t mark;      // token start (method/target/name) or version index
    uint32_t idx;       // request index
    bool done;          // verdict known
    bool owed;          // verdict not yet written out
    bool scan;          // an unconstrained value continues past the window
    bool tail;          // the skipped value ends in "\r\n\r\n" (end of the header block)
    uint8_t verdict;
    int32_t rule;
    uint32_t consumed;
    // framing
    uint32_t present;   // slots seen (first occurrence)
    uint32_t slot;      // slot of the current header value (kNoSlot: none)
    uint32_t nstate;    // name DFA state
    uint32_t ninfo;     // NI_* flags of the current header name
    bool have_cl, chunked, cl_bad, cl_ws, in_ows;
    uint32_t ndig;      // Content-Length digits; Transfer-Encoding: bytes of "chunked" matched (0xFF: no)
    uint64_t clv, cl;   // clv: Content-Length value; in the chunked body: the chunk size
    // DFA of the current slot (kDfasPerPass == 1).  A slot without one walks
    // the image's null DFA (kImgNullDfaOff: class 0 for every byte, state 0
    // looping), so a step needs no test; dmask == 0 marks it.
    uint32_t dcls, dtrans, dmask, drow, st, saved;  // drow: bytes per transition row
    uint32_t dabs1;     // st - 1 < dabs1: neither dead (0) nor absorbing (>= dabs1 + 1)
    uint64_t acc[kChunksPerPass];
    uint32_t cg, dg;    // chunk group, DFA group of this pass
};
static_assert(kDfasPerPass == 1, "one DFA per slot per framing pass");

// A lane without a request: nothing to frame, nothing owed; UNSUPPORTED should it come to owe.
__device__ __forceinline__ void lane_idle(Lane &L) {
    L.done = true;
    L.owed = false;
    L.verdict = V_UNSUPPORTED;
    L.rule = -1;
    L.consumed = 0;
    L.mode = M_DONE;
    L.base = 0;
    L.a0 = L.pa = L.w = L.lena = 0;
}
// A lane that sits a tile out (lat_request): no window, no answer; the rest of its state stays.
__device__ __forceinline__ void lane_park(Lane &L) {
    L.done = true;
    L.owed = false;
    L.base = 0;
    L.a0 = L.pa = L.lena = 0;
}
// The request arena[off .. off + len) onto an idle lane, owed from here on; true: placed.  One outside
// the arena is out of contract: it stays answered UNSUPPORTED, and no address is made of its offset.
__device__ __forceinline__ bool lane_place(Lane &L, const uint8_t *arena, uint64_t off, uint32_t len,
                                           uint64_t arena_len) {
    if (!l7_in_arena(off, len, arena_len)) {
        L.owed = true;
        return false;
    }
    const uint64_t a = (uint64_t)(arena + off);
    L.base = a & ~(uint64_t)15;
    L.a0 = (uint32_t)(a & 15);
    L.lena = len > 0xFFFFFF00u ? 0xFFFFFF00u + L.a0 : L.a0 + len;  // > 4 GiB - 256: framing stops there
    L.done = false;
    L.owed = true;
    return true;
}
// The rule set this pass runs the lane's entry on, or -1 (kHot: the pass of the rule set staged in
// LDS; hot_ok: there is one).  An entry HTTP answers without classifying it -- unknown connection,
// no parser, no rule set -- comes to owe its UNSUPPORTED here, in the hot pass when there is one.
template <bool kHot>
__device__ __forceinline__ int32_t lane_ruleset(Lane &L, DevConn conn, const HttpTables &T, bool hot_ok,
                                                uint32_t answer_other) {
    const HttpConnClass c = l7_http_conn_class(conn.ruleset, conn.proto, T);
    if (c.mine && c.ruleset < 0 && answer_other && (kHot || !hot_ok)) L.owed = true;
    const bool is_hot = c.ruleset >= 0 && hot_ok && c.ruleset == T.hot_ruleset;
    return c.ruleset >= 0 && is_hot == kHot ? c.ruleset : -1;
}
// The usable hot rule set: in range, its image within the LDS budget.
__device__ __forceinline__ bool hot_ruleset_ok(const HttpTables &T) {
    const int32_t hot = T.hot_ruleset;
    return hot >= 0 && (uint32_t)hot < T.nrulesets && T.rulesets[hot].image_len <= kLdsImageBytes;
}
// Rule set rs's image (at most kBytes of it) into LDS, by the whole workgroup; the caller's barrier follows.
template <uint32_t kBytes>
__device__ __forceinline__ void stage_image(uint8_t *s_img, const HttpTables &T, uint32_t rs) {
    const uint32_t tid = threadIdx.x;
    const DevRuleset r = T.rulesets[rs];
    const uint4 *src = (const uint4 *)(T.images + r.image_off);
    const uint32_t n16 = (r.image_len + 15) / 16;
    // every load issued before the first store: one memory round trip, not
    // one per 8 KiB (a small launch -- one request -- waits on this)
    constexpr uint32_t kIters = (kBytes / 16 + kBlock - 1) / kBlock;
    uint4 t[kIters];
#pragma unroll
    for (uint32_t k = 0; k < kIters; k++)
        if (tid + k * kBlock < n16) t[k] = src[tid + k * kBlock];
#pragma unroll
    for (uint32_t k = 0; k < kIters; k++)
        if (tid + k * kBlock < n16) ((uint4 *)s_img)[tid + k * kBlock] = t[k];
}

// No DFA on the lane's slot: the null DFA, dead from the start.
__device__ __forceinline__ void null_dfa(Lane &L) {
    L.st = 0;
    L.dcls = L.dtrans = kImgNullDfaOff;
    L.dmask = L.drow = 0;
    L.dabs1 = ~0u;
}

template <bool kLds>
__device__ __forceinline__ void slot_begin(const Img<kLds> &I, Lane &L, uint32_t slot) {
    const uint32_t lo = I.u8(offsetof(ImgHeader, slot_dfa) + slot) + L.dg;
    const uint32_t hi = I.u8(offsetof(ImgHeader, slot_dfa) + slot + 1);
    null_dfa(L);
    if (lo < hi) {
        const uint32_t d = HDR_U32(I, dfa_off) + lo * sizeof(DevDfa);
        L.dcls = I.u32(d + 0);
        L.dtrans = I.u32(d + 4);
        L.dmask = I.u32(d + 8);
        const uint32_t nc_st = I.u32(d + 12);
        L.drow = 2 * (nc_st & 0xFFFF);
        L.st = nc_st >> 16;
        L.dabs1 = I.u32(d + 16) - 1;
    }
}

// One DFA step, branch-free: state 0 is a real row that loops back to itself
// and every slot has a class table (the null DFA's when it has no DFA).  The
// row address is a 24-bit multiply-add on the state (states and row sizes are
// 16-bit): one instruction behind the state, the class term added beforehand.
__device__ __forceinline__ uint32_t row_addr(uint32_t trans, uint32_t st, uint32_t row, uint32_t k) {
    return __umul24(st, row) + (trans + 2 * k);
}
template <bool kLds>
__device__ __forceinline__ void dfa_step(const Img<kLds> &I, Lane &L, uint32_t c) {
    L.st = I.u16(row_addr(L.dtrans, L.st, L.drow, I.u8(L.dcls + c)));
}
// the walk goes on: the state is neither dead nor absorbing
__device__ __forceinline__ bool walk_live(const Lane &L) { return L.st - 1u < L.dabs1; }

// AND the end state's masks of the pass's chunks into the accumulators.
template <bool kLds>
__device__ __forceinline__ void slot_end(const Img<kLds> &I, Lane &L) {
    if (L.dmask == 0) return;  // no DFA of this pass on the slot
    const uint32_t nchunks = HDR_U8(I, nchunks);
    const uint32_t nc = nchunks > L.cg ? min(nchunks - L.cg, (uint32_t)kChunksPerPass) : 0;
    const uint32_t base = L.dmask + 8 * (L.st * nchunks + L.cg);
#pragma unroll
    for (int c = 0; c < kChunksPerPass; c++)
        if ((uint32_t)c < nc) L.acc[c] &= I.u64(base + 8 * c);
}

template <bool kLds>
__device__ __forceinline__ void acc_init(const Img<kLds> &I, Lane &L) {
    const uint32_t nchunks = HDR_U8(I, nchunks);
#pragma unroll
    for (int c = 0; c < kChunksPerPass; c++)
        L.acc[c] = L.cg + c < nchunks ? I.u64(HDR_U32(I, init_off) + 8 * (L.cg + c)) : 0;
}

template <bool kLds>
__device__ __forceinline__ void frame_reset(const Img<kLds> &I, Lane &L) {
    L.pa = L.a0;
    L.mode = M_METHOD;
    L.mark = L.a0;
    L.present = 0;
    L.have_cl = L.chunked = false;
    L.cl = 0;
    slot_begin(I, L, SLOT_METHOD);
}

__device__ __forceinline__ void finish(Lane &L, uint8_t v, int32_t rule = -1) {
    L.done = true;
    L.scan = false;
    L.mode = M_DONE;
    L.verdict = v;
    L.rule = rule;
    if (v != V_ALLOW && v != V_DENY) L.consumed = 0;
}

// Headers complete (framing succeeded for this pass): next pass or verdict.
// The verdict of a request whose body is chunked: the chunks (and trailers)
// are walked after it to find where the request ends.
__device__ __forceinline__ void verdict_then_body(Lane &L, uint8_t v, int32_t rule) {
    if (!L.chunked) {
        finish(L, v, rule);
        return;
    }
    L.verdict = v;
    L.rule = rule;
    L.mode = M_CHSIZE;
    L.mark = L.pa;
    L.clv = 0;
}

template <bool kLds>
__device__ __forceinline__ void headers_done(const Img<kLds> &I, Lane &L, const uint64_t *nfa_bits) {
    const uint64_t total = L.chunked ? (uint64_t)(L.pa - L.a0) : (uint64_t)(L.pa - L.a0) + L.cl;
    if (total > 0xFFFFFFFFull) {
        finish(L, V_PARSE_ERROR);
    } else if (total > (uint64_t)(L.lena - L.a0)) {
        finish(L, V_INCOMPLETE);
    } else {
        L.consumed = (uint32_t)total;
        const uint32_t ndg = max((uint32_t)HDR_U8(I, max_slot_dfas), 1u);
        const uint32_t nchunks = HDR_U8(I, nchunks);
        if (L.dg + 1 < ndg) {  // more DFAs on some slot: frame again for this chunk group
            L.dg++;
            frame_reset(I, L);
        } else {
            const uint32_t nc = nchunks > L.cg ? min(nchunks - L.cg, (uint32_t)kChunksPerPass) : 0;
            // headers the rule set constrains but the request lacks
            uint32_t missing = HDR_U32(I, ref_slots) & 0xFFFF & ~L.present;
            while (missing) {
                const uint32_t s = __builtin_ctz(missing);
                missing &= missing - 1;
#pragma unroll
                for (int c = 0; c < kChunksPerPass; c++)
                    if ((uint32_t)c < nc) L.acc[c] &= I.u64(HDR_U32(I, absent_off) + 8 * (s * nchunks + L.cg + c));
            }
            // matchers the NFA pre-pass evaluated (present slots; an absent one
            // is covered by the absent masks above)
            const uint32_t nnfa = HDR_U8(I, nnfa);
            if (nnfa) {
                const uint64_t bits = nfa_bits[L.idx];
                const uint32_t refs = HDR_U32(I, nfa_off);
                for (uint32_t k = 0; k < nnfa; k++) {
                    const uint32_t ref = refs + k * (uint32_t)sizeof(DevNfaRef);
                    if (!((L.present >> I.u8(ref + offsetof(DevNfaRef, slot))) & 1)) continue;
                    const uint32_t mo = I.u32(ref + offsetof(DevNfaRef, mask_off)) +
                                        8 * ((uint32_t)((bits >> k) & 1) * nchunks + L.cg);
#pragma unroll
                    for (int c = 0; c < kChunksPerPass; c++)
                        if ((uint32_t)c < nc) L.acc[c] &= I.u64(mo + 8 * c);
                }
            }
            int32_t hit = -1;
#pragma unroll
            for (int c = kChunksPerPass - 1; c >= 0; c--)
                if ((uint32_t)c < nc && L.acc[c]) hit = (int32_t)(64 * (L.cg + c) + (uint32_t)__builtin_ctzll(L.acc[c]));
            if (hit >= 0) {
                verdict_then_body(L, V_ALLOW, (int32_t)I.u32(HDR_U32(I, rule_off) + 4 * (uint32_t)hit));
            } else if (L.cg + kChunksPerPass < nchunks) {  // next chunk group
                L.cg += kChunksPerPass;
                L.dg = 0;
                acc_init(I, L);
                frame_reset(I, L);
            } else {
                verdict_then_body(L, (uint8_t)HDR_U8(I, terminal), -1);
            }
        }
    }
}

// Header line complete (CRLF seen); false = Content-Length framing error.
template <bool kLds>
__device__ __forceinline__ bool line_done(const Img<kLds> &I, Lane &L) {
    bool ok = true;
    if (L.ninfo & NI_CL) {
        ok = !(L.have_cl || L.ndig == 0 || L.ndig > 10 || L.cl_bad);
        L.have_cl = true;
        L.cl = L.clv;
    }
    if ((L.ninfo & NI_TE) && L.ndig == 7) L.chunked = true;  // the value is "chunked" (case-insensitive)
    if (L.slot != kNoSlot) {
        slot_end(I, L);
        L.present |= 1u << L.slot;
    }
    return ok;
}

struct Out {
    uint8_t *verdict;
    int32_t *rule;
    uint32_t *consumed;
    const uint64_t *nfa_bits;  // NFA pre-pass results (HttpTables::nfa_bits)
};

__device__ __forceinline__ void emit(const Lane &L, const Out &O) {
    O.verdict[L.idx] = L.verdict;
    O.rule[L.idx] = L.rule;
    O.consumed[L.idx] = L.consumed;
}

}  // namespace

}  // namespace l7

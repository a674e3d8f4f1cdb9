// HTTP classifier, layer 5: one request per wave for small calls -- lat_request
// (a request's lines framed side by side) and lat_fast (the closed form for
// well-formed heads).  Needs the tile layer.
#pragma once
#include "http_tile.h"

namespace l7 {

namespace {

// ---------------------------------------------------------------- latency path
// The latency path's own tile maps (one request: a head of more than kLatLines
// lines, a chunked body, a further framing pass) keep two 128-byte steps in
// flight, not three: 32 VGPRs fewer where this kernel's registers run out.
constexpr int kLatMapDepth = 2;
constexpr uint32_t kLatLines = 63;  // header lines one wave frames side by side (lane k: line k)

// One request per wave, for the small calls of the synchronous drop-ins (one
// Allowed(), a few requests): the tile kernel's one lane walks a request's
// lines one after the other, every byte a chain of dependent LDS reads (a
// 1.1 KB cfg2 request: ~43k cycles of framing on one lane, the same with
// warm caches).  Here the request's lines are framed side by side.
//
// Every line of a request ends at its first CR: the method, target, name and
// value walks all stop there, and anything but LF after it is an error.  So
// the wave first finds the CRs (a ballot scan, 1 KiB per step, up to the
// empty line that ends the header block), then lane k runs the ordinary
// framer over line k alone -- lane 0 the request line from the request's
// start, lane k >= 1 from line k's first byte in M_LINE, each with L.lena at
// its line's end (its CR + 2) -- and what the lines leave behind is merged
// the way the sequential walk accumulates it: any error makes the request
// PARSE_ERROR; a slot counts at its first occurrence only (the lowest line),
// and its masks AND into the rule accumulators, which start at the init masks
// on lane 0 and at all ones on the other lanes; two Content-Length lines are
// an error and the first one's value counts; a chunked Transfer-Encoding line
// makes the body chunked.  (A repeated slot's value is walked by its DFA where
// the sequential framer skips it: both stop at the same bytes and fail on the
// same ones, and the walk's masks are dropped.)  Lane 0 then ends the header
// block as the framer does (headers_done on the merged state) and, when the
// answer needs more -- a chunked body, another framing pass of a large rule
// set -- carries on sequentially from there.  A header block of more than
// kLatLines lines is framed sequentially from the start by lane 0.
// All lanes enter with the same L (the request; done = false, owed = true).
template <bool kLds>
__device__ __forceinline__ void lat_request(const Lane &L, const uint8_t *img, uint8_t *wave_lds, uint32_t lane,
                                            const Out &O) {
    const Img<kLds> I{img};
    const uint32_t a0 = L.a0, lena = L.lena;
    if (lena == a0) {  // nothing yet
        if (lane == 0) {
            Lane W = L;
            finish(W, V_INCOMPLETE);
            emit(W, O);
        }
        return;
    }
    LAT_T0
    // ---- the CRs, in order, until the empty line (crpos: kLatLines + 2 entries)
    const uint32_t nch = (lena + 15) >> 4;
    uint32_t *crpos = reinterpret_cast<uint32_t *>(wave_lds);
    const uint64_t below = (1ull << lane) - 1;
    uint32_t ncr = 0;
    int hend = -1;     // index of the empty line that ends the header block
    bool all = false;  // every byte scanned
    // The scan also yields the tile map run_tile would stream (span mode: every
    // lane's request has this base, so chunk c is bit c): the value-stop bits of
    // the first kMapChunks chunks, one ballot per 64.
    TileMap TM;
#pragma unroll
    for (int q = 0; q < (int)kMapWords; q++) TM.m[q] = 0;
    TM.off = 0;
    TM.from = 0;
    // crpos[r]: the r-th CR's position | kLfKnown (the byte after it was in the
    // scan's registers) | kLfYes (and it is LF)
    constexpr uint32_t kLfKnown = 1u << 31, kLfYes = 1u << 30, kPos = kLfYes - 1;
    for (uint32_t c0 = 0;; c0 += 64) {
        const uint32_t c = c0 + lane;
        uint32_t m = 0;
        uint4 w = make_uint4(0, 0, 0, 0);
        if (c < nch) {
            w = gload16(L.base + 16ull * c);
            m = cr_mask(w);
            const uint32_t p0 = 16 * c;
            if (p0 < a0) m &= 0xFFFFu << (a0 - p0);
            if (p0 + 16 > lena) m &= (1u << (lena - p0)) - 1u;
        }
        const uint64_t sb = __ballot(c < nch && stop_any(w) != 0);
        if (c0 < kMapChunks) {
#pragma unroll
            for (int q = 0; q < (int)kMapWords; q += 2)
                if ((uint32_t)q == c0 / 32) {
                    TM.m[q] = (uint32_t)sb;
                    TM.m[q + 1] = (uint32_t)(sb >> 32);
                }
        }
        const uint32_t nb0 = (uint32_t)__shfl_down((int)(w.x & 0xFF), 1);  // the next chunk's first byte
        const uint32_t cnt = (uint32_t)__builtin_popcount(m);
        uint32_t ex = 0;  // exclusive prefix of cnt over the lanes (cnt <= 16: five ballots)
#pragma unroll
        for (int b = 0; b < 5; b++) ex += (uint32_t)__popcll(__ballot((cnt >> b) & 1) & below) << b;
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readfirstlane((int)__ockl_wfred_add_u32(cnt));
        for (uint32_t r = ncr + ex; m; m &= m - 1, r++) {
            const uint32_t b = (uint32_t)__builtin_ctz(m);
            const bool known = b < 15 || (lane < 63 && c + 1 < nch);
            const uint32_t nx = b < 15 ? byte_of(w, b + 1) : nb0;
            if (r < kLatLines + 2) crpos[r] = (16 * c + b) | (known ? kLfKnown : 0u) | (known && nx == '\n' ? kLfYes : 0u);
        }
        ncr += tot;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t have = min(ncr, kLatLines + 1);
        const uint64_t eb =
            __ballot(lane >= 1 && lane < have && (crpos[lane] & kPos) == (crpos[lane - 1] & kPos) + 2);
        if (eb) {
            hend = (int)__builtin_ctzll(eb);
            break;
        }
        if (c0 + 64 >= nch) {
            all = true;
            break;
        }
        if (ncr > kLatLines) break;
    }
    LAT_T(9);
    if (!(hend > 0 || (all && ncr <= kLatLines))) {  // too many lines: sequentially, lane 0
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        Lane W = L;
        if (lane != 0) lane_park(W);
        run_tile<kLds, true, true, kLatMapDepth>(W, img, wave_lds, lane, O);
        return;
    }
    // ---- lane k: line k
    uint32_t nl;
    if (hend > 0) {
        nl = (uint32_t)hend;
    } else {
        const uint32_t sp = ncr ? (crpos[ncr - 1] & kPos) + 2 : a0;  // an unterminated last line
        nl = ncr + (sp < lena ? 1u : 0u);
    }
    uint32_t start = a0, cr = 0;
    const bool has_cr = lane < nl && lane < ncr;
    if (lane < nl && lane > 0) start = (crpos[lane - 1] & kPos) + 2;
    if (has_cr) cr = crpos[lane] & kPos;
    const uint32_t lend = has_cr ? min(cr + 2, lena) : lena;
    // (a line that would start at the request's end follows "\r\r" there: the
    // line before it fails on its LF, and this one has no byte to frame)
    const bool act = lane < nl && start < lend;
    const uint32_t cr_end_w = hend > 0 ? crpos[hend] : 0u, cr_end = cr_end_w & kPos;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // crpos read: the window area is the lanes' again
    __builtin_amdgcn_wave_barrier();
    const bool complete = has_cr && cr + 2 <= lena;
    Lane W = L;
    W.owed = false;
    W.cg = 0;
    W.dg = 0;
    acc_init(I, W);
    frame_reset(I, W);
    if (act) {
        W.lena = lend;
        if (lane > 0) {
#pragma unroll
            for (int c = 0; c < kChunksPerPass; c++) W.acc[c] = ~0ull;
            W.pa = W.mark = start;
            W.mode = M_LINE;
            null_dfa(W);
            W.slot = kNoSlot;
        }
    } else {
        lane_park(W);
    }
    run_tile<kLds, true, false, kLatMapDepth>(W, img, wave_lds, lane, O, &TM);
    LAT_T(10);
    // ---- merge (a line that reached its end finished INCOMPLETE there)
    const bool bad = act && W.verdict == V_PARSE_ERROR;
    const bool inc = act && !bad && !complete;
    const uint64_t clb = __ballot(act && W.have_cl);
    const bool err = __ballot(bad) != 0 || __popcll(clb) > 1;
    const bool any_inc = __ballot(inc) != 0;
    const uint64_t cl = clb ? (uint64_t)__shfl((unsigned long long)W.cl, (int)__builtin_ctzll(clb)) : 0ull;
    const bool chunked = __ballot(act && W.chunked) != 0;
    const uint32_t pres = act ? W.present : 0u;
    bool keep = act;
#pragma unroll
    for (int sl = 0; sl < 16; sl++) {
        const bool mine = lane >= 1 && act && pres == (1u << sl);
        const uint64_t mk = __ballot(mine);
        if (mine && lane != (uint32_t)__builtin_ctzll(mk)) keep = false;
    }
    const uint32_t present = __ockl_wfred_or_u32(keep ? pres : 0u);
    uint64_t acc[kChunksPerPass];
#pragma unroll
    for (int c = 0; c < kChunksPerPass; c++) acc[c] = __ockl_wfred_and_u64(keep ? W.acc[c] : ~0ull);
    if (lane != 0) {
        lane_park(W);
    } else {
        W.done = false;
        W.owed = true;
        W.scan = W.tail = false;
        W.lena = lena;
        if (err) {
            finish(W, V_PARSE_ERROR);
        } else if (hend <= 0 || any_inc || cr_end + 1 >= lena) {
            finish(W, V_INCOMPLETE);
        } else if ((cr_end_w & kLfKnown) ? !(cr_end_w & kLfYes) : *(const uint8_t *)(L.base + cr_end + 1) != '\n') {
            finish(W, V_PARSE_ERROR);
        } else {
            W.pa = cr_end + 2;
            W.mode = M_LINE;
            W.present = present;
#pragma unroll
            for (int c = 0; c < kChunksPerPass; c++) W.acc[c] = acc[c];
            W.have_cl = clb != 0;
            W.cl = cl;
            W.chunked = chunked;
            headers_done(I, W, O.nfa_bits);
        }
    }
    if (__ballot(lane == 0 && !W.done)) run_tile<kLds, true, false, kLatMapDepth>(W, img, wave_lds, lane, O);  // body / next pass
    else if (lane == 0) emit(W, O);
    LAT_T(11);
}

// ---------------------------------------------------------------- latency path: well-formed heads
// lat_request runs the general framer on each lane's line, and on one wave its
// instruction path -- every mode of the resumable state machine, per byte --
// is what a synchronous call waits for (cfg2's 1.1 KB request: ~38k cycles of
// parse_window for six lines).  Most requests a proxy sees are well formed,
// and for those the framer's outcome has a short closed form, computed here
// with the bytes in LDS, the token boundaries from wave-wide masks, one lane
// per header line and one lane per DFA walk:
//
//   the header block [a0, H) ends at the first empty line; in it, no byte is a
//   CTL other than HT / CR / LF or DEL, every CR is followed by LF and every
//   LF follows a CR; line 0 is  method SP target SP "HTTP/" DIGIT "." DIGIT
//   with a method of 1..16 tchars and a target of >= 1 bytes (no SP: the
//   second SP ends it); every other line is  name ":" value  with a name of
//   1..15 [0-9A-Za-z-] (the image's name table: fast_line's lookup) and no
//   Content-Length or Transfer-Encoding header (their framing stays with the
//   framer); the rule set needs one framing pass (one DFA per slot, at most
//   kChunksPerPass chunks, no NFA matchers); at most 62 header lines.
//
// Under those conditions the framer walks the method and the target through
// their slot DFAs (the target until its state is absorbing), gives each
// header line its name's slot at the slot's first occurrence when a rule
// looks at it, walks that value from its first non-OWS byte through the
// slot's DFA with the trailing OWS excluded (until absorbing outside OWS),
// ANDs the end states' masks and the absent slots' masks into the init masks,
// and answers the first rule left (else the terminal verdict) with consumed =
// H - a0 (no Content-Length) -- which is what this computes.  Anything else,
// or a request longer than 4 KiB, returns false and goes to lat_request
// (envoy/cilium_l7policy.cc:127-182, envoy/cilium_network_policy.h:128-192).
constexpr uint32_t kFastMaxChunks = 256;  // 4 KiB of request bytes in the wave's LDS area
constexpr uint32_t kFastOffCr = kFastMaxChunks * 16, kFastOffLf = kFastOffCr + 2 * kFastMaxChunks;
constexpr uint32_t kFastOffBad = kFastOffLf + 2 * kFastMaxChunks, kFastOffPos = kFastOffBad + 2 * kFastMaxChunks;
static_assert(kFastOffPos + 4 * 64 <= kWaveLds, "fast path LDS layout");

template <bool kLds>
__device__ __forceinline__ bool lat_fast(const Lane &L, const uint8_t *img, uint8_t *wave_lds, uint32_t lane,
                                         const Out &O) {
    const Img<kLds> I{img};
    LAT_T0
    const uint32_t a0 = L.a0, lena = L.lena;
    const uint32_t nch = (lena + 15) >> 4;
    // the rule set: one framing pass, no NFA matchers, a name table
    const uint32_t nchunks = HDR_U8(I, nchunks);
    if (lena <= a0 || nch > kFastMaxChunks || HDR_U8(I, nnfa) != 0 || HDR_U8(I, max_slot_dfas) > 1 ||
        nchunks > (uint32_t)kChunksPerPass || HDR_U8(I, ntab_bits) == 0)
        return false;
    uint16_t *crm = reinterpret_cast<uint16_t *>(wave_lds + kFastOffCr);
    uint16_t *lfm = reinterpret_cast<uint16_t *>(wave_lds + kFastOffLf);
    uint16_t *badm = reinterpret_cast<uint16_t *>(wave_lds + kFastOffBad);
    uint32_t *crpos = reinterpret_cast<uint32_t *>(wave_lds + kFastOffPos);
    const uint64_t below = (1ull << lane) - 1;
    // ---- the request into LDS, its CR / LF / refused-byte masks, the first 64 CRs in order
    uint32_t ncr = 0;
    for (uint32_t c0 = 0; c0 < nch; c0 += 64) {
        const uint32_t c = c0 + lane;
        uint32_t m = 0;
        if (c < nch) {
            const uint4 w = gload16(L.base + 16ull * c);
            *reinterpret_cast<uint4 *>(wave_lds + 16 * c) = w;
            const uint32_t p0 = 16 * c;
            uint32_t in = 0xFFFFu;  // bytes of [a0, lena)
            if (p0 < a0) in &= 0xFFFFu << (a0 - p0);
            if (p0 + 16 > lena) in &= (1u << (lena - p0)) - 1u;
            m = byte_mask(w, '\r') & in;
            crm[c] = (uint16_t)m;
            lfm[c] = (uint16_t)(byte_mask(w, '\n') & in);
            badm[c] = (uint16_t)(fast_bad_mask(w) & in);
        }
        const uint32_t cnt = (uint32_t)__builtin_popcount(m);
        uint32_t ex = 0;
#pragma unroll
        for (int b = 0; b < 5; b++) ex += (uint32_t)__popcll(__ballot((cnt >> b) & 1) & below) << b;
        for (uint32_t r = ncr + ex; m; m &= m - 1, r++)
            if (r < 64) crpos[r] = 16 * c + (uint32_t)__builtin_ctz(m);
        ncr += (uint32_t)__builtin_amdgcn_readfirstlane((int)__ockl_wfred_add_u32(cnt));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    LAT_T(13);
    // the empty line: the first CR two bytes after the one before it
    const uint32_t have = min(ncr, 64u);
    const uint32_t mycr = lane < have ? crpos[lane] : 0u;
    const uint32_t prevcr = lane >= 1 && lane < have ? crpos[lane - 1] : 0u;
    const uint64_t eb = __ballot(lane >= 1 && lane < have && mycr == prevcr + 2);
    if (!eb) return false;
    const uint32_t hend = (uint32_t)__builtin_ctzll(eb);  // lines 0 .. hend-1, then the empty line
    if (hend > 62) return false;
    const uint32_t H = (uint32_t)__shfl((int)mycr, (int)hend) + 2;  // end of the header block
    if (H > lena) return false;
    // ---- the block's bytes: nothing refused, CR and LF only as CRLF
    bool bad = false;
    for (uint32_t c = lane; 16 * c < H; c += 64) {
        const uint32_t p0 = 16 * c;
        uint32_t in = 0xFFFFu;
        if (p0 < a0) in &= 0xFFFFu << (a0 - p0);
        if (p0 + 16 > H) in &= (1u << (H - p0)) - 1u;
        const uint32_t cr = crm[c], prev = c ? (uint32_t)crm[c - 1] >> 15 : 0u;
        bad |= (badm[c] & in) != 0 || (lfm[c] & in) != (((cr << 1) | prev) & in);
    }
    if (__ballot(bad)) return false;
    LAT_T(9);
    // ---- lane k: line k = [s, e), e its CR
    const uint32_t s = lane == 0 ? a0 : prevcr + 2, e = mycr;
    const bool line = lane < hend;
    auto chunk = [&](uint32_t k) { return *reinterpret_cast<const uint4 *>(wave_lds + 16 * k); };
    // the 16 bytes at p (p + 16 may pass the copy's end only inside its last chunk's area)
    auto bytes16 = [&](uint32_t p) {
        const uint32_t k0 = p >> 4, o = p & 15, i = o >> 2, sh = (o & 3) * 8;
        const uint4 a = chunk(k0), b = k0 + 1 < kFastMaxChunks ? chunk(k0 + 1) : make_uint4(0, 0, 0, 0);
        const uint32_t d0 = i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : a.w;
        const uint32_t d1 = i == 0 ? a.y : i == 1 ? a.z : i == 2 ? a.w : b.x;
        const uint32_t d2 = i == 0 ? a.z : i == 1 ? a.w : i == 2 ? b.x : b.y;
        const uint32_t d3 = i == 0 ? a.w : i == 1 ? b.x : i == 2 ? b.y : b.z;
        const uint32_t d4 = i == 0 ? b.x : i == 1 ? b.y : i == 2 ? b.z : b.w;
        uint4 f;
        f.x = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
        f.y = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
        f.z = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
        f.w = (uint32_t)((((uint64_t)d4 << 32) | d3) >> sh);
        return f;
    };
    auto byte_at = [&](uint32_t p) { return (uint32_t)wave_lds[p]; };
    bool refuse = false;
    // request line (lane 0): exactly two SPs and no HT (HT ends a target, and
    // not SP after it is an error), a method of 1..15 [0-9A-Za-z-], the version
    uint32_t sp1 = 0, sp2 = 0;
    if (lane == 0) {
        uint32_t nsp = 0;
        bool ht = false;
        for (uint32_t p = s & ~15u; p < e; p += 16) {
            const uint4 w = chunk(p >> 4);
            uint32_t in = 0xFFFFu;
            if (p < s) in &= 0xFFFFu << (s - p);
            if (p + 16 > e) in &= (1u << (e - p)) - 1u;
            uint32_t m = byte_mask(w, ' ') & in;
            ht |= (byte_mask(w, '\t') & in) != 0;
            const uint32_t q1 = p + (uint32_t)__builtin_ctz(m | 0x10000u);
            const uint32_t m2 = m & (m - 1);
            const uint32_t q2 = p + (uint32_t)__builtin_ctz(m2 | 0x10000u);
            sp2 = nsp == 0 ? q2 : nsp == 1 ? q1 : sp2;
            sp1 = nsp == 0 ? q1 : sp1;
            nsp += (uint32_t)__builtin_popcount(m);
        }
        const uint4 f = bytes16(s), v = bytes16(sp2 + 1);
        refuse = nsp != 2 || ht || sp1 == s || sp1 - s > 15 || sp2 == sp1 + 1 || e - sp2 != 9 ||
                 (uint32_t)__builtin_ctz(nonalnum_mask(f) | 0x10000u) != sp1 - s ||
                 !(v.x == 0x50545448u && (v.y & 0x00FF00FFu) == 0x002E002Fu && ((v.y >> 8) & 0xFF) - '0' < 10u &&
                   (v.y >> 24) - '0' < 10u);
    }
    // header lines (lanes 1 .. hend-1): the name's flags from the name table
    uint32_t ninfo = 0, vs = 0;
    if (line && lane > 0) {
        const uint4 f = bytes16(s);
        const uint32_t en = (uint32_t)__builtin_ctz(nonalnum_mask(f) | 0x10000u);
        if (en == 0 || en == 16 || s + en >= e || byte_of(f, en) != ':') {
            refuse = true;
        } else {
            auto keep = [en](uint32_t j) { return en >= 4 * j + 4 ? 0xFFFFFFFFu : en <= 4 * j ? 0u : (1u << (8 * (en - 4 * j))) - 1u; };
            const uint32_t w0 = (f.x | 0x20202020u) & keep(0), w1 = (f.y | 0x20202020u) & keep(1);
            const uint32_t w2 = (f.z | 0x20202020u) & keep(2), w3 = (f.w | 0x20202020u) & keep(3);
            const uint32_t h = l7_name_hash(w0, w1, w2, w3, en, HDR_U32(I, ntab_mul), HDR_U8(I, ntab_bits));
            const uint32_t ent = HDR_U32(I, ntab_off) + h * (uint32_t)sizeof(DevNameEnt);
            const uint4 n = I.u128(ent);
            const uint32_t meta = I.u32(ent + 16);
            const bool hit = (meta & 0xFF) == en && n.x == w0 && n.y == w1 && n.z == w2 && n.w == w3;
            ninfo = hit ? (meta >> 8) & 0xFF : 0u;
            if (ninfo & (NI_CL | NI_TE)) refuse = true;  // body framing: the framer's
            vs = s + en + 1;  // then past the OWS (M_OWS)
            const uint32_t o = (uint32_t)__builtin_ctz((~ws_mask(bytes16(vs)) & 0xFFFFu) | 0x10000u);
            vs += o;
            if (o == 16)
                while (vs < e && (byte_at(vs) == ' ' || byte_at(vs) == '\t')) vs++;
        }
    }
    if (__ballot(refuse)) return false;
    LAT_T(10);
    // slots: a header's at its first occurrence when some rule looks at it
    const uint32_t ref = HDR_U32(I, ref_slots);
    uint32_t slot = kNoSlot;
    if (line && lane > 0) {
        if (ninfo & NI_HOST) slot = SLOT_AUTHORITY;
        else if (ninfo & NI_CUSTOM) slot = SLOT_CUSTOM0 + (ninfo & NI_CUSTOM) - 1;
        if (slot != kNoSlot && !((ref >> slot) & 1)) slot = kNoSlot;
    }
#pragma unroll
    for (uint32_t sl = SLOT_AUTHORITY; sl < (uint32_t)kNumSlots; sl++) {
        const uint64_t mk = __ballot(slot == sl);
        if (slot == sl && lane != (uint32_t)__builtin_ctzll(mk)) slot = kNoSlot;
    }
    LAT_T(14);
    // ---- the DFA walks: lane 0 the target, lane 63 the method, lane k its value
    sp1 = (uint32_t)__shfl((int)sp1, 0);
    sp2 = (uint32_t)__shfl((int)sp2, 0);
    uint32_t wslot = slot, from = vs, to = e, kind = 2;  // kind: 0 method, 1 target, 2 value
    if (lane == 0) { wslot = SLOT_PATH; from = sp1 + 1; to = sp2; kind = 1; }
    if (lane == 63) { wslot = SLOT_METHOD; from = a0; to = sp1; kind = 0; }
    uint64_t acc[kChunksPerPass];
#pragma unroll
    for (int c = 0; c < kChunksPerPass; c++) acc[c] = ~0ull;
    const uint32_t nc = min(nchunks, (uint32_t)kChunksPerPass);
    if (wslot != kNoSlot) {
        const uint32_t lo = I.u8(offsetof(ImgHeader, slot_dfa) + wslot);
        const uint32_t hi = I.u8(offsetof(ImgHeader, slot_dfa) + wslot + 1);
        if (lo < hi) {
            const uint32_t d = HDR_U32(I, dfa_off) + lo * sizeof(DevDfa);
            const uint32_t dcls = I.u32(d + 0), dtrans = I.u32(d + 4), dmask = I.u32(d + 8);
            const uint32_t nc_st = I.u32(d + 12), dncls = nc_st & 0xFFFF, dabs = I.u32(d + 16);
            uint32_t st = nc_st >> 16, saved = 0;
            bool in_ows = false;
            uint32_t p = from;
            // the framer's walks (parse_window M_METHOD / M_TARGET / M_VALUE), 16
            // bytes a step: their classes read together, then the transitions
            bool go = p < to && (kind == 0 || (st != 0 && st < dabs));
            while (go) {
                const uint4 f = bytes16(p);
                uint32_t k[16];
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) k[j] = I.u8(dcls + byte_of(f, j));
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) {
                    if (go) {
                        if (kind == 2) {
                            const uint32_t c = byte_of(f, j);
                            const bool ws = c == ' ' || c == '\t';
                            if (ws && !in_ows) saved = st;
                            in_ows = ws;
                        }
                        if (st) st = I.u16(dtrans + 2 * (st * dncls + k[j]));
                        p++;
                        go = p < to && (kind == 0 || in_ows || (st != 0 && st < dabs));
                    }
                }
            }
            if (kind == 2 && p >= to && in_ows) st = saved;  // trailing OWS is not part of the value
            const uint32_t base = dmask + 8 * (st * nchunks);
#pragma unroll
            for (int cc = 0; cc < kChunksPerPass; cc++)
                if ((uint32_t)cc < nc) acc[cc] = I.u64(base + 8 * cc);
        }
    }
    LAT_T(15);
    // ---- merge (headers_done on one pass)
    const uint32_t present = __ockl_wfred_or_u32(lane > 0 && lane < 63 && slot != kNoSlot ? 1u << slot : 0u) |
                             (1u << SLOT_METHOD) | (1u << SLOT_PATH);
    uint64_t a[kChunksPerPass];
#pragma unroll
    for (int c = 0; c < kChunksPerPass; c++) a[c] = __ockl_wfred_and_u64(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < kChunksPerPass; c++)
            a[c] &= (uint32_t)c < nchunks ? I.u64(HDR_U32(I, init_off) + 8 * c) : 0ull;
        uint32_t missing = ref & 0xFFFF & ~present;
        while (missing) {
            const uint32_t sl = __builtin_ctz(missing);
            missing &= missing - 1;
#pragma unroll
            for (int c = 0; c < kChunksPerPass; c++)
                if ((uint32_t)c < nc) a[c] &= I.u64(HDR_U32(I, absent_off) + 8 * (sl * nchunks + c));
        }
        int32_t hit = -1;
#pragma unroll
        for (int c = kChunksPerPass - 1; c >= 0; c--)
            if ((uint32_t)c < nc && a[c]) hit = (int32_t)(64 * c + (uint32_t)__builtin_ctzll(a[c]));
        Lane W = L;
        W.consumed = H - a0;
        if (hit >= 0) finish(W, V_ALLOW, (int32_t)I.u32(HDR_U32(I, rule_off) + 4 * (uint32_t)hit));
        else finish(W, (uint8_t)HDR_U8(I, terminal), -1);
        emit(W, O);
    }
    LAT_T(11);
    return true;
}

}  // namespace

}  // namespace l7

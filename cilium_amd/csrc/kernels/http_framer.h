// HTTP classifier, layer 3: the resumable framer over one 256-byte window of
// a lane's request (parse_window).  Needs the geometry (kWin), the byte
// classes and the lane.
#pragma once
#include "http_bytes.h"
#include "http_geom.h"
#include "http_lane.h"

namespace l7 {

namespace {

__constant__ uint32_t kVer[10] = {'H', 'T', 'T', 'P', '/', 0x100, '.', 0x100, '\r', '\n'};

// ---------------------------------------------------------------- byte cursor
// Bytes of the lane's window, read from LDS one at a time (branch-free; the
// long-token loops below fetch them ahead of use).
struct Cursor {
    const uint8_t *slot;
    uint32_t swz;       // chunk swizzle of this lane, << 4
    uint32_t w;         // window start position
    __device__ __forceinline__ uint4 chunk(uint32_t k) const {
        return *(const uint4 *)(slot + (((k << 4) & (kWin - 16)) ^ swz));
    }
    // byte at position p (w <= p < w + kWin)
    __device__ __forceinline__ uint32_t at(uint32_t p) const { return slot[((p - w) & (kWin - 1)) ^ swz]; }
};

// One step of the pipelined walks (method, target, name, value): the
// transition on class k out of state st -- the read the next state waits for
// -- goes first, behind it the class of byte c1 and the byte at position p2.
// With the image in LDS the three reads and their one wait are one asm block:
// left to the compiler, the class read sinks to its use at the head of the
// next iteration, two dependent LDS round trips a byte.  The reads need no
// bounds: c1 is a byte, p2 wraps inside the lane's slot (as Cursor::at).
template <bool kLds>
__device__ __forceinline__ void walk_step(const Img<kLds> &I, const Cursor &C, uint32_t trans, uint32_t row, uint32_t cls,
                                          uint32_t &st, uint32_t &k, uint32_t c1, uint32_t p2, uint32_t &c2) {
    const uint32_t ta = row_addr(trans, st, row, k);
    if constexpr (kLds) {
        const uint32_t ib = (uint32_t)(uintptr_t)I.p;
        const uint32_t ba = (uint32_t)(uintptr_t)C.slot + (((p2 - C.w) & (kWin - 1)) ^ C.swz);
        // each read lands in its own address register: no register beyond the
        // three addresses, and no result can overwrite an address not yet used
        uint32_t s_ = ib + ta, k_ = ib + cls + c1, c_ = ba;
        asm volatile("ds_read_u16 %0, %0\n\tds_read_u8 %1, %1\n\tds_read_u8 %2, %2\n\ts_waitcnt lgkmcnt(0)"
                     : "+v"(s_), "+v"(k_), "+v"(c_)
                     :
                     : "memory");
        st = s_;
        k = k_;
        c2 = c_;
    } else {
        st = I.u16(ta);
        k = I.u8(cls + c1);
        c2 = C.at(p2);
    }
}

// First byte at or after pa (and before lim, inside the window) that ends a
// token, 16 bytes a step: kKind 0 = request target (<= 0x20 or DEL), 1 =
// header value (CTL other than HT, or DEL), 2 = simple header name (not
// [0-9A-Za-z-]).  lim if none.
template <int kKind>
__device__ __forceinline__ uint32_t find_stop(const Cursor &C, uint32_t pa, uint32_t lim) {
    while (pa < lim) {
        const uint4 w = C.chunk((pa - C.w) >> 4);
        uint32_t m = (kKind == 0 ? tstop_mask(w) : kKind == 1 ? vstop_mask(w) : nonalnum_mask(w)) & (0xFFFFu << (pa & 15));
        const uint32_t cend = (pa & ~15u) + 16;
        if (cend > lim) m &= (1u << (lim & 15)) - 1u;
        if (m) return (pa & ~15u) + (uint32_t)__builtin_ctz(m);
        pa = cend;
    }
    return lim;
}

// OWS after a header name is over (L.pa at the value's first byte, inside the
// window): a value nobody looks at is skipped, anything else is walked.
template <bool kLds>
__device__ __forceinline__ void ows_done(const Img<kLds> &I, Lane &L) {
    if (L.slot == kNoSlot && !(L.ninfo & (NI_CL | NI_TE))) {
        L.mode = M_SKIP;
    } else {
        L.mode = M_VALUE;
        if (L.slot != kNoSlot) {
            slot_begin(I, L, L.slot);
        } else {
            null_dfa(L);
        }
        L.in_ows = false;
        L.clv = 0;
        L.ndig = 0;
        L.cl_bad = L.cl_ws = false;
    }
}

// Header name -> slot, as at the end of M_NAME (L.ninfo set).
template <bool kLds>
__device__ __forceinline__ void name_slot(const Img<kLds> &I, Lane &L) {
    uint32_t s = kNoSlot;
    if (L.ninfo & NI_HOST) s = SLOT_AUTHORITY;
    else if (L.ninfo & NI_CUSTOM) s = SLOT_CUSTOM0 + (L.ninfo & NI_CUSTOM) - 1;
    if (s != kNoSlot && ((L.present >> s) & 1)) s = kNoSlot;                // first occurrence only
    if (s != kNoSlot && !((HDR_U32(I, ref_slots) >> s) & 1)) s = kNoSlot;  // nobody looks at it
    L.slot = s;
}

// A header line's start, 16 bytes at a time (L.mode == M_LINE, L.pa + 16 <=
// lim): the 16 bytes at L.pa are cut out of two window chunks at once.
//   "\r\n"                        -> end of the header block (M_ENDLF's work);
//   name of 1..15 [0-9A-Za-z-] + ":" -> the name's flags from the image's name
//                                    table in one probe (instead of a DFA step
//                                    per byte), its slot, and OWS over when it
//                                    ends inside the 16 bytes;
//   anything else                 -> left to the byte-wise framer (M_LINE).
// The outcome is exactly the byte-wise one's (DevNameEnt).
template <bool kLds>
__device__ __forceinline__ void fast_line(const Img<kLds> &I, Lane &L, const Cursor &C, const uint64_t *nfa_bits) {
    const uint32_t k0 = (L.pa - C.w) >> 4, o = L.pa & 15, i = o >> 2, sh = (o & 3) * 8;
    const uint4 a = C.chunk(k0), b = C.chunk(k0 + 1);  // (b unused when o == 0)
    const uint32_t d1 = i == 0 ? a.y : i == 1 ? a.z : i == 2 ? a.w : b.x;
    const uint32_t d0 = i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : a.w;
    const uint32_t d2 = i == 0 ? a.z : i == 1 ? a.w : i == 2 ? b.x : b.y;
    const uint32_t d3 = i == 0 ? a.w : i == 1 ? b.x : i == 2 ? b.y : b.z;
    const uint32_t d4 = i == 0 ? b.x : i == 1 ? b.y : i == 2 ? b.z : b.w;
    uint4 f;
    f.x = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
    f.y = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
    f.z = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
    f.w = (uint32_t)((((uint64_t)d4 << 32) | d3) >> sh);
    const uint32_t b0 = f.x & 0xFF;
    if (b0 == '\r') {  // M_LINE -> M_ENDLF -> headers_done
        if (((f.x >> 8) & 0xFF) != '\n') {
            finish(L, V_PARSE_ERROR);
        } else {
            L.pa += 2;
            headers_done(I, L, nfa_bits);
        }
        return;
    }
    const uint32_t e = (uint32_t)__builtin_ctz(nonalnum_mask(f) | 0x10000u);
    if (e == 0 || e == 16 || byte_of(f, e) != ':') return;  // the byte-wise framer decides
    const uint32_t nb = HDR_U8(I, ntab_bits);
    if (nb == 0) return;
    // lower-cased name bytes (OR 0x20 is exact on [0-9A-Za-z-]), zero past e
    auto keep = [e](uint32_t j) { return e >= 4 * j + 4 ? 0xFFFFFFFFu : e <= 4 * j ? 0u : (1u << (8 * (e - 4 * j))) - 1u; };
    const uint32_t w0 = (f.x | 0x20202020u) & keep(0), w1 = (f.y | 0x20202020u) & keep(1);
    const uint32_t w2 = (f.z | 0x20202020u) & keep(2), w3 = (f.w | 0x20202020u) & keep(3);
    const uint32_t h = l7_name_hash(w0, w1, w2, w3, e, HDR_U32(I, ntab_mul), nb);
    const uint32_t ent = HDR_U32(I, ntab_off) + h * (uint32_t)sizeof(DevNameEnt);
    const uint4 n = I.u128(ent);
    const uint32_t meta = I.u32(ent + 16);
    const bool hit = (meta & 0xFF) == e && n.x == w0 && n.y == w1 && n.z == w2 && n.w == w3;
    L.mark = L.pa;
    L.ninfo = hit ? (meta >> 8) & 0xFF : 0u;
    name_slot(I, L);
    // OWS: the first byte after ':' that is not SP / HT, if among the 16
    const uint32_t v = (uint32_t)__builtin_ctz((~ws_mask(f) & (0xFFFFu << (e + 1)) & 0xFFFFu) | 0x10000u);
    if (v < 16) {
        L.pa += v;
        ows_done(I, L);
    } else {
        L.pa += e + 1;
        L.mode = M_OWS;
    }
}

// ---------------------------------------------------------------- parse one window
// Consumes [L.pa, min(window end, request end)).  Every loop has a single
// exit; errors set the mode to M_DONE so later blocks fall through.
template <bool kLds>
__device__ __forceinline__ void parse_window(const Img<kLds> &I, Lane &L, Cursor &C, const uint64_t *nfa_bits) {
    const uint32_t lim = min(L.w + kWin, L.lena);
    C.w = L.w;
    const uint32_t ncls_name = HDR_U16(I, name_ncls);
    const uint32_t name_cls = HDR_U32(I, name_cls_off), name_trans = HDR_U32(I, name_trans_off);

    // ---- request line
    if (L.mode == M_METHOD) {  // 1*tchar SP
        // software pipeline as for the target
        uint32_t c = 0;
        if (L.pa < lim) {
            c = C.at(L.pa);
            uint32_t k = I.u8(L.dcls + c);
            uint32_t c1 = C.at(L.pa + 1);
            bool go = is_tchar(c);
            while (go) {
                uint32_t c2;
                walk_step(I, C, L.dtrans, L.drow, L.dcls, L.st, k, c1, L.pa + 2, c2);
                L.pa++;
                c = c1;
                c1 = c2;
                go = (L.pa < lim) & is_tchar(c);
            }
        }
        if (L.pa < lim) {
            if (c != ' ' || L.pa == L.mark) {
                finish(L, V_PARSE_ERROR);
            } else {
                slot_end(I, L);
                L.present |= 1u << SLOT_METHOD;
                L.pa++;
                L.mark = L.pa;
                L.mode = M_TARGET;
                slot_begin(I, L, SLOT_PATH);
            }
        }
    }
    if (L.mode == M_TARGET) {  // 1*(VCHAR / obs-text) SP
        uint32_t c = 0;
        if (L.pa < lim) {
            // software pipeline: the transition on byte p (the read the next
            // state waits for) is issued first, byte p+2 and the class of byte
            // p+1 behind it.  The look-ahead reads wrap inside the lane's slot
            // (Cursor::at) and their bytes are used only below lim; the loop
            // has one exit, taken with c the byte at L.pa whenever L.pa < lim.
            c = C.at(L.pa);
            uint32_t k = I.u8(L.dcls + c);
            uint32_t c1 = C.at(L.pa + 1);
            bool go = (c > 0x20) & (c != 0x7F) & walk_live(L);
            while (go) {
                uint32_t c2;
                walk_step(I, C, L.dtrans, L.drow, L.dcls, L.st, k, c1, L.pa + 2, c2);
                L.pa++;
                c = c1;
                c1 = c2;
                go = (L.pa < lim) & (c > 0x20) & (c != 0x7F) & walk_live(L);
            }
        }
        if (L.pa < lim && c > 0x20 && c != 0x7F) {  // absorbing state: the rest of the target cannot change it
            L.pa = find_stop<0>(C, L.pa, lim);
            c = L.pa < lim ? C.at(L.pa) : 0;
        }
        if (L.pa < lim) {
            if (c != ' ' || L.pa == L.mark) {
                finish(L, V_PARSE_ERROR);
            } else {
                slot_end(I, L);
                L.present |= 1u << SLOT_PATH;
                L.pa++;
                L.mark = 0;
                L.mode = M_VERSION;
            }
        }
    }
    if (L.mode == M_VERSION) {  // "HTTP/" DIGIT "." DIGIT CRLF
        if (L.mark == 0 && L.pa + 10 <= lim) {  // all ten bytes in the window: compare them at once
            const uint32_t k0 = (L.pa - L.w) >> 4, o = L.pa & 15, i = o >> 2, sh = o & 3;
            const uint4 a = C.chunk(k0), b = C.chunk(k0 + 1);  // (b unused when the bytes end in a)
            const uint32_t e0 = i == 0 ? a.x : i == 1 ? a.y : i == 2 ? a.z : a.w;
            const uint32_t e1 = i == 0 ? a.y : i == 1 ? a.z : i == 2 ? a.w : b.x;
            const uint32_t e2 = i == 0 ? a.z : i == 1 ? a.w : i == 2 ? b.x : b.y;
            const uint32_t e3 = i == 0 ? a.w : i == 1 ? b.x : i == 2 ? b.y : b.z;
            const uint32_t r0 = __builtin_amdgcn_alignbyte(e1, e0, sh);
            const uint32_t r1 = __builtin_amdgcn_alignbyte(e2, e1, sh);
            const uint32_t r2 = __builtin_amdgcn_alignbyte(e3, e2, sh);
            if (r0 == 0x50545448u && (r1 & 0x00FF00FFu) == 0x002E002Fu && ((r1 >> 8) & 0xFF) - '0' < 10u &&
                (r1 >> 24) - '0' < 10u && (r2 & 0xFFFFu) == 0x0A0Du) {
                L.pa += 10;
                L.mark = 10;
            }
        }
        for (; L.pa < lim && L.mark < 10; L.pa++, L.mark++) {
            const uint32_t c = C.at(L.pa);
            const uint32_t want = kVer[L.mark];
            if (want == 0x100 ? c - '0' >= 10u : c != want) break;
        }
        if (L.mark == 10) L.mode = M_LINE;
        else if (L.pa < lim) finish(L, V_PARSE_ERROR);
    }
    // ---- header lines
    while (L.mode >= M_LINE && L.mode < M_DONE && L.pa < lim) {
        if (L.mode == M_LINE && L.pa + 16 <= lim) fast_line(I, L, C, nfa_bits);
        if (L.mode == M_LINE) {
            if (C.at(L.pa) == '\r') {
                L.pa++;
                L.mode = M_ENDLF;
            } else {
                L.mode = M_NAME;
                L.mark = L.pa;
                L.nstate = kNameStart;
            }
        }
        if (L.mode == M_ENDLF && L.pa < lim) {
            if (C.at(L.pa) != '\n') {
                finish(L, V_PARSE_ERROR);
            } else {
                L.pa++;
                headers_done(I, L, nfa_bits);  // done, or a new pass from the request start
            }
        }
        if (L.mode == M_NAME) {  // 1*tchar ":"  (obs-fold SP/HT is not a tchar)
            uint32_t c = 0;
            if (L.pa < lim) {
                c = C.at(L.pa);
                uint32_t k = I.u8(name_cls + c);  // 0 = not a tchar
                uint32_t c1 = C.at(L.pa + 1);
                bool go = (k != 0) & (L.nstate != kNameOther);
                while (go) {
                    uint32_t c2;
                    walk_step(I, C, name_trans, 2 * ncls_name, name_cls, L.nstate, k, c1, L.pa + 2, c2);
                    L.pa++;
                    c = c1;
                    c1 = c2;
                    go = (L.pa < lim) & (k != 0) & (L.nstate != kNameOther);
                }
                if (L.pa < lim && k != 0) {
                    // a name the rule set does not know (the DFA state loops on
                    // every tchar): only where it ends matters.  [0-9A-Za-z-]
                    // runs are skipped 16 bytes a step, other tchars one by one.
                    L.pa = find_stop<2>(C, L.pa, lim);
                    c = L.pa < lim ? C.at(L.pa) : 0;
                    while (L.pa < lim && c != ':' && is_tchar(c)) {
                        L.pa++;
                        c = L.pa < lim ? C.at(L.pa) : 0;
                    }
                }
            }
            if (L.pa < lim) {
                if (c != ':' || L.pa == L.mark) {
                    finish(L, V_PARSE_ERROR);
                } else {
                    L.pa++;
                    L.ninfo = L.nstate >= kNameStart ? I.u8(HDR_U32(I, name_info_off) + L.nstate) : 0;
                    name_slot(I, L);
                    L.mode = M_OWS;
                }
            }
        }
        if (L.mode == M_OWS) {
            for (; L.pa < lim; L.pa++) {
                const uint32_t c = C.at(L.pa);
                if (c != ' ' && c != '\t') break;
            }
            if (L.pa < lim) ows_done(I, L);
        }
        if (L.mode == M_VALUE && !(L.ninfo & (NI_CL | NI_TE))) {  // a value some rule looks at: DFA walk only
            // software pipeline as for the target: byte p+1 and its class are
            // read while the transition on byte p is in flight
            uint32_t c = 0, nx = 0;  // nx: the byte after c when in hand (| 0x100)
            if (L.pa < lim) {
                c = C.at(L.pa);
                uint32_t k = I.u8(L.dcls + c);
                uint32_t c1 = C.at(L.pa + 1);
                // CR ends it, other CTLs are errors; an absorbing state outside an
                // OWS run ends the walk (trailing OWS needs the state before it)
                bool go = !value_stop(c) & (L.in_ows | walk_live(L));
                while (go) {
                    const bool ws = (c == ' ') | (c == '\t');
                    L.saved = (ws & !L.in_ows) ? L.st : L.saved;
                    L.in_ows = ws;
                    uint32_t c2;
                    walk_step(I, C, L.dtrans, L.drow, L.dcls, L.st, k, c1, L.pa + 2, c2);
                    L.pa++;
                    c = c1;
                    c1 = c2;
                    go = (L.pa < lim) & !value_stop(c) & (L.in_ows | walk_live(L));
                }
                if (L.pa + 1 < lim) nx = c1 | 0x100;
            }
            if (L.pa < lim && !((c < 0x20 && c != '\t') || c == 0x7F)) {  // absorbing: skip to the value's end
                L.pa = find_stop<1>(C, L.pa, lim);
                c = L.pa < lim ? C.at(L.pa) : 0;
                nx = 0;
            }
            if (L.pa < lim) {
                if (c != '\r') {
                    finish(L, V_PARSE_ERROR);
                } else {
                    if (L.in_ows) L.st = L.saved;  // trailing OWS is not part of the value
                    if (nx) {  // M_LF's work on the byte in hand
                        L.pa += 2;
                        if (nx != ('\n' | 0x100)) finish(L, V_PARSE_ERROR);
                        else if (line_done(I, L)) L.mode = M_LINE;
                        else finish(L, V_PARSE_ERROR);
                    } else {
                        L.pa++;
                        L.mode = M_LF;
                    }
                }
            }
        }
        if (L.mode == M_VALUE) {  // Content-Length / Transfer-Encoding (and possibly a rule's DFA on it)
            uint32_t c = 0;
            const bool te = (L.ninfo & NI_TE) != 0;
            for (; L.pa < lim; L.pa++) {
                c = C.at(L.pa);
                if ((c < 0x20 && c != '\t') || c == 0x7F) break;  // CR ends it; other CTLs are errors
                const bool ws = c == ' ' || c == '\t';
                if (ws && !L.in_ows) L.saved = L.st;
                L.in_ows = ws;
                if (!ws) {
                    if (te) {  // "chunked", case-insensitive, then trailing OWS only
                        const uint32_t want = (uint32_t)(0x64656B6E756863ull >> (8 * min(L.ndig, 7u))) & 0xFF;
                        L.ndig = (!L.cl_ws && L.ndig < 7 && (c | 0x20) == want) ? L.ndig + 1 : 0xFF;
                    } else if (c - '0' < 10u && !L.cl_ws) {
                        L.clv = L.clv * 10 + (c - '0');
                        L.ndig++;
                    } else {
                        L.cl_bad = true;
                    }
                }
                L.cl_ws |= ws;
                dfa_step(I, L, c);
            }
            if (L.pa < lim) {
                if (c != '\r') {
                    finish(L, V_PARSE_ERROR);
                } else {
                    if (L.in_ows) L.st = L.saved;  // trailing OWS is not part of the value
                    L.pa++;
                    L.mode = M_LF;
                }
            }
        }
        if (L.mode == M_SKIP) {  // a value nobody looks at: find CR (or a CTL / DEL) 16 bytes a step
            uint32_t stop = 0, next = 0;  // next: the byte after the stop when the chunk holds it (| 0x100)
            while (L.pa < lim) {
                const uint4 w = C.chunk((L.pa - L.w) >> 4);
                const uint32_t any = stop_bits(w.x) | stop_bits(w.y) | stop_bits(w.z) | stop_bits(w.w);
                uint32_t m = any ? stop_mask(w) & (0xFFFFu << (L.pa & 15)) : 0;
                const uint32_t cend = L.pa - (L.pa & 15) + 16;
                if (cend > lim) m &= (1u << (lim & 15)) - 1u;  // lim inside this chunk
                const uint32_t p = cend - 16 + (uint32_t)__builtin_ctz(m | 0x10000u);
                L.pa = min(p, lim);
                if (p < cend) {
                    const uint32_t c = byte_of(w, p & 15);
                    if (c != '\t') {
                        stop = c | 0x100;
                        if (p + 1 < cend && p + 1 < lim) next = byte_of(w, (p + 1) & 15) | 0x100;
                        break;
                    }
                    L.pa++;
                }
            }
            if (stop) {
                if (stop != ('\r' | 0x100)) {
                    finish(L, V_PARSE_ERROR);
                } else if (next) {  // M_LF's work on the byte in hand
                    L.pa += 2;
                    if (next != ('\n' | 0x100)) finish(L, V_PARSE_ERROR);
                    else if (line_done(I, L)) L.mode = M_LINE;
                    else finish(L, V_PARSE_ERROR);
                } else {
                    L.pa++;
                    L.mode = M_LF;
                }
            } else if (L.pa < L.lena) {
                L.scan = true;  // the value continues past the window: the wave scans it
            }
        }
        if (L.mode == M_LF && L.pa < lim) {
            if (C.at(L.pa) != '\n') {
                finish(L, V_PARSE_ERROR);
            } else {
                L.pa++;
                if (line_done(I, L)) L.mode = M_LINE;
                else finish(L, V_PARSE_ERROR);
            }
        }
    }
    // ---- chunked body: chunk = 1*HEXDIG [";" ext] CRLF data CRLF; size 0 ends
    // the chunks, then trailer lines up to an empty line (oracle/http_ref.c)
    while (L.mode > M_DONE && L.pa < lim) {
        const uint32_t c = C.at(L.pa);
        switch (L.mode) {
        case M_CHSIZE: {
            const uint32_t d = c - '0' < 10u ? c - '0' : (c | 0x20) - 'a' < 6u ? (c | 0x20) - 'a' + 10 : 0xFF;
            if (d != 0xFF) {
                L.clv = L.clv * 16 + d;
                L.pa++;
                if (L.clv > 0xFFFFFFFFull) finish(L, V_PARSE_ERROR);
            } else if (L.pa == L.mark) {
                finish(L, V_PARSE_ERROR);
            } else if (c == ';') {
                L.pa++;
                L.mode = M_CHEXT;
            } else if (c == '\r') {
                L.pa++;
                L.mode = M_CHLF;
            } else {
                finish(L, V_PARSE_ERROR);
            }
            break;
        }
        case M_CHEXT:
            if (c == '\n') finish(L, V_PARSE_ERROR);
            else if (c == '\r') L.mode = M_CHLF;
            L.pa++;
            break;
        case M_CHLF:
            if (c != '\n') { finish(L, V_PARSE_ERROR); break; }
            L.pa++;
            L.mode = L.clv ? M_CHDATA : M_TRL;
            break;
        case M_CHDATA:  // skip the data by its length
            if ((uint64_t)(L.pa - L.a0) + L.clv > 0xFFFFFFFFull) {
                finish(L, V_PARSE_ERROR);
            } else if ((uint64_t)L.pa + L.clv > L.lena) {
                L.pa = L.lena;
                finish(L, V_INCOMPLETE);
            } else {
                L.pa += (uint32_t)L.clv;
                L.mode = M_CHDCR;
            }
            break;
        case M_CHDCR:
            if (c != '\r') { finish(L, V_PARSE_ERROR); break; }
            L.pa++;
            L.mode = M_CHDLF;
            break;
        case M_CHDLF:
            if (c != '\n') { finish(L, V_PARSE_ERROR); break; }
            L.pa++;
            L.mode = M_CHSIZE;
            L.mark = L.pa;
            L.clv = 0;
            break;
        case M_TRL:
            if (c == '\n') { finish(L, V_PARSE_ERROR); break; }
            L.mode = c == '\r' ? M_TRLEND : M_TRLSCAN;
            L.pa++;
            break;
        case M_TRLSCAN:
            if (c == '\n') finish(L, V_PARSE_ERROR);
            else if (c == '\r') L.mode = M_TRLLF;
            L.pa++;
            break;
        case M_TRLLF:
            if (c != '\n') { finish(L, V_PARSE_ERROR); break; }
            L.pa++;
            L.mode = M_TRL;
            break;
        default:  // M_TRLEND
            if (c != '\n') { finish(L, V_PARSE_ERROR); break; }
            L.pa++;
            finish(L, L.verdict, L.rule);
            L.consumed = L.pa - L.a0;
            break;
        }
    }
}

}  // namespace

}  // namespace l7

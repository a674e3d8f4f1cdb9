// The Kafka wire decoder shared by the three kernels that walk requests:
// the classifier (kafka_classify.hip), the compressed-set kernel
// (kafka_inflate.hip) and the deny-reply walk (deny_reply.hip).  One decoder
// family over a byte source (KD<R>, kd_*: io.ReadFull / LimitReader reads,
// vendor/github.com/optiopay/kafka/proto/serialization.go:19-203), the plain
// byte source over the chunk cursor of kafka_dec.h (CurRd), and readMessageSet
// (messages.go:363-494) stated once: the steps of one message (kd_message) and
// the set loop on them (kd_message_set).  Product code.
#pragma once
#include "kafka_dec.h"

namespace l7 {
namespace {

// The request (or a decoded inner set) through the lane's 16-byte chunk cursor
// and nothing else: the byte source of the walks that keep no staging slot.
struct CurRd {
    static constexpr bool kWin = false;
    const uint8_t *b;
    Cur *c;
    __device__ __forceinline__ uint64_t be(uint32_t pos, int n) { return be_load(*c, b + pos, n); }
    __device__ __forceinline__ uint32_t le4(uint32_t pos) { return le_load4(*c, b + pos); }
};
// h.msg of a walk through it: the CRC through the cursor
struct CurCrc {
    const uint32_t *tab;
    CurRd r;
    __device__ __forceinline__ bool msg(uint32_t pos, uint32_t n, uint32_t stored) {
        return crc32_ieee(tab, *r.c, r.b + pos, n) == stored;
    }
};

// ---------------- io.ReadFull / LimitReader decoding over a byte source ----------------
template <class R>
struct KD {
    R *r;
    uint32_t pos, end;
    int32_t limit;  // LimitReader remaining, -1 = none
    int err;        // 0 ok, 1 EOF, 2 ErrUnexpectedEOF, 3 other
};
template <class R>
__device__ __forceinline__ uint32_t kd_read(KD<R> &d, uint32_t n) {
    const uint32_t at = d.pos;
    if (n == 0) return at;
    uint32_t a = d.end - d.pos;
    if (d.limit >= 0 && (uint32_t)d.limit < a) a = (uint32_t)d.limit;
    if (a == 0) { d.err = 1; return at; }
    const uint32_t take = a < n ? a : n;
    d.pos += take;
    if (d.limit >= 0) d.limit -= (int32_t)take;
    if (take < n) d.err = 2;
    return at;
}
template <class R>
__device__ __forceinline__ int64_t kd_int(KD<R> &d, int n) {
    if (d.err) return 0;
    const uint32_t at = kd_read(d, (uint32_t)n);
    if (d.err) return 0;
    const uint64_t v = d.r->be(at, n);
    return n == 1 ? (int64_t)(int8_t)v : n == 2 ? (int64_t)(int16_t)v : n == 4 ? (int64_t)(int32_t)v : (int64_t)v;
}
template <class R>
__device__ __forceinline__ void kd_skip(KD<R> &d, int n) {
    if (d.err) return;
    kd_read(d, (uint32_t)n);
}
template <class R>
__device__ __forceinline__ void kd_string(KD<R> &d, uint32_t &off, uint32_t &len) {  // DecodeString; len < 1 => ""
    off = 0; len = 0;
    if (d.err) return;
    const int16_t sl = (int16_t)kd_int(d, 2);
    if (d.err || sl < 1) return;
    const uint32_t at = kd_read(d, (uint32_t)sl);
    if (d.err) return;
    off = at; len = (uint32_t)sl;
}
template <class R>
__device__ __forceinline__ int32_t kd_arraylen(KD<R> &d, bool nullable, bool &bad) {  // DecodeArrayLen
    const int32_t l = (int32_t)kd_int(d, 4);
    bad = false;
    if (l < 0) { if (nullable) return -1; bad = true; return 0; }
    if ((uint32_t)l > kMaxParseBuf) { bad = true; return 0; }
    return l;
}
// np fixed-size entries whose fields are all skipped: passed in one step when
// they all lie inside the input (the per-field loop then cannot fail)
template <class R>
__device__ __forceinline__ bool kd_bulk(KD<R> &d, int32_t np, uint32_t esize) {
    if (d.err || np < 0) return false;
    uint32_t a = d.end - d.pos;
    if (d.limit >= 0 && (uint32_t)d.limit < a) a = (uint32_t)d.limit;
    const uint64_t need = (uint64_t)(uint32_t)np * esize;
    if (need > a) return false;
    d.pos += (uint32_t)need;
    if (d.limit >= 0) d.limit -= (int32_t)need;
    return true;
}
template <class R>
__device__ __forceinline__ void kd_bytes(KD<R> &d) {
    if (d.err) return;
    const int32_t sl = (int32_t)kd_int(d, 4);
    if (d.err || sl < 1) return;
    if ((uint32_t)sl > kMaxParseBuf) { d.err = 3; return; }
    kd_read(d, (uint32_t)sl);
}

// DecodeBytes kept as a span: the same reads and errors, and where the bytes
// lie (len 0: nil or empty)
template <class R>
__device__ __forceinline__ void kd_span(KD<R> &d, uint32_t &off, uint32_t &len) {
    off = 0; len = 0;
    if (d.err) return;
    const int32_t sl = (int32_t)kd_int(d, 4);
    if (d.err || sl < 1) return;
    if ((uint32_t)sl > kMaxParseBuf) { d.err = 3; return; }
    const uint32_t at = kd_read(d, (uint32_t)sl);
    if (d.err) return;
    off = at; len = (uint32_t)sl;
}

// One message of readMessageSet's loop (messages.go:363-494), read from the
// set's decoder: what the loop does next.
enum KMsgStep {
    kMsgError = -1,  // the request fails
    kMsgEnd = 0,     // the set ends here without an error (short read, size <= 0, CRC mismatch, codec 3): no drain
    kMsgPlain,       // an uncompressed message, read whole
    kMsgPacked,      // a gzip / snappy message, read whole: m says which and where its value lies
};
struct KMsg {
    int codec;
    uint32_t vat, vlen;
};
// h.msg(pos, len, stored) answers whether the CRC of the message's bytes
// [pos, pos + len) equals stored.
template <class R, class H>
__device__ __forceinline__ KMsgStep kd_message(KD<R> &dec, int16_t version, H &h, KMsg &m) {
    kd_skip(dec, 8);
    if (dec.err) return kMsgEnd;
    const int32_t msize = (int32_t)kd_int(dec, 4);
    if (dec.err || msize <= 0) return kMsgEnd;
    if ((uint32_t)msize > kMaxParseBuf) return kMsgError;
    const uint32_t at = kd_read(dec, (uint32_t)msize);
    if (dec.err) return kMsgEnd;
    KD<R> md{dec.r, at, at + (uint32_t)msize, -1, 0};
    const uint32_t crc = (uint32_t)kd_int(md, 4);
    if (msize <= 4) return kMsgEnd;
    if (!h.msg(at + 4, (uint32_t)msize - 4, crc)) return kMsgEnd;  // stop, no drain
    kd_skip(md, 1);
    const int8_t attr = (int8_t)kd_int(md, 1);
    if (version >= 1) kd_skip(md, 8);
    m.codec = attr & 3;
    if (m.codec == 3) return kMsgEnd;  // `return nil, err` with err == nil
    kd_bytes(md);
    kd_span(md, m.vat, m.vlen);
    if (md.err) return kMsgError;
    return m.codec ? kMsgPacked : kMsgPlain;
}

// readMessageSet on the shared position; 0 ok, -1 error.  The hooks: h.msg and,
// where the reader has a window (R::kWin), h.msg_win, the CRC compare of
// kd_message.  H::kLeaveAtPacked says what a compressed message does to the
// walk, the one place where the two users differ: the classifier (false) notes
// it in zflag for kafka_inflate_kernel, which decodes it (and reads its set),
// and goes on, since a successful decode changes nothing here; the deny-reply
// walk (true) leaves the set there, as its host twin proxylib/kafka_response.cc
// does.
template <class R, class H>
__device__ __forceinline__ int kd_message_set(R &r, uint32_t &pos, uint32_t end, int32_t size, int16_t version,
                                              bool &zflag, H &h) {
    if (size < 0) return 0;
    if ((uint32_t)size > kMaxParseBuf) return -1;
    KD<R> dec{&r, pos, end, size, 0};
    int rc = 0;
    if constexpr (!R::kWin) {
        for (;;) {
            KMsg m;
            const KMsgStep st = kd_message(dec, version, h, m);
            if (st <= kMsgEnd) { rc = st; break; }  // (0 or -1)
            if (st == kMsgPacked) {
                if constexpr (H::kLeaveAtPacked) break;
                zflag = true;
            }
        }
        pos = dec.pos;
        return rc;
    }
    // From here on: a reader with a window (the classifier's), which goes on
    // after a compressed message.
    static_assert(!R::kWin || !H::kLeaveAtPacked, "the window walk goes on after a compressed message");
    if constexpr (R::kWin) {
        // Messages whose header, key and value all lie inside the message and
        // the set take this path: one 36-byte window read per message (offset,
        // size, CRC, magic, attributes, [timestamp,] key length and, with no
        // key, value length), the fields at fixed places.  It takes exactly the
        // steps of the loop below and commits a message only when every one of
        // them succeeds; anything else goes to that loop, from the same message.
        const uint32_t hmin = version >= 1 ? 22u : 14u;  // crc magic attr [ts] klen vlen
        for (;;) {
            uint32_t avail = dec.end - dec.pos;
            if ((uint32_t)dec.limit < avail) avail = (uint32_t)dec.limit;
            if (avail < 12 + hmin) break;
            uint32_t x[9];
            r.win9(dec.pos, x);
            const uint32_t msize = bswap32(x[2]);
            if ((int32_t)msize < (int32_t)hmin || 12 + msize > avail) break;
            const uint32_t at = dec.pos + 12;
            const uint32_t crc = bswap32(x[3]);
            const uint32_t attr = (x[4] >> 8) & 0xFF;
            const int32_t klen = (int32_t)bswap32(version >= 1 ? __builtin_amdgcn_alignbyte(x[7], x[6], 2)
                                                               : __builtin_amdgcn_alignbyte(x[5], x[4], 2));
            const uint32_t ko = at + (version >= 1 ? 14u : 6u);  // key length field
            uint32_t vo = ko + 4;
            int32_t vlen;
            if (klen < 1) {
                vlen = (int32_t)bswap32(version >= 1 ? __builtin_amdgcn_alignbyte(x[8], x[7], 2)
                                                     : __builtin_amdgcn_alignbyte(x[6], x[5], 2));
            } else {
                if ((uint32_t)klen > msize || vo + (uint32_t)klen + 4 > at + msize) break;
                vo += (uint32_t)klen;
                // from the window in the slot when it holds the field (short
                // keys), else through the cursor, kept on byte at + 4's chunk
                // where the CRC starts (crc_head hashes it without a round trip)
                const uint32_t o = vo - r.span;
                if (o <= 60u) {
                    vlen = (int32_t)r.win_be4(o);
                } else {
                    const Cur keep = r.cur;
                    vlen = (int32_t)r.be(vo, 4);
                    r.cur = keep;
                }
            }
            if (vlen >= 1 && ((uint32_t)vlen > msize || vo + 4 + (uint32_t)vlen > at + msize)) break;
            // committed: the message is read whole
            dec.pos = at + msize;
            dec.limit -= (int32_t)(12 + msize);
            if (!h.msg_win(at + 4, msize - 4, crc)) { pos = dec.pos; return 0; }  // stop, no drain
            if ((attr & 3) == 3) { pos = dec.pos; return 0; }
            if (attr & 3) zflag = true;
        }
    }
    // The field-by-field loop, kd_message's steps written out, at function
    // scope as it always stood.  (Written on kd_message, or merely moved into
    // a block of its own, the classifier's kernels come out with other spill
    // counts and one of them with one more VGPR; they sit at their register
    // limits, so the loop stays as it was.)
    for (;;) {
        kd_skip(dec, 8);
        if (dec.err) break;
        const int32_t msize = (int32_t)kd_int(dec, 4);
        if (dec.err || msize <= 0) break;
        if ((uint32_t)msize > kMaxParseBuf) { rc = -1; break; }
        const uint32_t at = kd_read(dec, (uint32_t)msize);
        if (dec.err) break;
        KD<R> md{&r, at, at + (uint32_t)msize, -1, 0};
        const uint32_t crc = (uint32_t)kd_int(md, 4);
        if (msize <= 4) break;
        if (!h.msg(at + 4, (uint32_t)msize - 4, crc)) break;  // stop, no drain
        kd_skip(md, 1);
        const int8_t attr = (int8_t)kd_int(md, 1);
        if (version >= 1) kd_skip(md, 8);
        const int codec = attr & 3;
        if (codec == 3) break;  // `return nil, err` with err == nil
        kd_bytes(md);
        kd_bytes(md);
        if (md.err) { rc = -1; break; }
        if (codec != 0) zflag = true;  // (kLeaveAtPacked is false here)
    }
    pos = dec.pos;
    return rc;
}

}  // namespace
}  // namespace l7

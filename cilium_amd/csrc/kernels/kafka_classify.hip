// Kafka request classification on gfx950 (product code).
//
// One lane per request frame.  Each lane restates, sequentially over its own
// bytes, the reference's decode path: proto.ReadReq framing
// (vendor/github.com/optiopay/kafka/proto/messages.go:124-165), the typed
// decoders (:504-537, :767-824, :1033-1054, :1173-1228, :1389-1430,
// :1591-1647, :1810-1858) with io.ReadFull / LimitReader semantics
// (serialization.go:19-203), readMessageSet with CRC32-IEEE per message and
// stop-without-drain (:363-494), then MatchesRule (pkg/kafka/policy.go:200-225)
// against the connection's rule set using the precomputed topic / key views
// (engine/kafka_compile.h).  Requests with compressed messages are listed for
// kafka_inflate_kernel (kafka_inflate.hip), which decodes them.
//
// Round 5: the decoders are one template over the byte source (kafka_walk
// here; KD<R>, kd_* and kd_message_set in kafka_wire.h, shared with the
// compressed-set and deny-reply kernels), and the two loops that dominate
// the instruction count take a straight-line path when their input is well
// formed: a message whose
// header, key and value lie inside it and its set is read from one 36-byte
// window (three or four chunk loads issued together, the fields at fixed
// places), and a fetch / offsets / offset-fetch partition array whose
// fixed-size entries lie inside the request is passed in one step.  Anything
// else takes the field-by-field loop from the same position, so the verdicts
// are those of the reference's decoders either way.  (Round 5 also built and
// measured two restructurings, both bit-exact and both slower on produce
// requests: an LDS-staged walk with a segment-parallel CRC, and this walk
// with the CRCs deferred to a wave-cooperative pass; their sources are in git
// history at commit e7ccfd8 and their numbers in DESIGN.md.)
#include <hip/hip_runtime.h>

#include "../device_tables.h"
#include "kafka_wire.h"
#include "launch.h"

namespace l7 {

namespace {

constexpr int kBlock = 256;  // threads per workgroup: the CRC tables are shared by its waves


// The request in HBM through the lane's 16-byte chunk cursor.
struct GRd {
    static constexpr bool kWin = true;
    const uint8_t *b;
    uint32_t end;     // the request's length: the call's until the frame's is known, then that (every read
                      // lies inside the frame).  lastr(), the last 16-byte chunk holding a byte of it (window
                      // and block loads never pass it), as a ksched position (rel), is formed from it where
                      // it is used: the walk holds the length anyway, and a chunk address was two registers
    __device__ __forceinline__ uint32_t lastr() const {
        uint32_t e = end;
        asm volatile("" : "+v"(e));
        return (rel(e) - 1) & ~15u;
    }
    Cur cur;
    uint8_t *stage;   // the lane's CRC staging slot (win9 stages the message window there)
    uint32_t span;    // the span the slot holds: the 64 bytes from request byte span (modulo 2^32: the
                      // head's lies up to 15 bytes before byte 0), a 16-byte aligned address, or
                      // ksched::kNoSpan.  (ksched, kafka_sched.h, counts positions from the 16-byte aligned
                      // address at or below b: rel(pos).)  stage_head, win9 and the
                      // window-path CRC set it; the exact-path CRC takes the slot without saying what
                      // it leaves.  Chunks past lastr() hold that chunk's bytes, not their own: every field
                      // read here ends at or below the request's last byte (kd_read bounds it, a
                      // string's last word is masked), so it lies in chunks that hold their own.
    __device__ __forceinline__ const uint8_t *base() const {
        return reinterpret_cast<const uint8_t *>((uintptr_t)b & ~(uintptr_t)15);
    }
    __device__ __forceinline__ uintptr_t lastc() const { return (uintptr_t)base() + lastr(); }
    __device__ __forceinline__ uint32_t rel(uint32_t pos) const { return pos + (uint32_t)((uintptr_t)b & 15); }
    // The request's first 64 bytes (size, kind, version, client id, and for a
    // produce its acks, timeout, first topic and partition) staged into the
    // slot in one round trip; the fields there are read from LDS until win9 or
    // a CRC takes the slot over, where the cursor took a round trip per chunk
    // (cfg5 Kafka 15.54 -> 15.26 ms)
    __device__ __forceinline__ void stage_head() {
        crc_stage_at(stage, base(), 0, lastr());
        span = 0u - rel(0);
    }
    // little-endian 4 bytes at byte rel (rel + 4 <= 64) of the staged chunks
    __device__ __forceinline__ uint32_t slot_le4(uint32_t rel) {
        // (the addresses are formed here, at the read: hoisted out of the message loops they were
        // two more values held across the CRC, and spilled)
        asm volatile("" : "+v"(rel));
        const uint32_t la = (uint32_t)(uintptr_t)(stage + 16 * lane_id());
        const uint32_t w0 = rel >> 2, w1 = w0 < 15 ? w0 + 1 : 15;
        uint32_t lo, hi;
        asm volatile("s_waitcnt vmcnt(0)\n\tds_read_b32 %0, %2\n\tds_read_b32 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(lo), "=&v"(hi)
                     : "v"(la + ((w0 >> 2) << 10) + ((w0 & 3) << 2)), "v"(la + ((w1 >> 2) << 10) + ((w1 & 3) << 2))
                     : "memory");
        return __builtin_amdgcn_alignbyte(hi, lo, rel & 3);
    }
    // A field whose four bytes lie in the span comes from the slot, any other
    // through the cursor (which a slot read leaves as it is): after a message
    // set the slot holds the block its last message ended in, so the partition
    // or topic header behind the set is read without a round trip as far as
    // that block reaches.
    __device__ __forceinline__ uint32_t le4(uint32_t pos) {
        const uint32_t o = pos - span;
        if (o <= 60u) return slot_le4(o);
        return le_load4(cur, b + pos);
    }
    __device__ __forceinline__ uint64_t be(uint32_t pos, int n) {
        const uint32_t o = pos - span;
        if (n <= 4 && o <= 60u) {
            const uint32_t v = bswap32(slot_le4(o));
            return n == 4 ? v : v >> (32 - 8 * n);
        }
        return be_load(cur, b + pos, n);
    }
    // bytes [pos, pos + 36) as little-endian words.  When the span holds them
    // (the block the message before ended in, which the CRC left in the slot)
    // they are cut from it as they lie; else the four chunks that can hold them
    // are staged together into the slot (one memory round trip), chunks past the
    // request's last one clamped to it (their bytes are never used), and read
    // back.  The cursor is left on the chunk of byte pos + 16, where the
    // message's CRC input starts, and the slot keeps the window block for the
    // CRC (crc32_ieee_window: its bytes there cost no further round trip; cfg5
    // Kafka 16.06 -> 15.53 ms)
    __device__ __forceinline__ void win9(uint32_t pos, uint32_t (&x)[9]) {
        const uintptr_t a = (uintptr_t)(b + pos);
        const uintptr_t c0 = a & ~(uintptr_t)15;
        uint32_t w[16];
        {
            const uint32_t s = rel(pos);
            const uint32_t wb = ksched::window_base(span + rel(0), s);
            if (wb - rel(0) != span) {
                span = wb - rel(0);
                crc_stage_at(stage, base(), wb, lastr());
            }
            // the window's first chunk is the slot's first or (s - wb >= 16, at most 28) its second,
            // and then its last word lies in the slot's fourth chunk, which is read as that
            const uint32_t la3 = (uint32_t)(uintptr_t)(stage + 16 * lane_id()) + 3072;
            const uint32_t la = la3 - 3072 + (((s - wb) >> 4) << 10);
            uint4 v0, v1, v2, v3;
            asm volatile("s_waitcnt vmcnt(0)\n\t"
                         "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\t"
                         "ds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %5\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=v"(v0), "=v"(v1), "=v"(v2), "=v"(v3)
                         : "v"(la), "v"(la3)
                         : "memory");
            const uint4 vv[4] = {v0, v1, v2, v3};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                w[4 * k] = vv[k].x; w[4 * k + 1] = vv[k].y; w[4 * k + 2] = vv[k].z; w[4 * k + 3] = vv[k].w;
            }
        }
        const uint32_t s = (uint32_t)(a & 15), q = s >> 2;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const uint32_t lo = q == 0 ? w[i] : q == 1 ? w[i + 1] : q == 2 ? w[i + 2] : w[i + 3];
            const uint32_t hi = q == 0 ? w[i + 1] : q == 1 ? w[i + 2] : q == 2 ? w[i + 3] : w[i + 4];
            x[i] = __builtin_amdgcn_alignbyte(hi, lo, s & 3);
        }
        // byte pos + 16 is in chunk 1 (s < 16): hand it to the cursor
        cur.line = (rel(pos) & ~15u) + 16 <= lastr() ? c0 + 16 : ~(uintptr_t)0;
        cur.w0 = w[4]; cur.w1 = w[5]; cur.w2 = w[6]; cur.w3 = w[7];
    }
    // big-endian 4 bytes at byte o (o + 4 <= 64) of the slot, which holds the window block win9 left
    // there: a field past the 36 bytes win9 returns, without a round trip
    __device__ __forceinline__ uint32_t win_be4(uint32_t o) { return bswap32(slot_le4(o)); }
};

__device__ __forceinline__ bool is_topic_api_key(int k) {
    // 0 1 2 3 4 5 6 8 9 19 20 21 23 24 27 28 34 35 37
    if (k < 0 || k > 37) return false;
    const uint64_t m = (1ull << 0) | (1ull << 1) | (1ull << 2) | (1ull << 3) | (1ull << 4) | (1ull << 5) | (1ull << 6) |
                       (1ull << 8) | (1ull << 9) | (1ull << 19) | (1ull << 20) | (1ull << 21) | (1ull << 23) |
                       (1ull << 24) | (1ull << 27) | (1ull << 28) | (1ull << 34) | (1ull << 35) | (1ull << 37);
    return (m >> k) & 1;
}
__device__ __forceinline__ int kind_typed(int kind) {  // 0 nil request, 1 typed with topics/ClientID, 2 ConsumerMetadata
    return (kind == 0 || kind == 1 || kind == 2 || kind == 3 || kind == 8 || kind == 9) ? 1 : (kind == 10 ? 2 : 0);
}

// The typed decoders of one request after its frame checks (kinds 0 1 2 3 8 9
// 10); h.client(off, len) gets the ClientID, h.topic(off, len) each topic
// string in wire order.  0 ok, -1 error.
template <class R, class H>
__device__ __forceinline__ int kafka_walk(R &r, uint32_t rawlen, int kind, bool &zflag, H &h) {
    KD<R> d{&r, 0, rawlen, -1, 0};
    bool bad = false;
    int rc = 0;
    kd_skip(d, 4); kd_skip(d, 2);
    const int16_t ver = (int16_t)kd_int(d, 2);
    kd_skip(d, 4);
    uint32_t co, cl;
    kd_string(d, co, cl);
    if (!d.err && cl > 0) h.client(co, cl);
    int32_t nt, np;
    uint32_t o, l;
    switch (kind) {
    case 0:  // Produce
        if (ver >= 3) kd_string(d, o, l);
        kd_skip(d, 2); kd_skip(d, 4);
        nt = kd_arraylen(d, false, bad);
        if (bad) { rc = -1; break; }
        // (both loops count down: the count and the index were two registers each across the sets' CRCs)
        for (; nt > 0 && rc == 0; nt--) {
            kd_string(d, o, l);
            if (d.err) break;
            h.topic(o, l);
            np = kd_arraylen(d, false, bad);
            if (bad) { rc = -1; break; }
            for (; np > 0; np--) {
                kd_skip(d, 4);
                if (d.err) { rc = -1; break; }
                const int32_t ss = (int32_t)kd_int(d, 4);
                if (d.err) { rc = -1; break; }
                rc = kd_message_set(r, d.pos, d.end, ss, ver, zflag, h);
                if (rc) break;
            }
        }
        break;
    case 1:  // Fetch
        kd_skip(d, 4); kd_skip(d, 4); kd_skip(d, 4);
        if (ver >= 3) kd_skip(d, 4);
        if (ver >= 4) kd_skip(d, 1);
        nt = kd_arraylen(d, false, bad);
        if (bad) { rc = -1; break; }
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            h.topic(o, l);
            np = kd_arraylen(d, false, bad);
            if (bad) { rc = -1; break; }
            if (kd_bulk(d, np, ver >= 5 ? 24u : 16u)) continue;
            for (int32_t p = 0; p < np && !d.err; p++) {
                kd_skip(d, 4); kd_skip(d, 8);
                if (ver >= 5) kd_skip(d, 8);
                kd_skip(d, 4);
            }
        }
        break;
    case 2:  // Offset
        kd_skip(d, 4);
        if (ver >= 2) kd_skip(d, 1);
        nt = kd_arraylen(d, false, bad);
        if (bad) { rc = -1; break; }
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            h.topic(o, l);
            np = kd_arraylen(d, false, bad);
            if (bad) { rc = -1; break; }
            if (kd_bulk(d, np, ver == 0 ? 16u : 12u)) continue;
            for (int32_t p = 0; p < np && !d.err; p++) {
                kd_skip(d, 4); kd_skip(d, 8);
                if (ver == 0) kd_skip(d, 4);
            }
        }
        break;
    case 3:  // Metadata
        nt = kd_arraylen(d, true, bad);
        if (bad) { rc = -1; break; }
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            if (!d.err) h.topic(o, l);
        }
        if (ver >= 4) kd_skip(d, 1);
        break;
    case 8:  // OffsetCommit
        kd_string(d, o, l);
        if (ver >= 1) { kd_skip(d, 4); kd_string(d, o, l); }
        if (ver >= 2) kd_skip(d, 8);
        nt = kd_arraylen(d, false, bad);
        if (bad) { rc = -1; break; }
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            h.topic(o, l);
            np = kd_arraylen(d, false, bad);
            if (bad) { rc = -1; break; }
            for (int32_t p = 0; p < np && !d.err; p++) {
                kd_skip(d, 4); kd_skip(d, 8);
                if (ver == 1) kd_skip(d, 8);
                uint32_t o2, l2;
                kd_string(d, o2, l2);
            }
        }
        break;
    case 9:  // OffsetFetch
        kd_string(d, o, l);
        nt = kd_arraylen(d, true, bad);
        if (bad) { rc = -1; break; }
        for (int32_t t = 0; t < nt && !d.err; t++) {
            kd_string(d, o, l);
            h.topic(o, l);
            np = kd_arraylen(d, false, bad);
            if (bad) { rc = -1; break; }
            if (kd_bulk(d, np, 4u)) continue;
            for (int32_t p = 0; p < np && !d.err; p++) kd_skip(d, 4);
        }
        break;
    case 10:  // ConsumerMetadata
        kd_string(d, o, l);
        if (ver >= 1) kd_skip(d, 1);
        break;
    }
    if (rc == 0 && d.err) rc = -1;
    return rc;
}

// Interned id of the request string at [pos, pos + n) (topic or client id),
// -1 if the rule tables do not know it: word hash (l7_whash_*), linear
// probing, then a word-wise compare: the first 16 bytes against the slot's
// copy (the words were read for the hash), the rest against the 4-byte
// aligned, zero-padded table string.
template <class R>
__device__ __forceinline__ int32_t str_lookup(const DevStrSlot *tab, uint32_t mask, const uint8_t *strings, R &r,
                                              uint32_t pos, uint32_t n) {
    uint32_t h = kWHashSeed;
    uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;  // the first 16 bytes, zero-padded
    for (uint32_t i = 0; i < n; i += 4) {
        const uint32_t rem = n - i;
        const uint32_t keep = rem >= 4 ? 0xFFFFFFFFu : (1u << (8 * rem)) - 1u;
        const uint32_t w = r.le4(pos + i) & keep;
        h = l7_whash_step(h, w);
        p0 = i == 0 ? w : p0;
        p1 = i == 4 ? w : p1;
        p2 = i == 8 ? w : p2;
        p3 = i == 12 ? w : p3;
    }
    h = l7_whash_final(h, n);
    for (uint32_t slot = h & mask;; slot = (slot + 1) & mask) {
        const DevStrSlot e = tab[slot];
        if (!e.used) return -1;
        if (e.hash == h && e.len == n) {
            bool eq = e.pre[0] == p0 && e.pre[1] == p1 && e.pre[2] == p2 && e.pre[3] == p3;
            const uint32_t *t = reinterpret_cast<const uint32_t *>(strings + e.str_off);
            for (uint32_t i = 16; i < n && eq; i += 4) {
                const uint32_t rem = n - i;
                const uint32_t keep = rem >= 4 ? 0xFFFFFFFFu : (1u << (8 * rem)) - 1u;
                eq = t[i >> 2] == (r.le4(pos + i) & keep);
            }
            if (eq) return e.id;
        }
    }
}

struct ReqInfo {
    // One word, not three: kind, version and the typed class were three registers held across the walk
    // and its CRCs, and at 6 waves per SIMD (80 VGPRs) three spilled ones.  Each use extracts its field.
    uint32_t kv;    // kind << 16 | version (both int16, as on the wire)
    int32_t client; // interned id, -2 unknown / empty
    __device__ __forceinline__ int kind_() const { return (int)(int16_t)(kv >> 16); }
    __device__ __forceinline__ int version_() const { return (int)(int16_t)(kv & 0xFFFF); }
    // 0 nil request, 1 typed with topics/ClientID, 2 ConsumerMetadata
    __device__ __forceinline__ int typed_() const { return kind_typed(kind_()); }
};

__device__ __forceinline__ bool rule_matches(const DevKafkaRule &r, const ReqInfo &q) {
    if (!r.any_key && (q.kind_() < 0 || q.kind_() > 63 || !((r.keymask >> q.kind_()) & 1))) return false;
    if (r.has_version && r.version != q.version_()) return false;
    if (!r.has_topic && r.client < 0) return true;
    if (q.typed_() == 1) return r.client < 0 || r.client == q.client;
    if (q.typed_() == 2) return true;
    return !(r.has_topic && is_topic_api_key(q.kind_()));
}

// first position of topic `tid`'s rule list that matches, kInf if none
__device__ __forceinline__ uint32_t topic_first(const KafkaTables &T, const DevKafkaRuleset &rs, const ReqInfo &q,
                                                int32_t tid) {
    if (tid < 0 || rs.ntopics == 0) return kInf;
    uint32_t off, cnt;
    if (rs.tdense_off != ~0u) {
        const uint4 *ep = reinterpret_cast<const uint4 *>(T.index + rs.tdense_off +
                                                          (uint32_t)(sizeof(DevKafkaTopicEnt) / 4) * (uint32_t)tid);
        const uint4 e0 = ep[0], e1 = ep[1], e2 = ep[2];
        off = e0.y;
        cnt = e0.z;
        if (cnt == 0) return kInf;
        DevKafkaRule r0;
        const uint32_t w[6] = {e1.x, e1.y, e1.z, e1.w, e2.x, e2.y};
        __builtin_memcpy(&r0, w, sizeof r0);
        if (rule_matches(r0, q)) return e0.x;
        for (uint32_t i = 1; i < cnt; i++) {
            const uint32_t p = T.index[off + i];
            if (rule_matches(T.rules[rs.rule_first + p], q)) return p;
        }
        return kInf;
    } else {
        const uint32_t *dir = T.index + rs.topics_off;
        uint32_t lo = 0, hi = rs.ntopics;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (dir[3 * m] < (uint32_t)tid) lo = m + 1; else hi = m;
        }
        if (lo >= rs.ntopics || dir[3 * lo] != (uint32_t)tid) return kInf;
        off = dir[3 * lo + 1];
        cnt = dir[3 * lo + 2];
    }
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t p = T.index[off + i];
        if (rule_matches(T.rules[rs.rule_first + p], q)) return p;
    }
    return kInf;
}

// MatchesRule over a decoded request: ntopics topics whose best first-match
// positions' maximum is cmax.  Returns the allowing rule's position or kInf.
__device__ __forceinline__ uint32_t matches_rule(const KafkaTables &T, const DevKafkaRuleset &rs, const ReqInfo &q,
                                                 uint32_t ntopics, uint32_t cmax) {
    uint32_t best = kInf;
    if (ntopics == 0) {
        const int key = (q.kind_() >= 0 && q.kind_() < 64) ? q.kind_() : 64;
        const uint32_t off = T.index[rs.bykey_off + 2 * key], cnt = T.index[rs.bykey_off + 2 * key + 1];
        for (uint32_t i = 0; i < cnt; i++) {
            const uint32_t p = T.index[off + i];
            if (rule_matches(T.rules[rs.rule_first + p], q)) { best = p; break; }
        }
    } else {
        for (uint32_t i = 0; i < rs.ntopicless; i++) {
            const uint32_t p = T.index[rs.topicless_off + i];
            if (p >= cmax) break;  // cannot beat topic completion
            if (rule_matches(T.rules[rs.rule_first + p], q)) { best = p; break; }
        }
        if (best == kInf) best = cmax;
    }
    return best;
}

// ---------------- the lane-serial classification ----------------
// What the hooks keep for the access log (l7g_classify_logged): nothing, or the
// request's row of topic-name spans.
struct NoTopicLog {};
struct TopicLog {
    LogSpan *row;
    uint32_t stride;
};
template <class L>
struct ExactHooks {
    static constexpr bool kLeaveAtPacked = false;  // (kd_message_set: listed for kafka_inflate_kernel)
    const KafkaTables &T;
    int32_t rsi;  // the connection's rule set, T.rulesets[rsi]: its address is formed at each use (the index is
                  // one register across the walk, the address two)
    ReqInfo &q;
    GRd &r;
    const uint32_t *crctab;
    uint8_t *stage;
    uint32_t ntopics, cmax;
    L log;
    __device__ __forceinline__ const DevKafkaRuleset &rs() const {
        int32_t k = rsi;
        asm volatile("" : "+v"(k));
        return T.rulesets[k];
    }
    __device__ __forceinline__ void client(uint32_t o, uint32_t l) {
        q.client = str_lookup(T.client_hash, T.client_mask, T.strings, r, o, l);
        if (q.client < 0) q.client = -2;
    }
    __device__ __forceinline__ void topic(uint32_t o, uint32_t l) {
        if (q.typed_() != 1) return;
        if constexpr (!std::is_same<L, NoTopicLog>::value) {
            // GetTopics(): every topic in wire order, duplicates kept; the row holds the first `stride`
            if (ntopics < log.stride) log.row[ntopics] = LogSpan{o, l};
        }
        ntopics++;
        const int32_t tid = l > 0 ? str_lookup(T.topic_hash, T.topic_mask, T.strings, r, o, l) : -1;
        const uint32_t e = topic_first(T, rs(), q, tid);
        cmax = cmax > e ? cmax : e;
    }
    // CRC32-IEEE of the message bytes [pos, pos + n) against the stored value
    __device__ __forceinline__ bool msg(uint32_t pos, uint32_t n, uint32_t stored) {
        r.span = ksched::kNoSpan;  // the CRC takes the slot over
        return crc32_ieee_staged(crctab, r.cur, r.b + pos, n, stage, r.lastc()) == stored;
    }
    // the same, right after the walk's window read of this message (kd_message_set's fast path)
    // (whatever the answer, the slot then holds the block the message ended in, or still its window block)
    __device__ __forceinline__ bool msg_win(uint32_t pos, uint32_t n, uint32_t stored) {
        const uint32_t p = r.rel(pos), wb = r.rel(r.span);
        r.span = ksched::keep_base(wb, p + n) - r.rel(0);
        return crc32_ieee_window(crctab, r.cur, r.b, wb, p, p + n, stage, r.lastr()) == stored;
    }
};

}  // namespace

// sel: this protocol's request indices from partition_kernel (mixed batches),
// else requests 0..n-1.  answer_other: answer entries on connections that are
// not Kafka (single-protocol engines, where partition_kernel does not run).
// kWaves: waves per SIMD it is built for -- 6 (80 VGPRs) when memcached runs
// beside it in the workgroup slot it leaves per CU, 5 (96 VGPRs, almost no
// spills) when it runs alone (cfg3 0.619 -> 0.601 ms; beside memcached the
// 5-wave build loses: profiles/r6/ab6za_*).
// kLog (l7g_classify_logged): the same classification, and beside each ALLOW /
// DENY verdict the request's access-log record (LogRec, device_tables.h) and,
// from the topic hook, the first lstride topic-name spans into its row of
// ltopics.  Where a produce request's later topics begin depends on its
// messages' CRCs (a message set that stops without draining), so the spans come
// from this walk, not from a second pass.  The unlogged instantiations ignore
// the last three arguments.  The logged one is built for 4 waves per SIMD, where
// the extra live values (row pointer, stride, record words) fit without spills.
template <int kWaves, bool kLog>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kWaves, 8))) void kafka_classify_kernel(
    Batch B, KafkaTables T, const uint32_t *__restrict__ sel, const uint32_t *__restrict__ sel_count,
    uint32_t answer_other, uint32_t *__restrict__ zlist, uint32_t *__restrict__ zcount, uint32_t *__restrict__ work,
    uint32_t main_sweep, LogRec *__restrict__ lrec, LogSpan *__restrict__ ltopics, uint32_t lstride) {
    const uint32_t n = B.n, nconns = B.nconns;
    static_assert(kBlock >= 256, "one CRC table entry per thread");
    __shared__ uint32_t crctab[kCrcTables * 256];
    // per wave: the CRC's 64-byte-per-lane staging area (crc32_ieee_staged)
    __shared__ __attribute__((aligned(16))) uint8_t crcstage[kBlock / 64][4096];
    // (the wave's index as a scalar: the slot's address stays in scalar registers, not in a VGPR per lane)
    uint8_t *stage = crcstage[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))];
    crc_tables_init<kBlock>(crctab, threadIdx.x);
    // (L7_KAFKA_CLASSES length classes, class c at sel + c * n, sel_count[c] entries each)
    constexpr int kCls = L7_KAFKA_CLASSES;
    uint32_t kc[kCls] = {n};
    uint32_t m = n;
    if (sel) {
        m = 0;
        for (int c = 0; c < kCls; c++) { kc[c] = sel_count[c]; m += kc[c]; }
    }
    // Entries after the grid's first sweep are taken 64 at a time (one per
    // lane) by whichever wave is free, from a per-launch counter the launcher
    // zeroes, so the persistent grid's waves finish together; else (no
    // counter) a fixed stride.  A lane whose entry is past the list end has no
    // later one either, so the loop may run divergent.
    // (Taking 2 or 4 groups per atomic: cfg3 0.62 -> 0.77 / 1.07 ms, the
    // longest-first order makes the tail longer; profiles/r5/ab5e_*.)
    // main_sweep != 0: this launch is the helper grid beside the main one (whose
    // first sweep is that many entries): it takes no sweep of its own, only
    // groups from the counter, so both grids draw from one sequence and every
    // entry is taken exactly once.
    const uint32_t stride = main_sweep ? main_sweep : gridDim.x * kBlock;
    auto next_entry = [&](uint32_t i) -> uint32_t {
        if (!work) return i + stride;
        const uint32_t lane = lane_id();
        uint32_t t = 0;
        if (lane == (uint32_t)__builtin_amdgcn_readfirstlane(lane)) t = atomicAdd(work, 64u);
        return stride + __builtin_amdgcn_readfirstlane(t) + lane;
    };
    for (uint32_t i = main_sweep ? next_entry(0) : blockIdx.x * kBlock + threadIdx.x; i < m; i = next_entry(i)) {
        uint32_t idx = i;
        if (sel) {
            // the length classes longest first: long produce requests start first, short ones fill the tail
            // (unrolled over constant indices: a loop indexing kc[] kept it in scratch, a chain of
            // dependent scratch loads per entry)
            uint32_t c = 0, j = i;
            bool hit = false;
#pragma unroll
            for (int k = kCls - 1; k > 0; k--) {
                if (!hit) {
                    if (j >= kc[k]) j -= kc[k];
                    else { c = (uint32_t)k; hit = true; }
                }
            }
            idx = sel[(size_t)c * n + j];
        }
        const uint32_t ci = B.conn_ids[idx];
        const DevConn conn = L7_CONN(B.conns, nconns, ci);
        const uint64_t off = B.offs[idx];
        const uint32_t len = B.lens[idx];
        uint8_t verdict = V_PARSE_ERROR;
        int32_t rule = -1;
        uint32_t consumed = 0;
        bool zflag = false;  // compressed messages passed: kafka_inflate_kernel decides them
        if (conn.proto != PROTO_KAFKA || conn.ruleset < 0 || (uint32_t)conn.ruleset >= T.nrulesets) {
            if (!answer_other || (L7_PROTO_OWNED(conn.proto) && conn.proto != PROTO_KAFKA)) continue;
            verdict = V_UNSUPPORTED;  // unknown connection / no parser
        }
        // ---- proto.ReadReq
        do {
            if (verdict == V_UNSUPPORTED) break;
            if (!l7_in_arena(off, len, B.arena_len)) { verdict = V_UNSUPPORTED; break; }  // out of contract
            if (len < 4) { verdict = V_INCOMPLETE; break; }
            GRd r{B.arena + off, len, {}, stage, ksched::kNoSpan};
            r.stage_head();
            r.cur.line = ~(uintptr_t)0;
            const int32_t size = (int32_t)r.be(0, 4);
            if (size <= 0) break;
            if (len < 6) { verdict = V_INCOMPLETE; break; }
            if ((uint64_t)(uint32_t)size + 4 > kMaxParseBuf) break;
            const uint32_t rawlen = (uint32_t)size + 4;
            if (rawlen > len) { verdict = V_INCOMPLETE; break; }
            r.end = rawlen;
            if (rawlen < 12) break;
            ReqInfo q;
            q.kv = (uint32_t)r.be(4, 4);  // (rawlen >= 12: both fields)
            q.client = -2;
            // fields are read where they are used: a copy would hold 9 VGPRs across the decode
            using Log = typename std::conditional<kLog, TopicLog, NoTopicLog>::type;
            Log lg{};
            if constexpr (kLog) lg = TopicLog{ltopics + (size_t)idx * lstride, lstride};
            ExactHooks<Log> h{T, conn.ruleset, q, r, crctab, stage, 0, 0, lg};
            if (q.typed_() && kafka_walk(r, rawlen, q.kind_(), zflag, h) == -1) break;
            consumed = rawlen;
            verdict = V_DENY;
            if constexpr (kLog) {
                const uint32_t corr = (uint32_t)r.be(8, 4);  // (rawlen >= 12)
                uint4 *o = reinterpret_cast<uint4 *>(lrec + idx);
                // (kind in the upper half of word 0, version in word 1, each as its 16 wire bits)
                o[0] = make_uint4(LOG_KAFKA | (h.ntopics > lstride ? 0x100u : 0u) | (q.kv & 0xFFFF0000u),
                                  q.kv & 0xFFFFu, corr, h.ntopics);
                o[1] = make_uint4(0, 0, 0, 0);
            }
            const DevKafkaRuleset &rs = h.rs();
            if (!rs.any) break;
            const uint32_t best = matches_rule(T, rs, q, h.ntopics, h.cmax);
            if (best != kInf) { verdict = V_ALLOW; rule = T.rules[rs.rule_first + best].gid; }
        } while (false);
        B.verdict[idx] = verdict;
        B.rule[idx] = rule;
        B.consumed[idx] = consumed;
        if (zflag && zlist && (verdict == V_ALLOW || verdict == V_DENY)) zlist[atomicAdd(zcount, 1u)] = idx;
    }
}

hipError_t KafkaPhaseTimes(uint64_t *, bool) { return hipErrorNotSupported; }

// leave_per_cu > 0 (persistent grid only): that many workgroup slots per CU left
// free for a kernel running beside this one on another stream
// helper (with leave_per_cu > 0 and a counter): not the main grid but a second, small one for the slots
// the main grid left, launched behind the kernel that ran in them; it draws from the same counter
// log (l7g_classify_logged): the logged instantiations, which also write the records and topic rows
hipError_t LaunchKafkaClassify(const Batch &B, const KafkaTables &T, const uint32_t *sel, const uint32_t *sel_count,
                               bool answer_other, uint32_t *zlist, uint32_t *zcount, uint32_t *work,
                               hipStream_t stream, int leave_per_cu, bool helper, const LogOut *log) {
    if (B.n == 0) return hipSuccess;
    uint32_t blocks = (B.n + kBlock - 1) / kBlock;
    const bool beside = leave_per_cu > 0;
    if (helper && (!beside || !work)) return hipErrorInvalidValue;
    const bool lg = log != nullptr;
    // (logged: one build for both places, the 4-wave one -- 118 VGPRs, no spill and no scratch, where
    // the 5-wave build spills 21 VGPRs and the 6-wave one 37; profiles/access_log/kernel_resources.txt)
    const auto kernel = lg ? kafka_classify_kernel<4, true>
                           : (beside ? kafka_classify_kernel<6, false> : kafka_classify_kernel<5, false>);
    // persistent grid: as many workgroups as the CUs hold at once (per build)
    static int per_cu[2][2] = {};
    if (per_cu[lg][beside] == 0) {
        int p = 0;
        per_cu[lg][beside] =
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&p, kernel, kBlock, 0) == hipSuccess && p > 0 ? p : 32;
    }
    const int pc = per_cu[lg][beside], ncu = DeviceCuCount();
    const int slots = beside && pc > leave_per_cu ? pc - leave_per_cu : pc;
    if (!work) blocks = blocks > 8192 ? 8192 : blocks;  // grid-stride beyond this
    else if (blocks > (uint32_t)(ncu * slots)) blocks = (uint32_t)(ncu * slots);
    // (helper: blocks is the main grid's, as its launch computed them)
    const uint32_t grid = helper ? min(blocks, (uint32_t)(ncu * min(leave_per_cu, pc))) : blocks;
    const uint32_t main_sweep = helper ? blocks * (uint32_t)kBlock : 0u;
    LogRec *lrec = lg ? log->rec : nullptr;
    LogSpan *ltopics = lg ? log->topics : nullptr;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, B, T, sel, sel_count, answer_other ? 1u : 0u, zlist,
                       zcount, work, main_sweep, lrec, ltopics, lg ? log->stride : 0u);
    return hipGetLastError();
}

}  // namespace l7

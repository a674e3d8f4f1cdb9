// Stand-alone check of the Kafka window-path CRC's block schedule
// (cilium_amd/csrc/kernels/kafka_sched.h), the integer code the kernel runs:
// every message start mod 64, every message size 14 .. 400 (the size field:
// CRC, magic, attributes, [timestamp,] key and value), both message formats,
// and every window block the walk can have for the message (staged from the
// message's own chunk, or left in the slot by the message before it).
// Built and run by tests/test_kafka_block_schedule.py.  Exit status 0 and one
// line "ok <cases> <handed over>" when every case holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kafka_sched.h"

namespace ks = l7::ksched;

struct Range {
    uint32_t lo, hi;
};
struct Recorder {
    uint32_t in_slot;             // base of the block the slot holds
    uint32_t head_chunk;          // the cursor's chunk
    std::vector<uint32_t> staged;  // every block staged after the window block
    std::vector<Range> hashed;
    const char *err = nullptr;
    void fail(const char *m) { if (!err) err = m; }
    void head(uint32_t p, uint32_t h) {
        if (h == 0 || h > 15) fail("head length");
        if ((p & ~15u) != head_chunk || ((p + h - 1) & ~15u) != head_chunk) fail("head leaves the cursor's chunk");
        hashed.push_back({p, p + h});
    }
    void slot(uint32_t base, uint32_t lo, uint32_t hi) {
        if (base != in_slot) fail("slot: block not in the slot");
        if (lo > hi || hi > 64 || (lo & 7)) fail("slot: range");
        hashed.push_back({base + lo, base + hi});
    }
    void stage(uint32_t next) {
        if (next & 15) fail("staged block not 16-byte aligned");
        staged.push_back(next);
        in_slot = next;
    }
    void window(uint32_t wb, uint32_t lo, uint32_t next) {
        if (wb != in_slot) fail("window: block not in the slot");
        if (lo != 16 && lo != 32 && lo != 48) fail("window: offset");
        hashed.push_back({wb + lo, wb + 64});
        stage(next);
    }
    void block(uint32_t a, uint32_t next) {
        if (a != in_slot) fail("block: not the one staged");
        hashed.push_back({a, a + 64});
        if (next != ks::kNoSpan) stage(next);
    }
};

int main() {
    unsigned long cases = 0, handed = 0;
    for (int fmt = 0; fmt < 2; fmt++) {
        const uint32_t hmin = fmt ? 22u : 14u;
        for (uint32_t smod = 0; smod < 64; smod++) {
            for (uint32_t msize = hmin < 14 ? 14 : hmin; msize <= 400; msize++) {
                const uint32_t s = 1024 + smod, p = s + 16, e = s + 12 + msize;
                // the span before the walk reads the message: none, or any block that holds its window
                for (uint32_t sb : {ks::kNoSpan, s & ~15u, (s & ~15u) - 16, (s & ~15u) - 32, (s & ~15u) + 16}) {
                    const uint32_t wb = ks::window_base(sb, s);
                    const bool from_slot = sb != ks::kNoSpan && wb == sb && ks::in_span(sb, s, ks::kWindow);
                    if (!from_slot && wb != (s & ~15u)) { printf("window base: s %u sb %u\n", s, sb); return 1; }
                    if (wb > s || s + ks::kWindow > wb + 64 || (wb & 15)) { printf("window not in its block\n"); return 1; }
                    Recorder r;
                    r.in_slot = wb;
                    r.head_chunk = p & ~15u;
                    ks::crc_schedule(wb, p, e, r);
                    const uint32_t keep = ks::keep_base(wb, e);
                    const char *err = r.err;
                    uint32_t at = p;
                    for (const Range &g : r.hashed) {
                        if (g.lo != at || g.hi < g.lo) err = err ? err : "hashed ranges do not tile in order";
                        if (g.hi > e) err = err ? err : "hashed range past the message's end";
                        at = g.hi;
                    }
                    if (at != e) err = err ? err : "hashed ranges do not reach the message's end";
                    if (r.staged.empty()) {
                        if (keep != wb || e > wb + 64) err = err ? err : "nothing staged, slot not the window block";
                    } else {
                        // the last block staged holds the message's last byte, and the blocks are wb's successors
                        if (keep != r.staged.back() || !(keep < e && e <= keep + 64))
                            err = err ? err : "kept block is not the one the message ends in";
                        for (size_t k = 0; k < r.staged.size(); k++)
                            if (r.staged[k] != wb + 64 * (uint32_t)(k + 1)) err = err ? err : "staged blocks are not consecutive";
                    }
                    if (r.in_slot != keep) err = err ? err : "keep_base is not what the schedule left in the slot";
                    for (size_t k = 1; k < r.staged.size(); k++)
                        if (r.staged[k] <= r.staged[k - 1]) err = err ? err : "staged blocks not ascending";
                    // the message after it starts at e: its window block is the kept one whenever that holds it
                    const uint32_t nwb = ks::window_base(keep, e);
                    if (ks::in_span(keep, e, ks::kWindow) != (nwb == keep)) err = err ? err : "hand-over";
                    if (nwb != keep && nwb != (e & ~15u)) err = err ? err : "next window base";
                    if (err) {
                        printf("fmt %d s %u msize %u sb %u wb %u: %s\n", fmt, s, msize, sb, wb, err);
                        return 1;
                    }
                    cases++;
                    handed += nwb == keep;
                }
            }
        }
    }
    printf("ok %lu %lu\n", cases, handed);
    return 0;
}

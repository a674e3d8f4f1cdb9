// The scratch layouts of the session calls (cilium_amd/csrc/kernels/
// sess_scratch.h) on the host, with no HIP header in sight.  For every layout,
// over n x nconns x temp bytes: each region starts 256-byte aligned, the
// regions lie in the stated order and none reaches into the next, and every
// offset and the total equal the formulas the sizing functions and launchers
// each spelled by hand before the layouts were stated once -- written out
// below as they stood, not taken from the header.  stdout: one JSON object.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cilium_amd/csrc/kernels/sess_scratch.h"

static int g_bad = 0;
static long g_checked = 0;

static void fail(const char *what, uint32_t n, uint32_t nconns, size_t temp) {
    if (g_bad++ < 20) fprintf(stderr, "%s: n=%u nconns=%u temp=%zu\n", what, n, nconns, temp);
}

// the round-up as the launchers wrote it
static size_t A(size_t b) { return (b + 255) & ~(size_t)255; }

struct Region {
    size_t got, want, bytes;  // the layout's offset, the formula's, the bytes the region holds
};

// aligned, in order, disjoint, and as the formulas say
static void check(const char *what, const std::vector<Region> &r, size_t got_total, size_t want_total, uint32_t n,
                  uint32_t nconns, size_t temp) {
    g_checked++;
    bool ok = got_total == want_total && (got_total & 255) == 0;
    for (size_t k = 0; k < r.size(); k++) {
        const size_t next = k + 1 < r.size() ? r[k + 1].got : got_total;
        ok = ok && r[k].got == r[k].want && (r[k].got & 255) == 0;
        ok = ok && (k == 0 ? r[k].got == 0 : r[k].got > r[k - 1].got);  // in order (only the temp may be empty, last)
        ok = ok && r[k].got + r[k].bytes <= next;                       // no overlap
    }
    if (!ok) fail(what, n, nconns, temp);
}

int main() {
    const uint32_t ns[] = {1, 255, 256, 257, 1u << 20, 0x7FFFFFFFu};
    const uint32_t cs[] = {0, 1, 4096, 0xFFFFFFFFu};
    const size_t temps[] = {0, 1, 255, 256, 257, 767, (size_t)1 << 20, ((size_t)1 << 33) + 5};
    for (uint32_t n : ns)
        for (uint32_t nconns : cs)
            for (size_t temp : temps) {
                const size_t N = n, C = nconns;
                {  // l7g_kafka_forward
                    const size_t kb = A(N * 8 + 256), sb = A((C + 1) * 8);
                    const l7::KafkaForwardScratch L = l7::KafkaForwardLayout(n, nconns, temp);
                    check("kafka forward",
                          {{L.keys, 0, N * 8 + 256},
                           {L.sorted, kb, N * 8 + 256},
                           {L.seg, 2 * kb, (C + 1) * 8},
                           {L.temp, 2 * kb + sb, temp}},
                          L.total, 2 * A(N * 8 + 256) + A((C + 1) * 8) + A(temp), n, nconns, temp);
                }
                {  // l7g_mc_forward
                    const size_t kb = A(N * 8 + 256), ib = A(N + 256), eb = A(N * 16 + 256), sb = A((C + 1) * 16);
                    const size_t fixed = 2 * kb + ib + 2 * eb + sb;
                    const l7::McForwardScratch L = l7::McForwardLayout(n, nconns, temp);
                    check("mc forward",
                          {{L.keys, 0, N * 8 + 256},
                           {L.sorted, kb, N * 8 + 256},
                           {L.info, 2 * kb, N + 256},
                           {L.el, 2 * kb + ib, N * 16 + 256},
                           {L.sc, 2 * kb + ib + eb, N * 16 + 256},
                           {L.seg, 2 * kb + ib + 2 * eb, (C + 1) * 16},
                           {L.temp, fixed, temp}},
                          L.total,
                          2 * A(N * 8 + 256) + A(N + 256) + 2 * A(N * 16 + 256) + A((C + 1) * 16) + A(temp), n, nconns,
                          temp);
                }
                {  // l7g_kafka_responses
                    const l7::KafkaResponsesScratch L = l7::KafkaResponsesLayout(n);
                    check("kafka responses", {{L.where, 0, N * 4 + 256}}, L.total, A(N * 4 + 256), n, nconns, temp);
                }
                const size_t kb = (N * sizeof(uint64_t) + 256 + 255) & ~(size_t)255;  // KeyBytes(n)
                {  // the cassandra classifier and l7g_cass_replies
                    const l7::CassandraScratch L = l7::CassandraLayout(n, false, temp);
                    check("cassandra", {{L.keys, 0, N * 8 + 256}, {L.sorted, kb, N * 8 + 256}, {L.temp, 2 * kb, temp}},
                          L.total, 2 * kb + ((temp + 255) & ~(size_t)255), n, nconns, temp);
                    if (L.pkeys != L.temp || L.psorted != L.temp) fail("cassandra: no PREPARE regions", n, nconns, temp);
                }
                {  // the same with sessions
                    const l7::CassandraScratch L = l7::CassandraLayout(n, true, temp);
                    check("cassandra sessions",
                          {{L.keys, 0, N * 8 + 256},
                           {L.sorted, kb, N * 8 + 256},
                           {L.pkeys, 2 * kb, N * 8 + 256},
                           {L.psorted, 3 * kb, N * 8 + 256},
                           {L.temp, 4 * kb, temp}},
                          L.total, 4 * kb + ((temp + 255) & ~(size_t)255), n, nconns, temp);
                    // (CassandraSortedUseKeys: one offset with sessions and without)
                    if (L.sorted != l7::CassandraLayout(n, false, temp).sorted) fail("cassandra: sorted moved", n, nconns, temp);
                }
            }
    // the carving helper itself: offsets advance by the rounded size
    l7::Carve c;
    if (c.take(1) != 0 || c.take(256) != 256 || c.take(0) != 512 || c.take(257) != 512 || c.at != 1024) fail("Carve", 0, 0, 0);
    printf("{\"checked\": %ld, \"bad\": %d}\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}

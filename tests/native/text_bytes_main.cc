// The White_Space rune rule of cilium_amd/csrc/kernels/text_bytes.h on the
// host, over every input it can be given: all 2^24 values of (c0, c1, c2) with
// avail in {1, 2, 3}.  Printed: every byte sequence accepted with avail = 3 and
// its width, and the count of points that break one of
//   - the width is at most avail;
//   - the result depends only on the first `width` bytes: a sequence is
//     accepted with width 1 (2) iff it is with the bytes after the first
//     (second) zeroed, and with avail >= its width it is accepted as with 3;
//   - avail below the width gives 0.
// Then proxylib/shim.cc's SpaceLen (from libl7gpu.so) against the rule on each
// accepted sequence and on each near miss read from stdin (hex, one a line):
// alone, cut short at every length, followed by another byte and after one, in
// buffers of exactly their size.  stdout: one JSON object.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../cilium_amd/csrc/kernels/text_bytes.h"

namespace l7 {
size_t SpaceLen(const uint8_t *s, size_t i, size_t n);  // proxylib/shim.cc, from libl7gpu.so
}
using l7::ws_rune_len;

// SpaceLen at s[i] of an n-byte buffer of its own against the rule on the same bytes
static long spacelen_disagrees(const std::string &s, size_t i) {
    const size_t n = s.size();
    uint8_t *b = (uint8_t *)malloc(n);
    memcpy(b, s.data(), n);
    const uint32_t avail = n - i >= 3 ? 3u : (uint32_t)(n - i);
    const uint32_t want = ws_rune_len(b[i], avail >= 2 ? b[i + 1] : 0u, avail >= 3 ? b[i + 2] : 0u, avail);
    const size_t got = l7::SpaceLen(b, i, n);
    free(b);
    if (got != want) fprintf(stderr, "SpaceLen %zu != rule %u at %zu of %zu bytes\n", got, want, i, n);
    return got != want;
}

int main() {
    long points = 0, bad = 0;
    std::vector<std::string> accepted;
    std::string json;
    for (uint32_t c0 = 0; c0 < 256; c0++)
        for (uint32_t c1 = 0; c1 < 256; c1++)
            for (uint32_t c2 = 0; c2 < 256; c2++) {
                const uint32_t w3 = ws_rune_len(c0, c1, c2, 3);
                const bool one = ws_rune_len(c0, 0, 0, 3) == 1, two = ws_rune_len(c0, c1, 0, 3) == 2;
                for (uint32_t avail = 1; avail <= 3; avail++) {
                    const uint32_t w = ws_rune_len(c0, c1, c2, avail);
                    points++;
                    bool ok = w <= avail;                       // no wider than what exists
                    ok = ok && (w == 1) == one && (w3 == 2) == two;  // the first `width` bytes decide
                    ok = ok && w == (avail >= w3 ? w3 : 0u);    // cut short: none; else as with all three
                    if (!ok && bad++ < 20) fprintf(stderr, "%02x %02x %02x avail %u: %u (with 3: %u)\n", c0, c1, c2, avail, w, w3);
                }
                // each accepted sequence once: its first w3 bytes, the rest zero
                if (w3 && (w3 >= 2 || c1 == 0) && (w3 >= 3 || c2 == 0)) {
                    const char b[3] = {(char)c0, (char)c1, (char)c2};
                    accepted.emplace_back(b, w3);
                    char hex[16];
                    snprintf(hex, sizeof hex, "%02x%02x%02x", c0, c1, c2);
                    json += std::string(json.empty() ? "" : ", ") + "[\"" + std::string(hex, 2 * w3) + "\", " + std::to_string(w3) + "]";
                }
            }
    std::vector<std::string> seqs = accepted;
    char line[256];
    long near = 0;
    while (fgets(line, sizeof line, stdin)) {
        std::string s;
        for (size_t k = 0; line[k] && line[k + 1] && line[k] != '\n'; k += 2) s.push_back((char)strtol(std::string(line + k, 2).c_str(), nullptr, 16));
        if (!s.empty()) { seqs.push_back(s); near++; }
    }
    long disagree = 0, calls = 0;
    for (const std::string &s : seqs) {
        for (size_t n = 1; n <= s.size(); n++) {  // alone, and cut short at every length
            disagree += spacelen_disagrees(s.substr(0, n), 0);
            calls++;
        }
        for (size_t k = 1; k < s.size(); k++) {  // from its later bytes on
            disagree += spacelen_disagrees(s, k);
            calls++;
        }
        disagree += spacelen_disagrees(s + "x", 0) + spacelen_disagrees("x" + s, 1) + spacelen_disagrees("\xe2" + s + "\x80\x80", 1);
        calls += 3;
    }
    printf("{\"points\": %ld, \"violations\": %ld, \"accepted\": [%s], \"near\": %ld, \"spacelen_calls\": %ld, "
           "\"spacelen_disagree\": %ld}\n", points, bad, json.c_str(), near, calls, disagree);
    return 0;
}

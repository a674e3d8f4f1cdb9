// The cassandra query parser of cilium_amd/csrc/kernels/cass_parse.h on the
// host, as the kernels use it: cass_parse_query on the raw query bytes, then
// parts[3] of the path through cass_seg3 into a string sink, under the keyspace
// that a USE query (parsed the same way) left.  The header is included
// directly; nothing of libl7gpu.so is called.
//
// stdin: one case a line, "<use query, hex> <query, hex>" ("-" = none / the
// empty query).  Each query sits in a heap buffer of exactly its size, so a
// read past its end is a read past an allocation.
// stdout: one line a case, "<status> <action id> <parts[2], hex> <parts[3], hex>"
// ("-" = empty): status CQ_OK / CQ_INVALID / CQ_PANIC; parts[2] is the action
// string up to its first '/', built from the keyword and fields[1] the way the
// access log builds it; for a status other than CQ_OK both strings are empty.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../cilium_amd/csrc/kernels/cass_parse.h"
#include "../../cilium_amd/csrc/regex/unicode_tables.h"

struct StrSink {
    std::string s;
    void raw(uint32_t c) { s.push_back((char)c); }
    void rune(uint32_t r) {
        uint8_t e[4];
        s.append((const char *)e, l7::cass_encode(r, e));
    }
};

struct Buf {  // exactly n bytes on the heap
    uint8_t *p;
    uint32_t n;
    explicit Buf(const std::string &hex) {
        n = hex == "-" ? 0 : (uint32_t)(hex.size() / 2);
        p = (uint8_t *)malloc(n);
        for (uint32_t k = 0; k < n; k++) p[k] = (uint8_t)strtol(hex.substr(2 * k, 2).c_str(), nullptr, 16);
    }
    ~Buf() { free(p); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
};

static std::string hex_of(const std::string &s) {
    if (s.empty()) return "-";
    static const char *d = "0123456789abcdef";
    std::string h;
    for (unsigned char c : s) { h.push_back(d[c >> 4]); h.push_back(d[c & 15]); }
    return h;
}

int main() {
    std::vector<uint32_t> L;
    for (int i = 0; i < UNI_LOWER_NPAIRS; i++) { L.push_back(UNI_LOWER_PAIRS[i][0]); L.push_back(UNI_LOWER_PAIRS[i][1]); }
    const uint32_t nl = (uint32_t)(L.size() / 2);
    std::string line;
    int c;
    std::string out;
    while (true) {
        line.clear();
        while ((c = getchar()) != EOF && c != '\n') line.push_back((char)c);
        if (line.empty() && c == EOF) break;
        const size_t sp = line.find(' ');
        if (sp == std::string::npos) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        const Buf use(line.substr(0, sp)), q(line.substr(sp + 1));
        const uint8_t *ks = nullptr;
        l7::CassQuery K{};
        if (use.n) {
            K = l7::cass_parse_query(use.p, use.n, L.data(), nl);
            if (K.status == l7::CQ_OK && K.is_use) ks = use.p;
        }
        const l7::CassQuery Q = l7::cass_parse_query(q.p, q.n, L.data(), nl);
        StrSink a, t;
        if (Q.status == l7::CQ_OK) {
            static const char *const one[] = {"select", "delete", "insert", "update", "use"};
            static const char *const two[] = {"alter", "create", "drop", "truncate", "list"};
            if (Q.kw >= l7::CW_SELECT && Q.kw <= l7::CW_USE) {
                a.s = one[Q.kw - l7::CW_SELECT];
            } else {
                a.s = std::string(two[Q.kw - l7::CW_ALTER]) + "-";
                const bool slash = l7::cass_emit(q.p, Q.f1s, Q.f1e, Q.fc, L.data(), nl, a);
                const uint32_t w1 = slash ? (uint32_t)l7::CW_NONE : l7::cass_word(q.p, Q.f1s, Q.f1e);
                if (w1 == l7::CW_MATERIALIZED) a.s += "-view";
                else if (w1 == l7::CW_CUSTOM) a.s = "create-index";
            }
            l7::cass_seg3(Q, q.p, ks, K.ts, K.te, K.fc, L.data(), nl, t);
        }
        out += std::to_string((int)Q.status) + " " + std::to_string(Q.action) + " " + hex_of(a.s) + " " + hex_of(t.s) + "\n";
        if (c == EOF) break;
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

// C-ABI implementation (include/l7gpu.h): engine lifetime, policy versions,
// compiled tables across ranks, the connection table and its upload, and the
// statistics, profile and debug exports (product code).  The launch plan is
// classify.cc, the session tables cass_sessions.cc, kafka_sessions.cc and
// mc_sessions.cc, the host-buffer calls host_call.cc, the resident services service.cc;
// engine_state.h holds what they share.
#include <algorithm>
#include <cstring>

#include "engine/nfa_pool.h"
#include "engine_state.h"
#include "kernels/cass_parse.h"
#include "policy/npds_proto.h"
#include "regex/nfa_walk.h"
#include "regex/re_dfa.h"

namespace {

template <class T>
size_t Put(std::vector<uint8_t> &blob, const std::vector<T> &v) {
    size_t off = (blob.size() + 255) & ~(size_t)255;
    blob.resize(off + v.size() * sizeof(T) + 16);  // +16: aligned 16-byte reads may run past the end
    if (!v.empty()) memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

// Resolve connection i to its rule set (once per connection / policy version).
bool ResolveOne(l7g_engine *e, size_t i, std::string *err) {
    const l7g_conn_t &a = e->attrs[i];
    DevConn &c = e->conns[i];
    c = DevConn{-1, PROTO_NONE, 0, 0xFFFF};
    c.proto = a.proto;
    if (L7_PROTO_OWNED(a.proto)) {
        const auto key = std::make_tuple(a.policy, a.proto, a.port, (uint8_t)(a.ingress != 0));
        auto it = e->skeys.find(key);
        if (it == e->skeys.end() && e->skey_list.size() < FlowStatsMaxKeys()) {
            it = e->skeys.emplace(key, (uint16_t)e->skey_list.size()).first;
            e->skey_list.push_back(key);
        }
        if (it != e->skeys.end()) c.skey = it->second;
    }
    c.flags = (uint8_t)(a.flags & 3);
    const bool proxylib = (a.flags & L7G_CONN_PROXYLIB) != 0;
    if (a.proto == PROTO_HTTP) {
        // remote identity: Envoy's HTTP filter uses the source on ingress and the
        // destination on egress (cilium_l7policy.cc:144-150); proxylib matches
        // the connection's SrcId in both directions (connection.go:176-179)
        uint64_t remote = (a.ingress || proxylib) ? a.src_id : a.dst_id;
        c.ruleset = e->hc->RulesetFor(a.policy, a.ingress != 0, a.port, remote, proxylib, err);
        if (c.ruleset < 0) return false;
        e->has_http = true;
    } else if (a.proto == PROTO_KAFKA) {
        // Kafka rules are selected by the source identity in both directions
        // (pkg/proxy/kafka.go:327,357)
        c.ruleset = e->kc->RulesetFor(a.policy, a.ingress != 0, a.port, a.src_id, proxylib, err);
        if (c.ruleset < 0) return false;
        e->has_kafka = true;
    } else if (a.proto == PROTO_MEMCACHE) {
        // proxylib matches on the connection's SrcId in both directions
        // (proxylib/proxylib/connection.go:176-179)
        c.ruleset = e->mc->RulesetFor(a.policy, a.ingress != 0, a.port, a.src_id, err);
        if (c.ruleset < 0) return false;
        e->has_mc = true;
    } else if (a.proto == PROTO_R2D2) {  // proxylib r2d2: SrcId in both directions, as memcached
        c.ruleset = e->r2->RulesetFor(a.policy, a.ingress != 0, a.port, a.src_id, err);
        if (c.ruleset < 0) return false;
        e->has_r2 = true;
    } else if (a.proto == PROTO_CASSANDRA) {  // proxylib cassandra: SrcId in both directions
        c.ruleset = e->cs->RulesetFor(a.policy, a.ingress != 0, a.port, a.src_id, err);
        if (c.ruleset < 0) return false;
        e->has_cs = true;
    }
    return true;
}

// The HTTP rule set serving the most connections has its image staged in LDS
// by every workgroup (if it fits); the others are read from HBM/L2.
void PickHot(l7g_engine *e) {
    std::vector<uint32_t> uses(e->hc->image().rulesets.size(), 0);
    for (size_t i = 0; i < e->attrs.size(); i++)
        if (e->attrs[i].proto == PROTO_HTTP && e->conns[i].ruleset >= 0) uses[e->conns[i].ruleset]++;
    e->hot_ruleset = -1;
    uint32_t best = 0;
    for (size_t r = 0; r < uses.size(); r++)
        if (uses[r] > best && e->hc->image().rulesets[r].image_len <= kLdsImageBytes) { best = uses[r]; e->hot_ruleset = (int32_t)r; }
    e->any_cold = false;
    for (size_t i = 0; i < e->attrs.size(); i++)
        if (e->attrs[i].proto == PROTO_HTTP && e->conns[i].ruleset != e->hot_ruleset) e->any_cold = true;
    e->any_big_image = false;
    for (size_t r = 0; r < uses.size(); r++)
        if (uses[r] && e->hc->image().rulesets[r].image_len > kGroupImageBytes) e->any_big_image = true;
}

size_t TableRulesets(const l7g_engine *e) {
    return e->hc->image().rulesets.size() + e->kc->image().rulesets.size() + e->mc->image().rulesets.size() +
           e->r2->image().rulesets.size() + e->cs->image().rulesets.size();
}

// Resolve every connection (policy update / connection table replaced).
bool ResolveConns(l7g_engine *e, std::string *err) {
    e->conns.assign(e->attrs.size(), DevConn{-1, PROTO_NONE, 0, 0xFFFF});
    e->has_http = e->has_kafka = e->has_mc = e->has_r2 = e->has_cs = false;
    for (size_t i = 0; i < e->attrs.size(); i++)
        if (!ResolveOne(e, i, err)) return false;
    PickHot(e);
    e->tables_dirty = e->conns_dirty = true;
    return true;
}

// The device table blob: every compiler's image, each 256-byte aligned.
struct BlobLayout {
    size_t o_rs, o_img, o_nfa, k_rs, k_r, k_idx, k_th, k_ch, k_s, m_rs, m_img, m_nfa, r_rs, r_img, r_nfa, c_rs, c_img,
        c_nfa, c_low;
};
BlobLayout AssembleBlob(const l7g_engine *e, std::vector<uint8_t> &blob) {
    BlobLayout L;
    const HttpImage &H = e->hc->image();
    L.o_rs = Put(blob, H.rulesets); L.o_img = Put(blob, H.images); L.o_nfa = Put(blob, H.nfa_pool);
    const KafkaImage &K = e->kc->image();
    L.k_rs = Put(blob, K.rulesets); L.k_r = Put(blob, K.rules); L.k_idx = Put(blob, K.index);
    L.k_th = Put(blob, K.topic_hash); L.k_ch = Put(blob, K.client_hash); L.k_s = Put(blob, K.strings);
    const McImage &M = e->mc->image();
    L.m_rs = Put(blob, M.rulesets); L.m_img = Put(blob, M.images); L.m_nfa = Put(blob, M.nfa_pool);
    const R2Image &R = e->r2->image();
    L.r_rs = Put(blob, R.rulesets); L.r_img = Put(blob, R.images); L.r_nfa = Put(blob, R.nfa_pool);
    const CassImage &CI = e->cs->image();
    L.c_rs = Put(blob, CI.rulesets); L.c_img = Put(blob, CI.images); L.c_nfa = Put(blob, CI.nfa_pool);
    L.c_low = Put(blob, CI.lower);
    return L;
}

// Swap in a policy version with its compilers (fresh, or holding imported
// tables); on a compile failure the previous version stays in force.
int SwapIn(l7g_engine *e, std::unique_ptr<PolicySet> ps, std::unique_ptr<HttpCompiler> hc,
           std::unique_ptr<KafkaCompiler> kc, std::unique_ptr<McCompiler> mc, std::unique_ptr<R2Compiler> r2,
           std::unique_ptr<CassCompiler> cs, char *err, size_t errlen) {
    std::string m;
    auto swap = [&] {
        std::swap(e->ps, ps);
        std::swap(e->hc, hc);
        std::swap(e->kc, kc);
        std::swap(e->mc, mc);
        std::swap(e->r2, r2);
        std::swap(e->cs, cs);
    };
    swap();
    if (!ResolveConns(e, &m)) {  // roll back: previous version stays in force
        swap();
        std::string m2;
        ResolveConns(e, &m2);
        set_err(err, errlen, m);
        return -1;
    }
    return 0;
}

// Swap in a loaded policy version; on a compile failure the previous version
// stays in force (an NPDS NACK).  Caller holds e->mu.
int PolicySwap(l7g_engine *e, std::unique_ptr<PolicySet> ps, char *err, size_t errlen) {
    auto hc = std::make_unique<HttpCompiler>(ps.get());
    auto kc = std::make_unique<KafkaCompiler>(ps.get(), e->kafka_dense_budget);
    auto mc = std::make_unique<McCompiler>(ps.get());
    auto r2 = std::make_unique<R2Compiler>(ps.get());
    auto cs = std::make_unique<CassCompiler>(ps.get());
    return SwapIn(e, std::move(ps), std::move(hc), std::move(kc), std::move(mc), std::move(r2), std::move(cs), err,
                  errlen);
}

}  // namespace

// The tables and the connection table on the device, as of the current policy
// version and connections (caller holds e->mu).
hipError_t Upload(l7g_engine *e) {
    hipError_t rc;
    if (e->tables_dirty) {
        std::vector<uint8_t> blob;
        const BlobLayout L = AssembleBlob(e, blob);
        const HttpImage &H = e->hc->image();
        const KafkaImage &K = e->kc->image();
        const McImage &M = e->mc->image();
        const R2Image &R = e->r2->image();
        const CassImage &CI = e->cs->image();
        uint8_t *d = nullptr;
        if ((rc = hipMalloc(&d, blob.size())) != hipSuccess) return rc;
        if ((rc = hipMemcpy(d, blob.data(), blob.size(), hipMemcpyHostToDevice)) != hipSuccess) { hipFree(d); return rc; }
        if (e->d_blob) { WaitLastClassify(e); hipFree(e->d_blob); }
        e->d_blob = d;
        e->blob_bytes = blob.size();
        HttpTables &T = e->ht;
        T.rulesets = (const DevRuleset *)(d + L.o_rs);
        T.images = d + L.o_img;
        T.nrulesets = (uint32_t)H.rulesets.size();
        T.hot_ruleset = e->hot_ruleset;
        T.nfa_pool = H.nfa_pool.empty() ? nullptr : d + L.o_nfa;
        T.nfa_bits = nullptr;
        // large NFAs (W > kNfaMaxWords): 2 W words of scratch per lane, given at launch
        auto lane_words = [](uint32_t w) { return w > (uint32_t)kNfaMaxWords ? 2 * w : 0u; };
        T.nfa_scratch = nullptr;
        T.nfa_lane_words = lane_words(e->hc->nfa_max_words());
        KafkaTables &KT = e->kt;
        KT.rulesets = (const DevKafkaRuleset *)(d + L.k_rs);
        KT.rules = (const DevKafkaRule *)(d + L.k_r);
        KT.index = (const uint32_t *)(d + L.k_idx);
        KT.topic_hash = (const DevStrSlot *)(d + L.k_th);
        KT.client_hash = (const DevStrSlot *)(d + L.k_ch);
        KT.strings = (const uint8_t *)(d + L.k_s);
        KT.nrulesets = (uint32_t)K.rulesets.size();
        KT.topic_mask = K.topic_mask;
        KT.client_mask = K.client_mask;
        McTables &MT = e->mt;
        MT.rulesets = (const DevRuleset *)(d + L.m_rs);
        MT.images = d + L.m_img;
        MT.nrulesets = (uint32_t)M.rulesets.size();
        MT.images_len = (uint32_t)M.images.size();
        MT.nfa_pool = M.nfa_pool.empty() ? nullptr : d + L.m_nfa;
        MT.max_chunks = (uint32_t)M.max_chunks;
        MT.nfa_scratch = nullptr;
        MT.nfa_lane_words = lane_words(e->mc->nfa_max_words());
        R2Tables &RT = e->rt;
        RT.rulesets = (const DevRuleset *)(d + L.r_rs);
        RT.images = d + L.r_img;
        RT.nrulesets = (uint32_t)R.rulesets.size();
        RT.nfa_pool = R.nfa_pool.empty() ? nullptr : d + L.r_nfa;
        RT.nfa_scratch = nullptr;
        RT.nfa_lane_words = lane_words(e->r2->nfa_max_words());
        CassTables &CT = e->ct;
        CT.rulesets = (const DevRuleset *)(d + L.c_rs);
        CT.images = d + L.c_img;
        CT.nrulesets = (uint32_t)CI.rulesets.size();
        CT.nfa_pool = CI.nfa_pool.empty() ? nullptr : d + L.c_nfa;
        CT.lower = (const uint32_t *)(d + L.c_low);
        CT.nlower = (uint32_t)(CI.lower.size() / 2);
        CT.nfa_scratch = nullptr;
        CT.nfa_lane_words = lane_words(e->cs->nfa_max_words());
        e->tables_dirty = false;
    }
    if (e->conns_dirty) {
        // kernels of the previous batch may still read the table: it is
        // rewritten (or freed) only once they have finished
        if ((rc = WaitLastClassify(e)) != hipSuccess) return rc;
        size_t need = std::max<size_t>(e->conns.size(), 1);
        if (need > e->conns_cap) {
            if (e->d_conns) { hipFree(e->d_conns); e->d_conns = nullptr; }
            if ((rc = hipMalloc(&e->d_conns, need * sizeof(DevConn))) != hipSuccess) return rc;
            e->conns_cap = need;
        }
        if (!e->conns.empty() &&
            (rc = hipMemcpy(e->d_conns, e->conns.data(), e->conns.size() * sizeof(DevConn), hipMemcpyHostToDevice)) != hipSuccess)
            return rc;
        e->conns_dirty = false;
    }
    return hipSuccess;
}

// capi_internal.h: proto_form 0 = JSON, 1 = NPDS DiscoveryResponse; proxylib
// != 0 = the proxylib instance's update (instance.go:168-219), which also
// NACKs what only proxylib's policymap rejects (PolicySet::px_nack).
int l7g_policy_update_view(l7g_engine *e, const uint8_t *buf, size_t len, int proto_form, int proxylib, char *err,
                           size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    auto ps = std::make_unique<PolicySet>();
    std::string m;
    const bool ok = proto_form ? LoadPolicySetProto(buf, len, ps.get(), &m)
                               : LoadPolicySet((const char *)buf, len, ps.get(), &m);
    if (!ok) { set_err(err, errlen, m); return -1; }
    if (proxylib && !ps->px_nack.empty()) { set_err(err, errlen, ps->px_nack); return -1; }
    const int rc = PolicySwap(e, std::move(ps), err, errlen);
    if (rc == 0) {
        e->policy_src.assign((const char *)buf, len);
        e->policy_form = proto_form;
        e->policy_px = proxylib;
    }
    return rc;
}

extern "C" {

l7g_engine *l7g_engine_create(int device, char *err, size_t errlen) {
    const bool host_only = device == L7G_HOST_ONLY;  // rule compiler only: no HIP calls, classify unavailable
    if (!host_only) {
        int ndev = 0;
        hipError_t rc = hipGetDeviceCount(&ndev);
        if (rc != hipSuccess || device < 0 || device >= ndev) {
            set_err(err, errlen, std::string("no such HIP device: ") + std::to_string(device) + " (" + hipGetErrorString(rc) + ")");
            return nullptr;
        }
        if ((rc = hipSetDevice(device)) != hipSuccess) { set_err(err, errlen, hipGetErrorString(rc)); return nullptr; }
    }
    auto *e = new l7g_engine();
    e->device = host_only ? -1 : device;
    const char *v = host_only ? nullptr : getenv("L7G_SERVICE");
    e->svc_on = !(v && v[0] == '0');
    e->ps = std::make_unique<PolicySet>();
    e->hc = std::make_unique<HttpCompiler>(e->ps.get());
    // L7G_KAFKA_DENSE_BUDGET=<words>: the Kafka compiler's dense-table budget (tests of the
    // sorted-directory form of a rule set; unset, kDenseTopicBudget)
    if (const char *b = getenv("L7G_KAFKA_DENSE_BUDGET"); b && b[0] >= '0' && b[0] <= '9')
        e->kafka_dense_budget = (size_t)strtoull(b, nullptr, 10);
    e->kc = std::make_unique<KafkaCompiler>(e->ps.get(), e->kafka_dense_budget);
    e->mc = std::make_unique<McCompiler>(e->ps.get());
    e->r2 = std::make_unique<R2Compiler>(e->ps.get());
    e->cs = std::make_unique<CassCompiler>(e->ps.get());
    return e;
}

void l7g_engine_destroy(l7g_engine *e) {
    if (!e) return;
    if (e->device < 0) { delete e; return; }
    hipSetDevice(e->device);
    StopServices(e);
    hipDeviceSynchronize();
    if (e->d_blob) hipFree(e->d_blob);
    if (e->d_conns) hipFree(e->d_conns);
    e->hctx.clear();
    e->scr.clear();
    if (e->d_flow) hipFree(e->d_flow);
    SessionsFree(e);
    KafkaSessionsFree(e);
    McSessionsFree(e);
    if (e->d_zreg) hipFree(e->d_zreg);
    if (e->zreg_ev) hipEventDestroy(e->zreg_ev);
    for (hipEvent_t ev : e->prof_ev)
        if (ev) hipEventDestroy(ev);
    delete e;
}

int l7g_policy_update(l7g_engine *e, const char *json, size_t len, char *err, size_t errlen) {
    return l7g_policy_update_view(e, (const uint8_t *)json, len, 0, 0, err, errlen);
}

int l7g_policy_update_proto(l7g_engine *e, const uint8_t *buf, size_t len, char *err, size_t errlen) {
    return l7g_policy_update_view(e, buf, len, 1, 0, err, errlen);
}

// ---- compiled tables across ranks (engine/serial.h)
constexpr uint64_t kTablesMagic = 0x3154473754L;  // "T7G1"
// format and struct-layout tag: an image from a build with another layout of
// the device records is refused (it would be read at the wrong offsets)
// (3: HTTP images carry the null DFA behind their header, kImgNullDfaOff)
constexpr uint64_t kTablesAbi = 3ull << 56 | (uint64_t)sizeof(DevRuleset) << 48 | (uint64_t)sizeof(DevNfa) << 36 |
                                (uint64_t)sizeof(ImgHeader) << 24 | (uint64_t)sizeof(DevKafkaRuleset) << 12 |
                                (uint64_t)sizeof(McImgHeader);

int l7g_tables_export(l7g_engine *e, uint8_t *buf, size_t cap, size_t *len) {
    std::lock_guard<std::mutex> g(e->mu);
    Ser s;
    s.u64(kTablesMagic);
    s.u64(kTablesAbi);
    s.u64((uint64_t)e->policy_form);
    s.u64((uint64_t)e->policy_px);
    s.str(e->policy_src);
    e->hc->Save(s);
    e->kc->Save(s);
    e->mc->Save(s);
    e->r2->Save(s);
    e->cs->Save(s);
    if (len) *len = s.out.size();
    if (!buf || cap < s.out.size()) return -2;
    memcpy(buf, s.out.data(), s.out.size());
    return 0;
}

int l7g_tables_import(l7g_engine *e, const uint8_t *buf, size_t len, char *err, size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    Des d(buf, len);
    if (d.u64() != kTablesMagic) { set_err(err, errlen, "not an l7g_tables_export image"); return -1; }
    if (d.u64() != kTablesAbi) { set_err(err, errlen, "tables image from a build with another table layout"); return -1; }
    const int form = (int)d.u64(), px = (int)d.u64();
    const std::string src = d.str();
    if (!d.ok) { set_err(err, errlen, "truncated tables image"); return -1; }
    auto ps = std::make_unique<PolicySet>();
    std::string m;
    const bool ok = form ? LoadPolicySetProto((const uint8_t *)src.data(), src.size(), ps.get(), &m)
                         : LoadPolicySet(src.data(), src.size(), ps.get(), &m);
    if (!ok) { set_err(err, errlen, m); return -1; }
    auto hc = std::make_unique<HttpCompiler>(ps.get());
    auto kc = std::make_unique<KafkaCompiler>(ps.get(), e->kafka_dense_budget);
    auto mc = std::make_unique<McCompiler>(ps.get());
    auto r2 = std::make_unique<R2Compiler>(ps.get());
    auto cs = std::make_unique<CassCompiler>(ps.get());
    if (!hc->Load(d) || !kc->Load(d) || !mc->Load(d) || !r2->Load(d) || !cs->Load(d) || d.p != d.end) {
        set_err(err, errlen, "corrupt or inconsistent tables image");
        return -1;
    }
    const int rc = SwapIn(e, std::move(ps), std::move(hc), std::move(kc), std::move(mc), std::move(r2), std::move(cs),
                          err, errlen);
    if (rc == 0) {
        e->policy_src = src;
        e->policy_form = form;
        e->policy_px = px;
    }
    return rc;
}

uint64_t l7g_tables_compiled(l7g_engine *e) {
    std::lock_guard<std::mutex> g(e->mu);
    return e->hc->compiled + e->kc->compiled + e->mc->compiled + e->r2->compiled + e->cs->compiled;
}

uint64_t l7g_tables_digest(l7g_engine *e) {
    std::lock_guard<std::mutex> g(e->mu);
    std::vector<uint8_t> blob;
    AssembleBlob(e, blob);
    uint64_t h = 1469598103934665603ull;  // FNV-1a 64
    for (uint8_t b : blob) h = (h ^ b) * 1099511628211ull;
    return h;
}

int32_t l7g_policy_index(l7g_engine *e, const char *name, size_t len) {
    std::lock_guard<std::mutex> g(e->mu);
    auto it = e->ps->by_name.find(std::string(name, len));
    return it == e->ps->by_name.end() ? -1 : it->second;
}

int32_t l7g_policy_nrules(l7g_engine *e) {
    std::lock_guard<std::mutex> g(e->mu);
    return e->ps->nrules;
}

int l7g_conns_set(l7g_engine *e, const l7g_conn_t *conns, uint32_t n, char *err, size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    e->attrs.assign(conns, conns + n);
    std::string m;
    if (!ResolveConns(e, &m)) { set_err(err, errlen, m); return -1; }
    e->sess_reset.All(e->sess.by_id != nullptr);  // every connection is new
    e->ksess_reset.All(e->ksess.tab != nullptr);
    e->mcsess_reset.All(e->mcsess.stats != nullptr);
    return 0;
}

int l7g_conn_update(l7g_engine *e, uint32_t index, const l7g_conn_t *conn, char *err, size_t errlen) {
    std::lock_guard<std::mutex> g(e->mu);
    if (index >= e->attrs.size()) {
        l7g_conn_t none{};
        none.policy = -1;
        e->attrs.resize((size_t)index + 1, none);
        e->conns.resize((size_t)index + 1, DevConn{-1, PROTO_NONE, 0, 0xFFFF});
    }
    const l7g_conn_t prev = e->attrs[index];
    const size_t nrs = TableRulesets(e);
    e->attrs[index] = *conn;
    std::string m;
    if (!ResolveOne(e, index, &m)) {
        e->attrs[index] = prev;
        ResolveOne(e, index, &m);
        set_err(err, errlen, m);
        return -1;
    }
    if (TableRulesets(e) != nrs) e->tables_dirty = true;
    if (conn->proto == PROTO_HTTP || prev.proto == PROTO_HTTP) {
        const int32_t hot = e->hot_ruleset;
        PickHot(e);
        if (hot != e->hot_ruleset) e->tables_dirty = true;
    }
    e->conns_dirty = true;
    // the new-connection event: proxylib makes a new parser there
    e->sess_reset.Add(e->sess.by_id != nullptr, &index, 1);
    e->ksess_reset.Add(e->ksess.tab != nullptr, &index, 1);
    e->mcsess_reset.Add(e->mcsess.stats != nullptr, &index, 1);
    return 0;
}

// the access-log record's layout as the kernels write it (LogRec / LogSpan, device_tables.h)
static_assert(sizeof(l7g_logrec_t) == 32 && sizeof(LogRec) == 32 && sizeof(l7g_span_t) == 8 && sizeof(LogSpan) == 8,
              "record and span sizes");
static_assert(offsetof(l7g_logrec_t, api_key) == 2 && offsetof(l7g_logrec_t, u.http.method_len) == 4 &&
                  offsetof(l7g_logrec_t, u.http.nheaders) == 24 && offsetof(l7g_logrec_t, u.kafka.api_version) == 4 &&
                  offsetof(l7g_logrec_t, u.kafka.correlation_id) == 8 && offsetof(l7g_logrec_t, u.kafka.ntopics) == 12,
              "record fields");
static_assert(L7G_LOG_HTTP == LOG_HTTP && L7G_LOG_KAFKA == LOG_KAFKA, "record kinds");

const char *l7g_kafka_api_key_name(int16_t key) { return KafkaApiKeyName(key); }

// the members l7g_classify_logged_all adds (kernels/generic_log.hip writes words 1..4)
static_assert(offsetof(l7g_logrec_t, u.mc_text.cmd_off) == 4 && offsetof(l7g_logrec_t, u.mc_text.nkeys) == 12 &&
                  offsetof(l7g_logrec_t, u.mc_binary.key_off) == 4 && offsetof(l7g_logrec_t, u.mc_binary.key_len) == 8 &&
                  offsetof(l7g_logrec_t, u.r2d2.cmd_len) == 4 && offsetof(l7g_logrec_t, u.r2d2.nfields) == 16 &&
                  offsetof(l7g_logrec_t, u.cassandra.table_len) == 4 && offsetof(l7g_logrec_t, u.cassandra.word_len) == 16 &&
                  offsetof(l7g_logrec_t, reserved) == 28,
              "generic record fields");
static_assert(L7G_LOG_MC_TEXT == LOG_MC_TEXT && L7G_LOG_MC_BINARY == LOG_MC_BINARY && L7G_LOG_R2D2 == LOG_R2D2 &&
                  L7G_LOG_CASSANDRA == LOG_CASSANDRA,
              "generic record kinds");

const char *l7g_cass_action_name(int16_t id) { return id >= 0 && id < kCassActions ? CassActionName(id) : nullptr; }

int l7g_stats(l7g_engine *e, l7g_stats_t *out) {
    std::lock_guard<std::mutex> g(e->mu);
    memset(out, 0, sizeof *out);
    out->policies = (uint32_t)e->ps->policies.size();
    out->rules = (uint32_t)e->ps->nrules;
    const HttpImage &H = e->hc->image();
    out->http_rulesets = (uint32_t)H.rulesets.size();
    out->http_chunks = (uint32_t)H.chunks;
    out->http_dfas = (uint32_t)H.dfas;
    out->http_dfa_states = (uint32_t)H.dfa_states;
    const KafkaImage &K = e->kc->image();
    out->kafka_rulesets = (uint32_t)K.rulesets.size();
    out->kafka_rules = (uint32_t)K.rules.size();
    out->kafka_topics = (uint32_t)K.ntopics;
    out->table_bytes = e->blob_bytes;
    out->http_image_bytes = H.images.size();
    out->hot_ruleset = e->hot_ruleset;
    out->hot_image_bytes = e->hot_ruleset >= 0 ? H.rulesets[e->hot_ruleset].image_len : 0;
    const McImage &M = e->mc->image();
    out->mc_rulesets = (uint32_t)M.rulesets.size();
    out->mc_rules = (uint32_t)M.rules;
    out->mc_dfas = (uint32_t)M.dfas;
    out->mc_dfa_states = (uint32_t)M.dfa_states;
    out->http_nfas = (uint32_t)H.nfas;
    out->mc_nfas = (uint32_t)M.nfas;
    out->nfa_pool_bytes = H.nfa_pool.size() + M.nfa_pool.size() + e->r2->image().nfa_pool.size();
    out->r2d2_rulesets = (uint32_t)e->r2->image().rulesets.size();
    out->r2d2_rules = (uint32_t)e->r2->image().rules;
    return 0;
}

int l7g_flow_stats_enable(l7g_engine *e, int on) {
    std::lock_guard<std::mutex> g(e->mu);
    if (e->device < 0) return (int)hipErrorNoDevice;
    e->flow_stats = on != 0;
    return 0;
}

int l7g_flow_stats(l7g_engine *e, l7g_flow_stat_t *out, uint32_t cap, uint32_t *n, int reset) {
    std::lock_guard<std::mutex> g(e->mu);
    if (n) *n = 0;
    if (e->device < 0) return (int)hipErrorNoDevice;
    hipError_t rc = hipSetDevice(e->device);
    if (rc == hipSuccess) rc = WaitLastClassify(e);
    std::vector<uint64_t> h(e->flow_cap * 4, 0);
    if (rc == hipSuccess && e->flow_cap)
        rc = hipMemcpy(h.data(), e->d_flow, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (rc != hipSuccess) return (int)rc;
    uint32_t k = 0;
    for (size_t i = 0; i < e->flow_cap && i < e->skey_list.size(); i++) {
        if (!(h[4 * i] | h[4 * i + 1] | h[4 * i + 2] | h[4 * i + 3])) continue;
        if (k < cap && out) {
            const auto &t = e->skey_list[i];
            out[k] = l7g_flow_stat_t{std::get<0>(t), std::get<1>(t), std::get<3>(t), (uint16_t)std::get<2>(t),
                                     h[4 * i], h[4 * i + 1], h[4 * i + 2], h[4 * i + 3]};
        }
        k++;
    }
    if (n) *n = k;
    // the reset completes before e->mu is released: the next call's flowstats
    // kernel (on a non-blocking stream) cannot overlap it
    if (reset && e->flow_cap) {
        rc = hipMemsetAsync(e->d_flow, 0, e->flow_cap * 4 * sizeof(uint64_t), nullptr);
        if (rc == hipSuccess) rc = hipStreamSynchronize(nullptr);
    }
    return (int)rc;
}

int l7g_profile_enable(l7g_engine *e, int on) {
    std::lock_guard<std::mutex> g(e->mu);
    if (e->device < 0) return (int)hipErrorNoDevice;
    hipError_t rc = hipSetDevice(e->device);
    for (hipEvent_t &ev : e->prof_ev)
        if (rc == hipSuccess && !ev) rc = hipEventCreate(&ev);
    if (rc == hipSuccess) e->profile = on != 0;
    return (int)rc;
}

int l7g_profile_last(l7g_engine *e, float out_ms[4]) {
    std::lock_guard<std::mutex> g(e->mu);
    for (int k = 0; k < 4; k++) out_ms[k] = 0.f;
    bool any = false;
    for (auto &kv : e->scr) any = any || kv.second->launched;
    if (!e->profile || !any) return (int)hipErrorNotReady;
    hipError_t rc = hipEventSynchronize(e->prof_ev[4]);
    for (int k = 0; k < 4 && rc == hipSuccess; k++)
        if (e->prof_ran[k]) rc = hipEventElapsedTime(&out_ms[k], e->prof_ev[k], e->prof_ev[k + 1]);
    return (int)rc;
}

int l7g_debug_phase_times(l7g_engine *e, uint64_t *out16, int reset) {
    if (!e || e->device < 0) return (int)hipErrorNoDevice;
    hipSetDevice(e->device);
    return (int)HttpPhaseTimes(out16, reset != 0);
}

int l7g_debug_frame_phase_times(l7g_engine *e, uint64_t *out8, int reset) {
    if (!e || e->device < 0) return (int)hipErrorNoDevice;
    hipSetDevice(e->device);
    return (int)FramePhaseTimes(out8, reset != 0);
}

int l7g_debug_kafka_phase_times(l7g_engine *e, uint64_t *out8, int reset) {
    if (!e || e->device < 0) return (int)hipErrorNoDevice;
    hipSetDevice(e->device);
    return (int)KafkaPhaseTimes(out8, reset != 0);
}

int l7g_debug_regex(const char *pat, size_t patlen, int anchored, const uint8_t *s, size_t slen, char *err,
                    size_t errlen) {
    std::string m;
    auto ast = re::Parse(std::string(pat, patlen), &m);
    if (!ast) { set_err(err, errlen, m); return -1; }
    re::DFA d;
    std::vector<re::Pattern> ps{{ast.get(), anchored != 0}};
    if (!re::BuildDFA(ps, 1 << 16, &d, &m)) { set_err(err, errlen, m); return -1; }
    auto acc = re::RunDFA(d, s, slen);
    return (int)(acc[0] & 1);
}

int l7g_debug_regex_nfa(const char *pat, size_t patlen, int anchored, const uint8_t *s, size_t slen, char *err,
                        size_t errlen) {
    std::string m;
    auto ast = re::Parse(std::string(pat, patlen), &m);
    if (!ast) { set_err(err, errlen, m); return -1; }
    re::BitNfa n;
    if (!re::BuildBitNfa({ast.get(), anchored != 0}, kNfaMaxPositions, &n, &m, kNfaMaxWords)) {
        set_err(err, errlen, m);
        return -1;
    }
    std::vector<uint8_t> pool;
    const uint64_t off = AppendDevNfa(n, &pool, &m);
    if (off == ~0ull) { set_err(err, errlen, m); return -1; }
    std::vector<uint64_t> scratch(2 * (size_t)n.W);  // (a large NFA's state sets)
    return nfa_run(pool.data(), off, s, (uint32_t)slen, scratch.data()) ? 1 : 0;
}

}  // extern "C"
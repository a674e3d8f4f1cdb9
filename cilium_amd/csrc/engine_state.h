// The engine behind the C-ABI (include/l7gpu.h): its state, the thresholds of
// its launch plan, and the few internals shared by capi.cc (lifetime, policy,
// tables, connections, statistics), classify.cc (the launch plan and the call
// frame of every device-pointer entry: DevIn, DevOut, CallBegin, CallEnd),
// cass_sessions.cc, kafka_sessions.cc and mc_sessions.cc (the session tables;
// their shared lifetime is sessions.h), host_call.cc (the per-thread host staging path:
// HostCtx, StagePair, CallViews) and service.cc (the resident services).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/l7gpu.h"
#include "capi_internal.h"
#include "engine/cass_compile.h"
#include "engine/http_compile.h"
#include "engine/kafka_compile.h"
#include "engine/mc_compile.h"
#include "engine/r2_compile.h"
#include "kernels/launch.h"  // (with it: device_tables.h, call_layout.h, copy_in_types.h, service_types.h)
#include "policy/policy.h"

using namespace l7;

// Scratch of the l7g_classify calls on one caller stream: the partition lists,
// the NFA pre-pass bits, the counter histograms, the compressed-Kafka decode
// region, and the completion event of the last call on that stream.  Calls on
// different streams use different scratch and run concurrently; calls on one
// stream are ordered by the stream itself.
struct StreamScratch {
    // protocol split (grow-only), in words: [counts(kCntWords) | n memcached entries (ListEnt, 4 words each) |
    // n HTTP entries | L7_KAFKA_CLASSES x n Kafka idx | n idx of Kafka requests with compressed messages]
    uint32_t *d_sel = nullptr;
    size_t sel_cap = 0;
    // NFA pre-pass results, u64 per request (grow-only)
    uint64_t *d_nfa = nullptr;
    size_t nfa_cap = 0;
    // counter histogram scratch (kernels/counters.hip), allocated on first use
    uint32_t *d_hist = nullptr;
    // cassandra USE list: [count | n request indices] (grow-only)
    void *d_use = nullptr;  // cassandra: USE keys, sorted keys, sort temp (bytes)
    size_t use_cap = 0;
    // work counters of unpartitioned batches (HTTP tile counters), allocated on first use
    uint32_t *d_work = nullptr;
    // HTTP requests grouped by rule set (kernels/http_group.hip), grow-only:
    // [big-image list(n entries, 4 words each) | ctl(8) | hist(R) | cursor(R) |
    //  segments(3 x (n / kGroupSegEntries + R + 1)) | grouped list(n)]
    uint32_t *d_grp = nullptr;
    size_t grp_cap = 0;
    // large NFAs' state sets: a lane's 2 W words for each lane of a launch (grow-only)
    uint64_t *d_bignfa = nullptr;
    size_t bignfa_bytes = 0;
    // l7g_deny_replies: [counters | Kafka index list | scan temporary storage] (bytes, grow-only)
    void *d_reply = nullptr;
    size_t reply_cap = 0;
    // l7g_kafka_forward: [keys | sorted keys | per-connection segments | sort temporary storage];
    // l7g_kafka_responses: the entry each response found (bytes, grow-only)
    void *d_ksess = nullptr;
    size_t ksess_cap = 0;
    // l7g_mc_forward: [keys | sorted keys | info bytes | scan elements | scanned | per-connection segments |
    // sort / scan temporary storage] (bytes, grow-only)
    void *d_mcsess = nullptr;
    size_t mcsess_cap = 0;
    // completion of the last call's kernels on this stream
    hipEvent_t done_ev = nullptr;
    bool launched = false;
    uint64_t last_use = 0;
    // the memcached kernel beside the Kafka kernel (large mixed batches)
    hipStream_t side = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    // Grows one of the grow-only buffers to `bytes` when need (in the units *cap
    // keeps) exceeds *cap.  The previous call on this stream may still use the
    // old buffer: it is freed only once that call's kernels have finished.
    template <class T>
    hipError_t Grow(T **buf, size_t *cap, size_t need, size_t bytes) {
        if (need <= *cap) return hipSuccess;
        hipError_t rc = hipSuccess;
        if (*buf) {
            if (launched) rc = hipEventSynchronize(done_ev);
            hipFree(*buf);
            *buf = nullptr;
            *cap = 0;
        }
        if (rc == hipSuccess) rc = hipMalloc(buf, bytes);
        if (rc == hipSuccess) *cap = need;
        return rc;
    }
    ~StreamScratch() {
        if (side) hipStreamSynchronize(side);
        if (fork_ev) hipEventDestroy(fork_ev);
        if (join_ev) hipEventDestroy(join_ev);
        if (side) hipStreamDestroy(side);
        for (void *p : {(void *)d_bignfa, (void *)d_grp, (void *)d_sel, (void *)d_nfa, (void *)d_hist, d_use, (void *)d_work,
                        d_reply, d_ksess, d_mcsess})
            if (p) hipFree(p);
        if (done_ev) hipEventDestroy(done_ev);
    }
};
constexpr size_t kMaxStreamScratch = 16;   // per-stream scratch sets; beyond: the least recently used one is handed over
constexpr uint32_t kDynTilesMin = 1u << 18;  // unpartitioned HTTP batches from this size take tiles from a counter
// l7g_classify_host calls up to this size run zero-copy (kernels on the pinned staging)
constexpr uint32_t kZeroCopyMaxRequests = 256;
constexpr size_t kZeroCopyMaxBytes = 256 * 1024;
// batches below this size skip the protocol split when one classifier can walk them alone
constexpr uint32_t kPartitionMin = 4096;
constexpr uint32_t kBesideMin = 1u << 20;  // memcached kernel beside Kafka from this batch size
// host calls up to this size check their connections for cold rule sets
constexpr uint32_t kHostScanMax = 4096;
// at most this many requests: the HTTP requests are framed one per wave, their
// lines side by side (http_latency_kernel), not one per lane
constexpr uint32_t kLatencyMax = 64;
// batches from this size with HTTP requests on more than one rule set take the grouped path
constexpr uint32_t kGroupMin = 1u << 16;
constexpr size_t kNfaScratchBytes = 256ull << 20;  // large NFAs: state-set scratch per stream (lanes in flight)

// A grow-only buffer on the device with its pinned host twin: what a
// host-buffer call stages beside the call layout (HostCtx below).
struct StagePair {
    uint8_t *dev = nullptr, *pin = nullptr;
    size_t cap = 0;  // bytes of each; 0 after a failed allocation
    // At least `need` bytes of each.  The stream's last call may still use the
    // old ones: it ends before they are freed.  (some slack: batches vary)
    hipError_t Grow(hipStream_t s, size_t need) {
        if (need <= cap) return hipSuccess;
        hipStreamSynchronize(s);
        Free();
        const size_t c = need + need / 4;
        hipError_t rc = hipMalloc(&dev, c);
        if (rc == hipSuccess) rc = hipHostMalloc(&pin, c, hipHostMallocDefault);
        if (rc == hipSuccess) cap = c;
        return rc;
    }
    void Free() {
        if (dev) hipFree(dev);
        if (pin) hipHostFree(pin);
        dev = pin = nullptr;
        cap = 0;
    }
    StagePair() = default;
    StagePair(const StagePair &) = delete;
    ~StagePair() { Free(); }
};

// l7g_classify_host's per-thread staging: its own stream, device arena and
// request arrays (grow-only), so host-buffer calls from different threads
// overlap instead of queueing on one stream.
// Inputs go over as ONE copy from a pinned staging buffer and outputs come
// back as ONE copy (both packed by the host as kernels/call_layout.h lays
// them out); a small call is not copied at all (the kernels read and write
// the pinned buffers in place, see HostRun).
struct HostCtx {
    hipStream_t s = nullptr;
    uint8_t *dev = nullptr;        // device: [inputs | outputs]
    uint8_t *pin_in = nullptr;     // pinned host staging of the inputs
    uint8_t *pin_out = nullptr;    // pinned host staging of the outputs
    uint8_t *pin_in_dev = nullptr;   // their device addresses (zero-copy; looked up once)
    uint8_t *pin_out_dev = nullptr;
    uint32_t *pin_done = nullptr;     // pinned word the call's last kernel stores its sequence number to
    uint32_t *pin_done_dev = nullptr;
    uint32_t seq = 0;
    size_t in_cap = 0, out_cap = 0;
    // l7g_classify_logged_host, l7g_classify_logged_all_host: [records | span rows | text rows]
    StagePair log;
    // l7g_deny_replies_host: [verdict in | off | len | total | reply bytes]
    StagePair reply;
    // l7g_kafka_forward_host / l7g_kafka_responses_host: what the call layout has no place for (the verdicts
    // and tags in, the per-frame outputs back)
    StagePair ksess;
    // l7g_mc_forward_host / l7g_mc_replies_host: likewise (the verdicts and tags in, act back; the ops back)
    StagePair mcsess;
    ~HostCtx() {  // (the four pairs free themselves after this, the stream idle by then)
        if (s) hipStreamSynchronize(s);
        if (dev) hipFree(dev);
        if (pin_in) hipHostFree(pin_in);
        if (pin_out) hipHostFree(pin_out);
        if (pin_done) hipHostFree(pin_done);
        if (s) hipStreamDestroy(s);
    }
};

// where a call's inputs lie in pinned host memory: the thread's staging, or a
// batcher slot filled in place (its three arrays `stride` entries apart, its
// request bytes in one piece per lane)
struct HostIn {
    const uint64_t *off;
    const uint32_t *len, *conn;
    size_t stride;  // > 0: len and conn lie at CallLenOff(stride) and CallConnOff(stride) from off
    const l7g_host_seg *seg;
    int nseg;  // the arena is these pieces, concatenated
};

// The inputs of a call as its kernels see them: request i is arena[off[i] ..
// off[i] + len[i]) on connection conn[i].  Device pointers (host_call.cc's
// HostStage takes a caller's host arrays in the same form).
struct DevIn {
    const uint8_t *arena;
    uint64_t arena_len;
    const uint64_t *off;
    const uint32_t *len, *conn;
    uint32_t n;
};
// The views of call-layout inputs (kernels/call_layout.h) that start at `base`,
// the three arrays `stride` entries long: a staging on the device, or the
// pinned one.
inline DevIn CallViews(const uint8_t *base, size_t stride, uint64_t arena_len, uint32_t n) {
    return {base + CallArenaOff(stride), arena_len, (const uint64_t *)base, (const uint32_t *)(base + CallLenOff(stride)),
            (const uint32_t *)(base + CallConnOff(stride)), n};
}
// l7g_classify's outputs (device pointers; counters may be null)
struct DevOut {
    uint8_t *verdict;
    int32_t *rule;
    uint32_t *consumed;
    uint64_t *counters;
};
// What a caller of Classify other than l7g_classify adds (classify.cc)
struct ClassifyOpts {
    const uint32_t *host_conn = nullptr;  // the connection indices in host memory as well
    const CopyIn *pre = nullptr;          // the inputs' copy from pinned memory, still to be done
    bool *signaled = nullptr;             // out: the call's last kernel stores pre->done
    const LogOut *log = nullptr;          // l7g_classify_logged's outputs
    const LogText *text = nullptr;        // l7g_classify_logged_all's (with log)
};

// ---- resident services (kernels/service.h): the synchronous drop-in calls
// (one Allowed(), one OnData) posted to a polling workgroup instead of launched
constexpr uint32_t kSvcHttpMax = 8;    // HTTP requests per call (one per wave of the workgroup)
constexpr uint32_t kSvcMcMax = 64;     // memcached requests per call (one wave)
constexpr size_t kSvcInBytes = CallInCap(kSvcMcMax, kZeroCopyMaxBytes);
constexpr size_t kSvcOutBytes = CallOutCap(kSvcMcMax);
static_assert(kSvcInBytes == 1024 + 256 * 1024 + 64 && kSvcOutBytes == 64 * 9 + 64, "the services' staging");
// a service leaves after this many shader-clock cycles without a call (~50 ms at 2.4 GHz)
constexpr uint64_t kSvcIdleCycles = 120000000ull;
struct Service {
    std::mutex mu;  // one call at a time, held from its posting to its answers
    hipStream_t s = nullptr;
    SvcBox *box = nullptr, *box_dev = nullptr;  // pinned, coherent
    SvcBox *box_ready = nullptr;  // box, published once the service is allocated (read without mu)
    uint8_t *pin_in = nullptr, *pin_in_dev = nullptr, *pin_out = nullptr, *pin_out_dev = nullptr;
    uint8_t *dev_in = nullptr;
    uint32_t seq = 0;
    bool launched = false;  // a workgroup may be serving (launched, not yet seen leaving)
    // its launch arguments: the tables and connections it serves with
    HttpTables ht{};
    McTables mt{};
    const DevConn *conns = nullptr;
    uint32_t nconns = 0;
    uint64_t calls = 0, launches = 0;
    ~Service() {
        if (s) hipStreamSynchronize(s);
        if (dev_in) hipFree(dev_in);
        if (pin_in) hipHostFree(pin_in);
        if (pin_out) hipHostFree(pin_out);
        if (box) hipHostFree(box);
        if (s) hipStreamDestroy(s);
    }
};

// The new-connection events one protocol's device tables have not seen yet: connection indices, or every connection.
struct SessionResets {
    std::vector<uint32_t> pending;
    bool all = false;
    void Clear() { All(false); }
    void All(bool on) { pending.clear(); all = on; }  // l7g_conns_set: every connection is new (on: sessions are)
    void Add(bool on, const uint32_t *conn, size_t n) { if (on && !all) pending.insert(pending.end(), conn, conn + n); }
};

struct l7g_engine {
    int device = 0;
    // [0] HTTP, [1] memcached (l7g_service_enable; L7G_SERVICE=0 turns them off)
    Service svc[2];
    std::atomic<bool> svc_on{true};  // (ServiceTry reads it before it takes mu)
    std::mutex mu;
    std::unique_ptr<PolicySet> ps;
    std::unique_ptr<HttpCompiler> hc;
    std::unique_ptr<KafkaCompiler> kc;
    // index[] words up to which a Kafka rule set gets its dense per-topic table (kafka_compile.h;
    // L7G_KAFKA_DENSE_BUDGET at engine creation lowers it, for tests of the sorted-directory form)
    size_t kafka_dense_budget = kDenseTopicBudget;
    std::unique_ptr<McCompiler> mc;
    std::unique_ptr<R2Compiler> r2;
    std::unique_ptr<CassCompiler> cs;
    std::vector<l7g_conn_t> attrs;
    std::vector<DevConn> conns;
    uint8_t *d_blob = nullptr;
    size_t blob_bytes = 0;
    // the policy version's source (l7g_tables_export ships it with the compiled tables)
    std::string policy_src;
    int policy_form = 0, policy_px = 0;
    DevConn *d_conns = nullptr;
    size_t conns_cap = 0;
    HttpTables ht{};
    KafkaTables kt{};
    McTables mt{};
    R2Tables rt{};
    CassTables ct{};
    bool tables_dirty = true, conns_dirty = true;
    bool has_http = false, has_kafka = false, has_mc = false, has_r2 = false, has_cs = false;
    int32_t hot_ruleset = -1;  // HTTP rule set staged in LDS (most connections)
    bool any_big_image = false;  // some HTTP rule set's image exceeds kGroupImageBytes
    // l7g_classify_host contexts, one per calling thread (guarded by hmu)
    std::mutex hmu;
    std::map<std::thread::id, std::unique_ptr<HostCtx>> hctx;
    bool any_cold = false;     // some HTTP connection uses another rule set
    // decode region of kafka_inflate_kernel (one slice per workgroup, 1 GiB),
    // allocated with the first Kafka batch and shared by every stream: each
    // call's inflate launch waits for zreg_ev, the previous one's completion
    uint8_t *d_zreg = nullptr;
    hipEvent_t zreg_ev = nullptr;
    bool zreg_used = false;
    // per-stream scratch of l7g_classify (guarded by mu)
    std::map<hipStream_t, std::unique_ptr<StreamScratch>> scr;
    uint64_t calls = 0;
    // proxy statistics: key (policy, proto, port, ingress) per connection, and
    // the device accumulator u64[keys][4] (l7g_flow_stats_*)
    std::map<std::tuple<int32_t, uint8_t, uint32_t, uint8_t>, uint16_t> skeys;
    std::vector<std::tuple<int32_t, uint8_t, uint32_t, uint8_t>> skey_list;
    bool flow_stats = false;
    uint64_t *d_flow = nullptr;
    size_t flow_cap = 0;  // keys the accumulator holds
    // The sessions of three protocols, each kept the same way (sessions.h): the
    // device tables, one slot per connection index grown with the connection
    // table, and the new-connection events since the last launch (applied by
    // the protocol's ...Sync before the next one).
    // cassandra (l7g_cass_sessions_enable; on while sess.by_id is set; kernels/cassandra_session.hip)
    CassSessions sess{};
    SessionResets sess_reset;
    // Kafka (l7g_kafka_sessions_enable; on while ksess.tab is set; kernels/kafka_session.hip)
    KafkaSessions ksess{};
    SessionResets ksess_reset;
    uint64_t ksess_expired = 0;  // entries l7g_kafka_session_gc dropped since enable
    // memcached (l7g_mc_sessions_enable; on while mcsess.stats is set; kernels/memcached_session.hip): a ring
    // beside every slot
    McSessions mcsess{};
    uint32_t mcsess_ring_slots = 0;  // connections the ring has room for (follows mcsess.nslots)
    SessionResets mcsess_reset;
    // Every stream's last completion event (StreamScratch::done_ev) is waited
    // on -- never a caller's stream, which may be gone by then -- before the
    // engine rewrites or frees anything a launched kernel reads: the
    // connection table, the table blob, the proxy-statistics accumulator.
    // l7g_profile_*: timing events around each launch of the last call
    bool profile = false;
    hipEvent_t prof_ev[5] = {};
    bool prof_ran[4] = {};
};

#pragma GCC visibility push(hidden)  // (the functions below: shared by the host files, not exported)

// The protocols of a small call's connections, read on the host (e->mu held);
// the launch plan and the services both select by it.
struct ConnScan {
    uint32_t seen, owned;  // bit per protocol present; those some classifier owns
    bool any_cold;         // some HTTP request's rule set is not the hot one
    bool http_only, mc_only;  // every owned request is HTTP (memcached), which the engine serves
};
inline ConnScan ScanConns(const l7g_engine *e, const uint32_t *host_conn, uint32_t n) {
    ConnScan c{};
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t ci = host_conn[i];
        if (ci >= e->conns.size()) continue;
        const uint32_t pr = e->attrs[ci].proto;
        if (pr < 32) c.seen |= 1u << pr;
        c.any_cold = c.any_cold || (pr == PROTO_HTTP && e->conns[ci].ruleset != e->hot_ruleset);
    }
    c.any_cold = c.any_cold && e->any_cold;
    c.owned = c.seen & ((1u << PROTO_HTTP) | (1u << PROTO_KAFKA) | (1u << PROTO_MEMCACHE) | (1u << PROTO_R2D2) |
                        (1u << PROTO_CASSANDRA));
    c.http_only = c.owned == (1u << PROTO_HTTP) && e->has_http;
    c.mc_only = c.owned == (1u << PROTO_MEMCACHE) && e->has_mc;
    return c;
}

// The next sequence number of a done word (never 0, the word's initial value).
inline uint32_t NextSeq(uint32_t &seq) {
    if (!++seq) ++seq;
    return seq;
}

// Spins until load() returns seq; false once `limit` has passed (looked at every 256 polls).
template <class Load>
inline bool SpinUntil(Load load, uint32_t seq, std::chrono::milliseconds limit) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t k = 0;; k++) {
        if (load() == seq) return true;
        if ((k & 255) == 255 && std::chrono::steady_clock::now() - t0 > limit) return false;
        __builtin_ia32_pause();
    }
}

// an error message into a caller's buffer (truncated to fit)
inline void set_err(char *err, size_t errlen, const std::string &m) {
    if (!err || errlen == 0) return;
    size_t n = std::min(errlen - 1, m.size());
    memcpy(err, m.data(), n);
    err[n] = 0;
}

hipError_t Upload(l7g_engine *e);            // capi.cc (e->mu held)
hipError_t WaitLastClassify(l7g_engine *e);  // classify.cc (e->mu held), as Classify (takes e->mu)
// cass_sessions.cc (e->mu held): with sessions on, a slot for every connection and the pending resets applied
hipError_t SessionsSync(l7g_engine *e);
void SessionsFree(l7g_engine *e);
// kafka_sessions.cc (e->mu held): the same for the Kafka sessions
hipError_t KafkaSessionsSync(l7g_engine *e);
void KafkaSessionsFree(l7g_engine *e);
// mc_sessions.cc (e->mu held): the same for the memcached sessions
hipError_t McSessionsSync(l7g_engine *e);
void McSessionsFree(l7g_engine *e);
// classify.cc (e->mu held): the scratch of stream s, the call ordered behind that scratch's last user
hipError_t GetScratch(l7g_engine *e, hipStream_t s, StreamScratch **out);
// classify.cc (e->mu held, the entry's own checks passed): what every call over a batch starts with -- the
// device, the tables and connections uploaded, the named sessions synced, and (scratch not null) GetScratch --
// and ends with: done_ev recorded behind the call's launches, which WaitLastClassify waits on.
enum : unsigned { kSyncNone = 0, kSyncCass = 1, kSyncKafka = 2, kSyncMc = 4 };
hipError_t CallBegin(l7g_engine *e, unsigned sync, hipStream_t s, StreamScratch **scratch);
hipError_t CallEnd(StreamScratch *S, hipStream_t s, hipError_t rc);
// classify.cc: l7g_classify and its logged forms (device pointers; takes e->mu)
int Classify(l7g_engine *e, const DevIn &in, const DevOut &out, void *stream, const ClassifyOpts &o = {});
// cass_sessions.cc: l7g_cass_replies (device pointers; takes e->mu)
int CassReplies(l7g_engine *e, const DevIn &in, uint8_t *verdict, uint32_t *consumed, void *stream);
// classify.cc: l7g_deny_replies (device pointers; takes e->mu)
int DenyReplies(l7g_engine *e, const DevIn &in, const uint8_t *verdict, const l7g_reply_out_t *out, void *stream);
void StopServices(l7g_engine *e);  // service.cc, as the next two
void ReleaseServiceCUs(l7g_engine *e);
bool ServiceTry(l7g_engine *e, uint32_t n, uint64_t arena_len, const HostIn &in, uint8_t *verdict, int32_t *rule,
                uint32_t *consumed, hipError_t *rc_out);

#pragma GCC visibility pop

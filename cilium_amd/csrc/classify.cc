// The launch plan behind l7g_classify (product code): which kernels a call
// runs, on which lists, with which per-stream scratch, in which order.
#include <algorithm>

#include "deny_templates.h"
#include "engine_state.h"

// (0 in a variant build: the leg without the second Kafka grid, for A/B)
#ifndef L7G_KAFKA_HELPER
#define L7G_KAFKA_HELPER 1
#endif

int l7::DeviceCuCount() {
    static const int cus = [] {
        int dev = 0, c = 0;
        return hipGetDevice(&dev) == hipSuccess &&
                       hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0
                   ? c
                   : 256;
    }();
    return cus;
}

// Waits for the kernels of every stream's last call, and stops the services
// (their launch arguments are what the caller is about to rewrite).  Caller
// holds e->mu.
hipError_t WaitLastClassify(l7g_engine *e) {
    StopServices(e);
    hipError_t rc = hipSuccess;
    for (auto &kv : e->scr)
        if (kv.second->launched) {
            hipError_t r = hipEventSynchronize(kv.second->done_ev);
            if (r != hipSuccess) rc = r;
        }
    return rc;
}

// The scratch of stream s (created on first use; past kMaxStreamScratch the
// least recently used stream's scratch is handed over once s has been made
// to wait for that stream's last call).  Caller holds e->mu.
hipError_t GetScratch(l7g_engine *e, hipStream_t s, StreamScratch **out) {
    auto it = e->scr.find(s);
    if (it == e->scr.end()) {
        if (e->scr.size() >= kMaxStreamScratch) {
            auto lru = e->scr.begin();
            for (auto j = e->scr.begin(); j != e->scr.end(); ++j)
                if (j->second->last_use < lru->second->last_use) lru = j;
            std::unique_ptr<StreamScratch> sc = std::move(lru->second);
            e->scr.erase(lru);
            if (sc->launched) {
                hipError_t rc = hipStreamWaitEvent(s, sc->done_ev, 0);
                if (rc != hipSuccess) return rc;
            }
            it = e->scr.emplace(s, std::move(sc)).first;
        } else {
            auto sc = std::make_unique<StreamScratch>();
            hipError_t rc = hipEventCreateWithFlags(&sc->done_ev, hipEventDisableTiming);
            if (rc != hipSuccess) return rc;
            it = e->scr.emplace(s, std::move(sc)).first;
        }
    }
    // (a handle can be reused by a new stream while the old one's work is
    // still pending: order the call after that work whatever the stream;
    // nothing to wait for once it has completed -- the synchronous callers)
    if (it->second->launched && hipEventQuery(it->second->done_ev) != hipSuccess) {
        hipError_t rc = hipStreamWaitEvent(s, it->second->done_ev, 0);
        if (rc != hipSuccess) return rc;
    }
    it->second->last_use = ++e->calls;
    *out = it->second.get();
    return hipSuccess;
}

hipError_t CallBegin(l7g_engine *e, unsigned sync, hipStream_t s, StreamScratch **scratch) {
    hipError_t rc = hipSetDevice(e->device);
    if (rc == hipSuccess) rc = Upload(e);
    if (rc == hipSuccess && (sync & kSyncCass)) rc = SessionsSync(e);
    if (rc == hipSuccess && (sync & kSyncKafka)) rc = KafkaSessionsSync(e);
    if (rc == hipSuccess && (sync & kSyncMc)) rc = McSessionsSync(e);
    if (rc == hipSuccess && scratch) rc = GetScratch(e, s, scratch);
    return rc;
}

hipError_t CallEnd(StreamScratch *S, hipStream_t s, hipError_t rc) {
    if (rc == hipSuccess) rc = hipEventRecord(S->done_ev, s);
    if (rc == hipSuccess) S->launched = true;
    return rc;
}

// l7g_classify over the call frame (in, out; o: what the other callers add);
// host_conn: the connection indices in host memory as well
// (l7g_classify_host's calls), so that a small call whose requests all use the
// hot HTTP rule set skips the general HTTP kernel's launch
// pre: the call's inputs still to be copied from pinned host memory to where
// arena / off / len / conn point (HostRun); done by the first kernel when the
// call is one workgroup of one classifier, else by copy_in_kernel first.
// log: l7g_classify_logged's outputs (device memory).  The plan is the same;
// the Kafka grids are the logged instantiations, and http_log_kernel follows
// the classifiers (it reads their verdicts).
// text: l7g_classify_logged_all's (with log): the logged plan, with
// http_log_kernel moved before the cassandra step and generic_log_kernel after
// the cassandra classifier -- with sessions, before that call's commit.
int Classify(l7g_engine *e, const DevIn &in, const DevOut &out, void *stream, const ClassifyOpts &o) {
    const uint32_t n = in.n;
    uint64_t *const counters = out.counters;
    const uint32_t *const host_conn = o.host_conn;
    const CopyIn *const pre = o.pre;
    const LogOut *const log = o.log;
    const LogText *const text = o.text;
    std::lock_guard<std::mutex> g(e->mu);
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (log && (!log->rec || ((uintptr_t)log->rec & 15) || (log->stride && !log->topics) || pre))
        return (int)hipErrorInvalidValue;
    if (text && (!log || (text->stride && !text->text))) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    hipError_t rc = CallBegin(e, kSyncCass, s, n ? &S : nullptr);
    if (rc != hipSuccess || n == 0) return (int)rc;
    const Batch B{in.arena, in.arena_len, in.off, in.len, in.conn, e->d_conns, out.verdict, out.rule, out.consumed,
                  n, (uint32_t)e->conns.size()};
    // The kernels each classify only their own protocol's requests, so a
    // mixed batch needs one launch per protocol present.  When the engine
    // serves more than one protocol, partition_kernel runs first: it writes
    // the lists the classifiers walk (Kafka indices; memcached and HTTP packed
    // entries, ListEnt in device_tables.h), and answers
    // the requests no classifier owns (unknown connection, no parser) itself.
    // A single-protocol HTTP or memcached engine skips it; its one kernel walks the whole batch
    // and answers those requests.
    const int nproto = (int)e->has_http + (int)e->has_kafka + (int)e->has_mc + (int)e->has_r2 + (int)e->has_cs;
    // (a Kafka-only or memcached-only engine partitions too: the kind / length
    // lists keep the Kafka kernel's waves converged, 1.55 -> 0.99 ms on cfg3,
    // and the text / binary lists the memcached kernel's)
    // (a small memcached-only batch gains nothing from converged waves: its one
    // kernel walks the batch itself, one launch fewer on the latency path)
    bool partitioned = nproto > 1 || e->has_kafka || (e->has_mc && n >= kPartitionMin);
    bool any_cold = e->any_cold;
    // which kernels run: a small call whose connections the host can read (the
    // synchronous drop-ins: one Allowed(), one OnData) launches only the kernel
    // of the one protocol its requests use, unpartitioned, where it answers the
    // requests no parser owns too -- no partition pass, no counter memset, no
    // launch of the other protocols' kernels on an empty list
    bool run_http = e->has_http || nproto == 0, run_kafka = e->has_kafka, run_mc = e->has_mc;
    bool run_r2 = e->has_r2, run_cs = e->has_cs;
    if (host_conn && n <= kHostScanMax) {
        const ConnScan scan = ScanConns(e, host_conn, n);
        any_cold = scan.any_cold;
        if (scan.http_only) {
            partitioned = run_kafka = run_mc = run_r2 = run_cs = false;
        } else if (scan.mc_only) {
            partitioned = run_http = run_kafka = run_r2 = run_cs = false;
        }
    }
    if (n >= kPartitionMin) ReleaseServiceCUs(e);  // (persistent grids: every CU)
    uint32_t *sel_k = nullptr, *sel_z = nullptr, *cnt = nullptr;
    ListEnt *sel_m = nullptr, *sel_h = nullptr;
    if (partitioned) {
        const size_t need = kCntWords + PartitionListWords(n);
        rc = S->Grow(&S->d_sel, &S->sel_cap, need, need * sizeof(uint32_t));
        if (rc != hipSuccess) return (int)rc;
        cnt = S->d_sel;  // (its words: device_tables.h kCnt*)
        // the entry lists first: 16-byte aligned behind the counts block
        static_assert(kCntWords % 4 == 0 && sizeof(ListEnt) == 16, "entry lists start on 16 bytes");
        sel_m = reinterpret_cast<ListEnt *>(S->d_sel + kCntWords);
        sel_h = sel_m + (size_t)n;
        sel_k = reinterpret_cast<uint32_t *>(sel_h + (size_t)n);
        sel_z = sel_k + L7_KAFKA_CLASSES * (size_t)n;
        if (rc == hipSuccess) rc = hipMemsetAsync(cnt, 0, kCntWords * sizeof(uint32_t), s);
        if (rc == hipSuccess && e->has_kafka && !e->d_zreg) {
            rc = hipEventCreateWithFlags(&e->zreg_ev, hipEventDisableTiming);
            if (rc == hipSuccess) rc = hipMalloc(&e->d_zreg, (size_t)KafkaInflateBlocks() * KafkaInflateRegionBytes());
        }
        if (rc != hipSuccess) return (int)rc;
    }
    // rule sets with NFA-fallback matchers: the pre-pass writes one u64 per request
    HttpTables ht = e->ht;
    const bool nfa = e->ht.nfa_pool != nullptr && run_http;
    if (nfa && rc == hipSuccess) {
        rc = S->Grow(&S->d_nfa, &S->nfa_cap, n, (size_t)n * sizeof(uint64_t));
        if (rc != hipSuccess) return (int)rc;
        ht.nfa_bits = S->d_nfa;
    }
    // large NFAs: one scratch for the call's launches (they run one after
    // another on this stream), as many lanes as a budget allows; the kernels
    // loop over their requests with that many lanes
    McTables mt = e->mt;
    R2Tables rt = e->rt;
    CassTables ct = e->ct;
    uint32_t big_lanes = 0;
    {
        const uint32_t lw = std::max({ht.nfa_lane_words, mt.nfa_lane_words, rt.nfa_lane_words, ct.nfa_lane_words});
        if (lw && rc == hipSuccess) {
            const size_t lane_bytes = (size_t)lw * 8;
            size_t lanes = std::min<size_t>(((size_t)n + 255) & ~(size_t)255, kNfaScratchBytes / lane_bytes);
            lanes = std::max<size_t>(lanes & ~(size_t)255, 256);
            rc = S->Grow(&S->d_bignfa, &S->bignfa_bytes, lanes * lane_bytes, lanes * lane_bytes);
            if (rc != hipSuccess) return (int)rc;
            big_lanes = (uint32_t)(S->bignfa_bytes / lane_bytes);
            uint64_t *sc = S->d_bignfa;
            if (ht.nfa_lane_words) { ht.nfa_scratch = sc; ht.nfa_lane_words = lw; }
            if (mt.nfa_lane_words) { mt.nfa_scratch = sc; mt.nfa_lane_words = lw; }
            if (rt.nfa_lane_words) { rt.nfa_scratch = sc; rt.nfa_lane_words = lw; }
            if (ct.nfa_lane_words) { ct.nfa_scratch = sc; ct.nfa_lane_words = lw; }
        }
    }
    // profiling: event k is recorded before stage k (partition, http, kafka, memcache), event 4 after the last
    const bool prof = e->profile;
    auto mark = [&](int k) {
        if (prof && rc == hipSuccess) rc = hipEventRecord(e->prof_ev[k], s);
    };
    // the copy of a small call's inputs: inside the one kernel that reads them
    // when that kernel is one workgroup (HTTP: one request per wave, at most 8;
    // memcached: at most 64 requests, one wave), else a launch of its own
    const bool only_http = run_http && !partitioned && !run_kafka && !run_mc && !run_r2 && !run_cs;
    const bool only_mc = run_mc && !partitioned && !run_http && !run_kafka && !run_r2 && !run_cs;
    const CopyIn *fuse_http = pre && only_http && !nfa && n <= 8 ? pre : nullptr;
    const CopyIn *fuse_mc = pre && only_mc && n <= 64 ? pre : nullptr;
    if (pre && !fuse_http && !fuse_mc && rc == hipSuccess) {
        CopyIn c = *pre;
        c.done = nullptr;  // (the classifiers that follow end the call)
        rc = LaunchCopyIn(c, s);
    }
    // the one-workgroup kernel that ends the call stores the done word (and no
    // counters or proxy statistics follow it)
    const bool signal = (fuse_http || fuse_mc) && pre->done && !counters && !(e->flow_stats && !e->skey_list.empty());
    CopyIn fused_c{};
    if (fuse_http || fuse_mc) {
        fused_c = *pre;
        if (!signal) fused_c.done = nullptr;
    }
    if (fuse_http) fuse_http = &fused_c;
    if (fuse_mc) fuse_mc = &fused_c;
    if (o.signaled) *o.signaled = signal;
    const bool run[4] = {partitioned, run_http, run_kafka, run_mc};
    for (int k = 0; k < 4; k++) e->prof_ran[k] = run[k];
    mark(0);
    if (rc == hipSuccess && run[0]) rc = LaunchPartition(B, sel_k, sel_m, sel_h, cnt, s);
    mark(1);
    if (rc == hipSuccess && run[1] && nfa) rc = LaunchHttpNfa(B, ht, big_lanes, s);
    // tile counters: in the partition counts (zeroed above), or, for a large
    // unpartitioned batch, two words zeroed here (a small batch keeps the fixed
    // stride and saves the memset)
    uint32_t *tile_ctr = cnt ? cnt + kCntHttpTiles : nullptr;
    if (rc == hipSuccess && run[1] && !cnt && n >= kDynTilesMin) {
        if (!S->d_work) rc = hipMalloc(&S->d_work, 4 * sizeof(uint32_t));
        if (rc == hipSuccess) rc = hipMemsetAsync(S->d_work, 0, 2 * sizeof(uint32_t), s);
        tile_ctr = S->d_work;
    }
    // many rule sets in use: the HTTP requests sorted by rule set, so that each
    // workgroup stages one image per segment (kernels/http_group.hip)
    const bool grouped = run[1] && any_cold && n >= kGroupMin && ht.nrulesets >= 2 &&
                         ht.nrulesets <= kMaxGroupRulesets;
    if (rc == hipSuccess && grouped) {
        const size_t R = ht.nrulesets, segw = 3 * ((size_t)n / kGroupSegEntries + R + 1);
        const size_t need = 8 + 2 * R + segw + 5 * (size_t)n;
        rc = S->Grow(&S->d_grp, &S->grp_cap, need, need * sizeof(uint32_t));
        // (the big-image list holds entries, the general kernel's input: first, 16-byte aligned)
        ListEnt *gbig = reinterpret_cast<ListEnt *>(S->d_grp);
        uint32_t *ctl = S->d_grp + 4 * (size_t)n, *hist = ctl + 8, *cursor = hist + R, *segs = cursor + R,
                 *gsel = segs + segw;
        if (rc == hipSuccess) rc = hipMemsetAsync(ctl, 0, (8 + R) * sizeof(uint32_t), s);
        if (rc == hipSuccess)
            rc = LaunchHttpGroup(B, ht, sel_h, cnt ? cnt + kCntHttp : nullptr, n, !partitioned, ctl, hist, cursor, segs,
                                 gsel, gbig, s);
        if (rc == hipSuccess) rc = LaunchHttpGrouped(B, ht, gsel, segs, gbig, ctl, e->any_big_image, s);
    } else if (rc == hipSuccess && run[1]) {
        rc = LaunchHttpClassify(B, ht, sel_h, cnt ? cnt + kCntHttp : nullptr, any_cold, !partitioned, tile_ctr,
                                n <= kLatencyMax, fuse_http, s);
    }
    mark(2);
    // a large partitioned batch with both Kafka and memcached requests: the
    // memcached kernel runs on a side stream beside the Kafka kernel, which leaves
    // one workgroup slot per CU for it (cfg5: 37.31 -> 36.44 ms per step,
    // profiles/r6/ab6h_kafka_memcached_beside.txt)
    const bool km = partitioned && run[2] && run[3] && !prof && big_lanes == 0 && n >= kBesideMin && !pre;
    const int kafka_leave = km ? 1 : 0;
    hipStream_t ms = s;
    if (km && rc == hipSuccess) {
        if (!S->side) {
            rc = hipStreamCreateWithFlags(&S->side, hipStreamNonBlocking);
            if (rc == hipSuccess) rc = hipEventCreateWithFlags(&S->fork_ev, hipEventDisableTiming);
            if (rc == hipSuccess) rc = hipEventCreateWithFlags(&S->join_ev, hipEventDisableTiming);
        }
        if (rc == hipSuccess) rc = hipEventRecord(S->fork_ev, s);
        if (rc == hipSuccess) rc = hipStreamWaitEvent(S->side, S->fork_ev, 0);
        if (rc == hipSuccess) ms = S->side;
    }
    uint32_t *zcount = cnt ? cnt + kCntKafkaZ : nullptr;
    if (rc == hipSuccess && run[2])
        rc = LaunchKafkaClassify(B, e->kt, sel_k, cnt, !partitioned, sel_z, zcount, cnt ? cnt + kCntKafkaWork : nullptr,
                                 s, kafka_leave, false, log);
    // requests with gzip / snappy messages: decoded, their sets read, failures answered
    auto inflate = [&]() {
        if (rc != hipSuccess || !run[2] || !sel_z) return;
        // the engine's one decode region: after the previous inflate launch on any stream
        if (e->zreg_used) rc = hipStreamWaitEvent(s, e->zreg_ev, 0);
        if (rc == hipSuccess) rc = LaunchKafkaInflate(B, sel_z, zcount, e->d_zreg, s);
        if (rc == hipSuccess) rc = hipEventRecord(e->zreg_ev, s);
        if (rc == hipSuccess) e->zreg_used = true;
    };
    if (ms == s) inflate();
    mark(3);
    if (rc == hipSuccess && run[3])
        rc = LaunchMemcacheClassify(B, mt, sel_m, sel_h, cnt ? cnt + kCntMc : nullptr, !partitioned, big_lanes, ms,
                                    fuse_mc, kafka_leave, km ? cnt + kCntMcWork : nullptr);
    if (ms != s && rc == hipSuccess) {
        // the memcached kernel, at its raised priority, is done well before the
        // Kafka grid: a small second Kafka grid behind it on the side stream takes
        // over the slots it ran in and draws from the same work counter; it also
        // appends to the compressed-request list, so the inflate launch follows the join
        // (cfg5: 33.46 -> 33.10 ms per step, profiles/beside_leg/ab_variants_visit2.txt)
        if (L7G_KAFKA_HELPER)
            rc = LaunchKafkaClassify(B, e->kt, sel_k, cnt, !partitioned, sel_z, zcount, cnt + kCntKafkaWork, ms,
                                     kafka_leave, true, log);
        if (rc == hipSuccess) rc = hipEventRecord(S->join_ev, ms);
        if (rc == hipSuccess) rc = hipStreamWaitEvent(s, S->join_ev, 0);
        inflate();
    }
    // r2d2 (proxylib's example line protocol): one lane per request over the whole batch
    if (rc == hipSuccess && run_r2) rc = LaunchR2d2Classify(B, rt, !partitioned, big_lanes, s);
    // every parser's access-log records: the HTTP post-pass here, where the HTTP
    // verdicts are final, so that the generic one (which overwrites the kind 0
    // it gives the other protocols' requests) can run before a session commit
    if (rc == hipSuccess && text) rc = LaunchHttpLog(B, log->rec, s);
    // cassandra (proxylib): the batch's USE requests, then one lane per request
    // (with sessions on: against the session tables, then the batch's USE and PREPARE requests committed)
    bool generic_logged = false;
    if (rc == hipSuccess && run_cs) {
        const bool sessions = e->sess.by_id != nullptr;
        const size_t need = CassandraScratchBytes(n, sessions);
        if (need == 0) rc = hipErrorInvalidValue;
        if (rc == hipSuccess) rc = S->Grow(&S->d_use, &S->use_cap, need, need);
        if (rc == hipSuccess && sessions && text) {
            rc = LaunchCassandraSessionClassifyLogged(B, ct, e->sess, S->d_use, S->use_cap, !partitioned, big_lanes, *log,
                                                      *text, s);
            generic_logged = true;
        } else if (rc == hipSuccess && sessions) {
            rc = LaunchCassandraSessionClassify(B, ct, e->sess, S->d_use, S->use_cap, !partitioned, big_lanes, s);
        } else if (rc == hipSuccess) {
            rc = LaunchCassandraClassify(B, ct, S->d_use, S->use_cap, !partitioned, big_lanes, s);
        }
    }
    mark(4);
    // access-log records: every request's but Kafka's (written above), from the verdicts
    if (rc == hipSuccess && log && !text) rc = LaunchHttpLog(B, log->rec, s);
    if (rc == hipSuccess && text && !generic_logged)
        rc = LaunchGenericLog(B, *log, *text, ct, run_cs ? CassandraSortedUseKeys(S->d_use, n) : nullptr, CassSessions{},
                              s);
    // proxy statistics (accumulated on the device until read)
    if (rc == hipSuccess && e->flow_stats && !e->skey_list.empty()) {
        const size_t nk = e->skey_list.size();
        if (nk > e->flow_cap) {  // grow, keeping what was accumulated
            uint64_t *d = nullptr;
            // every stream's earlier flowstats kernels may still add into the old
            // accumulator: they finish before it is copied (e->mu is held, so no
            // new launch can race with the copy)
            if (e->d_flow) rc = WaitLastClassify(e);
            if (rc == hipSuccess) rc = hipMalloc(&d, nk * 4 * sizeof(uint64_t));
            if (rc == hipSuccess) rc = hipMemsetAsync(d, 0, nk * 4 * sizeof(uint64_t), s);
            if (rc == hipSuccess && e->d_flow)
                rc = hipMemcpyAsync(d, e->d_flow, e->flow_cap * 4 * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
            if (rc == hipSuccess) {
                if (e->d_flow) {
                    hipStreamSynchronize(s);
                    hipFree(e->d_flow);
                }
                e->d_flow = d;
                e->flow_cap = nk;
            }
        }
        if (rc == hipSuccess) rc = LaunchFlowStats(B, (uint32_t)nk, e->d_flow, s);
    }
    // per-rule allow hits and per-verdict totals, from the outputs
    if (rc == hipSuccess && counters) {
        if (!S->d_hist) rc = hipMalloc(&S->d_hist, CountersScratchBytes());
        if (rc == hipSuccess)
            rc = LaunchCounters(out.verdict, out.rule, n, (uint32_t)e->ps->nrules, counters, S->d_hist, s);
    }
    return (int)CallEnd(S, s, rc);
}

// l7g_deny_replies: the post-pass over a classified batch, on the caller's
// stream with that stream's reply scratch.  Nothing of l7g_classify's plan is
// involved: the kernels read the verdicts and the connection table.
int DenyReplies(l7g_engine *e, const DevIn &in, const uint8_t *verdict, const l7g_reply_out_t *out, void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (!out || !out->off || !out->len || !out->total || (!out->buf && out->cap)) return (int)hipErrorInvalidValue;
    if (in.n && (!in.off || !in.len || !in.conn || !verdict)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    StreamScratch *S = nullptr;
    hipError_t rc = CallBegin(e, kSyncNone, s, &S);  // (the connection table the kernels read)
    if (rc != hipSuccess) return (int)rc;
    const size_t need = DenyRepliesScratchBytes(in.n);
    if (need == 0) return (int)hipErrorInvalidValue;
    if ((rc = S->Grow(&S->d_reply, &S->reply_cap, need, need)) != hipSuccess) return (int)rc;
    const Batch B{in.arena, in.arena_len, in.off, in.len, in.conn, e->d_conns, const_cast<uint8_t *>(verdict), nullptr,
                  nullptr, in.n, (uint32_t)e->conns.size()};
    rc = LaunchDenyReplies(B, out->buf, out->cap, out->off, out->len, out->total, S->d_reply, S->reply_cap, s);
    return (int)CallEnd(S, s, rc);
}

extern "C" {

int l7g_deny_replies(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                     const uint32_t *conn, uint32_t n, const uint8_t *verdict, const l7g_reply_out_t *out,
                     void *stream) {
    return DenyReplies(e, {arena, arena_len, off, len, conn, n}, verdict, out, stream);
}

const uint8_t *l7g_deny_reply_template(int proto, size_t *len) {
    const uint8_t *p = nullptr;
    size_t n = 0;
    if (proto == L7G_PROTO_HTTP) { p = reinterpret_cast<const uint8_t *>(kDenied403); n = kDenied403Len; }
    if (proto == L7G_PROTO_CASSANDRA) { p = kCassUnauth; n = kCassUnauthLen; }
    if (proto == L7G_PROTO_R2D2) { p = reinterpret_cast<const uint8_t *>(kR2Error); n = kR2ErrorLen; }
    if (len) *len = n;
    return p;
}

int l7g_classify(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                 const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule, uint32_t *consumed,
                 uint64_t *counters, void *stream) {
    return Classify(e, {arena, arena_len, off, len, conn, n}, {verdict, rule, consumed, counters}, stream);
}

int l7g_classify_logged(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                        const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                        uint32_t *consumed, uint64_t *counters, const l7g_log_out_t *log, void *stream) {
    if (!log) return (int)hipErrorInvalidValue;
    const LogOut lo{reinterpret_cast<LogRec *>(log->rec), reinterpret_cast<LogSpan *>(log->topics), log->topic_stride};
    ClassifyOpts o;
    o.log = &lo;
    return Classify(e, {arena, arena_len, off, len, conn, n}, {verdict, rule, consumed, counters}, stream, o);
}

int l7g_classify_logged_all(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                            const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                            uint32_t *consumed, uint64_t *counters, const l7g_log_all_out_t *log, void *stream) {
    if (!log) return (int)hipErrorInvalidValue;
    const LogOut lo{reinterpret_cast<LogRec *>(log->rec), reinterpret_cast<LogSpan *>(log->spans), log->span_stride};
    const LogText tx{log->text, log->text_stride};
    ClassifyOpts o;
    o.log = &lo;
    o.text = &tx;
    return Classify(e, {arena, arena_len, off, len, conn, n}, {verdict, rule, consumed, counters}, stream, o);
}

int l7g_frame_streams(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                      const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_frames,
                      uint64_t *frame_off, uint32_t *frame_len, uint32_t *frame_conn, uint32_t *nframes, void *stream) {
    std::lock_guard<std::mutex> g(e->mu);
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (max_frames == 0 || (uint64_t)n * max_frames > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
    hipError_t rc = hipSetDevice(e->device);
    if (rc == hipSuccess) rc = Upload(e);  // (the connection table the walk reads)
    if (rc == hipSuccess)
        rc = LaunchFrameStreams(arena, arena_len, s_off, s_len, s_conn, n, e->d_conns, (uint32_t)e->conns.size(),
                                max_frames, frame_off, frame_len, frame_conn, nframes, (hipStream_t)stream);
    return (int)rc;
}

int l7g_classify_streams(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                         const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_frames,
                         uint64_t *frame_off, uint32_t *frame_len, uint32_t *frame_conn, uint32_t *nframes,
                         uint8_t *verdict, int32_t *rule, uint32_t *consumed, uint64_t *counters, void *stream) {
    int rc = l7g_frame_streams(e, arena, arena_len, s_off, s_len, s_conn, n, max_frames, frame_off, frame_len,
                               frame_conn, nframes, stream);
    if (rc != 0) return rc;
    // every slot, the empty ones on connection ~0 (answered UNSUPPORTED)
    return Classify(e, {arena, arena_len, frame_off, frame_len, frame_conn, n * max_frames},
                    {verdict, rule, consumed, counters}, stream);
}

}  // extern "C"

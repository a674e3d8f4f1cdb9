// Host entry points of the kernels (product code): every launcher, scratch
// size and phase-time reader the C-ABI's host files call.  The .hip file that
// defines one includes this header too, so the compiler checks the two.
#pragma once
#include <hip/hip_runtime_api.h>

#include "../device_tables.h"
#include "copy_in_types.h"
#include "service_types.h"

namespace l7 {

// The current device's CU count (classify.cc), for the persistent grids: asked once per process, 256
// when the runtime does not say.
int DeviceCuCount();
// sel (here, LaunchHttpGroup, LaunchMemcacheClassify): entry lists (ListEnt, device_tables.h)
hipError_t LaunchHttpClassify(const Batch &B, const HttpTables &T, const ListEnt *sel, const uint32_t *sel_count,
                              bool any_cold, bool answer_other, uint32_t *tile_ctr, bool latency, const CopyIn *ci,
                              hipStream_t stream);
hipError_t LaunchKafkaClassify(const Batch &B, const KafkaTables &T, const uint32_t *sel, const uint32_t *sel_count,
                               bool answer_other, uint32_t *zlist, uint32_t *zcount, uint32_t *work,
                               hipStream_t stream, int leave_per_cu = 0, bool helper = false,
                               const LogOut *log = nullptr);
// the logged calls' post-pass (kernels/http_log.hip): the records of every request but Kafka's
hipError_t LaunchHttpLog(const Batch &B, LogRec *rec, hipStream_t stream);
// l7g_deny_replies (kernels/deny_reply.hip): the replies of the requests whose verdict is DENY, packed
// in request order (B.verdict is read; B.rule and B.consumed are not used)
size_t DenyRepliesScratchBytes(uint32_t n);
hipError_t LaunchDenyReplies(const Batch &B, uint8_t *buf, uint64_t cap, uint64_t *roff, uint32_t *rlen,
                             uint64_t *total, void *scratch, size_t scratch_bytes, hipStream_t stream);
hipError_t LaunchKafkaInflate(const Batch &B, const uint32_t *zlist, const uint32_t *zcount, uint8_t *region,
                              hipStream_t stream);
uint32_t KafkaInflateBlocks();
uint32_t KafkaInflateRegionBytes();
hipError_t LaunchMemcacheClassify(const Batch &B, const McTables &T, const ListEnt *sel, const ListEnt *sel2,
                                  const uint32_t *sel_count, bool answer_other, uint32_t scratch_lanes,
                                  hipStream_t stream, const CopyIn *ci = nullptr, int beside_slots = 0,
                                  uint32_t *work = nullptr);
hipError_t LaunchR2d2Classify(const Batch &B, const R2Tables &T, bool answer_other, uint32_t scratch_lanes,
                              hipStream_t stream);
size_t CassandraScratchBytes(uint32_t n, bool sessions = false);
hipError_t LaunchCassandraClassify(const Batch &B, const CassTables &T, void *scratch, size_t scratch_bytes,
                                   bool answer_other, uint32_t nfa_lanes, hipStream_t stream);
// cassandra sessions (kernels/cassandra_session.hip): classify against the session tables and commit the batch
hipError_t LaunchCassandraSessionClassify(const Batch &B, const CassTables &T, const CassSessions &SS, void *scratch,
                                          size_t scratch_bytes, bool answer_other, uint32_t nfa_lanes,
                                          hipStream_t stream);
// l7g_classify_logged_all (kernels/generic_log.hip): the records of memcached, r2d2 and cassandra requests,
// after LaunchHttpLog; use_keys: CassandraSortedUseKeys of this call's cassandra scratch (null: no cassandra
// classifier ran); with sessions the launch is made by LaunchCassandraSessionClassifyLogged, before the commit
hipError_t LaunchGenericLog(const Batch &B, const LogOut &L, const LogText &X, const CassTables &T,
                            const uint64_t *use_keys, const CassSessions &SS, hipStream_t stream);
hipError_t LaunchCassandraSessionClassifyLogged(const Batch &B, const CassTables &T, const CassSessions &SS,
                                                void *scratch, size_t scratch_bytes, bool answer_other,
                                                uint32_t nfa_lanes, const LogOut &L, const LogText &X,
                                                hipStream_t stream);
const uint64_t *CassandraSortedUseKeys(const void *scratch, uint32_t n);
hipError_t LaunchCassandraCommit(const Batch &B, const CassTables &T, const CassSessions &S,
                                 const uint64_t *use_sorted, const uint64_t *prep_sorted, hipStream_t stream);
hipError_t LaunchCassandraReplies(const Batch &B, const CassSessions &S, void *scratch, size_t scratch_bytes,
                                  hipStream_t stream);
hipError_t LaunchCassandraSessionReset(const CassSessions &S, const uint32_t *conn, uint32_t n, hipStream_t stream);
hipError_t LaunchCassandraSessionLive(const CassSessions &S, unsigned long long *out2, hipStream_t stream);
// Kafka sessions (kernels/kafka_session.hip): l7g_kafka_forward, l7g_kafka_responses and the table's upkeep;
// scratch: the ...ScratchBytes of the call (0: the batch is too large), 256-byte aligned
size_t KafkaSessForwardScratchBytes(uint32_t n, uint32_t nconns);
hipError_t LaunchKafkaSessForward(const KafkaSessBatch &B, const KafkaSessions &S, const uint8_t *verdict,
                                  const uint64_t *tag, uint64_t now_ms, uint8_t *fwd, uint32_t *new_id, void *scratch,
                                  size_t scratch_bytes, hipStream_t stream);
size_t KafkaSessResponsesScratchBytes(uint32_t n);
hipError_t LaunchKafkaSessResponses(const KafkaSessBatch &B, const KafkaSessions &S, uint8_t *found, uint32_t *orig_id,
                                    int16_t *api_key, int16_t *api_version, uint64_t *tag, void *scratch,
                                    size_t scratch_bytes, hipStream_t stream);
// S.spare zeroed by the caller, who swaps the tables afterwards; *expired is added to
hipError_t LaunchKafkaSessGc(const KafkaSessions &S, uint64_t now_ms, uint64_t lifetime_ms, unsigned long long *expired,
                             hipStream_t stream);
hipError_t LaunchKafkaSessReset(const KafkaSessions &S, const uint32_t *conn, uint32_t n, hipStream_t stream);
hipError_t LaunchKafkaSessLive(const KafkaSessions &S, unsigned long long *out2, hipStream_t stream);
// memcached sessions (kernels/memcached_session.hip): l7g_mc_forward, l7g_mc_replies and the slots' upkeep;
// scratch: McSessForwardScratchBytes of the call (0: the batch is too large), 256-byte aligned
size_t McSessForwardScratchBytes(uint32_t n, uint32_t nconns);
hipError_t LaunchMcSessForward(const McSessBatch &B, const McSessions &S, const uint8_t *verdict, const uint64_t *tag,
                               uint8_t *act, void *scratch, size_t scratch_bytes, hipStream_t stream);
hipError_t LaunchMcSessReplies(const McSessBatch &B, const McSessions &S, const McReplyOut &O, hipStream_t stream);
hipError_t LaunchMcSessReset(const McSessions &S, const uint32_t *conn, uint32_t n, hipStream_t stream);
hipError_t LaunchMcSessLive(const McSessions &S, unsigned long long *out2, hipStream_t stream);
hipError_t LaunchCounters(const uint8_t *verdict, const int32_t *rule, uint32_t n, uint32_t nrules,
                          uint64_t *counters, uint32_t *scratch, hipStream_t stream);
size_t CountersScratchBytes();
hipError_t LaunchFlowStats(const Batch &B, uint32_t nkeys, uint64_t *acc, hipStream_t stream);
uint32_t FlowStatsMaxKeys();
hipError_t LaunchHttpNfa(const Batch &B, const HttpTables &T, uint32_t scratch_lanes, hipStream_t stream);
hipError_t LaunchPartition(const Batch &B, uint32_t *sel_kafka, ListEnt *ent_mc, ListEnt *ent_http, uint32_t *counts,
                           hipStream_t stream);
hipError_t LaunchFrameStreams(const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off, const uint32_t *s_len,
                              const uint32_t *s_conn, uint32_t n, const DevConn *conns, uint32_t nconns,
                              uint32_t max_frames, uint64_t *frame_off, uint32_t *frame_len, uint32_t *conn_out,
                              uint32_t *nframes, hipStream_t stream);
hipError_t HttpPhaseTimes(uint64_t *out, bool reset);
hipError_t KafkaPhaseTimes(uint64_t *out, bool reset);
hipError_t LaunchCopyIn(const CopyIn &c, hipStream_t stream);
hipError_t FramePhaseTimes(uint64_t *out, bool reset);
hipError_t LaunchHttpGroup(const Batch &B, const HttpTables &T, const ListEnt *sel, const uint32_t *sel_count,
                           uint32_t n, bool answer_other, uint32_t *ctl, uint32_t *hist, uint32_t *cursor,
                           uint32_t *segs, uint32_t *gsel, ListEnt *gbig, hipStream_t stream);
hipError_t LaunchHttpGrouped(const Batch &B, const HttpTables &T, const uint32_t *gsel, const uint32_t *segs,
                             const ListEnt *gbig, uint32_t *ctl, bool any_big, hipStream_t stream);
hipError_t LaunchHttpService(SvcBox *box, const SvcStatic &S, const HttpTables &T, uint32_t seen0, uint64_t idle,
                             hipStream_t stream);
hipError_t LaunchMemcacheService(SvcBox *box, const SvcStatic &S, const McTables &T, uint32_t seen0, uint64_t idle,
                                 hipStream_t stream);

}  // namespace l7

/*
 * l7gpu.h — C-ABI of the MI355X-native batched L7 policy classifier.
 *
 * This is the drop-in boundary for the reference's L7 verdict path.  Every
 * entry point is plain C (pointers + sizes, no C++/torch types) so a Go cgo
 * package, Envoy's dlopen loader, or ctypes can bind it.  What each entry
 * replaces in the reference (file:line):
 *
 *   l7g_policy_update   proxylib Instance.PolicyUpdate            proxylib/proxylib/instance.go:168-219
 *                       Envoy NetworkPolicyMap::onConfigUpdate     envoy/cilium_network_policy.h:240-250
 *                       (policies in the cilium.NetworkPolicy shape, envoy/cilium/npds.proto:31-182,
 *                        as JSON; see DESIGN.md §Policy JSON)
 *   l7g_policy_index    NetworkPolicyMap::GetPolicyInstance        envoy/cilium_network_policy.h:213-221
 *   l7g_conns_set,      proxylib OnNewConnection / Close           proxylib/proxylib.go:57-74,112-116
 *   l7g_conn_update
 *                       Cilium::SocketOption (identity, port, dir) envoy/cilium_l7policy.cc:133-150
 *   l7g_classify        per request: AccessFilter::decodeHeaders -> NetworkPolicyMap::Allowed
 *                                                                  envoy/cilium_l7policy.cc:127-182,
 *                                                                  envoy/cilium_network_policy.h:223-237
 *                       kafka.ReadRequest + canAccess/MatchesRule  pkg/kafka/request.go:186-229,
 *                                                                  pkg/proxy/kafka.go:117-153,
 *                                                                  pkg/kafka/policy.go:200-225
 *                       proxylib OnData (memcache parser) -> Connection.Matches
 *                                                                  proxylib/proxylib.go:97-110,
 *                                                                  proxylib/memcached/parser.go:186-202,
 *                                                                  proxylib/proxylib/policymap.go:210-236
 *   l7g_frame_streams   the parsers' framing of a connection's input: proto.ReadReq's size prefix
 *                                                                  vendor/github.com/optiopay/kafka/proto/messages.go:124-165,
 *                       memcached text line / binary header        proxylib/memcached/text/parser.go:72-262,
 *                                                                  proxylib/memcached/binary/parser.go:72-139
 *   l7g_deny_replies    what is sent back for a DENY: req.CreateResponse(ErrTopicAuthorizationFailed)
 *                                                                  pkg/proxy/kafka.go:249-261,
 *                                                                  pkg/kafka/response.go:81-315,
 *                       Envoy's 403 local reply                    envoy/cilium_l7policy.cc:90-96,171-177,
 *                       the cassandra / r2d2 parsers' injected errors
 *                                                                  proxylib/cassandra/cassandraparser.go:269-278
 *   l7g_mc_forward,     the memcached parsers' reply bookkeeping: the text reply queue,
 *   l7g_mc_replies      the binary inject queue, reply framing        proxylib/memcached/text/parser.go:173-331,
 *                                                                  proxylib/memcached/binary/parser.go:58-165,
 *                       under the connection's op loop             proxylib/proxylib/connection.go:118-174
 *   counters argument   Endpoint.UpdateProxyStatistics counters    pkg/endpoint/endpoint.go:2207-2233
 *   of l7g_classify     (per-rule allow hits + per-verdict totals, accumulated on the device)
 *
 * Verdict codes match the oracle (oracle/l7ref.h) and DESIGN.md.
 */
#ifndef L7GPU_H
#define L7GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct l7g_engine l7g_engine;

enum { L7G_PROTO_HTTP = 1, L7G_PROTO_KAFKA = 2, L7G_PROTO_MEMCACHE = 3, L7G_PROTO_R2D2 = 4, L7G_PROTO_CASSANDRA = 5 };
/* L7G_PROTO_CASSANDRA has two modes.
 * Stateless (the default): nothing is kept between l7g_classify calls.  A
 * request's keyspace comes only from the last USE on its connection earlier in
 * the same batch (a USE from an earlier batch is not remembered, so "t" stays
 * ".t" rather than "ks.t"), and an EXECUTE is never resolved to its prepared
 * query (answered L7G_PARSE_ERROR, consumed 2).  The proxylib shim keeps both
 * per connection on the host and replays them into each batch.
 * Sessions (l7g_cass_sessions_enable, below): the engine keeps what
 * cassandraparser.go keeps per connection -- the keyspace of the last USE, the
 * statements PREPAREd by stream id, and their binding to prepared ids by the
 * RESULT/prepared replies given to l7g_cass_replies -- in device memory, and
 * l7g_classify / l7g_classify_host give the reference's answers across
 * batches, EXECUTE included, with no host pass over the bytes. */
enum {
    L7G_DENY = 0,        /* policy denies (HTTP 403 / Kafka ErrTopicAuthorizationFailed) */
    L7G_ALLOW = 1,       /* policy allows; rule = matched global rule id or -1 */
    L7G_PARSE_ERROR = 2, /* malformed request (connection is closed by the caller) */
    L7G_INCOMPLETE = 3,  /* more bytes are needed (proxylib MORE) */
    L7G_UNSUPPORTED = 4, /* no parser for the connection, a request outside the arena, a nested compressed
                            Kafka set beyond the decode space (kafka_inflate.hip) */
};

/* memcached: proxylib picks the text or binary parser from the first byte a
 * connection carries and keeps it (proxylib/memcached/parser.go:186-202).
 * L7G_CONN_PROXYLIB: an HTTP or Kafka connection served by the proxylib
 * "http" / "kafka" parser: proxylib's policymap semantics apply (no port entry
 * => DENY, SrcId is the remote in both directions; policymap.go:208-236,
 * connection.go:176-179) instead of Envoy's / the in-agent Kafka proxy's. */
enum { L7G_CONN_MC_TEXT = 1, L7G_CONN_MC_BINARY = 2, L7G_CONN_PROXYLIB = 4 };

/* Connection attributes (20 bytes; identical layout to the oracle's ref_conn_t). */
typedef struct {
    int32_t policy;   /* l7g_policy_index(name), -1 = no policy for this endpoint (deny) */
    uint32_t port;    /* destination port */
    uint8_t ingress;  /* 1 = ingress */
    uint8_t proto;    /* L7G_PROTO_* */
    uint16_t flags;   /* L7G_CONN_MC_*: memcached parser chosen for the connection (0 = by first byte) */
    uint32_t src_id;  /* source security identity */
    uint32_t dst_id;  /* destination security identity */
} l7g_conn_t;

typedef struct {
    uint32_t policies, rules, http_rulesets, http_chunks, http_dfas, http_dfa_states;
    uint32_t kafka_rulesets, kafka_rules, kafka_topics;
    uint64_t table_bytes;       /* device table blob (0 until first upload) */
    uint64_t http_image_bytes;  /* all HTTP rule-set images */
    int32_t hot_ruleset;        /* HTTP rule set staged in LDS, -1 none */
    uint32_t hot_image_bytes;
    uint32_t mc_rulesets, mc_rules, mc_dfas, mc_dfa_states;
    uint32_t http_nfas;         /* distinct patterns on the bit-parallel NFA fallback */
    uint32_t mc_nfas;
    uint64_t nfa_pool_bytes;    /* their device tables */
    uint32_t r2d2_rulesets, r2d2_rules;
} l7g_stats_t;

/* Engine bound to one HIP device.  err receives a message on failure.
 * device == L7G_HOST_ONLY creates a compile-only engine (policy validation and
 * rule-table statistics; classification returns hipErrorNoDevice).
 * Environment, read here: L7G_SERVICE=0 (resident services off, below);
 * L7G_KAFKA_DENSE_BUDGET=<u32 words> (tests: the Kafka compiler's budget for
 * dense per-topic tables; 0 keeps every rule set to its sorted directory). */
#define L7G_HOST_ONLY (-1)
l7g_engine *l7g_engine_create(int device, char *err, size_t errlen);
void l7g_engine_destroy(l7g_engine *e);

/* Atomically replaces the policy set (0 = ok).  On error the previous policy
 * set stays in force (like an NPDS NACK).  Existing connections are re-resolved. */
int l7g_policy_update(l7g_engine *e, const char *json, size_t len, char *err, size_t errlen);
/* The same policy delivery as the NPDS stream carries it: buf is a serialized
 * envoy.api.v2.DiscoveryResponse whose resources are google.protobuf.Any of
 * type.googleapis.com/cilium.NetworkPolicy (envoy/cilium/npds.proto:31-182),
 * decoded by the library's own proto3 wire-format reader.  Same atomic swap and
 * NACK as l7g_policy_update; a response the JSON path would express the same
 * way compiles to identical tables. */
int l7g_policy_update_proto(l7g_engine *e, const uint8_t *buf, size_t len, char *err, size_t errlen);
int32_t l7g_policy_index(l7g_engine *e, const char *name, size_t len);
int32_t l7g_policy_nrules(l7g_engine *e);

/* Compiled tables across GPUs (the NPDS receiver is rank 0,
 * proxylib/proxylib/instance.go:168-219): one rank compiles, the others install.
 * l7g_tables_export writes the current policy version -- its source bytes and
 * every compiler's rule sets (device images plus the rule-list -> rule-set
 * cache) -- into buf; *len = the bytes needed.  Returns 0, or -2 when buf is
 * NULL or cap is too small (only *len is set).  l7g_tables_import installs such
 * an image: the policy is parsed, not compiled, and the connections are
 * re-resolved against the imported rule sets (one the exporter did not compile
 * is compiled here).  Same atomic swap / NACK as l7g_policy_update. */
int l7g_tables_export(l7g_engine *e, uint8_t *buf, size_t cap, size_t *len);
int l7g_tables_import(l7g_engine *e, const uint8_t *buf, size_t len, char *err, size_t errlen);
/* Rule sets this engine compiled itself since its policy version was installed
 * (0 on a rank that imported every rule set it uses). */
uint64_t l7g_tables_compiled(l7g_engine *e);
/* FNV-1a 64 of the device table blob the engine installs (equal digests <=>
 * byte-identical tables). */
uint64_t l7g_tables_digest(l7g_engine *e);

/* Replaces the connection table (connection i = conns[i]); compiles the rule
 * sets the connections need.  0 = ok. */
int l7g_conns_set(l7g_engine *e, const l7g_conn_t *conns, uint32_t n, char *err, size_t errlen);

/* Sets (or adds, growing the table) connection `index` alone; rule sets are
 * compiled on first use.  The proxylib shim calls it from OnNewConnection /
 * Close and when a memcached connection's parser is chosen.  0 = ok. */
int l7g_conn_update(l7g_engine *e, uint32_t index, const l7g_conn_t *conn, char *err, size_t errlen);

/* Classifies n requests resident in device memory: request i is
 * arena[off[i] .. off[i]+len[i]) on connection conn[i], inside
 * [arena, arena + arena_len) (an HTTP request reaching past it is answered
 * UNSUPPORTED).  The arena must stay readable up to the next 16-byte boundary
 * past its last byte (true of every hipMalloc / torch allocation); the kernels
 * read aligned 16-byte words.  Writes verdict[i],
 * rule[i] (global rule id, -1 = none) and consumed[i]: for ALLOW/DENY the
 * bytes of the first request (proxylib's PASS/DROP length, which may exceed
 * len[i] for memcached data blocks); for memcached INCOMPLETE the proxylib
 * MORE byte count (0 = NOP) and for memcached PARSE_ERROR the OpError code
 * (2 = INVALID_FRAME_TYPE; 0 = parser error); 0 otherwise.  Asynchronous on `stream`
 * (a hipStream_t, NULL = default stream).  counters may be NULL, else a
 * device array of (rules + 8) uint64 that accumulates per-rule allow hits
 * followed by per-verdict totals (added atomically, so calls on different
 * streams may share one array).  Batches with Kafka requests or with more
 * than one protocol use a scratch of 32 + (L7_KAFKA_CLASSES + 3) n uint32 (the
 * partition lists and work counters; 32 + 11 n with 8 classes), HTTP-only
 * batches of 2^18 or more requests 4 words (tile counters); scratch is kept per stream (up to
 * 16 streams, then handed over least recently used first), so calls on
 * different streams run concurrently and calls on one stream are ordered by
 * it.  With Kafka rules the engine also holds ONE 1 GiB decode region for
 * compressed message sets, allocated with the first Kafka batch and shared by
 * all streams: the decode kernels of calls on different streams run one after
 * the other (each waits for the previous one's completion event).  Returns 0
 * or a HIP error code. */
int l7g_classify(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                 const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule, uint32_t *consumed,
                 uint64_t *counters, void *stream);

/* Device framing of connection streams (replaces the host scan that proposes
 * where a connection's frames start: Kafka's BE int32 size prefix,
 * proto.ReadReq vendor/github.com/optiopay/kafka/proto/messages.go:124-165;
 * memcached text lines + storage data blocks and binary 24-byte header + body,
 * proxylib/memcached/{text,binary}/parser.go; HTTP/1 head + Content-Length;
 * r2d2 lines; cassandra 9-byte header + body).  Stream s is arena[s_off[s],
 * s_off[s] + s_len[s]) on connection s_conn[s] (a memcached connection without
 * a chosen parser takes the one the stream's first byte picks).  One device
 * lane walks each stream; output slots [s * max_frames, (s + 1) * max_frames):
 * frame k of stream s starts at frame_off (an arena offset) and is handed
 * frame_len = the bytes from there to the stream's end, as proxylib hands a
 * parser the joined input; frame_conn = s_conn[s]; nframes[s] frames.  The
 * walk stops at a frame whose end is not in the stream or cannot be known
 * before parsing it (a chunked HTTP body, an unreadable size): that frame is
 * the last, with the rest of the stream, and the classifier's consumed length
 * says where the next one starts.  Empty slots: length 0, connection ~0.  All
 * pointers are device memory; asynchronous on `stream`.  0 or a hipError_t. */
int l7g_frame_streams(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                      const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_frames,
                      uint64_t *frame_off, uint32_t *frame_len, uint32_t *frame_conn, uint32_t *nframes, void *stream);
/* l7g_frame_streams, then l7g_classify over all n * max_frames slots (the
 * empty ones answer L7G_UNSUPPORTED): a batch of connection streams in, one
 * verdict per frame out, with no host pass over the bytes.  A frame is
 * confirmed when its consumed length equals the distance to the next frame
 * (or, for the last, when the caller accepts a partial one). */
int l7g_classify_streams(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                         const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_frames,
                         uint64_t *frame_off, uint32_t *frame_len, uint32_t *frame_conn, uint32_t *nframes,
                         uint8_t *verdict, int32_t *rule, uint32_t *consumed, uint64_t *counters, void *stream);

/* Same with host buffers: copies in, classifies, copies out, synchronises.
 * Each calling thread gets its own stream and device staging, so calls from
 * several threads overlap (the engine lock covers only the enqueue). */
int l7g_classify_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                      const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                      uint32_t *consumed);

int l7g_stats(l7g_engine *e, l7g_stats_t *out);

/* Access-log records (opt-in; l7g_classify and l7g_classify_host are untouched
 * by it).  The logged calls classify exactly as the plain ones -- the same
 * launch plan, verdict / rule / consumed / counters, streams and scratch -- and
 * also write one fixed-size record per request with the fields the reference's
 * log entries carry: Envoy's HttpLogEntry (envoy/accesslog.cc:59-133,
 * InitFromRequest: method, path, host, protocol) and the Kafka proxy's
 * LogRecordKafka, one per topic (pkg/proxy/kafka.go:169-231,
 * pkg/proxy/accesslog/record.go:203-245: API key, version, correlation id,
 * topic).
 *
 * rec[i] means something only where verdict[i] is L7G_ALLOW or L7G_DENY; the
 * verdict array is the authority (a compressed Kafka request can still turn
 * L7G_PARSE_ERROR after its record was written).  Everywhere else kind and the
 * rest of rec[i] are unspecified.  Requests on memcached, r2d2 and cassandra
 * connections get kind 0.
 *
 * HTTP (kind 1): the method is request bytes [0, method_len), the path
 * [method_len + 1, method_len + 1 + path_len); host_off / host_len the value
 * of the first Host header (name matched without case, optional whitespace
 * trimmed; flags bit0 = such a header is present, its length 0 for an empty
 * value); head_len the offset just past the empty line; nheaders the number of
 * header lines (the caller reads them from [0, head_len)); api_key the
 * protocol version, (major digit << 4) | minor digit of "HTTP/x.y".
 *
 * Kafka (kind 2): api_key, api_version and correlation_id are the big-endian
 * fields at request bytes 4, 6 and 8 (GetAPIKey, GetVersion,
 * GetCorrelationID); ntopics the length of GetTopics()
 * (pkg/kafka/request.go:88-153: every topic in wire order, duplicates kept; 0
 * for an untyped request, ConsumerMetadata and a null Metadata / OffsetFetch
 * array).  topics is n rows of topic_stride spans: row i receives the spans
 * (from the request's first byte; an empty name is {0, 0}) of the first
 * min(ntopics, topic_stride) topic names; rows of requests that are not Kafka
 * are never written.  A request with more topics than the stride sets flags
 * bit0: submit it again, alone, with a stride of its ntopics.  topic_stride 0
 * with topics NULL is valid.
 *
 * rec and topics are device memory for l7g_classify_logged (rec 16-byte
 * aligned) and host memory for l7g_classify_logged_host, which always launches
 * (it does not post to a resident service) and gives l7g_classify_host's
 * verdicts. */
typedef struct { uint32_t off, len; } l7g_span_t; /* bytes from the request's first byte */
enum { L7G_LOG_NONE = 0, L7G_LOG_HTTP = 1, L7G_LOG_KAFKA = 2 };
typedef struct {
    uint8_t kind;    /* L7G_LOG_* */
    uint8_t flags;   /* HTTP bit0: a Host header is present.  Kafka bit0: ntopics > topic_stride */
    int16_t api_key; /* Kafka; HTTP: (major digit << 4) | minor digit */
    union {
        struct { uint32_t method_len, path_len, host_off, host_len, head_len, nheaders; } http;
        struct { int16_t api_version, pad; int32_t correlation_id; uint32_t ntopics; } kafka;
        /* l7g_classify_logged_all only (below) */
        struct { uint32_t cmd_off, cmd_len, nkeys; } mc_text;
        struct { uint32_t key_off, key_len; } mc_binary;
        struct { uint32_t cmd_len, file_off, file_len, nfields; } r2d2;
        struct { uint32_t table_len, keyword, word_off, word_len; } cassandra;
    } u;
    uint32_t reserved; /* 0 */
} l7g_logrec_t; /* 32 bytes */
typedef struct { l7g_logrec_t *rec; l7g_span_t *topics; uint32_t topic_stride; } l7g_log_out_t;
int l7g_classify_logged(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                        const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                        uint32_t *consumed, uint64_t *counters, const l7g_log_out_t *log, void *stream);
int l7g_classify_logged_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                             const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                             uint32_t *consumed, const l7g_log_out_t *log);
/* The API key's name as the policy language spells it (apiKeyToString,
 * pkg/proxy/kafka.go:162-167); NULL = unknown: print the key in decimal. */
const char *l7g_kafka_api_key_name(int16_t key);

/* Access-log records of every parser (opt-in; none of the calls above is
 * touched by it).  l7g_classify_logged_all is l7g_classify_logged -- the same
 * verdict / rule / consumed / counters, and for HTTP and Kafka requests byte
 * for byte the same record and row, spans / span_stride standing for topics /
 * topic_stride -- and also writes the fields of the one
 * LogEntry_GenericL7 { Proto, Fields } the proxylib parsers log per request on
 * memcached, r2d2 and cassandra connections.  As before a record means
 * something only where the verdict is L7G_ALLOW (entry type Request) or
 * L7G_DENY (Denied).  All offsets are from the request's first byte.
 *
 * memcached text (kind 3, Proto "textmemcached", text/parser.go:98-171):
 *   "command" is request bytes [cmd_off, cmd_off + cmd_len) -- tokens[0] of
 *   bytes.Fields(first line), which need not start at byte 0 -- and "keys" the
 *   nkeys key tokens joined by ", ": tokens[1:] for get*, tokens[2:] for gat*,
 *   tokens[1:2] for storage commands, delete, incr, decr and touch, none for
 *   every other command.  Row i of spans receives the first
 *   min(nkeys, span_stride) key spans; flags bit0 = nkeys > span_stride
 *   (submit the request again with a stride of its nkeys).
 * memcached binary (kind 4, "binarymemcached", binary/parser.go:97-105):
 *   "opcode" is api_key in decimal (request byte 1), "key" request bytes
 *   [key_off, key_off + key_len) with key_off = 24 + the extras length; a key
 *   length of 0 gives key_off 0.  Which of the two parsers a connection has is
 *   the classifier's choice (the connection's L7G_CONN_MC_* flags, else the
 *   request's first byte).
 * r2d2 (kind 5, "r2d2", r2d2parser.go:175-205): "cmd" is request bytes
 *   [0, cmd_len); nfields the length of strings.Split(line, " ") (empty fields
 *   count); "file" is [file_off, file_off + file_len) -- field 1 -- when
 *   nfields is 2, else empty (file_off and file_len 0).
 * cassandra (kind 6, "cassandra", cassandraparser.go:223-244): flags bit1 is
 *   set iff the reference logs an entry for the request: its path has exactly
 *   four '/'-separated parts, that is a QUERY or PREPARE (with sessions also a
 *   resolved EXECUTE) whose action and table hold no '/'.  Every other opcode
 *   has a two-part path and logs nothing.  "query_table" is the table as a
 *   rule's regex sees it (lowered; an undotted table of an action other than
 *   use prefixed with the keyspace and '.'), table_len bytes, of which the
 *   first min(table_len, text_stride) are written to row i of text; flags bit0
 *   = table_len > text_stride.  An empty table is logged as "".
 *   "query_action" is l7g_cass_action_name(api_key) for api_key 0..37.
 *   api_key -1 is an action outside the parser's queryActionMap, built by the
 *   caller as lower(kw) + "-" + lower(word) (+ "-view" when word lowers to
 *   "materialized"): kw is keyword (0 alter, 1 create, 2 drop, 3 truncate,
 *   4 list) and word the request bytes [word_off, word_off + word_len), the
 *   query's second field.  A resolved EXECUTE takes the action and table of
 *   its stored statement; limits of what a statement stores: for a stored
 *   action of -1 the word is gone (flags bit2: the action name is
 *   unavailable), and a stored table is kept only up to its first '/', so an
 *   EXECUTE of such a statement is logged with the cut table where the
 *   reference logs nothing.
 *   The keyspace is that of the last USE before the request on its connection
 *   in the batch; with sessions on, before the batch's first USE, the stored
 *   one, and statements resolve as they stood before the call.
 *
 * Rows of spans are written for Kafka and memcached text requests only, rows
 * of text for cassandra requests only, and never past the prefix named above.
 * spans NULL with span_stride 0 and text NULL with text_stride 0 are valid
 * (no rows are written); a non-zero stride with a NULL pointer is
 * hipErrorInvalidValue, a host-only engine answers hipErrorNoDevice.  rec,
 * spans and text are device memory for l7g_classify_logged_all (rec 16-byte
 * aligned) and host memory for l7g_classify_logged_all_host, which always
 * launches. */
enum { L7G_LOG_MC_TEXT = 3, L7G_LOG_MC_BINARY = 4, L7G_LOG_R2D2 = 5, L7G_LOG_CASSANDRA = 6 };
typedef struct {
    l7g_logrec_t *rec;                          /* n records, 16-byte aligned */
    l7g_span_t *spans; uint32_t span_stride;    /* n rows: Kafka topics, memcached text keys */
    uint8_t *text;     uint32_t text_stride;    /* n rows of bytes: cassandra query_table */
} l7g_log_all_out_t;
int l7g_classify_logged_all(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                            const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, int32_t *rule,
                            uint32_t *consumed, uint64_t *counters, const l7g_log_all_out_t *log, void *stream);
int l7g_classify_logged_all_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                                 const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict,
                                 int32_t *rule, uint32_t *consumed, const l7g_log_all_out_t *log);
/* CassActionName: the parser's name of action id 0..37; NULL outside. */
const char *l7g_cass_action_name(int16_t id);

/* Deny replies (opt-in; l7g_classify and everything it launches are untouched
 * by it).  A post-pass over a classified batch: for every request whose
 * verdict is L7G_DENY, the bytes the reference's enforcement point sends back,
 * packed in request order, with no host pass over the request bytes.
 *
 *   Kafka      req.CreateResponse(ErrTopicAuthorizationFailed), every topic and
 *              partition of the request echoed with errno 29
 *              (pkg/proxy/kafka.go:249-261, pkg/kafka/request.go:158-182,
 *              pkg/kafka/response.go:81-315, the encoders of
 *              vendor/.../proto/messages.go:610,911,1117,1342,1531,1716,1975):
 *              byte for byte what l7g_kafka_deny_response(request) writes, and
 *              nothing (len 0) where it returns -1 -- an untyped API key, or
 *              bytes that fail the typed decode
 *   HTTP       Envoy's 403 local reply, 87 bytes: sendLocalReply(Forbidden,
 *              "Access denied\r\n") (envoy/cilium_l7policy.cc:90-96,171-177)
 *   cassandra  the 35-byte unauthorized frame, unauthMsgBase
 *              (proxylib/cassandra/cassandraparser.go:269-278), with byte 0 =
 *              0x80 | (request byte 0 & 7) and bytes 2-3 = the request's stream
 *              id; nothing for a request shorter than 4 bytes
 *   r2d2       "ERROR\r\n" (proxylib/r2d2/r2d2parser.go:140-214)
 *   memcached  nothing (len 0), on purpose.  Whether and when a denied
 *              memcached request is answered depends on the connection's reply
 *              queue: the text parser injects at once only when the queue is
 *              empty and honours noreply, the binary parser goes by
 *              request / reply counters and enqueues twice.  The batch calls
 *              keep no such state; the proxylib shim does, per connection.
 * The protocol is the connection's (L7G_CONN_PROXYLIB connections included),
 * not the bytes': a DENY on an HTTP connection gives the 403 whatever the
 * request holds.
 *
 * verdict is what a classify call on the same stream wrote, or anything the
 * caller supplies: the call is memory-safe for any verdict array.  len[i] is 0
 * for every request whose verdict is not L7G_DENY, whose connection index is
 * outside the table or whose bytes are outside the arena.
 *
 * off, len and total are written for all n requests whatever cap is: reply i
 * is buf[off[i], off[i] + len[i]), off[] is the exclusive prefix sum of len[]
 * (a connection's consecutive requests have their replies contiguous and in
 * order), total[0] the bytes all replies need and total[1] the replies with
 * len > 0.  Reply i is written if and only if off[i] + len[i] <= cap, and no
 * byte at or past cap is touched: a caller that sees total[0] > cap calls again
 * with a larger buffer (buf NULL with cap 0 asks for the sizes only).
 *
 * All pointers are device memory for l7g_deny_replies, which is asynchronous on
 * `stream` and uses an engine-owned scratch, per stream and grow-only like
 * l7g_classify's: 256 + 4 n bytes (rounded up to 256) plus the prefix sum's
 * temporary storage (hipcub::DeviceScan: 9 KiB at n = 2^20, 1 MiB at 2^27).
 * n is at most 2^31 - 1.  l7g_deny_replies_host takes host memory (copies in, runs,
 * copies out, synchronises; the calling thread's stream, and a staging of 16 n
 * + cap bytes on the device and pinned, grow-only per calling thread).
 * Returns 0 or a hipError_t: hipErrorNoDevice on a host-only engine,
 * hipErrorInvalidValue for a NULL off, len or total or buf NULL with cap > 0.
 *
 * l7g_deny_reply_template: the fixed reply of L7G_PROTO_HTTP, _CASSANDRA
 * (before its three request bytes are set) or _R2D2 and its length; NULL and 0
 * for a protocol without one. */
typedef struct {
    uint8_t  *buf;   uint64_t cap;   /* reply bytes; buf may be NULL with cap 0 (sizes only) */
    uint64_t *off;   uint32_t *len;  /* n each: reply i is buf[off[i], off[i]+len[i]); len 0 = nothing to send */
    uint64_t *total;                 /* 2 words: [0] bytes all replies need, [1] replies with len > 0 */
} l7g_reply_out_t;
int l7g_deny_replies(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                     const uint32_t *conn, uint32_t n, const uint8_t *verdict, const l7g_reply_out_t *out,
                     void *stream);
int l7g_deny_replies_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                          const uint32_t *len, const uint32_t *conn, uint32_t n, const uint8_t *verdict,
                          const l7g_reply_out_t *out);
const uint8_t *l7g_deny_reply_template(int proto, size_t *len);

/* Cassandra sessions (off by default; with them off every answer is the
 * stateless one, byte for byte).
 *
 * l7g_cass_sessions_enable: max_statements > 0 turns them on (again: all
 * sessions start empty), 0 turns them off and frees the tables.  Two
 * open-addressed tables are allocated, statements by (connection, stream id)
 * and by (connection, prepared id), each with room for at least
 * max_statements entries (twice that, rounded up to a power of two; at most
 * 2^24 statements), and one 272-byte slot per connection index, grown with the
 * connection table.  A host-only engine returns hipErrorNoDevice.
 *
 * With sessions on, a request batch is classified against the state as it
 * stood before the call -- except the keyspace, which inside a batch is that
 * of the last USE before the request on its connection, and before the
 * batch's first USE the stored one -- and then committed in batch order per
 * connection: the last USE becomes the stored keyspace; every PREPARE whose
 * query parses is stashed under its stream id, whatever its verdict, with the
 * keyspace in force at its position (last PREPARE wins).  An EXECUTE whose id
 * was bound before its call began is matched against the connection's current
 * rule set (ALLOW with the rule id or DENY, consumed = the frame length); any
 * other id answers L7G_PARSE_ERROR, consumed 2, as in the stateless mode.
 *
 * l7g_cass_replies takes the reply direction: n buffers on device memory, as
 * l7g_classify takes requests.  Each is framed as cassandraparser.go frames a
 * reply (INCOMPLETE with the missing byte count; PARSE_ERROR 3 for a body over
 * 256 MB; PARSE_ERROR 0 where the parser panics; otherwise ALLOW, consumed =
 * the frame length -- replies are never denied), and a RESULT/prepared reply
 * binds the statement stashed under its stream id, as it stood before the
 * call, to its prepared id (last reply wins).  A buffer on a connection that
 * is not Cassandra answers L7G_UNSUPPORTED.  Returns hipErrorNotReady while
 * sessions are off.  l7g_cass_replies_host is the same on host buffers
 * (copies in, runs, copies out, synchronises; the calling thread's stream).
 *
 * Limits: a keyspace over 256 bytes, a table part over 240 bytes or a
 * prepared id over 64 bytes does not fit.  Requests that would need such a
 * keyspace or table answer L7G_UNSUPPORTED; such an id is not bound, so its
 * EXECUTE answers unprepared.  A full table drops the insert: a later EXECUTE
 * answers unprepared, which a client recovers from by preparing again.  No
 * limit ever turns into an ALLOW or DENY the reference would not give.
 *
 * Resets: l7g_conn_update(index) is the new-connection event and empties that
 * connection's session; l7g_conns_set empties all; l7g_cass_session_reset
 * empties the named ones.  A policy update resets nothing: the stored
 * statements are matched against the policy in force at EXECUTE.
 *
 * The state is engine-wide, not per stream: calls that touch one connection
 * (its requests, its replies, its resets) must be ordered by the caller, by
 * issuing them on one stream.  Sessions of different connections are
 * independent, so batches over disjoint connections may run on different
 * streams.
 *
 * l7g_cass_session_stats: [0] statements held by stream id, [1] by prepared
 * id, [2] inserts dropped (table full), [3] keyspaces / tables / ids over
 * their cap, [4] EXECUTEs resolved, [5] EXECUTEs answered unprepared; [2..5]
 * since sessions were enabled.  Waits for the launched calls. */
int l7g_cass_sessions_enable(l7g_engine *e, uint32_t max_statements, char *err, size_t errlen);
int l7g_cass_replies(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                     const uint32_t *conn, uint32_t n, uint8_t *verdict, uint32_t *consumed, void *stream);
int l7g_cass_replies_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                          const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *verdict, uint32_t *consumed);
int l7g_cass_session_reset(l7g_engine *e, const uint32_t *conn, uint32_t n);
void l7g_cass_session_stats(l7g_engine *e, uint64_t out[6]);

/* Kafka sessions (off by default): the correlation cache of the in-agent Kafka
 * proxy (pkg/kafka/correlation_cache.go) for device-resident batches, one
 * session per connection index.  A post-pass: l7g_classify and its kernels are
 * not involved.  l7g_kafka_corr_* stays the host path for small calls.
 *
 * l7g_kafka_sessions_enable: max_inflight > 0 turns them on (again: all
 * sessions start empty), 0 turns them off and frees the tables.  One
 * open-addressed table of 40-byte entries is allocated, its capacity the power
 * of two that is at least 2 x max_inflight (at most 2^28 in flight), a second
 * one of the same size for l7g_kafka_session_gc to compact into, and one
 * 8-byte slot per connection index (a generation and the next sequence number,
 * starting at 1), grown with the connection table.  A host-only engine returns
 * hipErrorNoDevice.  While sessions are off the other calls return
 * hipErrorNotReady.
 *
 * l7g_kafka_forward is HandleRequest (correlation_cache.go:116-147) for a
 * batch: n frames on device memory as l7g_classify took them, size prefix
 * included, at any byte alignment, with the verdicts it gave.  Request i is
 * forwarded iff verdict[i] == L7G_ALLOW, conn[i] is a valid connection index
 * whose protocol is Kafka, and the frame lies inside the arena.  The forwarded
 * requests of one connection are numbered in batch order: the k-th of them (k
 * from 0) gets id next + k in uint32 arithmetic, and the connection's next
 * advances by their count.  With len >= 12 the original id is big-endian bytes
 * 8..12 (pkg/kafka/request.go:57-70) and those four bytes are overwritten in
 * the arena with the new id -- no other byte of the arena is written; with
 * len < 12 the original id is 0 and nothing is written, but the entry is made
 * all the same.  The entry keeps the original id, the api key (bytes 4..6) and
 * version (bytes 6..8; 0 for what a shorter frame lacks), tag[i] (0 when tag
 * is NULL: the caller's handle on whatever else its response log record
 * needs, in place of the reference's *RequestMessage) and now_ms.
 *   fwd[i]: 0 not forwarded; 1 rewritten and cached; 2 the table had no free
 *   slot: the bytes are untouched, nothing is cached, the sequence number is
 *   spent, and the caller must not send this request under this session.
 *   new_id[i]: the new id when fwd[i] == 1, else 0.
 * The access-log record of a request carries the client's id
 * (pkg/proxy/kafka.go:169-181 runs before HandleRequest), so
 * l7g_classify_logged and l7g_deny_replies go before l7g_kafka_forward on the
 * stream.  An id repeats only after 2^32 forwards on one connection; a request
 * still in flight by then is out of contract.
 *
 * l7g_kafka_responses is CorrelateResponse (:158-178) for a batch of
 * size-prefixed response frames.  The id is big-endian bytes 4..8 if len >= 8,
 * else 0 (pkg/kafka/response.go:33-46).  A live entry of (conn[i], id) is a
 * hit: the original id is restored in place (if len >= 8), the entry is
 * forgotten, found[i] = 1 and orig_id, api_key, api_version and tag are those
 * of the request.  A miss leaves the bytes alone and sets found[i] and the
 * other outputs to 0; a connection that is invalid or not Kafka is a miss.
 * When several responses of one batch carry one id on one connection, the
 * earliest in batch order is the hit and the others are misses, as in the
 * reference's loop.
 *
 * The _host twins take host buffers on the calling thread's stream: inputs
 * staged as for l7g_classify_host, the small outputs copied back, the
 * caller's arena patched from new_id / orig_id (four bytes per hit) instead of
 * copied back; they synchronise.
 *
 * l7g_kafka_session_gc drops every entry with now_ms - created_ms >=
 * lifetime_ms (an entry from after now_ms has age 0; the reference's
 * RequestLifetime is 5 minutes, the clock is the caller's), re-inserts the
 * others into the second table and swaps the two, so that answered and stale
 * slots are gone as well: afterwards stats [1] == [0].  *expired (may be NULL)
 * is the number dropped.  Waits for the launched calls.  Without it the
 * never-used slots run out under churn and a miss then costs a probe of the
 * whole table -- correct, but slow: watch [1] against the capacity.
 *
 * Resets: l7g_conn_update(index) is the new-connection event: that
 * connection's entries stop resolving and its numbering restarts at 1;
 * l7g_conns_set empties all; l7g_kafka_session_reset empties the named ones.
 * A policy update resets nothing.  Resets are applied before the next launch.
 *
 * The state is engine-wide, not per stream: calls that touch one connection
 * must be ordered by the caller, by issuing them on one stream; calls over
 * disjoint connections may use different streams.
 *
 * l7g_kafka_session_stats: [0] live entries, [1] table slots that are not
 * never-used (live + answered + stale), [2] inserts dropped (table full), [3]
 * requests forwarded (fwd 1), [4] responses found, [5] responses missed, [6]
 * entries expired; [2..6] since sessions were enabled.  Waits for the
 * launched calls.  A host-only engine, or sessions off: zeros. */
int l7g_kafka_sessions_enable(l7g_engine *e, uint32_t max_inflight, char *err, size_t errlen);
int l7g_kafka_forward(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                      const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag /* may be NULL */, uint32_t n,
                      uint64_t now_ms, uint8_t *fwd, uint32_t *new_id, void *stream);
int l7g_kafka_responses(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                        const uint32_t *conn, uint32_t n, uint8_t *found, uint32_t *orig_id, int16_t *api_key,
                        int16_t *api_version, uint64_t *tag, void *stream);
int l7g_kafka_forward_host(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                           const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag, uint32_t n,
                           uint64_t now_ms, uint8_t *fwd, uint32_t *new_id);
int l7g_kafka_responses_host(l7g_engine *e, uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                             const uint32_t *len, const uint32_t *conn, uint32_t n, uint8_t *found, uint32_t *orig_id,
                             int16_t *api_key, int16_t *api_version, uint64_t *tag);
int l7g_kafka_session_gc(l7g_engine *e, uint64_t now_ms, uint64_t lifetime_ms, uint64_t *expired);
int l7g_kafka_session_reset(l7g_engine *e, const uint32_t *conn, uint32_t n);
void l7g_kafka_session_stats(l7g_engine *e, uint64_t out[7]);

/* Memcached sessions (off by default): the reply queue of the text parser
 * (proxylib/memcached/text/parser.go) and the request / reply counters and
 * inject queue of the binary parser (proxylib/memcached/binary/parser.go) for
 * device-resident batches, one session per connection index.  A post-pass:
 * l7g_classify and its kernels are not involved.  The proxylib shim stays the
 * host path for one connection per call.
 *
 * l7g_mc_sessions_enable: max_pending > 0 turns them on (again: all sessions
 * start empty), 0 turns them off and frees the memory.  Each connection's text
 * queue is a ring of 16-byte intents (reply class, denied bit, the caller's
 * tag) whose capacity C is the power of two that is at least max_pending (at
 * most 65536: larger values return hipErrorInvalidValue), and each connection
 * index has one 32-byte slot; both grow with the connection table.  Memory:
 * (32 + 16 C) bytes per connection index, plus 64 bytes.  A host-only engine
 * returns hipErrorNoDevice.  While sessions are off the other calls return
 * hipErrorNotReady.
 *
 * l7g_mc_forward is the request direction (OnData(reply = false) of both
 * parsers, from Matches on) for a batch: n requests on device memory as
 * l7g_classify took them, with the verdicts it gave.  Request i takes part iff
 * verdict[i] is L7G_ALLOW or L7G_DENY, conn[i] is a valid connection index
 * whose protocol is memcached, its bytes lie inside the arena, and (text) its
 * first line ends in "\r\n" inside the request and has a token -- which holds
 * for every request l7g_classify answered ALLOW or DENY.  The requests of one
 * connection are applied in batch order, by index, wherever they stand in the
 * batch.  The parser (text or binary) is the one l7g_classify used: the
 * connection's flag, else the request's first byte (>= 0x80: binary).  The
 * first participating request -- or the first reply stream, below -- locks it
 * in the slot; a later request of the other kind gets act 7, changes nothing
 * and is counted.  A caller who wants the reference exactly sets the flag.
 *   text: the command is the first token of bytes.Fields(first line); noreply
 *   is decided by the token count for storage commands, delete, incr, decr and
 *   touch, by the last token being "noreply" for flush_all and cache_memlimit,
 *   and quit is always noreply; watch sets the connection's watching mode,
 *   whatever the verdict.  An ALLOW that owes a reply is queued; a DENY that
 *   owes one is answered at once iff the queue is empty, else queued as
 *   denied; a noreply request changes nothing.
 *   binary: requestCount advances; a DENY is answered at once iff requestCount
 *   == replyCount + 1 (which advances replyCount), else it waits in the inject
 *   queue as in the reference -- where, after the first DENY of a connection's
 *   life has been injected, no later queued one is ever reached.
 *   act[i]: 0 not handled; 1 pass, reply owed; 2 pass, noreply; 3 drop, send
 *   the denied message now (binary: with byte 0 = request byte 0 | 0x81); 4
 *   drop, the denied message is queued behind the replies still owed; 5 drop,
 *   noreply; 6 the ring is full: nothing is queued and the caller must not
 *   forward the request; 7 kind mismatch.  Within one call the pushes of a
 *   connection succeed exactly while count < C, so every later pushing request
 *   of that connection in the call is 6 as well; requests that push nothing go
 *   on as usual.  Binary never answers 6.  The intent stores tag[i] (0 when
 *   tag is NULL).  Scratch per stream, grow-only: 49 n bytes plus 16 bytes per
 *   connection index plus the sort's and the scan's temporary storage; n is at
 *   most 2^31 - 1.
 *
 * l7g_mc_replies is the reply direction: stream s is arena[s_off[s], +s_len[s])
 * on connection s_conn[s], the reply bytes not yet passed, and the device runs
 * the op loop of proxylib/proxylib/connection.go:118-174 over it with max_ops
 * slots: until the ops are full; NOP ends it; an op of 0 bytes is
 * PARSER_ERROR (ops already written stay); MORE ends it; PASS advances the
 * input and the loop goes on, even over no input (so a queued inject follows
 * the reply it waited for in the same call); ERROR 2 (a binary reply without
 * bit 7 in its magic) neither advances nor ends the loop and fills the ops.
 * The device has no inject buffer, so the reference's "inject buffer full"
 * break never applies.  s_len 0 is legal: the "flush injects" call.  At most
 * one stream per connection per call: with a second one that connection's
 * results are unspecified (no memory outside its slot and ring is touched).
 * Outputs, slots [s * max_ops, (s + 1) * max_ops):
 *   op_kind  MORE 0, PASS 1, INJECT 3, ERROR 4 (FILTEROP_*)
 *   op_n     the op's byte count (INJECT: 28 per denied text intent popped, 37
 *            for the binary message; the bytes are l7g_mc_denied_message's)
 *   op_aux   (may be NULL) a text PASS that popped an intent: that intent's
 *            tag; a binary INJECT: the magic byte; else 0
 *   nops[s]  ops written
 *   result[s] 0 OK; 1 PARSER_ERROR; 2 not a memcached connection, an invalid
 *            connection index or a stream outside the arena (no ops, no state
 *            change); 3 no parser yet and no byte to make one from: no request
 *            and no reply has locked a parser and s_len is 0 (the reference's
 *            NOP; no ops, no state change).  With no parser yet and s_len > 0
 *            the stream makes one as memcached/parser.go:186-202 does -- the
 *            connection's flag, else the stream's first byte -- and runs.
 *   taken[s] the sum of the PASS counts; a binary PASS may reach past the
 *            bytes present, as in the reference.
 * A stream whose ops fill max_ops ends there; a later call with the bytes from
 * taken onward continues exactly where one call with more slots would have.
 *
 * The _host twins take host buffers on the calling thread's stream: inputs
 * staged as for l7g_classify_host, the small outputs copied back (op slots
 * past nops[s] come back 0); they synchronise.
 *
 * Resets: l7g_conn_update(index) is the new-connection event and empties that
 * connection's session; l7g_conns_set empties all; l7g_mc_session_reset
 * empties the named ones.  A policy update resets nothing.  Resets are applied
 * before the next launch.
 *
 * The state is engine-wide, not per stream: calls that touch one connection
 * (its requests, its replies, its resets) must be ordered by the caller, by
 * issuing them on one stream; calls over disjoint connections may use
 * different streams.
 *
 * l7g_mc_session_stats: [0] intents queued now, [1] connections with a
 * session (a locked parser), [2] pushes refused (ring full), [3] kind
 * mismatches, [4] denied messages due at once (act 3), [5] denied messages
 * injected from the queue, [6] reply frames passed (text: PASS ops that popped
 * an intent; binary: PASS ops), [7] parser errors; [2..7] since sessions were
 * enabled.  Waits for the launched calls.  A host-only engine, or sessions
 * off: zeros.
 *
 * l7g_mc_denied_message: the text parser's DeniedMsg (28 bytes) or, binary
 * != 0, the binary parser's DeniedMsgBase (37 bytes; the sender sets byte 0). */
int l7g_mc_sessions_enable(l7g_engine *e, uint32_t max_pending, char *err, size_t errlen);
int l7g_mc_forward(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off, const uint32_t *len,
                   const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag /* may be NULL */, uint32_t n,
                   uint8_t *act, void *stream);
int l7g_mc_replies(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                   const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_ops, uint8_t *op_kind,
                   uint32_t *op_n, uint64_t *op_aux /* may be NULL */, uint32_t *nops, uint8_t *result, uint64_t *taken,
                   void *stream);
int l7g_mc_forward_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *off,
                        const uint32_t *len, const uint32_t *conn, const uint8_t *verdict, const uint64_t *tag,
                        uint32_t n, uint8_t *act);
int l7g_mc_replies_host(l7g_engine *e, const uint8_t *arena, uint64_t arena_len, const uint64_t *s_off,
                        const uint32_t *s_len, const uint32_t *s_conn, uint32_t n, uint32_t max_ops, uint8_t *op_kind,
                        uint32_t *op_n, uint64_t *op_aux, uint32_t *nops, uint8_t *result, uint64_t *taken);
int l7g_mc_session_reset(l7g_engine *e, const uint32_t *conn, uint32_t n);
void l7g_mc_session_stats(l7g_engine *e, uint64_t out[8]);
const uint8_t *l7g_mc_denied_message(int binary, size_t *len);

/* Resident services: the synchronous drop-in calls of l7g_classify_host (and
 * so the Envoy adapter's Allowed() and proxylib's OnData) whose requests are
 * all HTTP (at most 8) or all memcached (at most 64) are posted to one polling
 * workgroup per protocol instead of launched: no launch and no completion
 * signal per call.  A service starts with the first such call, stays while
 * calls keep coming and leaves after ~50 ms without one, when a batch of
 * 4096 or more requests wants every CU, or before a policy or connection
 * update.  Answers are those of the launched path (the same device code); a
 * kernel fault is reported by the call that was waiting.  On by default
 * (L7G_SERVICE=0 at engine creation turns it off).  Returns the previous
 * setting. */
int l7g_service_enable(l7g_engine *e, int on);
/* [0] HTTP calls served, [1] HTTP workgroup launches, [2] memcached calls,
 * [3] memcached launches. */
void l7g_service_stats(l7g_engine *e, uint64_t out[4]);

/* Asynchronous batching for callers that decide one request at a time on an
 * event loop -- Envoy's cilium.l7policy decodeHeaders
 * (envoy/cilium_l7policy.cc:127-182), which would return StopIteration and
 * resume (continueDecoding / sendLocalReply) from the callback.  Submitters
 * copy their request straight into the open batch slot (pinned host memory in
 * the layout the device copy reads; a fetch-and-add on one of the slot's eight
 * lane words reserves the place, no lock).  Two flusher threads each seal the open slot once max_requests are in
 * it, its first request has waited max_wait_us, or a flush is asked for
 * (under load a batch can hold up to twice max_requests: requests keep coming
 * while the slot is sealed), classify it in place with one launch on their own
 * stream (so one batch is on the device while the next fills), and call each
 * request's callback from the flusher thread -- batches in the order they
 * were sealed, a thread's requests in submission order.  A device failure
 * answers every request of that batch L7G_UNSUPPORTED.  A callback must not
 * call l7g_batcher_flush or l7g_batcher_destroy (from a flusher thread both
 * return at once, doing nothing). */
typedef void (*l7g_done_fn)(void *ctx, uint8_t verdict, int32_t rule, uint32_t consumed);
typedef struct l7g_batcher l7g_batcher;
/* Slots hold max(2 x max_requests, 1024) requests and 2 KiB of request bytes
 * per request each; four slots are allocated (pinned) up front.  max_requests
 * is capped at 65536 (4 x 256 MiB pinned).  NULL when the engine has a device
 * and the slots cannot be pinned (the device path needs pinned slots). */
l7g_batcher *l7g_batcher_create(l7g_engine *e, uint32_t max_requests, uint32_t max_wait_us);
/* The batch size the batcher flushes at: max_requests as created, or 65536
 * when create capped it (a caller that asked for more learns it here). */
uint32_t l7g_batcher_max_requests(const l7g_batcher *b);
/* 0 = queued; -1 = the batcher is shutting down; -2 = backpressure: both
 * flushers are busy and the open slot is full, or the request is larger than
 * one of a slot's eight lanes (max(2 x max_requests, 1024) x 256 bytes) (the
 * callback is not called; the caller decides the request itself or retries). */
int l7g_batcher_submit(l7g_batcher *b, const uint8_t *req, uint32_t len, uint32_t conn, l7g_done_fn done, void *ctx);
/* Flushes now and returns once every request submitted before the call has
 * had its callback (0); -1 when called from a callback. */
int l7g_batcher_flush(l7g_batcher *b);
/* Flushes what is pending, then stops the flusher threads. */
void l7g_batcher_destroy(l7g_batcher *b);
/* Requests classified and launches made so far (for latency accounting). */
void l7g_batcher_stats(l7g_batcher *b, uint64_t *requests, uint64_t *launches);
/* Where the flusher threads' time went, summed over both, in ns: [0] waiting
 * for a sealed slot's entries to be published, [1] the device round trip (copy, launch, wait),
 * [2] callbacks, [3] waiting for the previous batch's callbacks (ordering);
 * [4] the largest batch. */
void l7g_batcher_timing(l7g_batcher *b, uint64_t out[5]);

/* Measurement hook (bench.py): with profiling on, l7g_classify records HIP
 * events on its stream around each kernel it launches; l7g_profile_last waits
 * for the last call and returns the device time in ms of its four stages
 * (partition, HTTP, Kafka, memcached; 0 = not launched).  Off by default. */
int l7g_profile_enable(l7g_engine *e, int on);

/* Proxy statistics (pkg/endpoint/endpoint.go:2207-2233 UpdateProxyStatistics,
 * the policy_l7_received/forwarded/denied/parse_errors_total counters of
 * pkg/metrics/metrics.go:269-296): while enabled, every l7g_classify adds, per
 * (policy, protocol, port, direction) of its connections, the requests that
 * completed a flow -- ALLOW = forwarded, DENY = denied, PARSE_ERROR = error,
 * each also received -- into a device accumulator.  l7g_flow_stats copies the
 * non-zero entries out (at most cap; *n = how many there are) and, with reset,
 * zeroes the accumulator.  Off by default. */
typedef struct {
    int32_t policy;
    uint8_t proto;     /* L7G_PROTO_* */
    uint8_t ingress;
    uint16_t port;
    uint64_t received, forwarded, denied, error;
} l7g_flow_stat_t;
int l7g_flow_stats_enable(l7g_engine *e, int on);
int l7g_flow_stats(l7g_engine *e, l7g_flow_stat_t *out, uint32_t cap, uint32_t *n, int reset);
int l7g_profile_last(l7g_engine *e, float out_ms[4]);

/* Profiling hook: per-phase cycle totals of the HTTP kernels, 16 slots (0
 * window DMA, 1 parse, 2 long-value scan, 3 other, 4 rounds, 5 scanned values,
 * 6 tiles, 7 rule-set image staging; latency kernel: 8 request fetch, 9 CR
 * scan, 10 lines framed, 11 merge + end of the header block, 12 requests),
 * summed over waves since the last reset.  Only a timing build
 * (-DL7G_PHASE_TIMING) records them; the product build returns
 * hipErrorNotSupported. */
int l7g_debug_phase_times(l7g_engine *e, uint64_t *out16, int reset);
/* The same for the Kafka kernel (-DL7G_KX_TIMING builds; slots: 0 framing,
 * 1 walk, 2 CRC pass, 3 topic lookups, 4 verdict + output, 5 walk rounds,
 * 6 window refills, 7 tiles). */
int l7g_debug_kafka_phase_times(l7g_engine *e, uint64_t *out8, int reset);
/* Per-phase cycle totals of the text-stream framer (-DL7G_FRAME_PHASES builds only; else an error). */
int l7g_debug_frame_phase_times(l7g_engine *e, uint64_t *out8, int reset);

/* Kafka correlation-ID rewriting of the in-agent Kafka proxy's forwarding
 * path (pkg/kafka/correlation_cache.go:97-213; one cache per client
 * connection, pkg/proxy/kafka.go:335).  Host code.
 *   l7g_kafka_corr_requests: HandleRequest for a batch of forwarded (allowed)
 *     request frames, in order: each frame's correlation id (bytes 8..12) is
 *     replaced in place by the cache's next sequence number (from 1), written
 *     to new_ids (may be null), and the original remembered.
 *   l7g_kafka_corr_responses: CorrelateResponse for a batch of broker
 *     response frames: a known id (bytes 4..8) is replaced in place by the
 *     original and forgotten; found[i] = 1 then, else 0 (frame untouched).
 *   l7g_kafka_corr_gc: drop entries at least lifetime_ms old (the reference
 *     runs this every RequestLifetime = 5 min); returns how many. */
typedef struct l7g_kafka_corr l7g_kafka_corr;
l7g_kafka_corr *l7g_kafka_corr_create(void);
void l7g_kafka_corr_destroy(l7g_kafka_corr *c);
int l7g_kafka_corr_requests(l7g_kafka_corr *c, uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t n,
                            uint32_t *new_ids);
int l7g_kafka_corr_responses(l7g_kafka_corr *c, uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t n,
                             uint8_t *found);
uint64_t l7g_kafka_corr_gc(l7g_kafka_corr *c, uint64_t lifetime_ms);
uint64_t l7g_kafka_corr_size(l7g_kafka_corr *c);

/* Test hook: compile one Go regexp with the product's DFA compiler and run
 * the compiled tables on the host.  Returns 1 match, 0 no match, -1 compile
 * error (err set).  anchored: 1 = full match, 0 = Go regexp.Match. */
int l7g_debug_regex(const char *pat, size_t patlen, int anchored, const uint8_t *s, size_t slen, char *err,
                    size_t errlen);
/* The same through the bit-parallel NFA fallback (the DevNfa tables and the
 * walk the device pre-pass runs); -1 also when the pattern needs more than
 * 1024 NFA positions. */
int l7g_debug_regex_nfa(const char *pat, size_t patlen, int anchored, const uint8_t *s, size_t slen, char *err,
                        size_t errlen);

#ifdef __cplusplus
}
#endif
#endif

"""A literal Python restatement of what the reference's two memcached parsers
keep per connection, and of the op loop that drives them (test infrastructure;
the yardstick of the device sessions, l7g_mc_forward / l7g_mc_replies):

  text    proxylib/memcached/text/parser.go:72-331   replyQueue, watching
  binary  proxylib/memcached/binary/parser.go:58-165 requestCount, replyCount,
          injectQueue -- the literal queue, double append included
  unified proxylib/memcached/parser.go:186-202       the parser a first byte makes
  loop    proxylib/proxylib/connection.go:118-174

The request direction takes the classifier's verdict in place of
Connection.Matches and the frame it framed in place of the parser's own
framing: everything from Matches on is restated.  Nothing here is derived from
the device code; tests/test_mc_sessions_host.py pins it to the reference's 31
recorded op sequences."""
import numpy as np

from generic_log_py import go_fields

DENY, ALLOW = 0, 1
PROTO_MEMCACHE = 3
MORE, PASS, DROP, INJECT, ERROR, NOP = 0, 1, 2, 3, 4, 256
OK, PARSER_ERROR = 0, 1
ERROR_INVALID_FRAME_TYPE = 2
DENIED_TEXT = b"CLIENT_ERROR access denied\r\n"                    # text/parser.go:327
DENIED_BINARY = bytes([0x81, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0x0d] + [0] * 12) + b"access denied"  # binary/parser.go:194-205
PAYLOAD_END = b"\r\nEND\r\n"

# act codes of l7g_mc_forward
A_NONE, A_PASS, A_PASS_NOREPLY, A_DROP_NOW, A_DROP_QUEUED, A_DROP_NOREPLY, A_FULL, A_MISMATCH = range(8)

STORAGE = (b"set", b"add", b"replace", b"append", b"prepend", b"cas")
ONE_LINE = STORAGE + (b"delete", b"incr", b"decr", b"touch", b"slabs", b"lru", b"flush_all", b"cache_memlimit",
                      b"version", b"misbehave")


class Panic(Exception):
    """A Go runtime panic inside a parser: OnData recovers it as PARSER_ERROR."""


def fields(b):
    return [bytes(b[s:e]) for s, e in go_fields(bytes(b))]


def is_retrieval(cmd):
    return cmd.startswith(b"get") or cmd.startswith(b"gat")


class TextParser:
    kind = 1

    def __init__(self, cap):
        self.reply_queue = []   # [command, denied, tag]
        self.watching = False
        self.cap = cap          # the device ring's capacity (the reference's slice has none)

    # ---- request direction (:98-198, from the token switch on)
    def on_request(self, frame, verdict, tag, counts):
        lf = frame.find(b"\r\n")
        tokens = fields(frame[:lf]) if lf >= 0 else []
        if not tokens:
            return None, b""    # (the parser would not have reached Matches: no ALLOW / DENY exists for it)
        cmd = tokens[0]
        noreply = False
        if is_retrieval(cmd):
            pass
        elif cmd in STORAGE:
            noreply = len(tokens) == (7 if cmd[0:1] == b"c" else 6)
        elif cmd == b"delete":
            noreply = len(tokens) == 3
        elif cmd in (b"incr", b"decr", b"touch"):
            noreply = len(tokens) == 4
        elif cmd in (b"flush_all", b"cache_memlimit"):
            noreply = tokens[-1] == b"noreply"
        elif cmd == b"quit":
            noreply = True
        elif cmd == b"watch":
            self.watching = True    # (before Matches: whatever the verdict)
        if verdict == ALLOW:
            if noreply:
                return A_PASS_NOREPLY, b""
            if len(self.reply_queue) >= self.cap:
                counts["full"] += 1
                return A_FULL, b""
            self.reply_queue.append([cmd, False, tag])
            return A_PASS, b""
        if noreply:
            return A_DROP_NOREPLY, b""
        if not self.reply_queue:
            counts["inject_now"] += 1
            return A_DROP_NOW, DENIED_TEXT
        if len(self.reply_queue) >= self.cap:
            counts["full"] += 1
            return A_FULL, b""
        self.reply_queue.append([cmd, True, tag])
        return A_DROP_QUEUED, b""

    # ---- reply direction (:73-81, :87-94, :203-262): one OnData -> (op, n, aux, injected bytes)
    def on_reply(self, data, counts):
        injected = 0
        for rep in self.reply_queue:
            if not rep[1]:
                break
            injected += 1
        if injected:
            del self.reply_queue[:injected]
            counts["inject_queued"] += injected
            return INJECT, injected * len(DENIED_TEXT), 0, DENIED_TEXT * injected
        if not data:
            return NOP, 0, 0, b""
        lf = data.find(b"\r\n")
        if lf < 0:
            return MORE, 1 if data[-1:] == b"\r" else 2, 0, b""
        tokens = fields(data[:lf])
        if not self.reply_queue:
            raise Panic("replyQueue[0]")
        intent = self.reply_queue[0]
        if self.watching:
            return PASS, lf + 2, 0, b""
        if not tokens:
            raise Panic("tokens[0]")
        cmd, t0 = intent[0], tokens[0]
        if t0 in (b"ERROR", b"CLIENT_ERROR", b"SERVER_ERROR") or cmd in ONE_LINE:
            return self._pop(lf + 2, counts)
        if is_retrieval(cmd) or cmd == b"stats":
            return self._until_end(data, counts)
        if cmd == b"lru_crawler":
            if t0 in (b"OK", b"BUSY", b"BADCLASS"):
                return self._pop(lf + 2, counts)
            return self._until_end(data, counts)
        return ERROR, 0, 0, b""

    def _pop(self, n, counts):
        tag = self.reply_queue.pop(0)[2]
        counts["passed"] += 1
        return PASS, n, tag, b""

    def _until_end(self, data, counts):
        end = data.find(PAYLOAD_END)
        if end > 0:
            return self._pop(end + len(PAYLOAD_END), counts)
        return MORE, 1, 0, b""

    def queued(self):
        return len(self.reply_queue)


class BinaryParser:
    kind = 2

    def __init__(self, cap):
        self.request_count = 0
        self.reply_count = 0
        self.inject_queue = []  # (magic, requestID)

    def on_request(self, frame, verdict, tag, counts):
        self.request_count = (self.request_count + 1) & 0xFFFFFFFF
        if verdict == ALLOW:
            return A_PASS, b""
        magic = 0x81 | frame[0]
        act, inj = A_DROP_QUEUED, b""
        if self.request_count == (self.reply_count + 1) & 0xFFFFFFFF:
            inj = self._denied(magic)
            counts["inject_now"] += 1
            act = A_DROP_NOW
        else:
            self.inject_queue.append((magic, self.request_count))
        self.inject_queue.append((magic, self.request_count))   # (:135, appended again)
        return act, inj

    def _denied(self, magic):
        self.reply_count = (self.reply_count + 1) & 0xFFFFFFFF
        return bytes([magic]) + DENIED_BINARY[1:]

    def on_reply(self, data, counts):
        if self.inject_queue and self.inject_queue[0][1] == (self.reply_count + 1) & 0xFFFFFFFF:
            magic = self.inject_queue.pop(0)[0]
            counts["inject_queued"] += 1
            return INJECT, len(DENIED_BINARY), magic, self._denied(magic)
        if not data:
            return NOP, 0, 0, b""
        if len(data) < 24:
            return MORE, 24 - len(data), 0, b""
        body = int.from_bytes(data[8:12], "big")
        keylen, extras = int.from_bytes(data[2:4], "big"), data[4]
        if keylen > 0 and 24 + keylen + extras > len(data):
            return MORE, 24 + keylen + extras - len(data), 0, b""
        if data[0] & 0x80 != 0x80:
            return ERROR, ERROR_INVALID_FRAME_TYPE, 0, b""
        self.reply_count = (self.reply_count + 1) & 0xFFFFFFFF
        n = (body + 24) & 0xFFFFFFFF
        if n:
            counts["passed"] += 1
        return PASS, n, 0, b""

    def queued(self):
        return 0


def op_loop(parser, data, max_ops, counts):
    """connection.go:118-174 over one reply stream, without an inject buffer:
    -> (ops [(kind, n, aux)], result, taken, injected bytes)."""
    ops, taken, inj = [], 0, b""
    data = bytes(data)
    while len(ops) < max_ops:
        try:
            op, n, aux, more = parser.on_reply(data, counts)
        except Panic:
            counts["errors"] += 1
            return ops, PARSER_ERROR, taken, inj
        inj += more
        if op == NOP:
            break
        if n == 0:
            counts["errors"] += 1
            return ops, PARSER_ERROR, taken, inj
        ops.append((op, n, aux))
        if op == MORE:
            break
        if op == PASS:
            taken += n
            data = data[n:]
        # (ERROR n != 0: neither advances nor ends the loop)
    return ops, OK, taken, inj


class Sessions:
    """The parsers of a connection table, driven by batches as the device calls are."""

    STATS = ("queued", "sessions", "full", "mismatch", "inject_now", "inject_queued", "passed", "errors")

    def __init__(self, conns, max_pending):
        self.cap = 1
        while self.cap < max_pending:
            self.cap <<= 1
        self.counts = dict.fromkeys(self.STATS[2:], 0)
        self.set_connections(conns)

    def set_connections(self, conns):
        self.mc = [int(p) == PROTO_MEMCACHE for p in conns["proto"]]
        self.flags = [int(f) & 3 for f in conns["flags"]]
        self.parsers = [None] * len(self.mc)

    def reset(self, c):
        self.parsers[c] = None

    def _make(self, c, first_byte):
        kind = self.flags[c] or (2 if first_byte >= 0x80 else 1)
        return (BinaryParser if kind == 2 else TextParser)(self.cap)

    def forward(self, frames, conn, verdict, tags=None, inside=None):
        """-> (act, injected bytes per request); inside[i] False: request i lies outside the arena."""
        n = len(frames)
        act, inj = np.zeros(n, np.uint8), [b""] * n
        for i, (f, c) in enumerate(zip(frames, np.asarray(conn).tolist())):
            v = int(verdict[i])
            if v not in (ALLOW, DENY) or c >= len(self.mc) or not self.mc[c] or not f:
                continue
            if inside is not None and not inside[i]:
                continue
            kind = self.flags[c] or (2 if f[0] >= 0x80 else 1)
            p = self.parsers[c]
            if kind == 1:
                lf = f.find(b"\r\n")
                if lf < 0 or not fields(f[:lf]):
                    continue
            if p is None:
                p = self.parsers[c] = self._make(c, f[0])
            if p.kind != kind:
                act[i] = A_MISMATCH
                self.counts["mismatch"] += 1
                continue
            a, b = p.on_request(bytes(f), v, 0 if tags is None else int(tags[i]), self.counts)
            act[i], inj[i] = a, b
        return act, inj

    def replies(self, streams, conn, max_ops, inside=None):
        """-> per stream (ops, result, taken, injected bytes); result 2 and 3 as l7g_mc_replies."""
        out = []
        for s, (d, c) in enumerate(zip(streams, np.asarray(conn).tolist())):
            if c >= len(self.mc) or not self.mc[c] or (inside is not None and not inside[s]):
                out.append(([], 2, 0, b""))
                continue
            if self.parsers[c] is None:
                if not d:
                    out.append(([], 3, 0, b""))
                    continue
                self.parsers[c] = self._make(c, d[0])
            out.append(op_loop(self.parsers[c], d, max_ops, self.counts))
        return out

    def stats(self):
        return dict(self.counts, queued=sum(p.queued() for p in self.parsers if p is not None),
                    sessions=sum(p is not None for p in self.parsers))

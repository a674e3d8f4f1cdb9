// The fixed replies a denied request is answered with (product code): the
// bytes exist once, here, for the proxylib shim (proxylib/shim.cc, which
// injects them one request at a time) and for the batch call l7g_deny_replies
// (kernels/deny_reply.hip, which writes them on the device).
//
//   kDenied403   Envoy's local reply for a denied HTTP request:
//                sendLocalReply(Forbidden, denied_403_body = "Access denied" +
//                CRLF) (envoy/cilium_l7policy.cc:90-96,171-177); 87 bytes
//   kCassUnauth  unauthMsgBase (proxylib/cassandra/cassandraparser.go:269-278);
//                35 bytes.  The sender sets byte 0 = 0x80 | (request byte 0 & 7)
//                and bytes 2-3 = the request's stream id.
//   kR2Error     the r2d2 parser's "ERROR\r\n" (proxylib/r2d2/r2d2parser.go:140-214);
//                7 bytes
//   kMcDeniedText    the text memcached parser's DeniedMsg (text/parser.go:327);
//                28 bytes
//   kMcDeniedBinary  the binary parser's DeniedMsgBase (binary/parser.go:194-205);
//                37 bytes.  The sender sets byte 0 = 0x81 | request byte 0.
//                Neither is written on the device: when they are due depends on
//                the connection's reply queue (the shim's, or the memcached
//                sessions', which report INJECT ops and leave the bytes to
//                l7g_mc_denied_message).
#pragma once
#include <stdint.h>

// (in a HIP translation unit the arrays live in the device's constant memory:
// the kernels index them; host code there does not use them)
#if defined(__HIPCC__)
#define L7_REPLY_CONST static __device__ __constant__ const
#else
#define L7_REPLY_CONST static const
#endif

namespace l7 {

L7_REPLY_CONST char kDenied403[] =
    "HTTP/1.1 403 Forbidden\r\ncontent-length: 15\r\ncontent-type: text/plain\r\n\r\nAccess denied\r\n";
L7_REPLY_CONST uint8_t kCassUnauth[35] = {0, 0, 0, 0, 0, 0, 0, 0, 0x1a, 0, 0, 0x21, 0, 0, 0x14, 'R', 'e', 'q',
                                          'u', 'e', 's', 't', ' ', 'U', 'n', 'a', 'u', 't', 'h', 'o', 'r', 'i', 'z',
                                          'e', 'd'};
L7_REPLY_CONST char kR2Error[] = "ERROR\r\n";
L7_REPLY_CONST char kMcDeniedText[] = "CLIENT_ERROR access denied\r\n";
L7_REPLY_CONST uint8_t kMcDeniedBinary[37] = {0x81, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0x0d, 0, 0, 0, 0, 0, 0, 0,
                                              0,    0, 0, 0, 0, 'a', 'c', 'c', 'e', 's', 's', ' ', 'd', 'e', 'n', 'i', 'e', 'd'};

constexpr uint32_t kDenied403Len = sizeof(kDenied403) - 1;  // (without the literal's NUL)
constexpr uint32_t kCassUnauthLen = sizeof(kCassUnauth);
constexpr uint32_t kR2ErrorLen = sizeof(kR2Error) - 1;
static_assert(kDenied403Len == 87 && kCassUnauthLen == 35 && kR2ErrorLen == 7, "reply template sizes");
static_assert(sizeof(kMcDeniedText) - 1 == 28 && sizeof(kMcDeniedBinary) == 37, "memcached denied messages");

}  // namespace l7

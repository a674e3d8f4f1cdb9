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

constexpr uint32_t kDenied403Len = sizeof(kDenied403) - 1;  // (without the literal's NUL)
constexpr uint32_t kCassUnauthLen = sizeof(kCassUnauth);
constexpr uint32_t kR2ErrorLen = sizeof(kR2Error) - 1;
static_assert(kDenied403Len == 87 && kCassUnauthLen == 35 && kR2ErrorLen == 7, "reply template sizes");

}  // namespace l7

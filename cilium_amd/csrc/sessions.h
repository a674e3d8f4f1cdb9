// What the sessions of every protocol share on the host (cass_sessions.cc,
// kafka_sessions.cc, mc_sessions.cc): one slot per connection index, grown
// with the connection table, the new-connection events applied before the next
// launch, and the frame of the entries -- enable, a call over a batch, reset,
// stats.  A protocol's file keeps its tables' sizes and caps, its launches and
// what only it has.  Every function here is called with e->mu held.
#pragma once
#include "engine_state.h"

// Runs `f` (enqueues on the null stream) once no launched kernel can touch the
// session tables, and waits for it.
template <class F>
hipError_t Quiet(l7g_engine *e, F f) {
    hipError_t rc = WaitLastClassify(e);
    if (rc == hipSuccess) rc = f();
    if (rc == hipSuccess) rc = hipStreamSynchronize(nullptr);
    return rc;
}

// With sessions on: a slot for every connection, and the pending resets
// applied (then forgotten).  zero_tables() enqueues the zeroing of the
// protocol's tables; reset(list, n) is its reset launch over n connection
// indices on the device.
template <class Slot, class ZeroTables, class Reset>
hipError_t SlotsSync(l7g_engine *e, Slot *&slots, uint32_t &nslots, SessionResets &resets, ZeroTables zero_tables,
                     Reset reset) {
    std::vector<uint32_t> &pending = resets.pending;
    hipError_t rc = hipSuccess;
    const size_t need = std::max<size_t>(e->conns.size(), 1);
    if (need > nslots) {  // grown with the connection table, the sessions so far kept
        const size_t cap = std::max(need, (size_t)nslots * 2);
        Slot *d = nullptr;
        if ((rc = hipMalloc(&d, cap * sizeof(Slot))) != hipSuccess) return rc;
        rc = Quiet(e, [&] {
            hipError_t r = hipMemsetAsync(d, 0, cap * sizeof(Slot), nullptr);
            if (r == hipSuccess && nslots)
                r = hipMemcpyAsync(d, slots, (size_t)nslots * sizeof(Slot), hipMemcpyDeviceToDevice, nullptr);
            return r;
        });
        if (rc != hipSuccess) { hipFree(d); return rc; }
        if (slots) hipFree(slots);
        slots = d;
        nslots = (uint32_t)cap;
    }
    if (resets.all) {
        // every session: zeroed slots and zeroed tables are the state sessions start in
        rc = Quiet(e, [&] {
            hipError_t r = hipMemsetAsync(slots, 0, (size_t)nslots * sizeof(Slot), nullptr);
            if (r == hipSuccess) r = zero_tables();
            return r;
        });
    } else if (!pending.empty()) {
        uint32_t *d = nullptr;
        const size_t bytes = pending.size() * sizeof(uint32_t);
        if ((rc = hipMalloc(&d, bytes)) != hipSuccess) return rc;
        rc = Quiet(e, [&] {
            hipError_t r = hipMemcpyAsync(d, pending.data(), bytes, hipMemcpyHostToDevice, nullptr);
            if (r == hipSuccess) r = reset(d, (uint32_t)pending.size());
            return r;
        });
        hipFree(d);
    }
    if (rc == hipSuccess) resets.Clear();
    return rc;
}

// l7g_*_sessions_enable begins: a device (else err says why), made current, and no launched kernel left to read the
// tables about to go.  It ends (rc: of the allocations and zeroing): a failure frees them again and goes to err.
inline hipError_t EnableBegin(l7g_engine *e, char *err, size_t errlen) {
    if (e->device < 0) { set_err(err, errlen, "a host-only engine keeps no sessions"); return hipErrorNoDevice; }
    hipError_t rc = hipSetDevice(e->device);
    if (rc == hipSuccess) rc = WaitLastClassify(e);
    if (rc != hipSuccess) set_err(err, errlen, hipGetErrorString(rc));
    return rc;
}
inline int EnableEnd(l7g_engine *e, hipError_t rc, void (*free_all)(l7g_engine *), char *err, size_t errlen) {
    if (rc == hipSuccess) rc = hipStreamSynchronize(nullptr);
    if (rc != hipSuccess) { free_all(e); set_err(err, errlen, hipGetErrorString(rc)); }
    return (int)rc;
}

// What every call over a batch starts with: its checks (on: this protocol's sessions are enabled), then CallBegin
// with those sessions synced (sync: kSync*).  The scratch follows the entry's array checks.
inline hipError_t Enter(l7g_engine *e, bool on, unsigned sync) {
    if (e->device < 0) return hipErrorNoDevice;
    if (!on) return hipErrorNotReady;
    return CallBegin(e, sync, nullptr, nullptr);
}

// l7g_*_session_reset: the indices join the pending events, which `sync` (the protocol's ...Sync) applies at once.
inline int SessionReset(l7g_engine *e, bool on, SessionResets &resets, const uint32_t *conn, uint32_t n,
                        hipError_t (*sync)(l7g_engine *)) {
    if (e->device < 0) return (int)hipErrorNoDevice;
    if (!on) return (int)hipErrorNotReady;
    resets.Add(true, conn, n);
    hipError_t rc = hipSetDevice(e->device);
    if (rc == hipSuccess) rc = sync(e);
    return (int)rc;
}

// l7g_*_session_stats: h[0 .. words + 2) = the device's statistics words and, behind them, the two live words,
// zeroed and then counted by live(out2) (the protocol's live launch on the null stream).  False: h is not filled.
template <class Live>
bool SessionStats(l7g_engine *e, bool on, hipError_t (*sync)(l7g_engine *), unsigned long long *stats, int words,
                  unsigned long long *h, Live live) {
    if (e->device < 0 || !on) return false;
    hipError_t rc = hipSetDevice(e->device);
    if (rc == hipSuccess) rc = sync(e);
    if (rc == hipSuccess)
        rc = Quiet(e, [&] {
            hipError_t r = hipMemsetAsync(stats + words, 0, 2 * sizeof(unsigned long long), nullptr);
            if (r == hipSuccess) r = live(stats + words);
            if (r == hipSuccess)
                r = hipMemcpyAsync(h, stats, (words + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, nullptr);
            return r;
        });
    return rc == hipSuccess;
}

// What the session tables of the three protocols share (cass_sessions.cc,
// kafka_sessions.cc, mc_sessions.cc): one slot per connection index, grown with the connection
// table, and the new-connection events applied before the next launch.
#pragma once
#include "engine_state.h"

// Runs `f` (enqueues on the null stream) once no launched kernel can touch the
// session tables, and waits for it.  Caller holds e->mu.
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
// indices on the device.  Caller holds e->mu.
template <class Slot, class ZeroTables, class Reset>
hipError_t SlotsSync(l7g_engine *e, Slot *&slots, uint32_t &nslots, std::vector<uint32_t> &pending, bool &reset_all,
                     ZeroTables zero_tables, Reset reset) {
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
    if (reset_all) {
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
    if (rc == hipSuccess) {
        pending.clear();
        reset_all = false;
    }
    return rc;
}

// lnr_handover.h -- the order of the two lanes' job launches (host only, no HIP: tests/handover_gate_main.cpp runs it under the thread
// sanitizer).
//
// A lane's round-0 job kernels flood the chip with single-wave workgroups for a whole bulk round.  The other lane's round-1 launch holds
// 1024- and 256-thread workgroups, and one that lands behind the flood finds no CU with enough free wave slots until the flood drains: that
// lane's next batch then starts a bulk round late.  Without a rule the two launches were a race won by 0.2 ms.  The rule: a lane passes the
// gate -- and enqueues round 0 -- only while the other lane is outside its hand-over, which runs from the gate to "my round-1 job kernels
// are enqueued, or I know there are none".  So the two floods alternate, and a round-1 launch never lands behind a flood.
//
// The state is guarded by the owner's mutex (lnr_ctx::mu) and signalled on its condition variable; `quit` is read under that mutex and
// lets a waiting lane through when the context is being closed.
#pragma once
#include <condition_variable>
#include <mutex>

namespace lnr_ho {

struct Handover {
    bool in[2] = {false, false};        // lane k is between its gate and the end of its hand-over
};

// Blocks until the other lane is outside its hand-over (or quit() holds), then takes the hand-over for lane `me`.  True when it had to
// wait: the other lane's round-1 launch has only just been enqueued, and the caller gives it a head start.
template <class Quit>
bool handover_enter(Handover &h, std::mutex &mu, std::condition_variable &cv, int me, Quit quit) {
    std::unique_lock<std::mutex> lk(mu);
    bool waited = false;
    while (h.in[me ^ 1] && !quit()) { waited = true; cv.wait(lk); }
    h.in[me] = true;
    return waited;
}

// Ends lane `me`'s hand-over and wakes the other lane.  False when the lane was not in one (every exit path may call it).
inline bool handover_leave(Handover &h, std::mutex &mu, std::condition_variable &cv, int me) {
    {
        std::lock_guard<std::mutex> g(mu);
        if (!h.in[me]) return false;
        h.in[me] = false;
    }
    cv.notify_all();
    return true;
}

}  // namespace lnr_ho

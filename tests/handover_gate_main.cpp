// Stand-alone program over linear_amd/csrc/lnr_handover.h (no HIP, no GPU): two threads run batches through the phase protocol of
// filter_dev -- gate, round-0 launch, hand-over, round-1 launch or none, random early exits -- and check the rule of the gate: while a
// lane is between its gate and the end of its hand-over the other lane is not.  Built with -fsanitize=thread by
// tests/test_handover_gate_cpu.py; a missed wake-up shows as the caller's time limit.
//   handover_gate_main <batches per lane> <seed>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include "../linear_amd/csrc/lnr_handover.h"

namespace {

std::mutex mu;
std::condition_variable cv;
lnr_ho::Handover ho;
bool quit_flag = false;             // (guarded by mu, as lnr_ctx::quit)
std::atomic<int> inside[2];         // lane k is between gate and hand-over end, by the lane's own account
std::atomic<long> violations{0}, waits{0}, early_exits{0}, no_round1{0};

struct Scope {                      // the shape of filter_dev's scope guard: leave() on every way out
    int me; bool held = false;
    explicit Scope(int m) : me(m) {}
    bool enter() {
        bool w = lnr_ho::handover_enter(ho, mu, cv, me, [] { return quit_flag; });
        held = true;
        if (inside[me ^ 1].load()) violations++;     // the other lane must be outside its hand-over now ...
        inside[me].store(1);
        return w;
    }
    void leave() {
        if (!held) return;
        held = false;
        inside[me].store(0);
        if (!lnr_ho::handover_leave(ho, mu, cv, me)) violations++;
    }
    ~Scope() { leave(); }
};

unsigned rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return s >> 8; }
void spin(unsigned n) { for (volatile unsigned k = 0; k < n; k++) {} }

void lane(int me, long batches, unsigned seed) {
    for (long b = 0; b < batches; b++) {
        Scope g(me);
        spin(rnd(seed) % 200);                      // prepare, seed lookup
        if (rnd(seed) % 16 == 0) { early_exits++; continue; }       // an error before the gate (prepare_batch)
        if (g.enter()) waits++;
        spin(rnd(seed) % 100);                      // round-0 launch
        if (inside[me ^ 1].load()) violations++;    // ... and at "round-0 enqueued"
        if (rnd(seed) % 16 == 0) { early_exits++; continue; }       // an error inside the hand-over: the guard lets go
        spin(rnd(seed) % 300);                      // round 0, tail A, flags
        if (rnd(seed) % 4 == 0) no_round1++;        // no read goes through the re-map round
        else spin(rnd(seed) % 100);                 // round-1 launch
        if (inside[me ^ 1].load()) violations++;
        g.leave();
        if (lnr_ho::handover_leave(ho, mu, cv, me)) violations++;   // a second leave is a no-op
        spin(rnd(seed) % 200);                      // tails, gather
    }
}

}  // namespace

int main(int argc, char **argv) {
    long batches = argc > 1 ? atol(argv[1]) : 10000;
    unsigned seed = argc > 2 ? (unsigned)atol(argv[2]) : 1u;
    std::thread a(lane, 0, batches, seed * 2 + 1), b(lane, 1, batches, seed * 2 + 2);
    a.join(); b.join();
    if (ho.in[0] || ho.in[1]) violations++;
    // a lane that waits at the gate of a lane that never leaves is let through by quit
    {
        Scope stuck(0);
        stuck.enter();
        std::thread w([] { (void)lnr_ho::handover_enter(ho, mu, cv, 1, [] { return quit_flag; }); (void)lnr_ho::handover_leave(ho, mu, cv, 1); });
        { std::lock_guard<std::mutex> l(mu); quit_flag = true; }
        cv.notify_all();
        w.join();
    }
    printf("%s batches %ld violations %ld waits %ld early_exits %ld no_round1 %ld\n", violations.load() ? "FAILED" : "ok", batches, violations.load(), waits.load(), early_exits.load(),
           no_round1.load());
    return violations.load() ? 1 : 0;
}

// hostwait.h -- bounded host spins on words a peer PE or the GPU writes (p2p.cpp,
// smallpath.cpp, signal.cpp, lock.cpp).  Internal to the library: kept out of its dynamic symbol table.
#pragma once
#include <sched.h>
#include <stdlib.h>
#include <time.h>

#pragma GCC visibility push(hidden)
namespace sosrt {

inline double now_s()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// Wall-clock bound of one wait (SHMEMX_P2P_TIMEOUT seconds, default 300, read once): a
// peer that never posts ends the job with a message instead of hanging it.
inline double wait_limit_s()
{
    static const double lim = [] {
        const char *e = getenv("SHMEMX_P2P_TIMEOUT");
        const double v = e ? atof(e) : 0.0;
        return v > 0 ? v : 300.0;
    }();
    return lim;
}

// Spin until ready() holds.  After every miss idle(spins) runs -- the caller's polling
// cadence: pause, yield, side checks -- and says whether to look at the clock this time.
// Once the clock checks span more than wait_limit_s(), expired(seconds) ends the job
// with the caller's message.
template <class Ready, class Idle, class Expired>
void spin_until(Ready ready, Idle idle, Expired expired)
{
    unsigned spins = 0;
    double t0 = 0;
    while (!ready()) {
        if (!idle(++spins)) continue;
        const double t = now_s();
        if (t0 == 0) t0 = t;
        else if (t - t0 > wait_limit_s()) expired(t - t0);
    }
}

// The idle() of a wait that probes a word.  Device memory: a probe is a launch and its
// completion, so look at the clock every time.  Memory the host addresses: a probe is a
// load, so pause for 255 spins, then yield and look.
struct ProbeCadence {
    bool device;
    bool operator()(unsigned spins) const
    {
        if (!device && (spins & 0xff)) {
            __builtin_ia32_pause();
            return false;
        }
        if (!device) sched_yield();
        return true;
    }
};

}  // namespace sosrt
#pragma GCC visibility pop

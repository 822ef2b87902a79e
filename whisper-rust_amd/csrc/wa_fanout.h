// wa_fanout.h - the thread fan-out under every lock-step wave (wa_wave.cpp).  Standard library only: tests/native/wave_fanout.cpp
// drives it with g++ alone.  rcs = wa_fan_out(n, job, done [, spawn]):
//   job(i) -> int  once per i < n: job(0) on the calling thread, job(1..n-1) on a thread each, all started before job(0) begins.
//   done(i)        exactly once per i, on i's thread after job(i) returned or threw; where thread i cannot be started, on the calling thread
//                  before job(0) begins, for i and every later member, whose jobs never run.  done must not throw.
//   rcs[i]         what job(i) returned; -1 where it threw or never ran.  Nothing escapes a worker; every started thread is joined on return.
//   spawn(i, f) -> std::thread starts f (a test passes one that fails).  Throws only where rcs cannot be allocated: nothing has run then.
#pragma once

#include <thread>
#include <vector>

struct wa_spawn_thread { template <class F> std::thread operator()(int, F f) const { return std::thread(f); } };

template <class Job, class Done, class Spawn = wa_spawn_thread>
std::vector<int> wa_fan_out(int n, Job job, Done done, Spawn spawn = Spawn()) {
    std::vector<int> rcs((size_t) (n > 0 ? n : 0), -1);
    std::vector<std::thread> th;
    auto run = [&](int i) { try { rcs[(size_t) i] = job(i); } catch (...) { } done(i); };
    int k = 1;                                      // members k .. n-1 have no thread
    try {
        th.reserve(rcs.size());
        for (; k < n; ++k) th.push_back(spawn(k, [&run, k] { run(k); }));
    } catch (...) { }
    for (int i = k; i < n; ++i) done(i);
    if (n > 0) run(0);
    for (std::thread & t : th) t.join();
    return rcs;
}

// The pause rule and the device slot of the one-launch decode forms (whisper-rust_amd/csrc/wa_one_launch.h), on the CPU
// (tests/test_one_launch_rule.py).
#include "wa_one_launch.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>

static int n_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++n_fail; } } while (0)

static void pause_rule() {
    wa_launch_form f(true);
    CHECK(f.enabled() && f.usable() && f.take_pass());
    const int pauses[8] = { 64, 128, 256, 512, 1024, 2048, 2048, 2048 };
    for (int t = 0; t < 8; ++t) {
        CHECK(f.timed_out() == pauses[t]);
        for (int p = 0; p < pauses[t]; ++p) {          // paused: not usable, and every pass the form would serve counts the pause down
            CHECK(f.enabled() && !f.usable());
            CHECK(!f.take_pass());
        }
        CHECK(f.usable() && f.take_pass() && f.take_pass() && f.usable());      // re-armed
    }
    CHECK(f.timed_out() == 0);                        // the 9th time-out switches it off
    CHECK(!f.enabled() && !f.usable() && !f.take_pass());
    wa_launch_form g(true);
    g.disable();
    CHECK(!g.enabled() && !g.usable() && !g.take_pass());
    CHECK(!wa_launch_form().enabled());
}

static void device_slot() {
    wa_device_slot s;
    CHECK(s.try_acquire());
    CHECK(!s.try_acquire());                          // held
    { wa_slot_guard g(s, false); CHECK(!g.held()); }
    std::thread([&] { s.release(); }).join();         // given back on a thread that did not take it
    CHECK(s.try_acquire());
    s.release();
    { wa_slot_guard g(s, true); CHECK(g.held() && !s.try_acquire()); }
    CHECK(s.try_acquire());                           // the guard gave it back
    std::atomic<bool> got(false);
    std::thread waiter([&] { s.acquire(); got = true; });
    std::this_thread::sleep_for(std::chrono::milliseconds(200));
    CHECK(!got);                                      // a blocked acquire ...
    s.release();
    waiter.join();                                    // ... wakes when the slot is released
    CHECK(got && !s.try_acquire());
    s.release();
}

int main() {
    pause_rule();
    device_slot();
    std::printf("one_launch_rule: %d failures\n", n_fail);
    return n_fail ? 1 : 0;
}

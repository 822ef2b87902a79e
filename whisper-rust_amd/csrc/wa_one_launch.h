// wa_one_launch.h - the device slot and the pause rule of the one-launch decode forms (wa_decode.cpp).  Standard library only: a CPU test
// compiles it (tests/native/one_launch_rule.cpp).
#pragma once

#include <algorithm>
#include <condition_variable>
#include <mutex>

// Only one one-launch pass may run on a device at a time: its workgroups wait for each other, so two of them interleaved by the dispatcher
// could each hold CUs the other needs.  A binary semaphore, not a mutex: no thread owns it - a lock-step group takes it on the member thread
// that completes a request set and gives it back on the one that collects last (wa_decode.cpp: wa_batcher).
class wa_device_slot {
    std::mutex m_;
    std::condition_variable cv_;
    bool busy_ = false;
public:
    void acquire() { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [this] { return !busy_; }); busy_ = true; }
    bool try_acquire() { std::lock_guard<std::mutex> lk(m_); if (busy_) return false; busy_ = true; return true; }
    void release() { { std::lock_guard<std::mutex> lk(m_); busy_ = false; } cv_.notify_one(); }
};
// the slot for one launch and its synchronisation; wait = false: only if it is free (held() tells)
class wa_slot_guard {
    wa_device_slot & s_;
    const bool held_;
public:
    wa_slot_guard(wa_device_slot & s, bool wait) : s_(s), held_(wait ? (s.acquire(), true) : s.try_acquire()) {}
    ~wa_slot_guard() { if (held_) s_.release(); }
    wa_slot_guard(const wa_slot_guard &) = delete;
    bool held() const { return held_; }
};

// A one-launch form of the decode step and its pause rule.  A hand-off time-out (e.g. a co-tenant kernel held CUs: the step's workgroups
// were not all resident) pauses the form for 64, 128, 256, 512, 1024, 2048, 2048, 2048 decoder passes, which the launch sequence serves,
// then it is tried again; the 9th time-out switches it off.  Not synchronised: a state's forms belong to the thread that decodes it, a
// lock-step group's form to whoever holds the group's lock.
class wa_launch_form {
    bool on_;
    int pause_ = 0, timeouts_ = 0;
public:
    explicit wa_launch_form(bool on = false) : on_(on) {}
    bool enabled() const { return on_; }
    bool usable() const { return on_ && pause_ == 0; }           // (for gates that serve no pass: may a run-ahead window start?)
    // once for every decoder pass the form would serve: false while it is off or paused (a paused form counts that pass down)
    bool take_pass() { if (!on_) return false; if (pause_ > 0) { pause_ -= 1; return false; } return true; }
    // a hand-off timed out: the passes the form now pauses for, 0 when this time-out switched it off
    int timed_out() { timeouts_ += 1; if (timeouts_ > 8) { on_ = false; return 0; } pause_ = 32 << std::min(timeouts_, 6); return pause_; }
    void disable() { on_ = false; }                              // a launch or its stream failed
};

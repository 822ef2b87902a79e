// wave_fanout.cpp - driver of tests/test_wave_math.py: wa_fan_out (whisper-rust_amd/csrc/wa_fanout.h, nothing else of the product) under a
// stand-in for the lock-step batcher.  g++ alone, no HIP, no device.
//
// The stand-in keeps what matters of wa_decode.cpp's batcher: a member count that `leave` decrements, and steps that return only when every
// member that has not left has asked for one.  A member that never leaves therefore hangs the others (the test's timeout), one that leaves
// twice shows in the counts.  Member i takes 1 + i % 3 steps, so members leave at different times; the thrower throws after its first step.
//
//   wave_fanout                        every case: n in {1, 2, 8} x { plain, job t throws (every t), thread k cannot be started (every k >= 1) }
//   wave_fanout <n> <throw> <fail>     one case (-1: none)
// One line per case: what ran where, the returned codes, the done counts and the members left in the group.
#include "wa_fanout.h"

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <system_error>

struct group {
    std::mutex m;
    std::condition_variable cv;
    int members = 0, waiting = 0;
    long pass = 0;
    void release() { waiting = 0; ++pass; cv.notify_all(); }            // (m held) a pass serves everyone who waits
    void step() {
        std::unique_lock<std::mutex> lk(m);
        if (++waiting >= members) { release(); return; }
        const long p = pass;
        cv.wait(lk, [&] { return pass != p; });
    }
    void leave() {
        std::unique_lock<std::mutex> lk(m);
        --members;
        if (waiting > 0 && waiting >= members) release();
    }
};

static void print_list(const char * name, const std::vector<int> & v) {
    printf(" %s=", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? "," : "", v[i]);
}

static void run_case(int n, int throw_at, int fail_at) {
    group g;
    g.members = n;
    const std::thread::id caller = std::this_thread::get_id();
    std::vector<std::thread::id> job_tid((size_t) n), done_tid((size_t) n);
    std::vector<int> ran((size_t) n, 0), done((size_t) n, 0), done_before_job0((size_t) n, 0);
    bool job0_began = false;        // written and read on the calling thread only
    auto job = [&](int i) {
        if (i == 0) job0_began = true;
        ran[(size_t) i] += 1;
        job_tid[(size_t) i] = std::this_thread::get_id();
        for (int s = 0; s < 1 + i % 3; ++s) {
            g.step();
            if (i == throw_at) throw std::runtime_error("job");
        }
        return 100 + i;
    };
    auto leave = [&](int i) {
        done[(size_t) i] += 1;
        done_tid[(size_t) i] = std::this_thread::get_id();
        if (done_tid[(size_t) i] == caller && !job0_began) done_before_job0[(size_t) i] = 1;
        g.leave();
    };
    auto spawn = [&](int i, auto f) {
        if (i == fail_at) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "spawn");
        return std::thread(f);
    };
    const std::vector<int> rcs = wa_fan_out(n, job, leave, spawn);

    std::vector<int> on_caller((size_t) n, 0), done_on_job_thread((size_t) n, 0);
    for (size_t i = 0; i < (size_t) n; ++i) {
        on_caller[i] = ran[i] && job_tid[i] == caller ? 1 : 0;
        done_on_job_thread[i] = ran[i] && done[i] && done_tid[i] == job_tid[i] ? 1 : 0;
    }
    printf("case n=%d throw=%d fail=%d", n, throw_at, fail_at);
    print_list("rcs", rcs);
    print_list("ran", ran);
    print_list("done", done);
    print_list("on_caller", on_caller);
    print_list("done_on_job_thread", done_on_job_thread);
    print_list("done_before_job0", done_before_job0);
    printf(" members_left=%d\n", g.members);
    fflush(stdout);
}

int main(int argc, char ** argv) {
    if (argc == 4) { run_case(atoi(argv[1]), atoi(argv[2]), atoi(argv[3])); return 0; }
    if (argc != 1) { fprintf(stderr, "usage: %s [n throw_at fail_at]\n", argv[0]); return 2; }
    for (int n : { 1, 2, 8 }) {
        run_case(n, -1, -1);
        for (int t = 0; t < n; ++t) run_case(n, t, -1);
        for (int k = 1; k < n; ++k) run_case(n, -1, k);
        for (int k = 2; k < n; ++k) run_case(n, 1, k);          // a thrower among the members that did start
    }
    return 0;
}

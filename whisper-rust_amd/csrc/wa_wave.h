// wa_wave.h - the lock-step wave ("the wave protocol"): what every caller that sends several states through the batch decoder
// at once uses - whisper_amd_full_batch, whisper_full_parallel, wa_long_waves, step_many.
#pragma once

#include "wa_internal.h"

#include <functional>

// One wave: the members form their lock-step groups, job(i) runs for member i (wa_fanout.h: job(0) on the calling thread), every member leaves
// its group exactly once whatever became of its job, every thread is joined, and only then the groups end: ctx->batch_* hold THIS wave's
// counters.  Returns job's values; -1 for a job that threw or whose thread could not be started (the members that did start finish on their own).
std::vector<int> wa_wave_run(whisper_context * ctx, const std::vector<whisper_state *> & members, const std::function<int(size_t)> & job);

// ctx->batch_* over the waves of one call: add() after each wave, publish() at the end (nothing is written where no wave ran)
struct wa_wave_totals {
    long steps = 0, rows = 0, one_launch = 0, served = 0, waves = 0;
    void add(const whisper_context * c) { steps += c->batch_steps; rows += c->batch_rows; one_launch += c->batch_one_launch; served += c->batch_served; ++waves; }
    void publish(whisper_context * c) const { if (waves) { c->batch_steps = steps; c->batch_rows = rows; c->batch_one_launch = one_launch; c->batch_served = served; } }
};

void wa_state_add_counters(whisper_state & dst, const whisper_state & src);    // a member state's timers and counts onto the state that reports them
// a member's params: no callbacks, no progress, no realtime printing.  print_timestamps and print_special stay the caller's to clear:
// print_special decides whether special tokens go into a segment's text (wa_full.cpp), and whisper_full_parallel's parts keep the caller's.
void wa_params_silent(whisper_full_params & pc);

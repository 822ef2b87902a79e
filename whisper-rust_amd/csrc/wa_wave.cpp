// wa_wave.cpp - the lock-step wave (wa_wave.h; DESIGN.md 4.4, "the wave protocol").
#include "wa_wave.h"
#include "wa_fanout.h"

namespace {
// Lock-step decode groups for states transcribed together on one device: groups of WHISPER_AMD_BATCH_GROUP members share a decoder pass
// (wa_decode.cpp: wa_batcher).  Where the pass is ONE launch (wa_rows.hip; it owns the device while it runs) the default is one group of up
// to 8 - every weight row read once for eight tokens.  Where only the launch sequence is available (a pass is then a chain of short
// latency-bound launches) groups of 4 run side by side on their own streams: two 4-row passes finish sooner than one 8-row pass after the
// other (round 2: 8 chunks 488x real time as one group, 589x as two).  WHISPER_AMD_NO_BATCHER (read once) forms no groups at all.  The destructor
// OVERWRITES ctx->batch_* with this wave's counters and hands the batchers back to the context's cache: no member may still be running then.
struct wa_batch_groups {
    whisper_context * ctx;
    const std::vector<whisper_state *> & members;
    std::vector<wa_batcher *> bats;
    wa_batch_groups(whisper_context * c, const std::vector<whisper_state *> & m) : ctx(c), members(m) {
        static const bool off = getenv("WHISPER_AMD_NO_BATCHER") != nullptr;
        int group = !members.empty() && members[0]->rows_form.enabled() ? WA_MAX_DECODERS : 4;
        if (const char * g = getenv("WHISPER_AMD_BATCH_GROUP")) group = std::max(2, std::min(WA_MAX_DECODERS, atoi(g)));
        bats.reserve(members.size() / 2 + 1);       // nothing below throws: a group half made would never be taken apart
        for (size_t i0 = 0; i0 < members.size() && !off; i0 += group) {
            const size_t n = std::min((size_t) group, members.size() - i0);
            wa_batcher * b = wa_batcher_create(*ctx, (int) n);       // null for a group of one: that chunk decodes on its own (the members of a quantised group too, unless the one-launch form serves it)
            bats.push_back(b);
            for (size_t i = i0; i < i0 + n; ++i) members[i]->batcher = b;
        }
    }
    ~wa_batch_groups() {
        for (auto * st : members) st->batcher = nullptr;
        ctx->batch_steps = ctx->batch_rows = ctx->batch_one_launch = ctx->batch_served = 0;
        for (auto * b : bats) if (b) {
            long st_ = 0, rw_ = 0, ol_ = 0, sv_ = 0;
            wa_batcher_stats(b, &st_, &rw_, &ol_, &sv_);
            ctx->batch_steps += st_; ctx->batch_rows += rw_; ctx->batch_one_launch += ol_; ctx->batch_served += sv_;
            wa_batcher_destroy(b);
        }
    }
};
} // namespace

std::vector<int> wa_wave_run(whisper_context * ctx, const std::vector<whisper_state *> & members, const std::function<int(size_t)> & job) {
    wa_batch_groups groups(ctx, members);           // ends after wa_fan_out has joined every worker
    return wa_fan_out((int) members.size(), [&](int i) { return job((size_t) i); }, [&](int i) { wa_batcher_leave(members[(size_t) i]->batcher); });
}

void wa_state_add_counters(whisper_state & dst, const whisper_state & src) {
    dst.t_mel_us += src.t_mel_us; dst.t_sample_us += src.t_sample_us; dst.t_encode_us += src.t_encode_us; dst.t_decode_us += src.t_decode_us;
    dst.t_batchd_us += src.t_batchd_us; dst.t_prompt_us += src.t_prompt_us;
    dst.n_sample += src.n_sample; dst.n_encode += src.n_encode; dst.n_decode += src.n_decode; dst.n_batchd += src.n_batchd; dst.n_prompt += src.n_prompt;
}

void wa_params_silent(whisper_full_params & pc) {
    pc.print_progress = false; pc.print_realtime = false;
    pc.new_segment_callback = nullptr; pc.new_segment_callback_user_data = nullptr; pc.progress_callback = nullptr; pc.progress_callback_user_data = nullptr;
}

// wa_stream.cpp - live streaming sessions: the whisper_amd_stream_* entry points of include/whisper_amd.h.
//
// A session owns a state, a 16 kHz ring in HBM and the resampler's carry.  A feed is one launch of k_stream_push (wa_stream.hip) on the state's
// stream: the packet is converted and resampled behind the carry and every output that became final goes into the ring.  A step is one launch
// of k_stream_window - the ring pieces of the window that is due, copied into the state's PCM buffer - and whisper_full_with_state on that
// buffer, read in place, with the session's prompt.  step_many gathers the due windows of up to 8 sessions in ONE launch and runs them as
// one wave (wa_wave_run, wa_wave.h), as whisper_amd_full_batch runs its chunks.  The plan - which samples, how many, when a line is committed -
// is wa_stream.h's, a restatement of the reference's examples/stream/stream.cpp; wa_stream_ref there, the same push and gather on the host, serves WHISPER_AMD_STREAM_HOST=1
// (read when a session opens) and every session after a HIP call of its own failed: ring and carry are copied down once and stay on the host.
//
// A VAD session (whisper_amd_stream_open_vad) is the same object with another plan: no steps, but the utterances the Silero VAD
// cuts.  Its ring axis IS the absolute axis (nothing is dropped).  The new whole 512-sample windows of up to 8 sessions go through ONE launch of
// k_stream_vad_front (wa_vad.hip), which reads them where they lie in the rings and writes their gate inputs into the sessions' pinned buffers;
// the calling thread then walks each session's LSTM (wa_vad_step) and its incremental segmenter (wa_stream_vad.h).  An utterance that became
// final is queued; a step gathers it - the same k_stream_window launch - and runs whisper_full_with_state on it, as for a window.
#include "wa_wave.h"
#include "wa_stream.h"
#include "wa_stream_vad.h"

#include <climits>
#include <cstring>
#include <deque>

struct whisper_amd_stream {
    whisper_context * ctx = nullptr;
    whisper_state * st = nullptr;
    whisper_amd_stream_params prm;
    wa_stream_plan plan;
    wa_audio_plan ap;
    const float * d_taps = nullptr;
    int64_t cap = 0, backlog = 0;
    float * d_ring = nullptr;
    float * d_carry[2] = { nullptr, nullptr };      // [cur] holds the carry, the push writes the other
    int cur = 0;
    uint8_t * d_zero = nullptr;                     // K/2 zero frames: the flush packet
    int64_t T = 0, n_out = 0;                       // frames fed, outputs final
    bool ended = false, host = false;
    wa_stream_ref ref;                              // host == true: the carry and the ring live here
    std::vector<whisper_token> prompt, prompt_run;  // for the following windows / the one the last window ran with
    wa_stream_step last;                            // the last window
    int64_t windows = 0, feeds_device = 0, feeds_host = 0;
    // a VAD session
    bool vad = false;
    whisper_amd_stream_vad_params vprm;
    whisper_vad_context * vctx = nullptr;           // the caller's: weights and model, read only
    wa_svad_segmenter seg;
    wa_vad_lstm lstm;
    std::vector<float> probs;
    std::deque<wa_svad_out> due;                    // utterances that are final and have not run
    int64_t win_done = 0;                           // windows processed: the front end stands at sample 512 win_done
    bool tail_done = false;                         // the end of input has been processed: partial window and the segmenter's flush
    float * h_gates = nullptr; size_t h_gates_cap = 0;          // pinned, [windows][512]: k_stream_vad_front writes it
    float * d_stage = nullptr; size_t d_stage_cap = 0;          // host ring only: the new windows laid out linearly, and their gate inputs
    float * d_stage_out = nullptr; size_t d_stage_out_cap = 0;
    wa_svad_out last_utt;
    int64_t fe_launches = 0;
};

static int64_t stream_due(const whisper_amd_stream & S) { return S.vad ? (int64_t) S.due.size() : S.plan.due(S.ended); }

// of a packet, or (flush) of the zero frames behind the end of input, which travel in wa_audio_silence_format
static int packet_format(const whisper_amd_stream & S, bool flush) { return flush ? wa_audio_silence_format(S.prm.format) : S.prm.format; }
static size_t frame_bytes(const whisper_amd_stream & S, bool flush) { return wa_audio_frame_bytes(packet_format(S, flush), S.prm.channels); }

// a HIP call of this session failed: its carry and ring move to the host for good
static bool stream_to_host(whisper_amd_stream & S) {
    (void) hipGetLastError();
    if (!S.ref.init(S.prm.sample_rate, S.prm.channels, S.prm.format, S.cap)) return false;
    if (S.d_ring) {
        if (!WA_HIP_OK(hipStreamSynchronize(S.st->stream)) ||
            !WA_HIP_OK(hipMemcpy(S.ref.ring.data(), S.d_ring, (size_t) S.cap * sizeof(float), hipMemcpyDeviceToHost))) return false;
        if (!S.ref.carry.empty() &&
            !WA_HIP_OK(hipMemcpy(S.ref.carry.data(), S.d_carry[S.cur], S.ref.carry.size() * sizeof(float), hipMemcpyDeviceToHost))) return false;
    }
    S.host = true;
    return true;
}

static bool push_device(whisper_amd_stream & S, const void * data, bool on_device, int64_t n_frames, int64_t n_new, bool flush) {
    whisper_state & st = *S.st;
    const void * d_in = data;
    if (!on_device) {
        const size_t bytes = (size_t) n_frames * frame_bytes(S, flush);
        if (!wa_dev_reserve(st.d_audio_in, st.d_audio_in_cap, bytes)) return false;
        if (!WA_HIP_OK(hipMemcpyAsync(st.d_audio_in, data, bytes, hipMemcpyHostToDevice, st.stream))) return false;
        d_in = st.d_audio_in;
    }
    const int format = packet_format(S, flush);
    if (!(wa_audio_format_base(format) ? wa_stream_push_launch : wa_stream_push_fmt_launch)(st.stream, d_in, n_frames, S.prm.channels, format, S.ap, S.d_taps, S.T,
                                                                                            S.d_carry[S.cur], S.d_carry[S.cur ^ 1], S.n_out, n_new, S.d_ring,
                                                                                            S.cap, S.plan.r_w)) return false;
    // the caller may release a host buffer on return; device input stays stream-ordered
    if (!on_device && !WA_HIP_OK(hipStreamSynchronize(st.stream))) return false;
    if (S.ap.K) S.cur ^= 1;
    return true;
}

static bool push_host(whisper_amd_stream & S, const void * data, bool on_device, int64_t n_frames, int64_t n_new, bool flush) {
    std::vector<uint8_t> in;
    if (on_device) {
        in.resize((size_t) n_frames * frame_bytes(S, flush));
        if (!WA_HIP_OK(hipStreamSynchronize(S.st->stream)) || !WA_HIP_OK(hipMemcpy(in.data(), data, in.size(), hipMemcpyDeviceToHost))) return false;
        data = in.data();
    }
    std::vector<float> out((size_t) std::max<int64_t>(n_new, 1));
    S.ref.T = S.T; S.ref.n_out = S.n_out;
    S.ref.format = packet_format(S, flush);
    const bool pushed = S.ref.push(data, n_frames, out.data()) == n_new;
    S.ref.format = S.prm.format;
    if (!pushed) return false;
    S.ref.ring_write(S.plan.r_w, out.data(), n_new);
    return true;
}

// ---- VAD sessions ----
// the oldest sample a VAD session still needs: the first utterance that is due, else the open speech or candidate (with its pad and the
// centisecond rounding's slack), else the first window not yet processed
static int64_t vad_keep_from(const whisper_amd_stream & S) {
    int64_t k = S.win_done * WA_VAD_WINDOW;
    const int64_t slack = S.seg.speech_pad_samples + 160;
    if (S.seg.is_speech_segment) k = std::min<int64_t>(k, S.seg.curr_speech_start - slack);
    if (S.seg.has_cur) k = std::min<int64_t>(k, S.seg.cur_start - slack);
    if (!S.due.empty()) k = std::min<int64_t>(k, wa_svad_range_of(S.due.front().seg, -1).start);
    return std::max<int64_t>(k, 0);
}

// the windows a session has not processed: whole ones, and after the end of input the partial one
static int vad_new_windows(const whisper_amd_stream & S, int & n_valid) {
    const int64_t have = S.plan.r_w - S.win_done * WA_VAD_WINDOW;
    int64_t n = have / WA_VAD_WINDOW + (S.ended && have % WA_VAD_WINDOW > 0 ? 1 : 0);
    n = std::min<int64_t>(n, WA_SVAD_MAX_WINDOWS);
    n_valid = (int) std::min<int64_t>(n * WA_VAD_WINDOW, have);
    return (int) n;
}

// gate inputs of n windows -> probabilities -> segmenter; then, at the end of input, the segmenter's flush
static void vad_consume(whisper_amd_stream & S, const float * gates, int n) {
    const wa_vad_model & m = wa_vad_ctx_model(S.vctx);
    std::vector<wa_svad_out> out;
    for (int k = 0; k < n; ++k) {
        const float p = wa_vad_step(m, S.lstm, gates + (size_t) k * WA_VAD_GATES);
        S.probs.push_back(p);
        S.seg.push(p, out);
    }
    S.win_done += n;
    if (S.ended && !S.tail_done && S.win_done * WA_VAD_WINDOW >= S.plan.r_w) { S.seg.flush(S.plan.r_w, out); S.tail_done = true; }
    for (const wa_svad_out & o : out) S.due.push_back(o);
}

// a session whose ring is on the host: its new windows staged linearly, the whole-recording front end on them
static bool vad_front_host(whisper_amd_stream & S, int n, int n_valid) {
    std::vector<float> lin((size_t) n * WA_VAD_WINDOW, 0.0f), gates((size_t) n * WA_VAD_GATES);
    int32_t slot[2], plen[2];
    const int np = wa_stream_ring_pieces(S.win_done * WA_VAD_WINDOW, n_valid, S.cap, slot, plen);
    S.ref.gather(np, slot, plen, lin.data());
    hipStream_t q = S.st->stream;
    if (!wa_dev_reserve(S.d_stage, S.d_stage_cap, lin.size()) || !wa_dev_reserve(S.d_stage_out, S.d_stage_out_cap, gates.size())) return false;
    if (!WA_HIP_OK(hipMemcpyAsync(S.d_stage, lin.data(), lin.size() * sizeof(float), hipMemcpyHostToDevice, q))) return false;
    if (!wa_vad_front_launch(wa_vad_ctx_dev(S.vctx), S.d_stage, n_valid, n, S.d_stage_out, (void *) q)) return false;
    S.fe_launches++;
    if (!WA_HIP_OK(hipMemcpyAsync(gates.data(), S.d_stage_out, gates.size() * sizeof(float), hipMemcpyDeviceToHost, q)) || !WA_HIP_OK(hipStreamSynchronize(q))) return false;
    vad_consume(S, gates.data(), n);
    return true;
}

// the new windows of every session of `ss` (VAD sessions of one context and one vctx): one k_stream_vad_front launch per group of 8
static bool vad_process(whisper_amd_stream ** ss, int n) {
    if (!WA_HIP_OK(hipSetDevice(ss[0]->ctx->device))) return false;
    for (bool again = true; again; ) {
        again = false;
        for (int g0 = 0; g0 < n; g0 += WA_SVAD_SESSIONS) {
            const int gn = std::min(WA_SVAD_SESSIONS, n - g0);
            wa_svad_table tab;
            memset(&tab, 0, sizeof(tab));
            whisper_amd_stream * row[WA_SVAD_SESSIONS];
            int cnt[WA_SVAD_SESSIONS], nr = 0;
            for (int i = 0; i < gn; ++i) {
                whisper_amd_stream & S = *ss[g0 + i];
                int n_valid = 0;
                const int nw = vad_new_windows(S, n_valid);
                if (nw == 0) {          // nothing new; the end of input may still close an open speech
                    if (S.ended && !S.tail_done) vad_consume(S, nullptr, 0);
                    continue;
                }
                if (nw == WA_SVAD_MAX_WINDOWS) again = true;
                if (!S.host) {
                    if (S.h_gates_cap < (size_t) nw * WA_VAD_GATES) {
                        if (S.h_gates) { (void) hipHostFree(S.h_gates); S.h_gates = nullptr; S.h_gates_cap = 0; }
                        const size_t want = std::max<size_t>((size_t) nw, 64) * WA_VAD_GATES;
                        if (WA_HIP_OK(hipHostMalloc((void **) &S.h_gates, want * sizeof(float), hipHostMallocDefault))) S.h_gates_cap = want;
                        else { S.h_gates = nullptr; WA_WARN("%s: no pinned buffer, session %d continues on the host\n", __func__, g0 + i); if (!stream_to_host(S)) return false; }
                    }
                }
                if (S.host) { if (!vad_front_host(S, nw, n_valid)) return false; continue; }
                wa_svad_session & z = tab.s[nr];
                z.ring = S.d_ring; z.out = S.h_gates; z.cap = (int32_t) S.cap; z.slot = (int32_t) ((S.win_done * WA_VAD_WINDOW) % S.cap); z.n_valid = n_valid;
                tab.first[nr + 1] = tab.first[nr] + nw;
                row[nr] = &S; cnt[nr] = nw; ++nr;
            }
            if (nr == 0) continue;
            tab.n_sessions = nr;
            hipStream_t q = row[0]->st->stream;
            bool ok = true;
            // the pushes that wrote the rings ran on their own states' streams: the joint launch runs on ONE member's
            for (int i = 1; i < nr && ok; ++i) ok = WA_HIP_OK(hipStreamSynchronize(row[i]->st->stream));
            ok = ok && wa_svad_front_launch(wa_vad_ctx_dev(row[0]->vctx), tab, (void *) q) && WA_HIP_OK(hipStreamSynchronize(q));
            if (ok) {
                for (int i = 0; i < nr; ++i) { row[i]->fe_launches++; vad_consume(*row[i], row[i]->h_gates, cnt[i]); }
            } else {
                for (int i = 0; i < nr; ++i) {
                    WA_WARN("%s: the device front end failed, session continues on the host\n", __func__);
                    int n_valid = 0;
                    if (!stream_to_host(*row[i])) return false;
                    const int nw = vad_new_windows(*row[i], n_valid);
                    if (!vad_front_host(*row[i], nw, n_valid)) return false;
                }
            }
        }
    }
    return true;
}

// the next window (step mode) or utterance (VAD mode) of a session, as the step the gather and window_done take
static bool stream_next(whisper_amd_stream & S, wa_stream_step & s) {
    if (!S.vad) return wa_stream_next(S.plan, S.ended, s);
    s = wa_stream_step();
    while (!S.due.empty()) {
        const wa_svad_out o = S.due.front();
        const wa_svad_range r = wa_svad_range_of(o.seg, S.plan.r_w);
        S.due.pop_front();
        if (r.len <= 0 || r.len > S.seg.cap_samples || S.plan.r_w - r.start > S.cap) {      // empty, or (never, by the feed's rule) no longer in the ring
            if (r.len > 0) WA_ERROR("%s: an utterance of %lld samples at %lld is not served\n", __func__, (long long) r.len, (long long) r.start);
            continue;
        }
        s.take = 0; s.n_new = (int) r.len; s.len = (int) r.len; s.commit = true; s.r0 = r.start;
        s.ranges.push_back({ r.start, r.len });
        S.last_utt = o;
        S.plan.r_old = r.start + r.len;
        return true;
    }
    return false;
}

// a packet, or (flush) the K/2 zero frames behind the end of input
static int stream_push(whisper_amd_stream & S, const void * data, int64_t n_frames, bool flush) {
    const int64_t n_new = wa_stream_final(S.ap, S.T + n_frames) - S.n_out;
    if (S.vad) {
        if (S.plan.r_w + n_new - vad_keep_from(S) > S.cap) {
            WA_ERROR("%s: refused: %lld new samples would overwrite audio from sample %lld on that is still needed (ring of %lld, write head %lld)\n", __func__,
                     (long long) n_new, (long long) vad_keep_from(S), (long long) S.cap, (long long) S.plan.r_w);
            return WHISPER_AMD_STREAM_FULL;
        }
        if ((S.plan.r_w + n_new) / WA_VAD_WINDOW > INT_MAX / WA_VAD_WINDOW - 8) {
            WA_ERROR("%s: refused: the session's sample axis is at its end; reset it\n", __func__);
            return WHISPER_AMD_STREAM_FAILED;
        }
    } else if (S.plan.pending() + n_new > S.backlog) {
        if (!S.prm.drop_late || n_new > S.backlog) {
            WA_ERROR("%s: refused: %lld new samples beside %lld pending do not fit a backlog of %lld\n", __func__, (long long) n_new,
                     (long long) S.plan.pending(), (long long) S.backlog);
            return WHISPER_AMD_STREAM_FULL;
        }
        WA_WARN("%s: cannot process audio fast enough, dropping %lld samples\n", __func__, (long long) S.plan.pending());
        S.plan.drop_pending();
    }
    if (!WA_HIP_OK(hipSetDevice(S.ctx->device))) return WHISPER_AMD_STREAM_FAILED;
    const bool on_device = wa_is_device_ptr(data);
    bool served = false;
    if (!S.host) {
        served = push_device(S, data, on_device, n_frames, n_new, flush);
        if (served) S.feeds_device++;
        else {
            WA_WARN("%s: the device path failed, this session continues on the host\n", __func__);
            if (!stream_to_host(S)) { WA_ERROR("%s: the ring could not be copied to the host\n", __func__); return WHISPER_AMD_STREAM_FAILED; }
        }
    }
    if (!served) {
        if (!push_host(S, data, on_device, n_frames, n_new, flush)) { WA_ERROR("%s: the host path failed\n", __func__); return WHISPER_AMD_STREAM_FAILED; }
        S.feeds_host++;
    }
    if (!flush) S.T += n_frames;
    S.n_out += n_new;
    S.plan.r_w += n_new;
    if (S.vad) {
        if (S.vprm.vad_on_feed) {
            whisper_amd_stream * one = &S;
            if (!vad_process(&one, 1)) return WHISPER_AMD_STREAM_FAILED;
        }
        return (int) S.due.size();
    }
    return (int) S.plan.due(S.ended || flush);
}

// the window's ring pieces as a row of the gather kernel's table
static wa_stream_window window_row(const whisper_amd_stream & S, const wa_stream_step & step) {
    wa_stream_window w;
    memset(&w, 0, sizeof(w));
    w.ring = S.d_ring; w.dst = S.st->d_audio; w.len = step.len;
    w.n_pieces = wa_stream_ring_pieces(step.r0, step.len, S.cap, w.slot, w.plen);
    return w;
}

static bool gather_host(whisper_amd_stream & S, const wa_stream_step & step) {
    std::vector<float> win((size_t) step.len);
    int32_t slot[2], plen[2];
    const int n = wa_stream_ring_pieces(step.r0, step.len, S.cap, slot, plen);
    S.ref.gather(n, slot, plen, win.data());
    return WA_HIP_OK(hipMemcpyAsync(S.st->d_audio, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice, S.st->stream)) &&
           WA_HIP_OK(hipStreamSynchronize(S.st->stream));
}

// the windows of `due` (at most WA_STREAM_SESSIONS) into their states' PCM buffers: one launch for those whose ring is on the device
static bool gather(const std::vector<whisper_amd_stream *> & due, const std::vector<wa_stream_step> & steps) {
    wa_stream_windows tab;
    memset(&tab, 0, sizeof(tab));
    int n = 0;
    whisper_amd_stream * first = nullptr;
    for (size_t i = 0; i < due.size(); ++i) if (!due[i]->host) {
        // pushes of device input are not synchronised: the joint launch runs on ONE member's stream
        if (due.size() > 1 && !WA_HIP_OK(hipStreamSynchronize(due[i]->st->stream))) return false;
        if (!first) first = due[i];
        tab.w[n++] = window_row(*due[i], steps[i]);
    }
    if (n > 0) {
        bool ok = wa_stream_window_launch(first->st->stream, tab, n);
        // complete before a lock-step group starts: a foreign kernel beside the one-launch passes costs hand-off time-outs
        if (ok && due.size() > 1) ok = WA_HIP_OK(hipStreamSynchronize(first->st->stream));
        if (!ok) {
            for (size_t i = 0; i < due.size(); ++i) if (!due[i]->host) {
                WA_WARN("%s: the device gather failed, session %d continues on the host\n", __func__, (int) i);
                if (!stream_to_host(*due[i])) return false;
            }
        }
    }
    for (size_t i = 0; i < due.size(); ++i) if (due[i]->host && !gather_host(*due[i], steps[i])) return false;
    return true;
}

static whisper_full_params window_params(whisper_amd_stream & S, const whisper_full_params & params) {
    whisper_full_params pc = params;
    S.prompt_run = S.prompt;
    if (S.prm.carry_prompt) { pc.prompt_tokens = S.prompt_run.empty() ? nullptr : S.prompt_run.data(); pc.prompt_n_tokens = (int) S.prompt_run.size(); }
    else {
        S.prompt_run.clear();
        if (params.prompt_tokens && params.prompt_n_tokens > 0) S.prompt_run.assign(params.prompt_tokens, params.prompt_tokens + params.prompt_n_tokens);
    }
    return pc;
}

static void window_done(whisper_amd_stream & S, const wa_stream_step & step, int rc) {
    S.last = step;
    S.windows++;
    if (rc == 0 && step.commit && S.prm.carry_prompt) {
        S.prompt.clear();
        for (const wa_segment & seg : S.st->result_all) for (const whisper_token_data & t : seg.tokens) S.prompt.push_back(t.id);
    }
}

static int step_many(whisper_amd_stream ** ss, int n, const whisper_full_params & params) {
    whisper_context * ctx = ss[0]->ctx;
    if (!WA_HIP_OK(hipSetDevice(ctx->device))) return WHISPER_AMD_STREAM_FAILED;
    std::vector<whisper_amd_stream *> due;
    std::vector<wa_stream_step> steps;
    for (int i = 0; i < n; ++i) {
        wa_stream_step s;
        if (stream_next(*ss[i], s)) { due.push_back(ss[i]); steps.push_back(s); }
        else if (s.dropped > 0) WA_WARN("%s: cannot process audio fast enough, dropped %lld samples\n", __func__, (long long) s.dropped);
    }
    int ran = 0, bad = 0;
    wa_wave_totals totals;
    for (size_t g0 = 0; g0 < due.size(); g0 += WA_STREAM_SESSIONS) {
        const size_t gn = std::min<size_t>(WA_STREAM_SESSIONS, due.size() - g0);
        const std::vector<whisper_amd_stream *> grp(due.begin() + g0, due.begin() + g0 + gn);
        const std::vector<wa_stream_step> gst(steps.begin() + g0, steps.begin() + g0 + gn);
        std::vector<int> rcs(gn, WHISPER_AMD_STREAM_FAILED);
        if (gather(grp, gst)) {
            std::vector<whisper_state *> members;
            std::vector<whisper_full_params> pcs;
            for (whisper_amd_stream * S : grp) {
                members.push_back(S->st);
                whisper_full_params pc = window_params(*S, params);        // a copy per member: the prompts differ
                wa_params_silent(pc);
                pc.print_timestamps = false; pc.print_special = false;     // print_special: no special tokens in a window's text (wa_full.cpp)
                pcs.push_back(pc);
            }
            rcs = wa_wave_run(ctx, members, [&](size_t i) { return whisper_full_with_state(ctx, members[i], pcs[i], members[i]->d_audio, gst[i].len); });
            totals.add(ctx);
        } else WA_ERROR("%s: the window gather failed\n", __func__);
        for (size_t i = 0; i < gn; ++i) {
            window_done(*grp[i], gst[i], rcs[i]);
            if (rcs[i] == 0) ++ran; else if (!bad) bad = rcs[i] < 0 ? rcs[i] : WHISPER_AMD_STREAM_FAILED;
        }
    }
    totals.publish(ctx);
    return bad ? bad : ran;
}

static void stream_free(whisper_amd_stream * s) {
    if (!s) return;
    if (s->ctx) (void) hipSetDevice(s->ctx->device);
    if (s->st && s->st->stream) (void) hipStreamSynchronize(s->st->stream);
    if (s->d_ring) (void) hipFree(s->d_ring);
    if (s->d_carry[0]) (void) hipFree(s->d_carry[0]);
    if (s->d_carry[1]) (void) hipFree(s->d_carry[1]);
    if (s->d_zero) (void) hipFree(s->d_zero);
    if (s->h_gates) (void) hipHostFree(s->h_gates);
    if (s->d_stage) (void) hipFree(s->d_stage);
    if (s->d_stage_out) (void) hipFree(s->d_stage_out);
    if (s->st) whisper_free_state(s->st);
    delete s;
}

static bool stream_clear(whisper_amd_stream & S) {
    S.plan.reset();
    S.T = 0; S.n_out = 0; S.ended = false; S.cur = 0;
    S.prompt.clear(); S.prompt_run.clear();
    S.last = wa_stream_step(); S.windows = 0;
    if (S.vad) {
        S.seg.reset(); S.lstm.reset(); S.probs.clear(); S.due.clear();
        S.win_done = 0; S.tail_done = false; S.last_utt = wa_svad_out(); S.fe_launches = 0;
    }
    if (S.host) { S.ref.reset(); return true; }
    const size_t C = (size_t) std::max(wa_stream_carry_len(S.ap), 1);
    return WA_HIP_OK(hipMemsetAsync(S.d_carry[0], 0, C * sizeof(float), S.st->stream)) &&
           WA_HIP_OK(hipMemsetAsync(S.d_carry[1], 0, C * sizeof(float), S.st->stream));
}

// the state, its PCM buffer, ring and carry of a session whose sizes are set; nullptr (the session freed) when nothing can serve it
static whisper_amd_stream * stream_make(whisper_amd_stream * s, size_t pcm_floats) {
    whisper_context * ctx = s->ctx;
    const char * env = getenv("WHISPER_AMD_STREAM_HOST");
    if (!WA_HIP_OK(hipSetDevice(ctx->device)) || !(s->st = whisper_init_state(ctx))) { stream_free(s); return nullptr; }
    if (!wa_dev_reserve(s->st->d_audio, s->st->d_audio_cap, pcm_floats)) { stream_free(s); return nullptr; }
    if (env && atoi(env) != 0) {
        if (!stream_to_host(*s)) { stream_free(s); return nullptr; }
        return s;
    }
    const size_t C = (size_t) std::max(wa_stream_carry_len(s->ap), 1), zb = (size_t) std::max(wa_stream_flush_frames(s->ap), 1) * frame_bytes(*s, true);
    bool ok = (!s->ap.K || (s->d_taps = wa_audio_taps_device(*ctx, s->ap)))
           && WA_HIP_OK(hipMalloc((void **) &s->d_ring, (size_t) s->cap * sizeof(float)))
           && WA_HIP_OK(hipMalloc((void **) &s->d_carry[0], C * sizeof(float))) && WA_HIP_OK(hipMalloc((void **) &s->d_carry[1], C * sizeof(float)))
           && WA_HIP_OK(hipMalloc((void **) &s->d_zero, zb)) && WA_HIP_OK(hipMemsetAsync(s->d_zero, 0, zb, s->st->stream))
           && WA_HIP_OK(hipMemsetAsync(s->d_ring, 0, (size_t) s->cap * sizeof(float), s->st->stream)) && stream_clear(*s);
    if (!ok) {          // no device ring: the session lives on the host from the start
        WA_WARN("%s: the device buffers could not be made, this session runs on the host\n", __func__);
        if (s->d_ring) { (void) hipFree(s->d_ring); s->d_ring = nullptr; }
        if (!stream_to_host(*s)) { stream_free(s); return nullptr; }
    }
    return s;
}

extern "C" {

void whisper_amd_stream_default_params(struct whisper_amd_stream_params * p) {
    if (!p) return;
    p->step_ms = 3000; p->length_ms = 10000; p->keep_ms = 200; p->sample_rate = WA_AUDIO_RATE; p->channels = 1; p->format = WHISPER_AMD_PCM_F32;
    p->backlog_ms = 30000; p->carry_prompt = 1; p->drop_late = 0;
}

struct whisper_amd_stream * whisper_amd_stream_open(struct whisper_context * ctx, const struct whisper_amd_stream_params * p) {
    if (!ctx || !p) { WA_ERROR("%s: refused: null context or params\n", __func__); return nullptr; }
    wa_stream_sizes z;
    if (!wa_audio_args_ok(nullptr, 0, p->channels, p->sample_rate, p->format)) {
        WA_ERROR("%s: refused: %d channels, %d Hz, format %d\n", __func__, p->channels, p->sample_rate, p->format);
        return nullptr;
    }
    if (!wa_stream_sizes_make(p->step_ms, p->length_ms, p->keep_ms, z) || p->backlog_ms < 0) {
        WA_ERROR("%s: refused: step %d ms, length %d ms, keep %d ms, backlog %d ms (step > 0, keep + length <= %d after the clamps)\n", __func__, p->step_ms,
                 p->length_ms, p->keep_ms, p->backlog_ms, WA_STREAM_MAX_WINDOW_MS);
        return nullptr;
    }
    whisper_amd_stream * s = nullptr;
    const bool ok = wa_guard(__func__, false, [&] {
        s = new whisper_amd_stream;
        s->ctx = ctx; s->prm = *p; s->plan.z = z; s->plan.drop_late = p->drop_late != 0;
        wa_audio_plan_make(p->sample_rate, s->ap);
        s->backlog = std::max<int64_t>((int64_t) p->backlog_ms * (WA_AUDIO_RATE / 1000), 2 * (int64_t) z.n_step + 1);   // the drop rule needs to see 2 n_step + 1
        s->cap = (int64_t) z.n_keep + z.n_len + s->backlog;
        s = stream_make(s, (size_t) std::max(z.n_keep + z.n_len, 256));
        return true;
    });
    if (ok) return s;           // null where stream_make failed: it has freed the session
    stream_free(s);
    return nullptr;
}

void whisper_amd_stream_close(struct whisper_amd_stream * s) { (void) wa_guard(__func__, 0, [&] { stream_free(s); return 0; }); }

int whisper_amd_stream_feed(struct whisper_amd_stream * s, const void * data, int64_t n_frames) {
    if (!s || n_frames < 0 || (!data && n_frames > 0) || n_frames > INT64_MAX / WA_AUDIO_MAX_L / 2) {
        WA_ERROR("%s: refused: null session or data, or a bad frame count\n", __func__);
        return WHISPER_AMD_STREAM_BAD_ARGS;
    }
    if (s->ended) { WA_ERROR("%s: refused: the session was flushed; reset it first\n", __func__); return WHISPER_AMD_STREAM_ENDED; }
    return wa_guard(__func__, WHISPER_AMD_STREAM_FAILED, [&] {
        return n_frames == 0 ? (int) (s->vad ? stream_due(*s) : s->plan.due(false)) : stream_push(*s, data, n_frames, false);
    });
}

int whisper_amd_stream_flush(struct whisper_amd_stream * s) {
    if (!s) { WA_ERROR("%s: refused: null session\n", __func__); return WHISPER_AMD_STREAM_BAD_ARGS; }
    return wa_guard(__func__, WHISPER_AMD_STREAM_FAILED, [&]() -> int {
        if (!s->ended) {
            const int Z = wa_stream_flush_frames(s->ap);
            if (Z > 0) {
                const std::vector<uint8_t> zeros((size_t) Z * frame_bytes(*s, true), 0);
                const int rc = stream_push(*s, s->host ? (const void *) zeros.data() : (const void *) s->d_zero, Z, true);
                if (rc < 0) return rc;
            }
            s->ended = true;
            if (s->vad && s->vprm.vad_on_feed && !vad_process(&s, 1)) return WHISPER_AMD_STREAM_FAILED;
        }
        return (int) (s->vad ? stream_due(*s) : s->plan.due(true));
    });
}

int whisper_amd_stream_pending(struct whisper_amd_stream * s) { return s ? (int) stream_due(*s) : WHISPER_AMD_STREAM_BAD_ARGS; }

int whisper_amd_stream_step_many(struct whisper_amd_stream ** ss, int n, const struct whisper_full_params * params) {
    if (!ss || !params || n <= 0) { WA_ERROR("%s: refused: null or empty arguments\n", __func__); return WHISPER_AMD_STREAM_BAD_ARGS; }
    if (n > 64) { WA_ERROR("%s: refused: %d sessions are more than 64\n", __func__, n); return WHISPER_AMD_STREAM_MIXED; }
    for (int i = 0; i < n; ++i) {
        if (!ss[i]) { WA_ERROR("%s: refused: session %d is null\n", __func__, i); return WHISPER_AMD_STREAM_BAD_ARGS; }
        if (ss[i]->ctx != ss[0]->ctx) { WA_ERROR("%s: refused: session %d belongs to another context\n", __func__, i); return WHISPER_AMD_STREAM_MIXED; }
        for (int j = 0; j < i; ++j) if (ss[j] == ss[i]) { WA_ERROR("%s: refused: session %d is listed twice\n", __func__, i); return WHISPER_AMD_STREAM_BAD_ARGS; }
    }
    return wa_guard(__func__, WHISPER_AMD_STREAM_FAILED, [&] { return step_many(ss, n, *params); });
}

int whisper_amd_stream_step(struct whisper_amd_stream * s, const struct whisper_full_params * params) {
    if (!s || !params) { WA_ERROR("%s: refused: null session or params\n", __func__); return WHISPER_AMD_STREAM_BAD_ARGS; }
    const char * const who = __func__;
    return wa_guard(who, WHISPER_AMD_STREAM_FAILED, [&]() -> int {
        if (!WA_HIP_OK(hipSetDevice(s->ctx->device))) return WHISPER_AMD_STREAM_FAILED;
        wa_stream_step step;
        if (!stream_next(*s, step)) {
            if (step.dropped > 0) WA_WARN("%s: cannot process audio fast enough, dropped %lld samples\n", who, (long long) step.dropped);
            return 0;
        }
        int rc = WHISPER_AMD_STREAM_FAILED;
        if (gather({ s }, { step })) {
            const whisper_full_params pc = window_params(*s, *params);      // the caller's, but for the prompt
            rc = whisper_full_with_state(s->ctx, s->st, pc, s->st->d_audio, step.len);
        } else WA_ERROR("%s: the window gather failed\n", who);
        window_done(*s, step, rc);
        return rc == 0 ? 1 : rc < 0 ? rc : WHISPER_AMD_STREAM_FAILED;
    });
}

struct whisper_state * whisper_amd_stream_state(struct whisper_amd_stream * s) { return s ? s->st : nullptr; }

int whisper_amd_stream_info(struct whisper_amd_stream * s, int64_t out[10]) {
    if (!s || !out) return WHISPER_AMD_STREAM_BAD_ARGS;
    out[0] = s->windows;
    out[1] = s->last.ranges.empty() ? 0 : s->last.ranges[0].start;
    out[2] = s->last.len; out[3] = s->last.take; out[4] = s->last.commit ? 1 : 0;
    out[5] = (int64_t) s->prompt_run.size();
    out[6] = s->plan.dropped; out[7] = stream_due(*s); out[8] = s->feeds_device; out[9] = s->feeds_host;
    return 0;
}

int64_t whisper_amd_stream_window_copy(struct whisper_amd_stream * s, float * dst, int64_t cap) {
    if (!s || cap < 0 || (cap > 0 && !dst)) return WHISPER_AMD_STREAM_BAD_ARGS;
    const int64_t n = std::min<int64_t>(cap, s->last.len);
    if (!WA_HIP_OK(hipSetDevice(s->ctx->device)) || !WA_HIP_OK(hipStreamSynchronize(s->st->stream))) return WHISPER_AMD_STREAM_FAILED;
    if (n > 0 && !WA_HIP_OK(hipMemcpy(dst, s->st->d_audio, (size_t) n * sizeof(float), hipMemcpyDeviceToHost))) return WHISPER_AMD_STREAM_FAILED;
    return s->last.len;
}

int whisper_amd_stream_prompt_copy(struct whisper_amd_stream * s, whisper_token * dst, int cap) {
    if (!s || cap < 0 || (cap > 0 && !dst)) return WHISPER_AMD_STREAM_BAD_ARGS;
    const int n = std::min(cap, (int) s->prompt_run.size());
    if (n > 0) memcpy(dst, s->prompt_run.data(), (size_t) n * sizeof(whisper_token));
    return (int) s->prompt_run.size();
}

void whisper_amd_stream_reset(struct whisper_amd_stream * s) {
    if (!s) return;
    (void) wa_guard(__func__, 0, [&] {
        (void) hipSetDevice(s->ctx->device);
        if (!stream_clear(*s)) WA_ERROR("whisper_amd_stream_reset: the carry could not be cleared\n");
        s->st->result_all.clear();
        s->st->prompt_past.clear();
        return 0;
    });
}

int whisper_amd_stream_tile(void) { return WA_STREAM_TILE; }

// ---- VAD sessions ----
void whisper_amd_stream_vad_default_params(struct whisper_amd_stream_vad_params * p) {
    if (!p) return;
    p->sample_rate = WA_AUDIO_RATE; p->channels = 1; p->format = WHISPER_AMD_PCM_F32; p->backlog_ms = 40000; p->carry_prompt = 0;
    p->max_utterance_ms = WA_SVAD_MAX_UTTERANCE_MS; p->vad_on_feed = 1;
    p->vad = whisper_vad_default_params();
    p->vad.max_speech_duration_s = 30.0f;
}

struct whisper_amd_stream * whisper_amd_stream_open_vad(struct whisper_context * ctx, struct whisper_vad_context * vctx,
                                                         const struct whisper_amd_stream_vad_params * p) {
    if (!ctx || !vctx || !p) { WA_ERROR("%s: refused: null context, VAD context or params\n", __func__); return nullptr; }
    if (!wa_audio_args_ok(nullptr, 0, p->channels, p->sample_rate, p->format)) {
        WA_ERROR("%s: refused: %d channels, %d Hz, format %d\n", __func__, p->channels, p->sample_rate, p->format);
        return nullptr;
    }
    const char * why = nullptr;
    if (!wa_svad_params_ok(p->vad, p->max_utterance_ms, &why)) { WA_ERROR("%s: refused: %s\n", __func__, why); return nullptr; }
    if (p->backlog_ms < 0 || p->backlog_ms > 3600000) { WA_ERROR("%s: refused: a backlog of %d ms\n", __func__, p->backlog_ms); return nullptr; }
    if (wa_vad_ctx_device(vctx) != ctx->device) {
        WA_ERROR("%s: refused: the VAD context lives on device %d, the context on device %d\n", __func__, wa_vad_ctx_device(vctx), ctx->device);
        return nullptr;
    }
    whisper_amd_stream * s = nullptr;
    const bool ok = wa_guard(__func__, false, [&] {
        s = new whisper_amd_stream;
        s->ctx = ctx; s->vad = true; s->vprm = *p; s->vctx = vctx;
        whisper_amd_stream_default_params(&s->prm);
        s->prm.sample_rate = p->sample_rate; s->prm.channels = p->channels; s->prm.format = p->format; s->prm.backlog_ms = p->backlog_ms;
        s->prm.carry_prompt = p->carry_prompt; s->prm.drop_late = 0;
        s->seg.init(p->vad, p->max_utterance_ms);
        s->lstm.reset();
        wa_audio_plan_make(p->sample_rate, s->ap);
        // an open speech of the cap's length and a candidate behind it, up to max_speech long, must fit beside one another
        s->backlog = std::max<int64_t>((int64_t) p->backlog_ms * (WA_AUDIO_RATE / 1000), (int64_t) WA_AUDIO_RATE * (int64_t) p->vad.max_speech_duration_s + 8192);
        s->cap = s->seg.cap_samples + s->backlog;
        s = stream_make(s, (size_t) std::max<int64_t>(s->seg.cap_samples, 256));
        return true;
    });
    if (ok) return s;           // null where stream_make failed: it has freed the session
    stream_free(s);
    return nullptr;
}

int whisper_amd_stream_vad_poll_many(struct whisper_amd_stream ** ss, int n) {
    if (!ss || n <= 0) { WA_ERROR("%s: refused: null or empty arguments\n", __func__); return WHISPER_AMD_STREAM_BAD_ARGS; }
    if (n > 64) { WA_ERROR("%s: refused: %d sessions are more than 64\n", __func__, n); return WHISPER_AMD_STREAM_MIXED; }
    for (int i = 0; i < n; ++i) {
        if (!ss[i]) { WA_ERROR("%s: refused: session %d is null\n", __func__, i); return WHISPER_AMD_STREAM_BAD_ARGS; }
        if (!ss[i]->vad || ss[i]->ctx != ss[0]->ctx || ss[i]->vctx != ss[0]->vctx) {
            WA_ERROR("%s: refused: session %d is no VAD session of the first one's context and VAD context\n", __func__, i);
            return WHISPER_AMD_STREAM_MIXED;
        }
        for (int j = 0; j < i; ++j) if (ss[j] == ss[i]) { WA_ERROR("%s: refused: session %d is listed twice\n", __func__, i); return WHISPER_AMD_STREAM_BAD_ARGS; }
    }
    const char * const who = __func__;
    return wa_guard(who, WHISPER_AMD_STREAM_FAILED, [&]() -> int {
        if (!vad_process(ss, n)) { WA_ERROR("%s: the front end failed\n", who); return WHISPER_AMD_STREAM_FAILED; }
        int64_t due = 0;
        for (int i = 0; i < n; ++i) due += (int64_t) ss[i]->due.size();
        return (int) std::min<int64_t>(due, INT_MAX);
    });
}

int whisper_amd_stream_utterance_info(struct whisper_amd_stream * s, int64_t out[8]) {
    if (!s || !out || !s->vad) return WHISPER_AMD_STREAM_BAD_ARGS;
    out[0] = s->windows;
    out[1] = s->last.ranges.empty() ? 0 : s->last.ranges[0].start;
    out[2] = s->last.len;
    out[3] = s->last_utt.seg.start; out[4] = s->last_utt.seg.end; out[5] = s->last_utt.split ? 1 : 0;
    out[6] = s->fe_launches; out[7] = s->win_done;
    return 0;
}

int64_t whisper_amd_stream_vad_probs_copy(struct whisper_amd_stream * s, float * dst, int64_t cap) {
    if (!s || !s->vad || cap < 0 || (cap > 0 && !dst)) return WHISPER_AMD_STREAM_BAD_ARGS;
    const int64_t n = std::min<int64_t>(cap, (int64_t) s->probs.size());
    if (n > 0) memcpy(dst, s->probs.data(), (size_t) n * sizeof(float));
    return (int64_t) s->probs.size();
}

} // extern "C"

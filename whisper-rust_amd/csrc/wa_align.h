// wa_align.h - forced alignment: the per-row scores of a known transcript, as the kernel of wa_align.hip computes them on the
// logits where the decoder pass left them, and the same arithmetic on the host (no HIP, no device: tests/native/align_math.cpp compiles this
// header alone).  The record is `struct whisper_amd_align_score` of include/whisper_amd.h.
//
// Definitions, on the RAW logits x[0 .. n_vocab) of a row with target t - no suppression, no timestamp rules: this is the model's
// distribution, not whisper_full's sampler -
//   mx        = the row maximum;  best_id = the lowest index that attains it
//   lse       = mx + log( sum_i exp((double) x_i - (double) mx) ), sum and exp in F64; a -inf logit contributes 0
//   plog      = (float) ((double) x_t - lse);   p = (float) exp((double) x_t - lse);   a -inf x_t gives plog = -inf, p = 0
//   best_plog = the same for best_id
//   rank      = #{ i : x_i > x_t or (x_i == x_t and i < t) }
// evaluated as  plog = (x_t - mx) - log1p( sum over i != best_id of exp(x_i - mx) ): the same value, but a row on which the model is sure of
// its choice (p -> 1, plog -> -0) keeps its relative precision.  Taken literally, x_t - (mx + log(1 + s)) carries the rounding of a sum of
// the size of mx, about |mx| 2^-53 absolute, which is more than one F32 ulp of plog once |plog| < |mx| 2^-29 (seen: 16 ulps at p = 1 - 1e-8).
// This is deliberately not the sequential F32 expf sum of whisper_full's sampler (wa_full.cpp: logsumexp_ref_order): that order cannot be split
// over a workgroup, and nothing in the reference computes these scores for a caller's text.  With an F64 sum the result does not depend on how
// the row is split, to far below one F32 ulp; the host function below adds in index order, the kernel in its own fixed order.
#pragma once
#include "../../include/whisper_amd.h"

#include <cmath>
#include <cstdint>
#include <limits>

#define WA_ALIGN_THREADS 256       // one workgroup of four waves per logits row

static_assert(sizeof(struct whisper_amd_align_score) == 24, "whisper_amd_align_score is 24 bytes");
static_assert(sizeof(struct whisper_amd_align_token) == 32, "whisper_amd_align_token is 32 bytes");

// one row on the host; t outside [0, n_vocab): plog = -inf, p = 0, rank = n_vocab (the public entry points refuse such a target before)
static inline void wa_align_score_row_host(const float * x, int n_vocab, int t, struct whisper_amd_align_score & o) {
    const float ninf = -std::numeric_limits<float>::infinity();
    float mx = ninf;
    int best = 0;
    for (int i = 0; i < n_vocab; ++i) if (x[i] > mx) { mx = x[i]; best = i; }
    const bool has_t = t >= 0 && t < n_vocab;
    const float xt = has_t ? x[t] : ninf;
    double sum = 0.0;
    int rank = 0;
    for (int i = 0; i < n_vocab; ++i) {
        if (x[i] != ninf && i != best) sum += exp((double) x[i] - (double) mx);
        rank += (x[i] > xt || (x[i] == xt && i < t)) ? 1 : 0;
    }
    const double l1p = log1p(sum);                       // lse - mx
    auto put = [&](float v, float & plog, float & p) {
        if (v == ninf) { plog = ninf; p = 0.0f; return; }
        const double lp = ((double) v - (double) mx) - l1p;
        plog = (float) lp; p = (float) exp(lp);
    };
    put(xt, o.plog, o.p);
    put(mx, o.best_plog, o.best_p);
    o.best_id = best;
    o.rank = has_t ? rank : n_vocab;
}

// logits [n_rows][ld], ld >= n_vocab
static inline void wa_align_score_host(const float * logits, long long ld, int n_rows, int n_vocab, const int32_t * target, struct whisper_amd_align_score * out) {
    for (int r = 0; r < n_rows; ++r) wa_align_score_row_host(logits + (long long) r * ld, n_vocab, target[r], out[r]);
}

// k_align_score on `stream` (hipStream_t): device logits [n_rows][ld] F32, device targets, device records.  Rows need no alignment beyond 4 bytes.
// false: refused arguments or a launch error; nothing was launched then.
bool wa_align_score_launch(void * stream, const float * d_logits, long long ld, int n_rows, int n_vocab, const int32_t * d_target,
                           struct whisper_amd_align_score * d_out);

// wa_align.hip - forced alignment: k_align_score turns every logits row of the teacher-forced pass into one 24-byte record
// (wa_align.h states the arithmetic) where the vocabulary product left it, so that a transcript's 46 MB of logits never cross to the host.
//
// One workgroup of four waves per row, two passes over the row (207 KB at n_vocab 51865: it stays in L2):
//   1. maximum and the lowest index that attains it;
//   2. sum of exp((double) x - (double) mx) in F64 over every index but best_id, and the target's rank.
// A row starts at any multiple of 4 bytes (n_vocab is odd: every other row of a packed buffer lies 4 bytes off a 16-byte boundary).  The
// row is cut into a head of 0..3 scalars up to the first 16-byte boundary, a body of 16-byte groups and a tail of 0..3 scalars; thread i
// takes head element i, groups i, i + 256, ... and tail element i.
// The order of every sum is fixed, so two runs give the same bits: a thread adds its elements in the order above, a wave folds its 64
// partial sums with shuffles at distances 32, 16, ... 1, and thread 0 adds the four wave sums in LDS in wave order.  No atomics.
// No LDS beyond those few words, no scratch.
#include "wa_align.h"

#include <hip/hip_runtime.h>

namespace {

struct al_best { float v; int i; };
// a row's leading element: the larger value, at equal values the lower index (an empty slot is { -inf, INT_MAX })
__device__ __forceinline__ al_best al_pick(al_best a, al_best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

}

__global__ __launch_bounds__(WA_ALIGN_THREADS) void k_align_score(const float * __restrict__ logits, long long ld, int n_vocab,
                                                                  const int32_t * __restrict__ target,
                                                                  struct whisper_amd_align_score * __restrict__ out) {
    __shared__ float  s_v[WA_ALIGN_THREADS / 64];
    __shared__ int    s_i[WA_ALIGN_THREADS / 64];
    __shared__ double s_sum[WA_ALIGN_THREADS / 64];
    __shared__ int    s_rank[WA_ALIGN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float * x = logits + (long long) blockIdx.x * ld;
    const float ninf = -__builtin_inff();

    int head = (int) (((16u - (unsigned) ((uintptr_t) x & 15u)) & 15u) >> 2);
    if (head > n_vocab) head = n_vocab;
    const int n_grp = (n_vocab - head) >> 2, tail0 = head + 4 * n_grp, n_tail = n_vocab - tail0;
    const float4 * xg = (const float4 *) (x + head);

    // ---- pass 1: maximum, lowest index ----
    al_best b = { ninf, 0x7fffffff };
    if (tid < head) b = al_pick(b, { x[tid], tid });
    for (int g = tid; g < n_grp; g += WA_ALIGN_THREADS) {
        const float4 v = xg[g];
        const int i0 = head + 4 * g;
        b = al_pick(b, { v.x, i0 }); b = al_pick(b, { v.y, i0 + 1 }); b = al_pick(b, { v.z, i0 + 2 }); b = al_pick(b, { v.w, i0 + 3 });
    }
    if (tid < n_tail) b = al_pick(b, { x[tail0 + tid], tail0 + tid });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        al_best o;
        o.v = __shfl_down(b.v, d, 64); o.i = __shfl_down(b.i, d, 64);
        b = al_pick(b, o);
    }
    if (lane == 0) { s_v[wave] = b.v; s_i[wave] = b.i; }
    __syncthreads();
    al_best top = { s_v[0], s_i[0] };
#pragma unroll
    for (int w = 1; w < WA_ALIGN_THREADS / 64; ++w) top = al_pick(top, { s_v[w], s_i[w] });
    if (top.i == 0x7fffffff) top.i = 0;            // (a row of NaNs only: nothing compares)
    const float mx = top.v;
    const double mxd = (double) mx;

    // ---- pass 2: F64 sum of exp(x - mx), rank of the target ----
    const int t = target[blockIdx.x];
    const bool has_t = t >= 0 && t < n_vocab;
    const float xt = has_t ? x[t] : ninf;
    double sum = 0.0;
    int rank = 0;
    auto take = [&](float v, int i) {
        if (v != ninf && i != top.i) sum += exp((double) v - mxd);           // (the maximum's own term is the 1 of log1p below)
        rank += (v > xt || (v == xt && i < t)) ? 1 : 0;
    };
    if (tid < head) take(x[tid], tid);
    for (int g = tid; g < n_grp; g += WA_ALIGN_THREADS) {
        const float4 v = xg[g];
        const int i0 = head + 4 * g;
        take(v.x, i0); take(v.y, i0 + 1); take(v.z, i0 + 2); take(v.w, i0 + 3);
    }
    if (tid < n_tail) take(x[tail0 + tid], tail0 + tid);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum  += __shfl_down(sum, d, 64);
        rank += __shfl_down(rank, d, 64);
    }
    if (lane == 0) { s_sum[wave] = sum; s_rank[wave] = rank; }
    __syncthreads();
    if (tid == 0) {
        double total = s_sum[0];
        int    rk    = s_rank[0];
#pragma unroll
        for (int w = 1; w < WA_ALIGN_THREADS / 64; ++w) { total += s_sum[w]; rk += s_rank[w]; }
        const double l1p = log1p(total);                 // lse - mx
        struct whisper_amd_align_score o;
        if (xt == ninf) { o.plog = ninf; o.p = 0.0f; }
        else { const double lp = ((double) xt - mxd) - l1p; o.plog = (float) lp; o.p = (float) exp(lp); }
        if (mx == ninf) { o.best_plog = ninf; o.best_p = 0.0f; }
        else { o.best_plog = (float) -l1p; o.best_p = (float) exp(-l1p); }
        o.best_id = top.i;
        o.rank = has_t ? rk : n_vocab;
        out[blockIdx.x] = o;
    }
}

bool wa_align_score_launch(void * stream, const float * d_logits, long long ld, int n_rows, int n_vocab, const int32_t * d_target,
                           struct whisper_amd_align_score * d_out) {
    if (n_rows == 0) return true;
    if (n_rows < 0 || n_vocab <= 0 || ld < n_vocab || !d_logits || !d_target || !d_out || ((uintptr_t) d_logits & 3) != 0) return false;
    hipLaunchKernelGGL(k_align_score, dim3((unsigned) n_rows), dim3(WA_ALIGN_THREADS), 0, (hipStream_t) stream, d_logits, ld, n_vocab, d_target, d_out);
    return hipGetLastError() == hipSuccess;
}

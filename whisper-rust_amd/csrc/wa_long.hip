// wa_long.hip - long recordings: k_long_pack writes the speech-only audio of every chunk of a whisper_amd_full_long call
// in ONE launch, from the caller's audio in HBM straight into the buffers whisper_full_with_state reads.
//
// A pure copy: no LDS.  The output - all chunks in one allocation, each on a 256-byte boundary, the gaps between them zero pieces - is cut
// into tiles of WA_LONG_TILE samples, one workgroup each.  The workgroup finds the piece that holds its first sample by binary search in the
// piece table; its threads take groups of 4 consecutive samples, lane i the group at 16 i bytes (1 KiB per wave instruction), and walk
// forward through the table from there.  A group that lies inside one piece is ONE 16-byte store, fed by one 16-byte load where the
// source address is 16-byte aligned and by four 4-byte loads where it is not; a group that straddles a piece edge, or the end of the
// output, goes sample by sample.  Plain vector stores only.
#include "wa_long.h"

#include <hip/hip_runtime.h>

__global__ __launch_bounds__(256) void k_long_pack(const float * __restrict__ samples, const wa_long_piece * __restrict__ pieces, int n_pieces,
                                                   long long n_out, float * __restrict__ out) {
    const long long t0 = (long long) blockIdx.x * WA_LONG_TILE;
    const long long t1 = t0 + WA_LONG_TILE < n_out ? t0 + WA_LONG_TILE : n_out;
    int lo = 0, hi = n_pieces - 1;                  // the last piece with dst <= t0 (pieces[0].dst == 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pieces[mid].dst <= t0) lo = mid; else hi = mid - 1;
    }
    int p = lo;
    for (long long g = t0 + 4 * (long long) threadIdx.x; g < t1; g += 4 * 256) {
        while (p + 1 < n_pieces && pieces[p + 1].dst <= g) ++p;
        const wa_long_piece q = pieces[p];
        if (g + 4 <= t1 && g + 4 <= q.dst + q.len) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q.src >= 0) {
                const float * s = samples + (q.src + (g - q.dst));
                if (((uintptr_t) s & 15) == 0) v = *(const float4 *) s;
                else v = make_float4(s[0], s[1], s[2], s[3]);
            }
            *(float4 *) (out + g) = v;
        } else {
            int e = p;
            for (int k = 0; k < 4 && g + k < t1; ++k) {
                const long long at = g + k;
                while (e + 1 < n_pieces && pieces[e + 1].dst <= at) ++e;
                const wa_long_piece r = pieces[e];
                out[at] = (r.src >= 0 && at >= r.dst && at < r.dst + r.len) ? samples[r.src + (at - r.dst)] : 0.0f;
            }
        }
    }
}

bool wa_long_pack_launch(void * stream, const float * d_samples, const wa_long_piece * d_pieces, int n_pieces, long long n_out, float * d_out) {
    if (n_out <= 0) return true;
    const long long blocks = (n_out + WA_LONG_TILE - 1) / WA_LONG_TILE;
    if (n_pieces <= 0 || !d_pieces || !d_out || ((uintptr_t) d_out & 15) != 0 || blocks > 0x7fffffffLL) return false;
    hipLaunchKernelGGL(k_long_pack, dim3((unsigned) blocks), dim3(256), 0, (hipStream_t) stream, d_samples, d_pieces, n_pieces, n_out, d_out);
    return hipGetLastError() == hipSuccess;
}

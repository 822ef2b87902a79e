// wa_long.h - long recordings: the pack kernel's launcher (wa_long.hip) for wa_long.cpp.  No HIP types: the stream travels as void *.
#pragma once

#include "wa_long_plan.h"

#define WA_LONG_TILE  4096      // output samples per workgroup of k_long_pack (exported: whisper_amd_long_tile)
#define WA_LONG_ALIGN 64        // floats: every chunk starts on a 256-byte boundary of the state's chunk buffer

// d_out[0 .. n_out) from the caller's audio d_samples: `d_pieces` (device) lists n_pieces pieces in ascending dst order that cover [0, n_out)
// without a gap, the first at dst 0; src = -1 writes zeros.  The caller has checked every src + len against its audio.  false: the launch failed.
bool wa_long_pack_launch(void * stream, const float * d_samples, const wa_long_piece * d_pieces, int n_pieces, long long n_out, float * d_out);

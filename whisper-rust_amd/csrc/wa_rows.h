// wa_rows.h - the decode step for 2..8 token ROWS as ONE persistent launch (wa_rows.hip).
//
// ref: whisper_build_graph_decoder whisper.cpp:2474-2852 with n_tokens = n_decoders_cur rows: beam search and best_of > 1 batch one
// token per live decoder (whisper.cpp:7404-7431), the reference's bench a 5-token batch (examples/bench/bench.cpp:110-123), and
// lock-step chunks (wa_decode.cpp: wa_batcher) one token per chunk.  wa_mega.hip is the one-row form of the same idea, tuned around
// a single token's dependency chain; with several rows the work per phase is larger and rows differ in where their K / V live, so
// this kernel is organised differently:
//   * every workgroup does everything (no roles): its slice of the rows of every matrix for ALL token rows, and - in the attention
//     phases - the (row, head) / (row, head, quarter) units dealt to it, so the encoder K / V of different chunks stream over all CUs;
//   * a workgroup's weight rows arrive by LDS-DMA, issued by a dedicated wave one phase ahead into one of two LDS slots: the streaming
//     is off the vector-memory queues of the waves that poll hand-offs, and the products read weights AND activations from LDS;
//   * LayerNorm is one wave per token row (no cross-wave reductions);
//   * hand-offs are the 8-byte {tag, value} granules of wa_mega.hip.
// One kernel per LayerNorm width and weight format family (wa_rows_args::quant), each with its own code and registers:
//   k_decode_rows_np*     F16 weights, F16 operand rows;
//   k_decode_rows_q_np*   Q5_0 / Q8_0 weights (quants + block scales), operand rows quantised to Q8_0, blocks handed over as 8 quads + scale;
//   k_decode_rows_q1_np*  Q4_1 / Q5_1 weights (quants + block scales + block minimums), operand rows quantised to Q8_1: the word that holds a
//                         Q8_0 block's F32 scale holds the F16 pair {d, s} instead, in LDS and in the ninth granule alike, and every product
//                         adds the block-ordered chain of m_w * s_x after the lane chains (wa_quant1.h).  Opt-in: WHISPER_AMD_ROWS_Q1=1, 1..8 rows.
//   k_decode_rows_k_np*   Q6_K / Q3_K weights (quants + 16 scale bytes and one F32 d per block of 256), operand rows quantised to Q8_K.  No producer
//                         holds a whole block of what it publishes, so attention outputs and the MLP's hidden row travel in F32, one granule
//                         per value, and the gathering waves quantise them into LDS; LayerNorm rows are quantised by the wave that holds
//                         them.  Opt-in: WHISPER_AMD_ROWS_K=1, 1..8 rows.
//   k_decode_rows_k5_np*, Q5_K and Q2_K weights, the K formats whose product has a minimum term (a dmin per block beside the d): as above, and the
//   k_decode_rows_k2_np*  quantising waves store each block's 16 sums with the row.  Q5_K: one lane of a weight row's eight runs the minimum chain of a
//                         token row beside the lane chains; Q2_K: the minimums enter the lane chains, per block before the product term.  Opt-in:
//                         WHISPER_AMD_ROWS_KM=1, 1..8 rows.
//   k_decode_rows_q4_np*  Q4_0 weights in the arena's packed form (wa_quant4.h: nibble words [g = 0..3][block] + F32 block scales; a slot row is K / 2 bytes,
//                         then - mq4_soff in - the scales), operand rows Q8_0 and everything but the seven layer products as k_decode_rows_q_np* (the
//                         token embedding is stored in Q5_0's layout).  The interleaved product has ONE chain per output: the eight lanes of a weight row
//                         split the blocks, four each in a round of 32, and hand the exact block sums as int16 through a per-wave LDS exchange area to the
//                         lane that runs a token row's chain.  Opt-in: WHISPER_AMD_ROWS_Q4=1, 1..8 rows.
//   k_decode_rows_q4k_np* Q4_K weights in the arena's packed form (wa_quant4.h: nibble words [l = 0..7][block][j = 0..3], 16 scale bytes, d and dmin per block),
//                         operand rows Q8_K with block sums, embedding fetch and logits as k_decode_rows_k5_np* (the token embedding lies in Q5_K's arrays;
//                         the logits' minimum term runs in four chains).  The interleaved product gives a token row bits that depend on its PLACE in
//                         the pass the reference would have run: rows below rows4 are gemm rows (four chain steps a block, operand rows by the
//                         four-row quantiser), the others gemv rows (one step, the row quantiser) - per chain lane and per quantising wave, so one
//                         launch serves rows of both kinds.  Lane l of an output's eight is activation lane l; the pair sums go round the eight
//                         lanes by DPP.  Opt-in: WHISPER_AMD_ROWS_Q4K=1, 1..8 rows.
// Arithmetic is the reference order throughout (same chains, trees, certified F64 sums as wa_exact.hip): logits are bit-identical to
// the launch sequence, which stays as the fallback.
#pragma once
#include "wa_mega.h"

#define WA_ROWS_MAX 8
#define WA_ROWS_MAXKV 2048           // most self-attention cells a row may attend over in this kernel (scores / probabilities in LDS)
#define WA_ROWS_CGR 2048             // granules per (layer, row, head) of the cross-attention exchange area

struct wa_rows_row {                 // where ONE token row's state lives (layer 0; the kernel adds the layer offsets)
    wa_f16 * kv_k, * kv_v;           // self K / V cells [layer][cell][d]
    const wa_f16 * cross_k, * cross_v;
    const int8_t * mask;             // [n_kv] 1 = cell hidden from this row (beams share cells by sequence id); null: every cell < n_kv visible
    int n_kv, kv_head;               // cells attended over; the cell this row's new key / value go to
    int token, pos;
    // next-token prediction for lock-step members that decode greedily (wa_decode.cpp: the run-ahead batcher; as wa_mega_args): with `smask` set
    // the launch leaves per-workgroup candidate records of the row's logits under the reference's logit rules (approximated: the host verifies
    // every token); with spec != 0 the row's token is picked from the records and state its previous pass left, not taken from `token`.
    int spec;
    const unsigned * rec_in; unsigned * rec_out;      // [n_workgroups][8]: {max text logit, id, max timestamp logit, id, sum exp(ts - max ts)} (wa_one_launch_dev.h: MO_REC_*)
    const int * ps_in; int * ps_out;                  // {last token, token before it (-1: none), seek_delta, has_ts}; ps_out[4] = the token this launch decoded (MO_PS_*)
    const unsigned * smask;                           // bit i set: token i is suppressed for the row's whole call; null: no records
    int s_last, s_penult, s_seek_delta, s_has_ts;     // spec == 0: the state after `token`, from the host
};

struct wa_rows_args {
    // model (as wa_mega_args)
    const wa_mega_layer * layers; int n_layer, d, n_head, n_vocab; float eps;
    double rn_d;
    const wa_f16 * te; const float * pe; const float * lnf_w, * lnf_b; const wa_f16 * gelu;
    const float * te_d; int quant;                      // quant: 0 F16 weights, 1 Q5_0 / Q8_0 (Q8_0 operand rows), 2 Q4_1 / Q5_1 (Q8_1 operand rows, block minimums), 3 Q6_K / Q3_K (Q8_K operand rows), 4 Q5_K / Q2_K (Q8_K operand rows with block sums, dmin), 5 Q4_0 (Q8_0 operand rows, packed nibble rows, one chain per output), 6 Q4_K (Q8_K operand rows with block sums, packed nibble rows, two chains per output stepped by the row's rule: rows4)
    const float * te_m;                                 // quant == 2: block minimums of the token embedding (the layers' are in wa_mega_layer); quant 4, 6: its blocks' dmin
    unsigned long long kv_layer_stride, cross_layer_stride;
    int cross_tpad, T;
    unsigned long long * granules; int row_gr;          // [layer][8][B][row_gr] hand-off granules (row_gr = 2 d; quant 3, 4, 6: 4 d, the MLP's hidden row travels in F32)
    unsigned long long * cross_gr;                      // [layer][B][head][WA_ROWS_CGR]
    float * logits;                                     // [B][n_vocab]
    unsigned * status;                                  // [0] 0 = ok, else the code of the hand-off that timed out; [1] = seq once the launch has run
    unsigned * row_status;                              // [B] (cleared by the caller) WA_MEGA_REDO: a soft-max sum of this row could not be certified order-independent -
                                                        // the row's logits may be an ulp off, the row is to be redone by the launch sequence; the other rows stand
    float * dbg;
    int * tok_out;                                      // [B] the token every row decoded (given, or picked from its records), null: not wanted
    float kq_scale; unsigned seq;
    int B, slot_bytes;
    int force_inorder;                                  // tests (WHISPER_AMD_ROWS_FORCE_INORDER): every cross soft-max total takes the in-order path of mb_unit_cross
    int token_beg, token_eot;                           // (records) first timestamp token, end-of-text token
    int n_out, out_row[WA_ROWS_MAX];                    // token rows whose logits are wanted (the reference flags batch.logits rows): logits row m = token row out_row[m]
    wa_rows_row rows[WA_ROWS_MAX];
    const int8_t * te_sc;                               // quant 3, 4, 6: the token embedding's 16 scale bytes per block (te: its quants, te_d: its d)
    int wtype;                                          // quant == 4: the ggml type of the weights, 13 Q5_K or 10 Q2_K - which of the two kernels is launched
    int rows4;                                          // quant == 6: token rows below this are gemm rows of the reference's pass (wa_q4_K_rows4(M) where the rows are ONE pass of M rows in token
                                                        // order - a whisper_decode batch, a beam step), the others gemv rows; 0 where every row is a pass of its own (lock-step rows, a single token)
};

// LDS the kernel needs for B rows of a d-wide model with `n_wg` workgroups; 0 when it does not fit (the caller keeps the launch sequence).
// slot_bytes = size of one of the two weight slots.
size_t wa_rows_lds_bytes(int d, int B, int n_wg, int quant, int * slot_bytes);
// n_wg workgroups of 512 threads, all resident at once (1 per CU); false: shape not supported
bool wa_launch_decode_rows(hipStream_t s, const wa_rows_args & a, int n_wg);

// wa_one_launch_dev.h - device side of what the two one-launch decode kernels share (wa_mega.hip: the single-token step, wa_rows.hip: the
// 2..8-row step; the host side is wa_one_launch.h): address-space types, the granule hand-off and its bounded poll, the test build's
// stalls, the reference-order score, the Q8_0 block quantiser, the attention outputs' publish and the next-token prediction records,
// which one kernel writes and either kernel reads.  What the two kernels organise differently (roles, LayerNorm drivers, products,
// attention units, LDS carving) stays in their files.
#pragma once
#include "wa_device.h"

typedef unsigned long long u64;
#define GAS __attribute__((address_space(1)))
typedef GAS u64 gu64;
typedef GAS unsigned gu32;
typedef const GAS wa_f16 * gch;      // every global access is spelled global: a pointer read from the argument block or from
typedef const GAS float * gcf;       // the layer table is generic to the compiler, and a flat access also waits on the LDS counter
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // (HIP's u32x4 class cannot be read through an address-space pointer)

// The kernel bodies are inlined into the kernel and read the launch arguments from the kernel-argument segment (scalar loads: every field
// stays wave-uniform); the kernel hands them its address and mo_uniform makes it provably uniform again.
template <class Args>
__device__ __forceinline__ const __attribute__((address_space(4))) Args * mo_uniform(const __attribute__((address_space(4))) Args * p) {
    const unsigned long long v = (unsigned long long) p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned) v), hi = __builtin_amdgcn_readfirstlane((unsigned) (v >> 32));
    return (const __attribute__((address_space(4))) Args *) (((unsigned long long) hi << 32) | lo);
}

// -------------------------------------------------------------------------------------------------
// hand-off: activations travel between workgroups as 8-byte {tag = launch sequence number, value} granules
// -------------------------------------------------------------------------------------------------
enum { E_QKV = 0, E_AO, E_X1, E_QC, E_AO2, E_X2, E_HF, E_X3 };      // the edges of a layer, one run of granules each

#define MO_SPIN_LIMIT 20000u      // polls (~0.5 us each, ~10 ms) before a hand-off is declared dead: the host then pauses the one-launch form and tries again later
struct mo_ctl { gu32 * status; unsigned seq; bool dead; };

__device__ __forceinline__ void gr_store(gu64 * g, unsigned seq, unsigned v) {
    __hip_atomic_store(g, ((u64) seq << 32) | (u64) v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 gr_load(gu64 * g) { return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// A granule whose readers all sit on the WRITER'S XCD (`local`, established at run time: mg_role_cross): a plain store keeps the line
// in that XCD's L2, where the readers' L1-bypassing polls find it - an sc1 store drops it from L2 and every reader goes out to the
// fabric (MI355X_MICROARCH.md, inter-workgroup visibility).  Never for a granule that another XCD reads: its L2 would stay stale.
__device__ __forceinline__ void gr_store_l(gu64 * g, unsigned seq, unsigned v, bool local) {
    if (local) __hip_atomic_store(g, ((u64) seq << 32) | (u64) v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else       __hip_atomic_store(g, ((u64) seq << 32) | (u64) v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) { return (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, CTRL, 0xf, 0xf, true); }

// One wave polls the granules idx(0..NPL-1) (idx < 0: none) until every tag equals this launch's sequence number.
// Every poll is bounded: a time-out is reported through `status`, and a status another wave has set ends this wave's poll too.
// How a lane without a granule loads is the kernel's choice, each measured in its kernel:
//   MO_POLL_OWN (single-token step): predicated loads; returns the polls it took (for the step's timeline).  (Measured there: a second,
//     staggered poll in flight per wave makes every hand-off LONGER - 0.377 -> 0.401 ms per token -, longer pauses between polls too (s_sleep 6: 0.384, 14: 0.402), none at all changes nothing; a
//     pause before the first poll of the gathers that follow an attention phase cuts their polls by 2-3 x and changes nothing either: the
//     hand-off time is the store-to-load path itself, not contention by the polls.)
//   MO_POLL_ALL (rows step): unconditional loads - a lane without a granule reads granule 0 -: predicated ones are issued one round trip
//     at a time there.
enum { MO_POLL_OWN = 0, MO_POLL_ALL = 1 };
template <int POLL> __device__ __forceinline__ auto mo_polls(unsigned spins) { if constexpr (POLL == MO_POLL_OWN) return spins; }
template <int POLL, int NPL, typename F>
__device__ __forceinline__ auto mo_sweep(gu64 * g, F idx, mo_ctl & c, int lane, unsigned (&v)[NPL], unsigned code) {
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int i = idx(k);
            if constexpr (POLL == MO_POLL_OWN) { if (i >= 0) { const u64 x = gr_load(g + i); v[k] = (unsigned) x; ok &= (unsigned) (x >> 32) == c.seq; } }
            else { const u64 x = gr_load(g + (i >= 0 ? i : 0)); v[k] = (unsigned) x; ok &= i < 0 || (unsigned) (x >> 32) == c.seq; }
        }
        if (__all(ok) || c.dead) return mo_polls<POLL>(spins);
        if ((spins & 127u) == 127u) {
            const unsigned st = __builtin_amdgcn_readfirstlane(__hip_atomic_load(c.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (st != 0u) { c.dead = true; return mo_polls<POLL>(spins); }
            if (spins >= MO_SPIN_LIMIT) {
                if (lane == 0) __hip_atomic_store(c.status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                c.dead = true;
                return mo_polls<POLL>(spins);
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// WA_CHAOS (the test build, libwhisper_chaos.so; tools/chaos_check.sh): a hash of (who, where, which launch) picks one site in eight to stall
// for ~25 us, so that the rest of the workgroup - and of the grid - runs far ahead of it.  Results must not change: nothing may rely on
// how long a product or a hand-off takes.  The kernels' site macros name the sites.
#ifdef WA_CHAOS
__device__ __forceinline__ void mo_chaos(unsigned a, unsigned b, unsigned c_, unsigned phase, unsigned seq) {
    unsigned h = (a * 2654435761u) ^ (b * 40503u) ^ (c_ * 2246822519u) ^ (phase * 3266489917u) ^ (seq * 668265263u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    if ((h & 7u) == 0u) for (int i = 0; i < 8; ++i) __builtin_amdgcn_s_sleep(127);
}
#endif

// -------------------------------------------------------------------------------------------------
// arithmetic
// -------------------------------------------------------------------------------------------------
// one key's score from its two 16-byte pieces (lane a of the key's 4-lane group): k_attn_exact's arithmetic
__device__ __forceinline__ float mo_score(const u32x4 & ka, const u32x4 & kb, const float (&qa)[8], const float (&qb)[8], float scale) {
    const wa_f16 * k8a = (const wa_f16 *) &ka, * k8b = (const wa_f16 *) &kb;
    float v[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        float t = fmaf(h2f(k8a[l]), qa[l], 0.0f);
        t = fmaf(h2f(k8b[l]), qb[l], t);
        t = t + dpp_f32<0x4e>(t);                // quad_perm [2,3,0,1]: s[j] + s[j+2]
        v[l] = t + dpp_f32<0xb1>(t);             // quad_perm [1,0,3,2]: (s0+s2) + (s1+s3)
    }
    const float t0 = v[0] + v[4], t1 = v[1] + v[5], t2 = v[2] + v[6], t3 = v[3] + v[7];
    return ((t0 + t1) + (t2 + t3)) * scale;
}

// words between the quad rows u = 0..7 of a Q8_0 operand row in LDS: nb | 8 puts the eight 16-byte reads of a product step on disjoint
// banks (u * nb alone: nb = 96 folds them onto two)
__device__ __forceinline__ int mq_ld(int nb) { return nb | 8; }

// quantize_row_q8_0 (ggml-cpu/arch/x86/quants.c) of a 32-element block held one value per lane of a half-wave (as wa_q8_store): returns the
// quad of lanes 4k..4k+3 packed over DPP in lane 4k, and in dq the block's scale rounded through F16.  All lanes take part.
__device__ __forceinline__ unsigned mq_quant32(float y, float & dq) {
    float a = fabsf(y);
    a = fmaxf(a, dpp_f32<0x128>(a)); a = fmaxf(a, dpp_f32<0x124>(a)); a = fmaxf(a, dpp_f32<0x122>(a)); a = fmaxf(a, dpp_f32<0x121>(a));
    a = fmaxf(a, __shfl_xor(a, 16, 32));
    const float id = a != 0.0f ? 127.f / a : 0.0f;
    dq = h2f(f2h(a / 127.f));
    const unsigned q = (unsigned) (int) rintf(y * id) & 0xffu;
    return q | (dpp_u32<0x101>(q) << 8) | (dpp_u32<0x102>(q) << 16) | (dpp_u32<0x103>(q) << 24);      // row_shl:1..3
}

// Threads 0..63 publish a head's 64 attention outputs (y = output tid of head h) into the row's run of `edge`: as 32 packed-F16 granules,
// or - Q: they are two Q8_0 blocks of the out-projection's operand - quantised HERE, once, instead of by every consumer: a block leaves as
// 8 quads + its scale (9 granules instead of 32 F32 values).
template <bool Q>
__device__ __forceinline__ void mo_attn_publish(float y, gu64 * edge, int h, unsigned seq, int tid) {
    if constexpr (Q) {
        float dq;
        const unsigned w = mq_quant32(y, dq);
        gu64 * eb = edge + (size_t) (2 * h + (tid >> 5)) * 9;
        if ((tid & 3) == 0) gr_store(eb + ((tid & 31) >> 2), seq, w);
        if ((tid & 31) == 0) gr_store(eb + 8, seq, __float_as_uint(dq));
    } else {
        const unsigned hv = (unsigned) f2h(y);
        const unsigned hi = dpp_u32<0x101>(hv);          // row_shl:1: lane i reads lane i + 1
        if ((tid & 1) == 0) gr_store(edge + ((h * 64 + tid) >> 1), seq, (hv & 0xffffu) | (hi << 16));
    }
}

// -------------------------------------------------------------------------------------------------
// next-token prediction.  A launch classifies every logit by the sampling state after its input token and leaves one candidate record
// per workgroup; the next launch - of either kernel - merges them into its input token.  Device arithmetic here is a prediction only
// (fast exp, any order): the host re-derives every token from the logits with the reference's rules.
// -------------------------------------------------------------------------------------------------
// a record (rec_in / rec_out: [n_workgroups][MO_REC_WORDS] words)
#define MO_REC_WORDS 8
enum { MO_REC_TEXT_V = 0, MO_REC_TEXT_I, MO_REC_TS_V, MO_REC_TS_I, MO_REC_TS_SUM };      // max text logit, its id, max timestamp logit, its id, sum exp(ts - max ts)
// the sampling state between launches (ps_in / ps_out; the rows step also leaves the token it decoded)
enum { MO_PS_LAST = 0, MO_PS_PENULT, MO_PS_SEEK_DELTA, MO_PS_HAS_TS, MO_PS_TOKEN };
// the picked token and the state after it, in LDS for the launch's own classifier
enum { MO_PK_TOKEN = 0, MO_PK_LAST, MO_PK_PENULT, MO_PK_SEEK_DELTA, MO_PK_HAS_TS };
struct mo_pick { int token, last, penult, seek_delta, has_ts; };

struct mo_best { float v; int i; };
#define MO_BEST_NONE { -INFINITY, 0x7fffffff }
__device__ __forceinline__ void mo_best_merge(mo_best & a, float v, int i) { if (v > a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; } }
__device__ __forceinline__ void mo_best_wave(mo_best & a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(a.v, o, WAVE); const int i = __shfl_xor(a.i, o, WAVE); mo_best_merge(a, v, i); }
}
__device__ __forceinline__ int mo_decide(const mo_best & bt, const mo_best & bs, float s_ts) {
    // whisper.cpp:6309-6333: timestamp mass above every text token => a timestamp; else the arg-max of everything allowed
    if (!(bs.v > -INFINITY)) return bt.v > -INFINITY ? bt.i : 0;
    if (!(bt.v > -INFINITY)) return bs.i;
    if (__logf(s_ts) + bs.v > bt.v) return bs.i;
    return bs.v > bt.v ? bs.i : bt.i;
}
// one wave: the records and the state the previous launch left, merged into this launch's token and the state after it
__device__ __forceinline__ void mo_pick_merge(mo_pick & p, const unsigned * rec_in, const int * ps_in, int n_rec, int token_beg, int lane) {
    const GAS int * ps = (const GAS int *) ps_in;
    const GAS unsigned * rec = (const GAS unsigned *) rec_in;
    p.penult = ps[MO_PS_LAST]; p.seek_delta = ps[MO_PS_SEEK_DELTA]; p.has_ts = ps[MO_PS_HAS_TS];
    mo_best bt = MO_BEST_NONE, bs = MO_BEST_NONE;
    // every record (n_rec <= 256: four per lane) in ONE round of loads - a loop over them paid a cold global round trip per
    // iteration, 4.4 us at the head of every launch
    u32x4 ra[4]; unsigned rb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = lane + 64 * j, gg = g < n_rec ? g : 0;
        ra[j] = *(const GAS u32x4 *) (rec + gg * MO_REC_WORDS); rb[j] = rec[gg * MO_REC_WORDS + MO_REC_TS_SUM];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (lane + 64 * j < n_rec) {
        mo_best_merge(bt, __uint_as_float(ra[j].x), (int) ra[j].y);
        mo_best_merge(bs, __uint_as_float(ra[j].z), (int) ra[j].w);
    }
    mo_best_wave(bt); mo_best_wave(bs);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (lane + 64 * j < n_rec) {
        const float m = __uint_as_float(ra[j].z);
        if (m > -INFINITY) s += __uint_as_float(rb[j]) * __expf(m - bs.v);
    }
    s = wave_sum(s);
    p.token = mo_decide(bt, bs, s);
    p.last = p.token;
    if (p.token > token_beg) { p.seek_delta = 2 * (p.token - token_beg); p.has_ts = 1; }
}
__device__ __forceinline__ void mo_pick_put(int * pk, const mo_pick & p) {
    pk[MO_PK_TOKEN] = p.token; pk[MO_PK_LAST] = p.last; pk[MO_PK_PENULT] = p.penult; pk[MO_PK_SEEK_DELTA] = p.seek_delta; pk[MO_PK_HAS_TS] = p.has_ts;
}

// Which logits the next pick may choose, by the sampling state after this launch's token (whisper.cpp:6264-6302), and a thread's
// running candidates among the logits it has added: the best text token, the best timestamp and the timestamps' mass relative to it.
struct mo_cand {
    bool no_ts, no_text; int ts_min, beg, eot;
    mo_best bt, bs; float s_ts;
};
__device__ __forceinline__ mo_cand mo_cand_init(const int * pk, int beg, int eot) {
    mo_cand c;
    const int st_last = pk[MO_PK_LAST], st_penult = pk[MO_PK_PENULT], st_seek = pk[MO_PK_SEEK_DELTA], st_has = pk[MO_PK_HAS_TS];
    const bool last_ts = st_last >= beg, penult_ts = st_penult < 0 || st_penult >= beg;
    c.no_ts = last_ts && penult_ts; c.no_text = last_ts && !penult_ts;
    c.ts_min = st_has ? beg + st_seek / 2 : beg;
    c.beg = beg; c.eot = eot;
    c.bt = MO_BEST_NONE; c.bs = MO_BEST_NONE; c.s_ts = 0.0f;
    return c;
}
// logit r of vocabulary row `row`; mw = the word of the suppression mask that holds the row's bit
__device__ __forceinline__ void mo_cand_add(mo_cand & c, float r, int row, unsigned mw) {
    if ((mw >> (row & 31)) & 1u) return;
    if (row >= c.beg) {
        if (!c.no_ts && row >= c.ts_min) {
            if (r > c.bs.v) { c.s_ts = c.s_ts * __expf(c.bs.v - r) + 1.0f; c.bs.v = r; c.bs.i = row; }
            else c.s_ts += __expf(r - c.bs.v);
        }
    } else if (!(c.no_text && row < c.eot)) mo_best_merge(c.bt, r, row);
}
// all eight waves: the threads' candidates reduced over the wave, then - through `scratch` (LDS, [8][MO_REC_WORDS]) - over the
// workgroup; lane 0 of wave 0 writes the workgroup's record at `rec`
__device__ __forceinline__ void mo_cand_record(mo_cand & c, unsigned * scratch, unsigned * rec, int lane, int wave) {
    const float m_loc = c.bs.v;
    mo_best_wave(c.bt); mo_best_wave(c.bs);
    float sw = m_loc > -INFINITY ? c.s_ts * __expf(m_loc - c.bs.v) : 0.0f;
    sw = wave_sum(sw);
    unsigned * mine = scratch + wave * MO_REC_WORDS;
    if (lane == 0) { mine[MO_REC_TEXT_V] = __float_as_uint(c.bt.v); mine[MO_REC_TEXT_I] = (unsigned) c.bt.i; mine[MO_REC_TS_V] = __float_as_uint(c.bs.v);
                     mine[MO_REC_TS_I] = (unsigned) c.bs.i; mine[MO_REC_TS_SUM] = __float_as_uint(sw); }
    wa_barrier_lds();
    if (wave == 0) {
        mo_best t2 = MO_BEST_NONE, s2 = MO_BEST_NONE;
        float sl = 0.0f, ml = -INFINITY;
        const unsigned * w = scratch + lane * MO_REC_WORDS;
        if (lane < 8) { t2.v = __uint_as_float(w[MO_REC_TEXT_V]); t2.i = (int) w[MO_REC_TEXT_I]; s2.v = __uint_as_float(w[MO_REC_TS_V]); s2.i = (int) w[MO_REC_TS_I];
                        sl = __uint_as_float(w[MO_REC_TS_SUM]); ml = s2.v; }
        mo_best_wave(t2); mo_best_wave(s2);
        float sg = ml > -INFINITY ? sl * __expf(ml - s2.v) : 0.0f;
        sg = wave_sum(sg);
        if (lane == 0) {
            GAS unsigned * ro = (GAS unsigned *) rec;
            ro[MO_REC_TEXT_V] = __float_as_uint(t2.v); ro[MO_REC_TEXT_I] = (unsigned) t2.i; ro[MO_REC_TS_V] = __float_as_uint(s2.v); ro[MO_REC_TS_I] = (unsigned) s2.i;
            ro[MO_REC_TS_SUM] = __float_as_uint(sg);
        }
    }
}

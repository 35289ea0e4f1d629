// Per-row mu-law sampler shared by the per-step sampler kernel (mlp.hip) and the persistent
// generation loop (gen_mlp.hip), so both paths draw bit-identical samples from identical
// logits.
//
// Reference: Generator.__call__ (model.py:514-517) samples
//     x_t = exp(log_softmax(z)).multinomial(1)
// which torch>=2 on CPU implements as argmax(p / q), q ~ Exp(1) (first index on ties);
// here argmax(z - log q), the same index up to fp rounding of near-ties.
// q comes either from a device buffer (bit-replay of the reference RNG stream) or from a
// counter-based Philox4x32-10 (counter = (lane, row, step, 0), key = seed).
#pragma once
#include "common.hpp"

// All-lane reductions over the wave without LDS: xor-1, xor-2 (DPP quad_perm), the
// 8-lane half mirror and the 16-lane mirror (DPP), then the lane pairs i, i ^ 16 and i, i ^ 32
// (permlane swaps).  Every step combines the same two operands in both lanes of a pair
// (a + b == b + a bitwise), so all 64 lanes end with the identical value.
template <typename Op>
__device__ __forceinline__ float wave_allreduce(float v, Op op) {
    v = op(v, __uint_as_float(dpp_u32<0xB1>(__float_as_uint(v))));    // quad_perm [1,0,3,2]
    v = op(v, __uint_as_float(dpp_u32<0x4E>(__float_as_uint(v))));    // quad_perm [2,3,0,1]
    v = op(v, __uint_as_float(dpp_u32<0x141>(__float_as_uint(v))));   // row_half_mirror
    v = op(v, __uint_as_float(dpp_u32<0x140>(__float_as_uint(v))));   // row_mirror
    uint32_t lo, hi;
    xpair16(__float_as_uint(v), lo, hi);
    v = op(__uint_as_float(lo), __uint_as_float(hi));
    xpair32(__float_as_uint(v), lo, hi);
    return op(__uint_as_float(lo), __uint_as_float(hi));
}
__device__ __forceinline__ float wave_max(float v) {
    return wave_allreduce(v, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ float wave_sum(float v) {
    return wave_allreduce(v, [](float a, float b) { return a + b; });
}

// (best, index) argmax over the wave, first index on ties (torch argmax); same step
// sequence as wave_allreduce
__device__ __forceinline__ void amax_take(float& best, int& bi, float ob, int oi) {
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
}
template <int CTRL>
__device__ __forceinline__ void amax_dpp(float& best, int& bi) {
    const float ob = __uint_as_float(dpp_u32<CTRL>(__float_as_uint(best)));
    const int oi = (int)dpp_u32<CTRL>((uint32_t)bi);
    amax_take(best, bi, ob, oi);
}
__device__ __forceinline__ int wave_argmax(float best, int bi) {
    amax_dpp<0xB1>(best, bi);
    amax_dpp<0x4E>(best, bi);
    amax_dpp<0x141>(best, bi);
    amax_dpp<0x140>(best, bi);
    uint32_t lo, hi, ilo, ihi;
    xpair16(__float_as_uint(best), lo, hi);
    xpair16((uint32_t)bi, ilo, ihi);
    best = __uint_as_float(lo);
    bi = (int)ilo;
    amax_take(best, bi, __uint_as_float(hi), (int)ihi);
    xpair32(__float_as_uint(best), lo, hi);
    xpair32((uint32_t)bi, ilo, ihi);
    best = __uint_as_float(lo);
    bi = (int)ilo;
    amax_take(best, bi, __uint_as_float(hi), (int)ihi);
    return bi;
}

// Philox4x32-10 (Salmon et al. 2011)
__device__ __forceinline__ uint4 philox4x32(uint4 c, uint2 k) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = c.x * 0xD2511F53u, hi0 = __umulhi(c.x, 0xD2511F53u);
        const uint32_t lo1 = c.z * 0xCD9E8D57u, hi1 = __umulhi(c.z, 0xCD9E8D57u);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// Exp(1) from a 32-bit draw: u in (0, 1], q = -log(u)
__device__ __forceinline__ float exp1_from_u32(uint32_t x) {
    const float u = ((float)(x >> 8) + 1.0f) * (1.0f / 16777216.0f);
    return -logf(u);
}

// Exp(1) noise of lane `lane` (q = 4 lane .. 4 lane + 3) for (row b, generation step `step`).
// Philox counters use the GLOBAL row row0 + b: a rank generating rows [row0, row0 + B) of a
// larger batch (rank-sharded generation) draws exactly the single-process stream.
// `step` is relative to the call (the index into a replayed noise buffer); the Philox counter
// is step0 + step, step0 the steps the stream had completed before the call (streaming:
// srnn_generate5).  Per-row origins (srnn_generate6, continuous batching): noise_row[b] replaces
// row0 + b and row_step0[b] replaces step0, so a stream keeps its draws whichever local row
// serves it and whatever the other rows' step counts are.  Both only move Philox counters: a
// replayed buffer keeps its call-relative index.  Null (the default): the counters above.
__device__ __forceinline__ floatx4 sample_noise(const float* noise, uint64_t seed, int B, int b,
                                                int step, int lane, int row0 = 0,
                                                uint32_t step0 = 0u,
                                                const int* noise_row = nullptr,
                                                const uint32_t* row_step0 = nullptr) {
    if (noise)
        return *reinterpret_cast<const floatx4*>(noise + ((int64_t)step * B + b) * 256 + 4 * lane);
    // (the origins are moved, the expression below is not touched: with the arrays null at
    //  compile time a caller's code is what it was without them)
    if (noise_row) row0 = noise_row[b] - b;
    if (row_step0) step0 = row_step0[b];
    const uint4 rnd = philox4x32(make_uint4((uint32_t)lane, (uint32_t)(row0 + b),
                                            (uint32_t)step + step0, 0u),
                                 make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    return floatx4{exp1_from_u32(rnd.x), exp1_from_u32(rnd.y), exp1_from_u32(rnd.z),
                   exp1_from_u32(rnd.w)};
}

// log q of a lane's 4 noise values (computed ahead of the logits: off the critical path)
__device__ __forceinline__ floatx4 log_noise(const floatx4& q) {
    return floatx4{logf(q[0]), logf(q[1]), logf(q[2]), logf(q[3])};
}

// The two halves of a row's draw as sample_row_ctrl uses them (sample_row below spells out
// the same operations: for identical scores every kernel returns the same index).
// Index of the largest of the row's 256 scores t (lane holds 4 lane + j), first index on ties.
__device__ __forceinline__ int row_argmax(const floatx4& t, int lane) {
    float best = t[0];
    int bi = 4 * lane;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        if (t[j] > best) { best = t[j]; bi = 4 * lane + j; }
    }
    return __builtin_amdgcn_readfirstlane(wave_argmax(best, bi));
}
// log_softmax of the row's logits v to logp_row
__device__ __forceinline__ void row_logp(const floatx4& v, float* logp_row, int lane) {
    float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    m = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += expf(v[j] - m);
    s = wave_sum(s);
    const float ls = logf(s);
#pragma unroll
    for (int j = 0; j < 4; ++j) logp_row[4 * lane + j] = (v[j] - m) - ls;
}

// The step's score pair of a row: {log-prob of the step's sample x, entropy of softmax(z)} in
// nats, both of the model's own distribution whatever the controls did to the draw; x is the
// index drawn, or the caller's sample at a forced step (wave-uniform).  Operation order, the
// same in every kernel (the per-sample kernels and the persistent loop give identical bits):
//   m = wave_max z;  d_j = z_j - m;  e_j = expf(d_j);  s = wave_sum(((e_0 + e_1) + e_2) + e_3);
//   ls = logf(s)                                        -- row_logp's operations in its order
//   score.x = (z_x - m) - ls                            -- row_logp's logp_row[x], bit for bit:
//             computed in every lane for j = x & 3, read from lane x >> 2
//   u = wave_sum(fma(e_3, d_3, fma(e_2, d_2, fma(e_1, d_1, fma(e_0, d_0, 0)))))
//             (a term with e_j == 0 is 0, also at z_j = -inf)
//   score.y = fmaxf(0, ls - u / s)
// logp_row non-null: the dense row as well, from the same m and ls.
__device__ __forceinline__ float2 row_score(const floatx4& v, int x, float* logp_row, int lane) {
    x = __builtin_amdgcn_readfirstlane(x);
    float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    m = wave_max(m);
    float s = 0.f, u = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float d = v[j] - m, e = expf(d);
        s += e;
        u = __builtin_fmaf(e, e > 0.f ? d : 0.f, u);
    }
    s = wave_sum(s);
    u = wave_sum(u);
    const float ls = logf(s);
    const int jx = x & 3;
    const float zx = jx == 0 ? v[0] : jx == 1 ? v[1] : jx == 2 ? v[2] : v[3];
    const float lpx = __uint_as_float(
        (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint((zx - m) - ls), x >> 2));
    if (logp_row) {
#pragma unroll
        for (int j = 0; j < 4; ++j) logp_row[4 * lane + j] = (v[j] - m) - ls;
    }
    return make_float2(lpx, fmaxf(0.f, ls - u / s));
}

// One wave, one row of Q = 256 logits (lane holds q = 4 lane + j), lq = log_noise(q).
// Returns the sampled index (wave-uniform); writes the row's log-probs to logp_row (if
// non-null).  The draw argmax_j softmax(z)_j / q_j (model.py:514) is taken in log space as
// argmax_j (z_j - log q_j): the softmax normaliser is common to all j, so the index needs no
// reduction but the argmax (first index on ties); log-probs, when asked for, come after.
// (Kept in its own words, not as a call of the two halves above: the persistent loop's plain
//  builds are register-exact as they are.  Same operations in the same order.)
__device__ __forceinline__ int sample_row(const floatx4& v, const floatx4& lq, float* logp_row,
                                          int lane) {
    float best = v[0] - lq[0];
    int bi = 4 * lane;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const float t = v[j] - lq[j];
        if (t > best) { best = t; bi = 4 * lane + j; }
    }
    bi = __builtin_amdgcn_readfirstlane(wave_argmax(best, bi));
    if (logp_row) {
        float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        m = wave_max(m);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += expf(v[j] - m);
        s = wave_sum(s);
        const float ls = logf(s);
#pragma unroll
        for (int j = 0; j < 4; ++j) logp_row[4 * lane + j] = (v[j] - m) - ls;
    }
    return bi;
}

// ---- sampling controls: temperature and top-k, per row ----------------------------------
// Extends the draw of model.py:514-517 (which has neither) in the same log-space form:
//   S = {j : z_j >= v_k}, v_k the k-th largest logit of the row (ties at v_k all kept);
//       k outside [1, Q - 1] is "off": S is every j
//   tau > 0:   x = argmax_{j in S} (z_j - tau log q_j)   (fp32: one fma; at tau = 1 it is
//              z_j - log q_j to the bit, so a default row draws sample_row's index)
//   tau <= 0:  x = argmax_{j in S} z_j                    (greedy; the noise is not read)
// first index on ties in both.  The log-probs stay the model's own log_softmax(z).

// Order-preserving unsigned key of a float and its inverse: a < b => key(a) < key(b), the
// bits come back exactly (-0 keeps its own key, just below +0's)
__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t key) {
    return __uint_as_float(key ^ (~(uint32_t)((int32_t)key >> 31) | 0x80000000u));
}

// Key of the k-th largest (1 <= k <= 256) of a row's 256 keys (4 per lane), wave-uniform, no
// LDS: the largest t with |{key >= t}| >= k, found bit by bit from the top.  Each of the 32
// steps is 4 compares into lane masks, 4 scalar popcounts and a scalar select; there is no
// early exit (every lane runs all 32 steps) and nothing to wait for.  All 64 lanes must be
// active.
__device__ __forceinline__ uint32_t wave_kth_largest_key(const uint32_t (&key)[4], int k) {
    uint32_t t = 0;
#pragma unroll
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t c = t | (1u << bit);
        const int n = __popcll(__ballot(key[0] >= c)) + __popcll(__ballot(key[1] >= c)) +
                      __popcll(__ballot(key[2] >= c)) + __popcll(__ballot(key[3] >= c));
        t = n >= k ? c : t;
    }
    return t;
}

// sample_row with the row's controls (tau, k wave-uniform).  The select comes first and is
// skipped by a wave-uniform branch when k is off.  It holds the row as keys IN PLACE of the
// logits (which are rebuilt from them afterwards, bit for bit), so no more values are live
// across it than across the plain draw: the persistent loop has no registers to spare.  The
// allowed set is then the float compare z_j >= v_k (which also keeps -0 with +0).
__device__ __forceinline__ int sample_row_ctrl(const floatx4& v, const floatx4& lq, float tau,
                                               int k, float* logp_row, int lane) {
    tau = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(tau)));
    k = __builtin_amdgcn_readfirstlane(k);
    floatx4 z = v;
    float vk = -__builtin_inff();
    if (k >= 1 && k <= 255) {
        uint32_t key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = float_key(z[j]);
        // (opaque to the compiler, or it would keep the logits live beside their keys)
        asm volatile("" : "+v"(key[0]), "+v"(key[1]), "+v"(key[2]), "+v"(key[3]));
        vk = key_float(wave_kth_largest_key(key, k));
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = key_float(key[j]);
    }
    floatx4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // (tau <= 0: greedy, the noise is not read -- log q may be -inf)
        const float sc = tau > 0.f ? __builtin_fmaf(-tau, lq[j], z[j]) : z[j];
        t[j] = z[j] >= vk ? sc : -__builtin_inff();
    }
    const int bi = row_argmax(t, lane);
    if (logp_row) row_logp(z, logp_row, lane);
    return bi;
}

// ---- nucleus (top-p), per row -------------------------------------------------------------
// Extends the definition above; S, tau and the draw keep their meaning.  For tau > 0 and
// 0 < p < 1 (anything else, NaN included, is "off"):
//   w_j = exp((z_j - max z) / tau) for j in S,  W = sum_S w_j
//   N = {j in S : z_j >= v_p},  v_p the LARGEST logit value v with
//       sum_{j in S, z_j >= v} w_j >= p W
//   (the smallest set of most probable classes whose tempered mass, renormalised over S,
//    reaches p: the class that crosses p is in, ties at v_p are all kept, as for k)
//   x = argmax_{j in N} (z_j - tau log q_j)
// Mass arithmetic: integer fixed point, u_j = rint(2^22 w_j) (0 outside S).  The largest class
// has u = 2^22 and 256 weights sum to at most 2^30, so every partial sum is an exact 32-bit
// integer whatever the order of the reduction, and the test is  sum >= T,
// T = max(1, ceil(p * float(U))), U = sum u_j.  (Error bound of a normalised partial mass:
// DESIGN.md §3.)

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += dpp_u32<0xB1>(v);
    v += dpp_u32<0x4E>(v);
    v += dpp_u32<0x141>(v);
    v += dpp_u32<0x140>(v);
    uint32_t lo, hi;
    xpair16(v, lo, hi);
    v = lo + hi;
    xpair32(v, lo, hi);
    return lo + hi;
}

// Key of v_p for a row held as keys (4 per lane), vk the top-k threshold (-inf: k off), tau > 0,
// 0 < p < 1, all wave-uniform.  Wave-level like wave_kth_largest_key -- no LDS, no barrier, no
// early exit, 32 steps -- but a step's count is a weighted one: 4 compare-selects and adds per
// lane, an integer wave sum and a scalar select.  The predicate "mass of {key >= c} >= T" is
// monotone in c and true at c = 0 (U >= T), so the bits found from the top give the largest
// such c: the key of the crossing class.  Live across the loop: the 4 keys and their 4 weights.
// Classes outside S weigh 0, so the result is never below vk.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_nucleus_key(const uint32_t (&key)[4], float vk,
                                                     float tau, float p) {
    float z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = key_float(key[j]);
    const float m = wave_max(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
    uint32_t u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        u[j] = z[j] >= vk ? (uint32_t)__builtin_rintf(4194304.0f * expf((z[j] - m) / tau)) : 0u;
    const uint32_t U =
        __builtin_amdgcn_readfirstlane(wave_sum_u32((u[0] + u[1]) + (u[2] + u[3])));
    uint32_t T = (uint32_t)__builtin_ceilf(p * (float)U);
    T = T < 1u ? 1u : T;
    uint32_t t = 0;
#pragma unroll
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t c = t | (1u << bit);
        const uint32_t s = ((key[0] >= c ? u[0] : 0u) + (key[1] >= c ? u[1] : 0u)) +
                           ((key[2] >= c ? u[2] : 0u) + (key[3] >= c ? u[3] : 0u));
        t = __builtin_amdgcn_readfirstlane(wave_sum_u32(s)) >= T ? c : t;
    }
    return t;
}

// sample_row_ctrl with the row's top_p as well (tau, k, p wave-uniform).  Both selects run on
// the row held as keys in place of the logits; each is skipped by a wave-uniform branch when
// its control is off, and with p off the draw is sample_row_ctrl(v, lq, tau, k)'s, bit for bit.
// tau <= 0 (greedy) ignores p.  The allowed set is the float compare z_j >= max(v_k, v_p).
__device__ __forceinline__ int sample_row_ctrl_z(const floatx4& v, const floatx4& lq, float tau,
                                                 int k, float p, floatx4& z, int lane) {
    tau = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(tau)));
    k = __builtin_amdgcn_readfirstlane(k);
    p = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(p)));
    const bool ksel = k >= 1 && k <= 255;
    const bool psel = p > 0.f && p < 1.f && tau > 0.f;
    z = v;
    float vk = -__builtin_inff();
    if (ksel || psel) {
        uint32_t key[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) key[j] = float_key(z[j]);
        // (opaque to the compiler, or it would keep the logits live beside their keys)
        asm volatile("" : "+v"(key[0]), "+v"(key[1]), "+v"(key[2]), "+v"(key[3]));
        if (ksel) vk = key_float(wave_kth_largest_key(key, k));
        if (psel) vk = key_float(wave_nucleus_key(key, vk, tau, p));
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = key_float(key[j]);
    }
    floatx4 t;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // (tau <= 0: greedy, the noise is not read -- log q may be -inf)
        const float sc = tau > 0.f ? __builtin_fmaf(-tau, lq[j], z[j]) : z[j];
        t[j] = z[j] >= vk ? sc : -__builtin_inff();
    }
    return row_argmax(t, lane);
}
__device__ __forceinline__ int sample_row_ctrl(const floatx4& v, const floatx4& lq, float tau,
                                               int k, float p, float* logp_row, int lane) {
    floatx4 z;
    const int bi = sample_row_ctrl_z(v, lq, tau, k, p, z, lane);
    if (logp_row) row_logp(z, logp_row, lane);
    return bi;
}

// The level of a call's sampling controls, from the arrays it was given: 3 with a score buffer
// (level 2 plus row_score: default controls draw the plain stream, so the one scored build
// serves every call), 2 with top_p, 1 with temperature, top_k or a forced prefix (n_forced: the
// controlled builds keep it), else 0.
// The one definition: it picks the samplers' instantiation (CT), the persistent loop's plan
// and its launch check.
inline int sample_ctrl_level(const void* temperature, const void* top_k, const void* top_p,
                             const void* n_forced = nullptr, const void* score = nullptr) {
    return score ? 3 : top_p ? 2 : (temperature || top_k || n_forced) ? 1 : 0;
}

// Autoregressive generation (Generator.__call__, model.py:445-520) on the device.
//
// The reference runs a Python loop per sample: ~10 small kernels + a host<->device
// round trip + a print per tier tick.  Here the whole loop stays on the GPU: the
// sample indices live in a device int64 buffer (never copied back until the end),
// every kernel that depends on the current sample position reads a device-side
// block base `*base` plus a compile-time-constant offset, so one block of 2 top-tier
// periods (2 * lookback samples, every tier ticking an even number of times so the
// GRU state ping-pong returns to buffer 0) is captured once as a hipGraph and
// replayed n_cond / 2 times.  Per sample: L1 gather -> hidden GEMM (relu) -> output
// GEMM -> softmax/sampler; per tier tick: input build -> input GEMM -> GRU cell(s) ->
// upsampling GEMM.
#include <vector>

#include "samplernn_hip_internal.hpp"
#include "ulaw_tables.h"
#include "../../include/samplernn_hip.h"
#include "gen_mlp.hpp"
#include "gru_layer.hpp"
#include "sampler.hpp"

int srnn_mlp_l1_impl(int dtype, const void* tab, const int64_t* x, int64_t ldx, int xoff,
                     const int* base, int B, int Tlen, int upper_dtype, const void* upper,
                     int64_t ldu, void* out, int64_t ldo, int D, int FS0, int Q, hipStream_t s);
int srnn_sample_impl(const float* z, int64_t ldz, int B, const float* noise, uint64_t seed,
                     int row0,
                     const int* base, int off, int L, int64_t* seq, int64_t ldseq,
                     float* logp_out, const float* temperature, const int* top_k,
                     const float* top_p, uint32_t step0, const int* n_forced, float* score,
                     hipStream_t s);
int srnn_sample_origin_impl(const float* z, int64_t ldz, int B, const float* noise,
                            uint64_t seed, int row0, const int* base, int off, int L,
                            int64_t* seq, int64_t ldseq, float* logp_out,
                            const float* temperature, const int* top_k, const float* top_p,
                            uint32_t step0, const int* n_forced, const int* noise_row,
                            const uint32_t* row_step0, float* score, hipStream_t s);
int gen_rows_step0_launch(const void* records, int64_t rw, int word, int B, uint32_t* step0,
                          hipStream_t s);
int gen_rows_err_launch(const int* err, int* sticky, hipStream_t s);

// Fused tier input (build_input + input projection of one tier tick), one row per block:
//   a[s] = 2*deq(seq[b, i - nfs + s]) (s < nfs) | cond[b, i/L - 1, s - nfs]   (rounded to T,
//          as the GEMM path's T operand)
//   x[b, o] = sum_s a[s] W_in[o, s] + bias[o] + add[b][o]
// add = the top tier's per-row bias (speaker + cond/input biases) or the upper tier's
// upsampled conditioning row (model.py:196-220).  in_dim <= 16 + cond_dim is small, so a
// thread per output with the row's inputs in LDS beats a GEMM launch plus an input kernel.
template <typename T>
__global__ __launch_bounds__(256) void tier_input_kernel(
    const int64_t* __restrict__ seq, int64_t ldseq, const int* __restrict__ base, int off,
    int nfs, const float* __restrict__ lut2, const float* __restrict__ cond, int n_cond, int C,
    int L, const T* __restrict__ w_in, int in_dim, const float* __restrict__ bias,
    const float* __restrict__ add, int64_t ldadd, T* __restrict__ x, int D) {
    extern __shared__ float av[];
    const int b = blockIdx.x;
    const int i = *base + off;
    for (int s = threadIdx.x; s < in_dim; s += blockDim.x) {
        float v;
        if (s < nfs) v = lut2[seq[(int64_t)b * ldseq + i - nfs + s]];
        else v = cond[((int64_t)b * n_cond + (i / L - 1)) * C + (s - nfs)];
        av[s] = to_f(from_f<T>(v));
    }
    __syncthreads();
    for (int o = threadIdx.x; o < D; o += blockDim.x) {
        const T* w = w_in + (int64_t)o * in_dim;
        float acc = 0.f;
        for (int s = 0; s < in_dim; ++s) acc += av[s] * to_f(w[s]);
        if (bias) acc += bias[o];
        acc += add[(int64_t)b * ldadd + o];
        x[(int64_t)b * D + o] = from_f<T>(acc);
    }
}

// Same computation tiled over (TI_RB rows) x (TI_OB outputs): the block stages its W_in
// rows (contiguous, coalesced) and its rows' inputs in LDS as fp32 (odd row stride: the 64
// lanes of a wave read 64 distinct banks), so every thread's loads are in flight at once
// instead of one dependent weight load per multiply-add (the per-row kernel above is
// latency-bound: 6 us at in_dim 16, 23 us at 107).  Each (row, output) still accumulates
// over s in order from 0 with the same fused multiply-adds, then + bias + add: results are
// bit-identical to tier_input_kernel.
// The bottom tick's launch also draws the next persistent sample loop's noise (planes
// blockIdx.z >= 1: log q of steps *base + off + s - L, s < nsteps, one wave per (step, row)),
// which saves that loop a launch of its own.
struct NoiseJob {
    const float* noise;      // (T, B, Q) Exp(1) draws, or null -> Philox(seed)
    uint64_t seed;
    int row0;                // global index of row 0 (Philox counters)
    int nsteps;              // 0: no noise work
    float* lq;               // (nsteps, B, Q)
    uint32_t step0;          // Philox step of the call's first sample (streaming)
    const int* noise_row;    // per-row Philox origins (sampler.hpp sample_noise), or null
    const uint32_t* row_step0;
};

// noise plane z >= 1 of a 256-thread launch: one wave per (step, row)
__device__ __forceinline__ void noise_plane(const NoiseJob& nz, const int* base, int off, int L,
                                            int B) {
    const int idx = (((int)blockIdx.z - 1) * (int)(gridDim.x * gridDim.y) +
                     (int)(blockIdx.y * gridDim.x + blockIdx.x)) * 4 + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (idx >= nz.nsteps * B) return;
    const int st = idx / B, b = idx - st * B;
    const int i = *base + off + st;
    *reinterpret_cast<floatx4*>(nz.lq + ((int64_t)st * B + b) * 256 + 4 * lane) =
        log_noise(sample_noise(nz.noise, nz.seed, B, b, i - L, lane, nz.row0, nz.step0,
                               nz.noise_row, nz.row_step0));
}

constexpr int TI_RB = 8, TI_OB = 64;
template <typename T>
__global__ __launch_bounds__(256) void tier_input_tiled_kernel(
    const int64_t* __restrict__ seq, int64_t ldseq, const int* __restrict__ base, int off,
    int nfs, const float* __restrict__ lut2, const float* __restrict__ cond, int n_cond, int C,
    int L, const T* __restrict__ w_in, int in_dim, const float* __restrict__ bias,
    const float* __restrict__ add, int64_t ldadd, T* __restrict__ x, int B, int D,
    NoiseJob nz) {
    if (blockIdx.z > 0) {
        noise_plane(nz, base, off, L, B);
        return;
    }
    extern __shared__ float tsh[];
    const int S1 = in_dim | 1;
    float* wsh = tsh;                       // [TI_OB][S1]
    float* ash = tsh + TI_OB * S1;          // [TI_RB][S1]
    const int o0 = blockIdx.x * TI_OB, b0 = blockIdx.y * TI_RB;
    const int i = *base + off;
    const int nw = min(TI_OB, D - o0) * in_dim;
    for (int e = threadIdx.x; e < nw; e += 256) {
        const int o = e / in_dim, s = e - o * in_dim;
        wsh[o * S1 + s] = to_f(w_in[(int64_t)o0 * in_dim + e]);
    }
    for (int e = threadIdx.x; e < TI_RB * in_dim; e += 256) {
        const int r = e / in_dim, s = e - r * in_dim;
        const int b = min(b0 + r, B - 1);
        float v;
        if (s < nfs) v = lut2[seq[(int64_t)b * ldseq + i - nfs + s]];
        else v = cond[((int64_t)b * n_cond + (i / L - 1)) * C + (s - nfs)];
        ash[r * S1 + s] = to_f(from_f<T>(v));
    }
    __syncthreads();
    const int o = threadIdx.x & 63, rg = threadIdx.x >> 6;
    if (o0 + o >= D) return;
    constexpr int RPT = TI_RB / 4;
    float acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) acc[j] = 0.f;
    const float* wr = wsh + o * S1;
    for (int s = 0; s < in_dim; ++s) {
        const float w = wr[s];
#pragma unroll
        for (int j = 0; j < RPT; ++j) acc[j] += ash[(rg + 4 * j) * S1 + s] * w;
    }
    const float bo = bias ? bias[o0 + o] : 0.f;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int b = b0 + rg + 4 * j;
        if (b >= B) break;
        float v = acc[j];
        if (bias) v += bo;
        v += add[(int64_t)b * ldadd + o0 + o];
        x[(int64_t)b * D + o0 + o] = from_f<T>(v);
    }
}

// ---- folded bottom tick (bf16, one GRU layer) ----------------------------------------
// The bottom tier's tick is x = W_in a + b_in + up_upper[fi]; gi = W_ih x + b_ih; GRU;
// up = W_up h + b_up (model.py:196-244).  With x linear in its three terms it folds to
//     gi = Min a + G[fi],  Min = W_ih W_in (3D x nfs),
//     G[fi] = W_ih up_upper[fi] + W_ih b_in + b_ih = Wfold[fi] h_upper + bfold[fi],
//     Wfold[fi] = W_ih W_up_upper[fi] (3D x D),  bfold[fi] = W_ih (b_up_upper[fi] + b_in) + b_ih
// so the upper tier's tick produces G for all its FS_upper positions with ONE skinny GEMM
// over its h (weights (FS_upper 3D, D), folded once per call) in place of its upsampling
// GEMM, and Min a is 16 multiply-adds per gate.  gh = W_hh h + b_hh of the NEXT tick only
// needs this tick's h, so it rides in this tick's upsampling GEMM (weights [W_up; W_hh]:
// the h operand is streamed once for both).  What stays between the sample loop launches
// is a gate-update kernel and one GEMM, instead of input kernel + GRU-cell GEMM + GEMM.
// Rounding differs from the unfolded bf16 path (x and up_upper are never rounded to bf16;
// the folded weights are), at the same bf16 scale; fp32 models keep the unfolded tick.

// Min[g][s] (row-padded to 16) = sum_o W_ih[g, o] W_in[o, s], and the folded upper-tick bias
// bfold[j][g] = sum_o W_ih[g, o] (b_in[o] + b_up1[j D + o]) + b_ih[g], j < fs1: one wave per
// gate row, once per generate call
constexpr int FOLD_MAX_FS1 = 8;
template <typename T>
__global__ __launch_bounds__(256) void fold_input_kernel(const T* __restrict__ wih,
                                                         const T* __restrict__ win, int nfs,
                                                         const float* __restrict__ bin,
                                                         const float* __restrict__ bih,
                                                         const float* __restrict__ bup1, int fs1,
                                                         float* __restrict__ Min,
                                                         float* __restrict__ bfold, int G3, int D) {
    const int g = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= G3) return;
    constexpr int NA = 17 + FOLD_MAX_FS1;
    float acc[NA];
#pragma unroll
    for (int s = 0; s < NA; ++s) acc[s] = 0.f;
    for (int o = lane; o < D; o += 64) {
        const float w = to_f(wih[(int64_t)g * D + o]);
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (s < nfs) acc[s] += w * to_f(win[(int64_t)o * nfs + s]);
        if (bin) acc[16] += w * bin[o];
#pragma unroll
        for (int j = 0; j < FOLD_MAX_FS1; ++j)
            if (j < fs1 && bup1) acc[17 + j] += w * bup1[(int64_t)j * D + o];
    }
#pragma unroll
    for (int s = 0; s < NA; ++s) acc[s] = wave_sum(acc[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < 16; ++s) Min[(int64_t)g * 16 + s] = acc[s];
        const float c0 = acc[16] + (bih ? bih[g] : 0.f);
#pragma unroll
        for (int j = 0; j < FOLD_MAX_FS1; ++j)
            if (j < fs1) bfold[(int64_t)j * G3 + g] = c0 + acc[17 + j];
    }
}

// gate update of the folded bottom tick: block = FG_RB rows x 256 units (+ noise planes)
constexpr int FG_RB = 2;
template <typename T>
__global__ __launch_bounds__(256) void fold_gru_kernel(
    const int64_t* __restrict__ seq, int64_t ldseq, const int* __restrict__ base, int off,
    int nfs, const float* __restrict__ lut2, int L, const float* __restrict__ Min,
    const float* __restrict__ G, int64_t ldg, const float* __restrict__ gh, int64_t ldgh,
    const float* __restrict__ hp, float* __restrict__ hn, T* __restrict__ hn_lp, int B, int D,
    NoiseJob nz) {
    if (blockIdx.z > 0) {
        noise_plane(nz, base, off, L, B);
        return;
    }
    __shared__ float ash[FG_RB][16];
    const int u = blockIdx.x * 256 + (int)threadIdx.x, b0 = blockIdx.y * FG_RB;
    // every operand that does not depend on the samples is loaded first, so its latency
    // overlaps the seq -> LUT chain below (clamped addresses, no branches)
    const int uc = min(u, D - 1);
    floatx4 mr[4], mz[4], mn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mr[j] = *reinterpret_cast<const floatx4*>(Min + (int64_t)uc * 16 + 4 * j);
        mz[j] = *reinterpret_cast<const floatx4*>(Min + (int64_t)(D + uc) * 16 + 4 * j);
        mn[j] = *reinterpret_cast<const floatx4*>(Min + (int64_t)(2 * D + uc) * 16 + 4 * j);
    }
    float gv[FG_RB][6], hv[FG_RB];
#pragma unroll
    for (int r = 0; r < FG_RB; ++r) {
        const int b = min(b0 + r, B - 1);
        const float* gr = G + (int64_t)b * ldg;
        const float* hr = gh + (int64_t)b * ldgh;
        gv[r][0] = gr[uc]; gv[r][1] = gr[D + uc]; gv[r][2] = gr[2 * D + uc];
        gv[r][3] = hr[uc]; gv[r][4] = hr[D + uc]; gv[r][5] = hr[2 * D + uc];
        hv[r] = hp[(int64_t)b * D + uc];
    }
    if (threadIdx.x < FG_RB * 16) {
        const int r = threadIdx.x >> 4, s = threadIdx.x & 15;
        const int b = min(b0 + r, B - 1);
        const int i = *base + off;
        // a[s] = 2 deq(seq[b, i - nfs + s]) rounded to T, as the unfolded input's operand
        ash[r][s] = s < nfs ? to_f(from_f<T>(lut2[seq[(int64_t)b * ldseq + i - nfs + s]])) : 0.f;
    }
    __syncthreads();
    if (u >= D) return;
#pragma unroll
    for (int r = 0; r < FG_RB; ++r) {
        const int b = b0 + r;
        if (b >= B) break;
        float gir = gv[r][0], giz = gv[r][1], gin = gv[r][2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float a = ash[r][4 * j + e];
                gir += a * mr[j][e];
                giz += a * mz[j][e];
                gin += a * mn[j][e];
            }
        const float ghr = gv[r][3], ghz = gv[r][4], ghn = gv[r][5];
        const float rg = 1.0f / (1.0f + expf(-(ghr + gir)));
        const float zg = 1.0f / (1.0f + expf(-(ghz + giz)));
        const float ng = tanhf(gin + ghn * rg);
        const float v = (hv[r] - ng) * zg + ng;
        hn[(int64_t)b * D + u] = v;
        hn_lp[(int64_t)b * D + u] = from_f<T>(v);
    }
}

// Input row of the folded top tick: a[b][s] = 2 deq(seq[b, i - nfs + s]) (s < nfs) |
// cond[b, i/L - 1, s - nfs] (s < in_dim) | 0 (s < AP), rounded to T as the unfolded input's
// GEMM operand; gi = a . Min1^T + P1[b] then replaces x = W_in a + row_bias, gi = W_ih x + b_ih
// (Min1 = W_ih W_in, P1 = W_ih row_bias + b_ih, folded once per call).  Two rows per block;
// planes blockIdx.z >= 1 draw the noise of the persistent launches of the tick's period.
constexpr int TA_AP = 128;
template <typename T>
__global__ __launch_bounds__(256) void tier_a_kernel(
    const int64_t* __restrict__ seq, int64_t ldseq, const int* __restrict__ base, int off,
    int nfs, const float* __restrict__ lut2, const float* __restrict__ cond, int n_cond, int C,
    int L, int in_dim, T* __restrict__ a, int B, NoiseJob nz) {
    if (blockIdx.z > 0) {
        noise_plane(nz, base, off, L, B);
        return;
    }
    const int b = blockIdx.x * 2 + (int)(threadIdx.x >> 7), s = threadIdx.x & 127;
    if (b >= B) return;
    const int i = *base + off;
    float v = 0.f;
    if (s < nfs) v = lut2[seq[(int64_t)b * ldseq + i - nfs + s]];
    else if (s < in_dim) v = cond[((int64_t)b * n_cond + (i / L - 1)) * C + (s - nfs)];
    a[(int64_t)b * TA_AP + s] = from_f<T>(v);
}

template <typename T>
__global__ void init_state_kernel(const float* __restrict__ h0, float* __restrict__ h,
                                  T* __restrict__ hlp, int B, int D) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B * D) return;
    const float v = h0[e % D];
    h[e] = v;
    if (hlp) hlp[e] = from_f<T>(v);
}

__global__ void advance_kernel(int* base, int by) { *base += by; }

template <typename T>
__global__ void copy_cast_kernel(const float* __restrict__ src, T* __restrict__ dst, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) dst[e] = from_f<T>(src[e]);
}

// ---- carried state (srnn_generate5) -----------------------------------------------------
// One record per row, in 4-byte words:
//   [0, 16)   header: tag, dtype, n_tiers, n_rnn, dim, L, fold flags, 0, steps (int64), 0...
//   [16, +L)  the row's last L sample indices (int32)
//   then      h of every (tier, layer), fp32, D each
//   then      fold only: gh of the next bottom tick (3D), gh1 of the next upper tick (3D)
// The T copies of h are not stored: every producer (fold_gru_kernel, the in-launch gate update,
// the GRU cell kernels) writes from_f<T>(h) beside the fp32 h, and so does the unpack.  The gh
// rows ARE stored: at a fresh start linear_fwd computes them, mid-stream the concatenated-weight
// GEMMs do, and the two need not agree to the bit.
constexpr uint32_t GS_TAG = 0x314E5253u;       // "SRN1"
constexpr int GS_HDR = 16;
struct GenStateMap {
    int L, D, n_h, fold;
    float* h[SRNN_MAX_TIERS * SRNN_MAX_RNN];    // pack: the live buffer; unpack: buffer [0]
    void* hlp[SRNN_MAX_TIERS * SRNN_MAX_RNN];   // unpack: the T copy, or null (fp32: h itself)
    float* gh0;
    int64_t ldgh0;
    float* gh1;
    int64_t ldgh1;
    uint32_t hdr[8];                            // words [0, 8) of a record of this call
    uint32_t q_zero;                            // the history of a fresh record (pack, no seq)
};

// grid (words of a record / 256, B): word w of row b
template <typename T>
__global__ __launch_bounds__(256) void gen_state_unpack_kernel(
    const uint32_t* __restrict__ st, int64_t rw, GenStateMap mp, int64_t* __restrict__ seq,
    int64_t ldseq) {
    int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x - GS_HDR;
    const int b = blockIdx.y;
    if (w < 0 || w + GS_HDR >= rw) return;
    const uint32_t v = st[(int64_t)b * rw + GS_HDR + w];
    if (w < mp.L) {
        seq[(int64_t)b * ldseq + w] = (int64_t)(v & 255u);
        return;
    }
    w -= mp.L;
    const int D = mp.D;
    if (w < (int64_t)mp.n_h * D) {
        const int j = (int)(w / D), u = (int)(w - (int64_t)j * D);
        const float f = __uint_as_float(v);
        mp.h[j][(int64_t)b * D + u] = f;
        if (mp.hlp[j]) ((T*)mp.hlp[j])[(int64_t)b * D + u] = from_f<T>(f);
        return;
    }
    w -= (int64_t)mp.n_h * D;
    if (!mp.fold) return;
    if (w < 3 * D) mp.gh0[(int64_t)b * mp.ldgh0 + w] = __uint_as_float(v);
    else if (w < 6 * D) mp.gh1[(int64_t)b * mp.ldgh1 + (w - 3 * D)] = __uint_as_float(v);
}

// The reverse; st_in (or null: a fresh start) supplies the rows' earlier step counts and may be
// st_out itself: only the thread that writes a row's count reads it.  The rows' last L samples
// are seq columns [hist, hist + L) (a call: its last; a session's chunk: the chunk's last).
__global__ __launch_bounds__(256) void gen_state_pack_kernel(
    uint32_t* __restrict__ st_out, const uint32_t* st_in, int64_t rw, GenStateMap mp,
    const int64_t* __restrict__ seq, int64_t ldseq, int64_t hist, int64_t T) {
    int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (w >= rw) return;
    uint32_t* o = st_out + (int64_t)b * rw;
    if (w < GS_HDR) {
        if (w == 8) {
            int64_t steps = T;
            if (st_in) steps += *reinterpret_cast<const int64_t*>(st_in + (int64_t)b * rw + 8);
            *reinterpret_cast<int64_t*>(o + 8) = steps;
        } else if (w != 9) {
            o[w] = w < 8 ? mp.hdr[w] : 0u;
        }
        return;
    }
    w -= GS_HDR;
    const int D = mp.D;
    uint32_t v = 0u;
    if (w < mp.L) {
        // (no seq: the q_zero history of a stream that has done no step)
        v = seq ? (uint32_t)seq[(int64_t)b * ldseq + hist + w] : mp.q_zero;
    } else if (w - mp.L < (int64_t)mp.n_h * D) {
        const int64_t e = w - mp.L;
        const int j = (int)(e / D), u = (int)(e - (int64_t)j * D);
        v = __float_as_uint(mp.h[j][(int64_t)b * D + u]);
    } else if (mp.fold) {
        const int64_t e = w - mp.L - (int64_t)mp.n_h * D;
        if (e < 3 * D) v = __float_as_uint(mp.gh0[(int64_t)b * mp.ldgh0 + e]);
        else if (e < 6 * D) v = __float_as_uint(mp.gh1[(int64_t)b * mp.ldgh1 + (e - 3 * D)]);
    }
    o[GS_HDR + w] = v;
}

namespace {

constexpr size_t ALIGN = 256;
inline size_t al(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

struct Bufs {
    void* x[SRNN_MAX_TIERS];
    float* h[SRNN_MAX_TIERS][SRNN_MAX_RNN][2];
    void* hlp[SRNN_MAX_TIERS][SRNN_MAX_RNN][2];
    float* up[SRNN_MAX_TIERS];
    void* a1;
    void* a2;
    float* logits;
    float* lut2;
    int* base;
    // persistent sample loop (gen_mlp.hip): hand-off granules + error word, one zeroed block
    unsigned long long* xa1;
    unsigned long long* xa2;
    void* wfr_hid;                   // fragment-order weight images (gen_mlp_prep_weights)
    void* wfr_out;
    unsigned long long* xz;
    int* gerr;
    float* lq;               // (lq_steps, B, Q) log q of the persistent launches' draws
    int lq_steps;            // FS0, or the upper tier's period FS0 FS1 when that tick draws
    size_t gm_bytes;
    // folded bottom tick (fold_ok): up[0] rows are [up (FS0 D) | gh of the next tick (3D)]
    bool fold;
    int64_t ldup0;           // row stride of up[0]
    void* wcat;              // (FS0 D + 3D, D) [W_up; W_hh] of the bottom tier
    float* bcat;             // [b_up; b_hh]
    float* fmin;             // (3D, 16) W_ih W_in, rows zero-padded
    void* wfold;             // (FS1 3D + 3D, D) [W_ih0 W_up1[j], j < FS1; W_hh1]
    float* bfold;            // (FS1 3D + 3D) [bfold[j]; b_hh1]
    GenMlpArgs::Tick* ticks; // [fi][cur]: the persistent loop's gate-update operands
    // folded top tick (fold_top: two tiers, the upper one is the top)
    bool fold_top;
    void* min1;              // (3D, TA_AP) W_ih1 W_in1, zero columns past in_dim
    float* p1;               // (B, 3D) W_ih1 row_bias + b_ih1
    void* atop;              // (B, TA_AP) the top tick's input row
    float* fg;               // (B, ldg1): [G of the current upper frame | gh1 of the next
    int64_t ldg1;            //  upper tick], ldg1 = FS1 3D + 3D
};

// The environment switches of the host driver, read once per call (tests flip them between
// calls of one process) so that every layout decision of a call sees the same values.
struct GenSwitches {
    bool fold, fold_f32, fold_top, noise_ahead, fuse_gates, persist;
    static GenSwitches read() {
        return {env_flag("SRNN_GEN_FOLD", 1) != 0,        env_flag("SRNN_GEN_FOLD_F32", 1) != 0,
                env_flag("SRNN_GEN_FOLD_TOP", 1) != 0,    env_flag("SRNN_GEN_NOISE_AHEAD", 1) != 0,
                env_flag("SRNN_GEN_FUSE_GATES", 1) != 0,  env_flag("SRNN_GEN_PERSIST", 1) != 0};
    }
};

// fp32 too (SRNN_GEN_FOLD_F32=0: unfolded fp32 ticks): the folds reassociate fp32 sums
// (W_ih (W_in a + b) -> (W_ih W_in) a + W_ih b), same precision, rounding in the last bits.
// The folded upper tick hands its carried gh to the GRU cell, which takes a precomputed gh in
// its ring form only: dim a multiple of the ring's k stage, 256 bytes (128 in bf16, 64 in fp32);
// other widths keep the unfolded ticks.
bool fold_ok(const SrnnModel* m, const GenSwitches& sw) {
    const SrnnTier& t = m->tier[0];
    return (m->dtype == SRNN_BF16 ? m->dim % 128 == 0 : (sw.fold_f32 && m->dim % 64 == 0)) &&
           m->n_tiers >= 2 &&
           m->n_rnn == 1 &&
           t.in_dim == t.n_frame_samples && t.n_frame_samples <= 16 && t.b_up &&
           m->tier[1].frame_size <= FOLD_MAX_FS1 &&
           sw.fold;
}

// carve (or size, if ws == nullptr) the workspace
size_t carve(const SrnnModel* m, int B, char* ws, Bufs* b, const GenMlpPlan* pl,
             const GenSwitches& sw) {
    const int D = m->dim, Q = m->q_levels;
    const size_t es = m->dtype == SRNN_F32 ? 4 : 2;
    const bool lp = m->dtype != SRNN_F32;
    size_t off = 0;
    auto take = [&](size_t bytes) -> char* {
        char* p = ws ? ws + off : nullptr;
        off += al(bytes);
        return p;
    };
    for (int k = 0; k < m->n_tiers; ++k) {
        const SrnnTier& t = m->tier[k];
        b->x[k] = take((size_t)B * D * es);
        for (int l = 0; l < m->n_rnn; ++l)
            for (int p = 0; p < 2; ++p) {
                b->h[k][l][p] = (float*)take((size_t)B * D * 4);
                b->hlp[k][l][p] = lp ? (void*)take((size_t)B * D * es) : (void*)b->h[k][l][p];
            }
        b->up[k] = (float*)take((size_t)B * (t.frame_size + 3) * D * 4);
    }
    b->fold = fold_ok(m, sw);
    b->ldup0 = (int64_t)m->tier[0].frame_size * D + (b->fold ? 3 * D : 0);
    b->wcat = nullptr;
    b->wfold = nullptr;
    b->ticks = nullptr;
    b->fold_top = false;
    b->min1 = b->atop = nullptr;
    b->p1 = nullptr;
    b->ldg1 = 0;
    b->bcat = b->fmin = b->bfold = b->fg = nullptr;
    if (b->fold) {
        const int N0 = m->tier[0].frame_size * D + 3 * D;
        b->wcat = take((size_t)N0 * D * es);
        b->bcat = (float*)take((size_t)N0 * 4);
        b->fmin = (float*)take((size_t)3 * D * 16 * 4);
        const int F1 = m->tier[1].frame_size;
        b->ldg1 = (int64_t)(F1 + 1) * 3 * D;
        b->wfold = take((size_t)b->ldg1 * D * es);
        b->bfold = (float*)take((size_t)b->ldg1 * 4);
        b->fg = (float*)take((size_t)B * b->ldg1 * 4);
        b->ticks = (GenMlpArgs::Tick*)take((size_t)2 * F1 * sizeof(GenMlpArgs::Tick));
        b->fold_top = m->n_tiers == 2 && m->tier[1].in_dim <= TA_AP && sw.fold_top;
        if (b->fold_top) {
            b->min1 = take((size_t)3 * D * TA_AP * es);
            b->p1 = (float*)take((size_t)B * 3 * D * 4);
            b->atop = take((size_t)B * TA_AP * es);
        }
    }
    b->a1 = take((size_t)B * D * es);
    b->a2 = take((size_t)B * D * es);
    b->logits = (float*)take((size_t)B * Q * 4);
    b->lut2 = (float*)take((size_t)Q * 4);
    b->base = (int*)take(64);
    b->xa1 = b->xa2 = b->xz = nullptr;
    b->wfr_hid = b->wfr_out = nullptr;
    b->gerr = nullptr;
    b->lq = nullptr;
    b->lq_steps = 0;
    b->gm_bytes = 0;
    if (pl && pl->ok) {
        const size_t start = off;
        b->gerr = (int*)take(8192);          // [0] error word, [64..) 2 keyed census arrays
        b->xa1 = (unsigned long long*)take(pl->xa_words * 8);
        b->xa2 = (unsigned long long*)take(pl->xa_words * 8);
        b->xz = (unsigned long long*)take(pl->xz_words * 8);
        b->lq_steps = m->tier[0].frame_size * (b->fold ? m->tier[1].frame_size : 1);
        b->lq = (float*)take((size_t)b->lq_steps * B * Q * 4);
        b->gm_bytes = off - start;
        // (after the block a call zeroes at its start: the images depend on the model alone)
        b->wfr_hid = pl->wfr_hid_bytes ? take(pl->wfr_hid_bytes) : nullptr;
        b->wfr_out = pl->wfr_out_bytes ? take(pl->wfr_out_bytes) : nullptr;
    }
    return off;
}

// Everything one generation call is given (the arguments of srnn_generate5, st unpacked), in
// the entries' parameter order: each extern "C" entry fills one by aggregate initialisation.
struct GenRequest {
    const SrnnModel* m;
    int n_seqs, n_cond;
    const float* cond;
    const float* row_bias;
    const float* noise;
    uint64_t seed;
    int row0;                             // global index of row 0 (rank-sharded generation)
    int64_t* seq;
    float* logp;
    void* workspace;
    size_t workspace_bytes;
    int flags;
    hipStream_t stream;
    const float* temperature = nullptr;   // per-row sampling controls (device, n_seqs), or null
    const int* top_k = nullptr;
    const float* top_p = nullptr;         // nucleus mass (device, n_seqs), or null
    const void* state_in = nullptr;       // carried state records (device), or null
    void* state_out = nullptr;
    size_t state_bytes = 0;
    uint32_t step0 = 0;                   // Philox step of sample L (steps done before the call)
    const int* n_forced = nullptr;        // per-row forced prefix lengths (device), or null
    const int* noise_row = nullptr;       // per-row Philox row (device, n_seqs), or null: row0 + b
    const uint32_t* row_step0 = nullptr;  // per-row Philox step origin (device), or null: step0
    float* score = nullptr;               // (n_cond L, n_seqs, 2) score pairs (device), or null
    bool row_origins() const { return noise_row || row_step0; }
    int level() const {
        return sample_ctrl_level(temperature, top_k, top_p, n_forced, score);
    }
};

// f(T{}) launches a kernel's instantiation for T, the element type of `dtype`
// (gemm_dispatch_types' idiom), and the launch is checked: a launch that differs between the
// dtypes only in its casts is written once
template <typename F>
inline int gen_typed_launch(int dtype, F&& f) {
    if (dtype == SRNN_F32) f(float{});
    else f(bf16{});
    SRNN_LAUNCH_CHECK();
    return 0;
}

// The private stream a call runs on (so that a hipGraph can be captured whatever the caller's
// stream is), the event that orders it after the caller's, and the captured block.  Released on
// every path; gen_finish has drained the stream by then.
struct GenStream {
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    GenStream() = default;
    GenStream(const GenStream&) = delete;
    GenStream& operator=(const GenStream&) = delete;
    int open(hipStream_t user) {
        SRNN_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        SRNN_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        SRNN_CHECK_HIP(hipEventRecord(ev, user));
        SRNN_CHECK_HIP(hipStreamWaitEvent(s, ev, 0));
        return 0;
    }
    ~GenStream() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        if (ev) (void)hipEventDestroy(ev);
        if (s) (void)hipStreamDestroy(s);
    }
};

struct Ctx {
    const GenRequest& rq;
    const GenSwitches sw;
    const bool fresh = false; // srnn_gen_state_fresh: the start of a call and its record, no step
    GenStream gs;
    Bufs b{};
    int L = 0;                // the top tier's period
    int64_t T = 0;            // steps of this call, n_cond L
    int64_t ldseq = 0;
    int64_t rw = 0;           // words of a state record
    hipStream_t s = nullptr;  // the call's private stream
    GenMlpPlan plan{};
    const GenMlpPlan* pl = nullptr;   // &plan (persistent sample loop), or null: per-sample kernels
    // lq holds the draws of block-relative steps [noise_beg, noise_end): drawn ahead by the
    // input launch of the bottom tick (FS0 steps) or, with the folded bottom tick, of the
    // upper tier's tick (its whole period)
    int noise_beg = 0, noise_end = -1;
    bool gate_done = false;   // the last persistent launch did the next bottom tick's gates
    // the folded bottom tick's GEMM runs inside the persistent launch that follows it
    // (GenMlpArgs::tg): set by tier_tick, consumed by that launch
    bool tick_gemm = false;
    GenMlpArgs::TickGemm pending{};
    GenStateMap mp{};         // the call's state record layout (header, gh rows; h per use)
    // a launch's noise source, drawing nothing ahead (the upper tick drew them) until given lq
    NoiseJob noise_job() const {
        return {rq.noise, rq.seed, rq.row0, 0, nullptr, rq.step0, rq.noise_row, rq.row_step0};
    }
};

#define RET(x) do { int _r = (x); if (_r) return _r; } while (0)

// one tier tick at block-relative offset `off`; `par` = tick parity of this tier
int tier_tick(Ctx& c, int k, int off, int par) {
    const GenRequest& r = c.rq;
    const SrnnModel* m = r.m;
    const SrnnTier& t = m->tier[k];
    const int D = m->dim, B = r.n_seqs, dt = m->dtype;
    const bool top = (k == m->n_tiers - 1);
    const bool lp = dt != SRNN_F32;
    const int cur = par, nxt = par ^ 1;
    if (k == 0 && c.b.fold) {
        // folded bottom tick: gate update (gi = Min a + G[fi], gh from the last tick's GEMM),
        // then [up | gh'] = h [W_up; W_hh]^T + [b_up; b_hh]
        const SrnnTier& u = m->tier[1];
        const int fi = (off / t.n_frame_samples) % u.frame_size;
        const NoiseJob nz = c.noise_job();
        const dim3 g2(cdiv(D, 256), cdiv(B, FG_RB), 1);
        const int64_t fs0d = (int64_t)t.frame_size * D;
        // [up | gh'] = h [W_up; W_hh]^T + [b_up; b_hh]: its own launch, or inside the
        // persistent launch that follows (c.tick_gemm)
        auto tick_gemm = [&]() -> int {
            if (c.tick_gemm) {
                SRNN_REQUIRE(c.pending.N == 0, "generate: tick GEMM left unconsumed");
                c.pending.A = c.b.hlp[0][0][nxt];
                c.pending.W = c.b.wcat;
                c.pending.bias = c.b.bcat;
                c.pending.C = c.b.up[0];
                c.pending.ldc = c.b.ldup0;
                c.pending.N = (int)(fs0d + 3 * D);
                c.pending.K = D;
                return 0;
            }
            return linear_fwd(dt, SRNN_F32, B, (int)(fs0d + 3 * D), D, c.b.hlp[0][0][nxt], D,
                              c.b.wcat, D, c.b.bcat, c.b.up[0], c.b.ldup0, 0, c.s);
        };
        if (c.gate_done) {
            // the gate update ran at the end of the last persistent launch (GenMlpArgs::tk)
            c.gate_done = false;
            return tick_gemm();
        }
        RET(gen_typed_launch(dt, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL((fold_gru_kernel<T>), g2, dim3(256), 0, c.s, r.seq, c.ldseq,
                               c.b.base, off, t.n_frame_samples, c.b.lut2, c.L, c.b.fmin,
                               c.b.fg + (size_t)fi * 3 * D, c.b.ldg1, c.b.up[0] + fs0d, c.b.ldup0,
                               c.b.h[0][0][cur], c.b.h[0][0][nxt], (T*)c.b.hlp[0][0][nxt], B, D,
                               nz);
        }));
        return tick_gemm();
    }
    if (k == 1 && c.b.fold_top) {
        // folded top tick: a (+ the period's noise) -> gi = a Min1^T + P1, gh1 carried ->
        // [G | gh1'] = h [Wfold; W_hh1]^T + [bfold; b_hh1]
        NoiseJob nz = c.noise_job();
        const int gx = cdiv(B, 2);
        int planes = 1;
        if (c.pl && c.b.lq && c.sw.noise_ahead) {
            nz.nsteps = c.b.lq_steps;
            nz.lq = c.b.lq;
            planes = 1 + cdiv(cdiv((int64_t)nz.nsteps * B, 4), gx);
            c.noise_beg = off;
            c.noise_end = off + nz.nsteps;
        }
        RET(gen_typed_launch(dt, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL((tier_a_kernel<T>), dim3(gx, 1, planes), dim3(256), 0, c.s, r.seq,
                               c.ldseq, c.b.base, off, t.n_frame_samples, c.b.lut2, r.cond,
                               r.n_cond, m->cond_dim, c.L, t.in_dim, (T*)c.b.atop, B, nz);
        }));
        const int64_t g0 = (int64_t)t.frame_size * 3 * D;
        RET(srnn_gru_cell_x_impl(dt, B, D, TA_AP, c.b.atop, TA_AP, c.b.min1, nullptr, c.b.p1,
                                 3 * D, c.b.fg + g0, c.b.ldg1, c.b.h[k][0][cur], D,
                                 c.b.h[k][0][nxt], D, c.b.hlp[k][0][nxt], D, c.s));
        return linear_fwd(dt, SRNN_F32, B, (int)c.b.ldg1, D, c.b.hlp[k][0][nxt], D, c.b.wfold,
                          D, c.b.bfold, c.b.fg, c.b.ldg1, 0, c.s);
    }
    // 1. x = A_in . W_in^T + (top: row_bias ; lower: b_in + upper-tier conditioning row)
    {
        const float* add;
        int64_t ldadd;
        const float* bias;
        if (top) {
            add = r.row_bias; ldadd = D; bias = nullptr;
        } else {
            const SrnnTier& u = m->tier[k + 1];
            // frame_index = (i // nfs_k) % FS_{k+1}  (model.py:491-492); base is a multiple of L
            const int fi = (off / t.n_frame_samples) % u.frame_size;
            add = c.b.up[k + 1] + (size_t)fi * D; ldadd = (int64_t)u.frame_size * D;
            bias = t.b_in;
        }
        const size_t tlds = (size_t)(TI_OB + TI_RB) * (t.in_dim | 1) * sizeof(float);
        if (tlds <= 160 * 1024) {
            NoiseJob nz = c.noise_job();
            int planes = 1;
            if (k == (c.b.fold ? 1 : 0) && c.pl && c.b.lq && c.sw.noise_ahead) {
                nz.nsteps = c.b.lq_steps;             // the persistent launches after this tick
                nz.lq = c.b.lq;
                const int per = cdiv(D, TI_OB) * cdiv(B, TI_RB);
                planes = 1 + cdiv(cdiv((int64_t)nz.nsteps * B, 4), per);
                c.noise_beg = off;
                c.noise_end = off + nz.nsteps;
            }
            const dim3 grid(cdiv(D, TI_OB), cdiv(B, TI_RB), planes);
            // (attribute raised once, to the whole LDS, before the first launch that needs it)
            if (tlds > 65536)
                RET(srnn_raise_lds(dt == SRNN_F32 ? (const void*)tier_input_tiled_kernel<float>
                                                  : (const void*)tier_input_tiled_kernel<bf16>,
                                   160 * 1024));
            RET(gen_typed_launch(dt, [&](auto z) {
                using T = decltype(z);
                hipLaunchKernelGGL((tier_input_tiled_kernel<T>), grid, dim3(256), tlds, c.s, r.seq,
                                   c.ldseq, c.b.base, off, t.n_frame_samples, c.b.lut2, r.cond,
                                   r.n_cond, m->cond_dim, c.L, (const T*)t.w_in, t.in_dim, bias,
                                   add, ldadd, (T*)c.b.x[k], B, D, nz);
            }));
        } else {
            const size_t lds = (size_t)t.in_dim * sizeof(float);
            RET(gen_typed_launch(dt, [&](auto z) {
                using T = decltype(z);
                hipLaunchKernelGGL((tier_input_kernel<T>), dim3(B), dim3(256), lds, c.s, r.seq,
                                   c.ldseq, c.b.base, off, t.n_frame_samples, c.b.lut2, r.cond,
                                   r.n_cond, m->cond_dim, c.L, (const T*)t.w_in, t.in_dim, bias,
                                   add, ldadd, (T*)c.b.x[k], D);
            }));
        }
    }
    // 3. GRU layers
    if (k == 1 && c.b.fold) {
        // folded upper tick: gh carried by its last GEMM ([Wfold; W_hh1] . h)
        const int64_t g0 = (int64_t)t.frame_size * 3 * D;
        RET(srnn_gru_cell_x_impl(dt, B, D, D, c.b.x[k], D, t.w_ih[0], t.b_ih[0], nullptr, 0,
                                 c.b.fg + g0, c.b.ldg1, c.b.h[k][0][cur], D, c.b.h[k][0][nxt], D,
                                 c.b.hlp[k][0][nxt], D, c.s));
        // G = h . Wfold^T + bfold and the next tick's gh1, (B, ldg1) fp32
        return linear_fwd(dt, SRNN_F32, B, (int)c.b.ldg1, D, c.b.hlp[k][0][nxt], D, c.b.wfold,
                          D, c.b.bfold, c.b.fg, c.b.ldg1, 0, c.s);
    }
    for (int l = 0; l < m->n_rnn; ++l) {
        const void* xin = l == 0 ? c.b.x[k] : c.b.hlp[k][l - 1][nxt];
        RET(srnn_gru_cell_impl(dt, B, D, D, xin, D, t.w_ih[l], t.b_ih[l], nullptr, 0,
                               c.b.hlp[k][l][cur], D, c.b.h[k][l][cur], D, t.w_hh[l], t.b_hh[l],
                               c.b.h[k][l][nxt], D, lp ? c.b.hlp[k][l][nxt] : nullptr, D, nullptr,
                               0, c.s));
    }
    // 4. LearnedUpsampling1d: up = h . W_up^T + b_up   (B, fs*D) fp32
    RET(linear_fwd(dt, SRNN_F32, B, t.frame_size * D, D, c.b.hlp[k][m->n_rnn - 1][nxt], D, t.w_up,
                   D, t.b_up, c.b.up[k], (int64_t)t.frame_size * D, 0, c.s));
    return 0;
}

int mlp_step(Ctx& c, int off) {
    const GenRequest& r = c.rq;
    const SrnnModel* m = r.m;
    const int D = m->dim, Q = m->q_levels, B = r.n_seqs, dt = m->dtype;
    const int FS0 = m->tier[0].frame_size;
    RET(srnn_mlp_l1_impl(dt, m->tab, r.seq, c.ldseq, off - FS0, c.b.base, B, 1, SRNN_F32,
                         c.b.up[0] + (size_t)(off % FS0) * D, c.b.ldup0, c.b.a1, D, D, FS0,
                         Q, c.s));
    RET(linear_fwd(dt, dt, B, D, D, c.b.a1, D, m->w_hid, D, m->b_hid, c.b.a2, D, 1, c.s));
    RET(linear_fwd(dt, SRNN_F32, B, Q, D, c.b.a2, D, m->w_out, D, m->b_out, c.b.logits, Q, 0,
                   c.s));
    if (r.row_origins())
        return srnn_sample_origin_impl(c.b.logits, Q, B, r.noise, r.seed, r.row0, c.b.base, off,
                                       c.L, r.seq, c.ldseq, r.logp, r.temperature, r.top_k,
                                       r.top_p, r.step0, r.n_forced, r.noise_row, r.row_step0,
                                       r.score, c.s);
    RET(srnn_sample_impl(c.b.logits, Q, B, r.noise, r.seed, r.row0, c.b.base, off, c.L, r.seq,
                         c.ldseq, r.logp, r.temperature, r.top_k, r.top_p, r.step0, r.n_forced,
                         r.score, c.s));
    return 0;
}

// `periods` consecutive top-tier periods starting at sample *base; tick parity restarts
// at 0 (callers only chain blocks with an even tick count per tier)
int run_block(Ctx& c, int periods) {
    const GenRequest& r = c.rq;
    const SrnnModel* m = r.m;
    int ticks[SRNN_MAX_TIERS] = {0};
    c.noise_end = -1;
    c.gate_done = false;
    for (int off = 0; off < periods * c.L; ++off) {
        for (int k = m->n_tiers - 1; k >= 0; --k) {
            if (off % m->tier[k].n_frame_samples != 0) continue;
            RET(tier_tick(c, k, off, ticks[k] & 1));
            ticks[k]++;
        }
        if (!c.pl) {
            RET(mlp_step(c, off));
        } else if (off % m->tier[0].frame_size == 0) {
            // the FS0 samples up to the next bottom-tier tick in one persistent launch
            GenMlpArgs a;
            memset(&a, 0, sizeof(a));
            a.tab = m->tab; a.w_hid = m->w_hid; a.b_hid = m->b_hid;
            a.w_out = m->w_out; a.b_out = m->b_out;
            a.wfr_hid = c.b.wfr_hid; a.wfr_out = c.b.wfr_out;
            a.up0 = c.b.up[0]; a.ldup = c.b.ldup0;
            a.noise = r.noise; a.seed = r.seed; a.row0 = r.row0;
            a.seq = r.seq; a.ldseq = c.ldseq; a.logp = r.logp;
            a.base = c.b.base; a.off = off; a.nsteps = m->tier[0].frame_size; a.L = c.L;
            a.B = r.n_seqs; a.D = m->dim; a.FS0 = m->tier[0].frame_size;
            a.xa1 = c.b.xa1; a.xa2 = c.b.xa2; a.xz = c.b.xz; a.err = c.b.gerr;
            a.census = c.b.gerr + 64;
            a.temperature = r.temperature; a.top_k = r.top_k; a.top_p = r.top_p;
            a.step0 = r.step0; a.n_forced = r.n_forced; a.score = r.score;
            // (a streamed call on the plain kernels always draws ahead: their in-loop draw,
            //  kept as it was, knows no step origin; nor does any build's know per-row origins)
            if (c.b.lq && (c.sw.noise_ahead || (r.step0 != 0 && !c.pl->ctrl) ||
                           r.row_origins())) {
                // drawn ahead by a tick's input launch, else by a launch here
                if (off < c.noise_beg || off + a.nsteps > c.noise_end) {
                    if (r.row_origins())
                        RET(gen_noise_origin_launch(r.noise, r.seed, r.row0, c.b.base, off,
                                                    a.nsteps, c.L, r.n_seqs, c.b.lq, r.step0,
                                                    r.noise_row, r.row_step0, c.s));
                    else
                        RET(gen_noise_launch(r.noise, r.seed, r.row0, c.b.base, off, a.nsteps,
                                             c.L, r.n_seqs, c.b.lq, r.step0, c.s));
                    c.noise_beg = off;
                    c.noise_end = off + a.nsteps;
                }
                a.lq = c.b.lq + (size_t)(off - c.noise_beg) * r.n_seqs * m->q_levels;
            }
            // the next bottom tick's gate update rides at the end of this launch unless an
            // upper tick (new G) comes first
            const int nx = off + m->tier[0].frame_size;
            if (c.b.fold && nx < periods * c.L && nx % m->tier[1].n_frame_samples != 0 &&
                c.sw.fuse_gates) {
                const int fi = (nx / m->tier[0].n_frame_samples) % m->tier[1].frame_size;
                a.tk = c.b.ticks + 2 * fi + (ticks[0] & 1);    // that tick's G row, cur / nxt
                c.gate_done = true;
            }
            if (c.pending.N) {        // this bottom tick's GEMM, in the launch
                a.tg = c.pending;
                c.pending = GenMlpArgs::TickGemm{};
            }
            RET(gen_mlp_launch(c.pl, a, r.row_origins(), c.s));
        }
    }
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, c.s, c.b.base, periods * c.L);
    SRNN_LAUNCH_CHECK();
    return 0;
}

// persistent sample loop plan for this model/batch (ok = 0: per-sample kernels)
void plan_for(const SrnnModel* m, int n_seqs, int level, GenMlpPlan* pl, const GenSwitches& sw) {
    if (!gen_mlp_plan(m->dtype, n_seqs, m->dim, m->tier[0].frame_size, m->q_levels, level, pl) ||
        !sw.persist)
        pl->ok = 0;
}

// words of a state record (even: the int64 step count stays 8-byte aligned in every row)
int64_t gen_state_row_words(const SrnnModel* m, const GenSwitches& sw) {
    const int64_t L = m->tier[m->n_tiers - 1].n_frame_samples;
    const int64_t w = GS_HDR + L + (int64_t)m->n_tiers * m->n_rnn * m->dim +
                      (fold_ok(m, sw) ? 6 * (int64_t)m->dim : 0);
    return (w + 1) & ~(int64_t)1;
}

// ---- the phases of a call (gen_run) ------------------------------------------------------
// gen_validate and gen_prepare depend on (model, n_seqs, control level, switches) and the
// workspace only -- what a session (below) keeps between its chunks; gen_start, gen_blocks
// and gen_finish are this call's.

// The rows' own Philox origins, read back (the only HIP call of the validation, and it queues
// nothing): a row below 0 or a step counter that would wrap within the call is refused.
int gen_validate_rows(Ctx& c) {
    const GenRequest& r = c.rq;
    if (!r.row_origins() || r.noise) return 0;   // (replayed noise: the arrays move no counter)
    const size_t B = (size_t)r.n_seqs;
    std::vector<uint32_t> v(B);
    auto read = [&](const void* src, const char* what) -> int {
        if (hipStreamSynchronize(r.stream) != hipSuccess ||
            hipMemcpy(v.data(), src, B * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            srnn_set_error("generate: reading %s: %s", what, hipGetErrorString(hipGetLastError()));
            return 2;
        }
        return 0;
    };
    if (r.noise_row) {
        RET(read(r.noise_row, "noise_row"));
        for (size_t b = 0; b < B; ++b)
            SRNN_REQUIRE((int32_t)v[b] >= 0, "generate: noise_row[%zu] = %d is negative", b,
                         (int32_t)v[b]);
    }
    if (r.row_step0) {
        RET(read(r.row_step0, "the rows' step0"));
        for (size_t b = 0; b < B; ++b)
            SRNN_REQUIRE((uint64_t)v[b] + (uint64_t)c.T <= 0xFFFFFFFFull,
                         "generate: row %zu: step0 %u + %lld steps overflow the 32-bit Philox step "
                         "counter", b, v[b], (long long)c.T);
    }
    return 0;
}

// Checks the request and lays the call out (plan, workspace, state record): host work only.
int gen_layout(Ctx& c) {
    const GenRequest& r = c.rq;
    const SrnnModel* m = r.m;
    SRNN_REQUIRE(r.row0 >= 0, "generate: negative row offset");
    SRNN_REQUIRE(m && r.n_seqs > 0 && r.n_cond > 0 && (r.seq || c.fresh) && r.workspace,
                 "generate: bad args");
    SRNN_REQUIRE(m->n_tiers >= 1 && m->n_tiers <= SRNN_MAX_TIERS, "generate: n_tiers");
    SRNN_REQUIRE(m->n_rnn >= 1 && m->n_rnn <= SRNN_MAX_RNN, "generate: n_rnn");
    SRNN_REQUIRE(m->q_levels == 256, "generate: q_levels must be 256");
    SRNN_REQUIRE(m->dim % 16 == 0, "generate: dim must be a multiple of 16");
    plan_for(m, r.n_seqs, r.level(), &c.plan, c.sw);
    if (r.flags & 2) c.plan.ok = 0;          // caller asked for the per-sample kernel path
    const size_t need = carve(m, r.n_seqs, (char*)r.workspace, &c.b, &c.plan, c.sw);
    SRNN_REQUIRE(r.workspace_bytes >= need, "generate: workspace %zu < %zu", r.workspace_bytes,
                 need);
    c.L = m->tier[m->n_tiers - 1].n_frame_samples;
    c.T = c.fresh ? 0 : (int64_t)r.n_cond * c.L;
    c.ldseq = (int64_t)c.L * (r.n_cond + 1);
    SRNN_REQUIRE((uint64_t)r.step0 + (uint64_t)c.T <= 0xFFFFFFFFull,
                 "generate: step0 %u + %lld steps overflow the 32-bit Philox step counter",
                 r.step0, (long long)c.T);
    SRNN_REQUIRE(!r.n_forced || c.T < (1 << 23), "generate: a forced prefix needs fewer than 2^23 "
                 "steps per call (%lld)", (long long)c.T);
    c.rw = gen_state_row_words(m, c.sw);
    const size_t sb = (size_t)c.rw * 4 * (size_t)r.n_seqs;
    SRNN_REQUIRE((!r.state_in && !r.state_out) || r.state_bytes == sb,
                 "generate: state of %zu bytes, this model / batch / fold layout needs %zu",
                 r.state_bytes, sb);
    SRNN_REQUIRE((((uintptr_t)r.state_in | (uintptr_t)r.state_out) & 7) == 0,
                 "generate: state buffers must be 8-byte aligned");
    c.pl = c.plan.ok ? &c.plan : nullptr;
    c.tick_gemm = c.pl && c.b.fold &&
                  gen_mlp_tick_gemm_ok(c.pl, (m->tier[0].frame_size + 3) * m->dim, m->dim,
                                       r.n_seqs);
    GenStateMap& mp = c.mp;
    mp.L = c.L;
    mp.D = m->dim;
    mp.n_h = m->n_tiers * m->n_rnn;
    mp.fold = c.b.fold ? 1 : 0;
    if (c.b.fold) {
        mp.gh0 = c.b.up[0] + (size_t)m->tier[0].frame_size * m->dim;
        mp.ldgh0 = c.b.ldup0;
        mp.gh1 = c.b.fg + (size_t)m->tier[1].frame_size * 3 * m->dim;
        mp.ldgh1 = c.b.ldg1;
    }
    const uint32_t hdr[8] = {GS_TAG, (uint32_t)m->dtype, (uint32_t)m->n_tiers, (uint32_t)m->n_rnn,
                             (uint32_t)m->dim, (uint32_t)c.L,
                             (c.b.fold ? 1u : 0u) | (c.b.fold_top ? 2u : 0u), 0u};
    memcpy(mp.hdr, hdr, sizeof(hdr));
    mp.q_zero = (uint32_t)(m->q_levels / 2);
    return 0;
}

// No HIP work is queued before the last check has passed.
int gen_validate(Ctx& c) {
    RET(gen_layout(c));
    return gen_validate_rows(c);
}

// What the model, the batch size and the plan determine: the 2 x LUT, the persistent loop's
// weight images, the folded ticks' concatenated and pre-multiplied weights, the tick table.
int gen_prepare(Ctx& c) {
    const SrnnModel* m = c.rq.m;
    const int D = m->dim, dt = m->dtype;
    const size_t es = dt == SRNN_F32 ? 4 : 2;
    hipStream_t s = c.s;
    // 2 * udequantize LUT (bit-exact reference table for mu-law q = 256)
    float lut2[256];
    for (int q = 0; q < 256; ++q) {
        float v;
        memcpy(&v, &SRNN_ULAW_LUT_BITS[q], 4);
        lut2[q] = 2.0f * v;
    }
    SRNN_CHECK_HIP(hipMemcpyAsync(c.b.lut2, lut2, sizeof(lut2), hipMemcpyHostToDevice, s));
    if (c.pl)
        RET(gen_mlp_prep_weights(c.pl, m->w_hid, m->w_out, D, m->q_levels, c.b.wfr_hid,
                                 c.b.wfr_out, s));
    std::vector<GenMlpArgs::Tick> tt;
    if (c.b.fold) {
        // folded bottom tick operands (see fold_gru_kernel): [W_up; W_hh], [b_up; b_hh]
        const SrnnTier& t0 = m->tier[0];
        const SrnnTier& t1 = m->tier[1];
        const size_t upw = (size_t)t0.frame_size * D;
        // b_hh (3D floats) to dst, zeros where the layer has none
        auto copy_bhh = [&](float* dst, const float* b_hh) {
            return b_hh ? hipMemcpyAsync(dst, b_hh, (size_t)3 * D * 4, hipMemcpyDeviceToDevice, s)
                        : hipMemsetAsync(dst, 0, (size_t)3 * D * 4, s);
        };
        SRNN_CHECK_HIP(hipMemcpyAsync(c.b.wcat, t0.w_up, upw * D * es, hipMemcpyDeviceToDevice, s));
        SRNN_CHECK_HIP(hipMemcpyAsync((char*)c.b.wcat + upw * D * es, t0.w_hh[0],
                                      (size_t)3 * D * D * es, hipMemcpyDeviceToDevice, s));
        SRNN_CHECK_HIP(hipMemcpyAsync(c.b.bcat, t0.b_up, upw * 4, hipMemcpyDeviceToDevice, s));
        SRNN_CHECK_HIP(copy_bhh(c.b.bcat + upw, t0.b_hh[0]));
        RET(gen_typed_launch(dt, [&](auto z) {
            using T = decltype(z);
            hipLaunchKernelGGL((fold_input_kernel<T>), dim3(cdiv(3 * D, 4)), dim3(256), 0, s,
                               (const T*)t0.w_ih[0], (const T*)t0.w_in, t0.n_frame_samples,
                               t0.b_in, t0.b_ih[0], t1.b_up, t1.frame_size, c.b.fmin, c.b.bfold,
                               3 * D, D);
        }));
        // Wfold[j] = W_ih0 (3D x D) . W_up1[j] (D x D, rows j D .. j D + D - 1), bf16 out
        {
            GemmProblem p;
            p.dtype = p.out_dtype = dt;
            p.M = 3 * D; p.N = D; p.K = D; p.batch = t1.frame_size;
            p.A = t0.w_ih[0]; p.lda = D;
            p.B = t1.w_up; p.ldb = D; p.sB = (int64_t)D * D;
            p.C = c.b.wfold; p.ldc = D; p.sC = (int64_t)3 * D * D;
            RET(srnn_gemm_run(p, s));
        }
        // [W_hh1; b_hh1] after the folded rows
        const size_t g0 = (size_t)t1.frame_size * 3 * D;
        SRNN_CHECK_HIP(hipMemcpyAsync((char*)c.b.wfold + g0 * D * es, t1.w_hh[0],
                                      (size_t)3 * D * D * es, hipMemcpyDeviceToDevice, s));
        SRNN_CHECK_HIP(copy_bhh(c.b.bfold + g0, t1.b_hh[0]));
        if (c.b.fold_top) {
            // Min1 = W_ih1 (3D x D) . W_in1 (D x in_dim), zero-padded to TA_AP columns
            SRNN_CHECK_HIP(hipMemsetAsync(c.b.min1, 0, (size_t)3 * D * TA_AP * es, s));
            GemmProblem p;
            p.dtype = p.out_dtype = dt;
            p.M = 3 * D; p.N = t1.in_dim; p.K = D;
            p.A = t1.w_ih[0]; p.lda = D;
            p.B = t1.w_in; p.ldb = t1.in_dim;
            p.C = c.b.min1; p.ldc = TA_AP;
            RET(srnn_gemm_run(p, s));
        }
        // gate-update operand table of the persistent loop, [fi][cur]
        tt.resize(2 * t1.frame_size);
        for (int fi = 0; fi < t1.frame_size; ++fi)
            for (int pc = 0; pc < 2; ++pc) {
                GenMlpArgs::Tick& e = tt[2 * fi + pc];
                e.fmin = c.b.fmin;
                e.G = c.b.fg + (size_t)fi * 3 * D;
                e.ldg = c.b.ldg1;
                e.gh = c.b.up[0] + upw;
                e.ldgh = c.b.ldup0;
                e.hp = c.b.h[0][0][pc];
                e.hn = c.b.h[0][0][pc ^ 1];
                e.hn_lp = c.b.hlp[0][0][pc ^ 1];
                e.lut2 = c.b.lut2;
            }
        SRNN_CHECK_HIP(hipMemcpyAsync(c.b.ticks, tt.data(), tt.size() * sizeof(tt[0]),
                                      hipMemcpyHostToDevice, s));
    }
    SRNN_CHECK_HIP(hipStreamSynchronize(s));     // the host staging arrays go out of scope
    return 0;
}

// The recurrent state of rows that have done no step, in buffer [0]: h0 of every tier and layer
// and, with folded ticks, the gh rows of their first tick.  A call's fresh start, and all of a
// fresh record (srnn_gen_state_fresh) but its q_zero history.
int gen_init_state(Ctx& c) {
    const SrnnModel* m = c.rq.m;
    const int D = m->dim, B = c.rq.n_seqs, dt = m->dtype;
    const bool lp = dt != SRNN_F32;
    hipStream_t s = c.s;
    // initial hidden states: h0 expanded over rows (model.py:224-228)
    for (int k = 0; k < m->n_tiers; ++k)
        for (int l = 0; l < m->n_rnn; ++l)
            RET(gen_typed_launch(dt, [&](auto z) {
                using T = decltype(z);
                hipLaunchKernelGGL((init_state_kernel<T>), dim3(cdiv(B * D, 256)), dim3(256), 0, s,
                                   m->tier[k].h0 + (size_t)l * D, c.b.h[k][l][0],
                                   lp ? (T*)c.b.hlp[k][l][0] : nullptr, B, D);
            }));
    if (c.b.fold) {
        const SrnnTier& t0 = m->tier[0];
        const SrnnTier& t1 = m->tier[1];
        RET(linear_fwd(dt, SRNN_F32, B, 3 * D, D, c.b.hlp[1][0][0], D, t1.w_hh[0], D, t1.b_hh[0],
                       c.mp.gh1, c.b.ldg1, 0, s));
        RET(linear_fwd(dt, SRNN_F32, B, 3 * D, D, c.b.hlp[0][0][0], D, t0.w_hh[0], D, t0.b_hh[0],
                       c.mp.gh0, c.b.ldup0, 0, s));
    }
    return 0;
}

// The headers (8 words each, read from the device onto stream s) of n records of row stride
// c.rw words must be of this call's layout: checked on the host before anything that uses the
// records is launched.
int gen_check_headers(Ctx& c, const void* records, int n, hipStream_t s) {
    std::vector<uint32_t> hd((size_t)n * 8);
    if (hipMemcpy2DAsync(hd.data(), 32, records, (size_t)c.rw * 4, 32, n, hipMemcpyDeviceToHost,
                         s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        srnn_set_error("generate: reading the state headers: %s",
                       hipGetErrorString(hipGetLastError()));
        return 2;
    }
    const uint32_t* w = c.mp.hdr;
    for (int b = 0; b < n; ++b) {
        const uint32_t* h = hd.data() + (size_t)b * 8;
        SRNN_REQUIRE(memcmp(h, w, 32) == 0,
                     "generate: state row %d has layout (tag %08x, dtype %u, tiers %u, rnn %u, "
                     "dim %u, L %u, fold %u), this call needs (tag %08x, dtype %u, tiers %u, "
                     "rnn %u, dim %u, L %u, fold %u)", b, h[0], h[1], h[2], h[3], h[4], h[5],
                     h[6], w[0], w[1], w[2], w[3], w[4], w[5], w[6]);
    }
    return 0;
}

// The block base (sample L) and the zeroed hand-off block of a call.
int gen_reset(Ctx& c) {
    hipStream_t s = c.s;
    SRNN_CHECK_HIP(hipMemsetAsync(c.b.base, 0, 64, s));
    if (c.pl) SRNN_CHECK_HIP(hipMemsetAsync(c.b.gerr, 0, c.b.gm_bytes, s));
    // (from c.L: the context outlives the drain)
    SRNN_CHECK_HIP(hipMemcpyAsync(c.b.base, &c.L, sizeof(int), hipMemcpyHostToDevice, s));
    return 0;
}

// With the folded top tick P1 = bf16(row_bias) . W_ih1^T + b_ih1 (else nothing: the top tier's
// input launch adds row_bias itself).
int gen_top_bias(Ctx& c) {
    if (!c.b.fold_top) return 0;
    const GenRequest& r = c.rq;
    const SrnnModel* m = r.m;
    const int D = m->dim, B = r.n_seqs, dt = m->dtype;
    const SrnnTier& t1 = m->tier[1];
    RET(gen_typed_launch(dt, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL((copy_cast_kernel<T>), dim3(cdiv(B * D, 256)), dim3(256), 0, c.s,
                           r.row_bias, (T*)c.b.x[1], B * D);
    }));
    return linear_fwd(dt, SRNN_F32, B, 3 * D, D, c.b.x[1], D, t1.w_ih[0], D, t1.b_ih[0], c.b.p1,
                      3 * D, 0, c.s);
}

// The carried state `records` into the workspace: buffer [0] of every h (and its T copy), the
// folded ticks' gh rows and the sample history seq[:, 0:L).
int gen_unpack(Ctx& c, const void* records) {
    const GenRequest& r = c.rq;
    const SrnnModel* m = r.m;
    const bool lp = m->dtype != SRNN_F32;
    GenStateMap mp = c.mp;
    for (int k = 0; k < m->n_tiers; ++k)
        for (int l = 0; l < m->n_rnn; ++l) {
            mp.h[k * m->n_rnn + l] = c.b.h[k][l][0];
            mp.hlp[k * m->n_rnn + l] = lp ? c.b.hlp[k][l][0] : nullptr;
        }
    return gen_typed_launch(m->dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL((gen_state_unpack_kernel<T>), dim3(cdiv(c.rw, 256), r.n_seqs),
                           dim3(256), 0, c.s, (const uint32_t*)records, c.rw, mp, r.seq, c.ldseq);
    });
}

// This call's start: the block base and the hand-off block, the fresh (or carried) recurrent
// state, and what follows from it and from row_bias.
int gen_start(Ctx& c) {
    const GenRequest& r = c.rq;
    // every record's header must be one of this call's layout: checked on the host before
    // anything of this call's own is launched
    if (r.state_in) RET(gen_check_headers(c, r.state_in, r.n_seqs, c.s));
    RET(gen_reset(c));
    RET(gen_init_state(c));
    RET(gen_top_bias(c));
    // the carried state replaces the fresh start's
    if (r.state_in) RET(gen_unpack(c, r.state_in));
    return 0;
}

// One block of `periods` periods captured from the call's stream and instantiated (an earlier
// block has run eagerly: it raised the per-kernel attributes, outside any capture).
int gen_capture(Ctx& c, int periods, hipGraph_t* graph, hipGraphExec_t* exec) {
    if (hipStreamBeginCapture(c.s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        srnn_set_error("generate: begin capture failed");
        return 2;
    }
    // (the capture is ended after a failed block too: the stream must leave capture mode)
    const int rc = run_block(c, periods);
    const hipError_t ce = hipStreamEndCapture(c.s, graph);
    RET(rc);
    if (ce != hipSuccess || hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0) != hipSuccess) {
        srnn_set_error("generate: graph capture/instantiate failed");
        return 2;
    }
    return 0;
}

// The blocks of two top-tier periods -- the first eagerly, the rest as replays of one captured
// block when asked for (flags & 1) -- and the odd period at the end.
int gen_blocks(Ctx& c) {
    const int nblocks = c.rq.n_cond / 2;
    int done = 0;
    if (nblocks > 0) {
        // first block eagerly: it raises the per-kernel attributes, outside any capture
        RET(run_block(c, 2));
        done = 1;
    }
    if ((c.rq.flags & 1) && nblocks > 1) {
        RET(gen_capture(c, 2, &c.gs.graph, &c.gs.exec));
        for (; done < nblocks; ++done)
            if (hipGraphLaunch(c.gs.exec, c.s) != hipSuccess) {
                srnn_set_error("generate: graph launch failed");
                return 2;
            }
    }
    for (; done < nblocks; ++done) RET(run_block(c, 2));
    if (c.rq.n_cond % 2) RET(run_block(c, 1));
    return 0;
}

// The records `out` of the state after T more steps than `in` counts (null: a fresh start), the
// rows' last L samples being seq columns [hist, hist + L).  `odd`: the steps ended in a
// one-period block.
int gen_pack(Ctx& c, void* out, const void* in, bool odd, const int64_t* seq, int64_t hist,
             int64_t T) {
    const SrnnModel* m = c.rq.m;
    // tick parity restarts at 0 in every block and the two-period blocks tick every tier
    // an even number of times, so only a trailing one-period block moves a tier's live h:
    // to buffer [1] where the tier ticks an odd number of times per period (the top tier
    // always does)
    GenStateMap mp = c.mp;
    for (int k = 0; k < m->n_tiers; ++k) {
        const int live = odd ? (c.L / m->tier[k].n_frame_samples) & 1 : 0;
        for (int l = 0; l < m->n_rnn; ++l) mp.h[k * m->n_rnn + l] = c.b.h[k][l][live];
    }
    hipLaunchKernelGGL(gen_state_pack_kernel, dim3(cdiv(c.rw, 256), c.rq.n_seqs), dim3(256), 0,
                       c.s, (uint32_t*)out, (const uint32_t*)in, c.rw, mp, seq, c.ldseq, hist, T);
    if (hipGetLastError() != hipSuccess) {
        srnn_set_error("generate: state pack launch");
        return 2;
    }
    return 0;
}

// Runs whatever the earlier phases returned (rc): packs the end state of a call that got
// through, drains the private stream before its resources go (generation is one long call),
// and reads the persistent loop's error word.
int gen_finish(Ctx& c, int rc) {
    const GenRequest& r = c.rq;
    if (!rc && r.state_out)
        rc = gen_pack(c, r.state_out, r.state_in, !c.fresh && r.n_cond % 2,
                      c.fresh ? nullptr : r.seq, c.ldseq - c.L, c.T);
    if (hipStreamSynchronize(c.s) != hipSuccess && !rc) {
        srnn_set_error("generate: %s", hipGetErrorString(hipGetLastError()));
        rc = 2;
    }
    if (!rc && c.pl && !c.fresh) {
        int e = 0;
        if (hipMemcpy(&e, c.b.gerr, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || e) {
            srnn_set_error(e == 2 ? "generate: persistent sample loop's workgroups were not all "
                                    "resident within 30 s (another process holds the CUs?)"
                                  : "generate: persistent sample loop lost a hand-off (spin limit)");
            rc = 2;
        }
    }
    return rc;
}

int gen_run(const GenRequest& rq) {
    Ctx c{rq, GenSwitches::read()};
    RET(gen_validate(c));
    RET(c.gs.open(rq.stream));
    c.s = c.gs.s;
    int rc = gen_prepare(c);
    if (!rc) rc = gen_start(c);
    if (!rc) rc = gen_blocks(c);
    return gen_finish(c, rc);
}

// srnn_gen_state_fresh: a call's phases up to its fresh start, then its end: the pack of T = 0
// steps, from no sample history
int gen_fresh(const GenRequest& rq) {
    Ctx c{rq, GenSwitches::read(), true};
    SRNN_REQUIRE(rq.state_out, "gen_state_fresh: bad args");
    RET(gen_validate(c));
    RET(c.gs.open(rq.stream));
    c.s = c.gs.s;
    int rc = gen_prepare(c);
    if (!rc) rc = gen_init_state(c);
    return gen_finish(c, rc);
}

// ---- sessions (srnn_gen_session_*) ---------------------------------------------------------
// A session is a Ctx that lives on: gen_layout and gen_prepare run once, at open, over a request
// whose every pointer names a session-owned buffer at a fixed address (the captured launches bake
// them in), and a chunk is the per-call phases -- gen_reset, gen_unpack, the blocks, gen_pack --
// from and to the session's own records.  The rows' Philox origins are device arrays
// (SrnnGenRows' path), so a captured block serves every chunk.

// the session's own arrays, carved from the arena ahead of the call workspace
struct SessBufs {
    int64_t* seq;            // (B, L (F + 1))
    float* cond;             // (B, F, C)
    float* row_bias;         // (B, D)
    float* temperature;      // (B) each; level >= 1
    int* top_k;
    int* n_forced;
    float* top_p;            // level >= 2
    int* noise_row;
    uint32_t* step0;
    float* logp;             // (F L, B, Q), SRNN_GEN_SESSION_LOGP
    float* score;            // (F L, B, 2), SRNN_GEN_SESSION_SCORE
    float* noise;            // (F L, B, Q), SRNN_GEN_SESSION_NOISE
    uint32_t* records;       // (B, rw)
    int* sticky;             // the first error word a chunk's persistent loop raised
    char* ws;                // the call workspace (carve)
    size_t ws_bytes;
};

// What (model, n_seqs, level, flags) determine of a session's layout, checked first: the arena's
// size and, given the arena, its carving.
int session_carve(const SrnnModel* m, int B, int F, int level, int flags, const GenSwitches& sw,
                  char* arena, SessBufs* sb, size_t* bytes) {
    SRNN_REQUIRE(m && B > 0 && F > 0 && level >= 0 && level <= 3 && !(flags & ~31),
                 "gen_session: bad args");
    // (level 3 is the scored level: the flag and the level go together)
    SRNN_REQUIRE((level == 3) == !!(flags & SRNN_GEN_SESSION_SCORE),
                 "gen_session: level 3 and SRNN_GEN_SESSION_SCORE go together");
    SRNN_REQUIRE(m->n_tiers >= 1 && m->n_tiers <= SRNN_MAX_TIERS, "generate: n_tiers");
    SRNN_REQUIRE(m->n_rnn >= 1 && m->n_rnn <= SRNN_MAX_RNN, "generate: n_rnn");
    SRNN_REQUIRE(m->q_levels == 256, "generate: q_levels must be 256");
    SRNN_REQUIRE(m->dim > 0 && m->dim % 16 == 0, "generate: dim must be a multiple of 16");
    const int64_t L = m->tier[m->n_tiers - 1].n_frame_samples;
    SRNN_REQUIRE(L > 0 && m->cond_dim >= 0 && (int64_t)F * L < (1ll << 31) - L,
                 "gen_session: max_frames %d x lookback %lld", F, (long long)L);
    GenMlpPlan pl;
    plan_for(m, B, level, &pl, sw);
    if (flags & SRNN_GEN_SESSION_PER_SAMPLE) pl.ok = 0;
    Bufs b;
    const size_t Bz = (size_t)B, steps = (size_t)F * L;
    size_t off = 0;
    auto take = [&](size_t n) -> char* {
        char* p = arena ? arena + off : nullptr;
        off += al(n);
        return p;
    };
    sb->seq = (int64_t*)take(Bz * (steps + L) * 8);
    sb->cond = (float*)take(Bz * F * (m->cond_dim > 0 ? m->cond_dim : 1) * 4);
    sb->row_bias = (float*)take(Bz * m->dim * 4);
    sb->temperature = level >= 1 ? (float*)take(Bz * 4) : nullptr;
    sb->top_k = level >= 1 ? (int*)take(Bz * 4) : nullptr;
    sb->n_forced = level >= 1 ? (int*)take(Bz * 4) : nullptr;
    sb->top_p = level >= 2 ? (float*)take(Bz * 4) : nullptr;
    sb->noise_row = (int*)take(Bz * 4);
    sb->step0 = (uint32_t*)take(Bz * 4);
    sb->logp = (flags & SRNN_GEN_SESSION_LOGP) ? (float*)take(steps * Bz * 256 * 4) : nullptr;
    sb->noise = (flags & SRNN_GEN_SESSION_NOISE) ? (float*)take(steps * Bz * 256 * 4) : nullptr;
    // (after every older array: a session without the flag is carved as it always was)
    sb->score = (flags & SRNN_GEN_SESSION_SCORE) ? (float*)take(steps * Bz * 8) : nullptr;
    sb->records = (uint32_t*)take((size_t)gen_state_row_words(m, sw) * 4 * Bz);
    sb->sticky = (int*)take(64);
    sb->ws_bytes = carve(m, B, nullptr, &b, &pl, sw);
    sb->ws = take(sb->ws_bytes);
    *bytes = off;
    return 0;
}

struct Session {
    SrnnModel model;         // the caller's, copied: rq.m
    GenRequest rq;           // over the session's own buffers; n_cond = max_frames (the strides)
    Ctx c;
    SessBufs sb{};
    const int max_frames, level, flags;
    hipGraph_t graph[2] = {nullptr, nullptr};      // [periods - 1]: the one- and the two-period
    hipGraphExec_t exec[2] = {nullptr, nullptr};   // block
    bool eager_done[2] = {false, false};
    volatile int* host_err = nullptr;              // pinned: the sticky error word, per chunk;
                                                   // from word 16 on, a staging row of B ints
    std::vector<int64_t> steps;                    // host mirror of the rows' step counts
    bool have_bias = false, forced_live = false, poisoned = false;
    bool staged = false;                           // the pinned noise_row row is in flight
    char error[512] = {0};                         // the text of the error that poisoned it
    SrnnGenSessionStats st{};
    Session(const SrnnModel& m, int n_seqs, int F, int lv, uint64_t seed, int row0, int fl,
            hipStream_t user)
        : model(m),
          rq{&model, n_seqs, F, nullptr, nullptr, nullptr, seed, row0, nullptr, nullptr, nullptr,
             0, fl & 3, user},
          c{rq, GenSwitches::read()}, max_frames(F), level(lv), flags(fl),
          steps((size_t)n_seqs, 0) {}
    // (a session never keeps starting work on a device after a fault)
    int poison() {
        if (!poisoned) snprintf(error, sizeof(error), "%s", srnn_last_error());
        poisoned = true;
        srnn_set_error("%s", error);
        return 2;
    }
    int poison_err_word() {
        const int e = *host_err;
        srnn_set_error(e == 2 ? "generate: persistent sample loop's workgroups were not all "
                                "resident within 30 s (another process holds the CUs?)"
                              : "generate: persistent sample loop lost a hand-off (spin limit)");
        return poison();
    }
    int refused() {
        srnn_set_error("%s", error);
        return 2;
    }
};

int session_open(Session& se, char* arena, size_t arena_bytes) {
    Ctx& c = se.c;
    GenRequest& r = se.rq;
    const SrnnModel* m = &se.model;
    const size_t B = (size_t)r.n_seqs;
    size_t need = 0;
    RET(session_carve(m, r.n_seqs, se.max_frames, se.level, se.flags, c.sw, arena, &se.sb, &need));
    SRNN_REQUIRE(arena_bytes >= need, "gen_session: arena %zu < %zu", arena_bytes, need);
    const SessBufs& sb = se.sb;
    r.cond = sb.cond;
    r.row_bias = sb.row_bias;
    r.noise = sb.noise;
    r.seq = sb.seq;
    r.logp = sb.logp;
    r.score = sb.score;
    r.workspace = sb.ws;
    r.workspace_bytes = sb.ws_bytes;
    r.temperature = sb.temperature;
    r.top_k = sb.top_k;
    r.top_p = sb.top_p;
    r.n_forced = sb.n_forced;
    r.noise_row = sb.noise_row;
    r.row_step0 = sb.step0;
    RET(gen_layout(c));
    SRNN_REQUIRE(r.level() == se.level, "gen_session: level");
    RET(c.gs.open(r.stream));
    c.s = c.gs.s;
    hipStream_t s = c.s;
    SRNN_CHECK_HIP(hipHostMalloc((void**)&se.host_err, 64 + B * 4, hipHostMallocDefault));
    *se.host_err = 0;
    // the buffers a chunk may leave as they are: controls at their defaults, Philox rows
    // row0 + b, nothing forced, a defined history
    std::vector<float> ones(B, 1.0f);
    std::vector<int> nrow(B);
    for (size_t b = 0; b < B; ++b) nrow[b] = r.row0 + (int)b;
    SRNN_CHECK_HIP(hipMemsetAsync(arena, 0, (size_t)(sb.ws - arena), s));
    for (float* p : {sb.temperature, sb.top_p})
        if (p) SRNN_CHECK_HIP(hipMemcpyAsync(p, ones.data(), B * 4, hipMemcpyHostToDevice, s));
    SRNN_CHECK_HIP(hipMemcpyAsync(sb.noise_row, nrow.data(), B * 4, hipMemcpyHostToDevice, s));
    RET(gen_prepare(c));                         // (synchronises: the staging vectors may go)
    se.st.prepares++;
    // every row starts from a fresh record (gen_fresh's)
    RET(gen_init_state(c));
    RET(gen_pack(c, sb.records, nullptr, false, nullptr, 0, 0));
    SRNN_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

// Everything a chunk is refused for, before anything is queued.
int session_check(const Session& se, const SrnnGenChunk& ck, const float* score_out) {
    const GenRequest& r = se.rq;
    SRNN_REQUIRE(ck.n_frames >= 1 && ck.n_frames <= se.max_frames,
                 "gen_session: a chunk of %d frames, the session was opened for 1..%d",
                 ck.n_frames, se.max_frames);
    const int64_t T = (int64_t)ck.n_frames * se.c.L;
    SRNN_REQUIRE(ck.cond, "gen_session: no cond");
    SRNN_REQUIRE(ck.row_bias || se.have_bias, "gen_session: the first chunk must give row_bias");
    SRNN_REQUIRE(sample_ctrl_level(ck.temperature, ck.top_k, ck.top_p) <= se.level,
                 "gen_session: a sampling control above the session's level %d", se.level);
    SRNN_REQUIRE(!ck.prefix == !ck.n_forced, "gen_session: prefix and n_forced go together");
    if (ck.prefix) {
        SRNN_REQUIRE(se.level >= 1, "gen_session: a forced prefix needs a session of level >= 1");
        SRNN_REQUIRE(ck.prefix_cols >= 1 && ck.prefix_cols <= T,
                     "gen_session: prefix of %d columns for %lld steps", ck.prefix_cols,
                     (long long)T);
        SRNN_REQUIRE(T < (1 << 23), "generate: a forced prefix needs fewer than 2^23 "
                     "steps per call (%lld)", (long long)T);
    }
    SRNN_REQUIRE(!ck.noise == !(se.flags & SRNN_GEN_SESSION_NOISE),
                 "gen_session: replayed noise is given by exactly the chunks of a session opened "
                 "for it");
    SRNN_REQUIRE(!ck.logp_out || (se.flags & SRNN_GEN_SESSION_LOGP),
                 "gen_session: log-probs need a session opened for them");
    SRNN_REQUIRE(!score_out || (se.flags & SRNN_GEN_SESSION_SCORE),
                 "gen_session: scores need a session opened for them (SRNN_GEN_SESSION_SCORE)");
    if (ck.noise_row)
        for (int b = 0; b < r.n_seqs; ++b)
            SRNN_REQUIRE(ck.noise_row[b] >= 0, "generate: noise_row[%zu] = %d is negative",
                         (size_t)b, ck.noise_row[b]);
    if (!(se.flags & SRNN_GEN_SESSION_NOISE))
        for (int b = 0; b < r.n_seqs; ++b)
            SRNN_REQUIRE((uint64_t)se.steps[b] + (uint64_t)T <= 0xFFFFFFFFull,
                         "generate: row %zu: step0 %llu + %lld steps overflow the 32-bit Philox "
                         "step counter", (size_t)b, (unsigned long long)se.steps[b], (long long)T);
    return 0;
}

// One block: the first of its length eagerly (it raises kernel attributes), the second captured
// and launched, every later one -- of this chunk and of all that follow -- a replay.
int session_block(Session& se, int periods) {
    Ctx& c = se.c;
    const int k = periods - 1;
    if (!(se.flags & SRNN_GEN_SESSION_GRAPH) || !se.eager_done[k]) {
        RET(run_block(c, periods));
        se.eager_done[k] = true;
        se.st.eager_blocks++;
        return 0;
    }
    if (!se.exec[k]) {
        RET(gen_capture(c, periods, &se.graph[k], &se.exec[k]));
        se.st.graphs_captured++;
    }
    if (hipGraphLaunch(se.exec[k], c.s) != hipSuccess) {
        srnn_set_error("generate: graph launch failed");
        return 2;
    }
    se.st.graph_launches++;
    return 0;
}

// Queues a checked chunk; every step is ordered on the session's stream.
int session_queue(Session& se, const SrnnGenChunk& ck, float* score_out, hipStream_t user) {
    Ctx& c = se.c;
    const GenRequest& r = se.rq;
    const SessBufs& sb = se.sb;
    const SrnnModel* m = r.m;
    const size_t B = (size_t)r.n_seqs, n = (size_t)ck.n_frames, L = (size_t)c.L;
    const size_t T = n * L;
    hipStream_t s = c.s;
    const hipMemcpyKind d2d = hipMemcpyDeviceToDevice;
    SRNN_CHECK_HIP(hipEventRecord(c.gs.ev, user));
    SRNN_CHECK_HIP(hipStreamWaitEvent(s, c.gs.ev, 0));
    if (m->cond_dim > 0) {
        const size_t fb = (size_t)m->cond_dim * 4;
        SRNN_CHECK_HIP(hipMemcpy2DAsync(sb.cond, (size_t)se.max_frames * fb, ck.cond, n * fb,
                                        n * fb, B, d2d, s));
    }
    if (ck.row_bias) {
        SRNN_CHECK_HIP(hipMemcpyAsync(sb.row_bias, ck.row_bias, B * m->dim * 4, d2d, s));
        RET(gen_top_bias(c));
        se.have_bias = true;
    }
    if (ck.temperature)
        SRNN_CHECK_HIP(hipMemcpyAsync(sb.temperature, ck.temperature, B * 4, d2d, s));
    if (ck.top_k) SRNN_CHECK_HIP(hipMemcpyAsync(sb.top_k, ck.top_k, B * 4, d2d, s));
    if (ck.top_p) SRNN_CHECK_HIP(hipMemcpyAsync(sb.top_p, ck.top_p, B * 4, d2d, s));
    if (ck.prefix) {
        const size_t pb = (size_t)ck.prefix_cols * 8;
        SRNN_CHECK_HIP(hipMemcpy2DAsync(sb.seq + L, (size_t)c.ldseq * 8, ck.prefix, pb, pb, B,
                                        d2d, s));
        SRNN_CHECK_HIP(hipMemcpyAsync(sb.n_forced, ck.n_forced, B * 4, d2d, s));
        se.forced_live = true;
    } else if (se.forced_live) {
        SRNN_CHECK_HIP(hipMemsetAsync(sb.n_forced, 0, B * 4, s));
        se.forced_live = false;
    }
    if (ck.noise) SRNN_CHECK_HIP(hipMemcpyAsync(sb.noise, ck.noise, T * B * 256 * 4, d2d, s));
    if (ck.noise_row) {
        // through the pinned staging row (a copy from pageable memory may wait for the stream);
        // one still in flight is waited for, whatever else that costs
        if (se.staged) SRNN_CHECK_HIP(hipStreamSynchronize(s));
        int* stage = (int*)se.host_err + 16;
        memcpy(stage, ck.noise_row, B * 4);
        SRNN_CHECK_HIP(hipMemcpyAsync(sb.noise_row, stage, B * 4, hipMemcpyHostToDevice, s));
        se.staged = true;
    }
    // the per-chunk part of gen_start (gen_reset with the base set from the device side: no
    // host memory is read), from the session's own records
    SRNN_CHECK_HIP(hipMemsetAsync(c.b.base, 0, 64, s));
    if (c.pl) SRNN_CHECK_HIP(hipMemsetAsync(c.b.gerr, 0, c.b.gm_bytes, s));
    SRNN_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)c.b.base, c.L, 1, s));
    RET(gen_rows_step0_launch(sb.records, c.rw, 8, r.n_seqs, sb.step0, s));
    RET(gen_unpack(c, sb.records));
    for (size_t k = 0; k < n / 2; ++k) RET(session_block(se, 2));
    if (n % 2) RET(session_block(se, 1));
    RET(gen_pack(c, sb.records, sb.records, n % 2 != 0, sb.seq, (int64_t)T, (int64_t)T));
    if (ck.seq_out)
        SRNN_CHECK_HIP(hipMemcpy2DAsync(ck.seq_out, T * 8, sb.seq + L, (size_t)c.ldseq * 8, T * 8,
                                        B, hipMemcpyDefault, s));
    if (ck.logp_out)
        SRNN_CHECK_HIP(hipMemcpyAsync(ck.logp_out, sb.logp, T * B * 256 * 4, hipMemcpyDefault, s));
    if (score_out)
        SRNN_CHECK_HIP(hipMemcpyAsync(score_out, sb.score, T * B * 8, hipMemcpyDefault, s));
    RET(gen_rows_err_launch(c.pl ? c.b.gerr : nullptr, sb.sticky, s));
    SRNN_CHECK_HIP(hipMemcpyAsync((void*)se.host_err, sb.sticky, sizeof(int),
                                  hipMemcpyDeviceToHost, s));
    return 0;
}

int session_chunk(Session& se, const SrnnGenChunk& ck, float* score_out, hipStream_t user) {
    if (se.poisoned) return se.refused();
    if (*se.host_err) return se.poison_err_word();
    RET(session_check(se, ck, score_out));
    if (session_queue(se, ck, score_out, user)) return se.poison();
    const int64_t T = (int64_t)ck.n_frames * se.c.L;
    for (int64_t& v : se.steps) v += T;
    se.st.chunks++;
    return 0;
}

int session_sync(Session& se) {
    if (se.poisoned) return se.refused();
    if (hipStreamSynchronize(se.c.s) != hipSuccess) {
        srnn_set_error("generate: %s", hipGetErrorString(hipGetLastError()));
        return se.poison();
    }
    se.staged = false;
    if (*se.host_err) return se.poison_err_word();
    return 0;
}

int session_set_rows(Session& se, const int32_t* rows, int n, const void* records, size_t bytes,
                     hipStream_t user) {
    if (se.poisoned) return se.refused();
    Ctx& c = se.c;
    const int B = se.rq.n_seqs;
    const size_t rb = (size_t)c.rw * 4;
    SRNN_REQUIRE(rows && records && n >= 1 && n <= B, "gen_session: bad args");
    SRNN_REQUIRE(bytes == rb * (size_t)n && ((uintptr_t)records & 7) == 0,
                 "generate: state of %zu bytes, this model / batch / fold layout needs %zu", bytes,
                 rb * (size_t)n);
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n; ++i) {
        SRNN_REQUIRE(rows[i] >= 0 && rows[i] < B && !seen[rows[i]],
                     "gen_session: rows must be distinct values in [0, %d)", B);
        seen[rows[i]] = 1;
    }
    hipStream_t s = c.s;
    if (hipEventRecord(c.gs.ev, user) != hipSuccess ||
        hipStreamWaitEvent(s, c.gs.ev, 0) != hipSuccess) {
        srnn_set_error("gen_session: %s", hipGetErrorString(hipGetLastError()));
        return se.poison();
    }
    // headers first: nothing is written where one is not of the session's layout
    if (const int rc = gen_check_headers(c, records, n, s)) return rc == 1 ? 1 : se.poison();
    se.staged = false;
    std::vector<int64_t> cnt((size_t)n);
    bool ok = hipMemcpy2DAsync(cnt.data(), 8, (const char*)records + 32, rb, 8, n,
                               hipMemcpyDeviceToHost, s) == hipSuccess &&
              hipStreamSynchronize(s) == hipSuccess;
    if (ok)
        for (int i = 0; i < n; ++i)
            SRNN_REQUIRE(cnt[i] >= 0, "gen_session: record %d has a negative step count", i);
    for (int i = 0; ok && i < n; ++i)
        ok = hipMemcpyAsync((char*)se.sb.records + rb * rows[i], (const char*)records + rb * i, rb,
                            hipMemcpyDeviceToDevice, s) == hipSuccess;
    if (!ok || hipStreamSynchronize(s) != hipSuccess) {
        srnn_set_error("gen_session: replacing rows: %s", hipGetErrorString(hipGetLastError()));
        return se.poison();
    }
    for (int i = 0; i < n; ++i) se.steps[rows[i]] = cnt[i];
    return 0;
}

int session_close(Session* se) {
    if (!se) return 0;
    int rc = 0;
    // the stream is drained before anything is released, on every path
    if (se->c.s && hipStreamSynchronize(se->c.s) != hipSuccess) {
        srnn_set_error("gen_session: close: %s", hipGetErrorString(hipGetLastError()));
        rc = 2;
    }
    for (int k = 0; k < 2; ++k) {
        if (se->exec[k]) (void)hipGraphExecDestroy(se->exec[k]);
        if (se->graph[k]) (void)hipGraphDestroy(se->graph[k]);
    }
    if (se->host_err) (void)hipHostFree((void*)se->host_err);
    delete se;
    return rc;
}

// the opaque handle of the C ABI is a Session
inline Session* session_of(const SrnnGenSession* h) { return (Session*)h; }

}  // namespace

extern "C" int srnn_gen_session_bytes(const SrnnModel* m, int n_seqs, int max_frames, int level,
                                      int flags, size_t* bytes) {
    SRNN_REQUIRE(bytes, "gen_session: bad args");
    SessBufs sb;
    return session_carve(m, n_seqs, max_frames, level, flags, GenSwitches::read(), nullptr, &sb,
                         bytes);
}

extern "C" int srnn_gen_session_open(const SrnnModel* m, int n_seqs, int max_frames, int level,
                                     uint64_t seed, int row0, int flags, void* arena,
                                     size_t arena_bytes, void* stream, SrnnGenSession** out) {
    SRNN_REQUIRE(out, "gen_session: bad args");
    *out = nullptr;
    SRNN_REQUIRE(m && arena && ((uintptr_t)arena & (ALIGN - 1)) == 0 && row0 >= 0,
                 "gen_session: the arena must be 256-byte aligned, the row offset >= 0");
    size_t need = 0;
    SessBufs sb;
    RET(session_carve(m, n_seqs, max_frames, level, flags, GenSwitches::read(), nullptr, &sb,
                      &need));
    SRNN_REQUIRE(arena_bytes >= need, "gen_session: arena %zu < %zu", arena_bytes, need);
    Session* se = new Session(*m, n_seqs, max_frames, level, seed, row0, flags,
                              (hipStream_t)stream);
    const int rc = session_open(*se, (char*)arena, arena_bytes);
    if (rc) {
        // (the open's error text stays: the drain sets one only where it fails itself)
        session_close(se);
        return rc;
    }
    *out = (SrnnGenSession*)se;
    return 0;
}

extern "C" int srnn_gen_session_chunk(SrnnGenSession* s, const SrnnGenChunk* chunk,
                                      void* stream) {
    SRNN_REQUIRE(s && chunk, "gen_session: bad args");
    return session_chunk(*session_of(s), *chunk, nullptr, (hipStream_t)stream);
}

// srnn_gen_session_chunk that also writes the chunk's score pairs (n_frames L, n_seqs, 2) to
// score_out (device or pinned memory), as logp_out is written; score_out null: that entry
extern "C" int srnn_gen_session_chunk2(SrnnGenSession* s, const SrnnGenChunk* chunk,
                                       float* score_out, void* stream) {
    SRNN_REQUIRE(s && chunk, "gen_session: bad args");
    return session_chunk(*session_of(s), *chunk, score_out, (hipStream_t)stream);
}

extern "C" int srnn_gen_session_sync(SrnnGenSession* s) {
    SRNN_REQUIRE(s, "gen_session: bad args");
    return session_sync(*session_of(s));
}

extern "C" int srnn_gen_session_state_get(SrnnGenSession* s, void* records, size_t bytes) {
    SRNN_REQUIRE(s && records, "gen_session: bad args");
    Session& se = *session_of(s);
    if (se.poisoned) return se.refused();
    const size_t sb = (size_t)se.c.rw * 4 * (size_t)se.rq.n_seqs;
    SRNN_REQUIRE(bytes == sb,
                 "generate: state of %zu bytes, this model / batch / fold layout needs %zu", bytes,
                 sb);
    if (hipMemcpyAsync(records, se.sb.records, sb, hipMemcpyDefault, se.c.s) != hipSuccess) {
        srnn_set_error("gen_session: reading the records: %s",
                       hipGetErrorString(hipGetLastError()));
        return se.poison();
    }
    return session_sync(se);
}

extern "C" int srnn_gen_session_state_set_rows(SrnnGenSession* s, const int32_t* rows, int n,
                                               const void* records, size_t bytes, void* stream) {
    SRNN_REQUIRE(s, "gen_session: bad args");
    return session_set_rows(*session_of(s), rows, n, records, bytes, (hipStream_t)stream);
}

extern "C" int srnn_gen_session_stats(const SrnnGenSession* s, SrnnGenSessionStats* stats) {
    SRNN_REQUIRE(s && stats, "gen_session: bad args");
    const Session& se = *session_of(s);
    *stats = se.st;
    stats->steps_min = stats->steps_max = se.steps[0];
    for (const int64_t v : se.steps) {
        stats->steps_min = v < stats->steps_min ? v : stats->steps_min;
        stats->steps_max = v > stats->steps_max ? v : stats->steps_max;
    }
    return 0;
}

extern "C" int srnn_gen_session_close(SrnnGenSession* s) { return session_close(session_of(s)); }

// rows per group of the persistent sample loop at sampling-control level `level` (0: the plain
// plan; 1: temperature / top_k / a forced prefix, 64 B more LDS; 2: with top_p, 96 B more; 3:
// level 2 with scores), or 0 where the call would run the per-sample kernels
extern "C" int srnn_gen_persistent_rows_level(int dtype, int n_seqs, int dim, int fs0,
                                              int q_levels, int level) {
    GenMlpPlan pl;
    if (level < 0 || level > 3) return 0;
    if (!gen_mlp_plan(dtype, n_seqs, dim, fs0, q_levels, level, &pl) ||
        !GenSwitches::read().persist)
        return 0;
    return pl.R;
}

extern "C" int srnn_gen_persistent_rows(int dtype, int n_seqs, int dim, int fs0, int q_levels) {
    return srnn_gen_persistent_rows_level(dtype, n_seqs, dim, fs0, q_levels, 0);
}

extern "C" int srnn_gen_persistent_rows_ctrl(int dtype, int n_seqs, int dim, int fs0,
                                             int q_levels) {
    return srnn_gen_persistent_rows_level(dtype, n_seqs, dim, fs0, q_levels, 1);
}

extern "C" int srnn_gen_workspace_size(const SrnnModel* m, int n_seqs, size_t* bytes) {
    SRNN_REQUIRE(m && bytes && n_seqs > 0, "gen_workspace_size: bad args");
    const GenSwitches sw = GenSwitches::read();
    Bufs b;
    GenMlpPlan pl;
    plan_for(m, n_seqs, 0, &pl, sw);      // (the workspace does not depend on the controls)
    *bytes = carve(m, n_seqs, nullptr, &b, &pl, sw);
    return 0;
}

extern "C" size_t srnn_gen_state_bytes(const SrnnModel* m, int n_seqs) {
    if (!m || n_seqs <= 0 || m->n_tiers < 1 || m->n_tiers > SRNN_MAX_TIERS || m->n_rnn < 1 ||
        m->n_rnn > SRNN_MAX_RNN || m->dim <= 0)
        return 0;
    return (size_t)gen_state_row_words(m, GenSwitches::read()) * 4 * (size_t)n_seqs;
}

// The six generations of the entry point (include/samplernn_hip.h states each): all fill one
// request, in its field order, and run it.
extern "C" int srnn_generate(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                             const float* row_bias, const float* noise, uint64_t seed,
                             int64_t* seq, float* logp, void* workspace, size_t workspace_bytes,
                             int flags, void* stream) {
    return gen_run({m, n_seqs, n_cond, cond, row_bias, noise, seed, 0, seq, logp, workspace,
                    workspace_bytes, flags, (hipStream_t)stream});
}

extern "C" int srnn_generate2(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                              const float* row_bias, const float* noise, uint64_t seed,
                              int row0, int64_t* seq, float* logp, void* workspace,
                              size_t workspace_bytes, int flags, void* stream) {
    return gen_run({m, n_seqs, n_cond, cond, row_bias, noise, seed, row0, seq, logp, workspace,
                    workspace_bytes, flags, (hipStream_t)stream});
}

// with per-row sampling controls (sampler.hpp sample_row_ctrl): with both arrays null every
// launch is the plain one; with either, the sampler kernels' controlled instantiations run
// (the persistent loop's own build, planned and checked as such)
extern "C" int srnn_generate3(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                              const float* row_bias, const float* noise, uint64_t seed,
                              int row0, int64_t* seq, float* logp, void* workspace,
                              size_t workspace_bytes, int flags, void* stream,
                              const float* temperature, const int32_t* top_k) {
    return gen_run({m, n_seqs, n_cond, cond, row_bias, noise, seed, row0, seq, logp, workspace,
                    workspace_bytes, flags, (hipStream_t)stream, temperature, top_k});
}

// with the rows' nucleus mass (sampler.hpp, the (tau, k, p) sample_row_ctrl): top_p given
// selects the level-2 instantiations; top_p null launches exactly what srnn_generate3 launches
extern "C" int srnn_generate4(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                              const float* row_bias, const float* noise, uint64_t seed,
                              int row0, int64_t* seq, float* logp, void* workspace,
                              size_t workspace_bytes, int flags, void* stream,
                              const float* temperature, const int32_t* top_k,
                              const float* top_p) {
    return gen_run({m, n_seqs, n_cond, cond, row_bias, noise, seed, row0, seq, logp, workspace,
                    workspace_bytes, flags, (hipStream_t)stream, temperature, top_k, top_p});
}

// that may start from a carried state (st->state_in), return the one it ends in
// (st->state_out), draw its Philox noise from step st->step0 on, and keep the rows' first
// st->n_forced[b] samples as given.  st null or all-default: srnn_generate4's launches.
extern "C" int srnn_generate5(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                              const float* row_bias, const float* noise, uint64_t seed,
                              int row0, int64_t* seq, float* logp, void* workspace,
                              size_t workspace_bytes, int flags, void* stream,
                              const float* temperature, const int32_t* top_k,
                              const float* top_p, const SrnnGenStream* st) {
    return srnn_generate6(m, n_seqs, n_cond, cond, row_bias, noise, seed, row0, seq, logp,
                          workspace, workspace_bytes, flags, stream, temperature, top_k, top_p, st,
                          nullptr);
}

// with the rows' own Philox origins (sampler.hpp sample_noise): rows->noise_row[b] in place of
// row0 + b, rows->step0[b] in place of st->step0.  rows null or both fields null:
// srnn_generate5's launches.
extern "C" int srnn_generate6(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                              const float* row_bias, const float* noise, uint64_t seed,
                              int row0, int64_t* seq, float* logp, void* workspace,
                              size_t workspace_bytes, int flags, void* stream,
                              const float* temperature, const int32_t* top_k,
                              const float* top_p, const SrnnGenStream* st,
                              const SrnnGenRows* rows) {
    static const SrnnGenStream none{};
    static const SrnnGenRows norows{};
    if (!st) st = &none;
    if (!rows) rows = &norows;
    return gen_run({m, n_seqs, n_cond, cond, row_bias, noise, seed, row0, seq, logp, workspace,
                    workspace_bytes, flags, (hipStream_t)stream, temperature, top_k, top_p,
                    st->state_in, st->state_out, st->state_bytes, rows->step0 ? 0u : st->step0,
                    st->n_forced, rows->noise_row, rows->step0});
}

// that also writes the steps' score pairs (sampler.hpp row_score) to score (n_cond L, n_seqs, 2):
// score given selects the scored instantiations (level 3); score null: srnn_generate6, same
// kernels.
extern "C" int srnn_generate7(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                              const float* row_bias, const float* noise, uint64_t seed,
                              int row0, int64_t* seq, float* logp, void* workspace,
                              size_t workspace_bytes, int flags, void* stream,
                              const float* temperature, const int32_t* top_k,
                              const float* top_p, const SrnnGenStream* st,
                              const SrnnGenRows* rows, float* score) {
    static const SrnnGenStream none{};
    static const SrnnGenRows norows{};
    if (!st) st = &none;
    if (!rows) rows = &norows;
    SRNN_REQUIRE(((uintptr_t)score & 7) == 0, "generate: score must be 8-byte aligned");
    return gen_run({m, n_seqs, n_cond, cond, row_bias, noise, seed, row0, seq, logp, workspace,
                    workspace_bytes, flags, (hipStream_t)stream, temperature, top_k, top_p,
                    st->state_in, st->state_out, st->state_bytes, rows->step0 ? 0u : st->step0,
                    st->n_forced, rows->noise_row, rows->step0, score});
}

// n_seqs records of a stream that has done no step, as a fresh start of n_seqs rows computes
// them: a call from them is the call with state_in = NULL, bit for bit
extern "C" int srnn_gen_state_fresh(const SrnnModel* m, int n_seqs, void* state_out,
                                    size_t state_bytes, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    GenRequest rq{m, n_seqs, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, workspace,
                  workspace_bytes, 0, (hipStream_t)stream};
    rq.state_out = state_out;
    rq.state_bytes = state_bytes;
    return gen_fresh(rq);
}

// Draw kernels of a generation call whose rows have their own Philox origins (srnn_generate6,
// continuous batching): the per-sample sampler and the draw-ahead kernel with sample_noise's
// noise_row / row_step0 arrays (sampler.hpp).
//
// They are mlp.hip's sample_kernel and gen_mlp.hip's gen_noise_kernel plus the two arrays, in a
// translation unit of their own: a call without the arrays launches those kernels, and keeping
// these out of their files keeps that code what it was, instruction for instruction (the
// compiler's output for a kernel moves with its module's other contents).
#include "samplernn_hip_internal.hpp"
#include "sampler.hpp"

// One wave per row, as sample_kernel: CT is the level of the row's sampling controls.
template <int CT>
__global__ __launch_bounds__(256) void sample_origin_kernel(
    const float* __restrict__ z, int64_t ldz, int B, const float* __restrict__ noise,
    uint64_t seed, int row0, const int* __restrict__ base, int off, int L,
    int64_t* __restrict__ seq, int64_t ldseq, float* __restrict__ logp_out,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, uint32_t step0, const int* __restrict__ n_forced,
    const int* __restrict__ noise_row, const uint32_t* __restrict__ row_step0) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int i = *base + off;        // absolute sample index being generated
    const int step = i - L;           // relative to the call: the index of logp and of `noise`
    const floatx4 v = *reinterpret_cast<const floatx4*>(z + (int64_t)b * ldz + 4 * lane);
    const floatx4 lq = log_noise(sample_noise(noise, seed, B, b, step, lane, row0, step0,
                                              noise_row, row_step0));
    float* lrow = logp_out ? logp_out + ((int64_t)step * B + b) * 256 : nullptr;
    int bi;
    if constexpr (CT == 2)
        bi = sample_row_ctrl(v, lq, temperature ? temperature[b] : 1.0f, top_k ? top_k[b] : 0,
                             top_p ? top_p[b] : 1.0f, lrow, lane);
    else if constexpr (CT == 1)
        bi = sample_row_ctrl(v, lq, temperature ? temperature[b] : 1.0f, top_k ? top_k[b] : 0,
                             lrow, lane);
    else
        bi = sample_row(v, lq, lrow, lane);
    // forced prefix (controlled instantiations): seq[b, i] stays as the caller gave it
    if constexpr (CT != 0) {
        if (n_forced && step < n_forced[b]) return;
    }
    if (lane == 0) seq[(int64_t)b * ldseq + i] = bi;
}

// The scored build (level 3), mlp.hip's sample_scored_kernel plus the two arrays
__global__ __launch_bounds__(256) void sample_origin_scored_kernel(
    const float* __restrict__ z, int64_t ldz, int B, const float* __restrict__ noise,
    uint64_t seed, int row0, const int* __restrict__ base, int off, int L,
    int64_t* __restrict__ seq, int64_t ldseq, float* __restrict__ logp_out,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, uint32_t step0, const int* __restrict__ n_forced,
    const int* __restrict__ noise_row, const uint32_t* __restrict__ row_step0,
    float* __restrict__ score) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int i = *base + off;
    const int step = i - L;
    const floatx4 v = *reinterpret_cast<const floatx4*>(z + (int64_t)b * ldz + 4 * lane);
    const floatx4 lq = log_noise(sample_noise(noise, seed, B, b, step, lane, row0, step0,
                                              noise_row, row_step0));
    float* lrow = logp_out ? logp_out + ((int64_t)step * B + b) * 256 : nullptr;
    floatx4 zz;
    int bi = sample_row_ctrl_z(v, lq, temperature ? temperature[b] : 1.0f, top_k ? top_k[b] : 0,
                               top_p ? top_p[b] : 1.0f, zz, lane);
    const bool forced = n_forced && step < n_forced[b];
    if (forced) bi = (int)seq[(int64_t)b * ldseq + i] & 255;
    const float2 sc = row_score(zz, bi, lrow, lane);
    if (lane == 0) {
        *reinterpret_cast<float2*>(score + ((int64_t)step * B + b) * 2) = sc;
        if (!forced) seq[(int64_t)b * ldseq + i] = bi;
    }
}

int srnn_sample_origin_impl(const float* z, int64_t ldz, int B, const float* noise,
                            uint64_t seed, int row0, const int* base, int off, int L,
                            int64_t* seq, int64_t ldseq, float* logp_out,
                            const float* temperature, const int* top_k, const float* top_p,
                            uint32_t step0, const int* n_forced, const int* noise_row,
                            const uint32_t* row_step0, float* score, hipStream_t s) {
    const int lv = sample_ctrl_level(temperature, top_k, top_p, n_forced, score);
    if (lv == 3) {
        hipLaunchKernelGGL(sample_origin_scored_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, z, ldz,
                           B, noise, seed, row0, base, off, L, seq, ldseq, logp_out, temperature,
                           top_k, top_p, step0, n_forced, noise_row, row_step0, score);
        SRNN_LAUNCH_CHECK();
        return 0;
    }
    auto k = lv == 2 ? sample_origin_kernel<2>
                     : lv == 1 ? sample_origin_kernel<1> : sample_origin_kernel<0>;
    hipLaunchKernelGGL(k, dim3(cdiv(B, 4)), dim3(256), 0, s, z, ldz, B, noise, seed, row0, base,
                       off, L, seq, ldseq, logp_out, temperature, top_k, top_p, step0, n_forced,
                       noise_row, row_step0);
    SRNN_LAUNCH_CHECK();
    return 0;
}

// A generation session's rows (generate.hip): the Philox step origin of row b is the step count
// of its state record (the int64 at word `word` of a record of rw words; the host has checked
// that it fits 32 bits), taken on the device so that a chunk needs no host round trip.
__global__ __launch_bounds__(256) void gen_rows_step0_kernel(const uint32_t* __restrict__ records,
                                                             int64_t rw, int word, int B,
                                                             uint32_t* __restrict__ step0) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) step0[b] = records[(int64_t)b * rw + word];
}

int gen_rows_step0_launch(const void* records, int64_t rw, int word, int B, uint32_t* step0,
                          hipStream_t s) {
    hipLaunchKernelGGL(gen_rows_step0_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s,
                       (const uint32_t*)records, rw, word, B, step0);
    SRNN_LAUNCH_CHECK();
    return 0;
}

// The persistent loop's error word of a chunk (zeroed at every chunk's start) into the session's
// sticky one: the first error stays.  `err` null (per-sample kernels): nothing to take.
__global__ void gen_rows_err_kernel(const int* __restrict__ err, int* __restrict__ sticky) {
    if (*sticky == 0 && *err != 0) *sticky = *err;
}

int gen_rows_err_launch(const int* err, int* sticky, hipStream_t s) {
    if (!err) return 0;
    hipLaunchKernelGGL(gen_rows_err_kernel, dim3(1), dim3(1), 0, s, err, sticky);
    SRNN_LAUNCH_CHECK();
    return 0;
}

// log q of the draws of nsteps generation steps, one wave per (step, row), as gen_noise_kernel
__global__ __launch_bounds__(256) void gen_noise_origin_kernel(
    const float* __restrict__ noise, uint64_t seed, int row0, const int* __restrict__ base,
    int off, int nsteps, int L, int B, float* __restrict__ lq, uint32_t step0,
    const int* __restrict__ noise_row, const uint32_t* __restrict__ row_step0) {
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (idx >= nsteps * B) return;
    const int s = idx / B, b = idx - s * B;
    const int i = *base + off + s;
    *reinterpret_cast<floatx4*>(lq + ((int64_t)s * B + b) * 256 + 4 * lane) =
        log_noise(sample_noise(noise, seed, B, b, i - L, lane, row0, step0, noise_row, row_step0));
}

int gen_noise_origin_launch(const float* noise, uint64_t seed, int row0, const int* base,
                            int off, int nsteps, int L, int B, float* lq, uint32_t step0,
                            const int* noise_row, const uint32_t* row_step0, hipStream_t s) {
    if (nsteps <= 0 || B <= 0) return 0;
    hipLaunchKernelGGL(gen_noise_origin_kernel, dim3(cdiv((int64_t)nsteps * B, 4)), dim3(256), 0,
                       s, noise, seed, row0, base, off, nsteps, L, B, lq, step0, noise_row,
                       row_step0);
    SRNN_LAUNCH_CHECK();
    return 0;
}

// One GEMM problem, C = act(alpha * op(A) op(B) + beta * Cin + bias) with optional ReLU-backward
// masks, as every GEMM backend sees it: built by the C entries (gemm.hip) and linear_fwd,
// validated once by srnn_gemm_run, then offered to the backends in the router's order.
#pragma once
#include "common.hpp"
#include "samplernn_hip.h"

struct GemmProblem {
    int dtype = SRNN_F32, out_dtype = SRNN_F32;
    int transA = 0, transB = 0;
    int M = 0, N = 0, K = 0, batch = 1;
    float alpha = 1.f, beta = 0.f;
    // operands with their leading dimensions and batch strides (elements)
    const void* A = nullptr;
    int64_t lda = 0, sA = 0;
    const void* B = nullptr;
    int64_t ldb = 0, sB = 0;
    void* C = nullptr;
    int64_t ldc = 0, sC = 0;
    const float* Cin = nullptr;
    int64_t ldcin = 0, sCin = 0;
    const float* bias = nullptr;
    int bias_mode = 0;  // 0 none, 1 per column, 2 per row (srnn_gemm_run: 0 when bias is null)
    int relu = 0;
    // optional relu-backward mask (input dtype): out = 0 where mask <= 0
    const void* mask = nullptr;
    int64_t ldmask = 0;
    // the same mask as bits in (mbi), the ReLU bits of this product's output (mbo); layouts:
    // srnn_bits_index
    const unsigned short* mbi = nullptr;
    int64_t ldmbi = 0;
    unsigned short* mbo = nullptr;
    int64_t ldmbo = 0;
    int tile = -1;  // < 0: the router chooses; else the code that forces one backend (gemm.hip)
    // optional epilogue requests (SrnnGemmEpilogue, samplernn_hip.h): results only gemm3's
    // pair-mode kernels compute.  A backend sets a bit of *served (caller-owned, may be null;
    // srnn_gemm_run clears it on entry) only beside the choice of the kernel variant that
    // computes that result, so "served" and "the launched kernel does it" cannot disagree;
    // a request that is not served leaves its buffer untouched and the caller falls back.
    unsigned* amax = nullptr;  // max |C| of a bf16-output product (the word zero beforehand)
    bf16* blk = nullptr;       // (with amax) also the column-blocked copy [N / 4][M][4] of C
    float* csum = nullptr;     // column sums of a bf16-output product per 128-row block
    int logsoftmax = 0;        // row log-softmax of an fp32-output NT product with N = 256
    unsigned* served = nullptr;

    int es() const { return dtype == SRNN_F32 ? 4 : 2; }      // element size of A, B, mask
    int eo() const { return out_dtype == SRNN_F32 ? 4 : 2; }  // element size of C
    bool kca() const { return !transA; }                      // A is k-contiguous
    bool kcb() const { return transB != 0; }                  // B is k-contiguous
    bool wants_epilogue() const { return amax || csum || logsoftmax; }
};

// p on a `bytes` boundary and its leading dimension a multiple of `mult` elements
static inline bool gemm_aligned(const void* p, int64_t ld, int bytes, int mult) {
    return ((uintptr_t)p % bytes == 0) && (ld % mult == 0);
}

// validates the problem and runs it on the first backend of the router that takes it
int srnn_gemm_run(const GemmProblem& p, hipStream_t s);

// The backends: -1 not taken (the router goes on), 0 done, > 0 error.  Each keeps its own
// eligibility tests at the top and fills its kernel argument block from the record.
int srnn_try_thin(const GemmProblem& p, hipStream_t s);     // gemm_small.hip
int srnn_try_skinny(const GemmProblem& p, hipStream_t s);   // gemm.hip
int srnn_try_blaslt(const GemmProblem& p, hipStream_t s);   // blaslt.cpp
int srnn_try_gemm3(const GemmProblem& p, hipStream_t s);    // gemm3.hip (tile 5: whenever eligible)
int srnn_try_gemm2(const GemmProblem& p, hipStream_t s);    // gemm2.hip
int srnn_try_general(const GemmProblem& p, hipStream_t s);  // gemm.hip: always takes

// f(T{}, TO{}) for the problem's input / output element types
template <typename F>
static inline int gemm_dispatch_types(int dtype, int out_dtype, F&& f) {
    if (dtype == SRNN_F32) return out_dtype == SRNN_F32 ? f(float{}, float{}) : f(float{}, bf16{});
    return out_dtype == SRNN_F32 ? f(bf16{}, float{}) : f(bf16{}, bf16{});
}

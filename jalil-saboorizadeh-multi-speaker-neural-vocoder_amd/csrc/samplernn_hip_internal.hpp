// Internal (C++) entry points shared between translation units of the library.
#pragma once
#include "gemm_problem.hpp"

int srnn_relu_bits_impl(int dtype, const void* a, int64_t lda, int M, int N, unsigned short* bits,
                        int64_t ldb, hipStream_t s);

// u16 index of (row r, 16-column group g) in a ReLU bit mask (gemm.hip): row-major [r][g] with
// row stride ld, or ld == 0: column-group-major [g][M] (the grouped layout)
__host__ __device__ __forceinline__ int64_t srnn_bits_index(int64_t r, int g, int64_t M, int64_t ld) {
    return ld ? r * ld + g : (int64_t)g * M + r;
}

// y[M,N] = act(x[M,K] . W[N,K]^T + bias)   (nn.Linear / Conv1d(k=1) forward)
static inline int linear_fwd(int dt, int odt, int M, int N, int K, const void* x, int64_t ldx,
                             const void* W, int64_t ldw, const float* bias, void* y, int64_t ldy,
                             int relu, hipStream_t s, float beta = 0.f, const float* yin = nullptr,
                             int64_t ldyin = 0) {
    GemmProblem p;
    p.dtype = dt; p.out_dtype = odt; p.transB = 1;
    p.M = M; p.N = N; p.K = K; p.beta = beta;
    p.A = x; p.lda = ldx; p.B = W; p.ldb = ldw; p.C = y; p.ldc = ldy;
    p.Cin = yin; p.ldcin = ldyin; p.bias = bias; p.bias_mode = 1; p.relu = relu;
    return srnn_gemm_run(p, s);
}

// raises a kernel's dynamic LDS limit to `bytes`, once per kernel in the process (persist.hip)
int srnn_raise_lds(const void* kernel, int bytes);

// integer value of an environment switch (dflt when unset or empty)
static inline int env_flag(const char* name, int dflt) {
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}
// whether an environment switch is turned off: set, and its first character is '0'
static inline bool env_off(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
}

// persist.hip: the per-device sticky failure flag of the persistent sweeps (device pointer,
// allocated zeroed on first use; null on a HIP error) and their spin limit (short when the
// SRNN_PERSIST_FORCE_FAIL test switch is set)
int* srnn_sticky_flag();
int srnn_persist_spin_limit(int dflt);
// persist.hip: co-residency of persistent grids (handoff.hpp) -- CUs of the current device,
// whether `blocks` one-per-CU workgroups fit it for every process sharing it, and the
// launch-time check with the kernel's occupancy (0 = fits, else reported error)
int srnn_device_cus();
extern "C" int srnn_device_share(void);
int srnn_persist_fits_cus(int64_t blocks);
int srnn_persist_check(const void* kernel, int threads, size_t lds, int64_t blocks,
                       const char* what);
// persist.hip: what every persistent kernel's argument block copies -- the sticky flag, the
// spin limit (dflt, or the test switch's short one) and the SRNN_PERSIST_FORCE_FAIL withhold
// switch; an error when the flag cannot be allocated
struct PersistCtl { int* sticky; int spin_limit; int withhold; };
int srnn_persist_ctl(PersistCtl& c, int spin_dflt, const char* what);
// persist.hip: launch of a persistent kernel taking the one argument block *args -- raise its
// dynamic LDS limit to lds_limit (0: leave it), srnn_persist_check for the grid, launch, check
int srnn_persist_launch(const void* kernel, dim3 grid, int threads, size_t lds, int lds_limit,
                        void* args, const char* what, hipStream_t s);

// gemm3.hip: grow-only device scratch buffers, one per slot, never freed (a captured HIP graph
// keeps the pointer current at its capture); null on a HIP error.  Allocated on first use,
// i.e. by the eager warm-up step, outside graph captures.
enum { SRNN_SCRATCH_SPLITK = 0, SRNN_SCRATCH_MASK = 1, SRNN_SCRATCH_NT = 2, SRNN_SCRATCH_BLASLT = 3,
       SRNN_SCRATCH_SLOTS = 4 };
void* srnn_scratch(int slot, size_t bytes);

// Deterministic split-K support.  srnn_splitk_scratch = srnn_scratch(SRNN_SCRATCH_SPLITK);
// srnn_splitk_sum writes C[m][n] = sum_z part[z][m][n] in z order (float4 columns:
// N % 4 == 0, C 16-B aligned, ldc % 4 == 0).
// the split-K factor srnn_try_gemm3 picks for a plain fp32-out product of `tiles` 256 x 256 tiles
int srnn_g3_pick_split(int tiles, int K);
float* srnn_splitk_scratch(size_t bytes);
int srnn_splitk_sum(const float* part, float* C, int64_t ldc, int M, int N, int ks, hipStream_t s);

// blaslt.cpp: plain large bf16 GEMMs (alpha, optional per-column bias, optional ReLU, beta 0)
// through hipBLASLt; 0 done, -1 not taken (run the library's own kernels), > 0 error
int srnn_blaslt_enabled();
// (srnn_try_blaslt, gemm_problem.hpp; batch > 1: strided batches, element strides sA / sB /
//  sC; sA or sB may be 0 -- one operand shared by every batch)

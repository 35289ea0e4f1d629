/* samplernn_hip.h -- C ABI of the MI355X-native SampleRNN hot path (libsamplernn_hip.so).
 *
 * Plain pointers and sizes only: every buffer argument is a device pointer allocated
 * and owned by the caller; `stream` is the caller's hipStream_t (NULL = default).
 * Every entry point returns 0 on success, 1 on a bad argument and 2 on a HIP error;
 * srnn_last_error() returns the text (per host thread).  Dtype codes: 0 = fp32,
 * 1 = bf16.  GEMM operands follow BLAS conventions on row-major storage.
 *
 * The reference (mahdeslami11/jalil-saboorizadeh-Multi-speaker-Neural-Vocoder) is pure
 * Python with no FFI; each entry point below names the reference function/operator it
 * replaces.  The drop-in binding is the Python package beside this header
 * (model.py / nn.py / utils.py / optim.py / trainer), see INTEGRATION.md.
 */
#ifndef SAMPLERNN_HIP_H
#define SAMPLERNN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRNN_MAX_TIERS 6
#define SRNN_MAX_RNN 4

const char* srnn_last_error(void);
/* 2.  Version 1 -> 2: srnn_gemm and srnn_gemm_bits gained the SrnnGemmEpilogue* argument in
 * front of `stream`; the seven entries that armed a max |C| / blocked copy / column sum /
 * log-softmax request for "the next GEMM" and read back whether one computed it are gone:
 * that struct carries the requests and the answer.                                       */
int srnn_abi_version(void);
/* Content hash (16 hex digits, csrc/srchash.py) of the sources this library was compiled
 * from; the Python binding refuses a library whose hash differs from its tree's (a stale
 * build).  Replaces no reference interface.                                             */
const char* srnn_build_hash(void);

/* ---- mu-law / linear quantisation ------------------------------------------------
 * utils.uquantize (utils.py:58-59 = midrise(ulaw(x)), utils.py:33-36,48-51): bit-exact to
 * the reference for every float32 / float64 input in [-1, 1] (q_levels = 256).        */
int srnn_uquantize_f32(const float* x, int64_t* out, int64_t n, int q_levels, void* stream);
int srnn_uquantize_f64(const double* x, int64_t* out, int64_t n, int q_levels, void* stream);
/* out = scale * udequantize(k) (utils.py:62-63, mode 0) or linear_dequantize
 * (utils.py:18-19, mode 1); scale = 2 gives the model's `2 * dequantize` (model.py:385,471) */
int srnn_udequantize(const int64_t* k, float* out, int64_t n, int q_levels, float scale,
                     int mode, void* stream);
/* srnn_udequantize of a rows x cols window with row stride ldk (a slice of the index stream,
 * model.py:385 `input_sequences[:, a:b]`) into contiguous rows (no copy of the slice first) */
int srnn_udequantize2d(const int64_t* k, int64_t ldk, float* out, int rows, int cols,
                       int q_levels, float scale, int mode, void* stream);

/* ---- dense projections -------------------------------------------------------------
 * C = act(alpha * op(A) . op(B) + beta * Cin + bias)  (bias_mode 1: per column, 2: per row)
 * Replaces the Conv1d(k=1) / nn.Linear / GRU-input / ConvTranspose1d matmuls of
 * model.py:85-116,148-178,287-301 and nn.py:12-43 (forward, dgrad and wgrad).
 * tile = -1 picks the backend and tile shape from the problem; a tile code that names one
 * backend (3 ring, 4 skinny, 5 256-tile, 6 thin) forces it, and the call fails with a "not
 * eligible" error -- C untouched -- when that backend cannot serve the problem (a batch,
 * its shape or alignment rules); 0 / 1 / 2 force the general kernel's 128 / 64 / 32 tile.
 * mask (optional, input dtype, row stride ldmask) zeroes outputs where mask <= 0 (the ReLU
 * backward of model.py:320-321); in a batch, mask's batch stride is strideC, as C's (there
 * is no stride argument of its own), whatever ldmask is.  beta == 0 never reads Cin, even
 * when it is given.  K == 0 gives act(beta * Cin + bias).
 * epi (optional, NULL = none): further results the same launch may compute, below. */

/* Optional results of one srnn_gemm / srnn_gemm_bits call, computed in the epilogue of the
 * 256 x 256 gemm3 pair-mode kernels alone.  The call clears `served` on entry and sets the bit
 * of every request the launched kernel computes; a request whose bit stays clear -- another
 * backend ran, the shape or epilogue does not fit, the call failed -- left its buffer
 * untouched, and the caller computes that result with a pass of its own.  Buffers are device
 * memory, caller-allocated; the struct itself is host memory read and written during the call
 * only.                                                                                     */
typedef struct SrnnGemmEpilogue {
    unsigned* amax;            /* max |C| as float bits, atomicMax into *amax, which must be
                                * zero beforehand: a bf16-output GEMM (model.py:311-320's da1
                                * = (da2 W_hid) * relu', the GEMM producing the dTab scatter's
                                * input).  Requested together with csum, amax alone is served */
    void* blk;                 /* only with amax: the same GEMM also writes a column-blocked
                                * copy of its bf16 output, blk[N / 4][M][4] (M x N bf16) -- the
                                * dTab scatter's operand layout (srnn_mlp_dtab4).  With grouped
                                * mask bits amax is served without it (AMAX set, BLK clear)  */
    float* csum;               /* column sums of the stored bf16 output per 128-row block,
                                * csum[M / 128][N] fp32 (every entry written once, no zeroing
                                * needed; the caller sums the M / 128 rows): a bf16-output GEMM
                                * without bit masks (model.py:320's da2 = (dz W_out) * relu',
                                * whose column sums are the hidden layer's bias gradient,
                                * model.py:317's Conv1d bias)                                */
    int logsoftmax;            /* nonzero: C receives log_softmax of every output row
                                * (model.py:325) instead of the row: logp = (v - max) -
                                * log(sum exp(v - max)), v = alpha A B^T + bias, the
                                * logsoftmax_nll arithmetic.  An fp32-output NT GEMM with
                                * N = 256 (one 256-column tile: whole rows), no mask, no ReLU,
                                * a per-column bias at most -- the SampleLevelMLP's logits,
                                * model.py:324                                               */
    unsigned served;           /* out: SRNN_EPI_* bits of the requests this call computed    */
} SrnnGemmEpilogue;
#define SRNN_EPI_AMAX 1u
#define SRNN_EPI_BLK 2u
#define SRNN_EPI_CSUM 4u
#define SRNN_EPI_LOGSOFTMAX 8u

int srnn_gemm(int dtype, int out_dtype, int transA, int transB, int M, int N, int K,
              float alpha, const void* A, int64_t lda, int64_t strideA, const void* B,
              int64_t ldb, int64_t strideB, float beta, const float* Cin, int64_t ldcin,
              int64_t strideCin, void* C, int64_t ldc, int64_t strideC, const float* bias,
              int bias_mode, int relu, int batch, int tile, const void* mask, int64_t ldmask,
              SrnnGemmEpilogue* epi, void* stream);

/* The same product (batch 1) with ReLU masks as bits -- bit c % 16 of the u16 at
 * [row * ld + c / 16] is (value(row, c) > 0): mask_bits (optional) zeroes the outputs whose
 * bit is clear (in place of srnn_gemm's bf16 mask, 16x fewer bytes for the ReLU backward of
 * model.py:320-321); bits_out (optional, bf16 out) receives the bits of C (the forward of
 * the ReLU layer, for that backward). */
int srnn_gemm_bits(int dtype, int out_dtype, int transA, int transB, int M, int N, int K,
                   float alpha, const void* A, int64_t lda, const void* B, int64_t ldb,
                   float beta, const float* Cin, int64_t ldcin, void* C, int64_t ldc,
                   const float* bias, int bias_mode, int relu, int tile,
                   const unsigned short* mask_bits, int64_t ldmb, unsigned short* bits_out,
                   int64_t ldbo, SrnnGemmEpilogue* epi, void* stream);
/* bits[row * ldb + c / 16] bit c % 16 = (a[row * lda + c] > 0), a in dtype (M x N).
 * ldb = 0: the grouped layout, u16 [c / 16][row] (N % 64 == 0) -- the same bits, rows
 * contiguous per 16-column group; srnn_gemm_bits takes it (ldmb = 0) and its bf16
 * pair-mode kernels stage it by LDS-DMA ahead of the epilogue.                         */
int srnn_relu_bits(int dtype, const void* a, int64_t lda, int M, int N, unsigned short* bits,
                   int64_t ldb, void* stream);

/* ---- GRU (torch.nn.GRU, model.py:148-165,244): one layer over a whole sequence ----------
 * (csrc/gru_layer.hpp).
 * The library picks the back end for (dtype, B, D) on this device: the XCD-grouped
 * persistent sweep, the LDS-resident persistent sweep, or one srnn_gru_cell launch per step
 * (fp32 always; SRNN_GRU_XCD=0 / SRNN_GRU_SEQ=0 switch a sweep off).  srnn_gru_layer_plan
 * names it and gives the work bytes of either direction (0: pass no work buffer);
 * _plan_for is the same for a device of `ncu` CUs shared by `share` processes.
 * Alignment.  Every operand is addressed by element (any ld / s, any base aligned to its
 * element), with these exceptions, which a call that misses them refuses (non-zero return,
 * nothing written): the XCD sweeps read W_hh / W_hh^T and their work buffer in 16-byte
 * pieces (16-byte aligned pointers); the seq sweeps do so for W_hh / W_hh^T, h0_lp, and for
 * the rows of out_lp and dgh_lp they hand over between steps (16-byte aligned pointers, ldo,
 * so, ldd and sd multiples of 8 elements).  The step kernels take a slower path when h,
 * dgh_next or a weight is not 16-byte aligned with a 16-byte row pitch. */
enum SrnnGruBackend { SRNN_GRU_STEPS = 0, SRNN_GRU_SEQ = 1, SRNN_GRU_XCD = 2 };
int srnn_gru_layer_plan(int dtype, int B, int D, int* backend, size_t* fwd_bytes,
                        size_t* bwd_bytes);
int srnn_gru_layer_plan_for(int dtype, int B, int D, int ncu, int share, int* backend,
                            size_t* fwd_bytes, size_t* bwd_bytes);
/* Forward: x[b][t] = x + b*ld + t*s for gi (3D, includes b_ih), out / out_lp (D; out_lp in
 * `dtype`, NULL in fp32) and gates (4D: r|z|n|gh_n); h0 (B, D) fp32.  hprev_lp (out_lp's
 * layout): [h0, out[:, :Fr-1]] in bf16 for the W_hh gradient -- only the XCD back end
 * writes it, pass NULL under any other plan. */
int srnn_gru_layer_fwd(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                       const float* h0, const void* whh, const float* bhh, float* out,
                       void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                       int64_t sg, void* hprev_lp, void* work, size_t work_bytes, void* stream);
/* Backward (t = Fr-1 .. 0) from dy, the forward's gates / out (hout) / h0, W_hh (3D, D) and
 * its transpose (D, 3D).  dgh / dgh_lp / dgi / dgi_lp share ldd / sd (3D per row and step);
 * ddir0 (B, D) receives dh_direct of step 0.  XCD plan: dgh_lp required, dgh / dgi (fp32),
 * dgi_lp and bsum ((B, 4D): sums over t of [dar | daz | dghn | dan]) optional.  Other plans:
 * dgh, dgi (and dgh_lp in bf16) required, dgi_lp and bsum NULL. */
int srnn_gru_layer_bwd(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                       const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                       int64_t so, const float* h0, const void* whh, const void* whh_t, float* dgh,
                       void* dgh_lp, float* dgi, void* dgi_lp, float* bsum, int64_t ldd,
                       int64_t sd, float* ddir0, void* work, size_t work_bytes, void* stream);

/* One time step for B rows: h_t from h_{t-1} and either x (gi computed in-kernel with
 * W_ih) or a precomputed gi = x W_ih^T + b_ih.  Optionally saves r|z|n|gh_n (4D/row).  */
int srnn_gru_cell(int dtype, int B, int D, int Din, const void* x, int64_t ldx, const void* wih,
                  const float* bih, const float* gi, int64_t ldgi, const void* h, int64_t ldh,
                  const float* hf, int64_t ldhf, const void* whh, const float* bhh, float* hout,
                  int64_t ldho, void* hout_lp, int64_t ldhl, float* gates, int64_t ldgt,
                  void* stream);
/* Backward of one step: dh_t = dy_t + dh_direct_{t+1} + dgh_{t+1} . W_hh, then the gate
 * backward.  Writes dgh_t (fp32 + optional T copy), dgi_t (fp32), dh_direct_t = z*dh_t.
 * Pass W_hh (3D, D) and/or its transpose (D, 3D); the transpose enables the deep-ring
 * kernel.                                                                                */
int srnn_gru_cell_bwd(int dtype, int B, int D, const float* dy, int64_t lddy,
                      const void* dgh_next, int64_t lddgn, const float* ddir_next,
                      const void* whh, const void* whh_t, const float* gates, int64_t ldgt,
                      const float* hprev, int64_t ldhp, float* dgh, int64_t lddgh, void* dgh_lp,
                      int64_t lddghl, float* dgi, int64_t lddgi, float* ddir, void* stream);

/* ---- Forced forms: one back end whatever the plan says, for tests, the benchmark's isolated
 * sweep and probes.  A call its back end does not take is an error ("not supported"); the
 * three queries answer for their back end alone, and 0 while its switch is off. */
/* Whole-sequence forward of one GRU layer in a single persistent launch (bf16, D <= 1024,
 * D % 128 == 0, (D/16) * ceil(B/32) workgroups co-resident): out[b][t] / out_lp /
 * gates[b][t] exactly as Fr calls of srnn_gru_cell with gi[b][t] = gi + b*ldgi + t*sgi.
 * work: >= (64 * ceil(B/32) + 1) ints (zeroed by the call; the last word is an error flag
 * raised if a workgroup gave up waiting).  srnn_gru_seq_supported returns 1 / 0.       */
int srnn_gru_seq_supported(int dtype, int B, int D);
int srnn_gru_seq_fwd(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi,
                     int64_t sgi, const float* h0, const void* h0_lp, const void* whh,
                     const float* bhh, float* out, void* out_lp, int64_t ldo, int64_t so,
                     float* gates, int64_t ldg, int64_t sg, int* work, size_t work_bytes,
                     void* stream);
/* Whole-sequence backward of one GRU layer (t = Fr-1 .. 0) in one persistent launch:
 * the Fr calls of srnn_gru_cell_bwd, with dh_direct kept on chip; ddir0 receives the
 * dh_direct of step 0.  dgh / dgh_lp / dgi share the row stride ldd and step stride sd.  */
int srnn_gru_seq_bwd(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy,
                     int64_t sdy, const float* gates, int64_t ldg, int64_t sg, const float* hout,
                     int64_t ldo, int64_t so, const float* h0, const void* whh_t, float* dgh,
                     void* dgh_lp, float* dgi, int64_t ldd, int64_t sd, float* ddir0, int* work,
                     size_t work_bytes, void* stream);
/* Whole-sequence GRU forward of one layer as ONE persistent launch with row groups placed per
 * XCD (gru_xcd.hip): W_hh resident in VGPRs, h hand-offs as data-tagged granules in the XCD's
 * L2.  Any B: up to 4 tiles of 16 rows per group (512 rows per launch at D = 1024; more rows run
 * as consecutive launches over row chunks, rows being independent).  Same operands and outputs as srnn_gru_seq_fwd (torch.nn.GRU recurrence,
 * model.py:148-165 / 244), gi includes b_ih; work = srnn_gru_xcd_work_bytes(dtype, B, D) bytes
 * (0 = shape or device not supported; zeroed by the call).  srnn_gru_xcd_error(work)
 * synchronises and returns nonzero if a hand-off was given up (bounded spin). */
size_t srnn_gru_xcd_work_bytes(int dtype, int B, int D);
int srnn_gru_xcd_fwd(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                     const float* h0, const void* whh, const float* bhh, float* out,
                     void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                     int64_t sg, void* work, size_t work_bytes, void* stream);
/* srnn_gru_xcd_fwd that also writes the previous-state sequence the W_hh gradient consumes,
 * hprev_lp[b][t] = bf16(t == 0 ? h0[b] : out[b][t - 1]) (same ldo / so layout as out_lp), so the
 * backward needs no shifted copy (model.py:222-244 carry; hprev_lp may be null). */
int srnn_gru_xcd_fwd2(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                      const float* h0, const void* whh, const float* bhh, float* out,
                      void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                      int64_t sg, void* hprev_lp, void* work, size_t work_bytes, void* stream);
/* Reverse sweep of one layer in the same organisation (W_hh^T K-slices in VGPRs, dgh
 * hand-offs as granules): same operands and outputs as srnn_gru_seq_bwd; work =
 * srnn_gru_xcd_bwd_work_bytes(dtype, B, D) bytes. */
size_t srnn_gru_xcd_bwd_work_bytes(int dtype, int B, int D);
int srnn_gru_xcd_bwd(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                     const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                     int64_t so, const float* h0, const void* whh_t, float* dgh, void* dgh_lp,
                     float* dgi, int64_t ldd, int64_t sd, float* ddir0, void* work,
                     size_t work_bytes, void* stream);
/* Same sweep with the bf16 TBPTT step's outputs: dgh / dgi (fp32) may be NULL; dgi_lp (bf16,
 * dgi's layout, the operand of the dW_ih / dX GEMMs) and bsum ((B, 4D) fp32: per batch row the
 * sums over t of [dar | daz | dghn | dan], from which b_hh / b_ih gradients are one column sum)
 * are optional.  Replaces the cast of dgi and the two bias column sums over B x Fr rows. */
int srnn_gru_xcd_bwd2(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                      const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                      int64_t so, const float* h0, const void* whh_t, float* dgh, void* dgh_lp,
                      float* dgi, void* dgi_lp, float* bsum, int64_t ldd, int64_t sd,
                      float* ddir0, void* work, size_t work_bytes, void* stream);
int srnn_gru_xcd_error(const void* work);
/* Sticky form for callers that do not keep the work buffer: nonzero if ANY persistent GRU
 * sweep (srnn_gru_xcd_fwd/bwd, srnn_gru_seq_fwd/bwd) since the previous call gave up a
 * hand-off, -1 on a HIP error; clears the flag and synchronises the device.  While the flag
 * is up srnn_adam_clip_multi skips its update (the failed step's gradients never reach the
 * weights).  The training path checks it once per Trainer iteration (the reference has no
 * equivalent: its cuDNN GRU cannot fail this way).                                        */
int srnn_persistent_error_take(void);
/* Co-residency of the persistent kernels (csrc/handoff.hpp, persist.hip): n processes run
   persistent grids on this device at once (a multi-rank rehearsal on one GPU; default 1).
   Support predicates (srnn_gru_xcd_work_bytes, srnn_gru_seq_supported, the generation plan)
   then only accept grids that fit the device n times over; every persistent launch checks
   occupancy x CUs >= workgroups x n and refuses (error) otherwise.  The reference has no
   counterpart (its GRU is torch.nn.GRU, model.py:148-165).                                 */
int srnn_set_device_share(int n);
int srnn_device_share(void);
/* Diagnostics: occupy `blocks` CUs (160 KiB LDS each) for `usec` us; *done += 1 per
   workgroup at the end (optional) -- the co-residency tests' stand-in for other work.      */
int srnn_hold_cus(int blocks, int usec, int* done, void* stream);
/* Stream-ordered access to that flag for data parallelism: dst = flag ? 1.f : 0.f, and
 * flag |= (src > 0).  The flag rides in a gradient bucket so every rank agrees.           */
int srnn_persistent_flag_to_f32(float* dst, void* stream);
int srnn_persistent_flag_or_f32(const float* src, void* stream);
/* Stream-ordered 4-byte copy of the flag into pinned host memory `dst`: the Trainer's lagged
 * per-iteration check reads step n's copy after enqueuing step n+1 (trainer/__init__.py:116-117
 * without a device synchronisation per iteration). */
int srnn_persistent_flag_snapshot(int* dst, void* stream);
/* dtype (fp32 / bf16) forms of srnn_persistent_flag_to_f32 / _or_f32 (bf16 gradient buckets) */
int srnn_persistent_flag_to(void* dst, int dtype, void* stream);
int srnn_persistent_flag_or(const void* src, int dtype, void* stream);

/* ---- SampleLevelMLP (model.py:308-325) ----------------------------------------------
 * a1[b*Tlen+t] = relu(sum_k tab[k][x[b*ldx + xoff + t + k]] + upper[b*Tlen+t])
 * tab / out in `dtype`; upper in `upper_dtype` (SRNN_F32 or SRNN_BF16)                  */
int srnn_mlp_l1(int dtype, const void* tab, const int64_t* x, int64_t ldx, int xoff, int B,
                int Tlen, int upper_dtype, const void* upper, int64_t ldu, void* out,
                int64_t ldo, int D, int FS0, int Q, void* stream);
/* The same (bf16 table, upper and a1) writing a1's ReLU mask as bits too (srnn_gemm_bits
 * layout, row stride ldb u16; ldb = 0: the grouped layout of srnn_relu_bits), for the
 * masked GEMM of the backward.                                                         */
int srnn_mlp_l1_bits(const void* tab, const int64_t* x, int64_t ldx, int xoff, int B, int Tlen,
                     const void* upper, int64_t ldu, void* out, int64_t ldo, int D, int FS0,
                     int Q, unsigned short* bits, int64_t ldb, void* stream);
/* dtab[x_{t+k}][k][:] += da_t  (Q, FS0, D) fp32 accumulate; backward of the folded     *
 * embedding+conv                                                                        */
int srnn_mlp_dtab(int dtype, const void* da, int64_t ldda, const int64_t* x, int64_t ldx,
                  int xoff, int B, int Tlen, void* dtab, int out_dtype, int D, int FS0, int Q,
                  void* work, size_t work_bytes, void* stream);
/* Same, and (colsum != NULL) the bottom tier's upsampling bias gradient from the same pass:
 * colsum[j * D + c] = sum over batch rows and t = j (mod FS0) of da[b, t, c] (fp32, FS0 x D);
 * *colsum_done (host int) = 1 when it was written (the direct position-major path), else 0
 * and the caller sums the columns itself.                                                   */
int srnn_mlp_dtab2(int dtype, const void* da, int64_t ldda, const int64_t* x, int64_t ldx,
                   int xoff, int B, int Tlen, void* dtab_out, int out_dtype, int D, int FS0, int Q,
                   void* work, size_t work_bytes, float* colsum, int* colsum_done, void* stream);
/* (deterministic: 2^-40 fixed-point int64 accumulation; work >= Q*FS0*D*8 bytes)        *
 * bf16 da and bf16 output at FS0 = 16, Q = 256, D % 8 == 0 take the packed form: two      *
 * columns per 64-bit LDS atomic in 32-bit fixed point at a power-of-2 scale from max |da| *
 * and the most frequent sample value (exact integer sums, deterministic).                 */
/* srnn_mlp_dtab2 with amax_in (device, may be NULL): max |da| as float bits, measured by  *
 * the GEMM that produced da (SrnnGemmEpilogue.amax), so the packed form skips its own pass *
 * over da.  Replaces nothing new in the reference: the same model.py:311-320 backward.    */
int srnn_mlp_dtab3(int dtype, const void* da, int64_t ldda, const int64_t* x, int64_t ldx,
                   int xoff, int B, int Tlen, void* dtab_out, int out_dtype, int D, int FS0, int Q,
                   void* work, size_t work_bytes, float* colsum, int* colsum_done,
                   const unsigned* amax_in, void* stream);
/* Backward of the SampleLevelMLP's output layer (model.py:320-324) in one pass over dz and
 * a2 (bf16, Q = 256, D % 128 == 0, M % 256 == 0; contiguous rows):
 *   da2[M, D]     = bf16(dz . W_out) * [a2 > 0]  -- wt is W_out^T (D, Q); bit-identical to
 *                   srnn_gemm's masked bf16 product on the 256 x 256 pair path
 *   dW[Q, D]      = dz^T . a2  (fp32; per-row-range partials summed in range order:
 *                   deterministic, no atomics)
 *   db[Q]         = column sums of dz, summed the same way (db may be NULL: not computed)
 *   csp[M/128, D] = column sums of the stored da2 per 128-row block, in the order of
 *                   SrnnGemmEpilogue.csum's epilogue (the caller sums the rows: the hidden
 *                   layer's bias gradient)
 * srnn_mlp_out_bwd_ranges returns R, the row ranges a launch uses, or 0 when the shape is
 * not served.  want > 0: that many, clamped to M / 128.  want = 0: the split-K factor
 * srnn_gemm gives the dz^T . a2 product on the 256 x 256 path when its k-slices are whole
 * 128-row blocks -- dW then has that product's bits -- else one workgroup per CU.
 * srnn_mlp_out_bwd runs with the R so obtained; *taken = 1 if it ran, 0 if the shape or an
 * operand's alignment is not served (nothing written: the caller runs the separate calls). */
int srnn_mlp_out_bwd_ranges(int dtype, int64_t M, int D, int Q, int want);
int srnn_mlp_out_bwd(int dtype, const void* dz, const void* a2, const void* wt, int64_t M, int D,
                     int Q, void* da2, float* dW, float* db, float* csp, int R, int* taken,
                     void* stream);
/* srnn_mlp_dtab3 with blk (device, may be NULL): the column-blocked copy of da
 * (blk[D / 4][B * Tlen][4], SrnnGemmEpilogue.blk) the packed form reads instead of da
 * (whole 128-B lines per load).  Same outputs bit for bit.  A sample histogram skewed past
 * the packed form's precision bound (one value at > 65,536 positions) makes the exact
 * 2^-40 form run instead; a non-finite da makes dTab and colsum NaN.  Replaces
 * model.py:311-320's backward like srnn_mlp_dtab.                                         */
int srnn_mlp_dtab4(int dtype, const void* da, int64_t ldda, const int64_t* x, int64_t ldx,
                   int xoff, int B, int Tlen, void* dtab_out, int out_dtype, int D, int FS0, int Q,
                   void* work, size_t work_bytes, float* colsum, int* colsum_done,
                   const unsigned* amax_in, const void* blk, void* stream);
/* 1 if the packed dTab kernels may run: they address their LDS bins without a base, valid
 * only while they have no static LDS (checked from the compiled kernels' attributes; 0 sends
 * srnn_mlp_dtab4 to the exact form).  Diagnostic; needs a device.                        */
int srnn_dtab_packed_ok(void);
/* The routes of srnn_mlp_dtab4 and of srnn_mlp_l1 / srnn_mlp_l1_bits (csrc/mlp_plan.hpp): each
 * operation has one plan, a pure function of the call's shapes, strides, pointer alignments
 * and switches, and these entries report it.  Every route of one operation writes the same
 * bits.  Diagnostic; they replace no reference interface and launch nothing.
 * dTab: packed (bf16 in and out, FS0 = 16, Q = 256, D % 8 == 0 and >= 768, ldda % 8 == 0;
 * SRNN_DTAB_PACK=0 switches it off), direct and posws (the position-major form, FS0 = 16:
 * straight into dtab_out when D >= 765, else through the int64 workspace; SRNN_DTAB_POS=0),
 * generic (any FS0, `cw` columns per workgroup), empty (no rows: zeros).
 * srnn_mlp_dtab_plan_for writes the route, and for it: cw (generic: 4 / 2 / 1), pd (packed: the
 * prefetch depth 1 / 2 / 4; SRNN_DTAB_PD, default by B), x8 (packed: the sample windows are
 * staged as bytes in work; needs room there, SRNN_DTAB_X8=0), use_blk (packed: blk is read;
 * SRNN_DTAB_BLK=0), colsum (1: the route writes colsum and sets *colsum_done when given one)
 * and need_bytes, the work bytes the call requires.  have_amax / have_blk: amax_in / blk would
 * be non-NULL; packed_ok: what srnn_dtab_packed_ok() answers on the device in question.
 * srnn_mlp_dtab_plan is the same with packed_ok taken from the current device.             */
enum SrnnDtabRoute { SRNN_DTAB_EMPTY = 0, SRNN_DTAB_GENERIC = 1, SRNN_DTAB_POSWS = 2,
                     SRNN_DTAB_DIRECT = 3, SRNN_DTAB_PACKED = 4 };
int srnn_mlp_dtab_plan_for(int dtype, int out_dtype, int B, int Tlen, int D, int FS0, int Q,
                           int64_t ldda, int have_amax, int have_blk, size_t work_bytes,
                           int packed_ok, int* route, int* cw, int* pd, int* x8, int* use_blk,
                           int* colsum, size_t* need_bytes);
int srnn_mlp_dtab_plan(int dtype, int out_dtype, int B, int Tlen, int D, int FS0, int Q,
                       int64_t ldda, int have_amax, int have_blk, size_t work_bytes, int* route,
                       int* cw, int* pd, int* x8, int* use_blk, int* colsum, size_t* need_bytes);
/* L1 gather: lds (bf16 table and upper, FS0 = 16, Q = 256, D % 16 == 0, Tlen <= 2029; the
 * table slice stays in LDS; SRNN_L1_LDS=0 switches it off), xcd (D % 128 == 0) -- both need
 * >= 4096 rows, 16-byte aligned tab / upper / out and 16-byte row pitches, and no device
 * `base` offset (generation's single rows) -- else generic.  tab / upper / out are looked at
 * as addresses only, never read.  *bits_pass = 1: with have_bits the mask bits come from a
 * separate srnn_relu_bits pass over out (every route but lds, which writes them itself).   */
enum SrnnL1Route { SRNN_L1_GENERIC = 0, SRNN_L1_XCD = 1, SRNN_L1_LDS = 2 };
int srnn_mlp_l1_plan_for(int dtype, int upper_dtype, int B, int Tlen, int D, int FS0, int Q,
                         const void* tab, const void* upper, int64_t ldu, const void* out,
                         int64_t ldo, int have_base, int have_bits, int* route, int* bits_pass);
/* Number of GEMMs srnn_gemm / srnn_gemm_bits handed to hipBLASLt so far in this process:
 * large plain bf16 problems (alpha, per-column bias, ReLU, beta 0, no mask; M N >= 4 Mi,
 * 2 M N K >= 2^33) run as the ROCm library GEMM (SRNN_BLASLT=0: the library's own gemm3
 * kernels).  Diagnostic; replaces no reference interface.                               */
int srnn_blaslt_calls(void);
/* Routing of srnn_blaslt_calls' path: plain bf16 problems with fewer than min_outputs
 * outputs (M N) or min_flop flop (2 M N K) stay on the hand-written kernels (defaults 4 Mi and
 * 2^33; env SRNN_BLASLT_MIN_MN / SRNN_BLASLT_MIN_MFLOP).  srnn_blaslt_set_tune(n): n > 1 times
 * the library heuristic's first n algorithms once per shape, outside graph capture, on the
 * call's own operands and keeps the fastest (0: the heuristic's first; env SRNN_BLASLT_TUNE).
 * Tuning knobs; replace no reference interface.                                           */
int srnn_blaslt_set_min(long long min_outputs, double min_flop);
int srnn_blaslt_set_tune(int n);
/* log_softmax (model.py:324-325) + NLL rows (nn.py:66-70) + dlogits (softmax-onehot)*g  */
/* dz = dlogp - exp(logp) * rowsum(dlogp)   (log_softmax backward, rows of Q)          */
int srnn_logsoftmax_bwd(const float* dlogp, int64_t lddl, const float* logp, int64_t ldl,
                        int64_t rows, int Q, void* dz, int dz_dtype, int64_t ldd, void* stream);
/* NLL over log-probs (nn.py:66-70): loss_row[r] = -logp[r, target]; and its gradient
 * dlogp[r, :] = 0 except dlogp[r, target] = -gscale                                      */
int srnn_nll_fwd(const float* logp, int64_t ldl, const int64_t* target, int64_t ldt, int Tlen,
                 int64_t rows, float* loss_row, void* stream);
int srnn_nll_bwd(const int64_t* target, int64_t ldt, int Tlen, int64_t rows, int Q,
                 float* dlogp, int64_t ldd, float gscale, const float* gmul, void* stream);
/* Fused backward of sequence_nll_loss_bits (nn.py:66-70) through the MLP's log_softmax
 * (model.py:324-325): dz = c (exp(logp) - onehot(target)), c = gscale * (*gmul), in dz_dtype
 * (fp32 / bf16) -- srnn_nll_bwd + srnn_logsoftmax_bwd in one pass, bit-identical to them,
 * without the dense fp32 dlogp. */
int srnn_nll_logsoftmax_bwd(const int64_t* target, int64_t ldt, int Tlen, int64_t rows, int Q,
                            const float* logp, int64_t ldl, float gscale, const float* gmul,
                            void* dz, int dz_dtype, int64_t ldd, void* stream);
/* (gmul: optional device scalar the scale is multiplied by -- the incoming loss gradient,
 *  read on the device so the backward never synchronises with the host)                 */
int srnn_logsoftmax_nll(const float* z, int64_t ldz, const int64_t* target, int64_t ldt,
                        int Tlen, int64_t rows, int Q, float* loss_row, float* logp,
                        int64_t ldl, void* dz, int dz_dtype, int64_t ldd, float gscale,
                        void* stream);

/* Host-side (no GPU) bit-exact quantisers with the same tables, for the CPU data path. */
int srnn_uquantize_f64_host(const double* x, int64_t* out, int64_t n, int q_levels);
int srnn_uquantize_f32_host(const float* x, int64_t* out, int64_t n, int q_levels);
int srnn_udequantize_host(const int64_t* k, float* out, int64_t n, int q_levels);

/* ---- weight norm (torch weight_norm dim=0, model.py:119-131,177-178,303-306) -------- */
int srnn_weight_norm_fwd(const float* g, const float* v, float* w, float* norm, int O,
                         int64_t R, void* stream);
int srnn_weight_norm_bwd(const float* g, const float* v, const float* dw, float* dg, float* dv,
                         int O, int64_t R, int accumulate, void* stream);
/* The always-on weight norm of LearnedUpsampling1d.conv_t (model.py:177-178) folded into its
 * GEMM operand: scale[i] = g[i] / ||v[i]||; dst[(j * Cout + o) * Cin + i] = v[i][o][j] * scale[i]
 * (dst fp32 or bf16; scale NULL = 1: a plain (2, 1, 0) permute); backward from the GEMM's
 * transposed weight gradient dwt[i][(j * Cout + o)] to dg[i] and dv (v's layout).          */
int srnn_weight_norm_scale(const float* g, const float* v, float* scale, int O, int64_t R,
                           void* stream);
int srnn_convt_fold(const float* v, const float* scale, void* dst, int dst_dtype, int Cin,
                    int Cout, int k, void* stream);
int srnn_convt_wn_bwd(const float* g, const float* v, const float* dwt, float* dg, float* dv,
                      int Cin, int Cout, int k, void* stream);

/* ---- layout / elementwise helpers ------------------------------------------------- */
int srnn_permute3(const float* src, void* dst, int dst_dtype, int d0, int d1, int d2, int p0,
                  int p1, int p2, int accumulate, void* stream);
int srnn_copy2d(int src_dtype, int dst_dtype, int rows, int cols, const void* src, int64_t lds,
                void* dst, int64_t ldd, void* stream);
int srnn_gather_rows(const float* table, int64_t ldt, const int64_t* idx, int64_t n, int cols,
                     void* out, int out_dtype, int64_t ldo, void* stream);
int srnn_scatter_add_rows(float* table, int64_t ldt, const int64_t* idx, int64_t n, int cols,
                          const float* src, int64_t lds, void* stream);
/* table[q,:] += sum_{r: idx[r]==q} src[r,:] in r order, q < trows -- the speaker-embedding
   backward (model.py:203-207, nn.Embedding's gradient) without atomics: deterministic     */
int srnn_index_add_rows(float* table, int64_t ldt, int trows, const int64_t* idx, int64_t n,
                        int cols, const float* src, int64_t lds, void* stream);
int srnn_axpby(float* out, const float* a, const float* b, float alpha, float beta, int64_t n,
               void* stream);
int srnn_add_bcast_rows(float* x, const float* v, int B, int F, int D, int64_t ldv, void* stream);
/* out[b][c] = sum_{f<F} src[(b*F + f)*lds + c]  (per-sequence frame sums, fp32)        */
int srnn_segsum(const float* src, int64_t lds, int B, int F, int D, float* out, void* stream);
int srnn_colsum(int dtype, const void* src, int64_t lds, int64_t rows, int cols, float* out,
                float alpha, int accumulate, float* work, int64_t work_elems, void* stream);

/* ---- optimizer: gradient_clipping(-1, 1) + Adam (optim.py:4-21, train.py:238) --------
 * Elementwise in-place clamp of g to [clip_lo, clip_hi] then torch.optim.Adam update.
 * p_bf16 (optional) receives the updated parameters rounded to bf16.                    */
int srnn_adam_clip(float* p, float* g, float* m, float* v, void* p_bf16, int64_t n,
                   float clip_lo, float clip_hi, double lr, double beta1, double beta2,
                   double eps, int64_t step, void* stream);
/* The same for `ntensors` parameters in one launch (per 64 tensors): host arrays of device
 * pointers and element counts; p_bf16 may be NULL (no copies) or hold NULL entries; a NULL
 * entry of g is an all-zero gradient (a parameter the step's backward did not reach).
 * Skipped entirely (on the device) while the persistent-sweep failure flag is up.        */
int srnn_adam_clip_multi(int ntensors, float* const* p, float* const* g, float* const* m,
                         float* const* v, void* const* p_bf16, const int64_t* n, float clip_lo,
                         float clip_hi, double lr, double beta1, double beta2, double eps,
                         int64_t step, void* stream);
/* srnn_adam_clip_multi over gradients of dtype gdtype (fp32, or bf16 from bf16 gradient
 * buckets) scaled by gscale before the clamp: under data parallelism the SUM-reduced buckets
 * are read in place with gscale = 1 / world (the mean before the clip, optim.py:11-13 applied
 * to the full-batch gradient).  fp32 gradients are written back clamped, bf16 ones only read. */
int srnn_adam_clip_multi2(int ntensors, float* const* p, void* const* g, int gdtype, float gscale,
                          float* const* m, float* const* v, void* const* p_bf16, const int64_t* n,
                          float clip_lo, float clip_hi, double lr, double beta1, double beta2,
                          double eps, int64_t step, void* stream);
/* srnn_adam_clip_multi2 with the step count on the device: dstep (NULL = use `step`) holds
 * the number of completed steps and the kernel takes step = *dstep + 1 for the bias
 * corrections (host formula, torch.optim.Adam).  With srnn_step_advance this makes the
 * optimizer step replayable from a captured HIP graph (trainer/__init__.py graph mode).   */
int srnn_adam_clip_multi3(int ntensors, float* const* p, void* const* g, int gdtype, float gscale,
                          float* const* m, float* const* v, void* const* p_bf16, const int64_t* n,
                          float clip_lo, float clip_hi, double lr, double beta1, double beta2,
                          double eps, int64_t step, const int64_t* dstep, void* stream);
/* dstep[0..n) += 1 unless the persistent-sweep failure flag is up (the step's update was
 * skipped, so its count must not advance either).  n <= 1024.                            */
int srnn_step_advance(int64_t* dstep, int n, void* stream);
/* Data-parallel gradient bucket packing: src[i] (fp32, n[i] elements, NULL = zeros) ->
 * flat + dst_off[i] in dtype (fp32 / bf16), all tensors in one launch.  The reference has no
 * distributed step; this feeds distributed.GradAllReduce's RCCL all-reduce.   */
int srnn_pack_grads(int ntensors, const float* const* src, const int64_t* n,
                    const int64_t* dst_off, void* flat, int dtype, void* stream);
/* bf16 copies of n fp32 tensors (dst[t][j] = bf16(src[t][j]), j < n[t]) in one launch per 64
 * tensors: ZeRO-1 data parallelism refreshes every parameter's bf16 copy after the parameter
 * all-gather (the reference's replicated Adam, optim.py:4-21, sharded over ranks).          */
int srnn_cast_multi(int ntensors, const float* const* src, void* const* dst, const int64_t* n,
                    void* stream);

/* ---- autoregressive generation (Generator.__call__, model.py:445-520) --------------- */
typedef struct SrnnTier {
    int frame_size;            /* upsampling ratio of this tier                           */
    int n_frame_samples;       /* nfs = cumprod(frame_sizes)                              */
    int in_dim;                /* columns of w_in: nfs (+ cond_dim for the top tier)      */
    const void* w_in;          /* (D, in_dim) [input_expand | cond_expand]               */
    const float* b_in;         /* (D) input_expand bias (lower tiers; top uses row_bias)  */
    const void* w_ih[SRNN_MAX_RNN];
    const float* b_ih[SRNN_MAX_RNN];
    const void* w_hh[SRNN_MAX_RNN];
    const float* b_hh[SRNN_MAX_RNN];
    const void* w_up;          /* (fs*D, D): row j*D+o = conv_t.weight[:, o, j]            */
    const float* b_up;         /* (fs*D):   [j*D+o] = upsampling.bias[o, j]               */
    const float* h0;           /* (n_rnn, D) learned / buffer initial state               */
} SrnnTier;

typedef struct SrnnModel {
    int n_tiers, n_rnn, dim, q_levels, cond_dim, dtype;
    SrnnTier tier[SRNN_MAX_TIERS]; /* index 0 = bottom tier (frame_sizes[0])             */
    const void* tab;           /* (FS0, Q, D) folded embedding . input conv               */
    const void* w_hid;         /* (D, D)  */
    const float* b_hid;
    const void* w_out;         /* (Q, D)  */
    const float* b_out;
} SrnnModel;

/* Rows per group R (8 or 16) of the persistent generation sample loop (gen_mlp.hip) for this
 * shape on this device, or 0 when srnn_generate will use per-sample kernels instead.
 * Replaces nothing in the reference: a capability query for the Generator wrapper. */
int srnn_gen_persistent_rows(int dtype, int n_seqs, int dim, int fs0, int q_levels);
/* The same query for a call with sampling controls (srnn_generate3 given an array): the plan
 * of the loop's controlled instantiation. */
int srnn_gen_persistent_rows_ctrl(int dtype, int n_seqs, int dim, int fs0, int q_levels);
/* Workspace bytes needed by srnn_generate for n_seqs rows. */
int srnn_gen_workspace_size(const SrnnModel* m, int n_seqs, size_t* bytes);
/* Generates n_cond * lookback samples for n_seqs rows.
 *   cond     (n_seqs, n_cond, cond_dim) fp32, per-row conditioning frames
 *   row_bias (n_seqs, D) fp32 = spk_expand(spk_embedding(spk)) + b_spk + b_cond + b_in (top)
 *   noise    (n_cond*L, n_seqs, Q) fp32 Exp(1) draws consumed as argmax(p/q), or NULL to
 *            draw q in-kernel from Philox4x32-10(seed)
 *   seq      (n_seqs, L + n_cond*L) int64, columns [0, L) pre-filled (q_zero); output
 *   logp     optional (n_cond*L, n_seqs, Q) fp32 per-step log-probs (debug / parity)
 *   flags    bit 0: replay the generation block as a hipGraph
 *            bit 1: per-sample kernels instead of the persistent sample loop (gen_mlp.hip,
 *                   used by default where the shape fits; env SRNN_GEN_PERSIST=0 also
 *                   disables it)                                                        */
int srnn_generate(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                  const float* row_bias, const float* noise, uint64_t seed, int64_t* seq,
                  float* logp, void* workspace, size_t workspace_bytes, int flags, void* stream);
/* srnn_generate for rows [row0, row0 + n_seqs) of a larger batch (rank-sharded generation,
 * SURVEY §8e, generate.py:241-253 run per rank): the Philox noise of local row b is that of
 * global row row0 + b, so the shards together draw exactly the single-process stream.    */
int srnn_generate2(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                   const float* row_bias, const float* noise, uint64_t seed, int row0,
                   int64_t* seq, float* logp, void* workspace, size_t workspace_bytes, int flags,
                   void* stream);
/* srnn_generate2 with per-row sampling controls.  Extends the draw of model.py:514-517
 * (multinomial of the model's softmax: no temperature, no truncation) inside the same launches:
 *   temperature (n_seqs) fp32 device array or NULL (= 1 for every row).  Domain: finite, >= 0.
 *   top_k       (n_seqs) int32 device array or NULL (= off for every row).  Domain: [0, Q];
 *               0 and Q both mean off.
 * Per row b, with z the step's logits and q its noise (the same noise as without controls:
 * Philox counters and the replayed `noise` indexing are unchanged):
 *   S = {j : z_j >= v_k}, v_k the k-th largest logit (ties at v_k all kept; off: every j)
 *   tau > 0:  x = argmax_{j in S} (z_j - tau log q_j)   (tau = 1, k off: srnn_generate2's draw,
 *                                                        bit for bit)
 *   tau = 0:  x = argmax_{j in S} z_j                    (greedy; the noise is not used)
 * first index on ties.  The kernels do not validate: k outside [1, Q - 1] is treated as off and
 * tau <= 0 (or NaN) as greedy; callers check the domain (model.sampling_controls does).
 * `logp` stays the model's own log-softmax of z, not the tempered / truncated distribution.
 * The arrays are read by every launch (and every graph replay): they must stay valid and
 * unchanged until the call returns.  Both NULL: exactly srnn_generate2 (same kernels).  With
 * either, the samplers' controlled instantiations run; the persistent loop's co-residency
 * check is made on that instantiation.                                                    */
int srnn_generate3(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                   const float* row_bias, const float* noise, uint64_t seed, int row0,
                   int64_t* seq, float* logp, void* workspace, size_t workspace_bytes, int flags,
                   void* stream, const float* temperature, const int32_t* top_k);
/* srnn_generate3 with a per-row nucleus (top-p) cut-off as the third control:
 *   top_p       (n_seqs) fp32 device array or NULL (= 1, off, for every row).  Domain: 0 < p <= 1.
 * Everything srnn_generate3 states stays; S is its top-k set.  For tau > 0 and p < 1:
 *   w_j = exp((z_j - max z) / tau) for j in S,  W = sum_S w_j
 *   N   = {j in S : z_j >= v_p}, v_p the LARGEST logit value v with
 *         sum_{j in S, z_j >= v} w_j >= p W
 *         (the smallest set of most probable classes whose tempered mass, renormalised over S,
 *          reaches p: the class that crosses p is included, ties at v_p are all kept)
 *   x   = argmax_{j in N} (z_j - tau log q_j), first index on ties
 * tau = 0 (greedy) ignores p; p = 1 skips the select and the row's draw is srnn_generate3's, bit
 * for bit.  Masses are compared in integer fixed point (u_j = rint(2^22 w_j), exact sums): a
 * normalised partial mass is off by less than 1e-4, and the comparison is
 * the same in every kernel.  The kernels do not validate: p outside (0, 1), or NaN, is treated
 * as off; callers check the domain (model.nucleus_control does).  Noise consumption and `logp`
 * are unchanged.  top_p NULL: exactly srnn_generate3 (same kernels).  top_p given: the samplers'
 * level-2 instantiations run, whichever of temperature / top_k are given, and the persistent
 * loop's co-residency check is made on that instantiation.                                  */
int srnn_generate4(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                   const float* row_bias, const float* noise, uint64_t seed, int row0,
                   int64_t* seq, float* logp, void* workspace, size_t workspace_bytes, int flags,
                   void* stream, const float* temperature, const int32_t* top_k,
                   const float* top_p);
/* srnn_gen_persistent_rows for a call at sampling-control level `level`: 0 none (the plain
 * plan), 1 temperature / top_k (srnn_gen_persistent_rows_ctrl), 2 with top_p.  Other levels: 0. */
int srnn_gen_persistent_rows_level(int dtype, int n_seqs, int dim, int fs0, int q_levels,
                                   int level);
/* The engine's row sampler on caller-chosen logits: one draw per row, by the same device
 * functions as srnn_generate4's loops, at the control level the arrays imply (all NULL: the
 * plain draw of srnn_generate).
 *   logits      (rows, 256) fp32, leading dimension ld >= 256 floats; rows 16-byte aligned
 *   noise       (rows, 256) fp32 Exp(1) draws (contiguous, 16-byte aligned), or NULL to draw
 *               from Philox4x32-10 with (seed, row0, step): the counters the loop uses for global
 *               row row0 + b at generation step `step` (seed, row0 and step are otherwise unused)
 *   temperature / top_k / top_p   (rows) device arrays or NULL, as in srnn_generate4
 *   index       (rows) int64, output
 *   logp        optional (rows, 256) fp32: log_softmax(logits), whatever the controls        */
int srnn_sample_rows(const float* logits, int64_t ld, int rows, const float* noise, uint64_t seed,
                     int row0, int step, const float* temperature, const int32_t* top_k,
                     const float* top_p, int64_t* index, float* logp, void* stream);
/* srnn_sample_rows that also writes the rows' score pairs: score (rows, 2) fp32, 8-byte aligned,
 * {log-prob of the row's drawn index, entropy of softmax(logits) in nats}, both of the model's
 * own distribution whatever the controls (score[0] is logp[index], bit for bit).  Given, it
 * selects the scored instantiation (level 3); NULL: exactly srnn_sample_rows, same kernels.    */
int srnn_sample_rows2(const float* logits, int64_t ld, int rows, const float* noise,
                      uint64_t seed, int row0, int step, const float* temperature,
                      const int32_t* top_k, const float* top_p, int64_t* index, float* logp,
                      void* stream, float* score);

/* ---- streaming: carried state and a forced prefix ------------------------------------------
 * Bytes of the opaque recurrent state of n_seqs rows of model m as srnn_generate5 reads and
 * writes it: row-major, one record per row, so the result is a multiple of n_seqs and the row
 * stride is the quotient.  A record depends on its row's history only: callers may reorder,
 * drop or duplicate rows by moving whole records.  0: bad arguments.  A record holds a header
 * (layout tag, dtype, n_tiers, n_rnn, dim, lookback L, fold flags, the row's completed step
 * count as int64), the row's last L sample indices, every tier / layer's fp32 hidden state and,
 * where a tier's tick is folded, the h W_hh^T + b_hh rows its next tick
 * takes.  The layout depends on the model, its dtype and the fold decisions (environment
 * switches such as SRNN_GEN_FOLD among them).                                                */
size_t srnn_gen_state_bytes(const SrnnModel* m, int n_seqs);

typedef struct SrnnGenStream {
    const void* state_in;      /* device: state to continue from, or NULL = fresh start (h0,
                                * q_zero history as pre-filled by the caller)                  */
    void* state_out;           /* device: receives the state the call ends in, or NULL; may
                                * alias state_in                                              */
    size_t state_bytes;        /* size of either buffer: srnn_gen_state_bytes(m, n_seqs)       */
    uint32_t step0;            /* generation steps the stream completed before this call: the
                                * Philox step of the call's sample t is step0 + t              */
    const int32_t* n_forced;   /* device (n_seqs) forced prefix lengths, or NULL (= 0)         */
} SrnnGenStream;

/* srnn_generate4 that may continue a stream and may be forced along a given prefix.  With st
 * NULL, or all of its fields 0 / NULL, it is exactly srnn_generate4 (same kernels).
 *   state_in   the call starts from these records in place of h0 / the pre-filled history: seq
 *              columns [0, L) are WRITTEN by the call from the records.  Every record's header
 *              must match the call's model, dtype and fold decisions, else the call fails with
 *              return code 1 and a message, before anything is written.
 *   state_out  the records of the state after the call's n_cond * L steps; a row's step count is
 *              its state_in count (0 on a fresh start) plus n_cond * L.
 *   step0      only moves the Philox counters (step0 + n_cond * L must fit 32 bits, else return
 *              code 1).  A replayed `noise` buffer and `logp` stay indexed from the call's own
 *              first step.  At step0 = 0 the draws are srnn_generate4's.
 *   n_forced   the caller pre-fills seq columns [L, L + n_forced[b]) of row b.  At those steps
 *              the row's logits, log-probs (`logp`) and noise consumption are what they would be
 *              anyway, but the step's sample is the given one in place of the draw (whatever
 *              temperature, top_k and top_p say) and seq is not written; the history the tiers
 *              and the following steps see is the forced one.  Values are clamped to
 *              [0, n_cond * L]; callers check the domain, and that the given samples lie in
 *              [0, Q) (Generator.__call__ does).  Given, it selects the samplers' controlled
 *              instantiations (level 1, or 2 with top_p) with temperature 1 and top-k off for the
 *              arrays that are NULL; n_cond * L must then be below 2^23.
 * A stream generated as consecutive calls, each continuing from the previous call's state_out
 * with its own slice of cond (and of a replayed noise buffer), equals the single call over all
 * the frames bit for bit, indices and log-probs: the calls split the stream at top-tier period
 * boundaries, where every tier ticks and nothing but the recorded state is carried.          */
int srnn_generate5(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                   const float* row_bias, const float* noise, uint64_t seed, int row0,
                   int64_t* seq, float* logp, void* workspace, size_t workspace_bytes, int flags,
                   void* stream, const float* temperature, const int32_t* top_k,
                   const float* top_p, const SrnnGenStream* st);

typedef struct SrnnGenRows {
    const int32_t*  noise_row;  /* device (n_seqs) or NULL: Philox row of local row b       */
    const uint32_t* step0;      /* device (n_seqs) or NULL: Philox step of row b's sample 0  */
} SrnnGenRows;

/* srnn_generate5 whose rows may each have their own Philox origin, so that a stream keeps its
 * noise whichever local row serves it and whatever the other rows' step counts are (continuous
 * batching: rows of one call at different points of different utterances).  With rows NULL, or
 * both of its fields NULL, it is exactly srnn_generate5 (same kernels).
 *   noise_row  the Philox row of local row b is noise_row[b] in place of row0 + b.  Every value
 *              must be >= 0, else return code 1 and a message, before anything is written.
 *              Equal values are allowed: such rows draw the same noise.
 *   step0      the Philox step of row b's sample t is step0[b] + t; st->step0 is then ignored.
 *              step0[b] + n_cond * L must fit 32 bits for every row, else return code 1 and a
 *              message, before anything is written.
 * Both arrays only move Philox counters: a replayed `noise` buffer and `logp` keep their index
 * from the call's own first step and the call's own row b, and with `noise` given the arrays are
 * not read.  The arrays are read on the host once (the call synchronises `stream` first) and by
 * the launches that draw noise; a call with either array draws every launch's noise ahead of the
 * persistent sample loop (as SRNN_GEN_NOISE_AHEAD=1 does, whatever that switch says), because
 * the loop's own draw knows no per-row origin.                                               */
int srnn_generate6(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                   const float* row_bias, const float* noise, uint64_t seed, int row0,
                   int64_t* seq, float* logp, void* workspace, size_t workspace_bytes, int flags,
                   void* stream, const float* temperature, const int32_t* top_k,
                   const float* top_p, const SrnnGenStream* st, const SrnnGenRows* rows);

/* srnn_generate6 that also writes every step's score pair: score (n_cond * L, n_seqs, 2) fp32,
 * device, 8-byte aligned, indexed as logp is (step * n_seqs + b):
 *   score[0]  log-prob of the step's sample -- the index drawn, or the caller's sample at a
 *             forced step -- equal to logp[step, b, sample] bit for bit
 *   score[1]  entropy of the model's softmax at that step, in nats, never negative
 * Both describe the model's own distribution, whatever temperature, top_k and top_p did to the
 * draw.  8 bytes per row-step where logp takes 1,024: with every step forced (st->n_forced) the
 * call scores given audio.  score given selects the samplers' scored instantiations (level 3:
 * level 2 plus the pair; default controls draw the plain stream bit for bit); with score NULL it
 * is exactly srnn_generate6 (same kernels).  srnn_gen_persistent_rows_level answers for level 3. */
int srnn_generate7(const SrnnModel* m, int n_seqs, int n_cond, const float* cond,
                   const float* row_bias, const float* noise, uint64_t seed, int row0,
                   int64_t* seq, float* logp, void* workspace, size_t workspace_bytes, int flags,
                   void* stream, const float* temperature, const int32_t* top_k,
                   const float* top_p, const SrnnGenStream* st, const SrnnGenRows* rows,
                   float* score);

/* Writes to state_out (device, state_bytes = srnn_gen_state_bytes(m, n_seqs), 8-byte aligned)
 * the records of n_seqs rows that have done no step: this process's header, step count 0, a
 * q_zero history (q_levels / 2), h0 of every tier and layer and, with folded ticks, their carried
 * products exactly as a fresh start of n_seqs rows computes them.  A srnn_generate5 / 6 call of
 * n_seqs rows with state_in set to these records equals the call with state_in = NULL bit for
 * bit -- indices, log-probs and state_out -- and all n_seqs records are equal, so any of them
 * may start a new stream in a row of a call whose other rows are mid-stream.  workspace: as for
 * srnn_generate (srnn_gen_workspace_size(m, n_seqs)).  Synchronises before it returns.         */
int srnn_gen_state_fresh(const SrnnModel* m, int n_seqs, void* state_out, size_t state_bytes,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- generation sessions: weights, workspace and graph kept across chunks -------------------
 * A session runs consecutive srnn_generate6 calls of one (model, n_seqs, control level, flags)
 * without their per-call set-up: the tick weights are folded, the workspace laid out and the
 * rows' fresh records made once, at open, and the captured generation block is replayed by every
 * later chunk.  What a chunk computes is what the srnn_generate6 call with the same inputs,
 * state_in = the session's records and rows = {noise_row, the records' step counts} computes, bit
 * for bit: a session always runs on the per-row-origin path.  Replaces nothing in the reference.
 * Device memory is the caller's: one arena of srnn_gen_session_bytes bytes, 256-byte aligned,
 * which the session carves and which must stay allocated and untouched until close.  The
 * SrnnModel is copied at open; the weights its pointers name must stay valid and UNCHANGED for
 * the session's life (the folded weights are made from them once).  A session's work runs on a
 * private stream; a session is used by one host thread at a time.                              */
typedef struct SrnnGenSession SrnnGenSession;

#define SRNN_GEN_SESSION_GRAPH      1   /* replay the generation blocks as hipGraphs          */
#define SRNN_GEN_SESSION_PER_SAMPLE 2   /* per-sample kernels, not the persistent sample loop */
#define SRNN_GEN_SESSION_LOGP       4   /* chunks may ask for log-probs                       */
#define SRNN_GEN_SESSION_NOISE      8   /* every chunk brings replayed noise (no Philox)      */
#define SRNN_GEN_SESSION_SCORE     16   /* chunks may ask for score pairs (srnn_generate7): the
                                         * session's level must then be 3, and only then; the
                                         * arena grows by max_frames * L * n_seqs * 8 bytes    */

/* Arena bytes of a session.  Domains: n_seqs >= 1, max_frames >= 1, level in {0, 1, 2} (the
 * sampling controls its chunks may carry: 0 none, 1 temperature / top_k / a forced prefix, 2
 * with top_p), flags a sum of SRNN_GEN_SESSION_*.  Writes *bytes; 1 on bad arguments.          */
int srnn_gen_session_bytes(const SrnnModel* m, int n_seqs, int max_frames, int level, int flags,
                           size_t* bytes);
/* Opens a session in `arena` and writes its handle to *out: validates, folds the tick weights
 * (what every srnn_generate call does at its start) and gives every row a fresh record
 * (srnn_gen_state_fresh's, step count 0).  Controls start at their defaults (temperature 1, top_k
 * off, top_p 1), the Philox row of row b at row0 + b.  seed: the Philox key of every chunk.
 * stream: work already queued there is waited for.  Synchronises before it returns.  Returns 1
 * (nothing queued, *out = NULL) on bad arguments or an arena smaller than
 * srnn_gen_session_bytes, 2 on a HIP error.                                                   */
int srnn_gen_session_open(const SrnnModel* m, int n_seqs, int max_frames, int level,
                          uint64_t seed, int row0, int flags, void* arena, size_t arena_bytes,
                          void* stream, SrnnGenSession** out);

typedef struct SrnnGenChunk {
    int n_frames;               /* conditioning frames of this chunk, in [1, max_frames]        */
    const float* cond;          /* device (n_seqs, n_frames, cond_dim)                          */
    const float* row_bias;      /* device (n_seqs, D), or NULL: as in the previous chunk; the
                                 * first chunk must give it                                    */
    const float* temperature;   /* device (n_seqs) each, or NULL: as in the previous chunk.     */
    const int32_t* top_k;       /*   temperature / top_k need level >= 1, top_p level 2;        */
    const float* top_p;         /*   domains as srnn_generate4 states them                      */
    const int64_t* prefix;      /* device (n_seqs, prefix_cols) forced samples in [0, Q), with  */
    int prefix_cols;            /*   n_forced device (n_seqs), as srnn_generate5's n_forced; or */
    const int32_t* n_forced;    /*   both NULL: nothing is forced in this chunk.  Level >= 1,
                                 *   prefix_cols in [1, n_frames * L], n_frames * L < 2^23      */
    const int32_t* noise_row;   /* HOST (n_seqs) Philox rows, every value >= 0, or NULL: as in
                                 * the previous chunk                                          */
    const float* noise;         /* device (n_frames * L, n_seqs, Q) Exp(1) draws: given exactly
                                 * by the chunks of a SRNN_GEN_SESSION_NOISE session            */
    int64_t* seq_out;           /* (n_seqs, n_frames * L) int64 sample indices, device or pinned
                                 * host memory, or NULL                                        */
    float* logp_out;            /* (n_frames * L, n_seqs, Q) fp32 log-probs, device or pinned
                                 * host memory, or NULL; needs SRNN_GEN_SESSION_LOGP            */
} SrnnGenChunk;

/* Queues one chunk on the session's stream and returns without waiting for it: the inputs are
 * copied into the session's buffers (after the work already queued on `stream`), the rows' step
 * origins are taken on the device from their records, the blocks run from the records (the
 * first two-period and the first one-period block of a session eagerly, the second of each
 * captured, every later one a replay), the end state is packed into the records, and seq_out /
 * logp_out are written.  The caller's buffers must stay valid until srnn_gen_session_sync.
 * Returns 1, with nothing queued, where the chunk is outside the domains above, where a row's
 * step count + n_frames * L overflows the 32-bit Philox counter, or where row_bias was never
 * given; 2 on a HIP error, which poisons the session: this and every later call return 2 with
 * the first error's text and launch nothing.                                                  */
int srnn_gen_session_chunk(SrnnGenSession* s, const SrnnGenChunk* chunk, void* stream);
/* srnn_gen_session_chunk that also writes the chunk's score pairs (n_frames * L, n_seqs, 2),
 * srnn_generate7's, to score_out (device or pinned host memory), as logp_out is written.  A
 * score asked of a session opened without SRNN_GEN_SESSION_SCORE returns 1 with a message,
 * nothing queued.  A session opened with the flag has level 3 (every control and a forced prefix
 * allowed).  score_out NULL: srnn_gen_session_chunk.                                          */
int srnn_gen_session_chunk2(SrnnGenSession* s, const SrnnGenChunk* chunk, float* score_out,
                            void* stream);
/* Waits for the session's queued work; 2 (and a poisoned session) where it failed or the
 * persistent sample loop raised its error word, as srnn_generate reports it.                   */
int srnn_gen_session_sync(SrnnGenSession* s);
/* Copies the rows' records (srnn_gen_state_bytes(m, n_seqs) bytes, the layout srnn_generate5
 * reads) to `records`, device or pinned host memory, after the queued chunks; synchronises.     */
int srnn_gen_session_state_get(SrnnGenSession* s, void* records, size_t bytes);
/* Replaces the whole records of rows rows[0..n) (HOST array, distinct values in [0, n_seqs))
 * by the n records at `records` (device, 8-byte aligned, bytes = n * srnn_gen_state_bytes(m, 1),
 * else return code 1); their step counts become the rows'.  Every header is checked on the host
 * against the session's layout before anything is written (return code 1 and srnn_generate5's
 * message).  Waits for the work queued on `stream` and synchronises the session's.              */
int srnn_gen_session_state_set_rows(SrnnGenSession* s, const int32_t* rows, int n,
                                    const void* records, size_t bytes, void* stream);

typedef struct SrnnGenSessionStats {
    int64_t prepares;           /* times the tick weights were folded (1: at open)              */
    int64_t graphs_captured;    /* blocks captured and instantiated (at most 2)                 */
    int64_t graph_launches;     /* blocks run as a graph launch                                 */
    int64_t eager_blocks;       /* blocks run as plain launches                                 */
    int64_t chunks;             /* chunks queued                                                */
    int64_t steps_min, steps_max;   /* the host mirror of the rows' step counts                 */
} SrnnGenSessionStats;
/* Diagnostic counters of a session (the idiom of srnn_blaslt_calls): host values, no HIP call. */
int srnn_gen_session_stats(const SrnnGenSession* s, SrnnGenSessionStats* stats);
/* Drains the session's stream, then releases its stream, graphs and host memory (the arena is
 * the caller's again), on every path; NULL is allowed.  2 where the drain reports a HIP error. */
int srnn_gen_session_close(SrnnGenSession* s);

#ifdef __cplusplus
}
#endif
#endif

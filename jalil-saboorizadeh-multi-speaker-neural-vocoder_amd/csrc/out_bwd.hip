// Backward of the SampleLevelMLP's output layer (model.py:320-324) in ONE pass over dz and a2,
// bf16, Q = 256:
//   da2[M, D]   = bf16(dz . W_out) * [a2 > 0]          (the hidden layer's output gradient)
//   dW_out[Q,D] = dz^T . a2,   db_out[Q] = colsum(dz)   (fp32, per-row-range partials)
//   csp[M/128, D] = column sums of the stored da2 per 128-row block (the hidden bias gradient)
// The three separate passes (masked da2 GEMM, split-K dW_out GEMM, colsum of dz) each fetch dz
// and a2 again; here every row of dz and a2 is staged into LDS once and serves all of them.
//
// One persistent 512-thread workgroup (8 waves) owns a 128-column slice of D and a contiguous
// range of 64-row chunks.  The slices of one row range sit on one XCD (g3_xcd_remap), so the
// range's dz comes from HBM once and from that XCD's L2 for the other slices.  Chunks stream
// through two 48-KiB LDS slots by LDS-DMA, chunk c + 1 in flight while chunk c computes (a
// third slot, two chunks of look-ahead, measured no faster: 0.705 against 0.672 ms at M = 524288):
//   dz image [64 rows][512 B], a2 image [64 rows][256 B], 16-B slot ^ ob_swz(row): one image
//   per chunk for every use --
//     dz by rows          (ds_read_b128)         A operand of da2  (k = q)
//     dz transposed       (ds_read_b64_tr_b16)   A operand of dW   (m = q, k = rows)
//     a2 transposed       (ds_read_b64_tr_b16)   B operand of dW   (k = rows, n = columns)
//     a2 in the C layout  (ds_read_b64)          da2's ReLU mask
// da2: wave w = the chunk's 64 rows x column tile w; its W_out^T fragments (8 k-units, 32 VGPRs)
// stay in registers for the whole launch.  The MFMA runs with the operands swapped and k
// ascending in one accumulator chain, as gemm3p_kernel does: da2 comes out bit-identical to the
// masked pair-mode GEMM.  A lane adds its stored values over the 8 row tiles of a 128-row block
// (two chunks) in row order and the 16 lanes of a row meet by DPP -- the order of that GEMM's
// column-sum epilogue, so csp and the bias gradient summed from it keep their bits too.
// dW: wave (qg, nh) = 64 q x 64 columns, 16 persistent accumulator tiles, k = the range's rows
// ascending in 32-row MFMA steps: with the row ranges equal to the split-K slices of the
// dz^T . a2 GEMM this replaces (srnn_mlp_out_bwd_ranges) the partials, and their sum in range
// order by srnn_splitk_sum, are that GEMM's bit for bit.  Optionally the workgroups of slice 0
// also multiply dz^T by a fragment of ones (db_out partials).  No atomics.
#include "gemm3_core.hpp"

namespace ob {
constexpr int NT = 512, CH = 64, Q = 256, BN = 128;
constexpr int DZB = CH * Q * 2;          // 32 KiB
constexpr int A2B = CH * BN * 2;         // 16 KiB
constexpr int SLOT = DZB + A2B;
constexpr int LDS = 2 * SLOT;            // 96 KiB
constexpr int NST = 2;                   // da2 stores per wave per chunk
}  // namespace ob

struct OutBwdArgs {
    const bf16* dz;      // [M][256]
    const bf16* a2;      // [M][D]
    const bf16* wt;      // [D][256]  (W_out^T, k-contiguous)
    bf16* da2;           // [M][D]
    float* dwp;          // [R][256][D]
    float* dbp;          // [R][256]
    float* csp;          // [M / 128][D]
    int M, D, R;
};

// 16-B slot swizzle of an image row (both images; 4 row bits -> 4 slot bits, a bijection).
// Transposed reads: a 32-lane half takes rows {0-3, 8-11} (+ 4) of a 32-B column pair -- bits
// 1-3 put them on 8 distinct 32-B bank groups (bit 2 of the row is constant in one read).
// Row reads: the ds_read_b128 lane groups are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}: rows
// 4-11 of a group read the neighbouring slot (^ 1), and both r -> swz(r) and
// r -> swz(r) ^ [4 <= r < 12] are bijections, so a group's 16 lanes hit 16 distinct bank quads.
__device__ __forceinline__ int ob_swz(int r) {
    return 2 * (r & 3) | ((r >> 2) & 1) | 8 * (((r >> 2) ^ (r >> 3)) & 1);
}

// Transposed fragments (ds_read_b64_tr_b16; EXEC is all ones at every call).  LDS byte addresses of
// the two reads of the fragment of image columns f0..f0+15 over the 32 rows at `img` (row stride
// RS bytes): lane l receives column f0 + (l & 15), rows 8 (l >> 4) .. + 3 from `lo` and .. + 4
// .. + 7 from `hi`.
template <int RS>
__device__ __forceinline__ void ob_traddr(unsigned img, int f0, int lane, unsigned& lo, unsigned& hi) {
    const int h = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const int j = (f0 >> 2) + p;                       // 8-B column chunk
    const int k0 = 8 * h + q, k1 = k0 + 4;
    lo = img + k0 * RS + (((j >> 1) ^ ob_swz(k0)) * 16) + (j & 1) * 8;
    hi = img + k1 * RS + (((j >> 1) ^ ob_swz(k1)) * 16) + (j & 1) * 8;
}

typedef unsigned ob_u2 __attribute__((ext_vector_type(2)));
typedef unsigned ob_u4 __attribute__((ext_vector_type(4)));

// Four fragments by eight transposed reads, as one asm statement: through the builtin the
// compiler cannot tell these reads from the LDS-DMA writes in flight to the OTHER slot and
// drains vmcnt before each group of them (the next chunk's DMA and the da2 stores would then
// be waited for in the middle of every chunk).  The compiler does not know the reads are
// asynchronous, so every destination is tied to a wait: WAIT: the statement itself ends in
// lgkmcnt(0); !WAIT: the caller passes the eight destinations through ob_land (a wait that
// names them as "+v") before anything reads them -- the halves are assembled into fragments
// (ob_frags) only after that.
template <bool WAIT>
__device__ __forceinline__ void ob_tr4(const unsigned (&lo)[4], const unsigned (&hi)[4],
                                       ob_u2 (&l)[4], ob_u2 (&h)[4]) {
    ob_u2 l0, l1, l2, l3, h0, h1, h2, h3;
    if constexpr (WAIT) {
        asm volatile(
            "ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %9\n\t"
            "ds_read_b64_tr_b16 %2, %10\n\tds_read_b64_tr_b16 %3, %11\n\t"
            "ds_read_b64_tr_b16 %4, %12\n\tds_read_b64_tr_b16 %5, %13\n\t"
            "ds_read_b64_tr_b16 %6, %14\n\tds_read_b64_tr_b16 %7, %15\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2), "=&v"(l3), "=&v"(h3)
            : "v"(lo[0]), "v"(hi[0]), "v"(lo[1]), "v"(hi[1]), "v"(lo[2]), "v"(hi[2]), "v"(lo[3]), "v"(hi[3])
            : "memory");
    } else {
        asm volatile(
            "ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %9\n\t"
            "ds_read_b64_tr_b16 %2, %10\n\tds_read_b64_tr_b16 %3, %11\n\t"
            "ds_read_b64_tr_b16 %4, %12\n\tds_read_b64_tr_b16 %5, %13\n\t"
            "ds_read_b64_tr_b16 %6, %14\n\tds_read_b64_tr_b16 %7, %15"
            : "=&v"(l0), "=&v"(h0), "=&v"(l1), "=&v"(h1), "=&v"(l2), "=&v"(h2), "=&v"(l3), "=&v"(h3)
            : "v"(lo[0]), "v"(hi[0]), "v"(lo[1]), "v"(hi[1]), "v"(lo[2]), "v"(hi[2]), "v"(lo[3]), "v"(hi[3])
            : "memory");
    }
    l[0] = l0; l[1] = l1; l[2] = l2; l[3] = l3;
    h[0] = h0; h[1] = h1; h[2] = h2; h[3] = h3;
}

// lands the eight destinations of an ob_tr4<false>: its consumers depend on this statement
__device__ __forceinline__ void ob_land(ob_u2 (&l)[4], ob_u2 (&h)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(l[0]), "+v"(h[0]), "+v"(l[1]), "+v"(h[1]), "+v"(l[2]), "+v"(h[2]), "+v"(l[3]), "+v"(h[3])
                 :
                 : "memory");
}

__device__ __forceinline__ void ob_frags(const ob_u2 (&l)[4], const ob_u2 (&h)[4], bf16x8 (&f)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __builtin_bit_cast(bf16x8, ob_u4{l[i][0], l[i][1], h[i][0], h[i][1]});
}

__global__ __launch_bounds__(512, 1) void out_bwd_kernel(OutBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, h = lane >> 4;
    const int D = g.D;
    const int nsl = D / ob::BN;
    // unit v = (row range, slice); an XCD's workgroups take consecutive units
    const int v = g3_xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int range = v / nsl, slice = v - range * nsl;
    const int n0 = slice * ob::BN;
    // ranges are whole 128-row blocks (chunk pairs): a block's column sums stay in one wave
    const int nblk = g.M / (2 * ob::CH);
    const int cb = 2 * (int)((int64_t)range * nblk / g.R), ce = 2 * (int)((int64_t)(range + 1) * nblk / g.R);

    // dW roles: qg = 64-q group, nh = 64-column half
    const int qg = wave >> 1, nh = wave & 1;
    const bool dob = slice == 0 && g.dbp;              // db: q tiles 2 nh, 2 nh + 1 of the group

    // per-lane DMA sources (element offsets from the chunk's first row): 4 dz pieces of 2
    // rows, 2 a2 pieces of 4 rows per wave
    int zoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kr = 2 * (wave * 4 + i) + (lane >> 5);
        zoff[i] = kr * ob::Q + (((lane & 31) ^ ob_swz(kr)) * 8);
    }
    int aoff[2];                                       // (< 64 D + D: an int)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int kr = 4 * (wave * 2 + i) + (lane >> 4);
        aoff[i] = kr * D + n0 + (((lane & 15) ^ ob_swz(kr)) * 8);
    }
    auto issue = [&](int c, char* img) {
        const bf16* zb = g.dz + (int64_t)c * ob::CH * ob::Q;
        const bf16* ab = g.a2 + (int64_t)c * ob::CH * D;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds(G3_GLB(zb + zoff[i]),
                                             G3_LDS(img + (wave * 4 + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds(G3_GLB(ab + aoff[i]),
                                             G3_LDS(img + ob::DZB + (wave * 2 + i) * 1024), 16, 0, 0);
    };

    // LDS byte offsets of this lane's reads inside a slot
    // dz row fragment of k-unit 0 (row tile rt adds rt * 16 * 512; k-unit u: slot ^ 4 u, i.e.
    // offset ^ (u << 6) -- u's slot bits and h's do not overlap)
    const int zrow = r16 * 512 + ((h ^ ob_swz(r16)) * 16);
    // a2 mask (C layout) of the wave's column tile (row tile rt adds rt * 16 * 256)
    const int mrow = ob::DZB + r16 * 256 + (((wave * 2 + (h >> 1)) ^ ob_swz(r16)) * 16) + (h & 1) * 8;

    // transposed reads (slot 0, row unit 0): dz q tile i, a2 column tile j
    const unsigned lds0 = (unsigned)(uintptr_t)G3_LDS(smem);
    unsigned tza[4][2], tab[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ob_traddr<512>(lds0, (qg * 4 + i) * 16, lane, tza[i][0], tza[i][1]);
        ob_traddr<256>(lds0 + ob::DZB, (nh * 4 + i) * 16, lane, tab[i][0], tab[i][1]);
    }

    floatx4 accw[4][4];                                // dW: q tile i, column tile j
    floatx4 accb[2];                                   // db: q tile 2 nh + i (every column the same)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) accw[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
        accb[i & 1] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    float cs[4] = {0.f, 0.f, 0.f, 0.f};                // the block's column sums of the stored da2
    u16x8 ones_u;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones_u[e] = 0x3f80;
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_u);

    // after the row-tile pair's permlane16_swap lane group g holds row tile (g & 1), 8 columns
    bf16* dst0 = g.da2 + (int64_t)((h & 1) * 16 + r16) * D + n0 + wave * 16 + (h >> 1) * 8;

    issue(cb, smem);
    // (loaded under the first chunk's DMA and landed here, so that the first iteration's
    //  issue of chunk cb + 1 is not followed by a wait for them: vmcnt is in order)
    // resident W_out^T fragments of column tile `wave`: k-unit u
    bf16x8 wfr[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
        wfr[u] = *reinterpret_cast<const bf16x8*>(
            g.wt + (int64_t)(n0 + wave * 16 + r16) * ob::Q + u * 32 + h * 8);
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(wfr[0]), "+v"(wfr[1]), "+v"(wfr[2]), "+v"(wfr[3]), "+v"(wfr[4]), "+v"(wfr[5]),
                   "+v"(wfr[6]), "+v"(wfr[7])
                 :
                 : "memory");
    for (int c = cb; c < ce; ++c) {
        const int sl = (c - cb) & 1;
        const char* img = smem + sl * ob::SLOT;
        // this wave's pieces of chunk c have landed; the previous chunk's da2 stores (and, after
        // a block's second chunk, its column-sum store) are younger and stay in flight
        if (c == cb) g3_wait_vm<0>();
        else if (c & 1) g3_wait_vm<ob::NST>();
        else g3_wait_vm<ob::NST + 1>();
        __builtin_amdgcn_s_barrier();
        if (c + 1 < ce) issue(c + 1, smem + (sl ^ 1) * ob::SLOT);

        // ---- da2 chunk tile: 4 row tiles of the wave's column tile, k = q ascending
        bf16* dst = dst0 + (int64_t)c * ob::CH * D;
        unsigned pk[4][2];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
            const u16x4 mk = *reinterpret_cast<const u16x4*>(img + mrow + rt * 16 * 256);
            // all 8 k-units' fragments in flight before the first MFMA (a read waited for
            // per MFMA exposes the LDS latency 8 times per row tile)
            bf16x8 zf[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                zf[u] = *reinterpret_cast<const bf16x8*>(img + (zrow ^ (u << 6)) + rt * 16 * 512);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr[u], zf[u], acc, 0, 0, 0);
            float x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                x[e] = __uint_as_float((unsigned)mk[e] << 16) > 0.f ? acc[e] : 0.f;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                pk[rt][e] = (unsigned)__bfloat16_as_ushort(__float2bfloat16(x[2 * e])) |
                            ((unsigned)__bfloat16_as_ushort(__float2bfloat16(x[2 * e + 1])) << 16);
                cs[2 * e] += __uint_as_float(pk[rt][e] << 16);
                cs[2 * e + 1] += __uint_as_float(pk[rt][e] & 0xffff0000u);
            }
        }
        // row tiles 2 p / 2 p + 1 combined: every lane stores 8 consecutive columns of one row
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const auto r = __builtin_amdgcn_permlane16_swap(pk[2 * p2][e], pk[2 * p2 + 1][e], false, false);
                pk[2 * p2][e] = r[0];
                pk[2 * p2 + 1][e] = r[1];
            }
            *reinterpret_cast<uint4*>(dst + (int64_t)p2 * 32 * D) =
                make_uint4(pk[2 * p2][0], pk[2 * p2][1], pk[2 * p2 + 1][0], pk[2 * p2 + 1][1]);
        }
        if (c & 1) {
            // the block is complete: the 16 lanes of a DPP row meet (every lane gets the total),
            // lane r16 keeps column 4 h + (r16 & 3) (four lanes store the same value)
            float o = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x = cs[e];
                x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false));
                x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xf, 0xf, false));
                x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x122, 0xf, 0xf, false));
                x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x121, 0xf, 0xf, false));
                o = ((r16 & 3) == e) ? x : o;
                cs[e] = 0.f;
            }
            g.csp[(int64_t)(c >> 1) * D + n0 + wave * 16 + h * 4 + (r16 & 3)] = o;
        }

        // ---- dW (+ db): k = the chunk's rows, two 32-row units
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 a[4], b[4];
            // a's reads fly under b's; b's statement waits for all sixteen, and ob_land ties
            // a's destinations to a wait of their own before ob_frags reads them
            {
                const unsigned so = (unsigned)(sl * ob::SLOT);
                unsigned lo[4], hi[4];
                ob_u2 al[4], ah[4], bl[4], bh[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { lo[i] = tza[i][0] + so + u * 32 * 512; hi[i] = tza[i][1] + so + u * 32 * 512; }
                ob_tr4<false>(lo, hi, al, ah);
#pragma unroll
                for (int j = 0; j < 4; ++j) { lo[j] = tab[j][0] + so + u * 32 * 256; hi[j] = tab[j][1] + so + u * 32 * 256; }
                ob_tr4<true>(lo, hi, bl, bh);
                ob_land(al, ah);
                __builtin_amdgcn_sched_barrier(0);
                ob_frags(al, ah, a);
                ob_frags(bl, bh, b);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    accw[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], accw[i][j], 0, 0, 0);
            }
            if (dob) {
                // (static fragment indices in both arms: a select would index a[] in scratch)
                if (nh == 0) {
                    accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], ones, accb[0], 0, 0, 0);
                    accb[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], ones, accb[1], 0, 0, 0);
                } else {
                    accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], ones, accb[0], 0, 0, 0);
                    accb[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[3], ones, accb[1], 0, 0, 0);
                }
            }
        }
    }

    // ---- the range's partials: lane holds rows 4 h + e, column r16 of each dW tile
    float* wp = g.dwp + (int64_t)range * ob::Q * D + n0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                wp[(int64_t)((qg * 4 + i) * 16 + h * 4 + e) * D + (nh * 4 + j) * 16 + r16] = accw[i][j][e];
    if (dob && r16 == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                g.dbp[(int64_t)range * ob::Q + (qg * 4 + 2 * nh + i) * 16 + h * 4 + e] = accb[i][e];
    }
}

// Row ranges a launch would use (0: the shape is not served).  want > 0 asks for that many
// (clamped to the count of 128-row blocks).  want = 0: the split-K factor srnn_try_gemm3 gives
// the dz^T . a2 GEMM this replaces, when its slices are whole blocks -- dW_out then keeps that
// GEMM's bits (the training step returns what it returned before) -- else one workgroup per CU.
extern "C" int srnn_mlp_out_bwd_ranges(int dtype, int64_t M, int D, int Q, int want) {
    if (dtype != SRNN_BF16 || Q != ob::Q || D <= 0 || D % ob::BN || M <= 0 || M % 256 ||
        M > ((int64_t)1 << 30))
        return 0;
    const int nblk = (int)(M / (2 * ob::CH));
    int R = want;
    if (R <= 0 && D % 256 == 0) {
        const int ks = srnn_g3_pick_split(D / 256, (int)M);
        if (ks > 1 && M % ((int64_t)ks * 2 * ob::CH) == 0) R = ks;
    }
    if (R <= 0) {
        const int ncu = srnn_device_cus();
        R = (ncu > 0 ? ncu : 256) / (D / ob::BN);
    }
    if (R < 1) R = 1;
    if (R > nblk) R = nblk;
    return R;
}

extern "C" int srnn_mlp_out_bwd(int dtype, const void* dz, const void* a2, const void* wt, int64_t M,
                                int D, int Q, void* da2, float* dW, float* db, float* csp, int R,
                                int* taken, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (taken) *taken = 0;
    if (R <= 0 || srnn_mlp_out_bwd_ranges(dtype, M, D, Q, R) != R) return 0;
    if ((uintptr_t)dz % 16 || (uintptr_t)a2 % 16 || (uintptr_t)wt % 16 || (uintptr_t)da2 % 16 ||
        (uintptr_t)dW % 16 || (uintptr_t)db % 16 || !csp)   // (db may be null: not computed)
        return 0;
    const size_t nw = (size_t)R * ob::Q * D, nb = (size_t)R * ob::Q;
    float* part = srnn_splitk_scratch((nw + nb) * sizeof(float));
    SRNN_REQUIRE(part, "mlp_out_bwd: partials scratch allocation failed");
    OutBwdArgs g;
    g.dz = (const bf16*)dz; g.a2 = (const bf16*)a2; g.wt = (const bf16*)wt; g.da2 = (bf16*)da2;
    g.dwp = part; g.dbp = db ? part + nw : nullptr; g.csp = csp;
    g.M = (int)M; g.D = D; g.R = R;
    if (const int rc = srnn_raise_lds((const void*)out_bwd_kernel, ob::LDS)) return rc;
    hipLaunchKernelGGL(out_bwd_kernel, dim3((unsigned)(R * (D / ob::BN))), dim3(ob::NT), ob::LDS, s, g);
    SRNN_LAUNCH_CHECK();
    if (const int rc = srnn_splitk_sum(g.dwp, dW, D, ob::Q, D, R, s)) return rc;
    if (db)
        if (const int rc = srnn_splitk_sum(g.dbp, db, ob::Q, 1, ob::Q, R, s)) return rc;
    if (taken) *taken = 1;
    return 0;
}

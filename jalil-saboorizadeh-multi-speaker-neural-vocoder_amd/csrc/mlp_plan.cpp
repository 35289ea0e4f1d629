// The sample-level MLP's plans (mlp_plan.hpp) and the C entries that report them.  Host code
// only: nothing here calls HIP but srnn_mlp_dtab_plan's question to the device.
#include <algorithm>

#include "mlp_plan.hpp"
#include "samplernn_hip_internal.hpp"

DtabSwitches DtabSwitches::read() {
    const char* pd = getenv("SRNN_DTAB_PD");
    const bool pd_set = pd && pd[0];
    return {!env_off("SRNN_DTAB_PACK"), !env_off("SRNN_DTAB_POS"), !env_off("SRNN_DTAB_X8"),
            !env_off("SRNN_DTAB_BLK"), pd_set, pd_set ? atoi(pd) : 0};
}

// Order: packed, position-major (direct when every workgroup takes all rows of its 4 columns,
// else through the int64 workspace), generic, empty.
DtabPlan dtab_plan(const DtabProblem& p, bool packed_ok, const DtabSwitches& sw) {
    DtabPlan pl = {};
    pl.work_bytes = dtab_work_bytes(p);
    const int64_t nrows = (int64_t)p.B * p.Tlen;
    const bool whole = cdiv(p.D, 4) >= 192;
    const bool pos_fits = p.FS0 == 16 && pos_lds_bytes(p.Q, p.Tlen) <= MLP_LDS_MAX && nrows > 0;
    // packed: bf16 in and out; its kernel writes nothing when the histogram is too skewed for
    // its scale and leaves dTab to the gated exact form, so it is taken only where that fits too
    if (pos_fits && whole && p.dtype == SRNN_BF16 && p.out_dtype == SRNN_BF16 && p.Q == 256 &&
        p.D % 8 == 0 && p.ldda % 8 == 0 && pk_lds_bytes(p.Q, p.Tlen) <= MLP_LDS_MAX &&
        p.work_bytes >= DTAB_STAT_BYTES && sw.pack && packed_ok) {
        pl.route = SRNN_DTAB_PACKED;
        // da prefetch depth (SRNN_DTAB_PD = 1 / 2, anything else 4), measured per B on one box
        // (profiles/r05_dtab_rowmajor_perm_ab.txt): two ahead up to B = 256, one ahead at
        // B = 512 (1.20 vs 1.29 / 1.32 ms; deeper prefetch there is slower, not faster)
        const int pd = sw.pd_set ? sw.pd : (p.B >= 384 ? 1 : 2);
        pl.pd = pd == 1 || pd == 2 ? pd : 4;
        pl.x8 = sw.x8 && p.work_bytes >= DTAB_X8_OFF + (size_t)p.B * dtab_wp8(p.Tlen);
        pl.use_blk = p.blk && sw.blk;
        // amax_in: max |da| already measured by the GEMM that wrote da (SrnnGemmEpilogue.amax):
        // the prep pass only counts the sample values
        pl.nb_da = p.amax_in ? 0 : (int)std::min<int64_t>(1024, std::max<int64_t>(1, nrows / 64));
        pl.colsum = true;
    } else if (pos_fits && sw.pos) {
        pl.route = whole ? SRNN_DTAB_DIRECT : SRNN_DTAB_POSWS;
        pl.colsum = whole;
    } else if (nrows > 0) {
        pl.route = SRNN_DTAB_GENERIC;
        const int W = p.Tlen + p.FS0 - 1;
        auto fits = [&](int cw) {
            return p.Q * p.FS0 * cw * 8 + W <= MLP_LDS_MAX && p.FS0 * cw <= DTAB_NT;
        };
        pl.cw = 4;
        while (pl.cw > 1 && !fits(pl.cw)) pl.cw /= 2;
        if (!fits(pl.cw)) pl.cw = 0;
    } else {
        pl.route = SRNN_DTAB_EMPTY;
    }
    return pl;
}

bool l1_lds_switch() { return env_flag("SRNN_L1_LDS", 1) != 0; }

// Order: LDS-resident table slice, XCD-sliced, generic.
L1Plan l1_plan(const L1Problem& p, bool lds_switch) {
    L1Plan pl = {};
    const int es = p.dtype == SRNN_F32 ? 4 : 2, ue = p.upper_dtype == SRNN_F32 ? 4 : 2;
    const int64_t nrows = (int64_t)p.B * p.Tlen;
    auto al16 = [](const void* q) { return (uintptr_t)q % 16 == 0; };
    // both row-sliced kernels: many rows, 16-byte loads and stores of upper / out / tab rows
    const bool sliced = !p.base && nrows >= 4096 && (p.ldu * ue) % 16 == 0 && al16(p.upper) &&
                        (p.ldo * es) % 16 == 0 && al16(p.out) && al16(p.tab);
    const int WP = l1_wp(p.Tlen, p.FS0), ncg = p.D / 16;
    if (sliced && es == 2 && ue == 2 && p.FS0 == 16 && p.Q == 256 && p.D % 16 == 0 &&
        ncg >= 1 && ncg <= 256 && l1_lds_bytes(p.Tlen, p.FS0) <= MLP_LDS_MAX && p.Tlen <= 4 * (L1L_NT / 2) &&
        WP <= 2 * L1L_NT && lds_switch) {
        pl.route = SRNN_L1_LDS;
        const int nrc = std::max(1, std::min(p.B, 256 / ncg));
        pl.bpc = (p.B + nrc - 1) / nrc;
        pl.nrc2 = (p.B + pl.bpc - 1) / pl.bpc;
        pl.rpt = (p.Tlen + L1L_NT / 2 - 1) / (L1L_NT / 2) <= 2 ? 2 : 4;
    } else {
        pl.route = sliced && p.D % 128 == 0 ? SRNN_L1_XCD : SRNN_L1_GENERIC;
        pl.bits_pass = p.bits != nullptr;   // (the LDS kernel writes the mask bits itself)
    }
    return pl;
}

extern "C" {

int srnn_mlp_dtab_plan_for(int dtype, int out_dtype, int B, int Tlen, int D, int FS0, int Q,
                           int64_t ldda, int have_amax, int have_blk, size_t work_bytes,
                           int packed_ok, int* route, int* cw, int* pd, int* x8, int* use_blk,
                           int* colsum, size_t* need_bytes) {
    SRNN_REQUIRE(route && cw && pd && x8 && use_blk && colsum && need_bytes,
                 "mlp_dtab_plan: null result pointer");
    static const unsigned given = 0;   // an address for "amax_in / blk given": never read
    DtabProblem p;
    p.dtype = dtype; p.out_dtype = out_dtype;
    p.B = B; p.Tlen = Tlen; p.D = D; p.FS0 = FS0; p.Q = Q;
    p.ldda = ldda; p.work_bytes = work_bytes;
    p.amax_in = have_amax ? &given : nullptr;
    p.blk = have_blk ? &given : nullptr;
    const DtabPlan pl = dtab_plan(p, packed_ok != 0, DtabSwitches::read());
    *route = pl.route; *cw = pl.cw; *pd = pl.pd; *x8 = pl.x8; *use_blk = pl.use_blk;
    *colsum = pl.colsum; *need_bytes = pl.work_bytes;
    return 0;
}

int srnn_mlp_dtab_plan(int dtype, int out_dtype, int B, int Tlen, int D, int FS0, int Q,
                       int64_t ldda, int have_amax, int have_blk, size_t work_bytes, int* route,
                       int* cw, int* pd, int* x8, int* use_blk, int* colsum, size_t* need_bytes) {
    return srnn_mlp_dtab_plan_for(dtype, out_dtype, B, Tlen, D, FS0, Q, ldda, have_amax, have_blk,
                                  work_bytes, srnn_dtab_packed_ok(), route, cw, pd, x8, use_blk,
                                  colsum, need_bytes);
}

int srnn_mlp_l1_plan_for(int dtype, int upper_dtype, int B, int Tlen, int D, int FS0, int Q,
                         const void* tab, const void* upper, int64_t ldu, const void* out,
                         int64_t ldo, int have_base, int have_bits, int* route, int* bits_pass) {
    SRNN_REQUIRE(route && bits_pass, "mlp_l1_plan: null result pointer");
    static int given_base = 0;         // addresses for "base / bits given": never read
    static unsigned short given_bits = 0;
    L1Problem p;
    p.dtype = dtype; p.upper_dtype = upper_dtype;
    p.B = B; p.Tlen = Tlen; p.D = D; p.FS0 = FS0; p.Q = Q;
    p.tab = tab; p.upper = upper; p.ldu = ldu; p.out = const_cast<void*>(out); p.ldo = ldo;
    p.base = have_base ? &given_base : nullptr;
    p.bits = have_bits ? &given_bits : nullptr;
    const L1Plan pl = l1_plan(p, l1_lds_switch());
    *route = pl.route; *bits_pass = pl.bits_pass;
    return 0;
}

}  // extern "C"

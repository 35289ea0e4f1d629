// The sample-level MLP's two dispatched operations as every entry sees them: one record per
// operation that the C entries fill (dtab.hip, mlp.hip, generate.hip), and one plan per
// record that names the route and sizes its work (mlp_plan.cpp).  The plans are pure functions
// of their arguments and the only place a route is chosen; the drivers and the Python side
// both ask them.
#pragma once
#include "common.hpp"
#include "samplernn_hip.h"

constexpr int MLP_LDS_MAX = 160 * 1024;  // dynamic LDS a workgroup of these kernels may ask for

// ---- dTab scatter: dTab[x[b, xoff + t + k]][k][:] += da[b, t, :]  (srnn_mlp_dtab4)
constexpr int DTAB_NT = 1024;            // threads of a scatter workgroup
constexpr size_t DTAB_STAT_BYTES = 1040; // sizeof(DtabStat), the packed form's statistics (dtab.hip)
constexpr size_t DTAB_X8_OFF = (DTAB_STAT_BYTES + 255) & ~(size_t)255;  // byte windows, in work

struct DtabProblem {
    int dtype = SRNN_BF16, out_dtype = SRNN_BF16;
    int B = 0, Tlen = 0, D = 0, FS0 = 0, Q = 0;
    const void* da = nullptr;  // (B Tlen, D), rows ldda apart
    int64_t ldda = 0;
    const int64_t* x = nullptr;  // row b's window starts at x + b * ldx + xoff
    int64_t ldx = 0;
    int xoff = 0;
    void* dtab_out = nullptr;  // (Q, FS0, D) in out_dtype
    void* work = nullptr;
    size_t work_bytes = 0;
    float* colsum = nullptr;            // optional (FS0, D) sums of da rows t = j (mod FS0)
    const unsigned* amax_in = nullptr;  // optional max |da| as float bits
    const void* blk = nullptr;          // optional column-blocked copy of da
};

struct DtabSwitches {
    bool pack, pos, x8, blk;  // SRNN_DTAB_PACK / _POS / _X8 / _BLK: off when they start with '0'
    bool pd_set;              // SRNN_DTAB_PD given (and not empty) ...
    int pd;                   // ... and its integer value
    static DtabSwitches read();  // per call
};

struct DtabPlan {
    int route;      // SrnnDtabRoute
    int cw;         // generic: columns per workgroup, 4 / 2 / 1 (0: FS0 too large for any)
    int pd;         // packed: prefetch depth in batches, 1 / 2 / 4
    bool x8;        // packed: the prep pass writes the windows as bytes into work
    bool use_blk;   // packed: da is read from blk
    int nb_da;      // packed: blocks of the prep pass that measure max |da| (0 with amax_in)
    bool colsum;    // the route writes colsum (when the caller passes one)
    size_t work_bytes;  // what the call requires of work
};

// bytes of work a call requires: the int64 accumulator, on every route
static inline size_t dtab_work_bytes(const DtabProblem& p) {
    return (size_t)((int64_t)p.Q * p.FS0 * p.D) * 8;
}
// dynamic LDS of the position-major and the packed kernels (FS0 = 16; 16 waves' index strips)
static inline int dtab_strip_bytes(int Tlen) { return (Tlen + 15 + 31) & ~15; }
static inline int pos_lds_bytes(int Q, int Tlen) {
    return Q * 16 * 4 * 8 + 4 * 16 * 8 + (DTAB_NT / 64) * dtab_strip_bytes(Tlen);
}
static inline int pk_lds_bytes(int Q, int Tlen) {
    return Q * 2 * 16 * 8 + 4 * 16 * 8 + 16 + (DTAB_NT / 64) * 2 * dtab_strip_bytes(Tlen);
}
// row pitch of the packed form's byte windows (FS0 = 16)
static inline int dtab_wp8(int Tlen) { return (Tlen + 15 + 15) & ~15; }

// packed_ok: the device fact srnn_dtab_packed_ok(), supplied by the entry
DtabPlan dtab_plan(const DtabProblem& p, bool packed_ok, const DtabSwitches& sw);

// ---- L1 gather: out[b Tlen + t] = relu(upper[b Tlen + t] + sum_k tab[k][x[b, xoff + t + k]])
constexpr int L1L_NT = 1024;             // threads of an LDS-resident gather workgroup

struct L1Problem {
    int dtype = SRNN_BF16, upper_dtype = SRNN_BF16;  // of tab / out, of upper
    int B = 0, Tlen = 0, D = 0, FS0 = 0, Q = 0;
    const void* tab = nullptr;  // (FS0, Q, D)
    const int64_t* x = nullptr;
    int64_t ldx = 0;
    int xoff = 0;
    const int* base = nullptr;  // optional device offset added to xoff (generation)
    const void* upper = nullptr;
    int64_t ldu = 0;
    void* out = nullptr;
    int64_t ldo = 0;
    unsigned short* bits = nullptr;  // optional ReLU mask of out (bf16 / bf16 only)
    int64_t ldb = 0;
};

struct L1Plan {
    int route;       // SrnnL1Route
    int nrc2, bpc;   // lds: chunks of batch rows and batch rows per chunk
    int rpt;         // lds: the mlp_l1_lds_kernel<2> or <4> instantiation
    bool bits_pass;  // a separate srnn_relu_bits pass over out follows
};

static inline int l1_wp(int Tlen, int FS0) { return (Tlen + FS0 - 1 + 4 + 15) & ~15; }
// dynamic LDS of the LDS-resident gather: its 16 x 256 x 16 table slice and two index rows
static inline int l1_lds_bytes(int Tlen, int FS0) { return 16 * 256 * 32 + 2 * l1_wp(Tlen, FS0); }

// lds_switch: SRNN_L1_LDS (default on), read per call.  Looks at the pointers' low bits only.
bool l1_lds_switch();
L1Plan l1_plan(const L1Problem& p, bool lds_switch);
int l1_run(const L1Problem& p, hipStream_t s);  // mlp.hip

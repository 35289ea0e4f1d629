// One GRU layer over a whole sequence (torch.nn.GRU recurrence, model.py:148-165 / 244), as
// every back end sees it: a forward and a backward record built by the C entries
// (gru_layer.cpp), a plan that names the back end for a shape, and three back ends per
// direction -- the XCD-grouped persistent sweeps (gru_xcd.hip), the LDS-resident sweeps
// (gru_seq.hip) and one cell launch per step (gru.hip's kernels, gru_layer.cpp's loops).
#pragma once
#include "common.hpp"
#include "samplernn_hip.h"

// Operand x[b][t] = x + b * ld + t * s (elements).  ncu / share: the device's CUs and the
// processes running persistent grids on it at once (persist.hip), as the plan was given them.
struct GruLayerFwd {
    int dtype = SRNN_BF16, B = 0, D = 0, Fr = 0;
    int ncu = 0, share = 1;
    const float* gi = nullptr;  // x . W_ih^T + b_ih (3D per row and step)
    int64_t ldgi = 0, sgi = 0;
    const float* h0 = nullptr;  // (B, D) initial state
    const void* h0_lp = nullptr;  // its `dtype` copy: h0 itself in fp32, else written by the driver
    const void* whh = nullptr;  // (3D, D)
    const float* bhh = nullptr;
    float* out = nullptr;
    void* out_lp = nullptr;  // `dtype` copy of out (bf16 only)
    int64_t ldo = 0, so = 0;
    float* gates = nullptr;  // r|z|n|ghn (4D per row and step)
    int64_t ldg = 0, sg = 0;
    void* hprev_lp = nullptr;  // optional [h0, out[:, :Fr-1]] in out_lp's layout (XCD only)
    void* work = nullptr;
    size_t work_bytes = 0;

    int es() const { return dtype == SRNN_F32 ? 4 : 2; }
    // the sub-record of rows c .. c+n-1 (same work area)
    GruLayerFwd rows(int c, int n) const {
        GruLayerFwd r = *this;
        r.B = n;
        r.gi += c * ldgi;
        r.h0 += (int64_t)c * D;
        if (h0_lp) r.h0_lp = (const char*)h0_lp + (int64_t)c * D * es();
        r.out += c * ldo;
        if (out_lp) r.out_lp = (char*)out_lp + c * ldo * es();
        r.gates += c * ldg;
        if (hprev_lp) r.hprev_lp = (char*)hprev_lp + c * ldo * es();
        return r;
    }
};

struct GruLayerBwd {
    int dtype = SRNN_BF16, B = 0, D = 0, Fr = 0;
    int ncu = 0, share = 1;
    const float* dy = nullptr;
    int64_t lddy = 0, sdy = 0;
    const float* gates = nullptr;  // the forward's
    int64_t ldg = 0, sg = 0;
    const float* hout = nullptr;  // the forward's out
    int64_t ldo = 0, so = 0;
    const float* h0 = nullptr;
    const void* whh = nullptr;    // (3D, D): the step kernels' plain form
    const void* whh_t = nullptr;  // (D, 3D)
    // outputs, 3D per row and step, one layout: dgh / dgi fp32, dgh_lp / dgi_lp in `dtype`;
    // which are required and which optional is each back end's (samplernn_hip.h)
    float* dgh = nullptr;
    void* dgh_lp = nullptr;
    float* dgi = nullptr;
    void* dgi_lp = nullptr;
    float* bsum = nullptr;  // (B, 4D) sums over t of [dar | daz | dghn | dan] (XCD only)
    int64_t ldd = 0, sd = 0;
    float* ddir0 = nullptr;  // (B, D) dh_direct of step 0
    void* work = nullptr;
    size_t work_bytes = 0;

    int es() const { return dtype == SRNN_F32 ? 4 : 2; }
    GruLayerBwd rows(int c, int n) const {
        GruLayerBwd r = *this;
        r.B = n;
        r.dy += c * lddy;
        r.gates += c * ldg;
        r.hout += c * ldo;
        r.h0 += (int64_t)c * D;
        if (dgh) r.dgh += c * ldd;
        if (dgh_lp) r.dgh_lp = (char*)dgh_lp + c * ldd * es();
        if (dgi) r.dgi += c * ldd;
        if (dgi_lp) r.dgi_lp = (char*)dgi_lp + c * ldd * es();
        if (bsum) r.bsum += (int64_t)c * 4 * D;
        r.ddir0 += (int64_t)c * D;
        return r;
    }
};

// ---- the plan: which back end runs (dtype, B, D) and the work bytes of either direction.
// A pure function of its arguments and the only place the choice is made; the driver and
// the Python side both ask it.  Order: XCD, seq, steps; fp32 always takes steps.
struct GruSwitches {
    bool xcd, seq;  // SRNN_GRU_XCD / SRNN_GRU_SEQ (default on), read per call
    static GruSwitches read();
};

struct GruPlan {
    int backend;  // SrnnGruBackend
    size_t fwd_work_bytes, bwd_work_bytes;
};
GruPlan gru_layer_plan(int dtype, int B, int D, int ncu, int share, const GruSwitches& sw);

// Work layout of a layer call: the back end's own area first (gru_*_area: 0 = the back end
// does not take the shape), then from the next 256-byte boundary the driver's sub-buffer --
// forward: the bf16 copy of h0 (seq and bf16 steps), backward: the steps' second ddir buffer.
size_t gru_xcd_fwd_area(int dtype, int B, int D, int ncu, int share);  // gru_xcd.hip
size_t gru_xcd_bwd_area(int dtype, int B, int D, int ncu, int share);
size_t gru_seq_area(int dtype, int B, int D, int ncu, int share);      // gru_seq.hip, both directions
static inline size_t gru_al256(size_t n) { return (n + 255) / 256 * 256; }

// The back ends: -1 not taken, 0 done, > 0 error.  Each keeps its own eligibility tests at
// the top and fills its kernel argument block from the record.
int gru_try_xcd_fwd(const GruLayerFwd& p, hipStream_t s);  // gru_xcd.hip
int gru_try_xcd_bwd(const GruLayerBwd& p, hipStream_t s);
int gru_try_seq_fwd(const GruLayerFwd& p, hipStream_t s);  // gru_seq.hip
int gru_try_seq_bwd(const GruLayerBwd& p, hipStream_t s);
int gru_steps_fwd(const GruLayerFwd& p, hipStream_t s);    // gru_layer.cpp: always take
int gru_steps_bwd(const GruLayerBwd& p, hipStream_t s);

// the plan's back end on the record (writes the driver's sub-buffer first)
int gru_layer_fwd(const GruLayerFwd& p, hipStream_t s);
int gru_layer_bwd(const GruLayerBwd& p, hipStream_t s);

// gru.hip: one step with gi given / with gh given and x . W_ih^T computed (generate.hip)
int srnn_gru_cell_impl(int dtype, int B, int D, int Din, const void* x, int64_t ldx,
                       const void* wih, const float* bih, const float* gi, int64_t ldgi,
                       const void* h, int64_t ldh, const float* hf, int64_t ldhf, const void* whh,
                       const float* bhh, float* hout, int64_t ldho, void* hout_lp, int64_t ldhl,
                       float* gates, int64_t ldgt, hipStream_t s);
int srnn_gru_cell_x_impl(int dtype, int B, int D, int Din, const void* x, int64_t ldx,
                         const void* wih, const float* bih, const float* gadd, int64_t ldgadd,
                         const float* gh, int64_t ldgh, const float* hf, int64_t ldhf, float* hout,
                         int64_t ldho, void* hout_lp, int64_t ldhl, hipStream_t s);

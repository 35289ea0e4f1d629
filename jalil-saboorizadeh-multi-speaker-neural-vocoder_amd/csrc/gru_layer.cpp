// GRU layer driver (gru_layer.hpp): the plan, the step back ends, the driver and every C
// entry of the recurrence that takes a whole sequence.  Host code only: the entries fill a
// record, the back ends (gru_xcd.hip, gru_seq.hip, the loops here) launch.
#include "gru_layer.hpp"
#include "samplernn_hip_internal.hpp"

GruSwitches GruSwitches::read() {
    return {env_flag("SRNN_GRU_XCD", 1) != 0, env_flag("SRNN_GRU_SEQ", 1) != 0};
}

// bytes of the driver's sub-buffers: the bf16 copy of h0 and the steps' second ddir
static size_t h0_copy_bytes(int dtype, int B, int D) {
    return dtype == SRNN_F32 ? 0 : (size_t)B * D * 2;
}
static size_t ddir_bytes(int B, int D) { return (size_t)B * D * 4; }

GruPlan gru_layer_plan(int dtype, int B, int D, int ncu, int share, const GruSwitches& sw) {
    if (B <= 0 || D <= 0) return {SRNN_GRU_STEPS, 0, 0};
    const size_t h0c = h0_copy_bytes(dtype, B, D);
    if (sw.xcd)
        if (const size_t f = gru_xcd_fwd_area(dtype, B, D, ncu, share))
            return {SRNN_GRU_XCD, f, gru_xcd_bwd_area(dtype, B, D, ncu, share)};
    if (sw.seq)
        if (const size_t a = gru_seq_area(dtype, B, D, ncu, share))
            return {SRNN_GRU_SEQ, gru_al256(a) + h0c, a};
    return {SRNN_GRU_STEPS, h0c, ddir_bytes(B, D)};
}

static inline void* at(const void* p, int64_t elems, int es) { return (char*)p + elems * es; }

// ---- the step back ends: one cell launch per step, reading the previous step's output
int gru_steps_fwd(const GruLayerFwd& p, hipStream_t s) {
    const bool lp = p.dtype != SRNN_F32;
    SRNN_REQUIRE(p.h0_lp && (!lp || p.out_lp) && !p.hprev_lp,
                 "gru_steps: needs h0_lp (and out_lp in bf16), writes no hprev_lp");
    for (int t = 0; t < p.Fr; ++t) {
        const float* hf = t ? p.out + (t - 1) * p.so : p.h0;
        const void* h = !t ? p.h0_lp : lp ? at(p.out_lp, (t - 1) * p.so, 2) : hf;
        const int64_t ldh = t ? p.ldo : p.D;
        if (const int rc = srnn_gru_cell_impl(
                p.dtype, p.B, p.D, p.D, nullptr, 0, nullptr, nullptr, p.gi + t * p.sgi, p.ldgi, h,
                ldh, hf, ldh, p.whh, p.bhh, p.out + t * p.so, p.ldo,
                lp ? at(p.out_lp, t * p.so, 2) : nullptr, p.ldo, p.gates + t * p.sg, p.ldg, s))
            return rc;
    }
    return 0;
}

// (dh_direct alternates between the caller's ddir0 -- even steps, so step 0 -- and work)
int gru_steps_bwd(const GruLayerBwd& p, hipStream_t s) {
    const bool lp = p.dtype != SRNN_F32;
    SRNN_REQUIRE(p.dgh && p.dgi && (!lp || p.dgh_lp) && !p.dgi_lp && !p.bsum,
                 "gru_steps_bwd: writes dgh, dgi (and dgh_lp in bf16), no dgi_lp / bsum");
    SRNN_REQUIRE(p.work && p.work_bytes >= ddir_bytes(p.B, p.D), "gru_steps_bwd: workspace");
    float* ddir[2] = {p.ddir0, (float*)p.work};
    for (int t = p.Fr - 1; t >= 0; --t) {
        const bool nxt = t + 1 < p.Fr;
        const void* dgn = lp ? at(p.dgh_lp, (t + 1) * p.sd, 2) : p.dgh + (t + 1) * p.sd;
        if (const int rc = srnn_gru_cell_bwd(
                p.dtype, p.B, p.D, p.dy + t * p.sdy, p.lddy, nxt ? dgn : nullptr, p.ldd,
                nxt ? ddir[(t + 1) % 2] : nullptr, p.whh, p.whh_t, p.gates + t * p.sg, p.ldg,
                t ? p.hout + (t - 1) * p.so : p.h0, t ? p.ldo : p.D, p.dgh + t * p.sd, p.ldd,
                lp ? at(p.dgh_lp, t * p.sd, 2) : nullptr, p.ldd, p.dgi + t * p.sd, p.ldd,
                ddir[t % 2], (void*)s))
            return rc;
    }
    return 0;
}

// ---- the driver
int gru_layer_fwd(const GruLayerFwd& p, hipStream_t s) {
    SRNN_REQUIRE(p.B > 0 && p.D > 0, "gru_layer_fwd: bad sizes");
    const GruPlan pl = gru_layer_plan(p.dtype, p.B, p.D, p.ncu, p.share, GruSwitches::read());
    SRNN_REQUIRE(!pl.fwd_work_bytes || (p.work && p.work_bytes >= pl.fwd_work_bytes),
                 "gru_layer_fwd: workspace %zu < %zu", p.work_bytes, pl.fwd_work_bytes);
    GruLayerFwd q = p;
    if (pl.backend != SRNN_GRU_XCD) {   // (the XCD sweep reads the fp32 state itself)
        const size_t h0c = h0_copy_bytes(p.dtype, p.B, p.D);
        // fp32: h0 serves as both; bf16: a copy in the tail of the work area
        q.h0_lp = h0c ? (char*)p.work + (pl.fwd_work_bytes - h0c) : (const void*)p.h0;
        if (h0c)
            if (const int rc = srnn_copy2d(SRNN_F32, p.dtype, p.B, p.D, p.h0, p.D,
                                           (void*)q.h0_lp, p.D, (void*)s))
                return rc;
    }
    const int rc = pl.backend == SRNN_GRU_XCD   ? gru_try_xcd_fwd(q, s)
                   : pl.backend == SRNN_GRU_SEQ ? gru_try_seq_fwd(q, s)
                                                : gru_steps_fwd(q, s);
    SRNN_REQUIRE(rc >= 0, "gru_layer_fwd: the planned back end %d declined", pl.backend);
    return rc;
}

int gru_layer_bwd(const GruLayerBwd& p, hipStream_t s) {
    SRNN_REQUIRE(p.B > 0 && p.D > 0, "gru_layer_bwd: bad sizes");
    const GruPlan pl = gru_layer_plan(p.dtype, p.B, p.D, p.ncu, p.share, GruSwitches::read());
    const int rc = pl.backend == SRNN_GRU_XCD   ? gru_try_xcd_bwd(p, s)
                   : pl.backend == SRNN_GRU_SEQ ? gru_try_seq_bwd(p, s)
                                                : gru_steps_bwd(p, s);
    SRNN_REQUIRE(rc >= 0, "gru_layer_bwd: the planned back end %d declined", pl.backend);
    return rc;
}

// ---- C entries (samplernn_hip.h): positional arguments into a record
static GruLayerFwd fwd_record(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi,
                              int64_t sgi, const float* h0, const void* h0_lp, const void* whh,
                              const float* bhh, float* out, void* out_lp, int64_t ldo, int64_t so,
                              float* gates, int64_t ldg, int64_t sg, void* hprev_lp, void* work,
                              size_t work_bytes) {
    GruLayerFwd p;
    p.dtype = dtype; p.B = B; p.D = D; p.Fr = Fr;
    p.ncu = srnn_device_cus(); p.share = srnn_device_share();
    p.gi = gi; p.ldgi = ldgi; p.sgi = sgi;
    p.h0 = h0; p.h0_lp = h0_lp; p.whh = whh; p.bhh = bhh;
    p.out = out; p.out_lp = out_lp; p.ldo = ldo; p.so = so;
    p.gates = gates; p.ldg = ldg; p.sg = sg;
    p.hprev_lp = hprev_lp; p.work = work; p.work_bytes = work_bytes;
    return p;
}

static GruLayerBwd bwd_record(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy,
                              int64_t sdy, const float* gates, int64_t ldg, int64_t sg,
                              const float* hout, int64_t ldo, int64_t so, const float* h0,
                              const void* whh, const void* whh_t, float* dgh, void* dgh_lp,
                              float* dgi, void* dgi_lp, float* bsum, int64_t ldd, int64_t sd,
                              float* ddir0, void* work, size_t work_bytes) {
    GruLayerBwd p;
    p.dtype = dtype; p.B = B; p.D = D; p.Fr = Fr;
    p.ncu = srnn_device_cus(); p.share = srnn_device_share();
    p.dy = dy; p.lddy = lddy; p.sdy = sdy;
    p.gates = gates; p.ldg = ldg; p.sg = sg;
    p.hout = hout; p.ldo = ldo; p.so = so; p.h0 = h0;
    p.whh = whh; p.whh_t = whh_t;
    p.dgh = dgh; p.dgh_lp = dgh_lp; p.dgi = dgi; p.dgi_lp = dgi_lp; p.bsum = bsum;
    p.ldd = ldd; p.sd = sd; p.ddir0 = ddir0; p.work = work; p.work_bytes = work_bytes;
    return p;
}

// a forced form's result: its one back end must take the call
static int forced(int rc, const char* what) {
    SRNN_REQUIRE(rc >= 0, "%s: shape/device not supported", what);
    return rc;
}

extern "C" {

int srnn_gru_layer_plan_for(int dtype, int B, int D, int ncu, int share, int* backend,
                            size_t* fwd_bytes, size_t* bwd_bytes) {
    SRNN_REQUIRE(backend && fwd_bytes && bwd_bytes, "gru_layer_plan: null result pointer");
    const GruPlan pl = gru_layer_plan(dtype, B, D, ncu, share, GruSwitches::read());
    *backend = pl.backend; *fwd_bytes = pl.fwd_work_bytes; *bwd_bytes = pl.bwd_work_bytes;
    return 0;
}

int srnn_gru_layer_plan(int dtype, int B, int D, int* backend, size_t* fwd_bytes,
                        size_t* bwd_bytes) {
    return srnn_gru_layer_plan_for(dtype, B, D, srnn_device_cus(), srnn_device_share(), backend,
                                   fwd_bytes, bwd_bytes);
}

int srnn_gru_layer_fwd(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                       const float* h0, const void* whh, const float* bhh, float* out,
                       void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                       int64_t sg, void* hprev_lp, void* work, size_t work_bytes, void* stream) {
    return gru_layer_fwd(fwd_record(dtype, B, D, Fr, gi, ldgi, sgi, h0, nullptr, whh, bhh, out,
                                    out_lp, ldo, so, gates, ldg, sg, hprev_lp, work, work_bytes),
                         (hipStream_t)stream);
}

int srnn_gru_layer_bwd(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                       const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                       int64_t so, const float* h0, const void* whh, const void* whh_t, float* dgh,
                       void* dgh_lp, float* dgi, void* dgi_lp, float* bsum, int64_t ldd,
                       int64_t sd, float* ddir0, void* work, size_t work_bytes, void* stream) {
    return gru_layer_bwd(bwd_record(dtype, B, D, Fr, dy, lddy, sdy, gates, ldg, sg, hout, ldo, so,
                                    h0, whh, whh_t, dgh, dgh_lp, dgi, dgi_lp, bsum, ldd, sd, ddir0,
                                    work, work_bytes),
                         (hipStream_t)stream);
}

// ---- the forced forms: one back end, whatever the plan would say; the three queries answer
// for their back end alone and 0 when its switch is off
int srnn_gru_seq_supported(int dtype, int B, int D) {
    return GruSwitches::read().seq &&
           gru_seq_area(dtype, B, D, srnn_device_cus(), srnn_device_share());
}

size_t srnn_gru_xcd_work_bytes(int dtype, int B, int D) {
    if (!GruSwitches::read().xcd) return 0;
    return gru_xcd_fwd_area(dtype, B, D, srnn_device_cus(), srnn_device_share());
}

size_t srnn_gru_xcd_bwd_work_bytes(int dtype, int B, int D) {
    if (!GruSwitches::read().xcd) return 0;
    return gru_xcd_bwd_area(dtype, B, D, srnn_device_cus(), srnn_device_share());
}

int srnn_gru_seq_fwd(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                     const float* h0, const void* h0_lp, const void* whh, const float* bhh,
                     float* out, void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                     int64_t sg, int* work, size_t work_bytes, void* stream) {
    return forced(gru_try_seq_fwd(fwd_record(dtype, B, D, Fr, gi, ldgi, sgi, h0, h0_lp, whh, bhh,
                                             out, out_lp, ldo, so, gates, ldg, sg, nullptr, work,
                                             work_bytes),
                                  (hipStream_t)stream),
                  "gru_seq");
}

int srnn_gru_seq_bwd(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                     const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                     int64_t so, const float* h0, const void* whh_t, float* dgh, void* dgh_lp,
                     float* dgi, int64_t ldd, int64_t sd, float* ddir0, int* work,
                     size_t work_bytes, void* stream) {
    return forced(gru_try_seq_bwd(bwd_record(dtype, B, D, Fr, dy, lddy, sdy, gates, ldg, sg, hout,
                                             ldo, so, h0, nullptr, whh_t, dgh, dgh_lp, dgi,
                                             nullptr, nullptr, ldd, sd, ddir0, work, work_bytes),
                                  (hipStream_t)stream),
                  "gru_seq");
}

int srnn_gru_xcd_fwd2(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                      const float* h0, const void* whh, const float* bhh, float* out,
                      void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                      int64_t sg, void* hprev_lp, void* work, size_t work_bytes, void* stream) {
    return forced(gru_try_xcd_fwd(fwd_record(dtype, B, D, Fr, gi, ldgi, sgi, h0, nullptr, whh, bhh,
                                             out, out_lp, ldo, so, gates, ldg, sg, hprev_lp, work,
                                             work_bytes),
                                  (hipStream_t)stream),
                  "gru_xcd");
}

int srnn_gru_xcd_fwd(int dtype, int B, int D, int Fr, const float* gi, int64_t ldgi, int64_t sgi,
                     const float* h0, const void* whh, const float* bhh, float* out,
                     void* out_lp, int64_t ldo, int64_t so, float* gates, int64_t ldg,
                     int64_t sg, void* work, size_t work_bytes, void* stream) {
    return srnn_gru_xcd_fwd2(dtype, B, D, Fr, gi, ldgi, sgi, h0, whh, bhh, out, out_lp, ldo, so,
                             gates, ldg, sg, nullptr, work, work_bytes, stream);
}

int srnn_gru_xcd_bwd2(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                      const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                      int64_t so, const float* h0, const void* whh_t, float* dgh, void* dgh_lp,
                      float* dgi, void* dgi_lp, float* bsum, int64_t ldd, int64_t sd,
                      float* ddir0, void* work, size_t work_bytes, void* stream) {
    return forced(gru_try_xcd_bwd(bwd_record(dtype, B, D, Fr, dy, lddy, sdy, gates, ldg, sg, hout,
                                             ldo, so, h0, nullptr, whh_t, dgh, dgh_lp, dgi, dgi_lp,
                                             bsum, ldd, sd, ddir0, work, work_bytes),
                                  (hipStream_t)stream),
                  "gru_xcd_bwd");
}

int srnn_gru_xcd_bwd(int dtype, int B, int D, int Fr, const float* dy, int64_t lddy, int64_t sdy,
                     const float* gates, int64_t ldg, int64_t sg, const float* hout, int64_t ldo,
                     int64_t so, const float* h0, const void* whh_t, float* dgh, void* dgh_lp,
                     float* dgi, int64_t ldd, int64_t sd, float* ddir0, void* work,
                     size_t work_bytes, void* stream) {
    return srnn_gru_xcd_bwd2(dtype, B, D, Fr, dy, lddy, sdy, gates, ldg, sg, hout, ldo, so, h0,
                             whh_t, dgh, dgh_lp, dgi, nullptr, nullptr, ldd, sd, ddir0, work,
                             work_bytes, stream);
}

}  // extern "C"

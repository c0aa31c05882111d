// bayhunter_amd/csrc/rf_plan.hip -- the launch plan of the receiver function (rf_plan.h): every rule of its three launchers, once.
// Host code only: no kernel, no HIP call, nothing static -- the plan is a function of the ask and the switches alone.
#include "rf_plan.h"
#include "bh_tuning.h"
#include "../../include/bh_engine.h"
#include <cmath>

namespace {

// w / a beyond which the Gauss low-pass exp(-(w/a)^2 / 4) is below RF_CUT = 1e-17: 2 sqrt(17 ln 10)
constexpr double RF_CUT_WA = 12.5132;

const struct { int code; const char *text; } RF_REFUSALS[] = { // by RfRefusal
    {BH_OK, ""},
    {BH_EUNSUPPORTED, "receiver function: nsamp above 262144 is not supported"},
    {BH_EUNSUPPORTED, "receiver function: the longest trace of the sites' own axes does not fit a workgroup's LDS (nsamp above 16384)"},
    {BH_EHIP, "receiver function: the device refused the synthesis kernels the 160 KiB LDS allowance (hipFuncSetAttribute)"},
};

RfPlan refuse(int refusal)
{
    RfPlan p{};
    p.refusal = refusal;
    p.code = RF_REFUSALS[refusal].code;
    return p;
}

} // namespace

const char *bh_rf_refusal_text(int refusal)
{
    return (refusal >= 0 && refusal <= RF_REFUSE_ALLOWANCE) ? RF_REFUSALS[refusal].text : "";
}

size_t bh_rf_lds_bytes(int nsamp)
{
    return (size_t)(nsamp / 2) * 16 + 16 + 64 * 16 + (size_t)(nsamp >= 128 ? nsamp / 128 : 1) * 16;
}

// Spectral cut-off.  Every bin carries the Gauss low-pass exp(-w^2 / (4 a^2)) (greens.cpp:343-398); where that
// factor is below RF_CUT = 1e-17 the bin is below 1e-17 of the pass band (|R/Z| is of order one): a tenth of the
// rounding unit (2^-53 = 1.1e-16) of the sums the transform forms, i.e. it is lost in the reference's own additions.
// Such bins are set to zero instead of being computed (the reference computes them and multiplies by ~0).  With
// a = 2.5, 20 Hz, nsamp 2048 that is every bin above 5.0 Hz: 510 of 1025 are computed, 8 passes of 64 lanes per model
// (round 2 cut at 1e-30: 678 bins, 11 passes).  tests/test_gpu_rf.py compares with the uncut transform (1e-13).
RfAxisCut bh_rf_axis_cut(int nsamp, double fsamp, double gauss)
{
    const int half = nsamp / 2;
    int logm = 0;
    while ((1 << logm) < half) ++logm;
    const double dw = 2.0 * M_PI * fsamp / nsamp;
    const double jc = std::floor(RF_CUT_WA * gauss / dw) + 1.0;
    return RfAxisCut{logm, !(jc < (double)half) ? half + 1 : (int)jc};
}

RfAxisRec bh_rf_axis_record(int nsamp, double fsamp, double tshift, double gauss)
{
    const RfAxisCut c = bh_rf_axis_cut(nsamp, fsamp, gauss);
    return RfAxisRec{fsamp, tshift, gauss, nsamp, c.logm, c.jcut, 0};
}

RfPlan bh_plan_rf(const RfAsk &q, const BhTuning &tun)
{
    const bool own_axes = q.build == RF_SITEAXIS;
    // ---- the LDS of a synthesis workgroup --------------------------------------------------------------------------------------
    // (site axes: every workgroup holds the LDS of the column's longest trace; a site's own tables lie inside it, bh_rf_lds_bytes
    // grows with nsamp)
    size_t lds = bh_rf_lds_bytes(q.nsamp);
    // a trace longer than a workgroup's LDS holds: the spectra go through a workspace -- on the shared axis only
    const bool longtrace = lds > BH_RF_MAX_LDS;
    if (longtrace && own_axes) return refuse(RF_REFUSE_SITE_LDS);
    if (longtrace && q.nsamp > BH_RF_MAX_NSAMP) return refuse(RF_REFUSE_NSAMP);

    RfPlan p{};
    p.workspace = longtrace;
    if (longtrace) {
        p.work_bytes = (size_t)q.B * (size_t)(q.nsamp / 2) * 2 * sizeof(double);
        lds -= (size_t)(q.nsamp / 2) * 16; // (the spectrum is in the workspace)
    }
    // Where the workgroups go.  Beside a dispersion launch (fused call, second stream) the synthesis workgroups must not take wave
    // slots before the dispersion kernel's wavefronts are resident -- that kernel counts on all of them being co-resident (one
    // round of wavefronts; displaced ones wait for a whole lifetime: 3.6 -> 7 ms measured when the 17.7 KB workgroups of round 3
    // slipped into the 18 KB of LDS the dispersion wavefronts leave free on a CU).  Asking for more LDS than that remainder keeps
    // them out of CUs whose dispersion wavefronts are still running, as in round 2 (40 KB).  Behind the start gate of plan_eval
    // the floor is not needed: the workgroups are dispatched after every dispersion wavefront is resident and only take what
    // finished wavefronts have freed (rf_keep_floor keeps it; rf_lds_gated: a floor of the gated call, fewer workgroups per CU at
    // a time).  The workspace form takes no floor.
    const bool gated = q.gated && tun.rf_keep_floor == 0;
    size_t lds_min = 0;
    if (q.beside_swd && !longtrace) lds_min = !gated ? (size_t)(q.rf_lds_beside_swd > 0 ? q.rf_lds_beside_swd : 0) : (size_t)(tun.rf_lds_gated > 0 ? tun.rf_lds_gated : 0);
    if (lds < lds_min) lds = lds_min;
    p.lds = lds;
    p.big_lds = lds > 64 * 1024; // beyond the default dynamic-LDS limit: a workgroup may take the CU's whole 160 KB

    // ---- the coefficient kernel ------------------------------------------------------------------------------------------------
    // (a lane per layer up to 32 layers; the 96-register build in a gated fused call, where it is resident beside the dispersion
    // wavefronts, unless rf_coef_big)
    const bool small = q.beside_swd && gated && tun.rf_coef_big == 0;
    if (q.Lmax <= 16) {
        p.coef = small ? RF_COEF_LAYERS16_SMALL : RF_COEF_LAYERS16;
        p.coef_grid = (unsigned)((q.B + 15) / 16);
    } else if (q.Lmax <= 32) {
        p.coef = small ? RF_COEF_LAYERS32_SMALL : RF_COEF_LAYERS32;
        p.coef_grid = (unsigned)((q.B + 7) / 8);
    } else {
        p.coef = RF_COEF_SERIAL;
        p.coef_grid = (unsigned)((q.B + 255) / 256);
    }

    // ---- the synthesis kernel ---------------------------------------------------------------------------------------------------
    p.synth = longtrace ? RF_SYNTH_LONG : (tun.rf_waves == 3 ? RF_SYNTH_W3 : RF_SYNTH_W4);
    p.block = (!longtrace && tun.rf_threads == 128) ? 128 : 256;
    p.no_realc = tun.rf_no_realc != 0 ? 1 : 0;
    p.no_rot = tun.rf_no_rot != 0 ? 1 : 0;
    p.no_cut = tun.rf_no_cut != 0 ? 1 : 0; // (tests flip it with bh_engine_set_tuning)
    if (!own_axes) {
        const RfAxisCut c = bh_rf_axis_cut(q.nsamp, q.fsamp, q.gauss);
        p.logm = c.logm;
        p.jcut = p.no_cut ? q.nsamp / 2 + 1 : c.jcut;
    }
    return p;
}

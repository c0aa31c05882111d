// bayhunter_amd/csrc/rf_plan.h -- what a receiver-function launch is asked for and what it is told: the launch plan behind the three
// launchers bh_launch_rf, bh_launch_rf_m, bh_launch_rf_t (rf_kernel.hip and its two further builds).
//
// No HIP type, and host only but for RfAxisRec at the end: the engine fills an RfAsk, bh_plan_rf (rf_plan.hip; pure: no HIP call,
// no allocation, nothing static) states every rule once -- the refusals, the LDS of a synthesis workgroup with its floor beside a
// dispersion launch, the HBM workspace of long traces, the coefficient and the synthesis kernel with their geometry, logm and jcut
// of the shared axis, the switches the kernels read -- and the launcher of the build launches what the plan names, with the kernels
// of its own translation unit.  tests/test_rf_plan.py holds the planner to a restatement of these rules, without a GPU.
#ifndef BH_RF_PLAN_H
#define BH_RF_PLAN_H

#include <stddef.h>
#include <stdint.h>

struct BhTuning; // bh_tuning.h

// LDS of one workgroup of the synthesis kernel for traces of nsamp samples: the half-length complex spectrum, the Nyquist bin and
// two twiddle tables.  A CU has 160 KB, one workgroup may use all
constexpr size_t BH_RF_MAX_LDS = 160 * 1024;
size_t bh_rf_lds_bytes(int nsamp);
// Longer traces (nsamp > 16384) keep the half-length spectrum in an HBM workspace (RfKernelArgs::zwork) and run the same
// butterflies there; the largest transform served (the second twiddle table, nsamp / 128 entries, stays in LDS)
constexpr int BH_RF_MAX_NSAMP = 1 << 18;

// The build that serves a launch: which translation unit's kernels, and what they read of the site table
enum RfBuild {
    RF_PLAIN = 0, // rf_kernel.hip: p and nsv as given
    RF_SITES,     // rf_kernel.hip, the site-indexed coefficient kernels (bh_sites_set_rf)
    RF_MISSING,   // rf_kernel_m.hip: sites that may lack the target (bh_sites_set_missing)
    RF_SITEAXIS,  // rf_kernel_t.hip: sites with their own time axis and filter (bh_sites_set_rf_axis)
    RF_BUILDS
};
// The coefficient kernels, in the order the launchers list them; the site-indexed builds take the same numbers
enum RfCoefKernel {
    RF_COEF_LAYERS16_SMALL = 0, // rf_coef_layers_kernel_small<16>: a lane per layer, the 96-register build, 16 models per workgroup
    RF_COEF_LAYERS32_SMALL,     // rf_coef_layers_kernel_small<32>: 8 models per workgroup
    RF_COEF_LAYERS16,           // rf_coef_layers_kernel<16>
    RF_COEF_LAYERS32,           // rf_coef_layers_kernel<32>
    RF_COEF_SERIAL,             // rf_coef_kernel: a lane per model
    RF_COEF_KERNELS
};
enum RfSynthKernel {
    RF_SYNTH_W4 = 0, // rf_synth_kernel: four wavefronts per SIMD
    RF_SYNTH_W3,     // rf_synth_kernel_w3: the register budget of three (bh_tuning.h rf_waves)
    RF_SYNTH_LONG,   // rf_synth_kernel_long: the spectrum in the HBM workspace; the site-axis build has none
    RF_SYNTH_KERNELS
};
// Why nothing is launched (the plan reports the first that holds), and what a launcher can fail with
enum RfRefusal {
    RF_REFUSE_NONE = 0,
    RF_REFUSE_NSAMP,     // the shared axis is longer than the largest transform served
    RF_REFUSE_SITE_LDS,  // site axes: the column's longest trace does not fit a workgroup's LDS (the table refuses it earlier)
    RF_REFUSE_ALLOWANCE  // (not a plan's: the launcher's) the device did not grant the synthesis kernels the CU's whole LDS
};
const char *bh_rf_refusal_text(int refusal); // the message of an RfRefusal ("" for RF_REFUSE_NONE)

struct RfAsk {
    int B, Lmax;
    int build;              // RfBuild
    int nsamp;              // of the shared axis; RF_SITEAXIS: the largest of the column (RfSiteTArgs::nsamp_max)
    double fsamp, gauss;    // of the shared axis (RF_SITEAXIS: not read)
    bool beside_swd;        // the launch runs on the second stream of a forked call, beside the dispersion launch
    bool gated;             // ... behind the start gate (the gate was wanted and the dispersion launch had workgroups)
    int rf_lds_beside_swd;  // the engine's LDS floor [bytes] of synthesis workgroups beside an ungated dispersion launch
};

struct RfPlan {
    int code, refusal;      // BH_OK and RF_REFUSE_NONE, or why nothing is launched
    int coef;               // RfCoefKernel, in workgroups of 256 threads:
    unsigned coef_grid;
    int synth;              // RfSynthKernel, a workgroup per model:
    unsigned block;
    size_t lds;             // ... and its dynamic LDS [bytes]
    bool big_lds;           // lds exceeds the 64 KiB every kernel may have: the kernel needs the 160 KiB allowance first
    bool workspace;         // the half-length spectra go through the HBM workspace (RfKernelArgs::zwork)
    size_t work_bytes;      // ... of this size (0 without)
    int logm, jcut;         // of the shared axis (RF_SITEAXIS: 0, the sites' records carry their own)
    int no_realc, no_rot, no_cut; // the switches the kernels read (bh_tuning.h)
};

RfPlan bh_plan_rf(const RfAsk &q, const BhTuning &tun);

// logm (the half-length transform has 2^logm points) and jcut (the first bin the Gauss low-pass leaves below RF_CUT = 1e-17 of the
// pass band, nsamp / 2 + 1 where it keeps them all) of one time axis: the plan's and every site record's
struct RfAxisCut {
    int logm, jcut;
};
RfAxisCut bh_rf_axis_cut(int nsamp, double fsamp, double gauss);

// The record of one site's own axis (bh_sites_set_rf_axis), as the synthesis kernels of rf_kernel_t.hip read it from the device
// table RfSiteTArgs::axis: its layout is device code (as RfKernelArgs', bh_device.h) and must not move.  It stands here, in a header
// that bh_device.h includes into every kernel unit, beside the one host function that fills it.
struct RfAxisRec {
    double fsamp, tshift, gauss;
    int32_t nsamp, logm, jcut; // (the rf_no_cut switch overrides jcut at launch)
    int32_t pad;
};
RfAxisRec bh_rf_axis_record(int nsamp, double fsamp, double tshift, double gauss);
#endif

// bayhunter_amd/csrc/bh_device.h -- shared declarations of the gfx950 kernels.
//
// Everything in csrc/ is written for CDNA4 (MI355X, wave64) only and is compiled with
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
// -ffp-contract=off matters: the reference's Fortran/C++ round every product and sum
// separately (x86-64 baseline, no FMA); the root search of surf96 branches on signs and on
// 1e-6-relative comparisons of those values, so the kernels keep the same rounding points.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "rf_plan.h"

#define BH_WAVE 64
// debug counter block of the dispersion kernels: BH_COUNTER_WORDS counters + 4 words per traced wavefront
#define BH_COUNTER_WORDS 16
#define BH_TRACE_WAVES 16384
#define BH_DEBUG_WORDS (BH_COUNTER_WORDS + 4 * BH_TRACE_WAVES)
#define BH_BOARD_WORDS (2 * 32768) // progress board: 2 wave slots x (8 XCCs x 4096 SIMD keys)

// ---- IEEE division with the denominator-only work factored out ----------------------------------
// hipcc expands the f64 `a / b` to   d = div_scale(b), n = div_scale(a), r = rcp(d),
// two Newton steps on r, q = n*r, rem = fma(-d, q, n), div_fmas(rem, r, q), div_fixup.
// When neither operand needs the power-of-two pre-scaling (both magnitudes in
// [2^-400, 2^400] here, far inside the hardware's trigger points) d = b, n = a, div_fmas is a
// plain fma and div_fixup returns its input, so  bh_quot(a, b, bh_rcp_refined(b))  is the SAME
// instruction sequence and returns the same bits as a / b -- but the five denominator-only
// instructions can be shared by several divisions or hoisted out of a dependent chain.
// tests/test_gpu_swd.py::test_shared_reciprocal_division_is_exact checks this on the device.
__device__ __forceinline__ double bh_rcp_refined(double b)
{
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}
__device__ __forceinline__ double bh_quot(double a, double b, double r)
{
    const double q = a * r;
    const double rem = __builtin_fma(-b, q, a);
    return __builtin_fma(rem, r, q);
}
// |x| in [2^-400, 2^400]  (biased exponent 623..1423); false for 0, denormals, inf, NaN
__device__ __forceinline__ bool bh_div_safe(double x)
{
    const unsigned ex = ((unsigned)__double2hiint(x) >> 20) & 0x7ffu;
    return (ex - 623u) <= 800u;
}

// hipFuncAttributeMaxDynamicSharedMemorySize applies per DEVICE: remember per device (bit d of *done) that a set of kernels
// has been allowed `bytes` of dynamic LDS.  (A process-wide flag left the second GPU of a process without it: ADVICE r03.)
#include <atomic>
inline bool bh_allow_big_lds(std::atomic<unsigned long long> *done, const void *const *kernels, int nkernels, int bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return false;
    const unsigned long long bit = 1ull << dev;
    if (done->load(std::memory_order_acquire) & bit) return true;
    for (int k = 0; k < nkernels; ++k)
        if (hipFuncSetAttribute(kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    done->fetch_or(bit, std::memory_order_release);
    return true;
}

struct SwdKernelArgs {
    int B, Lmax, K, igr, mode;
    const int32_t *nlay;
    const int32_t *perm; // optional: models in the order the wavefronts take them (deepest first), see bh_launch_order
    const double *h, *vp, *vs, *rho;
    ptrdiff_t sl, sb; // element strides: layer, model
    const double *periods;
    double *vel;      // [B][ldv] (+ column offset already applied)
    int ldv;          // row stride of vel in elements
    int32_t *err;     // [B]
    unsigned long long *neval; // optional global counter of secular evaluations (may be null)
    int look;         // trial velocities per round and model = lanes per model (1, 2, 4, 8 or 16), see SearchT::candidate
    int fair;         // alternate the issue priority of the two wavefronts of a SIMD (scheduling only)
    double *nev_high; // work array [bh_swd_nev_high_doubles(B, look)]: Neville orders the kernel does not keep in LDS
    int fast;         // 1: the build with the short refinement (SearchT<.., FAST>; phase-velocity targets take it)
    int counted;      // 1: Love scans skip the steps a mode count proves empty (SearchT: the counted scan; same bits)
    int farith;       // 1: a launch of the short refinement (fundamental-mode phase velocities) computes with the fast arithmetic (swd_fa.h)
    int32_t *gcount, *glist; // short refinement: models its guard fired on are appended here (count, indices), see SearchT
    // A group velocity's two chains of roots (SearchT: F_CHAIN_A / F_ONE).  igr = 2 (engine_swd.hip swd_target, for a job the plan
    // marks SwdPlan::first_roots; never a caller's value): the chain of first roots, unrounded into vel,
    // the value getsol keeps from the mode's first search into first[model].  second = 1 (igr = 1): B = Bm x K searches, entry
    // v = the second root of period v / Bm of model v % Bm, which reads vel and first and writes the group velocity (err untouched).
    int second, Bm;
    double *first;
};

// Which instantiation a launch of the lane kernel (swd_kernel) or of the trial-per-lane kernel (swd_lean_kernel) took: its
// template arguments (lane: IFUNC, LOOK, WPB, FAST, SIMPLE, FA; lean: J, CNT), workgroups and time slice (bh_engine_debug.h).
struct SwdLaneBuild {
    int key[6];
    unsigned grid_x;
    int fair;
};
void bh_launch_swd(const SwdKernelArgs &a, int iwave, hipStream_t stream, SwdLaneBuild *build = nullptr);
// perm[0..B) = model indices sorted by layer count, deepest first: wavefronts then hold models of (nearly)
// one depth -- no masked layers, and the long-running deep models start first.  Results do not depend on it.
void bh_launch_order(int B, const int32_t *nlay, int32_t *perm, int Lcut, int32_t *split, hipStream_t stream);
size_t bh_swd_lds_bytes(int Lmax, int K, int mode);
size_t bh_swd_nev_high_doubles(int B, int look);

// group kernel: G lanes per model, all dispersion targets of a call in one launch
struct SwdTarget {
    int iwave, igr, K, ldv, mode;
    int look; // trial velocities per round for this target's wavefronts (>= 1), see SearchT::candidate
    int inlook; // Love only: further trials inside a lane group (1..4), see swd_group_kernel
    const double *h, *vp, *vs, *rho; // model arrays this target reads (earth-flattened copies when flsph = 1)
    ptrdiff_t sl, sb;
    const double *periods;
    double *vel;  // [B][ldv] (+ column offset already applied)
    int32_t *err; // [B]
    const int32_t *perm; // optional: this target's own processing order (bh_launch_pair_order); else SwdMultiArgs::perm
    const int32_t *count; // optional (device): the launch covers the first *count entries of the processing order only (the
                          // re-run of the models the short refinement's guard fired on: perm = that list)
    int32_t *gcount, *glist; // short refinement: models its guard fired on are appended here (count, indices), see SearchT
    int refseq;              // 1: in a launch with the short refinement this (phase-velocity) target keeps the reference's sequence
    double *first;           // igr = 2 (the chain of a group velocity's first roots, SwdKernelArgs; engine_swd.hip swd_target): [B]
};
struct SwdMultiArgs {
    int B, Lmax, ntargets;
    const int32_t *nlay;
    const int32_t *perm; // optional, as in SwdKernelArgs
    // Two classes of models in processing order: [0, split[0]) have more than `Lcut` layers ("deep"),
    // the rest at most Lcut.  Each class gets its own launch with LDS rows for its depth, so that a
    // batch whose array capacity (Lmax) is far above its typical depth still packs many models per
    // wavefront.  Both classes run in ONE launch (blockIdx.z = class) with the same LDS budget per
    // wavefront: the deep class simply takes fewer models per wavefront (more lanes per model).
    // split == nullptr: one class (index 1), rows = Lmax.  rows[] / lanes[]: the group plan's (bh_plan_swd_group).
    const int32_t *split;
    int Lcut;
    int rows[2], lanes[2]; // per class (0 = deep, 1 = the rest): LDS rows per model, lanes per model (G)
    int wg_n0, wg_n1;      // the launch plan's: > 0 = one-dimensional grid of two targets, interleaved (wavefront counts)
    unsigned long long *neval;
    unsigned *board;  // optional: progress board of the group kernel, 2 words per physical SIMD (BH_BOARD_WORDS), see the kernel
    unsigned stamp;   // launch stamp (16 bits) that marks this launch's entries of the board
    unsigned *started; // optional: every workgroup adds 1 when it starts (cumulative over launches): a second stream waits
                       // for "all workgroups of this launch are resident" before it dispatches work beside them
    int prio_low;      // s_setprio level of a wavefront's unfavoured phase (0; 1 when receiver-function wavefronts at 0 run beside it)
    int fast;          // the build's sequences (SwdGroupBuild::fastm): 0 = reference, 1 = both, 2 = the short refinement only
    int adapt_ok;      // 1: a launch of one model per wavefront may let every wavefront size its lane groups and trials for its
                       // own model (swd_group_kernel<.., ADAPT>); 0: the caller fixed lanes or trials (experiments)
    int counted;       // 1: Love scans skip the steps a mode count proves empty (SearchT: the counted scan; same bits)
    int rerun;         // 1: the launch re-runs listed models (SwdTarget::count): plain two-dimensional grid, no SIMD pairing
    int farith;        // 1: launches in which every target takes the short refinement evaluate the secular functions with the fast
                       //    arithmetic (swd_fa.h, swd_group_kernel<.., FA>); the group plan's decision
    int restart;       // 1: in a launch of one model per wavefront a model the guard fires on starts again with the reference's
                       //    sequence in its own wavefront (the build with both sequences) instead of being listed for a re-run launch
    SwdTarget t[8];
    // (behind everything else: the builds that do not read them keep the parent's argument layout and machine code)
    int lean_prio;     // trial-per-lane kernel, a launch whose SIMDs each hold one Rayleigh and one Love wavefront: 0, or share | slice << 8 --
                       //    the Rayleigh wavefront has the high issue priority in `share` of every eight time slices of 2^slice cycles, the
                       //    Love wavefront in the others (swd_lean_kernel; the engine's decision, launch_swd_multi)
    int lean_half;     // ... and a launch of exactly two workgroups per CU: a target's wavefronts per XCD in the FIRST pass of workgroups
                       //    (CUs / 4), which says which Love position shares a SIMD with which Rayleigh position; 0: not known
};
// Dispersion periods per site (bh_sites_set_x, include/bh_engine_sites_x.h): an argument of its own of the SITE-PERIOD builds of
// the dispersion kernels (swd_lean_x.hip, swd_group_x.hip: the same sources compiled with BH_SWD_SITEX), so that SwdMultiArgs
// and the builds without it keep their layout and machine code.  A model of site s searches target `ty` of the launch at the
// n[s * nt + col[ty]] periods x[s * ldx + off[ty] ...]; SwdTarget::K is the CAPACITY of the target's ymod columns (the largest
// count of any site), SwdTarget::periods is not read.  A site out of range reads nothing of the tables and fails in band.
struct SwdSiteXArgs {
    const int32_t *site; // device [B]: site of every model (null: the call has no per-site periods)
    int nsites, nt, ldx; // row strides of n (the registered targets) and x (ymod's row)
    const int32_t *n;    // device [nsites][nt]
    const double *x;     // device [nsites][ldx], targets in ymod's column layout
    int col[8], off[8];  // per target of the launch (SwdMultiArgs::t): its registered target and column offset
};
// the count of periods (0 ... cap; -1: site out of range) of model ib for target ty of the launch
__device__ __forceinline__ int bh_site_count(const SwdSiteXArgs &X, int ty, int ib, int cap)
{
    const int s = X.site[ib];
    if (s < 0 || s >= X.nsites) return -1;
    const int n = X.n[(size_t)s * X.nt + X.col[ty]];
    return n < 0 ? 0 : (n > cap ? cap : n);
}
// ... and the periods themselves (per; the table's start for a site out of range: nothing of it is read)
__device__ __forceinline__ int bh_site_periods(const SwdSiteXArgs &X, int ty, int ib, int cap, const double *&per)
{
    const int n = bh_site_count(X, ty, ib, cap);
    per = n < 0 ? X.x : X.x + (size_t)X.site[ib] * X.ldx + X.off[ty];
    return n;
}
// The second roots of a split group velocity (SwdKernelArgs::second) at every model's own periods (bh_sites_set_x_all,
// include/bh_engine_sites_x_all.h): the site-period build of swd_kernel (swd_kernel_x.hip).  a as for bh_launch_swd, a.K the
// CAPACITY of the target's columns (a.B = a.Bm x a.K entries), a.periods not read; ty: the target of x (col / off) the launch is
// for.  An entry whose period index is at or beyond its site's count, or whose site is out of range, is idle and writes nothing.
void bh_launch_swd_second_x(const SwdKernelArgs &a, int iwave, const SwdSiteXArgs &x, int ty, hipStream_t stream, SwdLaneBuild *build = nullptr);
int bh_swd_pick_group(int B, int ntargets, int Lmax);
double bh_swd_plan(int B, int Lmax, int ntargets, const int *iwave, int Gforce, int *G, int *look);
size_t bh_swd_group_lds_bytes(int G, int J, int Lmax, int Kmax, int maxmode, bool sitex = false);
// Work space of the SIMD-pairing order (swd_kernel.hip: pair_order_kernel; engine_swd.hip: order_models).  The
// dispersion kernel's time is that of its slowest SIMD, a SIMD's time follows the SUM of the root-search lengths of the
// two wavefronts it holds, and which wavefronts of a launch share a SIMD is a fixed function of their grid index; so the
// models are dealt to the wavefronts by PREDICTED search length such that every SIMD gets a long and a short wavefront
// and the SIMDs that hold one wavefront only get the longest.  Scheduling only: per-model results do not depend on it.
struct SwdPairWork {
    int ncu = 0;                      // compute units of the device (the placement rule below is per CU)
    int32_t *perm[2] = {nullptr, nullptr};      // device, [B] each: processing order of target 0 / 1
    int32_t *slot_rank[2] = {nullptr, nullptr}; // device, [wavefronts of the target]: rank of the wavefront's load (0 = longest models)
    int cap_perm = 0, cap_rank[2] = {0, 0};
    int key_n0 = -1, key_n1 = -1;     // wavefront counts the slot_rank tables were built for
};
struct PairOrderTarget {
    int mpw, nwaves;          // models per wavefront, wavefronts of the target
    const int32_t *slot_rank; // [nwaves - 1]: load rank of every wavefront but the last (which may be partly filled)
    int32_t *perm;            // out [B]
    int xcd;                  // trial-per-lane kernel: > 0 = the order is sorted inside eight blocks of the batch, block x handed to the
                              // wavefronts that run on XCD x (workgroup index mod 8); the value = wavefronts of this target per workgroup (4, or 2
                              // where two targets alternate): every XCD's L2 then sees an eighth of the model arrays
};
// The words a dispersion call wants zero before its kernels run -- the guard's head (engine_swd.hip guard_space), the per-target
// failure flags, the counters -- where the ordering launch that precedes them zeroes them (the call's prologue: no fill
// dispatches of their own).  A count of 0: nothing to zero there.
struct SwdFills {
    int32_t *guard = nullptr;
    int32_t *err = nullptr;
    unsigned long long *counter = nullptr;
    int nguard = 0, nerr = 0, ncounter = 0; // words
};
bool bh_pair_order_fits(int B);
// The order of nt targets (0: the launch only zeroes) and the fills, one launch: a workgroup per XCD block where every target's
// order is blocked (PairOrderTarget::xcd and the divisibilities it stands for), else one workgroup.
// Returns the workgroups launched (8 or 1).
int bh_launch_pair_order(int B, int Lmax, const int32_t *nlay, const double *vs, ptrdiff_t sl, ptrdiff_t sb, int nt,
                         const PairOrderTarget *tg, const SwdFills &fills, hipStream_t stream);
struct SwdLaunchInfo {
    unsigned workgroups; // of the launch (what SwdMultiArgs::started is advanced by)
    long waves;          // wavefronts that do work
    size_t lds;          // bytes per workgroup
    int wpb;             // wavefronts per workgroup
};
// Trials per round that fit a wavefront of G-lane groups: `look` (at least 1), fewer while G x trials exceeds a wavefront.
inline int bh_trials_fit(int G, int look)
{
    int J = look > 1 ? look : 1;
    while (J > 1 && G * J > BH_WAVE) --J;
    return J;
}
// What one launch of the group kernel is asked for: its shape and the caller's requests (bh_plan_swd_group).
struct SwdGroupAsk {
    int B, Lmax, Lcut, ntargets; // Lcut < Lmax: two depth classes (SwdMultiArgs::split)
    int G0;                      // lanes per model of the engine's plan
    struct Target {
        int K, look, iwave, mode;
        bool group, refseq;      // a group velocity (igr != 0); SwdTarget::refseq
    } t[8];                      // (as SwdMultiArgs::t)
    bool fast, farith, restart;  // the short refinement, its fast arithmetic, restarts in place: asked for
    bool adapt_ok, rerun;        // SwdMultiArgs::adapt_ok and ::rerun
    bool counters;               // the build with counters and clocks (SwdMultiArgs::neval set)
    bool sitex;                  // periods per MODEL (SwdSiteXArgs): a wavefront's LDS holds a row of K periods for each of its models
    int scan;                    // the counted scan asked for: 0, 1 = wherever a Love target is, 2 = where it pays
};
// Which instantiation of swd_group_kernel a launch takes (its template arguments but WPB).
struct SwdGroupBuild {
    int fastm;                          // FASTM: 0 = reference sequence, 1 = both sequences, 2 = short refinement only
    bool simple, prof, adapt, cntb, fa; // SIMPLE, PROF (counters and clocks), ADAPT, CNTB (counted Love scan), FA
};
// Everything a launch of the group kernel does, decided by bh_plan_swd_group with no HIP call.
struct SwdGroupPlan {
    bool fits;               // false: a class's layers do not fit a workgroup's LDS (the call fails)
    int rows[2], lanes[2];   // per class (0 = deep, 1 = the rest; one class: both the same): LDS rows, lanes per model
    int wg_n0, wg_n1;        // > 0: the two targets' wavefronts interleaved in a one-dimensional grid (their counts)
    size_t wave_lds, lds;    // LDS of a wavefront's region, of a workgroup
    dim3 grid, block;
    int Gflags;              // the kernel's experiment flags (bh_tuning.h swd_redundant, swd_no_board, swd_no_fair)
    bool restart;            // guarded models restart in place (SwdMultiArgs::restart): no re-run launch follows
    SwdGroupBuild build;
    // SIMD-pairing geometry (SwdPairWork): pair = the launch admits the order (one class, a one-dimensional grid, at most two
    // targets, a batch pair_order_kernel takes); per target its models per wavefront and wavefronts
    bool pair;
    int pair_mpw[2], pair_waves[2];
    SwdLaunchInfo info;
};
struct BhTuning;
SwdGroupPlan bh_plan_swd_group(const SwdGroupAsk &q, const BhTuning &tun);
// The launch of plan g with arguments a (whose rows, lanes, wg_n*, fast, counted, farith and restart are g's).  Every build a plan
// can name is compiled (tests/test_swd_group_plan.py).
void bh_launch_swd_group(const SwdMultiArgs &a, const SwdGroupPlan &g, hipStream_t stream);
// ... of the site-period build of the same name (swd_group_x.hip; q.sitex was set): false if the plan's build is not compiled
bool bh_launch_swd_group_x(const SwdMultiArgs &a, const SwdGroupPlan &g, const SwdSiteXArgs &x, hipStream_t stream);
struct SwdGroupXStream { // what a site-period build is launched with
    hipStream_t st;
    const SwdSiteXArgs *x;
};
bool bh_swd_group_builds_fa_x(const SwdMultiArgs &a, const SwdGroupPlan &g, SwdGroupXStream s);
bool bh_swd_group_builds_adapt_x(const SwdMultiArgs &a, const SwdGroupPlan &g, SwdGroupXStream s);
bool bh_swd_group_builds_big_x(const SwdMultiArgs &a, const SwdGroupPlan &g, SwdGroupXStream s);
// The builds each translation unit of swd_group_kernel compiles (swd_group_fa.hip, swd_group_adapt.hip, swd_group_big.hip), one
// signature: launches g's build if it is one of them.
bool bh_swd_group_builds_fa(const SwdMultiArgs &a, const SwdGroupPlan &g, hipStream_t stream);
bool bh_swd_group_builds_adapt(const SwdMultiArgs &a, const SwdGroupPlan &g, hipStream_t stream);
bool bh_swd_group_builds_big(const SwdMultiArgs &a, const SwdGroupPlan &g, hipStream_t stream);
// swd_lean.hip: fundamental-mode phase velocities with the fast arithmetic, one lane per trial velocity (the kernel of the
// engine's default settings for batches up to a few ten thousand models); a.t[t].look = trials per model and round
int bh_swd_lean_trials(int B, int ntargets);
size_t bh_swd_lean_lds_bytes(int J, int Lmax, int Kmax, bool sitex = false); // sitex: a row of Kmax periods per model
int bh_launch_swd_lean(const SwdMultiArgs &a, hipStream_t stream, SwdLaunchInfo *info, SwdLaneBuild *build = nullptr);
int bh_launch_swd_lean_x(const SwdMultiArgs &a, const SwdSiteXArgs &x, hipStream_t stream, SwdLaunchInfo *info, SwdLaneBuild *build = nullptr);
// earth-flattening of a batch (surfdisp96.f:486-553): writes layer-major [Lmax][B] float64 copies
// (binary32-valued) of thickness, vp, vs and the Love / Rayleigh density mappings
void bh_launch_sphere(int B, int Lmax, const int32_t *nlay, const double *h, const double *vp,
                      const double *vs, const double *rho, ptrdiff_t sl, ptrdiff_t sb, double *oh,
                      double *ovp, double *ovs, double *orho_love, double *orho_ray, hipStream_t stream);
// np.interp of B rows from K0 to K1 abscissae (the > 60 periods path of surf96_modsw.py:119-122)
void bh_launch_interp(int B, int K0, const double *x0, const double *y0, int ld0, int K1,
                      const double *x1, double *y1, int ld1, hipStream_t stream);

struct RfKernelArgs {
    int B, Lmax, nsamp, nkeep, waveno;
    const int32_t *nlay;
    const double *h, *vp, *vs, *rho, *qp, *qs; // qp/qs may be null -> 500/225
    ptrdiff_t sl, sb;
    double p_s_per_deg, gauss, fsamp, tshift, nsv;
    double *coef;  // workspace [B][bh_rf_coef_doubles(Lmax)]
    double *rf;    // [B][ldr]
    int ldr;
    // fused likelihood (bh_evaluate_batch without synthetics, nocorr / exponential law): instead of the trace the synthesis
    // kernel writes, per model, the four sums the likelihood needs of it -- sum d^2, sum d_i d_(i+1), d_0, d_(n-1), d = trace -
    // yobs, formed in like_kernel's own order (same bits) -- to sums[B][4]; null: the trace is written
    const double *yobs;
    double *sums;
    double *zwork; // traces beyond BH_RF_MAX_LDS: workspace [B][nsamp / 2] complex (16 bytes each) for the half-length spectra, else null
    int lds_min;   // unused, 0 (the LDS request is the plan's, rf_plan.h); kept so that no kernel argument moves
    int no_realc;  // experiment switch (RfPlan::no_realc): 1 = always the general (complex-coefficient) recursion
    int coef_small; // unused, 0 (the coefficient kernel is the plan's); kept as lds_min
    int no_rot;    // experiment switch (RfPlan::no_rot): 1 = no rotation of the bins over a workgroup's wavefronts
};
// Receiver-function parameters per site (bh_sites_set_rf, include/bh_engine_sites_rf.h): the coefficient kernels give a model of
// site s the ray parameter p[s * ld] and near-surface velocity nsv[s * ld] instead of RfKernelArgs::p_s_per_deg / nsv (the
// synthesis kernel reads p from the record).  A site out of range reads nothing of the table and marks the record bad.
struct RfSiteArgs {
    const int32_t *site;    // device [B]: site of every model
    int nsites;
    int ld;                 // row stride of the tables (the number of targets)
    const double *p, *nsv;  // device [nsites][ld], already offset to the target's column
};
size_t bh_rf_coef_doubles(int Lmax);
// The launch plan (rf_plan.h): the engine asks bh_plan_rf, refuses by the plan's code and text, sizes the coefficient record and --
// by the plan -- the workspace, fills RfKernelArgs (the plan's switches included) and hands both to the launcher of the ask's build.
// A launcher decides nothing: it asks for the LDS allowance where the plan says so and launches the coefficient and the synthesis
// kernel the plan names, of its own translation unit.  BH_OK; BH_EHIP when the allowance fails (RF_REFUSE_ALLOWANCE has the text);
// BH_EINVAL for a plan its build does not serve.  sites: null for RF_PLAIN, else the table; every build reads the base it needs.
struct RfSiteTArgs;
int bh_launch_rf(const RfPlan &p, const RfKernelArgs &a, const RfSiteTArgs *sites, hipStream_t stream); // RF_PLAIN, RF_SITES
// Sites that lack a receiver-function target (bh_sites_set_missing, include/bh_engine_sites_missing.h): the builds of
// rf_kernel_m.hip (rf_kernel.hip compiled with BH_RF_MISSING).  n[s * ld] is the sample count of site s for the target (0 or the
// descriptor's): the coefficient stage marks the record of a model whose site has none ABSENT (rec[3] = 2, distinct from bad = 1),
// and a workgroup of the synthesis kernel that finds that mark writes nkeep zeros and leaves -- no recursion, no transform.
struct RfSiteMArgs : RfSiteArgs {
    const int32_t *n; // device [nsites][ld], already offset to the target's column
};
int bh_launch_rf_m(const RfPlan &p, const RfKernelArgs &a, const RfSiteTArgs *sites, hipStream_t stream); // RF_MISSING
// Sites with their own receiver-function time axis and Gauss filter (bh_sites_set_rf_axis, include/bh_engine_sites_rf_axis.h): the
// builds of rf_kernel_t.hip (rf_kernel.hip compiled with BH_RF_SITEAXIS on top of BH_RF_MISSING).  A workgroup of the synthesis
// kernel is one model: it reads its model's site and that site's record, and runs the transform of the site's own length with the
// site's own sampling, shift, filter width and cut; the site's n samples (RfSiteMArgs::n) are followed by zeros up to the column's
// capacity RfKernelArgs::nkeep.  The site's record (RfAxisRec, rf_plan.h) carries logm and jcut, formed on the host by the function the
// plan forms the shared axis's with (bh_rf_axis_cut).
struct RfSiteTArgs : RfSiteMArgs {
    const RfAxisRec *axis; // device [nsites][ld], already offset to the target's column
    int nsamp_max;         // the largest nsamp of the column: the LDS of every workgroup (RfAsk::nsamp)
};
int bh_launch_rf_t(const RfPlan &p, const RfKernelArgs &a, const RfSiteTArgs *sites, hipStream_t stream); // RF_SITEAXIS
// bh_probe_math ops 11-16: the synthesis kernel's own elementary functions (include/bh_engine_debug.h); -1 for another op
int bh_launch_rf_probe(int op, int n, const double *in, double *out, hipStream_t stream);
// bh_probe_math ops 17-23 and bh_probe_swd_secular: the dispersion kernels' fast arithmetic (swd_fa_probe.hip = swd_lean.hip built with
// BH_SWD_PROBE); -1 for another op / for arguments the entry point refuses.  model: [4][mtop] doubles on the device (d, a, b, rho).
int bh_launch_swd_fa_probe(int op, int n, const double *in, double *out, hipStream_t stream);
int bh_launch_swd_secular_probe(int evaluator, int ifunc, int mmax, int mtop, const double *model, int n, const double *wvno,
                                const double *omega, double *out, hipStream_t stream);

struct LikeTargetDev {
    int law, n, off; // off: column offset of this target's samples inside a ymod row
    const double *yobs, *yerr_scaled, *rinv; // device; yerr_scaled = yerr/min(yerr) (law 1)
    double logdet_extra;                     // ln prod(scaled err) (law 1) or ln|R| (law 3)
    const double *quad;                      // law 3: [B][nsplit] column-slab partial sums of d^T R^-1 d
    int nsplit;                              //        (gauss_kernel.hip); null -> in-kernel mat-vec
    const double *pre;                       // laws 0 / 2: [B][4] sums formed by the forward kernel (RfKernelArgs::sums); null -> from ymod
};
int bh_gauss_nsplit(int B, int n);
void bh_launch_gauss_quad(int B, int n, int ldy, const double *ymod, const double *yobs,
                          const double *rinv, int nsplit, double *partial, hipStream_t stream);
// Site tables of bh_evaluate_sites (include/bh_engine_sites.h): model b compares with the observed data of site site[b].
// Gauss contraction: the residual row of model b is ymod row b - yobs + site[b] * ldo (yobs already at the target's column
// offset); a site out of range reads site 0's row (its model is reported failed by the likelihood kernel).
struct GaussSiteArgs {
    const int32_t *site; // device [B]
    int nsites, ldo;
};
void bh_launch_gauss_quad_sites(int B, int n, int ldy, const double *ymod, const double *yobs, const GaussSiteArgs &sites,
                                const double *rinv, int nsplit, double *partial, hipStream_t stream);
// Correlation classes of a Gauss-law target (bh_sites_set_gauss, include/bh_engine_sites_gauss.h): the sites that fix the same noise
// correlation share one R^-1 -- class c's is rinv + c * n * n --, and a model's class is class_of[site[b]] (-1: its site lacks the
// target; a site out of range has none either).  The contraction's builds of gauss_kernel_c.hip group the rows on the device, class
// by class, into tiles of one class each: perm[row_start[c] ... row_start[c + 1]) are the rows of class c (in no fixed order: an
// output row depends on its own residual row, the matrix and the fixed k order only), tile_start[c] the first tile of class c.
struct GaussClassArgs {
    const int32_t *class_of;   // device [nsites]
    int nclass;
    const int32_t *row_start;  // device [nclass + 1]: prefix of the classes' row counts
    const int32_t *tile_start; // device [nclass + 1]: prefix of the classes' tile counts
    const int32_t *perm;       // device [B]: the rows, class by class
};
// int32 words of the grouping's work space: count, cursor [nclass], row_start, tile_start [nclass + 1], perm [B]
inline size_t bh_gauss_class_work_words(int B, int nclass) { return 4 * (size_t)nclass + 2 + (size_t)B; }
// bh_launch_gauss_quad_sites with the matrix of every row's class: same form, slabs and layout of `partial` as for (B, n) there
// (bh_gauss_nsplit), so the likelihood kernel sums the same slabs in the same order; the rows of no class get zeros.
void bh_launch_gauss_quad_classes(int B, int n, int ldy, const double *ymod, const double *yobs, const GaussSiteArgs &sites,
                                  const int32_t *class_of, int nclass, const double *rinv, int nsplit, double *partial,
                                  int32_t *work, hipStream_t stream);
struct LikeKernelArgs {
    int B, nt, ldy;
    const double *ymod; // [B][ldy]
    const int32_t *err_t; // [nt][B] per-target forward-model failure flags
    const double *noise; // [B][2*nt]
    LikeTargetDev t[8];
    double *logL;    // [B]
    double *misfits; // [B][nt+1]
    int32_t *err;    // [B]
};
void bh_launch_like(const LikeKernelArgs &a, hipStream_t stream);
// Which form a likelihood launch takes (every launcher of like_kernel.hip and like_kernel_m.hip): true = one wavefront per model --
// every target fits one wavefront, or comes with its sums already formed by the forward kernel (a receiver function's fused
// likelihood: nothing of its trace is read), and a Gauss law has its slab sums from the MFMA contraction; false = one workgroup per
// model, with *lds bytes of dynamic LDS for the in-kernel Gauss mat-vec.  (With a count table n is the capacity of the target's
// columns: a site's own count is at most that.)
inline bool bh_like_small_form(const LikeKernelArgs &a, size_t *lds)
{
    *lds = 0;
    bool small = true;
    for (int t = 0; t < a.nt; ++t) {
        if (a.t[t].law == 3 && a.t[t].quad == nullptr && (size_t)a.t[t].n * sizeof(double) > *lds) *lds = (size_t)a.t[t].n * sizeof(double);
        small = small && (a.t[t].n <= 64 || (a.t[t].pre != nullptr && a.t[t].law != 3)) && !(a.t[t].law == 3 && a.t[t].quad == nullptr);
    }
    return small;
}
// Likelihood kernel: LikeTargetDev::yobs / yerr_scaled / logdet_extra of target t become, for a model of site s,
// yobs + s * ldy + off, yerr_scaled + s * ldy + off (law 1) and logdet_extra[s * nt + t] (law 1).
struct LikeSiteArgs {
    const int32_t *site;         // device [B]: site of every model
    int nsites;
    const double *yobs;          // device [nsites][ldy]: observed data, targets in ymod's column order
    const double *yerr_scaled;   // device [nsites][ldy]: yerr / min(yerr) in the columns of law-1 targets (else unread)
    const double *logdet_extra;  // device [nsites][nt]: ln prod(yerr / min(yerr)) of law-1 targets (else unread)
};
void bh_launch_like_sites(const LikeKernelArgs &a, const LikeSiteArgs &sites, hipStream_t stream);
// ... with the sample count of every (site, target) from a table (bh_sites_set_x): LikeTargetDev::n is then the capacity of the
// target's columns.  n is uniform per workgroup / wavefront (one model each), the sums run over the site's first n samples in the
// order the kernels without the table use for that n.
struct LikeSiteXArgs : LikeSiteArgs {
    const int32_t *n; // device [nsites][nt]
};
void bh_launch_like_sites_x(const LikeKernelArgs &a, const LikeSiteXArgs &sites, hipStream_t stream);
// ... where a count may be 0: the site lacks the target (bh_sites_set_missing; like_kernel_m.hip, like_kernel.hip compiled with
// BH_LIKE_MISSING).  Such a target is skipped -- nothing of noise, yobs, ymod or its failure flag is read, nothing is added to logL
// or to the joint misfit, its own misfit is 0 -- so the sums are those of the present targets in their order.
void bh_launch_like_sites_m(const LikeKernelArgs &a, const LikeSiteXArgs &sites, hipStream_t stream);
// ... and a Gauss-law target's ln|R| (and, for the in-kernel mat-vec, R^-1) is that of the site's correlation class
// (bh_sites_set_gauss; like_kernel_c.hip, like_kernel.hip compiled with BH_LIKE_CLASSES on top of BH_LIKE_MISSING).  Per target of
// the call: class_of[t] null = no class table, the descriptor's values.  A class of -1 goes with a count of 0: skipped as above.
struct LikeClassArgs {
    const int32_t *class_of[8]; // device [nsites]
    const double *rinv[8];      // device [nclass][n][n]
    const double *logdet[8];    // device [nclass]
};
void bh_launch_like_sites_c(const LikeKernelArgs &a, const LikeSiteXArgs &sites, const LikeClassArgs &classes, hipStream_t stream);
// ... and every target's noise law is that of the model's site (bh_sites_set_laws, include/bh_engine_sites_laws.h; like_kernel_l.hip,
// like_kernel.hip compiled with BH_LIKE_LAWS on top of BH_LIKE_CLASSES).  LikeTargetDev::law of target t becomes law[site * nt + t]
// before the site's and the class's data are looked up, so law-1 and law-3 data are read by the site's law; the descriptor's law
// still decides the launch form and the LDS (bh_like_small_form).  An entry where the count is 0 is not read.  Law 3 stands only on
// a target whose descriptor is under law 3; LikeSiteXArgs::yerr_scaled / logdet_extra hold law-1 data wherever the TABLE says 1.
struct LikeLawArgs {
    const int32_t *law; // device [nsites][nt]
};
void bh_launch_like_sites_l(const LikeKernelArgs &a, const LikeSiteXArgs &sites, const LikeClassArgs &classes, const LikeLawArgs &laws,
                            hipStream_t stream);

void bh_launch_probe(int op, int n, const double *in, double *out, hipStream_t stream);

// ---- the site table's part of a fused call (bh_engine_impl.h: SiteTable; engine_eval.hip: plan_eval; DESIGN.md "The site table") ----
// How far the registered table lets the sites differ: every level admits what the one before it admits, and one thing more.
enum SiteLevel {
    SITES_NONE,          // no table
    SITES_SHARED,        // bh_sites_set: observed data per site; counts and periods are the descriptors'
    SITES_X,             // bh_sites_set_x: + counts and periods per site on fundamental-mode phase-velocity targets
    SITES_X_ALL,         // bh_sites_set_x_all: + on group-velocity and higher-mode targets
    SITES_MISSING,       // bh_sites_set_missing: + a count of 0, the site lacks the target
    SITES_MISSING_GAUSS, // bh_sites_set_missing_gauss: + on a Gauss-law target
    SITES_AXES           // bh_sites_set_axes: + a receiver function's count anywhere in 0 .. its descriptor's n
};
// The likelihood launcher of a fused call: bh_launch_like, _sites, _sites_x (a site's own sample counts), _sites_m (counts that may
// be 0), _sites_c (a Gauss-law target's ln|R| and R^-1 from its correlation classes), _sites_l (every target's law from the law table)
enum EvalLike { LIKE_PLAIN, LIKE_SITES, LIKE_SITES_X, LIKE_SITES_M, LIKE_SITES_C, LIKE_SITES_L };
// The contraction of a Gauss-law target: with the descriptor's data and matrix, with every model's site's data, or with the matrix
// of every model's correlation class as well (bh_sites_set_gauss)
enum EvalGauss { GAUSS_PLAIN, GAUSS_SITES, GAUSS_CLASSES };
// Why a fused call is refused, in the order of precedence (bh_plan_sites reports the first that holds)
enum SiteRefusal {
    REFUSE_NONE,
    REFUSE_NO_FORWARD,           // a target has no forward model to run
    REFUSE_RF_NEEDS_TABLE,       // counts that may be 0, a receiver-function target, no bh_sites_set_rf
    REFUSE_RF_AXIS_NEEDS_TABLE,  // a receiver function's counts differ from its descriptor's, no bh_sites_set_rf_axis
    REFUSE_GAUSS_NEEDS_TABLE,    // a Gauss-law target some site lacks has no class table
    REFUSE_LAW_GAUSS_NEEDS_TABLE,     // the law table has a present site under another law on a Gauss-law target without class table
    REFUSE_RF_AXIS_GAUSS_NEEDS_TABLE, // a Gauss-law receiver function with its own counts has no class table
    REFUSE_RF_AXIS_NO_MFMA       // ... or runs the BH_NO_MFMA in-kernel mat-vec
};
// What bh_plan_sites is asked: the call, the table in force and, per registered target, what the tables say of it.
struct SitePlanAsk {
    bool sites;              // bh_evaluate_sites (false: bh_evaluate_batch, which reads no table)
    int level;               // SiteLevel
    bool rf, rf_axis, laws;  // the tables of bh_sites_set_rf, bh_sites_set_rf_axis, bh_sites_set_laws are in force
    bool no_mfma;            // the Gauss law runs the in-kernel mat-vec (BH_NO_MFMA)
    int nt;
    struct Target {
        int kind, law;       // the descriptor's
        bool lacks;          // a site has count 0 for the target
        bool rf_own_counts;  // receiver function: a count is neither 0 nor the descriptor's
        bool law_other;      // the law table has a present site under another law than BH_LAW_GAUSS
        bool classes;        // the target has a class table (bh_sites_set_gauss)
    } t[8]; // (BH_MAX_TARGETS, as LikeKernelArgs::t)
};
// The site part of a fused call's plan: which tables its launches read, and the one refusal.
struct SitePlan {
    bool x_table, rf_table;  // the table's periods and counts (bh_sites_set_x) / receiver-function parameters (bh_sites_set_rf) are in force
    bool x_all;              // ... the periods of group-velocity targets too: their second roots read the table (bh_sites_set_x_all)
    bool missing;            // the table's counts may be 0: the receiver-function and likelihood builds that skip
    bool rf_axis;            // the sites' own time axes and filters are in force: the builds of bh_launch_rf_t
    bool laws;               // the sites' own noise laws are in force
    EvalLike like;
    EvalGauss gauss[8];      // (read for the Gauss-law targets)
    bool desc_counts;        // LIKE_SITES_C without a registered count table: the likelihood reads the descriptors' counts as one
    int refusal, code;       // SiteRefusal and its error code (BH_OK: none)
};
// Pure: no HIP call, no engine.  The precedence among the refusals is the order of SiteRefusal.
SitePlan bh_plan_sites(const SitePlanAsk &q);
const char *bh_site_refusal_text(int refusal); // the message of a SiteRefusal ("" for REFUSE_NONE)

// ---- the ellipticity target of a fused call (include/bh_engine_ellip_target.h; swd_ellip.hip, run_forward) ----
// One BH_TARGET_ELLIP target: a lane per (model, period) reads its velocity from vel (row stride ldvel: the columns of the
// dispersion target it shares the search with, or its own search's workspace), evaluates and polishes as bh_swd_ellip does, and
// writes y = the header's transform of hv -- 0.0 where that is not finite -- to y (the target's columns of ymod, row stride ldy).
// err_row: the target's row of err_t, which holds the search's failure flags when the kernel starts; a lane whose entry raises
// bh_swd_ellip's flag, or whose y is not finite, ORs 1 into its model's word.
struct EllipFusedArgs {
    int B, Lmax, K, nsteps, is_signed, zh;
    const int32_t *nlay;
    const double *h, *vp, *vs, *rho; // device
    ptrdiff_t sl, sb;
    const double *periods;           // [K] device
    const double *vel; int ldvel;
    double *y; int ldy;
    int32_t *err_row;
    // Periods per site (include/bh_engine_sites_ellip.h; site != null: the site build).  K is the CAPACITY of the target's columns and
    // `periods` is not read: model b of site s = site[b] has the xn[s * ldn] periods xper[s * ldx ...] -- the count table's and the
    // period table's column of the target.  A lane at or beyond its model's count (count 0: the site lacks the target) or of a site
    // out of range writes 0.0, raises no flag and evaluates nothing.
    const int32_t *site = nullptr; int nsites = 0;
    const int32_t *xn = nullptr; int ldn = 0;
    const double *xper = nullptr; int ldx = 0;
};
void bh_launch_ellip_fused(const EllipFusedArgs &a, hipStream_t stream);

// out = [val n][bound n][certified n]

// the engine as other translation units reach it (bh_engine.hip; posterior_kernel.hip, include/bh_engine_posterior.h)
struct bh_engine;
__attribute__((visibility("hidden"))) int bh_engine_fail_internal(bh_engine *e, int code, const char *what); // sets last_error
__attribute__((visibility("hidden"))) int bh_engine_device_internal(const bh_engine *e);

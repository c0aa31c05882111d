/*
 * include/bh_engine_debug.h -- measurement, diagnostic and experiment entry points of libbh_engine.so.
 *
 * NOT part of the drop-in contract (include/bh_engine.h): nothing here changes a result a caller of bh_engine.h sees, and a
 * BayHunter binding needs none of it.  bench.py, tools/ and the tests use it: launch-geometry knobs of the layer-parallel
 * dispersion kernel, the experiment switches (csrc/bh_tuning.h), HIP-event timing and evaluation counters, probes of the device
 * math library.  May change between ABI versions without notice.
 */
#ifndef BH_ENGINE_DEBUG_H
#define BH_ENGINE_DEBUG_H

#include "bh_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knob: lanes of a wavefront that cooperate on ONE model in the dispersion kernel
 * (1..32; 0 = choose from the batch size and layer count, the default).  Results do not depend on it. */
int bh_engine_set_swd_group(bh_engine *e, int lanes_per_model);
/* Tuning knob: trial phase velocities evaluated per round of the root search in the dispersion
 * kernel (1..16; 0 = choose from the batch size, the default; with one lane per model -- group 1 -- the
 * largest power of two not above it is used).  The search (surfdisp96.f:390-686) asks
 * for one secular-function value at a time; with look-ahead the kernel also evaluates, on further
 * lanes, the velocities the search will most probably ask for next and hands them over if and only
 * if it does.  Results do not depend on it. */
int bh_engine_set_swd_lookahead(bh_engine *e, int trials_per_round);

/* Which dispersion kernel the most recent call with dispersion targets launched (diagnostic; -1: none yet):
 *   BH_KERNEL_GROUP  several lanes per model, layer-parallel (swd_group_kernel),
 *   BH_KERNEL_LANE   one lane per evaluation, reference-exact or FA builds (swd_kernel),
 *   BH_KERNEL_LEAN   one lane per trial velocity with the fast arithmetic (swd_lean_kernel): BH_SEARCH_FAST + BH_ARITH_FAST
 *                    calls whose targets are all fundamental-mode phase velocities, in arrays of up to 32 layers.  It
 *                    evaluates 64 trial velocities per model and round in calls of up to 1024 (model, target) pairs, 32 up
 *                    to 5120, 16 up to 10240, 8 up to 28672 and 4 beyond; a model's velocities depend on that number in their last bits (~1e-9 relative; a
 *                    model whose guard fires under one count and not under another: the reference's 1e-6) and on nothing
 *                    else about the call. */
#define BH_KERNEL_GROUP 0
#define BH_KERNEL_LANE 1
#define BH_KERNEL_LEAN 2
int bh_engine_last_swd_kernel(const bh_engine *e);

/* Every dispersion kernel launch of the most recent call with dispersion targets (diagnostic; filled on the host from the launch
 * plans, in launch order).  family: BH_KERNEL_*; role: BH_SWD_MAIN (the call's targets), BH_SWD_RERUN (the models the guard of
 * the short refinement listed, again with the reference's sequence), BH_SWD_SECOND (the second roots of split group velocities).
 * key: the template arguments of the instantiation launched --
 *   BH_KERNEL_GROUP  FASTM, SIMPLE, PROF, ADAPT, CNTB, FA   (swd_group_kernel)
 *   BH_KERNEL_LANE   IFUNC, LOOK, WPB, FAST, SIMPLE, FA     (swd_kernel)
 *   BH_KERNEL_LEAN   J, CNT, 0, 0, 0, 0                     (swd_lean_kernel)
 * and the launch's features: two depth classes, two targets interleaved in one grid, the SIMD-pairing order of the models,
 * restart in place of guarded models, workgroups in x, the priority time slice of the lane kernel and of the trial-per-lane
 * kernel's launches of one Rayleigh and one Love wavefront per SIMD (log2 cycles; 0 = none).
 * Writes at most `max` records and returns their number in *n. */
typedef struct {
    int family, role, key[6];
    int two_classes, interleaved, pair_order, restart, grid_x, fair;
} bh_swd_launch;
#define BH_SWD_MAIN 0
#define BH_SWD_RERUN 1
#define BH_SWD_SECOND 2
int bh_engine_last_swd_launches(const bh_engine *e, bh_swd_launch *out, int max, int *n);

/* How the most recent call with dispersion targets ordered its models (diagnostic; scheduling only, -1: no engine).  Returns the
 * plan's order: BH_ORDER_NONE the caller's, BH_ORDER_DEPTH deepest first, BH_ORDER_LENGTH by predicted search length (the
 * trial-per-lane kernel), BH_ORDER_PAIR by predicted search length, paired over the SIMDs (the group kernel).
 * *workgroups: of the launch that computed it -- 0 none, 1 one workgroup over the batch, 8 one per XCD block of a blocked order.
 * *fills: what that launch zeroed for the call in place of fill dispatches of their own (BH_ORDER_LENGTH and BH_ORDER_PAIR: the
 * launch is the call's prologue) -- a sum of BH_FILL_GUARD (the head of the short refinement's guard lists), BH_FILL_FLAGS (the
 * per-target failure flags: once per layout of the call) and BH_FILL_COUNTERS (the evaluation counters, when counting is on). */
#define BH_ORDER_NONE 0
#define BH_ORDER_DEPTH 1
#define BH_ORDER_LENGTH 2
#define BH_ORDER_PAIR 3
#define BH_FILL_GUARD 1
#define BH_FILL_FLAGS 2
#define BH_FILL_COUNTERS 4
int bh_engine_last_swd_order(const bh_engine *e, int *workgroups, int *fills);
/* The processing order the most recent call with dispersion targets computed for target 0 / 1 of its launch (diagnostic): entry
 * w * m + i of out[0 .. B) is the model that wavefront w of the target takes as its i-th (m models per wavefront).  Returns B, 0
 * where the call kept the caller's order (BH_ORDER_NONE), a negative BH_E* for a bad argument (n < B).  Waits for the stream. */
int bh_engine_last_swd_perm(bh_engine *e, int target, int32_t *out, int n);

/* The bracket scan of Love targets (any root refinement).  Results never depend on this setting.
 * getsol's scan (surfdisp96.f:437-460) evaluates every step of its grid until the secular function changes sign.  For Love
 * waves the number of sign changes below a trial velocity is read off the recursion that evaluates the function (a Sturm
 * count), so two evaluations prove that the steps between them hold no sign change (they are skipped) or exactly one (it is
 * located by a search over the step index).  Grid points, bracket and every bit after it are the reference's.
 *   BH_SCAN_STEPS    every step evaluated, as the reference does.
 *   BH_SCAN_COUNTED  the counted scan wherever a launch holds a Love target -- except launches of several models per
 *                    wavefront that mix both root refinements (that kernel build does not carry it).
 *   BH_SCAN_AUTO     (default) the counted scan in the launches where it is measured to pay (docs/HISTORY.md 3.1a).
 * Rayleigh targets always step; the trial-per-lane kernel (BH_KERNEL_LEAN) steps for both wave types, sixteen steps a round. */
#define BH_SCAN_STEPS 0
#define BH_SCAN_COUNTED 1
#define BH_SCAN_AUTO 2
int bh_engine_set_swd_scan(bh_engine *e, int scan);
int bh_engine_get_swd_scan(const bh_engine *e);

/* Experiment switches (csrc/bh_tuning.h lists them: name, environment variable, default, meaning).  They change scheduling
 * and launch geometry, never a result.  The table is filled once per process from the environment; this call changes one
 * entry for the calls that follow (process-wide).  BH_EINVAL for an unknown name, and always in a build with
 * -DBH_NO_EXPERIMENTS.  Not needed by a caller that only wants results. */
int bh_engine_set_tuning(bh_engine *e, const char *name, int value);
int bh_engine_get_tuning(bh_engine *e, const char *name, int *value);

/* ---- diagnostics -------------------------------------------------------------------------
 * Evaluate one elementary function on the device for n float64 inputs (host pointers):
 * op 0 sqrt, 1 sin, 2 cos, 3 exp, 4 log, 5 1/x; op 6 / 7: in holds n pairs (a, b), out[i] = a/b
 * through the shared-reciprocal sequence of the kernels (6) or the plain operator (7); op 8 / 9 / 10:
 * sin / cos / exp through the kernels' glibc-exact restatement (csrc/bh_libm.h).  Used by the tests to document how far the
 * device math library is from the host's libm (SURVEY.md 7 "FMA contraction & device libm").
 * Ops 11-16 run the receiver-function synthesis kernel's own fast functions (csrc/rf_kernel.hip, the same inlined text and
 * compile flags): 11 rcp_nr (1/x: hardware seed + one Newton step), 12 rsq_nr (1/sqrt(x), x > 0), 13 / 14 sin / cos of
 * sincos_cw (Cody-Waite reduction, meant for |x| < 2^20), 15 exp_cw (clamped to [-800, 800]; NaN passes through),
 * 16 csqrt_f (principal complex square root): in and out hold n / 2 pairs (re, im), n even.
 * Ops 17-23 run the dispersion kernels' fast arithmetic (namespace fa of csrc/swd_fa.h, compiled in csrc/swd_fa_probe.hip with the
 * flags of the trial-per-lane kernel): 17 rcp (1/x: hardware seed + two Newton steps), 18 rcp1 (one step), 19 / 20 the s = sqrt(x)
 * and rs = 1/sqrt(x) of sqrt_rsqrt (x > 0, normal), 21 / 22 sin / cos of sincos (0 <= x <= 9e4), 23 expneg: out = e^-in
 * (0 <= in <= 700).  BH_EINVAL for any other op (negative, or 24 and beyond). */
int bh_probe_math(bh_engine *e, int op, int n, const double *in, double *out);

/* The secular function of ONE model at n points, evaluated by the dispersion kernels' own code (csrc/swd_fa_probe.hip): lane i
 * returns the value at wavenumber wvno[i] and angular frequency omega[i] (host pointers).  ifunc: 1 Love, 2 Rayleigh.  The model
 * is mtop rows of d, a, b, rho (thickness, vp, vs, density; binary32 as at the f2py boundary), the first mmax of them its layers
 * (the last one the half-space); rows mmax .. mtop - 1 are the ragged filler of a batch and are read by no evaluator.  No water
 * layer (llw = 1).  evaluator:
 *   0  the exact evaluators of csrc/swd_common.h (rayleigh_secular<true> / love_secular<true>: the reference's operations, the
 *      glibc-exact libm tables staged in LDS as the kernels stage them),
 *   1  fa::rayleigh_secular / fa::love_secular (csrc/swd_fa.h): what the FA builds of the lane kernel call,
 *   2  lean_rayleigh / lean_love over a LeanModel (csrc/swd_lean.hip: reciprocal rows by fa::rcp, a normalisation every second
 *      layer): what the trial-per-lane kernel calls.
 * Every evaluator returns the first entry of the surface vector scaled by the vector's max-norm (e1 / max(|e1|, |e2|) for Love,
 * e[0] / max |e| for Rayleigh).  BH_EINVAL -- with `out` untouched -- for another evaluator or wave type, mmax < 2, mmax > mtop,
 * mtop > 32 with evaluator 2 (the lean kernel's arrays) or > 100 (the Fortran's limit, surfdisp96.f:59) with the others.
 * The group kernel's layer-parallel FA build (swd_group_kernel<FA>) is NOT probed: its evaluation is spread over the lanes of a
 * group and cannot be separated from its kernel; it stays covered end to end (tests/test_gpu_swd_lean.py, test_gpu_swd.py). */
int bh_probe_swd_secular(bh_engine *e, int evaluator, int ifunc, int mmax, int mtop, const float *d, const float *a, const float *b,
                         const float *rho, int n, const double *wvno, const double *omega, double *out);

/* Instrumentation (off by default; bench.py and the tests turn it on).
 *   timing:   HIP events are recorded on the stream the kernels are launched on, around each
 *             kernel family of every *_batch call made after bh_timing_reset().  Nothing is
 *             synchronised until bh_timing_collect(), which waits for the events and returns the
 *             number of calls, the SUM over those calls of the span first-kernel-start ->
 *             last-kernel-end (total_ms) and of the time inside each kernel family:
 *             family_ms[0] dispersion (swd), [1] receiver function, [2] likelihood.
 *   counting: the dispersion kernels add up their secular-function evaluations; bh_last_neval()
 *             returns the count of the most recent call (the flop model of SURVEY.md 8(d) is
 *             layer-propagator steps = evaluations x (nlay-1)). */
int bh_engine_set_instrumentation(bh_engine *e, int timing, int counting);
int bh_timing_reset(bh_engine *e);
int bh_timing_collect(bh_engine *e, int *ncalls, double *total_ms, double family_ms[3]);
/* Per-call timing of the calls since bh_timing_reset(), from the same events: step_ms[i] = start of call i -> start of
 * call i+1 (back-to-back calls: one "step" each, gaps included), for the last call its own span.  Writes at most
 * `max` entries and returns their number in *n.  (No further events: a marker recorded on the launch stream between
 * two calls changes how the next call's two lane-kernel launches pair up on the SIMDs -- 8.1 -> 10.6 ms at B = 16 384.) */
int bh_timing_steps(bh_engine *e, int max, double *step_ms, int *n);
int bh_last_neval(bh_engine *e, uint64_t *neval);
/* raw counter block of the last counted call: [0] secular evaluations, [1..3] / [4..6] wave-cycles per phase
 * (development aid), [7] wavefronts, [8] / [9] evaluations of the Rayleigh / Love targets, [10] / [11] their
 * layer-propagator steps (evaluations x finite layers: the flop model of the roofline block in bench.py) */
int bh_debug_counters(bh_engine *e, uint64_t out[16]);
/* development aid: one record of 4 words per traced wavefront of the last counted dispersion launch
 * (start, end [100 MHz ticks], core cycles, rounds | wave type << 32 | HW_ID << 36); counter [7] = wavefronts */
int bh_debug_trace(bh_engine *e, uint64_t *out, int nwaves);
/* development aid: the models (batch indices, in no particular order) that the guard of the short refinement listed for the
 * re-run launch of the most recent dispersion call, for the target-th dispersion target of that call; B: that call's batch
 * size.  Writes at most `max` entries and returns their number in *n. */
int bh_debug_guard_list(bh_engine *e, int target, int B, int32_t *out, int max, int *n);


#ifdef __cplusplus
}
#endif
#endif

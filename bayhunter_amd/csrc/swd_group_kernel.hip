// bayhunter_amd/csrc/swd_group_kernel.hip -- Rayleigh/Love dispersion with G lanes per model (small batches).
// Same search, same bits as swd_kernel.hip (one lane per model); see the block comment at the kernel.
// Built with -mllvm -disable-machine-licm (Makefile): the round loop carries ~60 distinct f64 constants of the
// glibc-exact sincos / exp; hoisted out of the loop they cost more registers than the kernel has.
#include "../../include/bh_engine_debug.h"
#include "bh_device.h"
#include "bh_tuning.h"
#include <algorithm>
#include <cassert>
#include <type_traits>
#define BH_HD __device__ __forceinline__
#define BH_TAB static __device__ const
#include "bh_libm.h"

namespace {
#include "swd_common.h"

// =================================================================================================
// Kernel 2: G lanes = one model (64/G models per wavefront), G chosen at launch time.
// For batches that cannot fill the chip with one lane per model (B = 4096 gives only 64
// wavefronts for 1024 SIMDs) the work of ONE secular evaluation is spread over the G lanes of
// the model's group:
//   phase A  lane li computes the layer terms of layers li, li+G, ... (the transcendental-heavy
//            part: sqrt, sin/cos or exp, the compound-matrix entries) and parks them in LDS;
//   phase B  the strictly sequential bottom-up recursion over the parked layers.
//            Rayleigh, G >= 5: lane li owns component (li mod 5) of the 5-vector: it forms
//            ee(i) = sum_j e(j)*ca(j,i) from column i of the parked matrix, the five values are
//            exchanged through LDS, every lane takes the max-norm, divides its own component and
//            the normalised vector is exchanged again.  Otherwise (Love, or G < 5) every lane of
//            the group runs the whole recursion redundantly.
//            Either way all lanes of a group end up with the same secular value and step the
//            same search state; no broadcast is needed.
// Every floating-point operation and its order are those of kernel 1: the kernels return
// identical bits.  All dispersion targets of a call go into one launch (blockIdx.y = target),
// so Rayleigh and Love wavefronts share the chip.
// A workgroup is GROUP_WPB independent wavefronts that only share the LDS copy of the libm tables;
// after start-up there is no barrier: LDS operations of a wavefront execute in order, wave_sync()
// only pins the compiler's ordering.  Look-ahead, Love's in-group trials, the processing order and the
// two depth classes of ragged batches are described at their code.
// =================================================================================================
constexpr int CA_STRIDE = 26;
constexpr int LOVE_TERMS = 6; // doubles per parked Love layer and trial (5 used): up to 4 trials share a row

// Phase B of the group kernel, Rayleigh.  `cam` = this model's parked layers (column-major
// 5x5 each), e = half-space vector on entry / surface vector on exit.
//   PAR5   lane owns component `col`: one dot product per layer, the five results are exchanged
//          with ds_bpermute (faster than an LDS write/read round trip: 56 vs 116 cycles) and every
//          lane normalises all five itself -- one exchange per layer, no branch.
//   !PAR5  every lane runs the full 5x5 product (used for G < 5 and for the exact re-run).
//   RAGGED the wavefront holds models with different layer counts (or a water layer): layers a
//          model does not have are masked with selects; the uniform case has no masking at all.
template <bool PAR5, bool RAGGED, bool EXACT, bool FA = false>
__device__ __forceinline__ void rayleigh_chain_group(double e[5], const double *cam, int col,
                                                     int gbase, int mtop, int mmax, int llw,
                                                     DivRange &dr)
{
    // uniform wavefronts: the layer count is the same in every lane -> scalar loop control
    const int mstart = (RAGGED ? mtop : __builtin_amdgcn_readfirstlane(mmax)) - 2;
    if (PAR5) {
        // software-pipelined: the column of layer m-1 is fetched while layer m is exchanged
        const double *cc = cam + (size_t)(mstart > 0 ? mstart : 0) * CA_STRIDE + 5 * col;
        double c0 = cc[0], c1 = cc[1], c2 = cc[2], c3 = cc[3], c4 = cc[4];
#pragma unroll 3
        for (int m = mstart; m >= 0; --m) {
            const bool on = !RAGGED || (m <= mmax - 2 && m >= llw - 1);
            const double *cn = cam + (size_t)(m > 0 ? m - 1 : 0) * CA_STRIDE + 5 * col;
            double n0 = cn[0], n1 = cn[1], n2 = cn[2], n3 = cn[3], n4 = cn[4];
            double ee = 0.0;
            if (FA) { // (fast arithmetic: two short chains of fused multiply-adds)
                ee = __builtin_fma(e[4], c4, __builtin_fma(e[2], c2, e[0] * c0)) + __builtin_fma(e[3], c3, e[1] * c1);
            } else {
                ee = ee + e[0] * c0;
                ee = ee + e[1] * c1;
                ee = ee + e[2] * c2;
                ee = ee + e[3] * c3;
                ee = ee + e[4] * c4;
            }
            const double v0 = __shfl(ee, gbase + 0), v1 = __shfl(ee, gbase + 1), v2 = __shfl(ee, gbase + 2),
                         v3 = __shfl(ee, gbase + 3), v4 = __shfl(ee, gbase + 4);
            // keep the fetch of layer m-1 in THIS iteration (the compiler otherwise sinks it to the top of the next
            // one and waits for it there: ~100 cycles of the ~600 a layer takes); LDS returns in order, so by the
            // time the exchange above has arrived these have as well
            asm volatile("" : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3), "+v"(n4));
            double en[5];
            if (FA) {
                fa::normalize5(v0, v1, v2, v3, v4, en);
            } else {
                DivRange d2 = dr;
                normalize5<EXACT>(v0, v1, v2, v3, v4, en, d2);
                if (on) dr = d2;
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] = on ? en[i] : e[i];
            c0 = n0; c1 = n1; c2 = n2; c3 = n3; c4 = n4;
        }
    } else {
        for (int m = mstart; m >= 0; --m) {
            const bool on = !RAGGED || (m <= mmax - 2 && m >= llw - 1);
            const double *cc = cam + (size_t)m * CA_STRIDE;
            double ee[5], en[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                double acc = 0.0;
                if (FA) {
                    acc = __builtin_fma(e[4], cc[5 * i + 4], __builtin_fma(e[2], cc[5 * i + 2], e[0] * cc[5 * i])) +
                          __builtin_fma(e[3], cc[5 * i + 3], e[1] * cc[5 * i + 1]);
                } else {
#pragma unroll
                    for (int j = 0; j < 5; ++j) acc = acc + e[j] * cc[5 * i + j];
                }
                ee[i] = acc;
            }
            if (FA) {
                fa::normalize5(ee[0], ee[1], ee[2], ee[3], ee[4], en);
            } else {
                DivRange d2 = dr;
                normalize5<EXACT>(ee[0], ee[1], ee[2], ee[3], ee[4], en, d2);
                if (on) dr = d2;
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] = on ? en[i] : e[i];
        }
    }
}

// Phase B of the group kernel, Love: parked per layer (cosq, y, z, xmu, rcp(xmu)).
template <bool RAGGED, bool EXACT, bool COUNT, bool FA = false>
__device__ __forceinline__ void love_chain_group(double &e1, double &e2, const double *cam, int mtop,
                                                 int mmax, int llw, DivRange &dr, LoveCount &lc)
{
    const int mstart = (RAGGED ? mtop : __builtin_amdgcn_readfirstlane(mmax)) - 2;
    // software-pipelined: the terms of layer m-1 are fetched while layer m is processed
    const double2 *src = reinterpret_cast<const double2 *>(cam + (size_t)(mstart > 0 ? mstart : 0) * CA_STRIDE);
    double2 p0 = src[0], p1 = src[1], p2 = src[2];
#pragma unroll 3
    for (int m = mstart; m >= 0; --m) {
        const bool on = !RAGGED || (m <= mmax - 2 && m >= llw - 1);
        const double2 *nx = reinterpret_cast<const double2 *>(cam + (size_t)(m > 0 ? m - 1 : 0) * CA_STRIDE);
        const double2 q0 = nx[0], q1 = nx[1], q2 = nx[2];
        double n1 = e1, n2 = e2;
        DivRange d2 = dr;
        if (FA) fa::love_step(n1, n2, p0.x, p0.y, p1.x);
        else love_step<EXACT>(n1, n2, p0.x, p0.y, p1.x, p1.y, p2.x, d2);
        if (on) {
            if (COUNT) lc.layer(p2.y, e2, n2); // (p2.y: floor(q / pi) of the layer, parked by phase A)
            e1 = n1;
            e2 = n2;
            dr = d2;
        }
        p0 = q0; p1 = q1; p2 = q2;
    }
}
 // doubles per parked layer: 25 (Rayleigh, column-major 5x5) / 4 (Love)

__device__ __forceinline__ void park_ca25(double *dst, const Ca19 &c)
{
    // column i (0-based) at dst[5*i + j] = ca(j+1, i+1)
    const double ca11 = c.c[0], ca12 = c.c[1], ca13 = c.c[2], ca14 = c.c[3], ca15 = c.c[4];
    const double ca21 = c.c[5], ca23 = c.c[6], ca24 = c.c[7], ca22 = c.c[8];
    const double ca41 = c.c[9], ca42 = c.c[10], ca43 = c.c[11], ca51 = c.c[12], ca53 = c.c[13];
    const double ca31 = c.c[14], ca32 = c.c[15], ca33 = c.c[16], ca34 = c.c[17], ca35 = c.c[18];
    double2 *d2 = reinterpret_cast<double2 *>(dst);
    d2[0] = make_double2(ca11, ca21);  d2[1] = make_double2(ca31, ca41);   // col 1: 11 21 31 41 51
    d2[2] = make_double2(ca51, ca12);  d2[3] = make_double2(ca22, ca32);   // col 2: 12 22 32 42 52
    d2[4] = make_double2(ca42, ca41);  d2[5] = make_double2(ca13, ca23);   // (ca52 = ca41) col 3: 13 23 33 43 53
    d2[6] = make_double2(ca33, ca43);  d2[7] = make_double2(ca53, ca14);   // col 4: 14 24 34 44 54
    d2[8] = make_double2(ca24, ca34);  d2[9] = make_double2(ca22, ca21);   // (ca44 = ca22, ca54 = ca21)
    d2[10] = make_double2(ca15, ca14); d2[11] = make_double2(ca35, ca12);  // col 5: 15 25 35 45 55
    d2[12] = make_double2(ca11, 0.0);                                      // (ca25=ca14, ca45=ca12, ca55=ca11)
}

// Wavefronts per workgroup: they are independent (no barrier after start-up) and only share one LDS
// copy of the libm tables, which is what lets 8 wavefronts fit a CU's 160 KB of LDS.
constexpr int GROUP_WPB = 2;
constexpr unsigned PRIO_BLOCK = 8; // rounds between priority decisions (power of two)
constexpr int LIBM_TAB_PAD = (LIBM_TAB_BYTES + 15) & ~15;

// LDS ordering inside ONE wavefront: its LDS instructions execute in order, so a write by one lane is
// visible to a later read by another lane of the same wavefront; only the compiler must not reorder.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// WPB = wavefronts per workgroup (they only share the libm tables): 2 by default; 4 when receiver-function workgroups
// are to run beside the kernel -- a CU's eight wavefronts then hold two copies of the tables instead of four, which is
// what leaves a CU's LDS room for one RF workgroup (bh_engine.hip: co-resident receiver function).
// FAST: the build with the short refinement (SearchT<.., FAST>, swd_common.h) for the phase-velocity targets.
// PROF: the build with the evaluation counters, phase clocks and wavefront trace (launches with A.neval set).
// ADAPT: a launch of ONE model per wavefront (a chain window, a single model): every wavefront sizes its lane groups and its
// trials per round for its OWN model -- a lane per finite layer (8 ... 16), as many trials as lanes and the wavefront's LDS
// region admit (at most ADAPT_MAX_TRIALS), LDS rows for the model's own layers instead of the arrays' capacity.  With the
// capacity's rows (21 for the chains) four trials fit; a window's dispersion time falls with every further trial
// (4 / 6 / 8 trials: 1.82 / 1.53 / 1.42 ms for 1016 models of 3-9 layers), so the shallow models of a window get eight,
// its deep ones keep four.  Scheduling only: which values the search consumes does not depend on it.
constexpr int ADAPT_MAX_TRIALS = 8;
// CNTB: the build with the counted scan of Love targets (SearchT, swd_common.h: same brackets, same bits, a third of the scan's
// evaluations).  Its state machine and the mode count in Love's recursion cost every wavefront of the launch a little (code
// size, scalar registers), so it is compiled into the launches where it pays -- one model per wavefront (ADAPT: a single
// model, the chains' windows), launches of Love targets only -- and not where Rayleigh wavefronts set the time anyway
// (c2: Rayleigh + Love at B = 4096: 3.37 ms without, 3.47 with; the Rayleigh wavefront alone on its SIMD takes 3.06).
// FA: the build with the fast arithmetic (swd_fa.h; bh_engine_set_swd_arith): launches in which every target takes the short
// refinement (FASTM = 2) -- tolerance-level parity, a guard for signs the rounding error could decide.
// (the FA builds are compiled in a translation unit of their own, swd_group_fa.hip, which includes this file: own flags)
#ifndef BH_GROUP_WAVES
#define BH_GROUP_WAVES 2
#endif
// 1: the SITE-PERIOD builds (swd_group_x.hip includes this file once per translation unit's list of builds): a model's period
// list and count are its site's (SwdSiteXArgs, bh_device.h).  The wavefront stages a row of T.K (the capacity) periods for each
// of its models and SearchT -- which always held K and the period pointer per lane -- gets its model's; nothing else differs, so a
// model gets the bits of a launch whose target has its site's periods.  0: the builds this file always had, the same machine code.
#ifndef BH_SWD_SITEX
#define BH_SWD_SITEX 0
#endif
template <int WPB, int FASTM, bool SIMPLE, bool PROF, bool ADAPT, bool CNTB, bool FA = false>
#if BH_SWD_SITEX
__global__ __launch_bounds__(BH_WAVE * WPB) __attribute__((amdgpu_waves_per_eu(BH_GROUP_WAVES, BH_GROUP_WAVES))) void swd_group_kernel(SwdMultiArgs A, int Gflags, int wave_lds, SwdSiteXArgs X)
#else
__global__ __launch_bounds__(BH_WAVE * WPB) __attribute__((amdgpu_waves_per_eu(BH_GROUP_WAVES, BH_GROUP_WAVES))) void swd_group_kernel(SwdMultiArgs A, int Gflags, int wave_lds)
#endif
{
    // "this workgroup is resident": what a second stream waits for before it dispatches wavefronts beside these
    if (A.started != nullptr && threadIdx.x == 0) atomicAdd(A.started, 1u);
    const int cls = (A.split != nullptr) ? (int)blockIdx.z : 1; // 0 = the deep models of a ragged batch, 1 = the rest
    // Wavefront -> (target, index).  Two targets in a one-dimensional grid are INTERLEAVED wavefront by wavefront in
    // proportion to their wavefront counts, so that every CU gets its share of both: dispatched target after
    // target, the Rayleigh wavefronts fill whole CUs before the first Love wavefront starts, and a CU of eight
    // Rayleigh wavefronts runs them up to 30 % slower than a mixed one (LDS traffic: 150 LDS instructions per
    // Rayleigh round, 61 per Love round).  A workgroup's wavefronts only share the libm tables.
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / BH_WAVE));
    // PASSES (the re-run of the models a guard listed, one model per wavefront, reference sequence): the launch is a SMALL grid
    // (bh_plan_swd_group: bh_tuning.h swd_rerun_wgs = 256 per target) whose workgroups stride over the list, whose length lives on
    // the device -- nearly always it is empty or a handful of models, and a launch sized for the worst case (one wavefront per
    // model of the batch: 2048 workgroups at B = 4096) had to be dispatched workgroup by workgroup only to leave at once (4.5 us
    // alone, 0.2 ms when receiver-function workgroups of the other stream were waiting for the same wave slots).
    constexpr bool PASSES = ADAPT && FASTM == 0;
    int pass = 0;
next_pass:
    const int wg_x = (int)blockIdx.x + ((PASSES && A.rerun != 0) ? pass * (int)gridDim.x : 0);
    int wid = wg_x * WPB + wave, ty = (int)blockIdx.y;
    bool beyond = false; // (interleaved grid: a last, odd wavefront may have nothing to do)
    if (A.wg_n1 > 0) {
        const long long n1 = A.wg_n1, N = (long long)A.wg_n0 + n1;
        beyond = wid >= (int)N;
        const int l0 = (int)(((long long)wid * n1) / N), l1 = (int)((((long long)wid + 1) * n1) / N);
        ty = (l1 > l0) ? 1 : 0;
        wid = (l1 > l0) ? l0 : wid - l0;
    }
    int G = A.lanes[cls];
    const SwdTarget T = A.t[ty];
    int nlist = A.B; // entries of the processing order this launch covers
    if (T.count != nullptr) { // (a re-run of listed models: the count lives on the device)
        const int c = *T.count;
        nlist = c < nlist ? c : nlist;
    }
    int J = T.look > 1 ? T.look : 1; // look-ahead: trial velocities per round (per target), one lane group each
    int rows_own = 0;
    if (ADAPT) { // (one class, one model per wavefront: wavefront `wid` has model `wid` of the processing order)
        const int32_t *perm0 = T.perm != nullptr ? T.perm : A.perm;
        const bool v0 = !beyond && wid < nlist;
        int m0 = v0 ? A.nlay[perm0 ? perm0[wid] : wid] : 2;
        m0 = __builtin_amdgcn_readfirstlane(m0);
        m0 = m0 < 2 ? 2 : (m0 > A.rows[1] ? A.rows[1] : m0);
        const int fin = m0 - 1;
        G = fin < 8 ? 8 : (fin > 16 ? 16 : fin);
        const int fixed = (2 * NEV_MAX + ((T.K + 1) & ~1)) * (int)sizeof(double) + ((4 * m0 * (int)sizeof(float) + 15) & ~15) + 64;
        const int jl = (wave_lds - fixed) / (fin * CA_STRIDE * (int)sizeof(double));
        J = BH_WAVE / G;
        J = J > jl ? jl : J;
        J = J > ADAPT_MAX_TRIALS ? ADAPT_MAX_TRIALS : J;
        J = J < 1 ? 1 : J;
        rows_own = m0;
    }
    while (J > 1 && G * J > BH_WAVE) --J;
    // Love only: further trials INSIDE a lane group.  Its recursion is scalar (every lane of the group
    // would repeat it), so lane l runs trial l mod JL instead; only the layer terms cost JL passes.
    const int JL = (T.iwave == 1 && T.inlook > 1) ? T.inlook : 1;
    const int LPM = G * J;         // lanes per model: J groups of G lanes, group r evaluates candidate r
    const int MPW = ADAPT ? 1 : BH_WAVE / LPM; // models per wavefront (lanes >= MPW*LPM idle along as clones of lane 0)
    extern __shared__ __align__(16) unsigned char smem_all[];
    const int lane = threadIdx.x & (BH_WAVE - 1);
    // the workgroup's shared copy of the libm tables, then one private region per wavefront
    // this launch's range of the processing order (see SwdMultiArgs::split)
    int lo = 0, hi = nlist;
    if (A.split != nullptr) {
        const int ndeep = A.split[0];
        if (cls == 0) hi = ndeep;
        else lo = ndeep;
    }
    if (A.wg_n1 == 0 && lo + wg_x * WPB * MPW >= hi) return; // whole workgroup beyond the range (grid = worst case)
    const LibmTabs LT = stage_libm_tables(smem_all, threadIdx.x, BH_WAVE * WPB); // (a later pass writes the same values again)
    if (pass == 0) __syncthreads();
    if (beyond || lo + wid * MPW >= hi) return;
    unsigned char *smem = smem_all + LIBM_TAB_PAD + (size_t)wave * wave_lds;
    const bool spare = lane >= MPW * LPM;
    const int g = spare ? 0 : lane / LPM;        // model slot inside the wave
    const int rr = spare ? 0 : (lane % LPM) / G; // which candidate this lane's group evaluates
    const int li = spare ? 0 : lane % G;         // this lane's index inside its group
    const int slot = g * J + rr;                 // group index inside the wave
    const int sidx = lo + wid * MPW + g; // position in the processing order
    const bool valid = sidx < hi;
    const int32_t *perm = T.perm != nullptr ? T.perm : A.perm; // processing order: the target's own (SIMD pairing) or the batch's
    const int ib = valid ? (perm ? perm[sidx] : sidx) : 0;
    const int Lmax = ADAPT ? rows_own : A.rows[cls]; // LDS rows per model of this class (>= every layer count it meets)
#if BH_SWD_SITEX
    // K: this lane's model's own count (0 for a site out of range: the model fails in band); Kcap: the columns of its output row
    const int Kcap = T.K, KE = (Kcap + 1) & ~1;
    const int Kown = valid ? bh_site_count(X, ty, ib, Kcap) : 0;
    const int K = Kown > 0 ? Kown : 0;
#else
    const int K = T.K;
#endif
    const int ifunc = T.iwave; // 1 Love, 2 Rayleigh: uniform per wavefront

    // LDS carve-up of the wavefront's region (all offsets multiples of 16 B)
    const int prow = Lmax > 1 ? Lmax - 1 : 1;                      // parked rows per group: the finite layers
    double *ca = reinterpret_cast<double *>(smem);                 // [MPW*J][prow][CA_STRIDE]
    double *xs = ca + (size_t)MPW * J * prow * CA_STRIDE;          // [11][MPW]
    double *ys = xs + NEV_MAX * MPW;
#if BH_SWD_SITEX
    double *per_all = ys + NEV_MAX * MPW;                          // [MPW][KE]: a row per model
    float *mdl = reinterpret_cast<float *>(per_all + MPW * KE);    // [4][Lmax][MPW]
    const double *per = per_all + g * KE;
#else
    double *per = ys + NEV_MAX * MPW;                              // [K]
    float *mdl = reinterpret_cast<float *>(per + ((K + 1) & ~1));  // [4][Lmax][MPW]
#endif
    unsigned char *after = reinterpret_cast<unsigned char *>(mdl) + (((size_t)4 * Lmax * MPW * sizeof(float) + 15) & ~(size_t)15);
    double *cpl = reinterpret_cast<double *>(after); // [2][Kmax][MPW], only if a target has mode > 1

#if BH_SWD_SITEX
    for (int idx = lane; idx < MPW * Kcap; idx += BH_WAVE) {
        const int mg = idx / Kcap, kk = idx - mg * Kcap;
        const int sbx = lo + wid * MPW + mg;
        if (sbx < hi) {
            const double *pr = X.x;
            const int32_t *permx = T.perm != nullptr ? T.perm : A.perm;
            const int kb = bh_site_periods(X, ty, permx ? permx[sbx] : sbx, Kcap, pr);
            if (kk < kb) per_all[mg * KE + kk] = pr[kk];
        }
    }
#else
    for (int k = lane; k < K; k += BH_WAVE) per[k] = T.periods[k];
#endif
    // stage the models of this wave: consecutive lanes -> consecutive models (coalesced for
    // layer-major input), binary32 rounding like the f2py boundary
    for (int idx = lane; idx < Lmax * MPW; idx += BH_WAVE) {
        const int l = idx / MPW, mg = idx % MPW;
        const int sb = lo + wid * MPW + mg;
        const int b = sb < hi ? (perm ? perm[sb] : sb) : 0;
        float fd = 0.f, fa = 1.f, fb = 1.f, fr = 1.f;
        if (sb < hi && l < A.nlay[b]) {
            const ptrdiff_t o = (ptrdiff_t)b * T.sb + (ptrdiff_t)l * T.sl;
            fd = (float)T.h[o];
            fa = (float)T.vp[o];
            fb = (float)T.vs[o];
            fr = (float)T.rho[o];
        }
        mdl[(0 * Lmax + l) * MPW + mg] = fd;
        mdl[(1 * Lmax + l) * MPW + mg] = fa;
        mdl[(2 * Lmax + l) * MPW + mg] = fb;
        mdl[(3 * Lmax + l) * MPW + mg] = fr;
    }
    const int mmax = valid ? A.nlay[ib] : 2;
    int mtop = mmax;
    for (int off = 32; off > 0; off >>= 1) mtop = max(mtop, __shfl_xor(mtop, off));
    mtop = __builtin_amdgcn_readfirstlane(mtop);
    wave_sync();
    ModelLdsRt md;
    md.S = MPW;
    md.d = mdl + 0 * Lmax * MPW + g;
    md.a = mdl + 1 * Lmax * MPW + g;
    md.b = mdl + 2 * Lmax * MPW + g;
    md.rho = mdl + 3 * Lmax * MPW + g;
    const int llw = (md.Bf(0) <= 0.0f) ? 2 : 1;
    double *cam = ca + (size_t)slot * prow * CA_STRIDE; // this group's parked layers
    const bool par5 = (G >= 5) && !(Gflags & 0x100);
    const int gbase = slot * G; // first lane of this group
    // one layer count for the whole wavefront and no water layer: the recursion needs no masking
    const bool ragged = __ballot(mmax != mtop || llw != 1) != 0ull;
    const int col = li % 5;                          // the 5-vector component this lane owns

    constexpr bool FAST = FASTM != 0;
    constexpr bool BULK = FAST; // runs of plain bracket steps consumed in one go (the short-refinement build only)
    SearchT<0, NEV_MAX, FASTM, SIMPLE> S;
    S.XS = MPW;
    // RESTART (one model per wavefront, the build with both sequences, SwdMultiArgs::restart): when the guard of the short
    // refinement fires, the model starts again right here with the reference's sequence -- what the engine's re-run launch
    // would do for it afterwards, without the second launch (the guarded models of a sampler's window are its shallow ones:
    // their second search ends before the window's deep models do).  Same rows, same flags.
    bool refseq_now = T.refseq != 0, restarted = false;
    unsigned evals_before = 0u; // (evaluations of the abandoned first search: they count, as the re-run launch's would)
restart_with_the_reference_sequence:
    S.init(md, mmax, valid, T.igr, K, per, xs + g, ys + g, T.vel + (size_t)ib * T.ldv, li == 0 && rr == 0 && !spare,
#if BH_SWD_SITEX
           T.mode, cpl + g, cpl + (size_t)Kcap * MPW + g, ifunc, CNTB && A.counted != 0, refseq_now, FA);
    if (valid && li == 0 && rr == 0 && !spare && !restarted)
        for (int i = K; i < Kcap; ++i) (T.vel + (size_t)ib * T.ldv)[i] = 0.0; // the columns beyond the site's own periods
#else
           T.mode, cpl + g, cpl + (size_t)K * MPW + g, ifunc, CNTB && A.counted != 0, refseq_now, FA);
#endif
    S.evals += evals_before;

    // per-period constants of this lane's first layer (m = li) and of the half-space: they depend
    // on omega and the model only, not on the trial phase velocity -> recomputed when omega changes
    // (the build with both sequences AND the counted scan has no registers to keep them in: formed anew every round there)
    constexpr bool CACHE = !(CNTB && FASTM == 1);
    double c_omega = -1.0, c_xka = 0.0, c_xkb = 0.0, c_gammk = 0.0, h_xka = 0.0, h_xkb = 0.0, h_gammk = 0.0;
    double c_inv = 0.0; // fast arithmetic: 1 / rho (Rayleigh) resp. 1 / xmu (Love) of this lane's first layer
    const bool prof = PROF && (A.neval != nullptr);
    // (the phase clocks are a development aid; the one-model-per-wavefront build with both sequences and the counted scan has
    //  no registers for them)
    long long tA = 0, tB = 0, tS = 0, t0 = 0, t1c = 0, t2c = 0;
    constexpr bool CLK = PROF && !(ADAPT && CNTB && FASTM == 1);
    const bool clocks = CLK && (A.neval != nullptr);
    const unsigned long long w_start = clocks ? wall_clock64() : 0ull, c_start = clocks ? clock64() : 0ull;
    unsigned int nrounds = 0;
    // Two wavefronts share a SIMD; at equal priority the hardware serves the OLDER one first (MI355X_MICROARCH.md,
    // "two waves per SIMD"): the older runs its rounds in ~13 k cycles, the younger in ~17 k, finishes 30 % later and
    // sets the kernel's time.  The two therefore (a) alternate between a high and a low issue priority every
    // PRIO_BLOCK rounds, the two hardware wave slots of a SIMD in opposite phase -- each is the favoured one half of
    // the time -- and (b) tell each other how far they are: every PRIO_BLOCK rounds a wavefront publishes the
    // fraction of its period list its slowest model has behind it in a small board in global memory, indexed by
    // the physical SIMD, and reads its neighbour's; whoever is behind takes the high priority until they are level,
    // so that both reach the end of their lists together.  (Scheduling only: results do not depend on it.)
    unsigned hw_id, xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    const unsigned hw_slot = hw_id & 1u;
    const unsigned simd_key = ((xcc_id & 7u) << 12) | ((hw_id >> 4) & 0xfffu);
    unsigned *board = A.board ? A.board + 2u * simd_key : nullptr;
    const bool fair = (Gflags & 0x800) == 0;
    const unsigned total_p = (unsigned)(K * (T.mode > 0 ? T.mode : 1));
    while (__ballot(S.active) != 0ull) {
        if (fair && (nrounds & (PRIO_BLOCK - 1)) == 0) {
            bool high = (((nrounds / PRIO_BLOCK) ^ hw_slot) & 1u) != 0u;
            if (board != nullptr && !(Gflags & 0x400)) {
                // periods behind the slowest model of this wavefront, as a fraction (16 bits) of its list
                unsigned done = valid ? (S.active ? (unsigned)((S.iq - 1) * K + S.k) : total_p) : total_p;
                for (int off = 32; off > 0; off >>= 1) done = min(done, (unsigned)__shfl_xor((int)done, off));
                const unsigned frac = __builtin_amdgcn_readfirstlane(total_p ? (done << 12) / total_p : 4096u);
                const unsigned mine = (A.stamp << 16) | frac;
                // (plain store: written through the CU's L1 and KEPT in the XCD's L2 -- an agent-scope atomic store drops
                // the line, and every look at the board then went to memory: 25 MB per launch; the load bypasses L1.
                // Both wavefronts sit on the same CU, hence behind the same L2.)
                *reinterpret_cast<volatile unsigned *>(board + hw_slot) = mine;
                const unsigned other = __hip_atomic_load(board + (hw_slot ^ 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((other >> 16) == A.stamp && (other & 0xffffu) != frac) high = frac < (other & 0xffffu);
            }
            if (high) __builtin_amdgcn_s_setprio(3);
            else if (A.prio_low == 0) __builtin_amdgcn_s_setprio(0);
            else __builtin_amdgcn_s_setprio(1);
        }
        ++nrounds;
        // All lanes take part in the evaluation (finished models compute on stale values).
        if (clocks) t0 = clock64();
        const double omg = S.omega;
        const int cb = rr * JL + (li % JL); // the trial this lane carries through the recursion
        // (Rayleigh wavefronts take the instantiations without the counted scan -- `ifunc` is uniform per wavefront)
        const double cev = (J * JL == 1) ? S.ceval : ((!CNTB || ifunc == 2) ? S.template candidate<false>(cb) : S.template candidate<CNTB>(cb));
        const double wvno = omg / cev;
        double del;
        int nv = -1; // Love: the packed mode count of this lane's trial (LoveCount)
        if (ifunc == 2) {
            double omega = omg;
            if (omega < 1.0e-4) omega = 1.0e-4;
            const double wvno2 = wvno * wvno;
            if (!CACHE || omega != c_omega) {
                c_omega = omega;
                if (li <= mmax - 2) {
                    const double am = md.A(li), bm = md.Bv(li);
                    c_xka = omega / am;
                    c_xkb = omega / bm;
                    const double t = bm / omega;
                    c_gammk = 2.0 * t * t;
                    if (FA) c_inv = fa::rcp(md.R(li));
                }
                const double ah = md.A(mmax - 1), bh = md.Bv(mmax - 1);
                h_xka = omega / ah;
                h_xkb = omega / bh;
                const double t = bh / omega;
                h_gammk = 2.0 * t * t;
            }
            // ---- phase A: layer terms, one layer per lane (strided by G) -----------------------
            for (int m = li; m <= mmax - 2; m += G) {
                if (m >= llw - 1) {
                    double xka, xkb, gammk;
                    if (m == li) {
                        xka = c_xka;
                        xkb = c_xkb;
                        gammk = c_gammk;
                    } else { // deep models: further rounds are computed on the fly
                        const double am = md.A(m), bm = md.Bv(m);
                        xka = omega / am;
                        xkb = omega / bm;
                        const double t = bm / omega;
                        gammk = 2.0 * t * t;
                    }
                    const double gam = gammk * wvno2;
                    const double dpth = md.D(m);
                    const double rho1 = md.R(m);
                    LayerTerms v;
                    Ca19 c;
                    if (FA) {
                        fa::layer_products(wvno, xka, xkb, dpth, v);
                        fa::ca19(c, wvno2, gam, gammk, rho1, (m == li) ? c_inv : fa::rcp(rho1), v);
                    } else {
                        double wvnop = wvno + xka;
                        double wvnom = fabs(wvno - xka);
                        const double ra = sqrt(wvnop * wvnom);
                        wvnop = wvno + xkb;
                        wvnom = fabs(wvno - xkb);
                        const double rb = sqrt(wvnop * wvnom);
                        layer_products(ra * dpth, rb * dpth, ra, rb, wvno, xka, xkb, dpth, v, LT);
                        rayleigh_ca19(c, wvno2, gam, gammk, rho1, v);
                    }
                    park_ca25(cam + (size_t)m * CA_STRIDE, c);
                }
            }
            // half-space E vector (surfdisp96.f:800-808), redundantly in every lane
            double e[5];
            if (FA) {
                fa::rayleigh_halfspace(e, wvno, wvno2, h_xka, h_xkb, h_gammk, md.R(mmax - 1));
            } else {
                const double xka = h_xka, xkb = h_xkb, gammk = h_gammk;
                double wvnop = wvno + xka;
                double wvnom = fabs(wvno - xka);
                const double ra = sqrt(wvnop * wvnom);
                wvnop = wvno + xkb;
                wvnom = fabs(wvno - xkb);
                const double rb = sqrt(wvnop * wvnom);
                const double gam = gammk * wvno2;
                const double gamm1 = gam - 1.0;
                const double rho1 = md.R(mmax - 1);
                e[0] = rho1 * rho1 * (gamm1 * gamm1 - gam * gammk * ra * rb);
                e[1] = -rho1 * ra;
                e[2] = rho1 * (gamm1 - gammk * ra * rb);
                e[3] = rho1 * rb;
                e[4] = wvno2 - ra * rb;
            }
            wave_sync();
            if (clocks) t1c = clock64();
            // ---- phase B: the sequential recursion, bottom-up over the parked layers -----------
            {
                double e0[5] = {e[0], e[1], e[2], e[3], e[4]};
                DivRange dr;
                dr.reset();
                if (par5) {
                    if (ragged) rayleigh_chain_group<true, true, false, FA>(e, cam, col, gbase, mtop, mmax, llw, dr);
                    else rayleigh_chain_group<true, false, false, FA>(e, cam, col, gbase, mtop, mmax, llw, dr);
                } else {
                    if (ragged) rayleigh_chain_group<false, true, false, FA>(e, cam, col, gbase, mtop, mmax, llw, dr);
                    else rayleigh_chain_group<false, false, false, FA>(e, cam, col, gbase, mtop, mmax, llw, dr);
                }
                if (!FA && !dr.ok() && S.active) { // out-of-range operand somewhere: verbatim re-run (whole groups agree)
                    e[0] = e0[0]; e[1] = e0[1]; e[2] = e0[2]; e[3] = e0[3]; e[4] = e0[4];
                    rayleigh_chain_group<false, true, true>(e, cam, col, gbase, mtop, mmax, llw, dr);
                }
            }
            del = e[0];
            if (llw != 1) { // water layer on top (surfdisp96.f:850-866)
                const double xka = omega / md.A(0);
                const double wvnop = wvno + xka;
                const double wvnom = fabs(wvno - xka);
                const double ra = sqrt(wvnop * wvnom);
                const double dpth = md.D(0);
                const double rho1 = md.R(0);
                const double znul = 1.0e-5;
                LayerTerms v;
                if (FA) fa::layer_products(wvno, xka, wvno + 1.0, dpth, v); // (only w and cosp of the P wave are used)
                else layer_products(ra * dpth, znul, ra, znul, wvno, xka, znul, dpth, v, LT);
                const double w0 = -rho1 * v.w;
                del = v.cosp * e[0] + w0 * e[1];
            }
            wave_sync();
        } else {
            const double omega = omg;
            if (!CACHE || omega != c_omega) {
                c_omega = omega;
                if (li <= mmax - 2) {
                    c_xkb = omega / md.Bv(li);
                    if (FA) c_inv = fa::rcp(md.R(li) * md.Bv(li) * md.Bv(li));
                }
                const double beta1 = md.Bv(mmax - 1);
                h_xkb = omega / beta1;
                h_gammk = 1.0 / (beta1 * beta1); // e2 of the half-space (surfdisp96.f:731)
            }
            // ---- phase A (Love): cosq, y, z, xmu per layer, for each of the group's JL trials ----------
            for (int jj = 0; jj < JL; ++jj) {
                const double wv = (JL == 1) ? wvno : omg / S.template candidate<CNTB>(rr * JL + jj);
                for (int m = li; m <= mmax - 2; m += G) {
                    if (m >= llw - 1) {
                        const double beta1 = md.Bv(m);
                        const double rho1 = md.R(m);
                        const double dm = md.D(m);
                        const double xmu = rho1 * beta1 * beta1;
                        const double xkb = (m == li) ? c_xkb : omega / beta1;
                        double cosq, y, z, fl = 0.0;
                        if (FA) {
                            double q;
                            fa::love_terms(wv, xkb, dm, cosq, y, z, q);
                            if (CNTB) fl = (wv < xkb) ? love_zero_floor(q) : 0.0;
                            double2 *dst = reinterpret_cast<double2 *>(cam + (size_t)m * CA_STRIDE + LOVE_TERMS * jj);
                            dst[0] = make_double2(cosq, y * ((m == li) ? c_inv : fa::rcp(xmu))); // (the products of the recursion's
                            dst[1] = make_double2(z * xmu, 0.0);                                  //  step are formed here, in parallel)
                            dst[2] = make_double2(0.0, fl);
                            continue;
                        }
                        const double wvnop = wv + xkb;
                        const double wvnom = fabs(wv - xkb);
                        const double rb = sqrt(wvnop * wvnom);
                        const double q = dm * rb;
                        if (wv < xkb) {
                            double sinq;
                            bh_sincos(q, &sinq, &cosq, LT);
                            y = sinq / rb;
                            z = -rb * sinq;
                            if (CNTB) fl = love_zero_floor(q);
                        } else if (wv == xkb) {
                            cosq = 1.0;
                            y = dm;
                            z = 0.0;
                        } else {
                            double fac = 0.0;
                            if (q < 16.0) fac = bh_exp(-2.0 * q, LT);
                            cosq = (1.0 + fac) * 0.5;
                            const double sinq = (1.0 - fac) * 0.5;
                            y = sinq / rb;
                            z = rb * sinq;
                        }
                        double2 *dst = reinterpret_cast<double2 *>(cam + (size_t)m * CA_STRIDE + LOVE_TERMS * jj);
                        dst[0] = make_double2(cosq, y);
                        dst[1] = make_double2(z, xmu);
                        dst[2] = make_double2(bh_rcp_refined(xmu), fl);
                    }
                }
            }
            double e1, e2;
            LoveCount lc;
            {
                const double rho1 = md.R(mmax - 1);
                const double xkb = h_xkb;
                const double wvnop = wvno + xkb;
                const double wvnom = fabs(wvno - xkb);
                double rb;
                if (FA) {
                    double t_;
                    const double r2 = wvnop * wvnom;
                    fa::sqrt_rsqrt(r2 > 1.0e-290 ? r2 : 1.0, rb, t_);
                    rb = r2 > 1.0e-290 ? rb : 0.0;
                } else {
                    rb = sqrt(wvnop * wvnom);
                }
                e1 = rho1 * rb;
                e2 = h_gammk;
                lc.reset(wvno > xkb);
            }
            wave_sync();
            if (clocks) t1c = clock64();
            {
                const double s1 = e1, s2 = e2;
                const LoveCount lc0 = lc;
                DivRange dr;
                dr.reset();
                const double *camt = cam + LOVE_TERMS * (li % JL); // this lane's trial
                if (ragged) love_chain_group<true, false, CNTB, FA>(e1, e2, camt, mtop, mmax, llw, dr, lc);
                else love_chain_group<false, false, CNTB, FA>(e1, e2, camt, mtop, mmax, llw, dr, lc);
                if (!FA && !dr.ok() && S.active) {
                    e1 = s1;
                    e2 = s2;
                    lc = lc0;
                    love_chain_group<true, true, CNTB>(e1, e2, camt, mtop, mmax, llw, dr, lc);
                }
            }
            del = e1;
            if (CNTB) nv = lc.packed(e1, e2);
            wave_sync();
        }
        if (clocks) t2c = clock64();
        auto consume = [&](auto cnt_tag) {
            constexpr bool CNT = decltype(cnt_tag)::value;
        // Every lane of the model can read all J (velocity, value) pairs; the search consumes them for
        // as long as its next request is the very velocity (at the same omega) the next group evaluated.
        if (BULK && !CNT && J * JL > 2) { // (measured: pays from three trials per round on; with two it costs 6 % at B = 4096; Love's
                                          //  counted scan hardly ever takes plain steps: not compiled in for its wavefronts)
            // The same consumption with the runs of plain bracket steps taken in one go.  A trial is PLAIN for its model
            // when the search is scanning (ST_STEP), the value has the sign of del1, the velocity is inside the scan's
            // bounds and the request after it is again the plain next step: consuming it only moves (c1, del1) on.
            // Every lane judges the trial it carried; a ballot hands every model the verdicts of all its trials; the
            // leading run of plain trials is consumed by copying the last one's (velocity, value) -- what advance()
            // would have left after stepping through them one by one.  Anything else goes through advance().
            const int Jtot = J * JL;
            bool live = S.active;
            int jn = 0; // this model's next trial
            while (__ballot(live) != 0ull) {
                // trial jn must be the very request (trial 0 IS the pending request)
                const int tj = live ? jn : 0;
                const int srcn = (g * J + tj / JL) * G + (tj % JL);
                const double cj = __shfl(cev, srcn), dj = __shfl(del, srcn);
                const int nj = CNT ? __shfl(nv, srcn) : -1;
                if (jn > 0) live = live && S.ceval == cj && S.omega == omg;
                const double nxt = (S.idir > 0) ? cev + S.dc : cev - S.dc;
                // (a step that reaches a half-space velocity goes through advance(): the guard's probes)
                const bool plain = S.active && S.st == ST_STEP && !signs_differ(S.del1, del) && (!FA || fabs(del) >= fa::SIGN_FLOOR) &&
                                   !(cev < S.cm || cev >= S.betmxd + S.dc) && nxt > S.clow && fmax(cev, S.c1) < S.vsafe;
                const unsigned long long pm = __ballot(plain);
                bool run = false;
                if (live && S.st == ST_STEP) {
                    int t = jn;
                    while (t < Jtot && ((pm >> ((g * J + t / JL) * G + (t % JL))) & 1ull)) ++t;
                    run = t > jn;
                    if (run) {
                        const int src = (g * J + (t - 1) / JL) * G + ((t - 1) % JL);
                        const double cl = __shfl(cev, src), dl = __shfl(del, src);
                        // (the point the run leaves behind: the trial before the last, or -- a run of one -- the old c1)
                        const int srcp = (t - jn >= 2) ? (g * J + (t - 2) / JL) * G + ((t - 2) % JL) : src;
                        const double cq = __shfl(cev, srcp), dq = __shfl(del, srcp);
                        S.cp = (t - jn >= 2) ? cq : S.c1;
                        S.delp = (t - jn >= 2) ? dq : S.del1;
                        S.have_p = true;
                        S.c1 = cl;
                        S.del1 = dl;
                        S.del2 = dl;
                        S.c2 = (S.idir > 0) ? cl + S.dc : cl - S.dc;
                        S.ceval = S.c2;
                        S.evals += (unsigned)(t - jn);
                        S.isteps += t - jn;
                        jn = t;
                    }
                }
                if (live && !run) {
                    S.template advance<CNT>(dj, nj);
                    ++jn;
                }
                live = live && S.active && jn < Jtot;
            }
        } else if (CNT && J * JL > 2) { // (with two trials per round the order is the only one possible)
            // The counted scan asks for grid points in an order that depends on the values (start value, jump target, then an
            // index search): every trial lane carries one of the likely ones (SearchT::candidate), and a trial's value is taken
            // whenever the search asks for exactly its velocity -- in whatever order, each trial at most once.  Trial 0 IS the
            // pending request.  (Which values the search consumes does not depend on it: the requests are the search's own.)
            bool live = S.active;
            unsigned long long used = 0ull;
            int src = (g * J) * G; // a lane that carried trial 0
            const bool rep = !spare && li < JL; // one lane per trial answers
            const unsigned long long mine = (LPM >= 64) ? ~0ull : (((1ull << LPM) - 1ull) << (g * LPM)); // this model's lanes
            for (int it = 0; it < J * JL; ++it) {
                if (__ballot(live) == 0ull) break;
                const double dj = __shfl(del, src);
                const int nj = __shfl(nv, src);
                if (live) {
                    used |= 1ull << src;
                    S.template advance<CNT>(dj, nj);
                }
                live = live && S.active && S.omega == omg;
                const unsigned long long m = __ballot(live && rep && cev == S.ceval) & mine & ~used;
                live = live && m != 0ull;
                src = live ? (int)__builtin_ctzll(m) : src;
            }
        } else {
            bool live = S.active;
            const int Jtot = J * JL;
            for (int j = 0; j < Jtot; ++j) {
                double dj = del;
                int nj = nv;
                if (Jtot > 1) {
                    const int src = (g * J + j / JL) * G + (j % JL); // a lane that carried trial j
                    const double cj = __shfl(cev, src);
                    dj = __shfl(del, src);
                    if (CNT) nj = __shfl(nv, src);
                    // trial 0 IS the pending request (consumed unconditionally, also when a broken model
                    // has driven the search to NaN); a later trial only if the search now asks for it
                    if (j > 0) live = live && S.active && S.ceval == cj && S.omega == omg;
                }
                if (__ballot(live) == 0ull) break;
                if (FAST) {
                    // a plain bracket step (three in four of this build's transitions): the value has del1's sign, the
                    // velocity is inside the scan's bounds and the next request is the next grid point -- what advance()
                    // does then, without its way through the continuation tags
                    const double nx = (S.idir > 0) ? S.c2 + S.dc : S.c2 - S.dc;
                    const bool plain = live && S.st == ST_STEP && !signs_differ(S.del1, dj) && (!FA || fabs(dj) >= fa::SIGN_FLOOR) &&
                                       !(S.c2 < S.cm || S.c2 >= S.betmxd + S.dc) && nx > S.clow && fmax(S.c1, S.c2) < S.vsafe;
                    if (plain) {
                        S.cp = S.c1;      // (the point the scan leaves behind, see SearchT::step_done)
                        S.delp = S.del1;
                        S.have_p = true;
                        S.del2 = dj;
                        S.c1 = S.c2;
                        S.del1 = dj;
                        S.c2 = nx;
                        S.ceval = nx;
                        ++S.evals;
                        ++S.isteps;
                    } else if (live) {
                        S.template advance<CNT>(dj, nj);
                    }
                } else if (live) S.template advance<CNT>(dj, nj);
            }
        }
        };
        if (!CNTB || ifunc == 2) consume(std::false_type{});
        else consume(std::integral_constant<bool, CNTB>{});
        if (clocks) {
            const long long t3 = clock64();
            tA += t1c - t0;
            tB += t2c - t1c;
            tS += t3 - t2c;
        }
    }
    if (ADAPT && FASTM == 1 && A.restart != 0 && !restarted && __ballot(valid && S.has(S.F_GUARD)) != 0ull) {
        restarted = true;
        refseq_now = true;
        evals_before = S.evals;
        if (valid && li == 0 && rr == 0 && !spare && T.gcount != nullptr) {
            atomicAdd(T.gcount + BH_MAX_TARGETS, 1);     // this call: restarted in place
            atomicAdd(T.gcount + 2 * BH_MAX_TARGETS, 1); // cumulative
        }
        goto restart_with_the_reference_sequence;
    }
    if (board != nullptr) *reinterpret_cast<volatile unsigned *>(board + hw_slot) = (A.stamp << 16) | 0xffffu;
    if (valid && li == 0 && rr == 0 && !spare) {
#if BH_SWD_SITEX
        T.err[ib] = Kown < 0 ? 1 : S.errflag; // (site out of range)
#else
        T.err[ib] = S.errflag;
#endif
        if (!SIMPLE && T.igr == 2 && T.first != nullptr) T.first[ib] = S.del1st; // (the chain of a group velocity's first roots: SwdKernelArgs)
        if (FAST && S.has(S.F_GUARD) && T.gcount != nullptr) { // to be run again with the reference's sequence
            T.glist[atomicAdd(T.gcount, 1)] = ib;
            atomicAdd(T.gcount + 2 * BH_MAX_TARGETS, 1); // (cumulative, for bh_engine_guard_stats)
        }
    }
    if (prof) {
        unsigned long long tot = (li == 0 && rr == 0 && !spare) ? S.evals : 0u;
        unsigned long long lps = tot * (unsigned long long)(valid ? mmax - 1 : 0);
        for (int off = 32; off > 0; off >>= 1) {
            tot += __shfl_xor(tot, off);
            lps += __shfl_xor(lps, off);
        }
        if (lane == 0) {
            // [0] secular evaluations; per wave type ([8] Rayleigh / [9] Love) evaluations and ([10] / [11]) layer-
            // propagator steps = evaluations x finite layers of the model (the flop model of SURVEY.md 8(d))
            atomicAdd(A.neval, tot);
            atomicAdd(A.neval + (ifunc == 2 ? 8 : 9), tot);
            atomicAdd(A.neval + (ifunc == 2 ? 10 : 11), lps);
            // development aid: wave-cycles per phase, [1..3] Rayleigh A/B/state, [4..6] Love
            const int o = (ifunc == 2) ? 1 : 4;
            if (clocks) {
                atomicAdd(A.neval + o, (unsigned long long)tA);
                atomicAdd(A.neval + o + 1, (unsigned long long)tB);
                atomicAdd(A.neval + o + 2, (unsigned long long)tS);
            }
            const unsigned long long widx = atomicAdd(A.neval + 7, 1ull);
            if (clocks && widx < BH_TRACE_WAVES) { // development aid: one record per wavefront (tools/gpu_trace.py)
                unsigned long long *r = A.neval + BH_COUNTER_WORDS + 4 * widx;
                unsigned hwid, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                hwid = (hwid & 0xffffu) | ((xcc & 0xfu) << 16);
                r[0] = w_start;
                r[1] = wall_clock64();
                r[2] = ((unsigned long long)(clock64() - c_start) & 0xffffffffffull) | ((unsigned long long)(unsigned)(blockIdx.x * WPB + wave) << 40); // cycles | grid wavefront index << 40
                r[3] = (unsigned long long)nrounds | ((unsigned long long)ifunc << 32) | ((unsigned long long)hwid << 36);
            }
        }
    }
    if (PASSES && A.rerun != 0) { // the next entries of the list
        ++pass;
        goto next_pass;
    }
}

// Launches build <FM, SI, PR, AD, CN, FA> of the kernel if it is plan g's.  Every translation unit lists the builds it compiles
// (their flags and register budgets are what its machine code depends on: Makefile, swd_group_fa.hip, _adapt, _big).
// (site-period builds: the "stream" is the stream and the period table, SwdGroupXStream, and the functions below end in _x)
#if BH_SWD_SITEX
typedef SwdGroupXStream GroupStream;
#define BH_GROUP_FN(name) name##_x
#else
typedef hipStream_t GroupStream;
#define BH_GROUP_FN(name) name
#endif
template <int FM, bool SI, bool PR, bool AD, bool CN, bool FA = false>
bool launch_build(const SwdMultiArgs &a, const SwdGroupPlan &g, GroupStream stream)
{
    const SwdGroupBuild &b = g.build;
    if (b.fastm != FM || b.simple != SI || b.prof != PR || b.adapt != AD || b.cntb != CN || b.fa != FA) return false;
#if BH_SWD_SITEX
    hipLaunchKernelGGL((swd_group_kernel<GROUP_WPB, FM, SI, PR, AD, CN, FA>), g.grid, g.block, g.lds, stream.st, a, g.Gflags, (int)g.wave_lds, *stream.x);
#else
    hipLaunchKernelGGL((swd_group_kernel<GROUP_WPB, FM, SI, PR, AD, CN, FA>), g.grid, g.block, g.lds, stream, a, g.Gflags, (int)g.wave_lds);
#endif
    return true;
}
} // namespace

#if defined(BH_GROUP_BIG_TU)
// The build that needs more than 256 registers (this translation unit: swd_group_big.hip, ONE wavefront per SIMD as its register
// budget): one model per wavefront, both sequences, the counted Love scan AND the counters and clocks -- an instrumented launch of a
// sampler's window under BH_SEARCH_FAST_RAYLEIGH; counters and clocks are what it is for, not speed.
bool BH_GROUP_FN(bh_swd_group_builds_big)(const SwdMultiArgs &a, const SwdGroupPlan &g, GroupStream s)
{
    return launch_build<1, true, true, true, true>(a, g, s);
}
#elif defined(BH_GROUP_ADAPT_TU)
// The one-model-per-wavefront builds (ADAPT: a sampler's windows, single models, the re-run of guarded models) in a translation unit
// of their own (swd_group_adapt.hip: the same source, the same flags) -- a third of this file's instantiations: it halves the
// build's longest compile.  (Both sequences with the counted scan and the counters: swd_group_big.hip.)
bool BH_GROUP_FN(bh_swd_group_builds_adapt)(const SwdMultiArgs &a, const SwdGroupPlan &g, GroupStream s)
{
    return launch_build<2, true, true, true, false>(a, g, s) || launch_build<2, true, true, true, true>(a, g, s) ||
           launch_build<2, true, false, true, false>(a, g, s) || launch_build<2, true, false, true, true>(a, g, s) ||
           launch_build<1, true, true, true, false>(a, g, s) ||
           launch_build<1, true, false, true, false>(a, g, s) || launch_build<1, true, false, true, true>(a, g, s) ||
           launch_build<0, true, true, true, false>(a, g, s) || launch_build<0, true, true, true, true>(a, g, s) ||
           launch_build<0, true, false, true, false>(a, g, s) || launch_build<0, true, false, true, true>(a, g, s);
}
#elif defined(BH_GROUP_FA_TU)
// The builds with the fast arithmetic (this translation unit: swd_group_fa.hip).
bool BH_GROUP_FN(bh_swd_group_builds_fa)(const SwdMultiArgs &a, const SwdGroupPlan &g, GroupStream s)
{
    return launch_build<2, true, true, true, true, true>(a, g, s) || launch_build<2, true, true, true, false, true>(a, g, s) ||
           launch_build<2, true, false, true, true, true>(a, g, s) || launch_build<2, true, false, true, false, true>(a, g, s) ||
           launch_build<2, true, true, false, true, true>(a, g, s) || launch_build<2, true, true, false, false, true>(a, g, s) ||
           launch_build<2, true, false, false, true, true>(a, g, s) || launch_build<2, true, false, false, false, true>(a, g, s);
}
#else
namespace {
// The builds of several models per wavefront in the reference's arithmetic (this translation unit).
bool launch_builds(const SwdMultiArgs &a, const SwdGroupPlan &g, GroupStream s)
{
    return launch_build<2, true, true, false, false>(a, g, s) || launch_build<2, true, true, false, true>(a, g, s) ||
           launch_build<2, true, false, false, false>(a, g, s) || launch_build<2, true, false, false, true>(a, g, s) ||
           launch_build<2, false, true, false, false>(a, g, s) || launch_build<2, false, true, false, true>(a, g, s) ||
           launch_build<1, false, true, false, false>(a, g, s) ||
           launch_build<0, true, true, false, false>(a, g, s) || launch_build<0, true, true, false, true>(a, g, s) ||
           launch_build<0, true, false, false, false>(a, g, s) || launch_build<0, true, false, false, true>(a, g, s) ||
           launch_build<0, false, true, false, false>(a, g, s) || launch_build<0, false, true, false, true>(a, g, s);
}
#if !BH_SWD_SITEX
// (sitex: the site-period builds keep a row of Kmax periods for each of the wavefront's models)
size_t group_lds_bytes(int G, int J, int Lmax, int Kmax, int maxmode, bool sitex)
{
    const int MPW = BH_WAVE / (G * J);
    return ((size_t)MPW * J * (Lmax > 1 ? Lmax - 1 : 1) * CA_STRIDE + (size_t)2 * NEV_MAX * MPW +
            (size_t)((Kmax + 1) & ~1) * (sitex ? MPW : 1)) * sizeof(double) +
           (((size_t)4 * Lmax * MPW * sizeof(float) + 15) & ~(size_t)15) +
           (maxmode > 1 ? (size_t)2 * Kmax * MPW * sizeof(double) : 0);
}
#endif
} // namespace

#if BH_SWD_SITEX
bool bh_launch_swd_group_x(const SwdMultiArgs &a, const SwdGroupPlan &g, const SwdSiteXArgs &x, hipStream_t stream)
{
    const SwdGroupXStream s{stream, &x};
    return launch_builds(a, g, s) || bh_swd_group_builds_adapt_x(a, g, s) || bh_swd_group_builds_fa_x(a, g, s) || bh_swd_group_builds_big_x(a, g, s);
}
#else
// LDS of one workgroup = shared libm tables + GROUP_WPB wavefront regions
size_t bh_swd_group_lds_bytes(int G, int J, int Lmax, int Kmax, int maxmode, bool sitex)
{
    return LIBM_TAB_PAD + GROUP_WPB * ((group_lds_bytes(G, J, Lmax, Kmax, maxmode, sitex) + 15) & ~(size_t)15);
}

// A wavefront's LDS region small enough for 8 wavefronts (4 workgroups) per CU of 160 KB
constexpr size_t WAVE_LDS_TARGET = (160 * 1024 / 4 - LIBM_TAB_PAD) / GROUP_WPB;
constexpr size_t WG_LDS_CAP = 64 * 1024;

SwdGroupPlan bh_plan_swd_group(const SwdGroupAsk &q, const BhTuning &tun)
{
    SwdGroupPlan g{};
    const int nt = q.ntargets;
    int kmax = 0, maxmode = 1;
    for (int t = 0; t < nt; ++t) {
        kmax = q.t[t].K > kmax ? q.t[t].K : kmax;
        maxmode = q.t[t].mode > maxmode ? q.t[t].mode : maxmode;
    }
    g.Gflags = (tun.swd_redundant ? 0x100 : 0) | (tun.swd_no_board ? 0x400 : 0) | (tun.swd_no_fair ? 0x800 : 0);
    const bool two = q.Lcut < q.Lmax;
    // target t with G lanes per model: models per wavefront, wavefronts
    auto mpw_at = [&](int G, int t) { return BH_WAVE / (G * bh_trials_fit(G, q.t[t].look)); };
    auto waves_at = [&](int G, int t) { return (q.B + mpw_at(G, t) - 1) / mpw_at(G, t); };
    long nwaves = 1;
    for (int cls = two ? 0 : 1; cls <= 1; ++cls) {
        const int rows = (two && cls == 1) ? q.Lcut : q.Lmax;
        auto wave_bytes = [&](int G) {
            size_t w = 0;
            for (int t = 0; t < nt; ++t)
                w = std::max(w, (group_lds_bytes(G, bh_trials_fit(G, q.t[t].look), rows, kmax, maxmode, q.sitex) + 15) & ~(size_t)15);
            return w;
        };
        // fewer models per wavefront (more lanes per model) until the parked layers fit: first the
        // residency target, at the latest the 64 KB a workgroup may ask for
        int G = q.G0;
        // a batch that leaves half the chip idle anyway: one lane per layer of the deepest model of the
        // class (a single pass over the layers) instead of lanes for the typical depth
        // (only where that costs neither look-ahead nor residency)
        for (int Gwide = rows - 1 > 16 ? 16 : rows - 1; Gwide > G; --Gwide) {
            long w = 0;
            bool same = true;
            for (int t = 0; t < nt; ++t) {
                w += waves_at(Gwide, t);
                same = same && bh_trials_fit(Gwide, q.t[t].look) == bh_trials_fit(G, q.t[t].look);
            }
            if (w <= 256 && same) {
                G = Gwide;
                break;
            }
        }
        auto several = [&](int lanes) { // several models per wavefront for some target
            bool any = false;
            for (int t = 0; t < nt; ++t) any = any || mpw_at(lanes, t) > 1;
            return any;
        };
        while (several(G) && wave_bytes(G) > WAVE_LDS_TARGET) G += 1;
        // (the cap is what a workgroup of GROUP_WPB wavefronts may ask for by default)
        while (G < BH_WAVE && LIBM_TAB_PAD + GROUP_WPB * wave_bytes(G) > WG_LDS_CAP) G += 1;
        if (LIBM_TAB_PAD + GROUP_WPB * wave_bytes(G) > WG_LDS_CAP) return g; // (fits = false)
        g.rows[cls] = rows;
        g.lanes[cls] = G;
        g.wave_lds = std::max(g.wave_lds, wave_bytes(G));
        for (int t = 0; t < nt; ++t) nwaves = std::max(nwaves, (long)waves_at(G, t)); // worst case: the whole batch is in this class
    }
    g.fits = true;
    if (!two) {
        g.rows[0] = g.rows[1];
        g.lanes[0] = g.lanes[1];
    }
    // per target at the launched lanes of one class: models per wavefront, wavefronts
    int mpw[8], nw[8];
    for (int t = 0; t < nt; ++t) {
        mpw[t] = mpw_at(g.lanes[1], t);
        nw[t] = waves_at(g.lanes[1], t);
    }
    g.grid = dim3((unsigned)((nwaves + GROUP_WPB - 1) / GROUP_WPB), nt, two ? 2 : 1);
    if (nt == 2 && !two && tun.swd_no_mix == 0 && !q.rerun) { // two targets, one depth class: interleave their wavefronts (see the kernel)
        g.wg_n0 = nw[0];
        g.wg_n1 = nw[1];
        g.grid = dim3((nw[0] + nw[1] + GROUP_WPB - 1) / GROUP_WPB, 1, 1);
    }
    // SIMD-pairing order of the models (SwdPairWork): a one-dimensional grid of one class, workgroups of two wavefronts
    g.pair = !two && g.grid.y == 1 && g.grid.z == 1 && nt <= 2 && bh_pair_order_fits(q.B);
    for (int t = 0; t < 2; ++t) {
        g.pair_mpw[t] = t < nt ? mpw[t] : 1;
        g.pair_waves[t] = t < nt ? nw[t] : 0;
    }
    // One model per wavefront for every target (a chain window, a single model), one class, the usual targets: every wavefront
    // sizes its lane groups and trials for its own model (ADAPT, see the kernel) within the region all wavefronts can be
    // resident with.
    // (capacity up to 32 rows: at least two trials fit the region; deeper arrays keep the plan's own choice of fewer, wider
    // lane groups in a larger region)
    bool adapt = q.adapt_ok && tun.swd_no_adapt == 0 && !two && q.Lmax <= 32 && q.Lmax >= 2;
    bool any_phase = false, any_group = false, any_modes = false, any_refseq = false, any_love = false, all_love = true;
    for (int t = 0; t < nt; ++t) {
        const SwdGroupAsk::Target &T = q.t[t];
        adapt = adapt && mpw[t] == 1 && !T.group && T.mode <= 1 && T.K <= 64;
        any_phase = any_phase || (!T.group && !T.refseq);
        any_group = any_group || T.group;
        any_refseq = any_refseq || (!T.group && T.refseq);
        any_modes = any_modes || T.mode > 1;
        any_love = any_love || T.iwave == 1;
        all_love = all_love && T.iwave == 1;
    }
    if (adapt) g.wave_lds = WAVE_LDS_TARGET & ~(size_t)15;
    g.lds = LIBM_TAB_PAD + GROUP_WPB * g.wave_lds;
    g.block = dim3(BH_WAVE * GROUP_WPB);
    g.info = SwdLaunchInfo{g.grid.x * g.grid.y * g.grid.z, g.wg_n1 > 0 ? (long)g.wg_n0 + g.wg_n1 : nwaves * nt, g.lds, GROUP_WPB};
    // (one model per wavefront and SwdMultiArgs::restart: the build with both sequences, guarded models restart in place;
    //  not with the fast arithmetic: the reference's sequence runs in the reference's arithmetic -- the re-run launch)
    g.restart = adapt && q.restart && q.fast && any_phase && tun.swd_no_restart == 0 && !(q.farith && !any_group && !any_refseq && !any_modes);
    // fastm: 0 = reference sequence; with the short refinement asked for: 2 = no group-velocity target in the launch (nevill
    // not compiled in), 1 = mixed (group-velocity targets keep the reference sequence), 0 = group-velocity targets only.
    const int fastm = (q.fast && any_phase) ? ((any_group || any_refseq || g.restart) ? 1 : 2) : 0;
    // simple: fundamental-mode phase velocities only (builds 0 and 2; no second root, no mode loop in the kernel).
    const bool simple = !any_group && !any_modes && tun.swd_no_simple == 0;
    // The builds with the counted scan (CNTB, see the kernel): asked for, a Love target in the launch, and the launch is of the
    // kind it pays in -- one model per wavefront, or Love targets only.
    // q.scan: 1 = wherever a Love target is (BH_SCAN_COUNTED), 2 = where it pays (BH_SCAN_AUTO): with several models per
    // wavefront, launches of Love targets only (B = 4096: 2.06 -> 1.71 ms) and Rayleigh + Love launches of the short refinement
    // (there the LOVE wavefronts set the time: 379 rounds against the Rayleigh wavefronts' 302; counted 149 rounds of twice the
    // length: c2 2.51 -> 2.30 ms, c3 2.60 -> 2.49).  One model per wavefront (the trial lanes already walk the scan seven
    // steps a round: 1.25 -> 1.27 ms per window of the chains) and Rayleigh + Love launches of the reference's sequence (the
    // Rayleigh wavefronts set the time: c2 3.37 -> 3.47 ms) do not gain.
    // (not in a launch of several models per wavefront that mixes both refinements: that build would spill; one model per
    //  wavefront -- the chains' windows -- has it)
    const bool cntb = any_love && !(fastm == 1 && !adapt) && (q.scan == 1 || (q.scan == 2 && !adapt && (all_love ? fastm != 1 : fastm == 2)));
    // the fast arithmetic (FA, see the kernel): every target of the launch takes the short refinement, the usual targets
    const bool fa = q.farith && fastm == 2 && simple;
    // The builds without the counters exist for the SIMPLE launches only: there they are worth 2 % (c2 3.44 -> 3.37 ms; 4 instead
    // of 33 spilled SGPRs); a launch with group-velocity targets is 2 % SLOWER without them (c2g 5.55 -> 5.67 ms).  The ADAPT
    // builds (plain targets only) are all SIMPLE; the build with both sequences of several models per wavefront is not.
    const bool simple_build = adapt || (simple && fastm != 1);
    g.build = SwdGroupBuild{fastm, simple_build, q.counters || !simple_build, adapt, cntb, fa};
    // (the re-run: the kernel's PASSES, its workgroups stride over the list)
    if (adapt && fastm == 0 && q.rerun && tun.swd_rerun_wgs > 0 && g.grid.x > (unsigned)tun.swd_rerun_wgs) g.grid.x = (unsigned)tun.swd_rerun_wgs;
    return g;
}

void bh_launch_swd_group(const SwdMultiArgs &a, const SwdGroupPlan &g, hipStream_t stream)
{
    const bool launched = launch_builds(a, g, stream) || bh_swd_group_builds_adapt(a, g, stream) ||
                          bh_swd_group_builds_fa(a, g, stream) || bh_swd_group_builds_big(a, g, stream);
    assert(launched && "the plan's build is compiled");
    (void)launched;
}
#endif
#endif

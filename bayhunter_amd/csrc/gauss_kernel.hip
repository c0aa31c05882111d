// bayhunter_amd/csrc/gauss_kernel.hip -- the Gauss-law quadratic form d^T R^-1 d for a whole batch
// as a dense FP64 contraction on the matrix cores.
//
// Replaces, for BH_LAW_GAUSS targets, `madist = (ydiff.T).dot(c_inv).dot(ydiff)` of
// src/Targets.py:339-340 with c_inv = R^-1 / sigma^2 (:162-173): for the B residual rows
// D[B][n] and the constant R^-1[n][n] (host LAPACK pinv, once per chain, :150-160) it forms
// V = D * R^-1 tile by tile with v_mfma_f64_16x16x4_f64 and folds  Phi_b = sum_j V_bj D_bj  into
// the epilogue.  This is the one dense contraction of the whole path:
// 2*B*n^2 = 8.6 GFLOP at B = 4096, n = 1024 -- the per-model LDS mat-vec it replaces ran at
// 2.8 TFLOP/s (3.0 ms); the FP64 MFMA peak of MI355X is 78.6 TFLOP/s.
//
// Work split: workgroup (bx, by) = 64 models x one slab of columns; 4 waves, wave w owns models
// [16w, 16w+16) and all four 16-column blocks of the current 64-column tile (one A fragment feeds
// four MFMAs).  K is streamed through LDS in tiles of 32, the global loads of the next tile in flight while
// the MFMAs of the current one run (register double buffer).  Column slabs are summed later in a
// fixed order by like_kernel, so the result does not depend on scheduling (no atomics).
#include "bh_device.h"
#include "bh_tuning.h"
#include <cstdlib>
// BH_GAUSS_CLASSES (gauss_kernel_c.hip): the builds for sites with their own noise correlation (bh_sites_set_gauss,
// include/bh_engine_sites_gauss.h) -- the grouping kernels, the two contraction forms over tiles of one class each -- and their launcher only.
#ifndef BH_GAUSS_CLASSES
#define BH_GAUSS_CLASSES 0
#endif

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int KT = 32;  // K tile
constexpr int LDT = 80; // LDS row stride in doubles: 64 + 16 puts consecutive k rows 128 B apart mod 256 B

// SITES: the observed data of model b is the row of its site (GaussSiteArgs, bh_device.h), gathered per model row from a
// table that stays in L2; a site out of range reads site 0's row (the likelihood kernel reports that model failed)
__device__ __forceinline__ const double *site_row(const double *yobs, const GaussSiteArgs &S, int b)
{
    const int s = S.site[b];
    return yobs + (size_t)((s >= 0 && s < S.nsites) ? s : 0) * S.ldo;
}

#if BH_GAUSS_CLASSES
// ---- correlation classes: the rows grouped class by class (GaussClassArgs, bh_device.h) ----------------------------------------
// The sites of a device-resident call are unknown to the host, so three small launches sort the rows: the classes' row counts, the
// prefixes over their rows and TILES (a class's rows are padded to whole tiles: a workgroup streams one matrix), and the rows dealt
// to their class's range -- the counting sort posterior_kernel.hip uses by site.  The order of a class's wavefronts follows the
// atomics and is not fixed; it cannot show: in both contraction bodies an output row depends on its own residual row, the matrix and the fixed k
// order only (an MFMA accumulates every element of C on its own), and the epilogue reduces over columns -- never on the row's
// position in the tile.
__device__ __forceinline__ int row_class(const GaussSiteArgs &S, const int32_t *class_of, int b)
{
    const int s = S.site[b];
    return (s >= 0 && s < S.nsites) ? class_of[s] : -1;
}

// ctr[c] += the lanes of this wavefront whose class is c, ONE atomic per (wavefront, class) -- thousands of rows share a handful of
// classes, and an atomic per row would serialise on those few addresses.  The lanes of the
// lowest pending lane's class elect it leader; it adds their number and hands everyone its place behind the counter's old value.
// Returns the lane's place (c < 0: -1).  Every lane of the wavefront calls it (the loop is wave-uniform).
__device__ __forceinline__ int wave_class_add(int c, int32_t *ctr)
{
    const int lane = threadIdx.x & 63;
    int pos = -1;
    unsigned long long todo = __ballot(c >= 0);
    while (todo != 0) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(c, leader);
        const unsigned long long same = __ballot(c == lc);
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctr[lc], (int)__popcll(same));
        base = __shfl(base, leader);
        if (c == lc) pos = base + (int)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return pos;
}

__global__ __launch_bounds__(256) void gauss_class_count_kernel(int B, GaussSiteArgs S, const int32_t *class_of, int32_t *count)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    (void)wave_class_add(b < B ? row_class(S, class_of, b) : -1, count);
}

// (one thread: a handful of classes; at most BH_SITES_GAUSS_MAXCLASSES, include/bh_engine_sites_gauss.h)
__global__ void gauss_class_scan_kernel(int nclass, int tile_rows, const int32_t *count, int32_t *cursor, int32_t *row_start, int32_t *tile_start)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int rows = 0, tiles = 0;
    for (int c = 0; c < nclass; ++c) {
        row_start[c] = cursor[c] = rows;
        tile_start[c] = tiles;
        rows += count[c];
        tiles += (count[c] + tile_rows - 1) / tile_rows;
    }
    row_start[nclass] = rows;
    tile_start[nclass] = tiles;
}

// ... and the rows of no class (site out of range, class -1) belong to no tile: their slab sums are zeroed here (the likelihood
// kernel fails or skips those models without reading them)
__global__ __launch_bounds__(256) void gauss_class_scatter_kernel(int B, GaussSiteArgs S, const int32_t *class_of, int32_t *cursor,
                                                                  int32_t *perm, int nsplit, double *partial)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int c = b < B ? row_class(S, class_of, b) : -1;
    const int pos = wave_class_add(c, cursor);
    if (c >= 0) {
        perm[pos] = b;
    } else if (b < B) {
        for (int i = 0; i < nsplit; ++i) partial[(size_t)b * nsplit + i] = 0.0;
    }
}

// The tile of a workgroup: (class, first position in perm, rows), from the tile prefix; cls < 0: beyond the last tile (the grid is
// sized for the worst case, ceil(B / tile rows) + nclass)
struct ClassTile {
    int cls, first, rows;
};
__device__ __forceinline__ ClassTile class_tile(const GaussClassArgs &G, int tile, int tile_rows)
{
    ClassTile T{-1, 0, 0};
    if (tile >= G.tile_start[G.nclass]) return T;
    int lo = 0, hi = G.nclass; // the last class whose first tile is at or before `tile` (classes without rows have no tile)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (G.tile_start[mid] <= tile) lo = mid;
        else hi = mid;
    }
    T.cls = lo;
    T.first = G.row_start[lo] + (tile - G.tile_start[lo]) * tile_rows;
    T.rows = min(tile_rows, G.row_start[lo + 1] - T.first);
    return T;
}
// row `local` of the tile: its model, or B (no row: treated as gb >= B)
__device__ __forceinline__ int class_row(const GaussClassArgs &G, const ClassTile &T, int local, int B)
{
    return local < T.rows ? G.perm[T.first + local] : B;
}
#define BH_GAUSS_ROW(local) class_row(G, tile, (local), B)

__global__ __launch_bounds__(256, 2) void gauss_quad_classes_kernel(int B, int n, int ldy, const double *ymod,
                                                            const double *yobs, const double *rinv_all,
                                                            int nsplit, int cols_per_split, double *partial, GaussSiteArgs S, GaussClassArgs G)
{
    constexpr bool SITES = true;
#include "gauss_body.inc"
}
#else
#define BH_GAUSS_ROW(local) (m0 + (local))
__global__ __launch_bounds__(256, 2) void gauss_quad_kernel(int B, int n, int ldy, const double *ymod,
                                                            const double *yobs, const double *rinv,
                                                            int nsplit, int cols_per_split, double *partial)
{
    constexpr bool SITES = false;
    constexpr GaussSiteArgs S{};
#include "gauss_body.inc"
}

// the same with a site table (bh_evaluate_sites)
__global__ __launch_bounds__(256, 2) void gauss_quad_sites_kernel(int B, int n, int ldy, const double *ymod,
                                                            const double *yobs, const double *rinv,
                                                            int nsplit, int cols_per_split, double *partial, GaussSiteArgs S)
{
    constexpr bool SITES = true;
#include "gauss_body.inc"
}
#endif

// ---- the large-problem form (round 3): 128 models x 128 columns per workgroup ---------------------------------
// The 64 x 64 tiles above read 1 MB from L2 for every 8.4 MFLOP (every workgroup streams its 64 residual rows and
// its 64 columns of R^-1 over the whole K range): at 4096 x 1024^2 that is 1 GB per launch, 3.5 TB/s at 0.29 ms --
// the kernel was bound by the L2, not by the matrix cores (37-39 % of their peak).  A 128 x 128 tile halves the bytes
// per flop; eight wavefronts (4 x 2: 32 models x 64 columns each, 8 accumulator blocks, one A fragment feeding four
// MFMAs and one B fragment two) keep two wavefronts on every SIMD; K tiles of 32 are double-buffered in LDS with the
// global loads of tile t+1 in flight during the MFMAs of tile t: ONE barrier per tile (the old form: two).
// LDS layouts chosen for the fragment READS (five per four MFMAs): residuals [model][k] with a row pitch of KT + 1
// doubles -- the 16 models of an A fragment fall into 16 different banks --, R^-1 [k][column], 16 consecutive
// doubles per fragment row.  Staging stores: 8-byte stores for the residuals (conflict-free: 17 m + 4 q covers 16
// banks), 16-byte stores for R^-1.
#ifndef BH_GAUSS_KT
#define BH_GAUSS_KT 16
#endif
constexpr int BM = 128, BN = 128, KT2 = BH_GAUSS_KT;
constexpr int NPT = BM * KT2 / 512; // doubles of each tile a thread stages per K tile (4 at KT2 = 16, 8 at 32)
constexpr int PA = KT2 + 1;  // row pitch of the residual tile (doubles)
constexpr int PB = BN + 4;   // row pitch of the R^-1 tile (doubles; keeps 16-byte alignment)

#if BH_GAUSS_CLASSES
__global__ __launch_bounds__(512) void gauss_quad_classes_kernel_128(int B, int n, int ldy, const double *__restrict__ ymod,
                                                             const double *__restrict__ yobs, const double *__restrict__ rinv_all,
                                                             int nsplit, int kper, double *__restrict__ partial, GaussSiteArgs S, GaussClassArgs G)
{
    constexpr bool SITES = true;
#include "gauss_body_128.inc"
}
#else
__global__ __launch_bounds__(512) void gauss_quad_kernel_128(int B, int n, int ldy, const double *__restrict__ ymod,
                                                             const double *__restrict__ yobs, const double *__restrict__ rinv,
                                                             int nsplit, int kper, double *__restrict__ partial)
{
    constexpr bool SITES = false;
    constexpr GaussSiteArgs S{};
#include "gauss_body_128.inc"
}

// the same with a site table (bh_evaluate_sites)
__global__ __launch_bounds__(512) void gauss_quad_sites_kernel_128(int B, int n, int ldy, const double *__restrict__ ymod,
                                                             const double *__restrict__ yobs, const double *__restrict__ rinv,
                                                             int nsplit, int kper, double *__restrict__ partial, GaussSiteArgs S)
{
    constexpr bool SITES = true;
#include "gauss_body_128.inc"
}
#endif

} // namespace

// the 128 x 128 form pays where its grid fills the chip: at least one workgroup for every second CU
static bool use_big_tiles(int B, int n)
{
    const int force = bh_tuning().gauss_tile; // (bh_tuning.h: 64 / 128)
    if (force == 64) return false;
    if (force == 128) return true;
    return (long)((B + BM - 1) / BM) * ((n + BN - 1) / BN) >= 128;
}

// K ranges per tile of the 128 x 128 form: enough workgroups for two per CU (one per CU leaves two wavefronts per SIMD,
// measured 47 % of the matrix peak at 4096 x 1024^2 against 56 % with two)
static int big_ksplit(int B, int n)
{
    const long wgs = (long)((B + BM - 1) / BM) * ((n + BN - 1) / BN);
    int ks = 1;
    while (ks < 4 && wgs * ks < 512 && n / (2 * ks) >= 128) ks *= 2;
    return ks;
}

#if BH_GAUSS_CLASSES
// The form, the slabs, the K split and the layout of `partial` are those of (B, n) on the paths without classes (use_big_tiles,
// bh_gauss_nsplit -- the caller's nsplit --, big_ksplit): only the row tiles differ, ceil(B / tile rows) + nclass for the worst case.
void bh_launch_gauss_quad_classes(int B, int n, int ldy, const double *ymod, const double *yobs, const GaussSiteArgs &sites,
                                  const int32_t *class_of, int nclass, const double *rinv, int nsplit, double *partial,
                                  int32_t *work, hipStream_t stream)
{
    int32_t *count = work, *cursor = work + nclass, *row_start = work + 2 * (size_t)nclass, *tile_start = row_start + nclass + 1,
            *perm = tile_start + nclass + 1;
    const bool big = use_big_tiles(B, n);
    const int tile_rows = big ? BM : 64;
    (void)hipMemsetAsync(count, 0, (size_t)nclass * sizeof(int32_t), stream);
    hipLaunchKernelGGL(gauss_class_count_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, sites, class_of, count);
    hipLaunchKernelGGL(gauss_class_scan_kernel, dim3(1), dim3(64), 0, stream, nclass, tile_rows, count, cursor, row_start, tile_start);
    hipLaunchKernelGGL(gauss_class_scatter_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, sites, class_of, cursor, perm, nsplit, partial);
    const GaussClassArgs G{class_of, nclass, row_start, tile_start, perm};
    const int row_tiles = (B + tile_rows - 1) / tile_rows + nclass;
    if (big) {
        const int ks = big_ksplit(B, n);
        const int kper = (((n + ks - 1) / ks + KT2 - 1) / KT2) * KT2;
        hipLaunchKernelGGL(gauss_quad_classes_kernel_128, dim3(row_tiles, (n + BN - 1) / BN, ks), dim3(512), 0, stream, B, n, ldy, ymod,
                           yobs, rinv, nsplit, kper, partial, sites, G);
        return;
    }
    const int tiles = (n + 63) / 64;
    const int cols_per_split = ((tiles + nsplit - 1) / nsplit) * 64;
    hipLaunchKernelGGL(gauss_quad_classes_kernel, dim3(row_tiles, nsplit), dim3(256), 0, stream, B, n, ldy, ymod, yobs, rinv, nsplit,
                       cols_per_split, partial, sites, G);
}
#else
int bh_gauss_nsplit(int B, int n)
{
    if (use_big_tiles(B, n)) return 2 * ((n + BN - 1) / BN) * big_ksplit(B, n);
    const int tiles = (n + 63) / 64;
    int nsplit = 1;
    // enough workgroups for two per CU, but never less than one 64-column tile per slab
    while (nsplit < tiles && ((B + 63) / 64) * nsplit < 512) nsplit *= 2;
    if (nsplit > tiles) nsplit = tiles;
    return nsplit;
}

static void launch_gauss_quad(int B, int n, int ldy, const double *ymod, const double *yobs, const GaussSiteArgs *sites,
                              const double *rinv, int nsplit, double *partial, hipStream_t stream)
{
    if (use_big_tiles(B, n)) {
        const int ks = big_ksplit(B, n);
        const int kper = (((n + ks - 1) / ks + KT2 - 1) / KT2) * KT2;
        const dim3 grid((B + BM - 1) / BM, (n + BN - 1) / BN, ks);
        if (sites)
            hipLaunchKernelGGL(gauss_quad_sites_kernel_128, grid, dim3(512), 0, stream, B, n, ldy, ymod, yobs, rinv, nsplit, kper,
                               partial, *sites);
        else
            hipLaunchKernelGGL(gauss_quad_kernel_128, grid, dim3(512), 0, stream, B, n, ldy, ymod, yobs, rinv, nsplit, kper, partial);
        return;
    }
    const int tiles = (n + 63) / 64;
    const int cols_per_split = ((tiles + nsplit - 1) / nsplit) * 64;
    const dim3 grid((B + 63) / 64, nsplit);
    if (sites)
        hipLaunchKernelGGL(gauss_quad_sites_kernel, grid, dim3(256), 0, stream, B, n, ldy, ymod, yobs, rinv, nsplit, cols_per_split,
                           partial, *sites);
    else
        hipLaunchKernelGGL(gauss_quad_kernel, grid, dim3(256), 0, stream, B, n, ldy, ymod, yobs, rinv, nsplit, cols_per_split, partial);
}

void bh_launch_gauss_quad(int B, int n, int ldy, const double *ymod, const double *yobs,
                          const double *rinv, int nsplit, double *partial, hipStream_t stream)
{
    launch_gauss_quad(B, n, ldy, ymod, yobs, nullptr, rinv, nsplit, partial, stream);
}

void bh_launch_gauss_quad_sites(int B, int n, int ldy, const double *ymod, const double *yobs, const GaussSiteArgs &sites,
                                const double *rinv, int nsplit, double *partial, hipStream_t stream)
{
    launch_gauss_quad(B, n, ldy, ymod, yobs, &sites, rinv, nsplit, partial, stream);
}
#endif

// bayhunter_amd/csrc/gauss_body_128.inc -- the body of gauss_quad_kernel_128 and gauss_quad_sites_kernel_128 (gauss_kernel.hip), included inside each kernel.
// In scope: the kernel's arguments, GaussSiteArgs S and the compile-time `constexpr bool SITES` (true: the residual row of
// model b is taken against the observed data of its site, site_row).  The body is included rather than called: a device
// function inlined into the kernel is optimised in another order, and the kernels without sites keep the machine code they
// had before the site variants existed.
    __shared__ __align__(16) double Dm[2][BM * PA];
    __shared__ __align__(16) double Rt[2][KT2 * PB];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const int wm = w >> 1, wn = w & 1;
    const int fi = l & 15, fk = l >> 4;
#if BH_GAUSS_CLASSES
    // CLASSES (gauss_kernel_c.hip): the workgroup's rows are a tile of ONE correlation class, its models read through the permutation
    // (BH_GAUSS_ROW), rinv that class's matrix; a workgroup beyond the last tile leaves at once (uniform: before any barrier)
    const ClassTile tile = class_tile(G, blockIdx.x, BM);
    if (tile.cls < 0) return;
    const double *__restrict__ rinv = rinv_all + (size_t)tile.cls * n * n;
    const int c0 = blockIdx.y * BN;
#else
    const int m0 = blockIdx.x * BM, c0 = blockIdx.y * BN;
#endif
    // staging coordinates
    const int d_mdl = tid >> 2, d_kq = (tid & 3) * NPT;                           // residuals: model, NPT consecutive k
    const int r_row = tid / (BN / NPT), r_cq = (tid % (BN / NPT)) * NPT;          // R^-1: k row, NPT consecutive columns
    const int d_gb = BH_GAUSS_ROW(d_mdl);
    const bool d_ok = d_gb < B;
    const double *yrow = ymod + (size_t)(d_ok ? d_gb : 0) * ldy;
    const double *yo_d = (SITES && d_ok) ? site_row(yobs, S, d_gb) : yobs; // observed data of the staged model
    // this workgroup's share of K (blockIdx.z): the quadratic form is a sum over k as well, so a K range is one more slab
    const int kbeg = blockIdx.z * kper, kend = min(n, kbeg + kper);
    double dreg[NPT], rreg[NPT];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int k = k0 + d_kq + i;
            dreg[i] = (d_ok && k < kend) ? yrow[k] - yo_d[k] : 0.0;
        }
        const int k = k0 + r_row;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int col = c0 + r_cq + i;
            rreg[i] = (k < kend && col < n) ? rinv[(size_t)k * n + col] : 0.0;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NPT; ++i) Dm[buf][d_mdl * PA + d_kq + i] = dreg[i];
        double2 *dst = reinterpret_cast<double2 *>(&Rt[buf][r_row * PB + r_cq]);
#pragma unroll
        for (int i = 0; i < NPT / 2; ++i) dst[i] = make_double2(rreg[2 * i], rreg[2 * i + 1]);
    };
    double4_t c[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) c[rb][cb] = double4_t{0.0, 0.0, 0.0, 0.0};
    const int ntile = (kend - kbeg + KT2 - 1) / KT2;
    fetch(kbeg);
    stage(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntile) fetch(kbeg + (t + 1) * KT2);
        const double *da = &Dm[buf][(wm * 32 + fi) * PA + fk];
        const double *rb_ = &Rt[buf][fk * PB + wn * 64 + fi];
#pragma unroll
        for (int kk = 0; kk < KT2; kk += 4) {
            const double a0 = da[kk], a1 = da[16 * PA + kk];
            double bv[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) bv[cb] = rb_[kk * PB + cb * 16];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                c[0][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv[cb], c[0][cb], 0, 0, 0);
                c[1][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv[cb], c[1][cb], 0, 0, 0);
            }
        }
        if (t + 1 < ntile) stage(buf ^ 1);
        __syncthreads();
    }
    // epilogue: c[rb][cb][r] = V[model m0 + 32 wm + 16 rb + fk + 4 r][column c0 + 64 wn + 16 cb + fi]; fold in D of the same
    // entry, sum over this wavefront's 64 columns; one slab per (column block, column half)
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gb = BH_GAUSS_ROW(wm * 32 + rb * 16 + fk + 4 * r);
            const double *yo = (SITES && gb < B) ? site_row(yobs, S, gb) : yobs;
            double v = 0.0;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int col = c0 + wn * 64 + cb * 16 + fi;
                if (gb < B && col < n) v += c[rb][cb][r] * (ymod[(size_t)gb * ldy + col] - yo[col]);
            }
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 8);
            if (fi == 0 && gb < B) partial[(size_t)gb * nsplit + (blockIdx.y * 2 + wn) * gridDim.z + blockIdx.z] = v;
        }

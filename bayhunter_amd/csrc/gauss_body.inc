// bayhunter_amd/csrc/gauss_body.inc -- the body of gauss_quad_kernel and gauss_quad_sites_kernel (gauss_kernel.hip), included inside each kernel.
// In scope: the kernel's arguments, GaussSiteArgs S and the compile-time `constexpr bool SITES` (true: the residual row of
// model b is taken against the observed data of its site, site_row).  The body is included rather than called: a device
// function inlined into the kernel is optimised in another order, and the kernels without sites keep the machine code they
// had before the site variants existed.
    __shared__ double Dt[KT][LDT]; // residuals, [k][model]
    __shared__ double Rt[KT][LDT]; // R^-1 tile, [k][col]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
#if BH_GAUSS_CLASSES
    // CLASSES (gauss_kernel_c.hip): the workgroup's rows are a tile of ONE correlation class, its models read through the permutation
    // (BH_GAUSS_ROW), rinv that class's matrix; a workgroup beyond the last tile leaves at once (uniform: before any barrier)
    const ClassTile tile = class_tile(G, blockIdx.x, 64);
    if (tile.cls < 0) return;
    const double *rinv = rinv_all + (size_t)tile.cls * n * n;
#else
    const int m0 = blockIdx.x * 64;
#endif
    const int c_begin = blockIdx.y * cols_per_split;
    const int c_end = min(n, c_begin + cols_per_split);
    const int fi = l & 15, fk = l >> 4; // fragment coordinates
    double acc[4] = {0.0, 0.0, 0.0, 0.0};

    // staging coordinates: D tile: thread -> model tid/4, 8 consecutive k; R^-1 tile: thread -> row tid/8, 8 consecutive columns
    const int d_mdl = tid >> 2, d_kq = (tid & 3) * 8, d_gb = BH_GAUSS_ROW(d_mdl);
    const int r_kr = tid >> 3, r_cq = (tid & 7) * 8;
    const double *yo_d = (SITES && d_gb < B) ? site_row(yobs, S, d_gb) : yobs; // observed data of the staged model
    for (int jt = c_begin; jt < c_end; jt += 64) {
        double4_t c[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) c[b] = double4_t{0.0, 0.0, 0.0, 0.0};
        // software pipeline: the global loads of K tile t+1 are in flight while the MFMAs of tile t run
        double dreg[8], rreg[8];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = k0 + d_kq + i;
                dreg[i] = (d_gb < B && k < n) ? ymod[(size_t)d_gb * ldy + k] - yo_d[k] : 0.0;
            }
            const int k = k0 + r_kr;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int col = jt + r_cq + i;
                rreg[i] = (k < n && col < c_end) ? rinv[(size_t)k * n + col] : 0.0;
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < n; k0 += KT) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                Dt[d_kq + i][d_mdl] = dreg[i];
                Rt[r_kr][r_cq + i] = rreg[i];
            }
            __syncthreads();
            if (k0 + KT < n) fetch(k0 + KT);
#pragma unroll
            for (int kk = 0; kk < KT; kk += 4) {
                const double a = Dt[kk + fk][w * 16 + fi];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double bv = Rt[kk + fk][b * 16 + fi];
                    c[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, c[b], 0, 0, 0);
                }
            }
        }
        // epilogue: c[b][r] = V[model 16w + fk + 4r][col jt + 16b + fi]; fold in D of the same entry
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gb = BH_GAUSS_ROW(w * 16 + fk + 4 * r);
            const double *yo = (SITES && gb < B) ? site_row(yobs, S, gb) : yobs;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = jt + b * 16 + fi;
                if (gb < B && col < c_end) acc[r] += c[b][r] * (ymod[(size_t)gb * ldy + col] - yo[col]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double v = acc[r];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        const int gb = BH_GAUSS_ROW(w * 16 + fk + 4 * r);
        if (fi == 0 && gb < B) partial[(size_t)gb * nsplit + blockIdx.y] = v;
    }

// bayhunter_amd/csrc/like_body.inc -- the body of like_kernel and like_sites_kernel (like_kernel.hip), included inside each kernel.
// In scope: LikeKernelArgs A, LikeSiteArgs S and the compile-time `constexpr bool SITES` (true: model b compares with
// the observed data of its site S.site[b]; a site out of range fails the model in band and reads no observed data).
// The body is included rather than called: a device function inlined into the kernel is optimised in another order, and
// the kernels without sites keep the machine code they had before the site variants existed.
    __shared__ double red[4];
    extern __shared__ __align__(16) unsigned char smem[];
    double *dl = reinterpret_cast<double *>(smem); // [max n of the Gauss-law targets]
    const int ib = blockIdx.x;
    const int tid = threadIdx.x;
    const double *y = A.ymod + (size_t)ib * A.ldy;
    double logL = 0.0, joint = 0.0;
    bool failed = false;
#if !BH_LIKE_MISSING
    for (int t = 0; t < A.nt; ++t) failed = failed || (A.err_t[(size_t)t * A.B + ib] != 0);
#endif
    int site = 0;
    if (SITES) { // the workgroup's model: a scalar load
        site = S.site[ib];
        failed = failed || site < 0 || site >= S.nsites;
    }
#if BH_LIKE_MISSING
    // BH_LIKE_MISSING (like_kernel_m.hip): a target the model's site lacks (count 0) is no part of the model's likelihood -- its
    // failure flag is not read (the forward kernels leave it alone; a model with absurd values would set it), it is skipped below
    const bool on_table = !failed;
    for (int t = 0; t < A.nt && on_table; ++t)
        failed = failed || (S.n[(size_t)site * A.nt + t] != 0 && A.err_t[(size_t)t * A.B + ib] != 0);
#endif
    for (int t = 0; t < A.nt && !failed; ++t) {
#if BH_LIKE_LAWS
        const LikeTargetDev T = class_target(site_target(law_target(A.t[t], W, site, A.nt, t), S, site, A.ldy, A.nt, t), G, site, t); // (like_kernel_l.hip)
#elif BH_LIKE_CLASSES
        const LikeTargetDev T = class_target(site_target(A.t[t], S, site, A.ldy, A.nt, t), G, site, t); // (like_kernel_c.hip)
#else
        const LikeTargetDev T = SITES ? site_target(A.t[t], S, site, A.ldy, A.nt, t) : A.t[t];
#endif
        const int n = T.n;
#if BH_LIKE_MISSING
        if (n == 0) { // the site lacks this target (uniform over the model's lanes): nothing read, nothing added, misfit 0
            if (tid == 0) A.misfits[(size_t)ib * (A.nt + 1) + t] = 0.0;
            continue;
        }
#endif
        const double *ym = y + T.off;
        const double corr = A.noise[(size_t)ib * 2 * A.nt + 2 * t];
        const double sigma = A.noise[(size_t)ib * 2 * A.nt + 2 * t + 1];
        double s0 = 0.0, s1 = 0.0, sw = 0.0;
        double d0 = 0.0, dn = 0.0;
        if (T.pre != nullptr) { // the forward kernel formed the sums (fused likelihood, RfKernelArgs::sums): nothing to read of ymod
            const double *pre = T.pre + (size_t)ib * 4;
            s0 = pre[0];
            s1 = pre[1];
            d0 = pre[2];
            dn = pre[3];
        } else {
        for (int i = tid; i < n; i += 256) {
            const double d = ym[i] - T.yobs[i];
            s0 += d * d;
            if (T.law == 2 && i + 1 < n) s1 += d * (ym[i + 1] - T.yobs[i + 1]);
            if (T.law == 1) sw += d * d / T.yerr_scaled[i];
        }
        if (T.law == 3 && T.quad != nullptr) { // slab sums from the MFMA contraction, fixed order
            if (tid == 0)
                for (int sidx = 0; sidx < T.nsplit; ++sidx) sw += T.quad[(size_t)ib * T.nsplit + sidx];
        } else if (T.law == 3) { // (d^T R^-1) d with d staged in LDS; column access = coalesced over i
            __syncthreads();
            for (int i = tid; i < n; i += 256) dl[i] = ym[i] - T.yobs[i];
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                double acc = 0.0;
                for (int jj = 0; jj < n; ++jj) acc += dl[jj] * T.rinv[(size_t)jj * n + i];
                sw += acc * dl[i];
            }
        }
        if (T.law == 2) {
            d0 = ym[0] - T.yobs[0];
            dn = ym[n - 1] - T.yobs[n - 1];
        }
        }
        if (T.pre != nullptr) {
            // (already reduced)
        } else if (n <= 64 && !(T.law == 3 && T.quad == nullptr)) {
            // a short target (a dispersion curve beside a long receiver function): its samples all sit in the first
            // wavefront, the other three would only add zeros -- no barrier (same bits as block_sum); only thread 0's
            // values are used below
            for (int off = 32; off > 0; off >>= 1) s0 += __shfl_xor(s0, off);
            if (T.law == 2)
                for (int off = 32; off > 0; off >>= 1) s1 += __shfl_xor(s1, off);
            if (T.law == 1 || T.law == 3)
                for (int off = 32; off > 0; off >>= 1) sw += __shfl_xor(sw, off);
        } else {
            s0 = block_sum(s0, red);
            if (T.law == 2) s1 = block_sum(s1, red);
            if (T.law == 1 || T.law == 3) sw = block_sum(sw, red);
        }
        const double s2 = sigma * sigma;
        double phi, logdet = (2.0 * n) * log(sigma);
        if (T.law == 0) {
            phi = s0 / s2;
        } else if (T.law == 1) {
            phi = sw / s2;
            logdet += T.logdet_extra;
        } else if (T.law == 2) {
            // get_corr_inv (Targets.py:131-137): d[0] = d[-1] = 1 -- for n == 1 both hit the
            // same element, so the edge correction must not be applied twice
            const double edge = (n > 1) ? (d0 * d0 + dn * dn) : (d0 * d0);
            const double r2 = corr * corr;
            phi = ((1.0 + r2) * s0 - r2 * edge - 2.0 * corr * s1) / (s2 * (1.0 - r2));
            logdet += (n - 1) * log(1.0 - r2);
        } else {
            phi = sw / s2;
            logdet += T.logdet_extra;
        }
        const double part = -0.5 * ((double)n * log(2.0 * M_PI) + logdet);
        logL += part - phi / 2.0;
        const double rms = sqrt(s0 / (double)n);
        joint += rms;
        if (tid == 0) A.misfits[(size_t)ib * (A.nt + 1) + t] = rms;
    }
    if (tid == 0) {
        if (failed) { // Targets.py:325-328
            A.logL[ib] = -1e15;
#if BH_LIKE_MISSING
            for (int t = 0; t <= A.nt; ++t) // (a target the site lacks keeps its 0)
                A.misfits[(size_t)ib * (A.nt + 1) + t] = (t < A.nt && on_table && S.n[(size_t)site * A.nt + t] == 0) ? 0.0 : 1e15;
#else
            for (int t = 0; t <= A.nt; ++t) A.misfits[(size_t)ib * (A.nt + 1) + t] = 1e15;
#endif
            A.err[ib] = 1;
        } else {
            A.logL[ib] = logL;
            A.misfits[(size_t)ib * (A.nt + 1) + A.nt] = joint;
            A.err[ib] = 0;
        }
    }

// bayhunter_amd/csrc/rf_coef_body.inc -- the body of rf_coef_kernel and rf_coef_sites_kernel (rf_kernel.hip), included inside
// each kernel.  In scope: RfKernelArgs A, RfSiteArgs S and the compile-time `constexpr bool SITES`.
// SITES (bh_evaluate_sites with a table of bh_sites_set_rf): the model's ray parameter and near-surface velocity are its
// site's, S.p / S.nsv of row S.site[ib], put through the same expressions as the descriptor's values -- the record of a model
// of site s has the bits of a one-site launch whose descriptor holds site s's values.  A site out of range reads nothing of
// the table (the descriptor's values stand in) and marks the record bad.
// The body is included rather than called: a device function inlined into the kernel is optimised in another order, and
// rf_coef_kernel keeps the machine code it had before the site variant existed.
    const int ib = blockIdx.x * blockDim.x + threadIdx.x;
    if (ib >= A.B) return;
    const int Lmax = A.Lmax;
    double *rec = A.coef + (size_t)ib * rec_doubles(Lmax);
    const int nlay = A.nlay[ib];
    const ptrdiff_t base = (ptrdiff_t)ib * A.sb;
    const double R = 6371.0;
    double p_sd = A.p_s_per_deg, nsv_in = A.nsv;
    bool off_table = false;
    if (SITES) {
        const int s = S.site[ib];
        off_table = s < 0 || s >= S.nsites;
        if (!off_table) {
            p_sd = S.p[(size_t)s * S.ld];
            nsv_in = S.nsv[(size_t)s * S.ld];
        }
    }
    const double p = p_sd * 0.00899; // wrap.cpp:55
    const double p2 = p * p;
    double bad = 0.0;
    double nf = 0.0; // stays 0 while every coefficient of the record is finite
    double im = 0.0; // stays 0 while every interface matrix is real

    // top-layer quantities before flattening (q = 1 for the top layer anyway)
    const double vp0 = A.vp[base], vs0 = A.vs[base];
    // rfmini_modrf.py:125-130 and wrap.cpp:13,73-74
    const double kap = vp0 / vs0;
    const double poisson = (2 - kap * kap) / (2 - 2 * (kap * kap));
    const double nsv = (nsv_in > 0.0) ? nsv_in : vs0;
    const double vptop = nsv * sqrt((1. - poisson) / (.5 - poisson));
    const double vstop = nsv;

    // flatten layer by layer (model.cpp:221-252); z = depth of the layer top = running sum of h
    double ztop = 0.0, t0 = 0.0;
    double pvp = 0, pvs = 0, prh = 0; // previous (upper) layer, flattened
    for (int l = 0; l < nlay; ++l) {
        const ptrdiff_t o = base + (ptrdiff_t)l * A.sl;
        // thickness the way synrf.cpp:28-32 forms it from the depths z = cumsum(h)
        // (rfmini_modrf.py:119-123): z[l+1] - z[l]; the half-space gets -1
        const double znext = ztop + A.h[o];
        const bool half = (l == nlay - 1);
        double hh = half ? -1.0 : (znext - ztop);
        double vp = A.vp[o], vs = A.vs[o], rh = A.rho[o];
        const double qp = A.qp ? A.qp[o] : 500.0, qs = A.qs ? A.qs[o] : 225.0;
        const double zb = ztop + hh;
        double r = R - ztop;
        double q = R / r;
        const double zf = R * log(q);
        vp *= q;
        vs *= q;
        rh /= q;
        const bool lower_halfspace = !(hh > 0.0) && !(vp < 1.0 && rh < 0.1);
        if (!lower_halfspace) {
            r = R - zb;
            q = R / r;
            hh = R * log(q) - zf;
        }
        double *lay = rec + REC_HEAD + 8 * l;
        lay[0] = 1.0 / (vp * vp); lay[1] = 1.0 / (vs * vs); lay[2] = hh;
        lay[3] = 1.0 / (M_PI * qp); lay[4] = 1.0 / (2.0 * qp); lay[5] = 1.0 / (M_PI * qs); lay[6] = 1.0 / (2.0 * qs);
        for (int k = 0; k < 7; ++k) nf += nf1(lay[k]);
        // direct-wave delay (greens.cpp:510-526); only its NaN-ness can reach the RF
        const double vv = (A.waveno == 0) ? vp : vs;
        t0 += hh * sqrt(1. / (vv * vv) - p2);
        if (l == 0) {
            // free surface, greens.cpp:87-112 (plain sqrt) and displacement matrix :307-322
            const cd a = csqrt_d(C(1. / (vp * vp) - p2));
            const cd b = csqrt_d(C(1. / (vs * vs) - p2));
            const double t1 = 2. * vs * vs;
            const double t2 = t1 * p2 - 1.;
            const cd d1 = C(t2 * t2);
            const cd d2 = (t1 * t1 * p2) * a * b;
            const cd d = d1 + d2;
            const cd t3 = C(2. * t1 * p * t2) / d;
            cm2 ru;
            ru.c11 = (d2 - d1) / d;
            ru.c12 = -(b * t3);
            ru.c21 = a * t3;
            ru.c22 = ru.c11;
            store_cm2(rec + 16, ru);
            const double vp2 = vp * vp, vs2 = vs * vs, x = 1. - 2. * vs2 * p2;
            const cd a1 = conj(a), b1 = conj(b);
            const cd qq = crecip(C(x * x) + (4. * vs2 * vs2 * p2) * a1 * b1);
            cm2 hm;
            hm.c11 = qq * a1 * b1 * (2. * vs2 * p);
            hm.c12 = qq * b1 * (1. - 2. * vs2 * p2);
            hm.c21 = qq * a1 * (1. - 2. * vs2 * p2);
            hm.c22 = -(qq * a1 * b1 * (2. * vs2 * p));
            hm.c11 = 2.0 * hm.c11; hm.c12 = 2.0 * hm.c12; hm.c21 = 2.0 * hm.c21; hm.c22 = 2.0 * hm.c22;
            store_cm2(rec + 8, hm);
            nf += nonfinite(ru) + nonfinite(hm);
            im += imag_mass(ru);
            (void)vp2;
        } else {
            cm2 rd, td, ru, tu;
            interface_coeffs(p, pvp, pvs, prh, vp, vs, rh, rd, td, ru, tu);
            double *ic = rec + REC_HEAD + 8 * Lmax + 32 * (l - 1);
            store_cm2(ic, rd);
            store_cm2(ic + 8, td);
            store_cm2(ic + 16, ru);
            store_cm2(ic + 24, tu);
            nf += nonfinite(rd) + nonfinite(td) + nonfinite(ru) + nonfinite(tu);
            im += imag_mass(rd) + imag_mass(td) + imag_mass(ru) + imag_mass(tu);
        }
        pvp = vp; pvs = vs; prh = rh;
        ztop = znext;
    }
    if (t0 != t0) bad = 1.0;
    if (nlay < 2) bad = 1.0; // the reference reads an uninitialised matrix here (SURVEY App. B.10)
    // rotation Z/R -> P/SV with REAL vertical slownesses (greens.cpp:324-341)
    double do_decomp = 0.0, m11 = 0, m12 = 0, m21 = 0, m22 = 0;
    if (vstop > 0.01 && fabs(p) > 0.0001) {
        do_decomp = 1.0;
        const double aa = sqrt(1. / (vptop * vptop) - p * p), bb = sqrt(1. / (vstop * vstop) - p * p);
        m11 = -(2 * vstop * vstop * p * p - 1.) / (vptop * aa);
        m12 = 2. * p * vstop * vstop / vptop;
        m21 = -2. * p * vstop;
        m22 = (1. - 2. * vstop * vstop * p * p) / (vstop * bb);
        nf += nf1(m11) + nf1(m12) + nf1(m21) + nf1(m22);
    }
    // A non-finite coefficient makes every bin of the reference's spectrum non-finite, hence the whole trace (the
    // inverse FFT sums all bins); with the spectral cut-off the bins above it are not formed here, so the record
    // carries the flag instead of relying on the propagation
    if (nf != 0.0) bad = 1.0;
    if (SITES && off_table) bad = 1.0;
#if BH_RF_MISSING
    if (SITES && !off_table && S.n[(size_t)S.site[ib] * S.ld] == 0) bad = 2.0; // the model's site lacks this target: absent, not bad
#endif
    rec[0] = (double)nlay; rec[1] = p; rec[2] = do_decomp; rec[3] = bad;
    rec[4] = m11; rec[5] = m12; rec[6] = m21; rec[7] = m22;
    rec[REC_HEAD + 40 * (size_t)Lmax] = (im == 0.0) ? 1.0 : 0.0;

// ba_config_ref.cc — CPU reference of bundle adjustment with constant points, written from DESIGN.md 15.12 (the
// addendum to section 15) and section 15 alone.  It includes no product header; it includes tests/ba_ref/ba_ref.cc for
// everything the addendum leaves as it is (the observation, the blocks, the Schur product, PCG, the sums of 15.7) and
// restates what the addendum changes: the mask on J_x, the identity block of a constant point, the counts, the checks
// and the norm of the parameter tolerance.  -ffp-contract=off as ba_ref.
#include "../ba_ref/ba_ref.cc"

namespace {

// 15.12: the stored evaluation with a constant point's J_x as exact zeros
void MaskedEvaluate(const Problem& pb, const std::vector<uint8_t>& pvar, const State& s, Work* w) {
    Evaluate(pb, s, true, w);
    for (size_t o = 0; o < pb.nobs; ++o)
        if (!pvar[pb.opt[o]])
            for (int k = 0; k < 6; ++k) w->Jx[6 * o + k] = 0.0;
}

// 15.12: a constant point's block is the identity's and its gradient is zero.  Its V and g of 15.6 are sums of exact
// zeros, so every pose and camera block sees T = I - 0 and e = r - 0 of that point whichever finite inverse stands in
// Vinv while Blocks() runs; the identity is put there afterwards, for the Schur product and the back-substitution.
void MaskedBlocks(const Problem& pb, const std::vector<uint8_t>& pvar, double radius, Work* w) {
    Blocks(pb, radius, w);
    for (size_t j = 0; j < pb.npts; ++j) {
        if (pvar[j]) continue;
        const double identity[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
        for (int k = 0; k < 6; ++k) w->Vinv[6 * j + k] = identity[k];
        Sym3Mul(identity, &w->gp[3 * j], &w->vg[3 * j]);
    }
}

}  // namespace

extern "C" {

// ba_ref_solve with point_const (npts bytes, non-zero = constant; NULL = none) after xyz; everything else as there
int ba_config_ref_solve(size_t ncam, const int32_t* cmodels, double* cparams, const uint8_t* cconst, size_t nimg,
                 const uint32_t* icam, double* qvec, double* tvec, const uint8_t* pconst, size_t npts, double* xyz, const uint8_t* point_const,
                 size_t nobs, const uint32_t* obs_image, const uint32_t* obs_point, const double* obs_xy,
                 const double* opts, double* stats) {
    Problem pb;
    pb.ncam = ncam;
    pb.nimg = nimg;
    pb.npts = npts;
    pb.nobs = nobs;
    pb.nred = 6 * nimg + kP * ncam;
    pb.loss = static_cast<int>(opts[0]);
    pb.loss_scale = opts[1];
    const int max_it = static_cast<int>(opts[2]), max_lin = static_cast<int>(opts[3]), max_invalid = static_cast<int>(opts[4]);
    const double ftol = opts[5], gtol = opts[6], ptol = opts[7], pcg_tol = opts[8];
    for (int k = 0; k < 12; ++k) stats[k] = 0.0;
    pb.kc = 0;
    pb.cvar.assign(kP * ncam, 0);
    pb.ivar.assign(6 * nimg, 0);
    double nvar = 0.0;
    std::vector<uint8_t> pvar(npts, 1);
    for (size_t j = 0; j < npts; ++j) {
        if (point_const && point_const[j]) pvar[j] = 0;
        else nvar += 3.0;
    }
    for (size_t c = 0; c < ncam; ++c) {
        if (cmodels[c] < 0 || cmodels[c] > 10) return -1;
        const int np = NumParams(cmodels[c]);
        pb.kc = std::max(pb.kc, np);
        pb.cmodel.push_back(cmodels[c]);
        for (int k = 0; k < np; ++k) {
            if (!Finite(cparams[kP * c + k])) return -1;
            if (!cconst[kP * c + k]) {
                pb.cvar[kP * c + k] = 1;
                nvar += 1.0;
            }
        }
    }
    for (size_t k = 0; k < 6 * nimg; ++k)
        if (!pconst[k]) {
            pb.ivar[k] = 1;
            nvar += 1.0;
        }
    std::vector<uint32_t> icount(nimg, 0), pcount(npts, 0);
    for (size_t i = 0; i < nimg; ++i)
        if (icam[i] >= ncam) return -1;
    for (size_t o = 0; o < nobs; ++o) {
        if (obs_image[o] >= nimg || obs_point[o] >= npts) return -1;
        ++icount[obs_image[o]];
        ++pcount[obs_point[o]];
    }
    for (size_t j = 0; j < npts; ++j)
        if (pcount[j] < (pvar[j] ? 2u : 1u)) return -1;  // 15.12: a constant point needs one observation
    for (size_t k = 0; k < 4 * nimg; ++k)
        if (!Finite(qvec[k])) return -1;
    for (size_t k = 0; k < 3 * nimg; ++k)
        if (!Finite(tvec[k])) return -1;
    for (size_t k = 0; k < 3 * npts; ++k)
        if (!Finite(xyz[k])) return -1;
    for (size_t k = 0; k < 2 * nobs; ++k)
        if (!Finite(obs_xy[k])) return -1;
    stats[0] = nvar;
    if (nobs == 0 || nvar == 0.0) {  // 15.12: nothing is variable
        stats[8] = 6;
        return 0;
    }
    // 15.2: observations by image (input order within an image); by point (that order within a point); images by camera
    pb.icam.assign(icam, icam + nimg);
    pb.ioff.assign(nimg + 1, 0);
    pb.poff.assign(npts + 1, 0);
    pb.coff.assign(ncam + 1, 0);
    for (size_t i = 0; i < nimg; ++i) pb.ioff[i + 1] = pb.ioff[i] + icount[i];
    for (size_t j = 0; j < npts; ++j) pb.poff[j + 1] = pb.poff[j] + pcount[j];
    pb.oimg.resize(nobs);
    pb.opt.resize(nobs);
    pb.oxy.resize(2 * nobs);
    pb.pobs.resize(nobs);
    pb.cimg.resize(nimg);
    {
        std::vector<uint32_t> order(nobs);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return obs_image[a] < obs_image[b]; });
        for (size_t k = 0; k < nobs; ++k) {
            pb.oimg[k] = obs_image[order[k]];
            pb.opt[k] = obs_point[order[k]];
            pb.oxy[2 * k] = obs_xy[2 * order[k]];
            pb.oxy[2 * k + 1] = obs_xy[2 * order[k] + 1];
        }
        std::vector<uint32_t> by_point(nobs);
        std::iota(by_point.begin(), by_point.end(), 0u);
        std::stable_sort(by_point.begin(), by_point.end(), [&](uint32_t a, uint32_t b) { return pb.opt[a] < pb.opt[b]; });
        pb.pobs = by_point;
        std::vector<uint32_t> by_cam(nimg);
        std::iota(by_cam.begin(), by_cam.end(), 0u);
        std::stable_sort(by_cam.begin(), by_cam.end(), [&](uint32_t a, uint32_t b) { return icam[a] < icam[b]; });
        pb.cimg = by_cam;
        for (size_t i = 0; i < nimg; ++i) ++pb.coff[icam[i] + 1];
        for (size_t c = 0; c < ncam; ++c) pb.coff[c + 1] += pb.coff[c];
    }
    State cur, cand;
    cur.q.assign(qvec, qvec + 4 * nimg);
    cur.t.assign(tvec, tvec + 3 * nimg);
    cur.cp.assign(kP * ncam, 0.0);
    for (size_t c = 0; c < ncam; ++c)
        for (int k = 0; k < NumParams(cmodels[c]); ++k) cur.cp[kP * c + k] = cparams[kP * c + k];
    cur.X.assign(xyz, xyz + 3 * npts);
    cand = cur;
    Work w;
    w.sc_c.assign(pb.nred, 1.0);
    w.sc_p.assign(3 * npts, 1.0);
    w.Jp.resize(12 * nobs);
    w.Jc.resize(2 * kP * nobs);
    w.Jx.resize(6 * nobs);
    w.res.resize(2 * nobs);
    w.cost.resize(nobs);
    w.Vinv.resize(6 * npts);
    w.gp.resize(3 * npts);
    w.vg.resize(3 * npts);
    w.diag_p.resize(3 * npts);
    for (std::vector<double>* v : {&w.g_c, &w.b_c, &w.D_c, &w.diag_c, &w.x}) v->assign(pb.nred, 0.0);
    w.Minv_i.resize(36 * nimg);
    w.Minv_c.resize(kP * kP * ncam);
    w.cost_img.resize(nimg);
    w.yp.resize(3 * npts);
    w.jy2_img.resize(nimg);

    auto total_cost = [&]() { return Total(nimg, [&](size_t i) { return w.cost_img[i]; }); };
    auto gradient_max = [&]() {
        double m = 0.0;
        for (size_t k = 0; k < pb.nred; ++k) m = std::max(m, std::fabs(w.g_c[k] / w.sc_c[k]));
        for (size_t k = 0; k < 3 * npts; ++k) m = std::max(m, std::fabs(w.gp[k] / w.sc_p[k]));
        return m;
    };
    double radius = 1e4, decrease = 2.0;
    MaskedEvaluate(pb, pvar, cur, &w);
    MaskedBlocks(pb, pvar, radius, &w);
    for (size_t k = 0; k < pb.nred; ++k) w.sc_c[k] = 1.0 / (1.0 + std::sqrt(w.diag_c[k]));
    for (size_t k = 0; k < 3 * npts; ++k) w.sc_p[k] = 1.0 / (1.0 + std::sqrt(w.diag_p[k]));
    MaskedEvaluate(pb, pvar, cur, &w);
    MaskedBlocks(pb, pvar, radius, &w);
    double cost = total_cost();
    stats[1] = cost;
    int term = 3;
    bool stop = false;
    if (!Finite(cost)) {
        term = 5;
        stop = true;
    } else if (gradient_max() <= gtol) {
        term = 2;
        stop = true;
    }
    int invalid_run = 0;
    for (int it = 1; !stop && it <= max_it; ++it) {
        int kind = 0;
        stats[5] += Pcg(pb, &w, max_lin, pcg_tol, &kind);
        if (kind == 1) stats[6] += 1;
        if (kind == 2) stats[7] += 1;
        // back-substitution
        std::vector<double> wsum(3 * npts);
        PointPass(pb, w, w.x, &wsum);
        for (size_t j = 0; j < npts; ++j) {
            double s[3], out[3];
            for (int m = 0; m < 3; ++m) s[m] = w.gp[3 * j + m] + wsum[3 * j + m];
            Sym3Mul(&w.Vinv[6 * j], s, out);
            for (int m = 0; m < 3; ++m) w.yp[3 * j + m] = -out[m];
        }
        // |J y|^2 per image
        for (size_t i = 0; i < nimg; ++i) {
            const size_t o0 = pb.ioff[i], n = pb.ioff[i + 1] - o0;
            w.jy2_img[i] = Total(n, [&](size_t k) {
                const size_t o = o0 + k;
                double a[2];
                ObsTimesReduced(pb, w, o, i, w.x, a);
                const double* Jx = &w.Jx[6 * o];
                const double* y = &w.yp[3 * pb.opt[o]];
                for (int r = 0; r < 2; ++r) a[r] = a[r] + (Jx[3 * r] * y[0] + Jx[3 * r + 1] * y[1] + Jx[3 * r + 2] * y[2]);
                return a[0] * a[0] + a[1] * a[1];
            });
        }
        // the candidate
        for (size_t i = 0; i < nimg; ++i) {
            double dl[6];
            for (int m = 0; m < 6; ++m) dl[m] = w.sc_c[6 * i + m] * w.x[6 * i + m];
            QuatPlus(&cur.q[4 * i], dl, &cand.q[4 * i]);
            for (int m = 0; m < 3; ++m) cand.t[3 * i + m] = cur.t[3 * i + m] + dl[3 + m];
        }
        for (size_t k = 0; k < kP * ncam; ++k) cand.cp[k] = cur.cp[k] + w.sc_c[6 * nimg + k] * w.x[6 * nimg + k];
        for (size_t k = 0; k < 3 * npts; ++k) cand.X[k] = cur.X[k] + w.sc_p[k] * w.yp[k];
        Evaluate(pb, cand, false, &w);
        for (size_t i = 0; i < nimg; ++i) {
            const size_t o0 = pb.ioff[i];
            w.cost_img[i] = Total(pb.ioff[i + 1] - o0, [&](size_t k) { return w.cost[o0 + k]; });
        }
        const double cand_cost = total_cost();
        const double gy = Total(pb.nred, [&](size_t k) { return w.g_c[k] * w.x[k]; }) +
                          Total(3 * npts, [&](size_t k) { return w.gp[k] * w.yp[k]; });
        const double jy2 = Total(nimg, [&](size_t i) { return w.jy2_img[i]; });
        const double step2 = Total(pb.nred, [&](size_t k) { const double v = w.sc_c[k] * w.x[k]; return v * v; }) +
                             Total(3 * npts, [&](size_t k) { const double v = w.sc_p[k] * w.yp[k]; return v * v; });
        const double x2 = Total(4 * nimg, [&](size_t k) { return cur.q[k] * cur.q[k]; }) +
                          Total(3 * nimg, [&](size_t k) { return cur.t[k] * cur.t[k]; }) +
                          Total(kP * ncam, [&](size_t k) { return pb.cvar[k] ? cur.cp[k] * cur.cp[k] : 0.0; }) +
                          Total(3 * npts, [&](size_t k) { return pvar[k / 3] ? cur.X[k] * cur.X[k] : 0.0; });
        const double mcc = -(gy + 0.5 * jy2);
        bool rejected = false;
        if (!(Finite(mcc) && mcc > 0.0)) {
            stats[4] += 1;
            if (++invalid_run >= max_invalid) {
                term = 5;
                break;
            }
            rejected = true;
        } else {
            invalid_run = 0;
            if (std::sqrt(step2) <= ptol * (std::sqrt(x2) + ptol)) {
                term = 1;
                break;
            }
            const double new_cost = Finite(cand_cost) ? cand_cost : DBL_MAX;
            const double change = cost - new_cost;
            if (std::fabs(change) <= ftol * cost) {
                term = 0;
                break;
            }
            const double rel = change / mcc;
            if (rel > 1e-3) {
                stats[3] += 1;
                std::swap(cur, cand);
                const double z = 2.0 * rel - 1.0;
                const double f = 1.0 - z * z * z;
                radius = radius / (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
                radius = radius < 1e16 ? radius : 1e16;
                decrease = 2.0;
                MaskedEvaluate(pb, pvar, cur, &w);
                MaskedBlocks(pb, pvar, radius, &w);
                cost = total_cost();
                if (gradient_max() <= gtol) {
                    term = 2;
                    break;
                }
            } else {
                stats[4] += 1;
                rejected = true;
            }
        }
        if (rejected) {
            radius = radius / decrease;
            decrease = 2.0 * decrease;
            if (radius < 1e-32) {
                term = 4;
                break;
            }
            MaskedBlocks(pb, pvar, radius, &w);
        }
    }
    stats[2] = cost;
    stats[8] = term;
    std::copy(cur.q.begin(), cur.q.end(), qvec);
    std::copy(cur.t.begin(), cur.t.end(), tvec);
    for (size_t c = 0; c < ncam; ++c)
        for (int k = 0; k < NumParams(cmodels[c]); ++k) cparams[kP * c + k] = cur.cp[kP * c + k];
    std::copy(cur.X.begin(), cur.X.end(), xyz);
    return 0;
}

}  // extern "C"

// bacov_ref.cc — sequential CPU reference of the bundle-adjustment covariance, written from DESIGN.md section 24 alone.
// It includes no product header; it includes tests/ba_ref/ba_ref.cc for what section 24 takes from section 15 (the
// observation with its loss corrector, the 3 x 3 inverse, the 64-lane sum of 15.7).  Plain loops over dense arrays: no
// tiles, no plans, no padding.  -ffp-contract=off as ba_ref.
#include "../ba_ref/ba_ref.cc"

namespace {

struct Cov {
    size_t ncam, nimg, npts, nobs, m;
    std::vector<uint32_t> icam, oimg, opt, ioff, poff, pobs;
    std::vector<int> cmodel;
    std::vector<int32_t> icol, ccol;      // 6 per image, 12 per camera: column or -1
    std::vector<uint32_t> ocol;           // first column of owner (images, then cameras), nown + 1
    std::vector<uint32_t> col_owner, col_coord;
    std::vector<uint8_t> pvar;
    std::vector<double> oxy, Jp, Jc, Jx;  // 12, 24 and 6 per observation
};

// 24.1: the compact columns
void Columns(const uint8_t* cconst, const uint8_t* pconst, Cov* c) {
    c->icol.assign(6 * c->nimg, -1);
    c->ccol.assign(kP * c->ncam, -1);
    c->ocol.assign(c->nimg + c->ncam + 1, 0);
    for (size_t i = 0; i < c->nimg; ++i) {
        c->ocol[i] = static_cast<uint32_t>(c->col_owner.size());
        for (int k = 0; k < 6; ++k)
            if (!pconst[6 * i + k]) {
                c->icol[6 * i + k] = static_cast<int32_t>(c->col_owner.size());
                c->col_owner.push_back(static_cast<uint32_t>(i));
                c->col_coord.push_back(k);
            }
    }
    for (size_t a = 0; a < c->ncam; ++a) {
        c->ocol[c->nimg + a] = static_cast<uint32_t>(c->col_owner.size());
        for (int k = 0; k < NumParams(c->cmodel[a]); ++k)
            if (!cconst[kP * a + k]) {
                c->ccol[kP * a + k] = static_cast<int32_t>(c->col_owner.size());
                c->col_owner.push_back(static_cast<uint32_t>(c->nimg + a));
                c->col_coord.push_back(k);
            }
    }
    c->m = c->col_owner.size();
    c->ocol[c->nimg + c->ncam] = static_cast<uint32_t>(c->m);
}

// an observation's Jacobian entry (row a) by local column u: its pose (0 .. 5), then its camera (6 .. 17)
double Jloc(const Cov& c, size_t o, int a, int u) {
    return u < 6 ? c.Jp[12 * o + 6 * a + u] : c.Jc[2 * kP * o + kP * a + (u - 6)];
}

}  // namespace

extern "C" {

// the number of columns of the masks (24.1); -1 for a model outside 0 .. 10
long bacov_ref_num_columns(size_t ncam, const int32_t* cmodels, const uint8_t* cconst, size_t nimg, const uint8_t* pconst) {
    long m = 0;
    for (size_t c = 0; c < ncam; ++c) {
        if (cmodels[c] < 0 || cmodels[c] > 10) return -1;
        for (int k = 0; k < NumParams(cmodels[c]); ++k) m += cconst[kP * c + k] ? 0 : 1;
    }
    for (size_t k = 0; k < 6 * nimg; ++k) m += pconst[k] ? 0 : 1;
    return m;
}

// opts: loss type, loss scale, damping.  info (4): success, columns, min_pivot_ratio, failed column (-1).  col_owner,
// col_coord (m), matrix (m x m), point_present (npts), point_cov (npts x 9) are the caller's, sized by
// bacov_ref_num_columns.  Returns 0, -1 for input the product refuses as AMC_E_INVALID.  Nothing of the problem is written.
int bacov_ref_run(size_t ncam, const int32_t* cmodels, const double* cparams, const uint8_t* cconst, size_t nimg,
                  const uint32_t* icam, const double* qvec, const double* tvec, const uint8_t* pconst, size_t npts,
                  const double* xyz, const uint8_t* point_const, size_t nobs, const uint32_t* obs_image,
                  const uint32_t* obs_point, const double* obs_xy, const double* opts, double* info, uint32_t* col_owner,
                  uint32_t* col_coord, double* matrix, uint8_t* point_present, double* point_cov) {
    const int loss = static_cast<int>(opts[0]);
    const double loss_scale = opts[1], damping = opts[2];
    info[0] = 0.0;
    info[1] = 0.0;
    info[2] = 1.0;
    info[3] = -1.0;
    if (loss < 0 || loss > 2 || !(loss_scale > 0.0) || !Finite(loss_scale) || !(damping >= 0.0) || !Finite(damping)) return -1;
    Cov c;
    c.ncam = ncam;
    c.nimg = nimg;
    c.npts = npts;
    c.nobs = nobs;
    // the checks of 15.2 and 15.12
    std::vector<double> cp(kP * ncam, 0.0);
    for (size_t a = 0; a < ncam; ++a) {
        if (cmodels[a] < 0 || cmodels[a] > 10) return -1;
        c.cmodel.push_back(cmodels[a]);
        for (int k = 0; k < NumParams(cmodels[a]); ++k) {
            if (!Finite(cparams[kP * a + k])) return -1;
            cp[kP * a + k] = cparams[kP * a + k];
        }
    }
    for (size_t i = 0; i < nimg; ++i)
        if (icam[i] >= ncam) return -1;
    std::vector<uint32_t> icount(nimg, 0), pcount(npts, 0);
    for (size_t o = 0; o < nobs; ++o) {
        if (obs_image[o] >= nimg || obs_point[o] >= npts) return -1;
        ++icount[obs_image[o]];
        ++pcount[obs_point[o]];
    }
    c.pvar.assign(npts, 1);
    for (size_t j = 0; j < npts; ++j) {
        if (point_const && point_const[j]) c.pvar[j] = 0;
        if (pcount[j] < (c.pvar[j] ? 2u : 1u)) return -1;
    }
    for (size_t k = 0; k < 4 * nimg; ++k)
        if (!Finite(qvec[k])) return -1;
    for (size_t k = 0; k < 3 * nimg; ++k)
        if (!Finite(tvec[k])) return -1;
    for (size_t k = 0; k < 3 * npts; ++k)
        if (!Finite(xyz[k])) return -1;
    for (size_t k = 0; k < 2 * nobs; ++k)
        if (!Finite(obs_xy[k])) return -1;
    c.icam.assign(icam, icam + nimg);
    Columns(cconst, pconst, &c);
    const size_t m = c.m;
    info[1] = static_cast<double>(m);
    if (m > 8192) return -1;
    for (size_t j = 0; j < npts; ++j) {
        point_present[j] = 0;
        for (int k = 0; k < 9; ++k) point_cov[9 * j + k] = 0.0;
    }
    for (size_t k = 0; k < m; ++k) {
        col_owner[k] = c.col_owner[k];
        col_coord[k] = c.col_coord[k];
    }
    if (m == 0) {
        info[0] = 1.0;
        return 0;
    }
    // 15.2's orders: by image keeping the input order, by point keeping that order
    {
        std::vector<uint32_t> order(nobs);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return obs_image[a] < obs_image[b]; });
        c.oimg.resize(nobs);
        c.opt.resize(nobs);
        c.oxy.resize(2 * nobs);
        for (size_t k = 0; k < nobs; ++k) {
            c.oimg[k] = obs_image[order[k]];
            c.opt[k] = obs_point[order[k]];
            c.oxy[2 * k] = obs_xy[2 * order[k]];
            c.oxy[2 * k + 1] = obs_xy[2 * order[k] + 1];
        }
        c.pobs.resize(nobs);
        std::iota(c.pobs.begin(), c.pobs.end(), 0u);
        std::stable_sort(c.pobs.begin(), c.pobs.end(), [&](uint32_t a, uint32_t b) { return c.opt[a] < c.opt[b]; });
        c.ioff.assign(nimg + 1, 0);
        c.poff.assign(npts + 1, 0);
        for (size_t i = 0; i < nimg; ++i) c.ioff[i + 1] = c.ioff[i] + icount[i];
        for (size_t j = 0; j < npts; ++j) c.poff[j + 1] = c.poff[j] + pcount[j];
    }
    // 24.2: the Jacobian, unscaled and unmasked
    c.Jp.resize(12 * nobs);
    c.Jc.resize(2 * kP * nobs);
    c.Jx.resize(6 * nobs);
    for (size_t o = 0; o < nobs; ++o) {
        const uint32_t i = c.oimg[o], j = c.opt[o], a = c.icam[i];
        double r[2];
        Observation(c.cmodel[a], &cp[kP * a], &qvec[4 * i], &tvec[3 * i], &xyz[3 * j], &c.oxy[2 * o], loss, loss_scale, true,
                    r, &c.Jp[12 * o], &c.Jc[2 * kP * o], &c.Jx[6 * o]);
    }
    // 24.2: point blocks
    std::vector<double> Vinv(6 * npts, 0.0);
    for (size_t j = 0; j < npts; ++j) {
        if (!c.pvar[j]) continue;
        double V[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t k = c.poff[j]; k < c.poff[j + 1]; ++k) {
            const double* J = &c.Jx[6 * c.pobs[k]];
            V[0] = V[0] + (J[0] * J[0] + J[3] * J[3]);
            V[1] = V[1] + (J[0] * J[1] + J[3] * J[4]);
            V[2] = V[2] + (J[0] * J[2] + J[3] * J[5]);
            V[3] = V[3] + (J[1] * J[1] + J[4] * J[4]);
            V[4] = V[4] + (J[1] * J[2] + J[4] * J[5]);
            V[5] = V[5] + (J[2] * J[2] + J[5] * J[5]);
        }
        V[0] = V[0] + damping;
        V[3] = V[3] + damping;
        V[5] = V[5] + damping;
        Sym3Inverse(V, &Vinv[6 * j]);
    }
    // 24.3: B, the lower triangle of S
    std::vector<double> S(m * m, 0.0);
    std::vector<double> campart(78 * nimg, 0.0);
    for (size_t i = 0; i < nimg; ++i) {
        const uint32_t a = c.icam[i];
        for (int u = 0; u < 18; ++u)
            for (int v = 0; v <= u; ++v) {
                const int32_t cu = u < 6 ? c.icol[6 * i + u] : c.ccol[kP * a + u - 6];
                const int32_t cv = v < 6 ? c.icol[6 * i + v] : c.ccol[kP * a + v - 6];
                if (cu < 0 || cv < 0) continue;
                const size_t o0 = c.ioff[i];
                const double s = Total(c.ioff[i + 1] - o0, [&](size_t k) {
                    return Jloc(c, o0 + k, 0, u) * Jloc(c, o0 + k, 0, v) + Jloc(c, o0 + k, 1, u) * Jloc(c, o0 + k, 1, v);
                });
                if (v >= 6)
                    campart[78 * i + (u - 6) * (u - 5) / 2 + (v - 6)] = s;
                else
                    S[cu * m + cv] = s;
            }
    }
    for (size_t a = 0; a < ncam; ++a)
        for (int u = 0; u < kP; ++u)
            for (int v = 0; v <= u; ++v) {
                const int32_t cu = c.ccol[kP * a + u], cv = c.ccol[kP * a + v];
                if (cu < 0 || cv < 0) continue;
                double s = 0.0;
                for (size_t i = 0; i < nimg; ++i)
                    if (c.icam[i] == a) s = s + campart[78 * i + u * (u + 1) / 2 + v];
                S[cu * m + cv] = s;
            }
    // 24.3: the point terms, point by point in ascending index; W kept for 24.6
    std::vector<std::vector<uint32_t>> owners(npts);
    std::vector<std::vector<double>> Ws(npts);  // per owner 3 x 12
    for (size_t j = 0; j < npts; ++j) {
        if (!c.pvar[j]) continue;
        std::vector<uint32_t>& own = owners[j];
        std::vector<uint32_t> cams;
        for (uint32_t k = c.poff[j]; k < c.poff[j + 1]; ++k) {
            const uint32_t i = c.oimg[c.pobs[k]], a = static_cast<uint32_t>(nimg) + c.icam[i];
            if (c.ocol[i + 1] > c.ocol[i] && std::find(own.begin(), own.end(), i) == own.end()) own.push_back(i);
            if (c.ocol[a + 1] > c.ocol[a] && std::find(cams.begin(), cams.end(), a) == cams.end()) cams.push_back(a);
        }
        std::sort(cams.begin(), cams.end());
        own.insert(own.end(), cams.begin(), cams.end());
        std::vector<double>& W = Ws[j];
        W.assign(36 * own.size(), 0.0);
        std::vector<double> Y(36 * own.size(), 0.0);
        for (size_t s = 0; s < own.size(); ++s) {
            const uint32_t A = own[s], k0 = c.ocol[A], kn = c.ocol[A + 1] - k0;
            for (uint32_t p = 0; p < kn; ++p) {
                const uint32_t coord = c.col_coord[k0 + p];
                double w[3] = {0, 0, 0}, y[3];
                for (uint32_t k = c.poff[j]; k < c.poff[j + 1]; ++k) {
                    const uint32_t o = c.pobs[k], i = c.oimg[o];
                    if (A < nimg ? i != A : c.icam[i] != A - nimg) continue;
                    const int u = A < nimg ? static_cast<int>(coord) : 6 + static_cast<int>(coord);
                    const double j0 = Jloc(c, o, 0, u), j1 = Jloc(c, o, 1, u);
                    for (int a = 0; a < 3; ++a) w[a] = w[a] + (c.Jx[6 * o + a] * j0 + c.Jx[6 * o + 3 + a] * j1);
                }
                Sym3Mul(&Vinv[6 * j], w, y);
                for (int a = 0; a < 3; ++a) {
                    W[36 * s + 12 * a + p] = w[a];
                    Y[36 * s + 12 * a + p] = y[a];
                }
            }
        }
        for (size_t sa = 0; sa < own.size(); ++sa)
            for (size_t sb = 0; sb < own.size(); ++sb) {
                const uint32_t A = own[sa], B = own[sb];
                if (A < B) continue;
                const uint32_t ra = c.ocol[A], rb = c.ocol[B], ka = c.ocol[A + 1] - ra, kb = c.ocol[B + 1] - rb;
                for (uint32_t p = 0; p < ka; ++p)
                    for (uint32_t q = 0; q < kb; ++q) {
                        if (A == B && q > p) continue;
                        const double term = Y[36 * sa + p] * W[36 * sb + q] + Y[36 * sa + 12 + p] * W[36 * sb + 12 + q] +
                                            Y[36 * sa + 24 + p] * W[36 * sb + 24 + q];
                        S[(ra + p) * m + rb + q] = S[(ra + p) * m + rb + q] - term;
                    }
            }
    }
    // 24.4: Cholesky
    std::vector<double> L(m * m, 0.0);
    double min_ratio = 1.0;
    for (size_t q = 0; q < m; ++q) {
        double dq = S[q * m + q];
        for (size_t k = 0; k < q; ++k) dq = dq - (L[q * m + k] * L[q * m + k]);
        if (!(dq > 0.0) || !Finite(dq)) {
            info[2] = min_ratio;
            info[3] = static_cast<double>(q);
            return 0;
        }
        const double ratio = dq / S[q * m + q];
        if (ratio < min_ratio) min_ratio = ratio;
        const double lqq = std::sqrt(dq);
        L[q * m + q] = lqq;
        for (size_t p = q + 1; p < m; ++p) {
            double v = S[p * m + q];
            for (size_t k = 0; k < q; ++k) v = v - (L[p * m + k] * L[q * m + k]);
            L[p * m + q] = v / lqq;
        }
    }
    info[2] = min_ratio;
    // 24.5: Z = L^-1, Sigma = Z^T Z
    std::vector<double> Z(m * m, 0.0);
    for (size_t col = 0; col < m; ++col)
        for (size_t p = col; p < m; ++p) {
            double v = p == col ? 1.0 : 0.0;
            for (size_t k = col; k < p; ++k) v = v - (L[p * m + k] * Z[k * m + col]);
            Z[p * m + col] = v / L[p * m + p];
        }
    // (Z^T is walked row by row below: a transposed copy keeps the inner loop contiguous)
    std::vector<double> Zt(m * m);
    for (size_t k = 0; k < m; ++k)
        for (size_t a = 0; a < m; ++a) Zt[a * m + k] = Z[k * m + a];
    for (size_t a = 0; a < m; ++a)
        for (size_t b = 0; b <= a; ++b) {
            double s = 0.0;
            for (size_t k = a; k < m; ++k) s = s + (Zt[a * m + k] * Zt[b * m + k]);
            matrix[a * m + b] = s;
            matrix[b * m + a] = s;
        }
    // 24.6: point covariances
    for (size_t j = 0; j < npts; ++j) {
        if (!c.pvar[j]) continue;
        const std::vector<uint32_t>& own = owners[j];
        const std::vector<double>& W = Ws[j];
        double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t sa = 0; sa < own.size(); ++sa)
            for (size_t sb = 0; sb < own.size(); ++sb) {
                const uint32_t ra = c.ocol[own[sa]], rb = c.ocol[own[sb]];
                const uint32_t ka = c.ocol[own[sa] + 1] - ra, kb = c.ocol[own[sb] + 1] - rb;
                for (uint32_t p = 0; p < ka; ++p)
                    for (uint32_t q = 0; q < kb; ++q) {
                        const double sig = matrix[(ra + p) * m + rb + q];
                        for (int a = 0; a < 3; ++a) {
                            const double ws = W[36 * sa + 12 * a + p] * sig;
                            for (int b = 0; b < 3; ++b) M[3 * a + b] = M[3 * a + b] + ws * W[36 * sb + 12 * b + q];
                        }
                    }
            }
        const double* v = &Vinv[6 * j];
        const double Vi[3][3] = {{v[0], v[1], v[2]}, {v[1], v[3], v[4]}, {v[2], v[4], v[5]}};
        double P[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) P[a][b] = Vi[a][0] * M[b] + Vi[a][1] * M[3 + b] + Vi[a][2] * M[6 + b];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                point_cov[9 * j + 3 * a + b] = Vi[a][b] + (P[a][0] * Vi[0][b] + P[a][1] * Vi[1][b] + P[a][2] * Vi[2][b]);
        point_present[j] = 1;
    }
    info[0] = 1.0;
    return 0;
}

}  // extern "C"

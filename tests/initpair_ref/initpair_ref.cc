// Sequential CPU reference of the two-view triangulation of image pairs and of the scene normalisation, written from
// DESIGN.md section 21 without any product header.  It includes tests/tri_ref/tri_ref.cc for section 11's numerics (acos,
// the triangulation angle, the depth, the round-robin Jacobi and the dehomogenised smallest eigenvector).  Pixels arrive
// lifted to the normalised image plane (tests/initpair_ref_lib.py does that with the oracle's Camera::CamFromImg).
// Built by tests/initpair_ref_lib.py with -ffp-contract=off.
#include "../tri_ref/tri_ref.cc"

#include <algorithm>

namespace {

// 11.1: [R | t] from the quaternion (x, y, z, w) and the centre -(R^T t)
Pose PairPose(const double* q, const double* t) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy,
                         tyz + twx, 1.0 - (txx + tyy)};
    Pose p;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.P[r][c] = R[3 * r + c];
        p.P[r][3] = t[r];
    }
    for (int c = 0; c < 3; ++c) p.C[c] = -(p.P[0][c] * p.P[0][3] + p.P[1][c] * p.P[1][3] + p.P[2][c] * p.P[2][3]);
    return p;
}

// 21.2: TriangulatePoint's DLT on the normalised points (x1, y1) and (x2, y2)
Vec3 TriangulatePoint(const Pose& p1, const Pose& p2, double x1, double y1, double x2, double y2) {
    double A[4][4];
    for (int c = 0; c < 4; ++c) {
        A[0][c] = x1 * p1.P[2][c] - p1.P[0][c];
        A[1][c] = y1 * p1.P[2][c] - p1.P[1][c];
        A[2][c] = x2 * p2.P[2][c] - p2.P[0][c];
        A[3][c] = y2 * p2.P[2][c] - p2.P[1][c];
    }
    double ata[4][4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[k][r] * A[k][c];
            ata[r][c] = s;
        }
    return SmallestDehom(ata);
}

}  // namespace

extern "C" {

// per correspondence: accepted, xyz, tri_angle (every NaN the canonical quiet NaN) and, when asked for, the two depths.
// Returns 0, or -1 for offsets that do not start at 0 or decrease or an image index out of range.
int initpair_ref_triangulate(size_t nimg, const double* qvec, const double* tvec, size_t npairs, const uint32_t* pair_images,
                             const uint64_t* pair_offsets, const double* nxy1, const double* nxy2, double min_tri_angle,
                             uint8_t* accepted, double* xyz, double* tri_angle, double* depths) {
    if (pair_offsets[0] != 0) return -1;
    for (size_t p = 0; p < npairs; ++p)
        if (pair_offsets[p + 1] < pair_offsets[p] || pair_images[2 * p] >= nimg || pair_images[2 * p + 1] >= nimg) return -1;
    std::vector<Pose> poses(nimg);
    for (size_t i = 0; i < nimg; ++i) poses[i] = PairPose(qvec + 4 * i, tvec + 3 * i);
    for (size_t p = 0; p < npairs; ++p) {
        const Pose& p1 = poses[pair_images[2 * p]];
        const Pose& p2 = poses[pair_images[2 * p + 1]];
        for (uint64_t k = pair_offsets[p]; k < pair_offsets[p + 1]; ++k) {
            const Vec3 X = TriangulatePoint(p1, p2, nxy1[2 * k], nxy1[2 * k + 1], nxy2[2 * k], nxy2[2 * k + 1]);
            double a = TriAngle(p1.C, p2.C, X);
            const double d1 = Depth(p1, X), d2 = Depth(p2, X);
            accepted[k] = (a >= min_tri_angle && d1 >= DBL_EPSILON && d2 >= DBL_EPSILON) ? 1 : 0;
            if (a != a) a = std::numeric_limits<double>::quiet_NaN();
            for (int c = 0; c < 3; ++c) xyz[3 * k + c] = X.v[c];
            tri_angle[k] = a;
            if (depths) {
                depths[2 * k] = d1;
                depths[2 * k + 1] = d2;
            }
        }
    }
    return 0;
}

}  // extern "C"

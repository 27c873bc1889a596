// fusion_core.h — the float32 arithmetic of stereo fusion, shared by fusion.hip and the
// sequential reference in tests/fusion_ref: lift, projection, the three consistency tests, the median's order and the
// final point.  Both sides compile with -ffp-contract=off -fno-fast-math, so every expression below rounds the same way
// on the host and on the device.  Nothing here walks a cluster: the kernel and the reference each do that their own way.
#ifndef AMC_FUSION_CORE_H_
#define AMC_FUSION_CORE_H_

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FU_HD __host__ __device__ __forceinline__
#else
#define FU_HD inline
#endif

namespace fu {

// One image's camera, computed once in double by make_cam and rounded to float32 (23.1).
struct Cam {
    float P[12];   // K [R | t], row-major 3 x 4
    float A[9];    // (K R)^-1 = R^T K^-1: the lift's matrix
    float c[3];    // -R^T t: the camera's centre
    float RT[9];   // R^T: a camera-frame normal into the world
};

// The thresholds as the device compares them (host doubles rounded once).
struct Params {
    int32_t min_num_pixels, limit, probe, max_traversal_depth;  // limit = min(max_num_pixels, the library's bound)
    float max_depth_error, cos_max_normal, max_reproj_sq;
    float box_lo[3], box_hi[3];
};

inline Cam make_cam(const double* K, const double* R, const double* t) {
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const double Km[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    const double Ki[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
    Cam cam;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            double p = 0.0, a = 0.0;
            for (int k = 0; k < 3; ++k) {
                p += Km[3 * r + k] * R[3 * k + c];
                a += R[3 * k + r] * Ki[3 * k + c];
            }
            cam.P[4 * r + c] = (float)p;
            cam.A[3 * r + c] = (float)a;
            cam.RT[3 * r + c] = (float)R[3 * c + r];
        }
        cam.P[4 * r + 3] = (float)(Km[3 * r] * t[0] + Km[3 * r + 1] * t[1] + Km[3 * r + 2] * t[2]);
        cam.c[r] = (float)(-(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]));
    }
    return cam;
}

inline Params make_params(int min_num_pixels, int max_num_pixels, int max_cluster, int max_traversal_depth, double max_reproj_error,
                          double max_depth_error, double max_normal_error_deg, const double* box) {
    Params p;
    p.min_num_pixels = min_num_pixels;
    p.limit = max_num_pixels < max_cluster ? max_num_pixels : max_cluster;
    p.probe = max_num_pixels > max_cluster ? 1 : 0;
    p.max_traversal_depth = max_traversal_depth;
    p.max_depth_error = (float)max_depth_error;
    p.cos_max_normal = (float)std::cos(max_normal_error_deg * 3.14159265358979323846 / 180.0);
    p.max_reproj_sq = (float)(max_reproj_error * max_reproj_error);
    for (int k = 0; k < 3; ++k) {
        p.box_lo[k] = (float)box[k];
        p.box_hi[k] = (float)box[3 + k];
    }
    return p;
}

// The world point of pixel centre (u, v) at depth z.
FU_HD void lift(const Cam& cam, float u, float v, float z, float X[3]) {
    const float uz = u * z, vz = v * z;
    for (int k = 0; k < 3; ++k) X[k] = ((cam.A[3 * k] * uz + cam.A[3 * k + 1] * vz) + cam.A[3 * k + 2] * z) + cam.c[k];
}

// P X: p[2] is the depth, (p[0] / p[2], p[1] / p[2]) the pixel coordinate.
FU_HD void project(const Cam& cam, const float X[3], float p[3]) {
    for (int k = 0; k < 3; ++k) p[k] = ((cam.P[4 * k] * X[0] + cam.P[4 * k + 1] * X[1]) + cam.P[4 * k + 2] * X[2]) + cam.P[4 * k + 3];
}

// The pixel of a w x h map that contains the projection p, or false: behind the camera, outside, or not a number.
FU_HD bool pixel_of(const float p[3], int w, int h, int& row, int& col) {
    if (!(p[2] > 0.0f)) return false;
    const float u = p[0] / p[2], v = p[1] / p[2];
    if (!(u >= 0.0f && u < (float)w && v >= 0.0f && v < (float)h)) return false;
    col = (int)floorf(u);
    row = (int)floorf(v);
    return true;
}

// A camera-frame normal in the world.
FU_HD void world_normal(const Cam& cam, float nx, float ny, float nz, float N[3]) {
    for (int k = 0; k < 3; ++k) N[k] = (cam.RT[3 * k] * nx + cam.RT[3 * k + 1] * ny) + cam.RT[3 * k + 2] * nz;
}

// Test 3: the seed's point seen from the child's image against the child's own depth z (> 0).
FU_HD float depth_err(float proj_z, float z) { return fabsf(proj_z - z) / z; }
FU_HD bool depth_ok(const Params& p, float proj_z, float z) { return depth_err(proj_z, z) <= p.max_depth_error; }

// Test 4.
FU_HD float normal_dot(const float Ns[3], const float Nb[3]) { return (Ns[0] * Nb[0] + Ns[1] * Nb[1]) + Ns[2] * Nb[2]; }
FU_HD bool normal_ok(const Params& p, const float Ns[3], const float Nb[3]) { return normal_dot(Ns, Nb) >= p.cos_max_normal; }

// Test 5: the child's own point Xc in the seed's image against the seed's centre (su, sv).
FU_HD float reproj_sq(const Cam& seed_cam, const float Xc[3], float su, float sv) {
    float q[3];
    project(seed_cam, Xc, q);
    const float du = q[0] / q[2] - su, dv = q[1] / q[2] - sv;
    return du * du + dv * dv;
}
FU_HD bool reproj_ok(const Params& p, const Cam& seed_cam, const float Xc[3], float su, float sv) {
    return reproj_sq(seed_cam, Xc, su, sv) <= p.max_reproj_sq;
}

// The median's order: a total order on float32 bit patterns that agrees with < on numbers (-0 before +0).
FU_HD uint32_t order_key(float x) {
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(x);
#else
    std::memcpy(&b, &x, 4);
#endif
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The median from the two middle order statistics (the same value twice for an odd count).
FU_HD float median_of(float lo, float hi, bool odd) { return odd ? lo : (lo + hi) * 0.5f; }
FU_HD uint32_t median_of_u8(uint32_t lo, uint32_t hi) { return (lo + hi + 1u) >> 1; }  // the mean, rounded half up

// The unit normal, or zero when the length is not a positive number.
FU_HD void normalise(float n[3]) {
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    if (!(len > 0.0f) || !(len <= 3.402823466e38f)) {
        n[0] = n[1] = n[2] = 0.0f;
        return;
    }
    n[0] /= len;
    n[1] /= len;
    n[2] /= len;
}

// A point that is not a number is outside every box.
FU_HD bool in_box(const Params& p, const float X[3]) {
    for (int k = 0; k < 3; ++k)
        if (!(X[k] >= p.box_lo[k] && X[k] <= p.box_hi[k])) return false;
    return true;
}

// A claim cell holds step + 1 of the step that took the pixel; it counts in step `step` only when it is older.
FU_HD bool claimed(uint32_t cell, uint32_t step) { return cell > 0u && cell <= step; }

}  // namespace fu

#endif  // AMC_FUSION_CORE_H_

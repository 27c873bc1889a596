// initpair.hip — two-view triangulation of image pairs on gfx950 (include/amc_initpair.h): the correspondence loop of
// COLMAP 3.9.1's IncrementalMapper::RegisterInitialImagePair restated in DESIGN.md 21.2.  Every FP64 operation is
// written in the order of that section and of section 11, the order tests/initpair_ref follows too: the two are
// bit-identical.
//
// Work split (21.4).  One lane per image builds [R | t] and the projection centre as 11.1 does.  Then one lane per
// correspondence: the host gives it its pair's index, the pair gives the two images; the lane lifts both pixels with
// cam::cam_from_img (the models that need libm are lifted on the host, as everywhere in this library), solves the DLT
// with tri_core.h's two-view estimator, and takes the angle with tri_angle.h and the depths with tri_depth.  A lane
// reads its own two pixels and writes its own three outputs: no atomics, no LDS, no compaction; the host walks the
// accepted bytes in order.
#include <cfloat>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "amc_internal.h"
#include "camera_math.h"
#include "tri_core.h"
#include "../../include/amc_initpair.h"

using namespace amc;

namespace {

using tri::TriPose;

constexpr int kBlock = 256;
constexpr int kKC = cam::kMaxParams;
constexpr long long kDefaultBatchCorrs = 1ll << 22;  // correspondences per launch

struct Dev {
    uint32_t nimg;
    double min_tri_angle;
    const int32_t* cmodel;
    const double* cparams;
    const uint32_t* icam;
    const double *q, *t;
    TriPose* poses;
    const uint32_t* pimg;   // 2 per pair
    const uint32_t* cpair;  // per correspondence: its pair
    const double *xy1, *xy2;
    const double *nxy1, *nxy2;  // the host's lift of the libm models' pixels; nullptr when no camera needs it
    uint8_t* acc;
    double* xyz;
    double* angle;
    uint32_t first, last;  // the launch's correspondences
};

// tri_core.h's view of one correspondence: observation 0 is the first image's, observation 1 the second's
struct PairView {
    double u0, v0, u1, v1;
    const TriPose *p0, *p1;
    double min_tri_angle;
    __device__ __forceinline__ double x(uint64_t o) const { return o ? u1 : u0; }
    __device__ __forceinline__ double y(uint64_t o) const { return o ? v1 : v0; }
    __device__ __forceinline__ const TriPose& pose(uint64_t o) const { return o ? *p1 : *p0; }
};

unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// 11.1: [R | t] with the Rigid3d binding's quaternion -> matrix arithmetic, the centre -(R^T t)
__global__ __launch_bounds__(kBlock) void initpair_pose_kernel(Dev d) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= d.nimg) return;
    const double x = d.q[4 * i], y = d.q[4 * i + 1], z = d.q[4 * i + 2], w = d.q[4 * i + 3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy,
                         tyz + twx, 1.0 - (txx + tyy)};
    TriPose& p = d.poses[i];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.P[4 * r + c] = R[3 * r + c];
        p.P[4 * r + 3] = d.t[3 * i + r];
    }
    for (int c = 0; c < 3; ++c) p.C[c] = -(p.P[c] * p.P[3] + p.P[4 + c] * p.P[7] + p.P[8 + c] * p.P[11]);
    p.pad = 0.0;
}

// Camera::CamFromImg of one pixel of image `img`
__device__ __forceinline__ void lift(const Dev& d, uint32_t img, const double* xy, const double* nxy, size_t k, double& u, double& v) {
    const uint32_t c = d.icam[img];
    const int model = d.cmodel[c];
    if (cam::needs_libm(model)) {  // the host's value
        u = nxy[2 * k];
        v = nxy[2 * k + 1];
        return;
    }
    double prm[kKC];
    for (int i = 0; i < kKC; ++i) prm[i] = d.cparams[kKC * (size_t)c + i];
    cam::cam_from_img(model, prm, xy[2 * k], xy[2 * k + 1], u, v);
}

// 21.2 for one correspondence per lane
__global__ __launch_bounds__(kBlock) void initpair_corr_kernel(Dev d) {
    const uint64_t g = (uint64_t)d.first + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= d.last) return;
    const size_t k = (size_t)g;
    const uint32_t p = d.cpair[k];
    const uint32_t i1 = d.pimg[2 * (size_t)p], i2 = d.pimg[2 * (size_t)p + 1];
    PairView v;
    lift(d, i1, d.xy1, d.nxy1, k, v.u0, v.v0);
    lift(d, i2, d.xy2, d.nxy2, k, v.u1, v.v1);
    v.p0 = d.poses + i1;
    v.p1 = d.poses + i2;
    v.min_tri_angle = d.min_tri_angle;
    double X[3];
    // the DLT, then depth 1 >= eps && depth 2 >= eps && angle >= min_tri_angle (NaN fails every comparison)
    const bool ok = tri::tri_estimate_two(v, 0, 1, X);
    double a = tri::tri_angle(v.p0->C, v.p1->C, X);
    if (a != a) a = __longlong_as_double(0x7ff8000000000000ll);
    d.acc[k] = ok ? 1 : 0;
    d.xyz[3 * k] = X[0];
    d.xyz[3 * k + 1] = X[1];
    d.xyz[3 * k + 2] = X[2];
    d.angle[k] = a;
}

// What is wrong with the problem, or the empty string.  Nothing is read through an offset or an index before it has
// been checked.
std::string check_problem(const amc_pair_tri_problem& pb) {
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, np = pb.num_pairs;
    if (!pb.pair_offsets) return "NULL pair_offsets";
    if ((ncam && (!pb.camera_models || !pb.camera_params)) || (nimg && (!pb.image_cameras || !pb.qvec || !pb.tvec))) return "NULL array";
    if (ncam > 0x7fffffffu / 16 || nimg > 0x7fffffffu / 16 || np > 0x7fffffffu) return "too many cameras, images or pairs for 32-bit indices";
    if (np && !pb.pair_images) return "NULL pair_images";
    if (pb.pair_offsets[0] != 0) return "pair_offsets does not start at 0";
    for (size_t p = 0; p < np; ++p)
        if (pb.pair_offsets[p + 1] < pb.pair_offsets[p]) return "pair_offsets decreases at pair " + std::to_string(p);
    const uint64_t n = pb.pair_offsets[np];
    if (n > AMC_INITPAIR_MAX_CORRS)
        return std::to_string(n) + " correspondences, more than " + std::to_string(AMC_INITPAIR_MAX_CORRS) + " (AMC_INITPAIR_MAX_CORRS)";
    if (n && (!pb.corr_xy1 || !pb.corr_xy2)) return "NULL correspondences";
    for (size_t c = 0; c < ncam; ++c)
        if (pb.camera_models[c] < 0 || pb.camera_models[c] >= cam::kNumModels)
            return "camera " + std::to_string(c) + " has model " + std::to_string(pb.camera_models[c]);
    for (size_t i = 0; i < nimg; ++i)
        if (pb.image_cameras[i] >= ncam) return "image " + std::to_string(i) + " has camera index " + std::to_string(pb.image_cameras[i]);
    for (size_t p = 0; p < np; ++p)
        if (pb.pair_images[2 * p] >= nimg || pb.pair_images[2 * p + 1] >= nimg) return "pair " + std::to_string(p) + " names an image out of range";
    return std::string();
}

void free_arrays(amc_pair_tri_result* r) {
    std::free(r->accepted);
    std::free(r->xyz);
    std::free(r->tri_angle);
    r->accepted = nullptr;
    r->xyz = nullptr;
    r->tri_angle = nullptr;
}

// the host's plan: every correspondence's pair, and Camera::CamFromImg with the host's libm for the pixels whose
// camera model needs it (camera_math.h has the why)
struct Plan {
    std::vector<uint32_t> cpair;
    std::vector<double> nxy1, nxy2;
    bool host_lift = false;
};

void make_plan(const amc_pair_tri_problem& pb, Plan* plan) {
    const size_t np = pb.num_pairs;
    const uint64_t n = pb.pair_offsets[np];
    plan->cpair.resize(n);
    for (size_t p = 0; p < np; ++p)
        for (uint64_t k = pb.pair_offsets[p]; k < pb.pair_offsets[p + 1]; ++k) plan->cpair[k] = (uint32_t)p;
    bool any = false;
    for (size_t c = 0; c < pb.num_cameras && !any; ++c) any = cam::needs_libm(pb.camera_models[c]);
    if (!any) return;
    plan->nxy1.assign(2 * n, 0.0);
    plan->nxy2.assign(2 * n, 0.0);
    for (size_t p = 0; p < np; ++p)
        for (int side = 0; side < 2; ++side) {
            const uint32_t c = pb.image_cameras[pb.pair_images[2 * p + side]];
            if (!cam::needs_libm(pb.camera_models[c])) continue;
            const double* xy = side ? pb.corr_xy2 : pb.corr_xy1;
            std::vector<double>& nxy = side ? plan->nxy2 : plan->nxy1;
            for (uint64_t k = pb.pair_offsets[p]; k < pb.pair_offsets[p + 1]; ++k) {
                cam::cam_from_img(pb.camera_models[c], pb.camera_params + kKC * (size_t)c, xy[2 * k], xy[2 * k + 1], nxy[2 * k], nxy[2 * k + 1]);
                plan->host_lift = true;
            }
        }
}

int run_device(amc_ctx* ctx, const amc_pair_tri_problem& pb, const amc_pair_tri_opts& op, const Plan& plan, uint64_t batch,
               amc_pair_tri_result* result) {
    static const char* const hipchk_who = "amc_triangulate_pairs";
    const size_t ncam = pb.num_cameras, nimg = pb.num_images, np = pb.num_pairs;
    const uint64_t n = pb.pair_offsets[np];
    const CtxView cv = ctx_view(ctx);
    HIPCHK(hipSetDevice(cv.device));
    hipStream_t st = cv.stream;
    int32_t* d_cmodel;
    uint32_t *d_icam, *d_pimg, *d_cpair;
    double *d_cparams, *d_q, *d_t, *d_xy1, *d_xy2, *d_nxy1, *d_nxy2;
    Dev d{};
    const size_t nl = plan.host_lift ? n : 0;
    DevBuf<void> mem;  // the call's working set: allocated here, freed on return
    DevParts parts;
    parts.part(&d_cmodel, ncam).part(&d_cparams, kKC * ncam).part(&d_icam, nimg).part(&d_q, 4 * nimg).part(&d_t, 3 * nimg)
        .part(&d.poses, nimg).part(&d_pimg, 2 * np).part(&d_cpair, n).part(&d_xy1, 2 * n).part(&d_xy2, 2 * n)
        .part(&d_nxy1, 2 * nl).part(&d_nxy2, 2 * nl).part(&d.acc, n).part(&d.xyz, 3 * n).part(&d.angle, n);
    {
        const auto t0 = std::chrono::steady_clock::now();
        const hipError_t e = parts.carve(mem);
        if (e == hipErrorOutOfMemory) return api_fail(AMC_E_NOMEM, "%s: out of device memory", hipchk_who);
        HIPCHK(e);
        result->alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // an early return must not leave copies in flight that read the plan or write the result's arrays
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    StreamTimer timer(st), copies(st);
    HIPCHK(timer.start());
    auto up = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
    };
    auto down = [&](void* dst, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    HIPCHK(copies.span_begin());
    HIPCHK(up(d_cmodel, pb.camera_models, ncam * 4));
    HIPCHK(up(d_cparams, pb.camera_params, ncam * kKC * 8));
    HIPCHK(up(d_icam, pb.image_cameras, nimg * 4));
    HIPCHK(up(d_q, pb.qvec, nimg * 32));
    HIPCHK(up(d_t, pb.tvec, nimg * 24));
    HIPCHK(up(d_pimg, pb.pair_images, np * 8));
    HIPCHK(up(d_cpair, plan.cpair.data(), n * 4));
    HIPCHK(up(d_xy1, pb.corr_xy1, n * 16));
    HIPCHK(up(d_xy2, pb.corr_xy2, n * 16));
    if (plan.host_lift) {
        HIPCHK(up(d_nxy1, plan.nxy1.data(), n * 16));
        HIPCHK(up(d_nxy2, plan.nxy2.data(), n * 16));
    }
    HIPCHK(copies.span_end());
    d.nimg = (uint32_t)nimg;
    d.min_tri_angle = op.min_tri_angle;
    d.cmodel = d_cmodel;
    d.cparams = d_cparams;
    d.icam = d_icam;
    d.q = d_q;
    d.t = d_t;
    d.pimg = d_pimg;
    d.cpair = d_cpair;
    d.xy1 = d_xy1;
    d.xy2 = d_xy2;
    // (a problem whose libm cameras no pair uses has host_lift == false and never reads these)
    d.nxy1 = plan.host_lift ? d_nxy1 : nullptr;
    d.nxy2 = plan.host_lift ? d_nxy2 : nullptr;
    HIPCHK(timer.span_begin());
    hipLaunchKernelGGL(initpair_pose_kernel, dim3(blocks_for(nimg)), dim3(kBlock), 0, st, d);
    HIPCHK(hipGetLastError());
    for (uint64_t first = 0; first < n; first += batch) {
        d.first = (uint32_t)first;
        d.last = (uint32_t)std::min<uint64_t>(n, first + batch);
        hipLaunchKernelGGL(initpair_corr_kernel, dim3(blocks_for(d.last - d.first)), dim3(kBlock), 0, st, d);
        HIPCHK(hipGetLastError());
        result->num_batches += 1;
    }
    HIPCHK(timer.span_end());
    HIPCHK(copies.span_begin());
    HIPCHK(down(result->accepted, d.acc, n));
    HIPCHK(down(result->xyz, d.xyz, n * 24));
    HIPCHK(down(result->tri_angle, d.angle, n * 8));
    HIPCHK(copies.span_end());
    HIPCHK(timer.stop(result->device_ms));
    HIPCHK(timer.spans(result->kernel_ms));
    HIPCHK(copies.spans(result->copy_ms));
    return AMC_OK;
}

int run(amc_ctx* ctx, const amc_pair_tri_problem* pb, const amc_pair_tri_opts* options, amc_pair_tri_result* result) {
    const char* fn = "amc_triangulate_pairs";
    const auto host_t0 = std::chrono::steady_clock::now();
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx || !pb || !result) return api_fail(AMC_E_INVALID, "%s: NULL argument", fn);
    amc_pair_tri_opts op;
    amc_pair_tri_opts_default(&op);
    if (options) op = *options;
    // (the test hook is read before anything can fail, once per call)
    const uint64_t batch = (uint64_t)env_int("AMC_INITPAIR_BATCH_CORRS", kDefaultBatchCorrs, 1, kDefaultBatchCorrs);
    const std::string bad = check_problem(*pb);
    if (!bad.empty()) return api_fail(AMC_E_INVALID, "%s: %s", fn, bad.c_str());
    const uint64_t n = pb->pair_offsets[pb->num_pairs];
    result->num_pairs = pb->num_pairs;
    result->num_corrs = n;
    result->accepted = (uint8_t*)std::calloc(std::max<uint64_t>(n, 1), 1);
    result->xyz = (double*)std::calloc(std::max<uint64_t>(n, 1) * 3, 8);
    result->tri_angle = (double*)std::calloc(std::max<uint64_t>(n, 1), 8);
    if (!result->accepted || !result->xyz || !result->tri_angle) {
        free_arrays(result);
        return api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    int rc = AMC_OK;
    try {
        if (n) {
            Plan plan;
            make_plan(*pb, &plan);
            rc = run_device(ctx, *pb, op, plan, batch, result);
        }
    } catch (const std::bad_alloc&) {
        rc = api_fail(AMC_E_NOMEM, "%s: out of host memory", fn);
    }
    if (rc != AMC_OK) {
        free_arrays(result);
        return rc;
    }
    for (uint64_t k = 0; k < n; ++k) result->num_accepted += result->accepted[k];
    result->host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count() - result->device_ms;
    return AMC_OK;
}

}  // namespace

extern "C" {

void amc_pair_tri_opts_default(amc_pair_tri_opts* o) {
    if (!o) return;
    o->min_tri_angle = 0.0174532925199432954743716805978692718781530857086181640625 * 16.0;  // DegToRad(init_min_tri_angle)
    o->reserved = 0.0;
}

int amc_triangulate_pairs(amc_ctx* ctx, const amc_pair_tri_problem* problem, const amc_pair_tri_opts* options,
                          amc_pair_tri_result* result) {
    return run(ctx, problem, options, result);
}

void amc_pair_tri_result_free(amc_pair_tri_result* r) {
    if (!r) return;
    free_arrays(r);
}

}  // extern "C"

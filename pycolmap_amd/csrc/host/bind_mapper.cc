// bind_mapper.cc — IncrementalMapper (mapper_host.h): which candidate to register next, the registration
// itself and the images of the local adjustment after it; and the initial pair, the global adjustment and the image
// filter (initial_pair_host.h).  The graph and the reconstruction are the triangulator's.  An image that
// is not registered is not in the reconstruction (R1), so the mapper keeps its candidates itself.  Every method
// takes a device first: without one it raises pycolmap_amd._capi.AmcError and changes nothing.  The `_with`
// variants put a callable in the library's place (test hooks: the CPU tests pass the references).
#include <map>

#include "abspose_host.h"
#include "initial_pair_host.h"
#include "mapper_host.h"
#include "py_scene.h"
#include "reconstruction.h"

namespace amchost {
namespace {

template <typename T>
using CArray = py::array_t<T, py::array::c_style | py::array::forcecast>;

struct PyMapper {
    py::object triangulator;
    MapperCandidates candidates;
    std::map<uint32_t, py::object> candidate_images;  // a copy of what add_candidate was given, for the reconstruction
    MapperTrials trials;
    size_t num_total_reg_images = 0;
    py::dict last;  // last_registration()
    // the registered images in COLMAP's reg_image_ids_ order, the images the model held when the mapper
    // was made (existing_image_ids_), the images filter_images removed (filtered_images_)
    std::vector<uint32_t> reg_image_ids;
    std::set<uint32_t> existing_image_ids, filtered_images;
    py::dict last_pair;  // last_initial_pair()
};

void checked_mapper_options(const MapperOptions& o) {
    const std::string bad = o.Check();
    if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
}

std::vector<uint32_t> find_next_images_with(PyMapper& mp, const MapperOptions& o, const py::object& solver) {
    const auto t0 = std::chrono::steady_clock::now();
    checked_mapper_options(o);
    if (solver.is_none()) CallLibrary(nullptr, "");
    PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    const SparseModel model = checked_model(t.reconstruction.cast<PyReconstruction&>());
    const ModelIndex ix(model, o.BogusThresholds());
    const FlatVisibility flat = PlanVisibility(graph, model, ix, mp.candidates);
    std::vector<uint32_t> ranked;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    uint64_t calls = 0;
    const size_t nc = flat.cand_ids.size();
    if (nc == 0) {
    } else if (!solver.is_none()) {
        py::dict d;
        d["image_point_offsets"] = NpArray(flat.image_point_offsets, 1);
        d["point2D_point3D"] = NpArray(flat.point2D_point3D, 1);
        d["cand_width"] = NpArray(flat.cand_width, 1);
        d["cand_height"] = NpArray(flat.cand_height, 1);
        d["cand_point_offsets"] = NpArray(flat.cand_point_offsets, 1);
        d["cand_xy"] = NpArray(flat.cand_xy, 2);
        d["corr_offsets"] = NpArray(flat.corr_offsets, 1);
        d["corr_image"] = NpArray(flat.corr_image, 1);
        d["corr_point2D"] = NpArray(flat.corr_point2D, 1);
        const py::dict out = solver(d);
        const auto nobs = CArray<uint32_t>::ensure(out["num_observations"]);
        const auto nvis = CArray<uint32_t>::ensure(out["num_visible_points3D"]);
        const auto score = CArray<uint64_t>::ensure(out["score"]);
        if (!nobs || !nvis || !score || static_cast<size_t>(nobs.size()) != nc || static_cast<size_t>(nvis.size()) != nc || static_cast<size_t>(score.size()) != nc)
            throw py::value_error("find_next_images: the solver's result does not have the problem's shape");
        ranked = RankNextImages(flat, nobs.data(), nvis.data(), score.data(), o, mp.trials, &mp.filtered_images);
    } else {
        const amc_visibility_problem pb = flat.Problem();
        ResultGuard<amc_visibility_result, amc_visibility_result_free> res;
        CallLibrary([&](amc_ctx* ctx) { return amc_image_visibility(ctx, &pb, res.get()); }, "amc_image_visibility");
        calls = 1;
        device_ms = res->device_ms;
        kernel_ms = res->kernel_ms;
        copy_ms = res->copy_ms;
        ranked = RankNextImages(flat, res->num_observations, res->num_visible_points3D, res->score, o, mp.trials, &mp.filtered_images);
    }
    py::dict st;
    st["call"] = "find_next_images";
    st["num_candidates"] = nc;
    st["num_ranked"] = ranked.size();
    st["num_correspondences"] = flat.corr_image.size();
    st["num_device_calls"] = calls;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return ranked;
}

bool register_next_image_with(PyMapper& mp, const MapperOptions& o, uint32_t image_id, const py::object& solver) {
    const auto t0 = std::chrono::steady_clock::now();
    checked_mapper_options(o);
    if (solver.is_none()) CallLibrary(nullptr, "");
    PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    const auto cand = mp.candidates.find(image_id);
    if (cand == mp.candidates.end() || r.images.contains(py::int_(image_id)))
        throw py::value_error(CheckMessage(__FILE__, __LINE__, "!image.IsRegistered() && IsCandidate(image_id)", "image_id=" + std::to_string(image_id)));
    const MapperCandidate& c = cand->second;
    SparseModel model = checked_model(r);
    ModelIndex ix(model, o.BogusThresholds());
    const auto cam = ix.camera.find(c.camera_id);
    if (cam == ix.camera.end()) throw py::value_error("register_next_image: candidate " + std::to_string(image_id) + " names a camera the reconstruction does not hold");
    const RegistrationPairs pairs = CollectRegistrationPairs(graph, model, ix, c);
    PyCamera& pycam = r.cameras[py::int_(c.camera_id)].cast<PyCamera&>();
    pycam.CheckParams();
    const RegistrationRule rule = PlanRegistration(model, model.cameras[cam->second], pycam.has_prior_focal_length, o);
    // everything that can refuse the call has: from here on the trial counts
    mp.trials[image_id] += 1;
    py::dict last;
    last["image_id"] = image_id;
    last["success"] = false;
    last["num_visible_points3D"] = pairs.num_visible;
    last["num_pairs"] = pairs.size();
    last["num_inliers"] = 0;
    last["focal_factor"] = 1.0;
    last["estimate_focal_length"] = rule.estimate_focal_length;
    last["would_refine_focal_length"] = rule.refine_focal_length;
    last["would_refine_extra_params"] = rule.refine_extra_params;
    double device_ms = 0, kernel_ms = 0;
    uint64_t calls = 0;
    bool ok = pairs.num_visible >= static_cast<size_t>(o.abs_pose_min_num_inliers) && pairs.size() >= static_cast<size_t>(o.abs_pose_min_num_inliers);
    if (ok) {
        amc_abspose_opts eo;
        amc_abspose_opts_default(&eo);
        eo.estimate_focal_length = rule.estimate_focal_length ? 1 : 0;
        eo.num_focal_length_samples = 30;
        eo.min_focal_length_ratio = o.min_focal_length_ratio;
        eo.max_focal_length_ratio = o.max_focal_length_ratio;
        eo.max_error = o.abs_pose_max_error;
        eo.min_inlier_ratio = o.abs_pose_min_inlier_ratio;
        eo.confidence = 0.99999;
        eo.dyn_num_trials_multiplier = 3.0;
        eo.min_num_trials = 100;
        eo.max_num_trials = 10000;
        amc_abspose_refine_opts ro;
        amc_abspose_refine_opts_default(&ro);  // AbsolutePoseRefinementOptions(); intrinsics are never refined (J5)
        const std::array<double, 12> prm = CameraParams12(pycam);
        const int32_t cmodel = pycam.model;
        const size_t n = pairs.size();
        bool success = false;
        size_t num_inliers = 0;
        double focal_factor = 1.0, q[4] = {0, 0, 0, 1}, tv[3] = {0, 0, 0};
        std::vector<uint8_t> mask(n, 0);
        std::vector<double> refined_params;  // the solver's camera, when it returns one: it replaces the scaling
        if (!solver.is_none()) {
            py::dict d, est;
            d["camera_model"] = cmodel;
            d["camera_params"] = NpArray(prm, 12);
            d["points2D"] = NpArray(pairs.points2D, 2);
            d["points3D"] = NpArray(pairs.points3D, 3);
            est["estimate_focal_length"] = rule.estimate_focal_length;
            est["num_focal_length_samples"] = eo.num_focal_length_samples;
            est["min_focal_length_ratio"] = eo.min_focal_length_ratio;
            est["max_focal_length_ratio"] = eo.max_focal_length_ratio;
            est["max_error"] = eo.max_error;
            est["min_inlier_ratio"] = eo.min_inlier_ratio;
            est["confidence"] = eo.confidence;
            est["dyn_num_trials_multiplier"] = eo.dyn_num_trials_multiplier;
            est["min_num_trials"] = eo.min_num_trials;
            est["max_num_trials"] = eo.max_num_trials;
            d["estimation"] = est;
            py::dict rfn;  // the rule's refinement flags, for a solver that refines the camera with the pose (25.6)
            rfn["refine_focal_length"] = rule.refine_focal_length;
            rfn["refine_extra_params"] = rule.refine_extra_params;
            d["refinement"] = rfn;
            const py::dict out = solver(d);
            const auto sq = CArray<double>::ensure(out["qvec"]);
            const auto stv = CArray<double>::ensure(out["tvec"]);
            const auto sm = CArray<uint8_t>::ensure(out["inlier_mask"]);
            if (!sq || !stv || !sm || sq.size() != 4 || stv.size() != 3 || static_cast<size_t>(sm.size()) != n)
                throw py::value_error("register_next_image: the solver's result does not have the problem's shape");
            success = out["success"].cast<bool>();
            num_inliers = out["num_inliers"].cast<size_t>();
            focal_factor = out["focal_factor"].cast<double>();
            std::copy(sq.data(), sq.data() + 4, q);
            std::copy(stv.data(), stv.data() + 3, tv);
            std::copy(sm.data(), sm.data() + n, mask.begin());
            if (out.contains("camera_params")) {
                const auto sp = CArray<double>::ensure(out["camera_params"]);
                if (!sp || sp.size() != 12)
                    throw py::value_error("register_next_image: the solver's camera_params are not 12 values");
                refined_params.assign(sp.data(), sp.data() + 12);
            }
        } else {
            const uint64_t off[2] = {0, n};
            ResultGuard<amc_abspose_result, amc_abspose_result_free> res;
            CallLibrary([&](amc_ctx* ctx) {
                return amc_estimate_absolute_poses(ctx, off, 1, &cmodel, prm.data(), pairs.points2D.data(), pairs.points3D.data(), &eo, &ro, 0, res.get());
            }, "amc_estimate_absolute_poses");
            calls = 1;
            device_ms = res->device_ms;
            kernel_ms = res->kernel_ms;
            success = res->success[0] != 0;
            num_inliers = res->num_inliers[0];
            focal_factor = res->focal_factor[0];
            std::copy(res->qvec, res->qvec + 4, q);
            std::copy(res->tvec, res->tvec + 3, tv);
            std::copy(res->inlier_mask, res->inlier_mask + n, mask.begin());
        }
        last["num_inliers"] = num_inliers;
        last["focal_factor"] = focal_factor;
        ok = success && num_inliers >= static_cast<size_t>(o.abs_pose_min_num_inliers);
        if (ok) {
            std::set<uint64_t> modified = t.modified;
            ApplyRegistration(c, pairs, mask.data(), q, tv, rule.estimate_focal_length && refined_params.empty(), focal_factor, &model, &ix,
                              &modified);
            if (!refined_params.empty()) {
                std::vector<double>& cp = model.cameras[cam->second].params;
                for (size_t k = 0; k < cp.size() && k < 12; ++k) cp[k] = refined_params[k];
            }
            r.images[py::int_(image_id)] = py::module_::import("copy").attr("copy")(mp.candidate_images.at(image_id));
            update_from_model(r, model);
            t.modified.swap(modified);
            mp.num_total_reg_images += 1;
            mp.reg_image_ids.push_back(image_id);
            mp.candidate_images.erase(image_id);
            mp.candidates.erase(cand);
        }
    }
    last["success"] = ok;
    mp.last = last;
    py::dict st;
    st["call"] = "register_next_image";
    st["num_pairs"] = pairs.size();
    st["num_device_calls"] = calls;
    FinishStats(st, t0, device_ms, kernel_ms, 0.0);
    return ok;
}

std::vector<uint32_t> find_local_bundle_with(PyMapper& mp, const MapperOptions& o, uint32_t image_id, const py::object& solver, uint64_t max_pair_points) {
    const auto t0 = std::chrono::steady_clock::now();
    checked_mapper_options(o);
    if (solver.is_none()) CallLibrary(nullptr, "");
    PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
    const SparseModel model = checked_model(t.reconstruction.cast<PyReconstruction&>());
    const ModelIndex ix(model, o.BogusThresholds());
    const FlatBundle flat = PlanLocalBundle(model, ix, o, image_id, max_pair_points);
    std::vector<uint32_t> bundle;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    uint64_t calls = 0;
    if (flat.NumPairs() == 0) {
        bundle = SelectLocalBundle(flat, o, nullptr);
    } else if (!solver.is_none()) {
        py::dict d;
        d["qvec"] = NpArray(flat.qvec, 4);
        d["tvec"] = NpArray(flat.tvec, 3);
        d["point_xyz"] = NpArray(flat.point_xyz, 3);
        d["pair_images"] = NpArray(flat.pair_images, 2);
        d["pair_offsets"] = NpArray(flat.pair_offsets, 1);
        d["shared_points"] = NpArray(flat.shared_points, 1);
        d["percentile"] = 75.0;
        const py::dict out = solver(d);
        const auto angle = CArray<double>::ensure(out["angle"]);
        if (!angle || static_cast<size_t>(angle.size()) != flat.NumPairs())
            throw py::value_error("find_local_bundle: the solver's result does not have the problem's shape");
        bundle = SelectLocalBundle(flat, o, angle.data());
    } else {
        const amc_pair_angle_problem pb = flat.Problem();
        amc_pair_angle_opts po;
        amc_pair_angle_opts_default(&po);
        ResultGuard<amc_pair_angle_result, amc_pair_angle_result_free> res;
        CallLibrary([&](amc_ctx* ctx) { return amc_shared_point_angles(ctx, &pb, &po, res.get()); }, "amc_shared_point_angles");
        calls = 1;
        device_ms = res->device_ms;
        kernel_ms = res->kernel_ms;
        copy_ms = res->copy_ms;
        bundle = SelectLocalBundle(flat, o, res->angle);
    }
    py::dict st;
    st["call"] = "find_local_bundle";
    st["num_overlapping_images"] = flat.overlapping.size();
    st["num_pairs"] = flat.NumPairs();
    st["num_shared_points"] = flat.shared_points.size();
    st["num_device_calls"] = calls;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return bundle;
}

// ---- the initial pair, the global adjustment and the image filter (initial_pair_host.h) ----
// Module-level functions that take the mapper first, as complete_tracks takes the triangulator: existing tests pin
// that the class has no such methods.
// reg_image_ids against a reconstruction that changed behind the mapper's back (K2): ids that left the model leave
// the list, model images the list lacks join it in ascending id
void sync_reg_image_ids(PyMapper& mp) {
    const PyReconstruction& r = mp.triangulator.cast<PyTriangulator&>().reconstruction.cast<const PyReconstruction&>();
    std::vector<uint32_t> kept, extra;
    std::set<uint32_t> seen;
    for (uint32_t id : mp.reg_image_ids)
        if (r.images.contains(py::int_(id)) && seen.insert(id).second) kept.push_back(id);
    for (auto item : r.images)
        if (!seen.count(item.first.cast<uint32_t>())) extra.push_back(item.first.cast<uint32_t>());
    std::sort(extra.begin(), extra.end());
    kept.insert(kept.end(), extra.begin(), extra.end());
    mp.reg_image_ids.swap(kept);
}

// RegisterInitialImagePair (21.1, 21.2).  two_view_solver: None, or a callable (camera1, points1, camera2, points2,
// matches, options) -> dict of the geometry after the pose step (pose_ok, config, inlier_matches (K, 2), qvec x y z w,
// tvec, tri_angle) in the place of estimate_calibrated_two_view_geometry and estimate_two_view_geometry_pose; pair_solver: None, or a callable that takes
// the flat problem of amc_triangulate_pairs as a dict of arrays and returns accepted, xyz and tri_angle.
bool register_initial_image_pair_with(PyMapper& mp, const MapperOptions& o, uint32_t id1, uint32_t id2, const py::object& two_view_solver,
                                      const py::object& pair_solver) {
    const auto t0 = std::chrono::steady_clock::now();
    checked_mapper_options(o);
    if (two_view_solver.is_none() || pair_solver.is_none()) CallLibrary(nullptr, "");
    PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    const auto cand1 = mp.candidates.find(id1), cand2 = mp.candidates.find(id2);
    if (id1 == id2 || cand1 == mp.candidates.end() || cand2 == mp.candidates.end() || r.images.contains(py::int_(id1)) || r.images.contains(py::int_(id2)))
        throw py::value_error(CheckMessage(__FILE__, __LINE__, "image_id1 != image_id2 && IsCandidate(image_id1) && IsCandidate(image_id2)",
                                           "image_id1=" + std::to_string(id1) + ", image_id2=" + std::to_string(id2)));
    const MapperCandidate& c1 = cand1->second;
    const MapperCandidate& c2 = cand2->second;
    SparseModel model = checked_model(r);
    ModelIndex ix(model, o.BogusThresholds());
    const auto cam1 = ix.camera.find(c1.camera_id), cam2 = ix.camera.find(c2.camera_id);
    if (cam1 == ix.camera.end() || cam2 == ix.camera.end()) throw py::value_error("register_initial_image_pair: a candidate names a camera the reconstruction does not hold");
    const py::object pycam1 = r.cameras[py::int_(c1.camera_id)], pycam2 = r.cameras[py::int_(c2.camera_id)];
    pycam1.cast<PyCamera&>().CheckParams();
    pycam2.cast<PyCamera&>().CheckParams();
    if (graph.NumPoints2D(id1) != c1.NumPoints2D() || graph.NumPoints2D(id2) != c2.NumPoints2D())
        throw py::value_error("register_initial_image_pair: a candidate's number of points2D differs from the graph's");
    const std::vector<uint32_t> matches = graph.FindCorrespondencesBetweenImages(id1, id2);
    const double identity_q[4] = {0, 0, 0, 1}, zero_t[3] = {0, 0, 0};
    FlatInitialPair flat = PlanInitialPair(model.cameras[cam1->second], model.cameras[cam2->second], c1, c2, matches, identity_q, zero_t);
    // EstimateInitialTwoViewGeometry
    TwoViewGeometryOptions tvo;
    tvo.ransac_options.min_num_trials = 30;
    tvo.ransac_options.max_error = o.init_max_error;
    const py::object pts1 = NpArray(c1.xy, 2), pts2 = NpArray(c2.xy, 2), marr = MatchesArray(matches);
    PyTwoViewGeometry G;
    bool pose_ok = false;
    if (two_view_solver.is_none()) {
        const py::module_ mod = py::module_::import("pycolmap_amd._pycolmap");
        const py::object geometry = mod.attr("estimate_calibrated_two_view_geometry")(pycam1, pts1, pycam2, pts2, marr, tvo);
        pose_ok = mod.attr("estimate_two_view_geometry_pose")(pycam1, pts1, pycam2, pts2, geometry).cast<bool>();
        G = geometry.cast<PyTwoViewGeometry>();
    } else {
        const py::dict out = two_view_solver(pycam1, pts1, pycam2, pts2, marr, tvo);
        const auto im = CArray<uint32_t>::ensure(out["inlier_matches"]);
        const auto sq = CArray<double>::ensure(out["qvec"]);
        const auto stv = CArray<double>::ensure(out["tvec"]);
        if (!im || !sq || !stv || im.size() % 2 != 0 || sq.size() != 4 || stv.size() != 3)
            throw py::value_error("register_initial_image_pair: the two-view solver's result does not have the expected shape");
        pose_ok = out["pose_ok"].cast<bool>();
        G.config = out["config"].cast<int>();
        G.inlier_matches.assign(im.data(), im.data() + im.size());
        std::copy(sq.data(), sq.data() + 4, G.cam2_from_cam1.rotation.xyzw.begin());
        std::copy(stv.data(), stv.data() + 3, G.cam2_from_cam1.translation.begin());
        G.tri_angle = out["tri_angle"].cast<double>();
    }
    // everything that can refuse the call has: from here on the trials count
    mp.trials[id1] += 1;
    mp.trials[id2] += 1;
    const size_t num_inliers = G.inlier_matches.size() / 2;
    const double tz = G.cam2_from_cam1.translation[2];
    bool ok = InitialPairAccepted(pose_ok, num_inliers, tz, G.tri_angle, o);
    py::dict last;
    last["image_id1"] = id1;
    last["image_id2"] = id2;
    last["success"] = false;
    last["num_correspondences"] = flat.NumCorrs();
    last["num_inliers"] = num_inliers;
    last["tri_angle"] = G.tri_angle;
    last["translation_z"] = tz;
    last["config"] = G.config;
    last["num_points3D"] = 0;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    uint64_t calls = 0;
    if (ok) {
        for (int k = 0; k < 4; ++k) flat.qvec[4 + k] = G.cam2_from_cam1.rotation.xyzw[k];
        for (int k = 0; k < 3; ++k) flat.tvec[3 + k] = G.cam2_from_cam1.translation[k];
        const size_t n = flat.NumCorrs();
        const double min_tri_angle = kMapperDegToRad * o.init_min_tri_angle;
        std::vector<uint8_t> accepted(n, 0);
        std::vector<double> xyz(3 * n, 0.0);
        if (!pair_solver.is_none()) {
            py::dict d = CamerasAndPosesDict(flat);
            d["pair_images"] = NpArray(flat.pair_images, 2);
            d["pair_offsets"] = NpArray(flat.pair_offsets, 1);
            d["corr_xy1"] = NpArray(flat.corr_xy1, 2);
            d["corr_xy2"] = NpArray(flat.corr_xy2, 2);
            d["min_tri_angle"] = min_tri_angle;
            const py::dict out = pair_solver(d);
            const auto sa = CArray<uint8_t>::ensure(out["accepted"]);
            const auto sx = CArray<double>::ensure(out["xyz"]);
            if (!sa || !sx || static_cast<size_t>(sa.size()) != n || static_cast<size_t>(sx.size()) != 3 * n)
                throw py::value_error("register_initial_image_pair: the solver's result does not have the problem's shape");
            std::copy(sa.data(), sa.data() + n, accepted.begin());
            std::copy(sx.data(), sx.data() + 3 * n, xyz.begin());
        } else {
            const amc_pair_tri_problem pb = flat.Problem();
            amc_pair_tri_opts po;
            amc_pair_tri_opts_default(&po);
            po.min_tri_angle = min_tri_angle;
            ResultGuard<amc_pair_tri_result, amc_pair_tri_result_free> res;
            CallLibrary([&](amc_ctx* ctx) { return amc_triangulate_pairs(ctx, &pb, &po, res.get()); }, "amc_triangulate_pairs");
            calls = 1;
            device_ms = res->device_ms;
            kernel_ms = res->kernel_ms;
            copy_ms = res->copy_ms;
            std::copy(res->accepted, res->accepted + n, accepted.begin());
            std::copy(res->xyz, res->xyz + 3 * n, xyz.begin());
        }
        const size_t created = ApplyInitialPair(c1, c2, flat, accepted.data(), xyz.data(), &model, &ix);
        const py::object copy = py::module_::import("copy").attr("copy");
        r.images[py::int_(id1)] = copy(mp.candidate_images.at(id1));
        r.images[py::int_(id2)] = copy(mp.candidate_images.at(id2));
        update_with_new_points(r, model);  // (the created points do not enter the triangulator's modified set, as in COLMAP)
        last["num_points3D"] = created;
        mp.num_total_reg_images += 2;
        mp.reg_image_ids.push_back(id1);
        mp.reg_image_ids.push_back(id2);
        mp.candidate_images.erase(id1);
        mp.candidate_images.erase(id2);
        mp.candidates.erase(id1);
        mp.candidates.erase(id2);
    }
    last["success"] = ok;
    mp.last_pair = last;
    py::dict st;
    st["call"] = "register_initial_image_pair";
    st["num_correspondences"] = flat.NumCorrs();
    st["num_device_calls"] = calls;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return ok;
}

// AdjustGlobalBundle with Reconstruction::Normalize (21.3).  solver: None, or BundleAdjuster._solve_with's callable.
bool adjust_global_bundle_with(PyMapper& mp, const MapperOptions& o, const BundleAdjustmentOptions& ba_options, const py::object& solver) {
    checked_mapper_options(o);
    sync_reg_image_ids(mp);
    if (mp.reg_image_ids.size() < 2) throw py::value_error(CheckMessage(__FILE__, __LINE__, "reg_image_ids.size() >= 2", "adjust_global_bundle"));
    if (solver.is_none()) CallLibrary(nullptr, "");
    PyReconstruction& r = mp.triangulator.cast<PyTriangulator&>().reconstruction.cast<PyReconstruction&>();
    {
        SparseModel m = checked_model(r);  // "avoid degeneracies in bundle adjustment"
        FilterObservationsWithNegativeDepth(&m);
        update_from_model(r, m);
    }
    PyBundleAdjuster adjuster{ba_options, GlobalBundleConfig(mp.reg_image_ids, mp.existing_image_ids, o.fix_existing_images), py::dict()};
    if (!adjuster_solve(adjuster, r, solver)) return false;
    const py::object stats = py::module_::import("pycolmap_amd._pycolmap").attr("_last_stats");
    SparseModel m = checked_model(r);
    const NormalizeResult nr = NormalizeModel(&m, mp.reg_image_ids);
    update_from_model(r, m);
    py::dict st(stats.attr("copy")());
    st["call"] = "adjust_global_bundle";
    st["normalize_scale"] = nr.scale;
    SetLastStats(st);
    return true;
}

// FilterImages (21.4): host code, no device
size_t filter_images(PyMapper& mp, const MapperOptions& o) {
    checked_mapper_options(o);
    sync_reg_image_ids(mp);
    PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    SparseModel m = checked_model(r);
    const std::vector<uint32_t> gone = PlanFilterImages(m, mp.reg_image_ids, o);
    if (gone.empty()) return 0;
    for (uint32_t id : gone) DeRegisterImage(&m, id);
    const py::object copy = py::module_::import("copy").attr("copy");
    for (uint32_t id : gone) {
        // the image becomes a candidate again, none of its points2D carrying a point3D
        py::object image = copy(r.images[py::int_(id)]);
        PyImage& im = image.cast<PyImage&>();
        MapperCandidate c;
        c.image_id = id;
        c.camera_id = im.camera_id;
        for (PyPoint2D& p : im.points2D) {
            p.point3D_id = kInvalidPoint3DId;
            c.xy.push_back(p.xy[0]);
            c.xy.push_back(p.xy[1]);
        }
        mp.candidate_images[id] = image;
        mp.candidates[id] = std::move(c);
        mp.filtered_images.insert(id);
        r.images.attr("pop")(py::int_(id));
    }
    update_from_model(r, m);
    std::set<uint64_t> modified;  // points that left the model leave the triangulator's modified set
    for (uint64_t pid : t.modified)
        if (r.points3D.contains(py::int_(pid))) modified.insert(pid);
    t.modified.swap(modified);
    sync_reg_image_ids(mp);
    return gone.size();
}

}  // namespace

void BindMapper(py::module_& m) {
    py::enum_<ImageSelectionMethod> PySelection(m, "ImageSelectionMethod");
    PySelection.value("MAX_VISIBLE_POINTS_NUM", ImageSelectionMethod::MAX_VISIBLE_POINTS_NUM)
        .value("MAX_VISIBLE_POINTS_RATIO", ImageSelectionMethod::MAX_VISIBLE_POINTS_RATIO)
        .value("MIN_UNCERTAINTY", ImageSelectionMethod::MIN_UNCERTAINTY);
    PySelection.def(py::init([](const std::string& s) {
        if (s == "MAX_VISIBLE_POINTS_NUM") return ImageSelectionMethod::MAX_VISIBLE_POINTS_NUM;
        if (s == "MAX_VISIBLE_POINTS_RATIO") return ImageSelectionMethod::MAX_VISIBLE_POINTS_RATIO;
        if (s == "MIN_UNCERTAINTY") return ImageSelectionMethod::MIN_UNCERTAINTY;
        throw py::value_error("Invalid string value " + s + " for enum ImageSelectionMethod");
    }));
    py::implicitly_convertible<std::string, ImageSelectionMethod>();
    py::class_<MapperOptions> PyMapOpts(m, "IncrementalMapperOptions");
    PyMapOpts.def(py::init<>())
        .def_readwrite("init_min_num_inliers", &MapperOptions::init_min_num_inliers, "Minimum number of inliers for initial image pair.")
        .def_readwrite("init_max_error", &MapperOptions::init_max_error, "Maximum error in pixels for two-view geometry estimation for initial image pair.")
        .def_readwrite("init_max_forward_motion", &MapperOptions::init_max_forward_motion, "Maximum forward motion for initial image pair.")
        .def_readwrite("init_min_tri_angle", &MapperOptions::init_min_tri_angle, "Minimum triangulation angle for initial image pair.")
        .def_readwrite("init_max_reg_trials", &MapperOptions::init_max_reg_trials, "Maximum number of trials to use an image for initialization.")
        .def_readwrite("abs_pose_max_error", &MapperOptions::abs_pose_max_error, "Maximum reprojection error in absolute pose estimation.")
        .def_readwrite("abs_pose_min_num_inliers", &MapperOptions::abs_pose_min_num_inliers, "Minimum number of inliers in absolute pose estimation.")
        .def_readwrite("abs_pose_min_inlier_ratio", &MapperOptions::abs_pose_min_inlier_ratio, "Minimum inlier ratio in absolute pose estimation.")
        .def_readwrite("abs_pose_refine_focal_length", &MapperOptions::abs_pose_refine_focal_length, "Whether to estimate the focal length in absolute pose estimation.")
        .def_readwrite("abs_pose_refine_extra_params", &MapperOptions::abs_pose_refine_extra_params, "Whether to estimate the extra parameters in absolute pose estimation.")
        .def_readwrite("local_ba_num_images", &MapperOptions::local_ba_num_images, "Number of images to optimize in local bundle adjustment.")
        .def_readwrite("local_ba_min_tri_angle", &MapperOptions::local_ba_min_tri_angle, "Minimum triangulation for images to be chosen in local bundle adjustment.")
        .def_readwrite("min_focal_length_ratio", &MapperOptions::min_focal_length_ratio, "The threshold used to filter and ignore images with degenerate intrinsics.")
        .def_readwrite("max_focal_length_ratio", &MapperOptions::max_focal_length_ratio, "The threshold used to filter and ignore images with degenerate intrinsics.")
        .def_readwrite("max_extra_param", &MapperOptions::max_extra_param, "The threshold used to filter and ignore images with degenerate intrinsics.")
        .def_readwrite("filter_max_reproj_error", &MapperOptions::filter_max_reproj_error, "Maximum reprojection error in pixels for observations.")
        .def_readwrite("filter_min_tri_angle", &MapperOptions::filter_min_tri_angle, "Minimum triangulation angle in degrees for stable 3D points.")
        .def_readwrite("max_reg_trials", &MapperOptions::max_reg_trials, "Maximum number of trials to register an image.")
        .def_readwrite("fix_existing_images", &MapperOptions::fix_existing_images, "If reconstruction is provided as input, fix the existing image poses.")
        .def_readwrite("num_threads", &MapperOptions::num_threads, "Number of threads.")
        .def_readwrite("image_selection_method", &MapperOptions::image_selection_method, "Method to find and select next best image to register.");
    MakeDataclass(PyMapOpts, {"init_min_num_inliers", "init_max_error", "init_max_forward_motion", "init_min_tri_angle", "init_max_reg_trials",
                              "abs_pose_max_error", "abs_pose_min_num_inliers", "abs_pose_min_inlier_ratio", "abs_pose_refine_focal_length",
                              "abs_pose_refine_extra_params", "local_ba_num_images", "local_ba_min_tri_angle", "min_focal_length_ratio",
                              "max_focal_length_ratio", "max_extra_param", "filter_max_reproj_error", "filter_min_tri_angle", "max_reg_trials",
                              "fix_existing_images", "num_threads", "image_selection_method"});

    py::class_<PyMapper>(m, "IncrementalMapper")
        .def(py::init([](const py::object& triangulator) {
                 if (!py::isinstance<PyTriangulator>(triangulator)) throw py::type_error("IncrementalMapper(triangulator: IncrementalTriangulator)");
                 PyMapper mp;
                 mp.triangulator = triangulator;
                 // BeginReconstruction: every image the model holds already counts as registered
                 const PyReconstruction& r = triangulator.cast<PyTriangulator&>().reconstruction.cast<PyReconstruction&>();
                 mp.num_total_reg_images = r.images.size();
                 for (auto item : r.images) mp.existing_image_ids.insert(item.first.cast<uint32_t>());
                 mp.reg_image_ids.assign(mp.existing_image_ids.begin(), mp.existing_image_ids.end());
                 return mp;
             }), "triangulator"_a)
        .def("add_candidate", [](PyMapper& mp, const py::object& image) {
                 const PyImage& im = image.cast<const PyImage&>();
                 PyTriangulator& t = mp.triangulator.cast<PyTriangulator&>();
                 const PyReconstruction& r = t.reconstruction.cast<const PyReconstruction&>();
                 const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
                 if (im.image_id == 0xFFFFFFFFu) throw py::value_error("add_candidate: the image has no image_id");
                 if (r.images.contains(py::int_(im.image_id))) throw py::value_error("add_candidate: image " + std::to_string(im.image_id) + " is in the reconstruction");
                 if (mp.candidates.count(im.image_id)) throw py::value_error("add_candidate: image " + std::to_string(im.image_id) + " is a candidate already");
                 if (!r.cameras.contains(py::int_(im.camera_id))) throw py::value_error("add_candidate: the reconstruction has no camera " + std::to_string(im.camera_id));
                 if (graph.NumPoints2D(im.image_id) != im.points2D.size())  // an image the graph does not hold: the graph's ValueError
                     throw py::value_error("add_candidate: image " + std::to_string(im.image_id) + " has " + std::to_string(im.points2D.size()) +
                                           " points2D, the graph gives it " + std::to_string(graph.NumPoints2D(im.image_id)));
                 MapperCandidate c;
                 c.image_id = im.image_id;
                 c.camera_id = im.camera_id;
                 for (const PyPoint2D& p : im.points2D) {
                     if (p.point3D_id != kInvalidPoint3DId) throw py::value_error("add_candidate: a point2D of image " + std::to_string(im.image_id) + " carries a point3D");
                     c.xy.push_back(p.xy[0]);
                     c.xy.push_back(p.xy[1]);
                 }
                 mp.candidate_images[im.image_id] = py::module_::import("copy").attr("copy")(image);
                 mp.candidates[im.image_id] = std::move(c);
             }, "image"_a, "An image that may be registered: an Image with points2D, none carrying a point3D, whose camera the reconstruction holds and whose id the graph knows.")
        .def_property_readonly("candidates", [](const PyMapper& mp) {
                 std::vector<uint32_t> ids;
                 for (const auto& kv : mp.candidates) ids.push_back(kv.first);
                 return ids;
             }, "The ids of the candidates, ascending.")
        .def("num_reg_trials", [](const PyMapper& mp, uint32_t image_id) {
                 const auto it = mp.trials.find(image_id);
                 return it == mp.trials.end() ? 0 : it->second;
             }, "image_id"_a)
        .def("num_total_reg_images", [](const PyMapper& mp) { return mp.num_total_reg_images; })
        .def("last_registration", [](const PyMapper& mp) { return py::dict(mp.last.attr("copy")()); },
             "What the last register_next_image call saw: image_id, success, num_visible_points3D, num_pairs, num_inliers, focal_factor,\n"
             "estimate_focal_length, and the two refinement flags COLMAP would have set (the refinement here never refines intrinsics).")
        .def("find_next_images", [](PyMapper& mp, const MapperOptions& o) { return find_next_images_with(mp, o, py::none()); }, "options"_a,
             "The candidates worth trying next, best first: never-tried ones before the others, each group by descending rank\n"
             "(visible points, their ratio or the visibility pyramid score), on the GPU (DESIGN.md section 20).")
        .def("_find_next_images_with", &find_next_images_with, "options"_a, "solver"_a, "find_next_images with a callable in the library's place (test hook).")
        .def("register_next_image", [](PyMapper& mp, const MapperOptions& o, uint32_t image_id) {
                 return register_next_image_with(mp, o, image_id, py::none());
             }, "options"_a, "image_id"_a,
             "Estimate the pose of a candidate from its 2D-3D correspondences on the GPU, add it to the reconstruction and\n"
             "continue the tracks of its inliers (DESIGN.md section 20).  False changes nothing but the trial count.")
        .def("_register_next_image_with", &register_next_image_with, "options"_a, "image_id"_a, "solver"_a,
             "register_next_image with a callable in the library's place (test hook).")
        .def("find_local_bundle", [](PyMapper& mp, const MapperOptions& o, uint32_t image_id) {
                 return find_local_bundle_with(mp, o, image_id, py::none(), AMC_MAPPER_MAX_PAIR_POINTS);
             }, "options"_a, "image_id"_a,
             "The images of the local bundle adjustment around a model image: its most overlapping images with a sufficient\n"
             "75th-percentile triangulation angle, on the GPU (DESIGN.md section 20).  The image itself is not in the list.")
        .def("_find_local_bundle_with", &find_local_bundle_with, "options"_a, "image_id"_a, "solver"_a,
             "max_pair_points"_a = static_cast<uint64_t>(AMC_MAPPER_MAX_PAIR_POINTS), "find_local_bundle with a callable in the library's place (test hook).")
        .def_property_readonly("triangulator", [](const PyMapper& mp) { return mp.triangulator; })
        .def_property_readonly("reconstruction", [](const PyMapper& mp) { return mp.triangulator.cast<PyTriangulator&>().reconstruction; })
        .def_property_readonly("correspondence_graph", [](const PyMapper& mp) { return mp.triangulator.cast<PyTriangulator&>().graph; })
        .def("__copy__", [](const PyMapper& mp) {
                 PyMapper c(mp);
                 c.last = py::dict(mp.last.attr("copy")());
                 c.last_pair = py::dict(mp.last_pair.attr("copy")());
                 return c;
             })
        .def("__deepcopy__", [](const PyMapper& mp, const py::dict& memo) {
                 const py::object deepcopy = py::module_::import("copy").attr("deepcopy");
                 PyMapper c(mp);
                 c.triangulator = deepcopy(mp.triangulator, memo);
                 for (auto& kv : c.candidate_images) kv.second = deepcopy(kv.second, memo);
                 c.last = py::dict(mp.last.attr("copy")());
                 c.last_pair = py::dict(mp.last_pair.attr("copy")());
                 return c;
             })
        .def("last_initial_pair", [](const PyMapper& mp) { return py::dict(mp.last_pair.attr("copy")()); },
             "What the last register_initial_image_pair call saw: image_id1, image_id2, success, num_correspondences, num_inliers,\n"
             "tri_angle, translation_z, config and num_points3D (DESIGN.md section 21); empty before the first call.")
        .def_property_readonly("reg_image_ids", [](PyMapper& mp) {
                 sync_reg_image_ids(mp);
                 return mp.reg_image_ids;
             }, "The registered images in COLMAP's order: those the model held when the mapper was made, ascending, then every\n"
                "registered image in registration order (DESIGN.md section 21).")
        .def_property_readonly("filtered_images", [](const PyMapper& mp) { return std::vector<uint32_t>(mp.filtered_images.begin(), mp.filtered_images.end()); },
             "The ids of the images filter_images removed from the model, ascending.")
        .def("__repr__", [](const PyMapper& mp) {
            const PyReconstruction& r = mp.triangulator.cast<PyTriangulator&>().reconstruction.cast<const PyReconstruction&>();
            return "IncrementalMapper(num_reg_images=" + std::to_string(r.images.size()) + ", num_candidates=" + std::to_string(mp.candidates.size()) +
                   ", num_total_reg_images=" + std::to_string(mp.num_total_reg_images) + ")";
        });

    m.def("register_initial_image_pair", [](PyMapper& mp, const MapperOptions& o, uint32_t image_id1, uint32_t image_id2) {
              return register_initial_image_pair_with(mp, o, image_id1, image_id2, py::none(), py::none());
          }, "mapper"_a, "options"_a, "image_id1"_a, "image_id2"_a,
          "Start a model from two candidates of the mapper: estimate their calibrated two-view geometry and relative pose on\n"
          "the GPU, put image 1 at the identity and image 2 at cam2_from_cam1, and triangulate every correspondence the graph\n"
          "holds between them in one device call (DESIGN.md section 21).  False changes nothing but the two trial counts.");
    m.def("_register_initial_image_pair_with", &register_initial_image_pair_with, "mapper"_a, "options"_a, "image_id1"_a, "image_id2"_a,
          "two_view_solver"_a, "pair_solver"_a, "register_initial_image_pair with callables in the library's place (test hook; DESIGN.md section 21).");
    m.def("adjust_global_bundle", [](PyMapper& mp, const MapperOptions& o, const BundleAdjustmentOptions& ba_options) {
              return adjust_global_bundle_with(mp, o, ba_options, py::none());
          }, "mapper"_a, "options"_a, "ba_options"_a,
          "Adjust every registered image and the points they see on the GPU, the first image's pose and the second's x position\n"
          "held, after deleting the observations with negative depth; then normalise the scene to an extent of 10\n"
          "(DESIGN.md section 21).  False when the model gives no residual.");
    m.def("_adjust_global_bundle_with", &adjust_global_bundle_with, "mapper"_a, "options"_a, "ba_options"_a, "solver"_a,
          "adjust_global_bundle with a callable in the library's place (test hook; DESIGN.md section 21).");
    m.def("filter_images", &filter_images, "mapper"_a, "options"_a,
          "From 20 registered images on, remove every registered image that sees no point3D or whose camera has bogus\n"
          "parameters: it leaves the reconstruction with its observations and becomes a candidate again (DESIGN.md section 21).\n"
          "Returns the number of images removed.  Host code: it needs no GPU.");
    m.def("_normalize_model", [](PyReconstruction& r, const std::vector<uint32_t>& reg_image_ids, double extent, double p0, double p1) {
              SparseModel model = checked_model(r);
              const NormalizeResult nr = NormalizeModel(&model, reg_image_ids, extent, p0, p1);
              update_from_model(r, model);
              return py::make_tuple(nr.applied, nr.scale, std::array<double, 3>{{nr.centroid[0], nr.centroid[1], nr.centroid[2]}});
          }, "reconstruction"_a, "reg_image_ids"_a, "extent"_a = 10.0, "p0"_a = 0.1, "p1"_a = 0.9,
          "adjust_global_bundle's normalisation on its own: (applied, scale, centroid) (test hook; DESIGN.md section 21).");
}

}  // namespace amchost

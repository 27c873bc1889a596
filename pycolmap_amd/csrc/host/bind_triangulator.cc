// bind_triangulator.cc — CorrespondenceGraph and IncrementalTriangulator (the reference's
// pycolmap/scene/correspondence_graph.h and pycolmap/sfm/incremental_triangulator.h; correspondence_graph.h,
// triangulator_host.h), complete_tracks and merge_tracks (track_ops_host.h) and
// retriangulate (retriangulate_host.h).
#include "correspondence_graph.h"
#include "py_scene.h"
#include "retriangulate_host.h"
#include "track_ops_host.h"
#include "triangulator_host.h"

namespace amchost {
namespace {

template <typename T>
using CArray = py::array_t<T, py::array::c_style | py::array::forcecast>;

void CheckTriangulatorOptions(const TriangulatorOptions& o) {
    const std::string bad = o.Check();
    if (!bad.empty()) throw py::value_error(CheckMessage(__FILE__, __LINE__, bad));
}

// TriangulateImage: one amc_triangulate_observations call per run of points2D.  Nothing of
// the reconstruction or of the modified set changes unless every call succeeds.  Without a device the call raises
// pycolmap_amd._capi.AmcError.
// solver: None, or a callable that stands in for the library (a test hook: the CPU tests pass the reference): it
// takes the flat problem as a dict of arrays and returns continued, cand_round, round_offsets and round_xyz.
size_t triangulate_image_with(PyTriangulator& t, const TriangulatorOptions& o, uint32_t image_id, const py::object& solver) {
    const auto t0 = std::chrono::steady_clock::now();
    CheckTriangulatorOptions(o);
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    SparseModel model = checked_model(r);
    ModelIndex ix(model, o);
    const auto self = ix.image.find(image_id);
    if (self == ix.image.end()) throw py::value_error(CheckMessage(__FILE__, __LINE__, "reconstruction.exists_image(image_id)", "image_id=" + std::to_string(image_id)));
    (void)graph.NumPoints2D(image_id);  // an image the graph does not hold: the graph's ValueError
    std::set<uint64_t> modified = t.modified;
    TriobsApplied total;
    uint64_t items = 0, observations = 0, calls = 0;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    auto apply = [&](const int32_t* continued, const uint32_t* cand_round, const uint64_t* round_offsets, const double* round_xyz, const FlatTriobs& flat) {
        const TriobsApplied a = ApplyTriobsResult(flat, continued, cand_round, round_offsets, round_xyz, &model, &ix, &modified);
        total.num_tris += a.num_tris;
        total.num_created += a.num_created;
        total.num_continued += a.num_continued;
    };
    if (!ix.image_bogus[self->second]) {
        FlatTriobs flat = FlattenModelForTriobs(model, ix);
        amc_triobs_opts opts;
        amc_triobs_opts_default(&opts);
        opts.create_max_angle_error = o.create_max_angle_error;
        opts.continue_max_angle_error = o.continue_max_angle_error;
        opts.min_angle = o.min_angle;
        const size_t npoints2D = model.images[self->second].points2D.size();
        for (size_t begin = 0; begin < npoints2D;) {
            begin = PlanTriangulationRun(graph, model, ix, o, image_id, begin, &flat);
            if (flat.NumItems() == 0) continue;
            if (!solver.is_none()) {
                py::dict d = CamerasAndPosesDict(flat);
                d["item_offsets"] = NpArray(flat.item_offsets, 1);
                d["cand_image"] = NpArray(flat.cand_image, 1);
                d["cand_xy"] = NpArray(flat.cand_xy, 2);
                d["cand_has_point"] = NpArray(flat.cand_has_point, 1);
                d["cand_xyz"] = NpArray(flat.cand_xyz, 3);
                d["no_create_two_view"] = NpArray(flat.no_create_two_view, 1);
                d["create_max_angle_error"] = o.create_max_angle_error;
                d["continue_max_angle_error"] = o.continue_max_angle_error;
                d["min_angle"] = o.min_angle;
                const py::dict out = solver(d);
                const auto cont = CArray<int32_t>::ensure(out["continued"]);
                const auto rnd = CArray<uint32_t>::ensure(out["cand_round"]);
                const auto roff = CArray<uint64_t>::ensure(out["round_offsets"]);
                const auto rxyz = CArray<double>::ensure(out["round_xyz"]);
                if (!cont || !rnd || !roff || !rxyz || static_cast<size_t>(cont.size()) != flat.NumItems() ||
                    static_cast<size_t>(rnd.size()) != flat.cand_image.size() || static_cast<size_t>(roff.size()) != flat.NumItems() + 1 ||
                    static_cast<uint64_t>(rxyz.size()) != 3 * roff.data()[flat.NumItems()])
                    throw py::value_error("triangulate_image: the solver's result does not have the problem's shape");
                items += flat.NumItems();
                observations += flat.cand_image.size();
                calls += 1;
                apply(cont.data(), rnd.data(), roff.data(), rxyz.data(), flat);
                continue;
            }
            const amc_triobs_problem pb = flat.Problem();
            ResultGuard<amc_triobs_result, amc_triobs_result_free> res;
            CallLibrary([&](amc_ctx* ctx) { return amc_triangulate_observations(ctx, &pb, &opts, res.get()); }, "amc_triangulate_observations");
            items += res->num_items;
            observations += res->num_candidates;
            calls += 1;
            device_ms += res->device_ms;
            kernel_ms += res->kernel_ms;
            copy_ms += res->copy_ms;
            apply(res->continued, res->cand_round, res->round_offsets, res->round_xyz, flat);
        }
    }
    update_with_new_points(r, model);
    t.modified.swap(modified);
    py::dict st;
    st["call"] = "triangulate_image";
    st["num_items"] = items;
    st["num_observations"] = observations;
    st["num_created_points"] = total.num_created;
    st["num_continued_observations"] = total.num_continued;
    st["num_device_calls"] = calls;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return total.num_tris;
}

// 18.0: the listed ids as a set, which is processed in ascending order; None = every point of the model
std::set<uint64_t> listed_point3D_ids(const SparseModel& model, const py::object& ids) {
    std::set<uint64_t> listed;
    if (ids.is_none()) {
        for (const ModelPoint3D& p : model.points3D) listed.insert(p.point3D_id);
        return listed;
    }
    for (const py::handle& id : py::iter(ids)) {
        try {
            listed.insert(id.cast<uint64_t>());
        } catch (const py::cast_error&) {
            throw py::type_error("point3D_ids: expected an iterable of non-negative ints");
        }
    }
    return listed;
}

// ---- complete_tracks, complete_all_tracks (track_ops_host.h) ----
// IncrementalTriangulator::CompleteTracks / CompleteAllTracks as module-level functions with the triangulator first:
// tests pin that the class has no such methods.  One amc_complete_tracks call on the superset closures (18.3), then
// the sequential walk on the host.  Nothing of the reconstruction or of the modified set changes unless everything
// succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
// ids: None = every point of the reconstruction.  solver: None, or a callable that stands in for the library (a test
// hook): it takes the flat problem as a dict of arrays and returns a dict with cand_pass.
size_t complete_tracks_with(PyTriangulator& t, const TriangulatorOptions& o, const py::object& ids, const py::object& solver) {
    const auto t0 = std::chrono::steady_clock::now();
    CheckTriangulatorOptions(o);
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    SparseModel model = checked_model(r);
    const ModelIndex ix(model, o);
    const std::set<uint64_t> listed = listed_point3D_ids(model, ids);
    const FlatComplete flat = PlanCompletion(graph, model, ix, o, listed);
    std::set<uint64_t> modified = t.modified;
    CompletionApplied applied;
    uint64_t calls = 0;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    if (flat.NumItems() != 0 && !solver.is_none()) {
        py::dict d = CamerasAndPosesDict(flat);
        d["item_xyz"] = NpArray(flat.item_xyz, 3);
        d["item_offsets"] = NpArray(flat.item_offsets, 1);
        d["cand_image"] = NpArray(flat.cand_image, 1);
        d["cand_xy"] = NpArray(flat.cand_xy, 2);
        d["complete_max_reproj_error"] = o.complete_max_reproj_error;
        const py::dict out = solver(d);
        const auto pass = CArray<uint8_t>::ensure(out["cand_pass"]);
        if (!pass || static_cast<size_t>(pass.size()) != flat.NumCandidates())
            throw py::value_error("complete_tracks: the solver's result does not have the problem's shape");
        calls = 1;
        applied = ApplyCompletion(flat, pass.data(), graph, o, &model, ix, &modified);
    } else if (flat.NumItems() != 0) {
        amc_complete_opts opts;
        amc_complete_opts_default(&opts);
        opts.complete_max_reproj_error = o.complete_max_reproj_error;
        const amc_complete_problem pb = flat.Problem();
        ResultGuard<amc_complete_result, amc_complete_result_free> res;
        CallLibrary([&](amc_ctx* ctx) { return amc_complete_tracks(ctx, &pb, &opts, res.get()); }, "amc_complete_tracks");
        calls = 1;
        device_ms = res->device_ms;
        kernel_ms = res->kernel_ms;
        copy_ms = res->copy_ms;
        applied = ApplyCompletion(flat, res->cand_pass, graph, o, &model, ix, &modified);
    }
    if (applied.num_completed != 0) update_with_errors(r, model);
    t.modified.swap(modified);
    py::dict st;
    st["call"] = ids.is_none() ? "complete_all_tracks" : "complete_tracks";
    st["num_items"] = flat.NumItems();
    st["num_candidates_tested"] = flat.NumCandidates();
    st["num_candidates_visited"] = applied.num_visited;
    st["num_completed_observations"] = applied.num_completed;
    st["num_device_calls"] = solver.is_none() ? calls : 0;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return applied.num_completed;
}

// ---- merge_tracks, merge_all_tracks (track_ops_host.h) ----
// One amc_merge_tracks call on the connected components of the listed points, then the merge logs applied root by
// root in ascending id order.  The solver stands in for the library as above and returns root_return,
// root_merge_offsets, merge_current, merge_other and merge_xyz.
size_t merge_tracks_with(PyTriangulator& t, const TriangulatorOptions& o, const py::object& ids, const py::object& solver) {
    const auto t0 = std::chrono::steady_clock::now();
    CheckTriangulatorOptions(o);
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    SparseModel model = checked_model(r);
    const ModelIndex ix(model, o);
    const std::set<uint64_t> listed = listed_point3D_ids(model, ids);
    const FlatMerge flat = PlanMerge(graph, model, ix, listed);
    std::set<uint64_t> modified = t.modified;
    MergeApplied applied;
    uint64_t calls = 0, pairs_tried = 0;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    if (flat.NumComponents() != 0 && !solver.is_none()) {
        py::dict d = CamerasAndPosesDict(flat);
        d["comp_point_offsets"] = NpArray(flat.comp_point_offsets, 1);
        d["comp_root_offsets"] = NpArray(flat.comp_root_offsets, 1);
        d["roots"] = NpArray(flat.roots, 1);
        d["point_xyz"] = NpArray(flat.point_xyz, 3);
        d["point_obs_offsets"] = NpArray(flat.point_obs_offsets, 1);
        d["obs_image"] = NpArray(flat.obs_image, 1);
        d["obs_xy"] = NpArray(flat.obs_xy, 2);
        d["obs_corr_offsets"] = NpArray(flat.obs_corr_offsets, 1);
        d["corr_obs"] = NpArray(flat.corr_obs, 1);
        d["merge_max_reproj_error"] = o.merge_max_reproj_error;
        const py::dict out = solver(d);
        const auto ret = CArray<uint32_t>::ensure(out["root_return"]);
        const auto moff = CArray<uint64_t>::ensure(out["root_merge_offsets"]);
        const auto cur = CArray<uint32_t>::ensure(out["merge_current"]);
        const auto oth = CArray<uint32_t>::ensure(out["merge_other"]);
        const auto mxyz = CArray<double>::ensure(out["merge_xyz"]);
        const size_t nroots = flat.roots.size();
        bool fits = ret && moff && cur && oth && mxyz && static_cast<size_t>(ret.size()) == nroots && static_cast<size_t>(moff.size()) == nroots + 1;
        if (fits) {
            for (size_t k = 0; k < nroots; ++k) fits = fits && moff.data()[k] <= moff.data()[k + 1];
            const uint64_t nm = moff.data()[nroots];
            fits = fits && moff.data()[0] == 0 && static_cast<uint64_t>(cur.size()) == nm && static_cast<uint64_t>(oth.size()) == nm &&
                   static_cast<uint64_t>(mxyz.size()) == 3 * nm;
        }
        if (!fits) throw py::value_error("merge_tracks: the solver's result does not have the problem's shape");
        calls = 1;
        applied = ApplyMergeResult(flat, ret.data(), moff.data(), cur.data(), oth.data(), mxyz.data(), &model, &modified);
    } else if (flat.NumComponents() != 0) {
        amc_merge_opts opts;
        amc_merge_opts_default(&opts);
        opts.merge_max_reproj_error = o.merge_max_reproj_error;
        const amc_merge_problem pb = flat.Problem();
        ResultGuard<amc_merge_result, amc_merge_result_free> res;
        CallLibrary([&](amc_ctx* ctx) { return amc_merge_tracks(ctx, &pb, &opts, res.get()); }, "amc_merge_tracks");
        calls = 1;
        pairs_tried = res->num_pairs_tried;
        device_ms = res->device_ms;
        kernel_ms = res->kernel_ms;
        copy_ms = res->copy_ms;
        applied = ApplyMergeResult(flat, res->root_return, res->root_merge_offsets, res->merge_current, res->merge_other, res->merge_xyz, &model, &modified);
    }
    if (applied.num_merges != 0) update_with_new_points(r, model);
    t.modified.swap(modified);
    py::dict st;
    st["call"] = ids.is_none() ? "merge_all_tracks" : "merge_tracks";
    st["num_components"] = flat.NumComponents();
    st["largest_component"] = flat.largest_component;
    st["num_pairs_tried"] = pairs_tried;
    st["num_merges"] = applied.num_merges;
    st["num_device_calls"] = solver.is_none() ? calls : 0;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return applied.num_merged;
}

// ---- retriangulate (retriangulate_host.h) ----
// IncrementalTriangulator::Retriangulate as a module-level function with the triangulator first: tests pin that the
// class has no such method.  The host colours the statically eligible pairs into rounds, one
// amc_retriangulate_pairs call runs every round on the device, and the host replays the result in the sequential
// order.  Nothing of the reconstruction, of the modified set or of the trial counters changes unless everything
// succeeds.  Without a device the call raises pycolmap_amd._capi.AmcError.
// solver: None, or a callable that stands in for the library (a test hook): it takes the flat problem as a dict of
// arrays and returns a dict with pair_ran, corr_action, created_offsets and created_xyz.  max_correspondences: the
// bound above which the call is refused (the library's; tests pass a smaller one).
size_t retriangulate_with(PyTriangulator& t, const TriangulatorOptions& o, const py::object& solver, uint64_t max_correspondences) {
    const auto t0 = std::chrono::steady_clock::now();
    CheckTriangulatorOptions(o);
    PyReconstruction& r = t.reconstruction.cast<PyReconstruction&>();
    const CorrespondenceGraph& graph = t.graph.cast<const CorrespondenceGraph&>();
    SparseModel model = checked_model(r);
    ModelIndex ix(model, o);
    const FlatRetri flat = PlanRetriangulation(graph, model, ix, o, t.re_trials, max_correspondences);
    std::set<uint64_t> modified = t.modified;
    RetriTrials trials = t.re_trials;
    RetriApplied applied;
    uint64_t calls = 0;
    double device_ms = 0, kernel_ms = 0, copy_ms = 0;
    if (flat.NumPairs() == 0) {
        applied = ApplyRetriResult(flat, nullptr, nullptr, nullptr, nullptr, &model, &ix, &modified, &trials);
    } else if (!solver.is_none()) {
        py::dict d = CamerasAndPosesDict(flat);
        d["obs_image"] = NpArray(flat.obs_image, 1);
        d["obs_xy"] = NpArray(flat.obs_xy, 2);
        d["obs_point"] = NpArray(flat.obs_point, 1);
        d["point_xyz"] = NpArray(flat.point_xyz, 3);
        d["pair_images"] = NpArray(flat.pair_images, 2);
        d["pair_offsets"] = NpArray(flat.pair_offsets, 1);
        d["corr_obs"] = NpArray(flat.corr_obs, 2);
        d["corr_two_view"] = NpArray(flat.corr_two_view, 1);
        d["round_offsets"] = NpArray(flat.round_offsets, 1);
        d["create_max_angle_error"] = o.create_max_angle_error;
        d["re_max_angle_error"] = o.re_max_angle_error;
        d["min_angle"] = o.min_angle;
        d["re_min_ratio"] = o.re_min_ratio;
        const py::dict out = solver(d);
        const auto ran = CArray<uint8_t>::ensure(out["pair_ran"]);
        const auto act = CArray<uint8_t>::ensure(out["corr_action"]);
        const auto coff = CArray<uint64_t>::ensure(out["created_offsets"]);
        const auto cxyz = CArray<double>::ensure(out["created_xyz"]);
        if (!ran || !act || !coff || !cxyz || static_cast<size_t>(ran.size()) != flat.NumPairs() || static_cast<size_t>(act.size()) != flat.NumCorrs() ||
            static_cast<size_t>(coff.size()) != flat.NumPairs() + 1 || static_cast<uint64_t>(cxyz.size()) != 3 * coff.data()[flat.NumPairs()])
            throw py::value_error("retriangulate: the solver's result does not have the problem's shape");
        applied = ApplyRetriResult(flat, ran.data(), act.data(), coff.data(), cxyz.data(), &model, &ix, &modified, &trials);
    } else {
        amc_retri_opts opts;
        amc_retri_opts_default(&opts);
        opts.create_max_angle_error = o.create_max_angle_error;
        opts.re_max_angle_error = o.re_max_angle_error;
        opts.min_angle = o.min_angle;
        opts.re_min_ratio = o.re_min_ratio;
        const amc_retri_problem pb = flat.Problem();
        ResultGuard<amc_retri_result, amc_retri_result_free> res;
        CallLibrary([&](amc_ctx* ctx) { return amc_retriangulate_pairs(ctx, &pb, &opts, res.get()); }, "amc_retriangulate_pairs");
        calls = 1;
        device_ms = res->device_ms;
        kernel_ms = res->kernel_ms;
        copy_ms = res->copy_ms;
        applied = ApplyRetriResult(flat, res->pair_ran, res->corr_action, res->created_offsets, res->created_xyz, &model, &ix, &modified, &trials);
    }
    if (applied.num_tris != 0) update_with_new_points(r, model);
    t.modified.swap(modified);
    t.re_trials.swap(trials);
    py::dict st;
    st["call"] = "retriangulate";
    st["num_pairs"] = flat.NumPairs();
    st["num_pairs_run"] = applied.num_pairs_run;
    st["num_rounds"] = flat.NumRounds();
    st["num_correspondences"] = flat.NumCorrs();
    st["num_continued_observations"] = applied.num_continued;
    st["num_created_points"] = applied.num_created;
    st["num_device_calls"] = calls;
    FinishStats(st, t0, device_ms, kernel_ms, copy_ms);
    return applied.num_tris;
}

}  // namespace

void BindTriangulator(py::module_& m) {
    py::class_<Correspondence>(m, "Correspondence")
        .def(py::init<>())
        .def(py::init<uint32_t, uint32_t>(), "image_id"_a, "point2D_idx"_a)
        .def_readwrite("image_id", &Correspondence::image_id)
        .def_readwrite("point2D_idx", &Correspondence::point2D_idx)
        .def("__copy__", [](const Correspondence& c) { return Correspondence(c); })
        .def("__deepcopy__", [](const Correspondence& c, const py::dict&) { return Correspondence(c); })
        .def("__repr__", [](const Correspondence& c) {
            return "Correspondence(image_id=" + std::to_string(c.image_id) + ", point2D_idx=" + std::to_string(c.point2D_idx) + ")";
        });
    py::class_<CorrespondenceGraph, std::shared_ptr<CorrespondenceGraph>>(m, "CorrespondenceGraph")
        .def(py::init<>())
        .def("num_images", &CorrespondenceGraph::NumImages)
        .def("num_image_pairs", &CorrespondenceGraph::NumImagePairs)
        .def("exists_image", &CorrespondenceGraph::ExistsImage, "image_id"_a)
        .def("num_observations_for_image", &CorrespondenceGraph::NumObservationsForImage, "image_id"_a)
        .def("num_correspondences_for_image", &CorrespondenceGraph::NumCorrespondencesForImage, "image_id"_a)
        .def("num_correspondences_between_images", &CorrespondenceGraph::NumCorrespondencesBetweenImages, "image_id1"_a, "image_id2"_a)
        .def("finalize", &CorrespondenceGraph::Finalize)
        .def("add_image", &CorrespondenceGraph::AddImage, "image_id"_a, "num_points2D"_a)
        .def("add_correspondences", [](CorrespondenceGraph& g, uint32_t image_id1, uint32_t image_id2, const py::object& matches) {
                 const auto arr = CArray<uint32_t>::ensure(matches);
                 if (!arr) throw py::value_error("add_correspondences: matches must be convertible to an N x 2 uint32 array");
                 if (!(arr.ndim() == 2 && arr.shape(1) == 2) && arr.size() != 0)
                     throw py::value_error("add_correspondences: expected an N x 2 array of point2D indices");
                 const auto frame = PythonCallFrame();
                 for (const std::string& w : g.AddCorrespondences(image_id1, image_id2, arr.data(), static_cast<size_t>(arr.size() / 2)))
                     Logging::Write(Logging::WARNING, frame.first, frame.second, w);
             }, "image_id1"_a, "image_id2"_a, "correspondences"_a)
        .def("extract_correspondences", [](const CorrespondenceGraph& g, uint32_t image_id, uint32_t point2D_idx) {
                 return g.ExtractCorrespondences(image_id, point2D_idx);
             }, "image_id"_a, "point2D_idx"_a)
        .def("extract_transitive_correspondences", [](const CorrespondenceGraph& g, uint32_t image_id, uint32_t point2D_idx, size_t transitivity) {
                 std::vector<Correspondence> found;
                 g.ExtractTransitiveCorrespondences(image_id, point2D_idx, transitivity, &found);
                 return found;
             }, "image_id"_a, "point2D_idx"_a, "transitivity"_a)
        .def("find_correspondences_between_images", [](const CorrespondenceGraph& g, uint32_t image_id1, uint32_t image_id2) {
                 return NpArray(g.FindCorrespondencesBetweenImages(image_id1, image_id2), 2);
             }, "image_id1"_a, "image_id2"_a)
        .def("has_correspondences", &CorrespondenceGraph::HasCorrespondences, "image_id"_a, "point2D_idx"_a)
        .def("is_two_view_observation", &CorrespondenceGraph::IsTwoViewObservation, "image_id"_a, "point2D_idx"_a)
        .def("__copy__", [](const CorrespondenceGraph& g) { return std::make_shared<CorrespondenceGraph>(g); })
        .def("__deepcopy__", [](const CorrespondenceGraph& g, const py::dict&) { return std::make_shared<CorrespondenceGraph>(g); })
        .def("__repr__", [](const CorrespondenceGraph& g) {
            return "CorrespondenceGraph(num_images=" + std::to_string(g.NumImages()) + ", num_image_pairs=" + std::to_string(g.NumImagePairs()) + ")";
        });

    py::class_<TriangulatorOptions> PyTrgOpts(m, "IncrementalTriangulatorOptions");
    PyTrgOpts.def(py::init<>())
        .def_readwrite("max_transitivity", &TriangulatorOptions::max_transitivity, "Maximum transitivity to search for correspondences.")
        .def_readwrite("create_max_angle_error", &TriangulatorOptions::create_max_angle_error, "Maximum angular error to create new triangulations.")
        .def_readwrite("continue_max_angle_error", &TriangulatorOptions::continue_max_angle_error, "Maximum angular error to continue existing triangulations.")
        .def_readwrite("merge_max_reproj_error", &TriangulatorOptions::merge_max_reproj_error, "Maximum reprojection error in pixels to merge triangulations.")
        .def_readwrite("complete_max_reproj_error", &TriangulatorOptions::complete_max_reproj_error, "Maximum reprojection error to complete an existing triangulation.")
        .def_readwrite("complete_max_transitivity", &TriangulatorOptions::complete_max_transitivity, "Maximum transitivity for track completion.")
        .def_readwrite("re_max_angle_error", &TriangulatorOptions::re_max_angle_error, "Maximum angular error to re-triangulate under-reconstructed image pairs.")
        .def_readwrite("re_min_ratio", &TriangulatorOptions::re_min_ratio, "Minimum ratio of common triangulations between an image pair over the number of correspondences between that image pair to be considered as under-reconstructed.")
        .def_readwrite("re_max_trials", &TriangulatorOptions::re_max_trials, "Maximum number of trials to re-triangulate an image pair.")
        .def_readwrite("min_angle", &TriangulatorOptions::min_angle, "Minimum pairwise triangulation angle for a stable triangulation.")
        .def_readwrite("ignore_two_view_tracks", &TriangulatorOptions::ignore_two_view_tracks, "Whether to ignore two-view tracks.")
        .def_readwrite("min_focal_length_ratio", &TriangulatorOptions::min_focal_length_ratio, "Thresholds for bogus camera parameters: images with bogus camera parameters are ignored in triangulation.")
        .def_readwrite("max_focal_length_ratio", &TriangulatorOptions::max_focal_length_ratio)
        .def_readwrite("max_extra_param", &TriangulatorOptions::max_extra_param);
    MakeDataclass(PyTrgOpts, {"max_transitivity", "create_max_angle_error", "continue_max_angle_error", "merge_max_reproj_error",
                              "complete_max_reproj_error", "complete_max_transitivity", "re_max_angle_error", "re_min_ratio",
                              "re_max_trials", "min_angle", "ignore_two_view_tracks", "min_focal_length_ratio",
                              "max_focal_length_ratio", "max_extra_param"});

    py::class_<PyTriangulator>(m, "IncrementalTriangulator")
        .def(py::init([](const py::object& graph, const py::object& reconstruction) {
                 if (!py::isinstance<CorrespondenceGraph>(graph) || !py::isinstance<PyReconstruction>(reconstruction))
                     throw py::type_error("IncrementalTriangulator(correspondence_graph: CorrespondenceGraph, reconstruction: Reconstruction)");
                 return PyTriangulator{graph, reconstruction, {}, {}};
             }), "correspondence_graph"_a, "reconstruction"_a)
        .def("_triangulate_image_with", &triangulate_image_with, "options"_a, "image_id"_a, "solver"_a,
             "triangulate_image with a callable in the library's place (test hook).")
        .def("triangulate_image", [](PyTriangulator& t, const TriangulatorOptions& o, uint32_t image_id) {
                 return triangulate_image_with(t, o, image_id, py::none());
             }, "options"_a, "image_id"_a,
             "Triangulate observations of image: continue the tracks its correspondences carry and create new ones, on the\n"
             "GPU (DESIGN.md section 17).  Returns the number of triangulated observations.")
        .def("add_modified_point3D", [](PyTriangulator& t, uint64_t point3D_id) { t.modified.insert(point3D_id); }, "point3D_id"_a)
        .def("clear_modified_points3D", [](PyTriangulator& t) { t.modified.clear(); })
        .def("get_modified_points3D", [](const PyTriangulator& t) {
                 const PyReconstruction& r = t.reconstruction.cast<const PyReconstruction&>();
                 py::set ids;
                 for (uint64_t id : t.modified)
                     if (r.points3D.contains(py::int_(id))) ids.add(py::int_(id));
                 return ids;
             }, "The recorded ids of changed points that still exist.")
        .def_property_readonly("correspondence_graph", [](const PyTriangulator& t) { return t.graph; })
        .def_property_readonly("reconstruction", [](const PyTriangulator& t) { return t.reconstruction; })
        .def("__copy__", [](const PyTriangulator& t) { return PyTriangulator(t); })
        .def("__deepcopy__", [](const PyTriangulator& t, const py::dict& memo) {
                 const py::object deepcopy = py::module_::import("copy").attr("deepcopy");
                 return PyTriangulator{deepcopy(t.graph, memo), deepcopy(t.reconstruction, memo), t.modified, t.re_trials};
             })
        .def("__repr__", [](const PyTriangulator& t) {
            const PyReconstruction& r = t.reconstruction.cast<const PyReconstruction&>();
            return "IncrementalTriangulator(num_images=" + std::to_string(r.images.size()) + ", num_points3D=" + std::to_string(r.points3D.size()) +
                   ", num_modified_points3D=" + std::to_string(t.modified.size()) + ")";
        });

    m.def("_complete_tracks_with", &complete_tracks_with, "triangulator"_a, "options"_a, "point3D_ids"_a, "solver"_a,
          "complete_tracks (point3D_ids=None: complete_all_tracks) with a callable in the library's place (test hook).");
    m.def("complete_tracks", [](PyTriangulator& t, const TriangulatorOptions& o, const py::iterable& point3D_ids) {
              return complete_tracks_with(t, o, point3D_ids, py::none());
          }, "triangulator"_a, "options"_a, "point3D_ids"_a,
          "Complete the tracks of the given points3D: attach the observations their correspondences lead to, up to\n"
          "complete_max_transitivity steps away, that have no point yet and reproject within complete_max_reproj_error, on\n"
          "the GPU (DESIGN.md section 18).  The ids are a set, taken in ascending order.  Returns the number of added\n"
          "observations.");
    m.def("complete_all_tracks", [](PyTriangulator& t, const TriangulatorOptions& o) {
              return complete_tracks_with(t, o, py::none(), py::none());
          }, "triangulator"_a, "options"_a, "Complete the tracks of all points3D of the reconstruction (DESIGN.md section 18).");

    m.def("_merge_tracks_with", &merge_tracks_with, "triangulator"_a, "options"_a, "point3D_ids"_a, "solver"_a,
          "merge_tracks (point3D_ids=None: merge_all_tracks) with a callable in the library's place (test hook).");
    m.def("merge_tracks", [](PyTriangulator& t, const TriangulatorOptions& o, const py::iterable& point3D_ids) {
              return merge_tracks_with(t, o, point3D_ids, py::none());
          }, "triangulator"_a, "options"_a, "point3D_ids"_a,
          "Merge the given points3D with the points their correspondences carry, wherever every observation of both\n"
          "reprojects within merge_max_reproj_error of the weighted mean position, on the GPU (DESIGN.md section 18).  The ids\n"
          "are a set, taken in ascending order.  Returns the number of merged observations.");
    m.def("merge_all_tracks", [](PyTriangulator& t, const TriangulatorOptions& o) {
              return merge_tracks_with(t, o, py::none(), py::none());
          }, "triangulator"_a, "options"_a, "Merge the tracks of all points3D of the reconstruction (DESIGN.md section 18).");

    m.def("_retriangulate_with", &retriangulate_with, "triangulator"_a, "options"_a, "solver"_a,
          "max_correspondences"_a = static_cast<uint64_t>(AMC_RETRI_MAX_CORRS),
          "retriangulate with a callable in the library's place, or None for the library (test hook).");
    m.def("retriangulate", [](PyTriangulator& t, const TriangulatorOptions& o) {
              return retriangulate_with(t, o, py::none(), AMC_RETRI_MAX_CORRS);
          }, "triangulator"_a, "options"_a,
          "Retriangulate the under-reconstructed image pairs: for every pair of the correspondence graph whose share of\n"
          "correspondences with a common point3D is below re_min_ratio and that has trials left, continue tracks within\n"
          "re_max_angle_error and create two-view points, on the GPU (DESIGN.md section 19).  Returns the number of\n"
          "triangulated observations.");
    m.def("_retriangulate_trials", [](const PyTriangulator& t) {
              py::dict d;
              for (const auto& kv : t.re_trials)
                  d[py::make_tuple(static_cast<uint32_t>(kv.first >> 32), static_cast<uint32_t>(kv.first))] = kv.second;
              return d;
          }, "triangulator"_a, "The trial counters of retriangulate, {(image_id1, image_id2): trials} (test hook, a copy).");
    m.def("_retriangulate_rounds", [](const std::vector<std::pair<uint32_t, uint32_t>>& pairs) { return ColourRetriRounds(pairs); },
          "pairs"_a, "The round of every image pair under retriangulate's greedy colouring, pairs in the given order (test hook).");
}

}  // namespace amchost

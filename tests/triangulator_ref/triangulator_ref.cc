// triangulator_ref.cc — CPU reference of the correspondence graph and of the incremental triangulator's
// TriangulateImage, written from DESIGN.md section 17 alone (it includes none of pycolmap_amd/csrc).  The LO-RANSAC,
// the acos and the triangulation angle are section 11's: this file includes tests/tri_ref/tri_ref.cc for them.  Plain
// scalar sequential C++, -ffp-contract=off: the GPU path must match it bit for bit.  Pixels arrive already lifted to the
// normalised image plane (the wrapper lifts them with the oracle's Camera::CamFromImg).
#include "../tri_ref/tri_ref.cc"

#include <algorithm>
#include <map>
#include <set>
#include <unordered_map>

namespace {

const double kDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;
const uint64_t kNoPoint = ~static_cast<uint64_t>(0);

// ---- 17.1: the graph ---------------------------------------------------------------------------------------------------
struct Corr {
    uint32_t image, idx;
};
struct GImage {
    size_t nobs = 0, ncorr = 0;
    std::vector<std::vector<Corr>> corrs;
};
struct Graph {
    std::map<uint32_t, GImage> images;
    std::map<std::pair<uint32_t, uint32_t>, size_t> pairs;

    static std::pair<uint32_t, uint32_t> Key(uint32_t a, uint32_t b) { return a < b ? std::make_pair(a, b) : std::make_pair(b, a); }
    // returns false for an unknown image
    bool AddCorrespondences(uint32_t id1, uint32_t id2, const uint32_t* m, size_t n) {
        if (id1 == id2) return true;  // ignored (with a warning)
        if (!images.count(id1) || !images.count(id2)) return false;
        GImage& a = images[id1];
        GImage& b = images[id2];
        size_t& pair = pairs[Key(id1, id2)];
        a.ncorr += n;
        b.ncorr += n;
        pair += n;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t p = m[2 * i], q = m[2 * i + 1];
            bool ok = p < a.corrs.size() && q < b.corrs.size();
            if (ok) {
                for (const Corr& c : a.corrs[p]) ok = ok && c.image != id2;
                for (const Corr& c : b.corrs[q]) ok = ok && c.image != id1;
            }
            if (ok) {
                a.corrs[p].push_back(Corr{id2, q});
                b.corrs[q].push_back(Corr{id1, p});
            } else {
                a.ncorr -= 1;
                b.ncorr -= 1;
                pair -= 1;
            }
        }
        return true;
    }
    void Finalize() {
        for (auto it = images.begin(); it != images.end();) {
            it->second.nobs = 0;
            for (const auto& c : it->second.corrs) it->second.nobs += !c.empty();
            if (it->second.nobs == 0)
                it = images.erase(it);
            else
                ++it;
        }
    }
    const std::vector<Corr>* Corrs(uint32_t image, uint32_t idx) const {
        const auto it = images.find(image);
        if (it == images.end() || idx >= it->second.corrs.size()) return nullptr;
        return &it->second.corrs[idx];
    }
    // false for an unknown image or index
    bool Transitive(uint32_t image, uint32_t idx, size_t transitivity, std::vector<Corr>* found) const {
        found->clear();
        const std::vector<Corr>* direct = Corrs(image, idx);
        if (!direct) return false;
        if (transitivity == 1) {
            *found = *direct;
            return true;
        }
        if (direct->empty()) return true;
        found->push_back(Corr{image, idx});
        std::set<std::pair<uint32_t, uint32_t>> seen{{image, idx}};
        size_t begin = 0, end = 1;
        for (size_t t = 0; t < transitivity; ++t) {
            for (size_t i = begin; i < end; ++i) {
                const Corr ref = (*found)[i];
                for (const Corr& c : *Corrs(ref.image, ref.idx))
                    if (seen.insert({c.image, c.idx}).second) found->push_back(c);
            }
            begin = end;
            end = found->size();
            if (begin == end) break;
        }
        (*found)[0] = found->back();
        found->pop_back();
        return true;
    }
    bool IsTwoView(uint32_t image, uint32_t idx) const {
        const std::vector<Corr>* c = Corrs(image, idx);
        if (!c || c->size() != 1) return false;
        return Corrs((*c)[0].image, (*c)[0].idx)->size() == 1;
    }
};

// ---- 17.2 - 17.3 on one observation list --------------------------------------------------------------------------------
struct Cand {
    double x, y;       // normalised
    const Pose* pose;
    bool has_point;
    double xyz[3];
};
struct TriOpts {
    double create_max_angle_error, continue_max_angle_error, min_angle;
};
struct ItemResult {
    int continued = -1;
    double continue_angle = 0;          // the best angle, when a candidate carried a point and the reference did not
    bool continue_tested = false;
    std::vector<uint32_t> round;        // per candidate
    std::vector<Vec3> xyz;              // per round
    std::vector<double> final_errors;   // the angular error of every observation of a round under its final model
};

// 11.2's residual before squaring
double AngularError(double x, double y, const Pose& p, const double* X) {
    const Obs o{x, y, &p};
    const double na = std::sqrt(o.x * o.x + o.y * o.y + 1.0);
    const double a[3] = {o.x / na, o.y / na, 1.0 / na};
    double q[3];
    for (int r = 0; r < 3; ++r) q[r] = p.P[r][0] * X[0] + p.P[r][1] * X[1] + p.P[r][2] * X[2] + p.P[r][3];
    const double nb = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double c = a[0] * (q[0] / nb) + a[1] * (q[1] / nb) + a[2] * (q[2] / nb);
    return Acos(c);
}

// cands: the found correspondences in Find's order, the reference observation last
ItemResult RunItem(const std::vector<Cand>& cands, bool no_create_two_view, const TriOpts& o) {
    ItemResult res;
    const size_t n = cands.size();
    res.round.assign(n, 0);
    bool ref_has = cands[n - 1].has_point;
    // Continue
    if (!ref_has) {
        double best = std::numeric_limits<double>::max();
        int best_k = -1;
        for (size_t k = 0; k + 1 < n; ++k) {
            if (!cands[k].has_point) continue;
            const double e = AngularError(cands[n - 1].x, cands[n - 1].y, *cands[n - 1].pose, cands[k].xyz);
            if (e < best) {
                best = e;
                best_k = static_cast<int>(k);
            }
        }
        if (best_k >= 0) {
            res.continue_tested = true;
            res.continue_angle = best;
            if (best <= kDegToRad * o.continue_max_angle_error) {
                res.continued = best_k;
                ref_has = true;
            }
        }
    }
    // Create
    std::vector<size_t> kept;
    for (size_t k = 0; k < n; ++k)
        if (!(k + 1 == n ? ref_has : cands[k].has_point)) kept.push_back(k);
    for (uint32_t round = 1;; ++round) {
        const size_t m = kept.size();
        if (m < 2) break;
        if (round == 1 && m == 2 && no_create_two_view) break;
        Options ro;
        ro.min_tri_angle = kDegToRad * o.min_angle;
        ro.max_error = kDegToRad * o.create_max_angle_error;
        ro.min_inlier_ratio = 0.02;
        ro.confidence = 0.9999;
        ro.multiplier = 3.0;
        ro.max_num_trials = 10000;
        ro.min_num_trials = m <= 15 ? static_cast<int64_t>(m * (m - 1) / 2) : 0;
        std::vector<Obs> obs;
        for (size_t k : kept) obs.push_back(Obs{cands[k].x, cands[k].y, cands[k].pose});
        const Report rep = LoRansac(ro, obs);
        if (!rep.success) break;
        res.xyz.push_back(rep.model);
        std::vector<size_t> left;
        for (size_t i = 0; i < m; ++i) {
            res.final_errors.push_back(AngularError(obs[i].x, obs[i].y, *obs[i].pose, rep.model.v));
            if (rep.mask[i])
                res.round[kept[i]] = round;
            else
                left.push_back(kept[i]);
        }
        if (left.size() < 3) break;
        kept.swap(left);
    }
    return res;
}

// 11.1: [R | t] from the quaternion (x, y, z, w) and the centre -(R^T t)
Pose MakePose(const double* q, const double* t) {
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

// ---- 17.2: the sequential TriangulateImage on a scene -----------------------------------------------------------------
struct SCamera {
    int model;
    uint64_t width, height;
    std::vector<double> params;
};
struct SImage {
    uint32_t camera;
    Pose pose;
    std::vector<double> nxy;        // 2 per point2D, normalised
    std::vector<uint64_t> point3D;  // per point2D, kNoPoint = none
};
struct SPoint {
    double xyz[3];
    double error = 0;
    std::vector<Corr> track;
};
struct Scene {
    std::map<uint32_t, SCamera> cameras;
    std::map<uint32_t, SImage> images;
    std::map<uint64_t, SPoint> points;
    Graph graph;
    std::set<uint64_t> modified;
    double min_continue_margin = std::numeric_limits<double>::infinity();
    double min_create_margin = std::numeric_limits<double>::infinity();
};

int NumFocal(int model) { return (model == 0 || model == 2 || model == 3 || model == 8 || model == 9) ? 1 : 2; }

// Camera::HasBogusParams
bool Bogus(const SCamera& c, double min_ratio, double max_ratio, double max_extra) {
    const int nf = NumFocal(c.model);
    const double cx = c.params[nf], cy = c.params[nf + 1];
    if (cx < 0 || cx > static_cast<double>(c.width) || cy < 0 || cy > static_cast<double>(c.height)) return true;
    const double max_size = static_cast<double>(std::max(c.width, c.height));
    for (int i = 0; i < nf; ++i) {
        const double ratio = c.params[i] / max_size;
        if (ratio < min_ratio || ratio > max_ratio) return true;
    }
    for (size_t i = nf + 2; i < c.params.size(); ++i)
        if (std::fabs(c.params[i]) > max_extra) return true;
    return false;
}

// options: the fourteen fields in the order of 17.2's table
int64_t TriangulateImage(Scene* s, const double* op, uint32_t image_id) {
    const size_t max_transitivity = static_cast<size_t>(op[0]);
    const TriOpts to{op[1], op[2], op[9]};
    const bool ignore_two_view = op[10] != 0.0;
    const auto iit = s->images.find(image_id);
    if (iit == s->images.end() || !s->graph.images.count(image_id)) return -1;
    SImage& image = iit->second;
    if (Bogus(s->cameras.at(image.camera), op[11], op[12], op[13])) return 0;
    int64_t count = 0;
    std::vector<Corr> found;
    for (uint32_t p = 0; p < image.point3D.size(); ++p) {
        // Find
        if (!s->graph.Transitive(image_id, p, max_transitivity, &found)) return -1;
        std::vector<Corr> who;
        std::vector<Cand> cands;
        for (const Corr& c : found) {
            const auto cit = s->images.find(c.image);
            if (cit == s->images.end()) continue;
            if (Bogus(s->cameras.at(cit->second.camera), op[11], op[12], op[13])) continue;
            Cand cd{cit->second.nxy[2 * c.idx], cit->second.nxy[2 * c.idx + 1], &cit->second.pose, false, {0, 0, 0}};
            const uint64_t pid = cit->second.point3D[c.idx];
            if (pid != kNoPoint) {
                cd.has_point = true;
                for (int k = 0; k < 3; ++k) cd.xyz[k] = s->points.at(pid).xyz[k];
            }
            who.push_back(c);
            cands.push_back(cd);
        }
        if (cands.empty()) continue;
        // the first found correspondence without a point decides the two-view rule
        bool no_two_view = false;
        for (size_t k = 0; k < cands.size(); ++k)
            if (!cands[k].has_point) {
                no_two_view = ignore_two_view && s->graph.IsTwoView(who[k].image, who[k].idx);
                break;
            }
        Cand ref{image.nxy[2 * p], image.nxy[2 * p + 1], &image.pose, image.point3D[p] != kNoPoint, {0, 0, 0}};
        who.push_back(Corr{image_id, p});
        cands.push_back(ref);
        const ItemResult r = RunItem(cands, no_two_view, to);
        if (r.continue_tested)
            s->min_continue_margin = std::min(s->min_continue_margin, std::fabs(r.continue_angle - kDegToRad * to.continue_max_angle_error));
        for (double e : r.final_errors)
            if (e == e) s->min_create_margin = std::min(s->min_create_margin, std::fabs(e - kDegToRad * to.create_max_angle_error));
        if (r.continued >= 0) {
            const Corr& c = who[r.continued];
            const uint64_t pid = s->images.at(c.image).point3D[c.idx];
            s->points.at(pid).track.push_back(Corr{image_id, p});
            image.point3D[p] = pid;
            s->modified.insert(pid);
            count += 1;
        }
        for (uint32_t round = 1; round <= r.xyz.size(); ++round) {
            SPoint pt;
            for (int k = 0; k < 3; ++k) pt.xyz[k] = r.xyz[round - 1].v[k];
            pt.error = -1.0;
            const uint64_t pid = s->points.empty() ? 1 : std::max<uint64_t>(1, s->points.rbegin()->first + 1);
            for (size_t k = 0; k < cands.size(); ++k)
                if (r.round[k] == round) {
                    pt.track.push_back(who[k]);
                    s->images.at(who[k].image).point3D[who[k].idx] = pid;
                }
            count += static_cast<int64_t>(pt.track.size());
            s->points[pid] = pt;
            s->modified.insert(pid);
        }
    }
    return count;
}

}  // namespace

extern "C" {

double triref_angular_error(const double* nxy, const double* q, const double* t, const double* X) {
    return AngularError(nxy[0], nxy[1], MakePose(q, t), X);
}

// The flat problem of include/amc_triobs.h with the candidates already lifted (cand_nxy).  Outputs: continued (items),
// cand_round (candidates), num_rounds (items), round_xyz (3 per round slot: item i's rounds start at slot
// slot_offsets[i], and the caller leaves it floor(n_i / 2) slots).  Returns 0, or -1 for invalid input.
int triref_observations(size_t nimg, const double* qvec, const double* tvec, size_t nitems, const uint64_t* off,
                        const uint32_t* cand_image, const double* cand_nxy, const uint8_t* cand_has, const double* cand_xyz,
                        const uint8_t* two_view, double create_max_angle_error, double continue_max_angle_error,
                        double min_angle, int32_t* continued, uint32_t* cand_round, uint32_t* num_rounds,
                        const uint64_t* slot_offsets, double* round_xyz) {
    if (off[0] != 0) return -1;
    std::vector<Pose> poses(nimg);
    for (size_t i = 0; i < nimg; ++i) poses[i] = MakePose(qvec + 4 * i, tvec + 3 * i);
    const TriOpts to{create_max_angle_error, continue_max_angle_error, min_angle};
    for (size_t i = 0; i < nitems; ++i) {
        if (off[i + 1] <= off[i]) return -1;
        std::vector<Cand> cands;
        for (uint64_t k = off[i]; k < off[i + 1]; ++k) {
            if (cand_image[k] >= nimg) return -1;
            cands.push_back(Cand{cand_nxy[2 * k], cand_nxy[2 * k + 1], &poses[cand_image[k]], cand_has[k] != 0,
                                 {cand_xyz[3 * k], cand_xyz[3 * k + 1], cand_xyz[3 * k + 2]}});
        }
        const ItemResult r = RunItem(cands, two_view && two_view[i], to);
        continued[i] = r.continued;
        for (size_t k = 0; k < cands.size(); ++k) cand_round[off[i] + k] = r.round[k];
        num_rounds[i] = static_cast<uint32_t>(r.xyz.size());
        for (size_t j = 0; j < r.xyz.size(); ++j)
            for (int c = 0; c < 3; ++c) round_xyz[3 * (slot_offsets[i] + j) + c] = r.xyz[j].v[c];
    }
    return 0;
}

void* triref_scene_new() { return new Scene(); }
void triref_scene_free(void* s) { delete static_cast<Scene*>(s); }
void triref_add_camera(void* s, uint32_t id, int model, uint64_t width, uint64_t height, const double* params, int nparams) {
    static_cast<Scene*>(s)->cameras[id] = SCamera{model, width, height, std::vector<double>(params, params + nparams)};
}
// q: x y z w; nxy: normalised points; point3D: ids or ~0
void triref_add_image(void* s, uint32_t id, uint32_t camera, const double* q, const double* t, size_t npts, const double* nxy,
                      const uint64_t* point3D) {
    SImage im;
    im.camera = camera;
    im.pose = MakePose(q, t);
    im.nxy.assign(nxy, nxy + 2 * npts);
    im.point3D.assign(point3D, point3D + npts);
    static_cast<Scene*>(s)->images[id] = im;
}
void triref_add_point(void* s, uint64_t id, const double* xyz, size_t len, const uint32_t* track_image, const uint32_t* track_idx) {
    SPoint p;
    for (int k = 0; k < 3; ++k) p.xyz[k] = xyz[k];
    for (size_t i = 0; i < len; ++i) p.track.push_back(Corr{track_image[i], track_idx[i]});
    static_cast<Scene*>(s)->points[id] = p;
}
void triref_graph_add_image(void* s, uint32_t id, size_t npts) { static_cast<Scene*>(s)->graph.images[id].corrs.resize(npts); }
int triref_graph_add_correspondences(void* s, uint32_t id1, uint32_t id2, const uint32_t* matches, size_t n) {
    return static_cast<Scene*>(s)->graph.AddCorrespondences(id1, id2, matches, n) ? 0 : -1;
}
void triref_graph_finalize(void* s) { static_cast<Scene*>(s)->graph.Finalize(); }
size_t triref_graph_num_images(void* s) { return static_cast<Scene*>(s)->graph.images.size(); }
int triref_graph_exists_image(void* s, uint32_t id) { return static_cast<Scene*>(s)->graph.images.count(id) ? 1 : 0; }
// out: nobs, ncorr; -1 for an unknown image
int triref_graph_image_counts(void* s, uint32_t id, uint64_t* out) {
    const Graph& g = static_cast<Scene*>(s)->graph;
    const auto it = g.images.find(id);
    if (it == g.images.end()) return -1;
    out[0] = it->second.nobs;
    out[1] = it->second.ncorr;
    return 0;
}
uint64_t triref_graph_pair_count(void* s, uint32_t id1, uint32_t id2) {
    const Graph& g = static_cast<Scene*>(s)->graph;
    const auto it = g.pairs.find(Graph::Key(id1, id2));
    return it == g.pairs.end() ? 0 : it->second;
}
// the transitive correspondences into out_image / out_idx (cap entries); returns their number, or -1
int64_t triref_graph_transitive(void* s, uint32_t id, uint32_t idx, size_t transitivity, uint32_t* out_image, uint32_t* out_idx,
                                size_t cap) {
    std::vector<Corr> found;
    if (!static_cast<Scene*>(s)->graph.Transitive(id, idx, transitivity, &found)) return -1;
    for (size_t i = 0; i < found.size() && i < cap; ++i) {
        out_image[i] = found[i].image;
        out_idx[i] = found[i].idx;
    }
    return static_cast<int64_t>(found.size());
}
int triref_graph_is_two_view(void* s, uint32_t id, uint32_t idx) { return static_cast<Scene*>(s)->graph.IsTwoView(id, idx) ? 1 : 0; }

int64_t triref_triangulate_image(void* s, const double* options14, uint32_t image_id) {
    return TriangulateImage(static_cast<Scene*>(s), options14, image_id);
}
size_t triref_num_points(void* s) { return static_cast<Scene*>(s)->points.size(); }
// ids, xyz (3 each), errors, track lengths, in ascending id order
void triref_get_points(void* s, uint64_t* ids, double* xyz, double* errors, uint64_t* lens) {
    size_t i = 0;
    for (const auto& kv : static_cast<Scene*>(s)->points) {
        ids[i] = kv.first;
        for (int k = 0; k < 3; ++k) xyz[3 * i + k] = kv.second.xyz[k];
        errors[i] = kv.second.error;
        lens[i] = kv.second.track.size();
        ++i;
    }
}
void triref_get_track(void* s, uint64_t id, uint32_t* image, uint32_t* idx) {
    const SPoint& p = static_cast<Scene*>(s)->points.at(id);
    for (size_t i = 0; i < p.track.size(); ++i) {
        image[i] = p.track[i].image;
        idx[i] = p.track[i].idx;
    }
}
void triref_get_point2D_ids(void* s, uint32_t image_id, uint64_t* ids) {
    const SImage& im = static_cast<Scene*>(s)->images.at(image_id);
    std::copy(im.point3D.begin(), im.point3D.end(), ids);
}
size_t triref_num_modified(void* s) { return static_cast<Scene*>(s)->modified.size(); }
void triref_get_modified(void* s, uint64_t* ids) {
    size_t i = 0;
    for (uint64_t id : static_cast<Scene*>(s)->modified) ids[i++] = id;
}
// the smallest distance of a deciding angle from its threshold so far: [0] Continue's best angle, [1] an observation's
// angular error under a created point
void triref_margins(void* s, double* out) {
    out[0] = static_cast<Scene*>(s)->min_continue_margin;
    out[1] = static_cast<Scene*>(s)->min_create_margin;
}

}  // extern "C"

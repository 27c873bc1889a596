// model_io.cc — reader (.bin, .txt) and writer (.bin) of COLMAP 3.9's sparse model files; see model_io.h.
#include "model_io.h"

#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace amchost {
namespace {

const char* const kModelNames[11] = {"SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE",
                                     "FULL_OPENCV", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"};
const int kModelParams[11] = {3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12};

[[noreturn]] void Bad(const std::string& path, const std::string& what) {
    throw std::invalid_argument(path + ": " + what);
}

bool Exists(const std::string& path) { return std::ifstream(path, std::ios::binary).good(); }

std::string Slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f.good()) Bad(path, "cannot be opened");
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// little-endian fields of a .bin file, bounds-checked
struct BinReader {
    const std::string& path;
    const std::string data;
    size_t at = 0;
    explicit BinReader(const std::string& p) : path(p), data(Slurp(p)) {}
    template <typename T>
    T Get() {
        if (data.size() - at < sizeof(T)) Bad(path, "is truncated");
        T v;
        std::memcpy(&v, data.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    std::string GetString() {
        const size_t e = data.find('\0', at);
        if (e == std::string::npos) Bad(path, "has an unterminated image name");
        std::string s = data.substr(at, e - at);
        at = e + 1;
        return s;
    }
    // a count whose records take at least `each` bytes
    uint64_t GetCount(size_t each) {
        const uint64_t n = Get<uint64_t>();
        if (n > (data.size() - at) / each) Bad(path, "holds a count larger than the file");
        return n;
    }
    void End() const {
        if (at != data.size()) Bad(path, "has trailing bytes");
    }
};

template <typename T>
void Put(std::string& out, T v) {
    out.append(reinterpret_cast<const char*>(&v), sizeof(T));
}

void Dump(const std::string& path, const std::string& bytes) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), static_cast<std::streamsize>(bytes.size()));
    if (!f.good()) throw std::runtime_error(path + ": cannot be written");
}

SparseModel ReadBin(const std::string& dir) {
    SparseModel m;
    {
        const std::string path = dir + "/cameras.bin";
        BinReader r(path);
        const uint64_t n = r.GetCount(24);
        for (uint64_t i = 0; i < n; ++i) {
            ModelCamera c;
            c.camera_id = r.Get<uint32_t>();
            c.model = r.Get<int32_t>();
            c.width = r.Get<uint64_t>();
            c.height = r.Get<uint64_t>();
            const int np = ModelNumParams(c.model);
            if (np < 0) Bad(path, "names the unknown camera model id " + std::to_string(c.model));
            for (int k = 0; k < np; ++k) c.params.push_back(r.Get<double>());
            m.cameras.push_back(std::move(c));
        }
        r.End();
    }
    {
        const std::string path = dir + "/images.bin";
        BinReader r(path);
        const uint64_t n = r.GetCount(73);
        for (uint64_t i = 0; i < n; ++i) {
            ModelImage im;
            im.image_id = r.Get<uint32_t>();
            for (double& q : im.qvec) q = r.Get<double>();
            for (double& t : im.tvec) t = r.Get<double>();
            im.camera_id = r.Get<uint32_t>();
            im.name = r.GetString();
            const uint64_t np = r.GetCount(24);
            im.points2D.resize(np);
            for (ModelPoint2D& p : im.points2D) {
                p.x = r.Get<double>();
                p.y = r.Get<double>();
                p.point3D_id = r.Get<uint64_t>();
            }
            m.images.push_back(std::move(im));
        }
        r.End();
    }
    {
        const std::string path = dir + "/points3D.bin";
        BinReader r(path);
        const uint64_t n = r.GetCount(51);
        for (uint64_t i = 0; i < n; ++i) {
            ModelPoint3D p;
            p.point3D_id = r.Get<uint64_t>();
            for (double& v : p.xyz) v = r.Get<double>();
            for (uint8_t& v : p.rgb) v = r.Get<uint8_t>();
            p.error = r.Get<double>();
            const uint64_t nt = r.GetCount(8);
            p.track.resize(nt);
            for (auto& t : p.track) {
                t.first = r.Get<uint32_t>();
                t.second = r.Get<uint32_t>();
            }
            m.points3D.push_back(std::move(p));
        }
        r.End();
    }
    return m;
}

// the data lines of a .txt file: comment lines ('#') are dropped everywhere; blank lines are dropped unless
// keep_blank (images.txt: an image without points2D has an empty second line)
std::vector<std::string> TextLines(const std::string& path, bool keep_blank) {
    std::istringstream ss(Slurp(path));
    std::vector<std::string> lines;
    std::string line;
    while (std::getline(ss, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        const size_t a = line.find_first_not_of(" \t");
        if (a != std::string::npos && line[a] == '#') continue;
        if (a == std::string::npos && !keep_blank) continue;
        lines.push_back(a == std::string::npos ? std::string() : line.substr(a));
    }
    return lines;
}

template <typename T>
T Field(std::istringstream& ss, const std::string& path, const std::string& line) {
    T v;
    if (!(ss >> v)) Bad(path, "has a malformed line: " + line);
    return v;
}
// doubles go through strtod: every decimal a writer prints with 17 digits comes back as the same bits
template <>
double Field<double>(std::istringstream& ss, const std::string& path, const std::string& line) {
    std::string tok;
    if (!(ss >> tok)) Bad(path, "has a malformed line: " + line);
    char* end = nullptr;
    const double v = std::strtod(tok.c_str(), &end);
    if (end == tok.c_str() || *end != '\0') Bad(path, "has a malformed number '" + tok + "' in line: " + line);
    return v;
}

SparseModel ReadTxt(const std::string& dir) {
    SparseModel m;
    {
        const std::string path = dir + "/cameras.txt";
        for (const std::string& line : TextLines(path, false)) {
            std::istringstream ss(line);
            ModelCamera c;
            c.camera_id = Field<uint32_t>(ss, path, line);
            const std::string name = Field<std::string>(ss, path, line);
            c.model = ModelIdFromName(name);
            if (c.model < 0) Bad(path, "names the unknown camera model " + name);
            c.width = Field<uint64_t>(ss, path, line);
            c.height = Field<uint64_t>(ss, path, line);
            for (int k = 0; k < ModelNumParams(c.model); ++k) c.params.push_back(Field<double>(ss, path, line));
            m.cameras.push_back(std::move(c));
        }
    }
    {
        const std::string path = dir + "/images.txt";
        const std::vector<std::string> lines = TextLines(path, true);
        size_t i = 0;
        while (i < lines.size()) {
            if (lines[i].empty()) {  // blank lines between images
                ++i;
                continue;
            }
            std::istringstream ss(lines[i]);
            ModelImage im;
            im.image_id = Field<uint32_t>(ss, path, lines[i]);
            for (double& q : im.qvec) q = Field<double>(ss, path, lines[i]);
            for (double& t : im.tvec) t = Field<double>(ss, path, lines[i]);
            im.camera_id = Field<uint32_t>(ss, path, lines[i]);
            std::getline(ss, im.name);  // the rest of the line: names may hold spaces
            const size_t a = im.name.find_first_not_of(" \t");
            im.name = a == std::string::npos ? std::string() : im.name.substr(a);
            if (im.name.empty()) Bad(path, "has an image line without a name: " + lines[i]);
            ++i;
            if (i < lines.size()) {  // the points2D line (may be empty)
                std::istringstream ps(lines[i]);
                std::string tok;
                while (ps >> tok) {
                    std::istringstream one(tok);
                    ModelPoint2D p;
                    p.x = Field<double>(one, path, lines[i]);
                    p.y = Field<double>(ps, path, lines[i]);
                    const std::string id = Field<std::string>(ps, path, lines[i]);
                    p.point3D_id = id == "-1" ? kInvalidPoint3DId : std::strtoull(id.c_str(), nullptr, 10);
                    im.points2D.push_back(p);
                }
                ++i;
            }
            m.images.push_back(std::move(im));
        }
    }
    {
        const std::string path = dir + "/points3D.txt";
        for (const std::string& line : TextLines(path, false)) {
            std::istringstream ss(line);
            ModelPoint3D p;
            p.point3D_id = Field<uint64_t>(ss, path, line);
            for (double& v : p.xyz) v = Field<double>(ss, path, line);
            for (uint8_t& v : p.rgb) v = static_cast<uint8_t>(Field<int>(ss, path, line));
            p.error = Field<double>(ss, path, line);
            uint32_t image_id;
            while (ss >> image_id) p.track.emplace_back(image_id, Field<uint32_t>(ss, path, line));
            m.points3D.push_back(std::move(p));
        }
    }
    return m;
}

}  // namespace

int ModelNumParams(int model) { return model >= 0 && model < 11 ? kModelParams[model] : -1; }
int ModelIdFromName(const std::string& name) {
    for (int i = 0; i < 11; ++i)
        if (name == kModelNames[i]) return i;
    return -1;
}

const ModelCamera* SparseModel::FindCamera(uint32_t camera_id) const {
    for (const ModelCamera& c : cameras)
        if (c.camera_id == camera_id) return &c;
    return nullptr;
}

SparseModel ReadSparseModelBin(const std::string& dir) { return ReadBin(dir); }
SparseModel ReadSparseModelTxt(const std::string& dir) { return ReadTxt(dir); }

SparseModel ReadSparseModel(const std::string& dir) {
    const bool bin = Exists(dir + "/cameras.bin") && Exists(dir + "/images.bin") && Exists(dir + "/points3D.bin");
    const bool txt = Exists(dir + "/cameras.txt") && Exists(dir + "/images.txt") && Exists(dir + "/points3D.txt");
    if (!bin && !txt) Bad(dir, "cameras, images, points3D files do not exist as .bin or .txt");
    SparseModel m = bin ? ReadBin(dir) : ReadTxt(dir);
    for (const ModelImage& im : m.images)
        if (!m.FindCamera(im.camera_id))
            Bad(dir, "image " + im.name + " names camera " + std::to_string(im.camera_id) + ", which the model does not hold");
    return m;
}

void WriteSparseModelBin(const std::string& dir, const SparseModel& m) {
    std::string b;
    Put<uint64_t>(b, m.cameras.size());
    for (const ModelCamera& c : m.cameras) {
        Put<uint32_t>(b, c.camera_id);
        Put<int32_t>(b, c.model);
        Put<uint64_t>(b, c.width);
        Put<uint64_t>(b, c.height);
        for (double p : c.params) Put<double>(b, p);
    }
    Dump(dir + "/cameras.bin", b);
    b.clear();
    Put<uint64_t>(b, m.images.size());
    for (const ModelImage& im : m.images) {
        Put<uint32_t>(b, im.image_id);
        for (double q : im.qvec) Put<double>(b, q);
        for (double t : im.tvec) Put<double>(b, t);
        Put<uint32_t>(b, im.camera_id);
        b.append(im.name);
        b.push_back('\0');
        Put<uint64_t>(b, im.points2D.size());
        for (const ModelPoint2D& p : im.points2D) {
            Put<double>(b, p.x);
            Put<double>(b, p.y);
            Put<uint64_t>(b, p.point3D_id);
        }
    }
    Dump(dir + "/images.bin", b);
    b.clear();
    Put<uint64_t>(b, m.points3D.size());
    for (const ModelPoint3D& p : m.points3D) {
        Put<uint64_t>(b, p.point3D_id);
        for (double v : p.xyz) Put<double>(b, v);
        for (uint8_t v : p.rgb) Put<uint8_t>(b, v);
        Put<double>(b, p.error);
        Put<uint64_t>(b, p.track.size());
        for (const auto& t : p.track) {
            Put<uint32_t>(b, t.first);
            Put<uint32_t>(b, t.second);
        }
    }
    Dump(dir + "/points3D.bin", b);
}

}  // namespace amchost

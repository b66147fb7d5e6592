// vrhip_render -- headless host: loads a .dat/.raw volume (or a synthetic field), sets camera
// and transfer function the way the reference's Qt widget does
// (/root/reference/src/qt/volumerenderwidget.cpp:916-938 TF table, :1079-1098 view matrix),
// renders through VolumeRenderCL and writes the float RGBA framebuffer to disk.  Replaces the
// Qt/OpenGL front end dropped by the north star.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <map>
#include <cctype>
#include <iterator>
#include <limits>
#include <string>
#include <vector>

#include <memory>
#include <chrono>

#include <hip/hip_runtime_api.h>

#include "tilegather.h"
#include "volumerendercl.h"
#include "vrhip_cli.h"

namespace {

struct Stop { double pos; int c[4]; };

// QEasingCurve::valueForProgress for the three curves the GUI offers (mainwindow.cpp:945-957), with the
// operation order of Qt's src/3rdparty/easing/easing.cpp (easeNone, easeInOutQuad, easeInOutCubic)
double ease(const std::string &kind, double t)
{
    t = std::min(1.0, std::max(0.0, t));
    if (kind == "quad") {
        t *= 2.0;
        if (t < 1) return t * t / 2.0;
        --t;
        return -0.5 * (t * (t - 2) - 1);
    }
    if (kind == "cubic") {
        t *= 2.0;
        if (t < 1) return 0.5 * t * t * t;
        t -= 2.0;
        return 0.5 * (t * t * t + 2);
    }
    return t;
}

// updateTransferFunction (volumerenderwidget.cpp:916-938): 1024 entries, entry i = the key-value
// animation over the stops at time qRound(i/1024*8192) of 8192; QVariantAnimation interpolates QColor
// per channel as qBound(0, int(f + (t - f) * localProgress), 255) with localProgress = (progress -
// start) / (end - start) in double; then max(0, c - 3).  setKeyValueAt replaces an earlier key at the
// same position; missing end stops (the GUI always has them) repeat the nearest stop's colour.
std::vector<unsigned char> tff_from_stops(std::vector<Stop> in, int n = 1024, const std::string &easing = "linear")
{
    std::stable_sort(in.begin(), in.end(), [](const Stop &a, const Stop &b) { return a.pos < b.pos; });
    std::vector<Stop> stops;
    for (const Stop &s : in) {
        if (!stops.empty() && stops.back().pos == s.pos) stops.back() = s;
        else stops.push_back(s);
    }
    if (stops.front().pos > 0.0) { Stop s = stops.front(); s.pos = 0.0; stops.insert(stops.begin(), s); }
    if (stops.back().pos < 1.0) { Stop s = stops.back(); s.pos = 1.0; stops.push_back(s); }
    std::vector<unsigned char> out(size_t(n) * 4, 0);
    for (int i = 0; i < n; ++i) {
        const double time = std::floor(double(i) / n * 8192.0 + 0.5);
        const double p = ease(easing, time / 8192.0);
        size_t k = 0;
        while (k + 2 < stops.size() && p >= stops[k + 1].pos) ++k;
        const Stop &a = stops[k], &b = stops[k + 1];
        const double lp = b.pos == a.pos ? 0.0 : (p - a.pos) / (b.pos - a.pos);
        for (int c = 0; c < 4; ++c) {
            int v = int(a.c[c] + (b.c[c] - a.c[c]) * lp);
            v = std::min(255, std::max(0, v));
            out[size_t(i) * 4 + c] = static_cast<unsigned char>(std::max(0, v - 3));
        }
    }
    return out;
}

// raw TF text file: 4096 whitespace-separated integers (mainwindow.cpp:680-719)
std::vector<unsigned char> tff_from_raw_file(const std::string &path)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("Could not open transfer function file " + path);
    std::vector<unsigned char> out;
    double v;
    while (in >> v) out.push_back(static_cast<unsigned char>(std::min(255.0, std::max(0.0, v))));
    if (out.empty() || out.size() % 4) throw std::runtime_error("Invalid transfer function file " + path);
    return out;
}

// `.tff` gradient-stop file (MainWindow::readTff, mainwindow.cpp:583-620): `pos r g b a` per line
std::vector<unsigned char> tff_from_stops_file(const std::string &path, const std::string &easing)
{
    std::ifstream in(path);
    if (!in) throw std::invalid_argument("Could not open transfer function file " + path);
    std::vector<Stop> stops;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        double v[5];
        int n = 0;
        while (n < 5 && (ls >> v[n])) ++n;
        if (n < 5) continue;
        Stop st;
        st.pos = v[0];
        for (int c = 0; c < 4; ++c) st.c[c] = int(v[1 + c]);
        stops.push_back(st);
    }
    if (stops.empty()) throw std::invalid_argument("Empty transfer function file.");
    return tff_from_stops(stops, 1024, easing);
}

// The GUI's JSON state (MainWindow::loadCamState, mainwindow.cpp:374-410; VolumeRenderWidget::read,
// volumerenderwidget.cpp:1457-1480): a flat object of strings, numbers and booleans.
struct CamState {
    bool has_rot = false, has_tr = false;
    double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 2};
    std::map<std::string, double> num;
    std::map<std::string, bool> flag;
};

CamState read_cam_state(const std::string &path)
{
    std::ifstream in(path);
    if (!in) throw std::invalid_argument("Couldn't open state file " + path);
    std::string js((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    CamState st;
    size_t i = 0;
    auto skip = [&]() { while (i < js.size() && std::isspace((unsigned char)js[i])) ++i; };
    auto str = [&]() {
        std::string out;
        ++i;   // opening quote
        while (i < js.size() && js[i] != '"') {
            if (js[i] == '\\' && i + 1 < js.size()) ++i;
            out += js[i++];
        }
        ++i;
        return out;
    };
    skip();
    if (i >= js.size() || js[i] != '{') throw std::invalid_argument("Invalid state file " + path);
    ++i;
    for (;;) {
        skip();
        if (i >= js.size() || js[i] == '}') break;
        if (js[i] == ',') { ++i; continue; }
        if (js[i] != '"') throw std::invalid_argument("Invalid state file " + path);
        const std::string key = str();
        skip();
        if (i < js.size() && js[i] == ':') ++i;
        skip();
        if (i < js.size() && js[i] == '"') {
            std::istringstream vs(str());
            if (key == "camRotation") { st.has_rot = bool(vs >> st.q[0] >> st.q[1] >> st.q[2] >> st.q[3]); }
            else if (key == "camTranslation") { st.has_tr = bool(vs >> st.t[0] >> st.t[1] >> st.t[2]); }
        } else if (js.compare(i, 4, "true") == 0) { st.flag[key] = true; i += 4; }
        else if (js.compare(i, 5, "false") == 0) { st.flag[key] = false; i += 5; }
        else {
            size_t used = 0;
            st.num[key] = std::stod(js.substr(i), &used);
            i += used;
        }
    }
    return st;
}

// updateViewMatrix (volumerenderwidget.cpp:1079-1098): M = R(q) T(t) S(t.z), row-major
std::array<float, 16> view_matrix(const double q[4], const double t[3])
{
    double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                      {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                      {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    std::array<float, 16> m{};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[r * 4 + c] = float(R[r][c] * t[2]);
        m[r * 4 + 3] = float(R[r][0] * t[0] + R[r][1] * t[1] + R[r][2] * t[2]);
    }
    m[15] = 1.f;
    return m;
}

// ---- camera paths the GUI records, replayed one frame per camera entry (frontend.py read_view_record,
// read_interaction_log, orbit_views: the same parse and the same double operations, float for float)
struct PathEvent {
    enum Kind { CAMERA, TRANSFER_FUNCTION, TIMESTEP } kind;
    explicit PathEvent(Kind k) : kind(k) {}
    std::array<float, 16> view{};
    std::vector<unsigned char> tff;
    int timestep = 0;
};

// QString::toFloat: the recorded numbers are read back as floats
double parse_f32(const std::string &tok)
{
    size_t used = 0;
    const double v = std::stod(tok, &used);
    if (used != tok.size()) throw std::invalid_argument("not a number: " + tok);
    return double(float(v));
}

std::vector<std::string> split_ws(const std::string &s)
{
    std::istringstream in(s);
    std::vector<std::string> out;
    std::string tok;
    while (in >> tok) out.push_back(tok);
    return out;
}

// `;`-separated entries of whitespace-separated numbers (recordViewConfig appends `w x y z; ` per view)
std::vector<std::vector<std::string>> read_entries(const std::string &path)
{
    std::ifstream in(path);
    if (!in) throw std::invalid_argument("Could not open view record " + path);
    std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>()), part;
    std::vector<std::vector<std::string>> out;
    std::istringstream ss(all);
    while (std::getline(ss, part, ';')) {
        std::vector<std::string> e = split_ws(part);
        if (!e.empty()) out.push_back(e);
    }
    return out;
}

// recordViewConfig (volumerenderwidget.cpp:1030-1048): <prefix>_quat.txt and <prefix>_trans.txt
std::vector<PathEvent> read_view_record(const std::string &prefix)
{
    const auto quats = read_entries(prefix + "_quat.txt"), trans = read_entries(prefix + "_trans.txt");
    if (quats.size() != trans.size())
        throw std::invalid_argument("view record " + prefix + ": " + std::to_string(quats.size()) + " rotations but " +
                                    std::to_string(trans.size()) + " translations");
    if (quats.empty()) throw std::invalid_argument("view record " + prefix + ": no views");
    std::vector<PathEvent> out;
    for (size_t i = 0; i < quats.size(); ++i) {
        if (quats[i].size() != 4 || trans[i].size() != 3)
            throw std::invalid_argument("view record " + prefix + ": malformed entry " + std::to_string(i));
        double q[4], t[3];
        for (int k = 0; k < 4; ++k) q[k] = parse_f32(quats[i][size_t(k)]);
        for (int k = 0; k < 3; ++k) t[k] = parse_f32(trans[i][size_t(k)]);
        PathEvent e(PathEvent::CAMERA);
        e.view = view_matrix(q, t);
        out.push_back(e);
    }
    return out;
}

// the interaction log (toggleInteractionLogging / logInteraction, volumerenderwidget.cpp:313-358), parsed as
// setSequenceStep (:364-408) does: the payload follows the last `;`; tffInterpolation lines are checked and dropped
// (the logged tables are already sampled)
std::vector<PathEvent> read_interaction_log(const std::string &path)
{
    std::ifstream in(path);
    if (!in) throw std::invalid_argument("Invalid file name for interaction log: " + path);
    std::vector<PathEvent> out;
    std::string line;
    bool any_camera = false;
    for (size_t n = 1; std::getline(in, line); ++n) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (split_ws(line).empty()) continue;
        const size_t pos = line.rfind(';');
        const std::string where = "interaction log " + path + ", line " + std::to_string(n) + ": ";
        if (pos == std::string::npos) throw std::invalid_argument(where + "no ';'");
        const std::string payload = pos + 2 <= line.size() ? line.substr(pos + 2) : std::string();
        try {
            if (line.find("camera") != std::string::npos) {
                std::string p = payload;
                p.erase(std::remove(p.begin(), p.end(), ','), p.end());
                const std::vector<std::string> tok = split_ws(p);
                if (tok.size() != 7) throw std::invalid_argument("a camera entry is 7 numbers");
                double q[4], t[3];
                for (int k = 0; k < 4; ++k) q[k] = parse_f32(tok[size_t(k)]);
                for (int k = 0; k < 3; ++k) t[k] = parse_f32(tok[size_t(4 + k)]);
                PathEvent e(PathEvent::CAMERA);
                e.view = view_matrix(q, t);
                out.push_back(e);
                any_camera = true;
            } else if (line.find("timestep") != std::string::npos) {
                const std::vector<std::string> tok = split_ws(payload);
                size_t used = 0;
                if (tok.size() != 1) throw std::invalid_argument("a timestep is one integer");
                PathEvent e(PathEvent::TIMESTEP);
                e.timestep = std::stoi(tok[0], &used);
                if (used != tok[0].size()) throw std::invalid_argument("a timestep is one integer");
                out.push_back(e);
            } else if (line.find("transferFunction") != std::string::npos) {
                PathEvent e(PathEvent::TRANSFER_FUNCTION);
                for (const std::string &tok : split_ws(payload)) {
                    size_t used = 0;
                    const long v = std::stol(tok, &used);
                    if (used != tok.size()) throw std::invalid_argument("not an integer: " + tok);
                    e.tff.push_back(static_cast<unsigned char>(v & 0xff));
                }
                if (e.tff.empty() || e.tff.size() % 4) throw std::invalid_argument("a transfer function is RGBA8 entries");
                out.push_back(e);
            } else if (line.find("tffInterpolation") != std::string::npos) {
                const std::vector<std::string> tok = split_ws(payload);
                if (tok.size() != 1 || (tok[0] != "linear" && tok[0] != "quad" && tok[0] != "cubic"))
                    throw std::invalid_argument("unknown interpolation");
            } else {
                throw std::invalid_argument("unknown event");
            }
        } catch (const std::logic_error &e) {   // (std::stod / stoi / stol throw invalid_argument or out_of_range)
            throw std::invalid_argument(where + e.what());
        }
    }
    if (!any_camera) throw std::invalid_argument("interaction log " + path + ": no camera entries");
    return out;
}

// a turntable: n views over 360 degrees about `axis`, each step composed onto the start rotation as the GUI's mouse
// rotation does (_rotQuat * step, volumerenderwidget.cpp:1115); QQuaternion::fromAxisAndAngle as frontend.py states it
std::vector<PathEvent> orbit_views(const double axis[3], int n, const double q[4], const double t[3])
{
    const double l = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    const double a[3] = {axis[0] / l, axis[1] / l, axis[2] / l};
    std::vector<PathEvent> out;
    for (int k = 0; k < n; ++k) {
        const double h = (360.0 * k / n * (M_PI / 180.0)) / 2.0, s = std::sin(h);
        const double p[4] = {std::cos(h), a[0] * s, a[1] * s, a[2] * s};
        const double r[4] = {q[0] * p[0] - q[1] * p[1] - q[2] * p[2] - q[3] * p[3],
                             q[0] * p[1] + q[1] * p[0] + q[2] * p[3] - q[3] * p[2],
                             q[0] * p[2] - q[1] * p[3] + q[2] * p[0] + q[3] * p[1],
                             q[0] * p[3] + q[1] * p[2] - q[2] * p[1] + q[3] * p[0]};
        PathEvent e(PathEvent::CAMERA);
        e.view = view_matrix(r, t);
        out.push_back(e);
    }
    return out;
}

// A path cut where its transfer function or time step changes: the frames of a segment share both
struct PathSegment {
    std::vector<std::array<float, 16>> views;
    const std::vector<unsigned char> *tff = nullptr;   // the table in force (nullptr: the options' table)
    int timestep = -1;                                 // the time step in force (-1: the first)
};

std::vector<PathSegment> path_segments(const std::vector<PathEvent> &ev)
{
    std::vector<PathSegment> segs(1);
    for (const PathEvent &e : ev) {
        if (e.kind == PathEvent::CAMERA) { segs.back().views.push_back(e.view); continue; }
        if (!segs.back().views.empty()) {
            PathSegment next;
            next.tff = segs.back().tff;
            next.timestep = segs.back().timestep;
            segs.push_back(next);
        }
        if (e.kind == PathEvent::TRANSFER_FUNCTION) segs.back().tff = &e.tff;
        else segs.back().timestep = e.timestep;
    }
    if (segs.back().views.empty()) segs.pop_back();   // (changes after the last camera entry render nothing)
    return segs;
}

void write_ppm(const std::string &path, const std::vector<float> &rgba, size_t w, size_t h)
{
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << w << " " << h << "\n255\n";
    std::vector<unsigned char> row(w * 3);
    for (size_t y = 0; y < h; ++y) {
        for (size_t x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                float v = rgba[(y * w + x) * 4 + c];
                row[x * 3 + c] = static_cast<unsigned char>(std::lround(std::min(1.f, std::max(0.f, v)) * 255.f));
            }
        f.write(reinterpret_cast<const char *>(row.data()), std::streamsize(row.size()));
    }
}

// --rgba8: PREFIX.ppm from the 8-bit pixels, their R, G, B bytes as they are
void write_ppm_rgba8(const std::string &path, const std::vector<unsigned char> &rgba8, size_t w, size_t h)
{
    std::ofstream f(path, std::ios::binary);
    f << "P6\n" << w << " " << h << "\n255\n";
    std::vector<unsigned char> rgb(w * h * 3);
    for (size_t i = 0; i < w * h; ++i)
        for (size_t c = 0; c < 3; ++c) rgb[i * 3 + c] = rgba8[i * 4 + c];
    f.write(reinterpret_cast<const char *>(rgb.data()), std::streamsize(rgb.size()));
}

// --rgba8: PREFIX.rgba.u8 (the last frame), PREFIX.frames.rgba.u8 (all frames of a multi-frame run) and PREFIX.ppm
void write_rgba8(const std::string &out, const std::vector<unsigned char> &frame8, const std::vector<unsigned char> &all8,
                 size_t w, size_t h)
{
    if (!all8.empty()) {
        std::ofstream af(out + ".frames.rgba.u8", std::ios::binary);
        af.write(reinterpret_cast<const char *>(all8.data()), std::streamsize(all8.size()));
    }
    std::ofstream raw(out + ".rgba.u8", std::ios::binary);
    raw.write(reinterpret_cast<const char *>(frame8.data()), std::streamsize(frame8.size()));
    write_ppm_rgba8(out + ".ppm", frame8, w, h);
}

// --stats: the counts, the moments when they were asked for (mean and std: population, in double, from sum and
// sum_sq over the non-NaN voxels) and the table, rows of vBins counts by ascending gradient bin
bool write_stats_json(const std::string &path, const VolumeRenderCL::stats_params &sp, const VolumeRenderCL::volume_stats &st)
{
    std::ofstream f(path);
    char num[64];
    auto real = [&](double v) -> std::string {   // (JSON has no inf or nan: as strings)
        if (!std::isfinite(v)) return v != v ? "\"nan\"" : v > 0 ? "\"inf\"" : "\"-inf\"";
        std::snprintf(num, sizeof num, "%.17g", v);
        return num;
    };
    f << "{\"bins\": [" << sp.vBins << ", " << sp.gBins << "], \"window\": [" << real(sp.vLo) << ", " << real(sp.vHi) << ", "
      << real(sp.gHi) << "],\n \"voxels\": " << st.voxels << ", \"nan\": " << st.nan << ", \"below\": " << st.below
      << ", \"above\": " << st.above << ", \"gradient_nan\": " << st.gradientNan << ", \"binned\": " << st.binned;
    if (sp.moments) {
        const double n = double(st.voxels - st.nan), mean = n > 0 ? st.sum / n : 0.0;
        const double var = n > 0 ? std::max(0.0, st.sumSq / n - mean * mean) : 0.0;
        f << ",\n \"min\": " << real(st.min) << ", \"max\": " << real(st.max) << ", \"sum\": " << real(st.sum)
          << ", \"sum_sq\": " << real(st.sumSq) << ", \"mean\": " << real(mean) << ", \"std\": " << real(std::sqrt(var));
    }
    f << ",\n \"hist\": [";
    for (unsigned j = 0; j < sp.gBins; ++j) {
        f << (j ? ",\n  [" : "[");
        for (unsigned i = 0; i < sp.vBins; ++i) f << (i ? ", " : "") << st.hist[size_t(j) * sp.vBins + i];
        f << "]";
    }
    f << "]}\n";
    f.flush();
    return bool(f);
}

// the --filter and --morph steps, in command-line order
void apply_volume_steps(VolumeRenderCL &vr, const Options &o)
{
    for (const VolumeStep &step : o.steps) {
        if (step.morph) {
            vr.morphVolume(o.morphs.at(step.index).params, vr.getTimestep());
            continue;
        }
        const FilterSpec &fs = o.filters.at(step.index);
        if (fs.kind == FilterSpec::GAUSS) vr.gaussianFilter(fs.sigma, fs.radius);
        else if (fs.kind == FilterSpec::MEDIAN) vr.medianFilter();
        else vr.filterVolume(fs.taps, vr.getTimestep());
    }
}

void hip_ok(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string("ERROR: ") + what + " (" + hipGetErrorString(e) + ")");
}

// PREFIX.frames.rgba.f32 (all frames, where a run keeps them), PREFIX.rgba.f32 (the last frame) and PREFIX.ppm
void write_frames(const std::string &out, const std::vector<float> &frame, const std::vector<float> &all_frames, size_t w, size_t h)
{
    if (!all_frames.empty()) {
        std::ofstream af(out + ".frames.rgba.f32", std::ios::binary);
        af.write(reinterpret_cast<const char *>(all_frames.data()), std::streamsize(all_frames.size() * sizeof(float)));
    }
    std::ofstream raw(out + ".rgba.f32", std::ios::binary);
    raw.write(reinterpret_cast<const char *>(frame.data()), std::streamsize(frame.size() * sizeof(float)));
    write_ppm(out + ".ppm", frame, w, h);
}

// the transfer-function table the options select (TransferFunctionWidget's default stops,
// transferfunctionwidget.cpp:338-346, unless a file is given)
std::vector<unsigned char> make_table(const Options::Render &rn)
{
    return !rn.tf_stops.empty() ? tff_from_stops_file(rn.tf_stops, rn.tf_easing)
           : rn.tf == "default" ? tff_from_stops({{0.0, {0, 0, 0, 0}}, {0.1, {125, 125, 125, 0}}, {1.0, {0, 0, 0, 255}}},
                                                 1024, rn.tf_easing)
                                : tff_from_raw_file(rn.tf);
}

std::array<float, 16> the_view(const Options::View &vw) { return vw.have_view ? vw.view : view_matrix(vw.q, vw.tr); }

// --camera-path / --orbit: the path's events and its segments (which point into the events: not to be copied)
struct CameraPath {
    std::vector<PathEvent> events;
    std::vector<PathSegment> segs;
    bool used() const { return !events.empty(); }
};

// What needs no GPU, between validate() and the first renderer (the order is the one stated above validate(),
// vrhip_cli.cpp): the camera path is read, --dump-views and --dump-tf write their file and end the run.  A path
// replaces --frames by one independent frame per camera entry.  Returns the exit status where the run ends here, -1
// where it goes on.
int front_end(Options &o, CameraPath &path)
{
    Options::View &vw = o.view;
    if (vw.have_path_arg) {
        std::ifstream probe(vw.camera_path + "_quat.txt");
        path.events = probe ? read_view_record(vw.camera_path) : read_interaction_log(vw.camera_path);
    } else if (vw.have_orbit) {
        if (!vw.state_file.empty()) {   // (the orbit starts from the camera the options select, --state included)
            const CamState st = read_cam_state(vw.state_file);
            if (st.has_rot) for (int k = 0; k < 4; ++k) vw.q[k] = st.q[k];
            if (st.has_tr) for (int k = 0; k < 3; ++k) vw.tr[k] = st.t[k];
        }
        path.events = orbit_views(vw.orbit_axis, vw.orbit_n, vw.q, vw.tr);
    }
    if (!o.out.dump_views.empty()) {   // front-end formula only
        std::ofstream f(o.out.dump_views, std::ios::binary);
        for (const PathEvent &e : path.events)
            if (e.kind == PathEvent::CAMERA)
                f.write(reinterpret_cast<const char *>(e.view.data()), std::streamsize(16 * sizeof(float)));
        return f ? 0 : 1;
    }
    if (path.used()) {
        path.segs = path_segments(path.events);
        o.batch.frames = 0;
        for (const PathSegment &sg : path.segs) o.batch.frames += int(sg.views.size());
        o.batch.independent = true;
        if (o.tech.pathtrace || o.render.img_ess) {
            std::cerr << "--camera-path / --orbit: ray caster only, no image-order ESS" << std::endl;
            return 1;
        }
    }
    validate_easing(o);
    if (!o.out.dump_tf.empty()) {   // front-end formula only
        const std::vector<unsigned char> table = make_table(o.render);
        std::ofstream f(o.out.dump_tf, std::ios::binary);
        f.write(reinterpret_cast<const char *>(table.data()), std::streamsize(table.size()));
        return f ? 0 : 1;
    }
    validate_source_and_output(o);
    return -1;
}

// a device, and the volume of the options on it
void open_volume(VolumeRenderCL &vr, const Options &o, int dev)
{
    vr.initialize(false, false, VENDOR_ANY, std::to_string(dev));
    if (!o.volume.dat.empty()) {
        DatRawReader::Properties p;
        p.dat_file_name = o.volume.dat;
        vr.setDeviceIngest(o.volume.device_ingest);
        vr.loadVolumeData(p);
    } else {
        DatRawReader::data_format f = o.volume.synth_fmt == "USHORT" ? DatRawReader::USHORT
                                      : o.volume.synth_fmt == "FLOAT" ? DatRawReader::FLOAT : DatRawReader::UCHAR;
        vr.loadSyntheticVolume(o.volume.synth_kind, o.volume.synth_n, f);
    }
}

// --mesh and --stats: the volume, the ESS switch, the time step and the filters, nothing else
void setup_volume_only(VolumeRenderCL &vr, const Options &o)
{
    open_volume(vr, o, o.ranks.device);
    vr.setObjEss(o.render.ess);
    if (o.volume.have_timestep) vr.setTimestep(size_t(o.volume.timestep));
    apply_volume_steps(vr, o);
}

// Everything the front end sets on a renderer; returns false when there is no frame to render.  A --state file
// overrides the options it names, as the GUI's widgets would forward them after loadCamState -- for this renderer and
// for what follows (with several ranks the file is applied once per renderer, its imgResFactor each time).
bool setup_renderer(VolumeRenderCL &vr, Options &o, int dev)
{
    Options::View &vw = o.view;
    Options::Render &rn = o.render;
    open_volume(vr, o, dev);
    if (!o.steps.empty()) {
        vr.setObjEss(rn.ess);
        apply_volume_steps(vr, o);
    }
    if (o.volume.downsample) {   // volumeDownsampling (volumerendercl.cpp:238-341) and nothing else
        const std::string base = vr.volumeDownsampling(0, o.volume.downsample);
        std::printf("{\"downsampled\": \"%s\"}\n", base.c_str());
        return false;
    }
    bool use_ao = rn.ao, show_box = rn.show_ess;
    if (!vw.state_file.empty()) {
        const CamState st = read_cam_state(vw.state_file);
        if (st.has_rot) for (int k = 0; k < 4; ++k) vw.q[k] = st.q[k];
        if (st.has_tr) for (int k = 0; k < 3; ++k) vw.tr[k] = st.t[k];
        if (st.num.count("rayStepSize")) rn.rate = st.num.at("rayStepSize");
        if (st.num.count("imgResFactor")) {
            vw.W = size_t(std::floor(double(vw.W) * st.num.at("imgResFactor")));
            vw.H = size_t(std::floor(double(vw.H) * st.num.at("imgResFactor")));
        }
        if (st.flag.count("useLerp")) rn.linear = st.flag.at("useLerp");
        if (st.flag.count("useOrtho")) rn.ortho = st.flag.at("useOrtho");
        if (st.flag.count("showContours")) rn.contours = st.flag.at("showContours");
        if (st.flag.count("useAerial")) rn.aerial = st.flag.at("useAerial");
        if (st.flag.count("useAO")) use_ao = st.flag.at("useAO");
        if (st.flag.count("showBox")) show_box = st.flag.at("showBox");
    }
    std::vector<unsigned char> table = make_table(rn);
    vr.setTransferFunction(table);
    vr.setIllumination(rn.illum);
    vr.setObjEss(rn.ess);
    vr.setCamOrtho(rn.ortho);
    vr.setLinearInterpolation(rn.linear);
    vr.setUseGradient(rn.gradient_bg);
    vr.setContours(rn.contours);
    vr.setAerial(rn.aerial);
    vr.setAmbientOcclusion(use_ao);
    if (show_box) vr.setShowESS(true);
    if (!rn.env_file.empty()) vr.createEnvironmentMap(rn.env_file);
    if (rn.img_ess) vr.setImgEss(true);   // state carried from frame to frame (--frames N)
    vr.setBackground(rn.bg);
    vr.updateSamplingRate(rn.rate);
    if (o.tech.pathtrace) {
        vr.setTechnique(VolumeRenderCL::TECH_PATHTRACE);
        vr.setExtinction(o.tech.extinction);
    }
    if (o.tech.mip) vr.setTechnique(VolumeRenderCL::TECH_MIP);
    if (o.tech.preint) vr.setTechnique(VolumeRenderCL::TECH_PREINT);
    if (o.tech.iso) {
        vr.setTechnique(VolumeRenderCL::TECH_ISO);
        vr.setIsoValue(float(o.tech.iso_value));
        vr.setIsoRefinement(unsigned(o.tech.iso_refine));
    }
    if (o.tf2d.any()) {
        const Options::Tf2d &t2 = o.tf2d;
        std::vector<unsigned char> table2;
        unsigned nv = unsigned(t2.nv);
        if (t2.table) {
            std::ifstream f(t2.file, std::ios::binary);
            table2.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
            if (!f.good() && !f.eof()) table2.clear();
            if (table2.size() != size_t(4) * size_t(t2.nv) * size_t(t2.ng))
                throw std::runtime_error("--tf2d: " + t2.file + " does not hold NV * NG RGBA8 entries");
        } else {
            nv = unsigned(table.size() / 4);
            table2 = VolumeRenderCL::rampTransferFunction2D(table, unsigned(t2.ng), float(t2.ghi), float(t2.g0), float(t2.g1));
        }
        vr.setTechnique(VolumeRenderCL::TECH_TF2D);
        vr.setTransferFunction2D(table2, nv, unsigned(t2.ng), float(t2.ghi));
    }
    if (rn.pin) vr.setSeed(rn.seed);
    vr.updateOutputImg(vw.W, vw.H, 0);
    vr.updateView(the_view(vw));
    return true;
}

// what segment s of the camera path has in force (transfer function, time step), on renderer vr
void apply_segment(VolumeRenderCL &vr, const Options &o, const CameraPath &path, size_t s)
{
    std::vector<unsigned char> table = path.segs[s].tff ? *path.segs[s].tff : make_table(o.render);
    vr.setTransferFunction(table);
    vr.setTimestep(size_t(path.segs[s].timestep < 0 ? 0 : path.segs[s].timestep));
}

// ---- the isosurface as a file (VolumeRenderCL::extractIsosurface)
void run_mesh(VolumeRenderCL &vr, const Options &o)
{
    const Options::Mesh &me = o.mesh;
    VolumeRenderCL::mesh_region region;
    if (me.have_region)
        for (size_t k = 0; k < 3; ++k) { region.lo[k] = unsigned(me.region[k]); region.hi[k] = unsigned(me.region[3 + k]); }
    if (me.indexed) {
        const VolumeRenderCL::welded_mesh im = vr.extractIsosurfaceIndexed(float(me.iso), me.normals, region);
        const size_t vertices = VolumeRenderCL::writePly(me.file, im);
        std::printf("{\"device\": \"%s\", \"mesh\": \"%s\", \"iso\": %.9g, \"triangles\": %zu, \"vertices\": %zu, "
                    "\"indexed\": true}\n",
                    vr.getCurrentDeviceName().c_str(), me.file.c_str(), me.iso, im.indices.size() / 3, vertices);
        return;
    }
    const VolumeRenderCL::iso_mesh m = vr.extractIsosurface(float(me.iso), me.normals, region);
    const size_t triangles = m.positions.size() / 9;
    if (me.ext() == ".ply") {
        const size_t vertices = VolumeRenderCL::writePly(me.file, m.positions, m.normals);
        std::printf("{\"device\": \"%s\", \"mesh\": \"%s\", \"iso\": %.9g, \"triangles\": %zu, \"vertices\": %zu}\n",
                    vr.getCurrentDeviceName().c_str(), me.file.c_str(), me.iso, triangles, vertices);
    } else {
        VolumeRenderCL::writeStl(me.file, m.positions);
        std::printf("{\"device\": \"%s\", \"mesh\": \"%s\", \"iso\": %.9g, \"triangles\": %zu}\n",
                    vr.getCurrentDeviceName().c_str(), me.file.c_str(), me.iso, triangles);
    }
}

// ---- what is in the volume (VolumeRenderCL::volumeStatistics)
void run_stats(VolumeRenderCL &vr, const Options &o)
{
    const Options::Stats &so = o.stats;
    VolumeRenderCL::stats_params sp;
    sp.vBins = unsigned(so.bins[0]);
    sp.gBins = unsigned(so.bins[1]);
    sp.vLo = float(so.window[0]);
    sp.vHi = float(so.window[1]);
    sp.gHi = float(so.window[2]);
    sp.moments = so.moments;
    if (so.have_region)
        for (size_t k = 0; k < 3; ++k) { sp.region.lo[k] = unsigned(so.region[k]); sp.region.hi[k] = unsigned(so.region[3 + k]); }
    const VolumeRenderCL::volume_stats st = vr.volumeStatistics(sp);
    if (!write_stats_json(so.file, sp, st)) throw std::runtime_error("cannot write " + so.file);
    if (!so.hist_file.empty()) {
        std::ofstream f(so.hist_file, std::ios::binary);
        f.write(reinterpret_cast<const char *>(st.hist.data()), std::streamsize(st.hist.size() * sizeof(uint64_t)));
        if (!f) throw std::runtime_error("cannot write " + so.hist_file);
    }
    std::printf("{\"device\": \"%s\", \"stats\": \"%s\", \"voxels\": %llu, \"binned\": %llu}\n",
                vr.getCurrentDeviceName().c_str(), so.file.c_str(), (unsigned long long)st.voxels,
                (unsigned long long)st.binned);
}

// the slices the options ask for: one plane or slab, or --slice-stack of them
std::vector<VolumeRenderCL::slice_params> make_slices(const Options::Slice &sl)
{
    const VolumeRenderCL::slice_mode mode = sl.slab_mode == "min" ? VolumeRenderCL::SLICE_MIN
                                            : sl.slab_mode == "mean" ? VolumeRenderCL::SLICE_MEAN : VolumeRenderCL::SLICE_MAX;
    const VolumeRenderCL::slice_output output = sl.value ? VolumeRenderCL::SLICE_VALUE : VolumeRenderCL::SLICE_TF;
    VolumeRenderCL::slice_params sp;
    double nrm[3] = {0, 0, 0};   // the unit normal
    if (sl.have_axis) {
        sp = VolumeRenderCL::axisSlice(sl.axis, float(sl.pos), float(sl.slab_t), unsigned(sl.slab_n), mode, output);
        nrm[sl.axis] = 1.0;
    } else {
        std::memset(&sp, 0, sizeof sp);
        const double *u = sl.vec + 3, *v = sl.vec + 6;
        const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double l = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        for (int k = 0; k < 3; ++k) {
            nrm[k] = l > 0.0 ? c[k] / l : 0.0;
            sp.origin[k] = float(sl.vec[k]);
            sp.u[k] = float(u[k]);
            sp.v[k] = float(v[k]);
            sp.w[k] = float(sl.slab_t * nrm[k]);
        }
        sp.samples = unsigned(sl.slab_n);
        sp.mode = unsigned(mode);
        sp.output = unsigned(output);
    }
    if (!sl.have_stack) return {sp};
    // spanning the box along the normal: centred where the normal's line through the box centre meets the
    // plane's parallel through it, over the box's extent along the normal
    const double d = sp.origin[0] * nrm[0] + sp.origin[1] * nrm[1] + sp.origin[2] * nrm[2];
    VolumeRenderCL::slice_params base = sp;
    for (int k = 0; k < 3; ++k) base.origin[k] = float(double(sp.origin[k]) - d * nrm[k]);
    const double span = 2.0 * (std::fabs(nrm[0]) + std::fabs(nrm[1]) + std::fabs(nrm[2]));
    return VolumeRenderCL::sliceStack(base, unsigned(sl.stack_n), float(span));
}

// ---- slice views (VolumeRenderCL::renderSlices): the slices of the options in calls of <= 64, written like the
// frames of --orbit
void run_slices(VolumeRenderCL &vr, const Options &o)
{
    const size_t W = o.view.W, H = o.view.H;
    const bool rgba8 = o.out.rgba8;
    const std::vector<VolumeRenderCL::slice_params> slices = make_slices(o.slice);
    std::vector<float> all_frames;
    std::vector<unsigned char> all_frames8;
    hip_ok(hipSetDevice(o.ranks.device), "hipSetDevice");
    const size_t chunk = std::min<size_t>(64, slices.size()), px = W * H * 4;
    float *dev = nullptr;
    hip_ok(hipMalloc(reinterpret_cast<void **>(&dev), chunk * px * sizeof(float)), "hipMalloc slices");
    all_frames.resize(slices.size() * px);
    if (rgba8) all_frames8.resize(slices.size() * px);
    for (size_t at = 0; at < slices.size(); at += chunk) {
        const size_t n = std::min(chunk, slices.size() - at);
        const std::vector<VolumeRenderCL::slice_params> part(slices.begin() + long(at), slices.begin() + long(at + n));
        if (rgba8) vr.renderSlicesRGBA8(W, H, part, dev, all_frames8.data() + at * px, false);
        else vr.renderSlices(W, H, part, dev);
        hip_ok(hipStreamSynchronize(static_cast<hipStream_t>(vr.stream())), "hipStreamSynchronize");
        hip_ok(hipMemcpy(all_frames.data() + at * px, dev, n * px * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    }
    (void)hipFree(dev);
    const std::vector<float> frame(all_frames.end() - long(px), all_frames.end());
    write_frames(o.out.prefix, frame, all_frames, W, H);
    if (rgba8) {
        const std::vector<unsigned char> frame8(all_frames8.end() - long(px), all_frames8.end());
        write_rgba8(o.out.prefix, frame8, all_frames8, W, H);
    }
    auto res = vr.getResolution();
    std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, \"slices\": %zu, "
                "\"samples\": %d, \"mode\": \"%s\", \"output\": \"%s\", \"out\": \"%s.rgba.f32\"}\n",
                vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, slices.size(), o.slice.slab_n,
                o.slice.slab_mode.c_str(), o.slice.value ? "value" : "tf", o.out.prefix.c_str());
}

// ---- a depth image (VolumeRenderCL::renderDepth) of the options' camera
void run_depth(VolumeRenderCL &vr, const Options &o)
{
    const Options::Depth &de = o.depth;
    const std::string &out = o.out.prefix;
    const VolumeRenderCL::depth_mode mode = de.mode == "max" ? VolumeRenderCL::DEPTH_MAX
                                            : de.mode == "opacity" ? VolumeRenderCL::DEPTH_OPACITY : VolumeRenderCL::DEPTH_ISO;
    VolumeRenderCL::depth_image d;
    std::array<unsigned int, 4> rect{{0, 0, 0, 0}};
    if (de.have_rect) for (size_t k = 0; k < 4; ++k) rect[k] = unsigned(de.rect[k]);
    vr.renderDepth(o.view.W, o.view.H, mode, float(de.threshold), d, unsigned(de.refine), rect);
    const size_t n = d.width * d.height;
    size_t hits = 0;
    float t_min = std::numeric_limits<float>::infinity(), t_max = -std::numeric_limits<float>::infinity();
    for (size_t i = 0; i < n; ++i) {
        if (d.kind[i] != VolumeRenderCL::DEPTH_HIT) continue;
        ++hits;
        t_min = std::min(t_min, d.xyzt[4 * i + 3]);
        t_max = std::max(t_max, d.xyzt[4 * i + 3]);
    }
    // grey: near = bright; finite t scaled between its minimum and maximum, non-hits black
    std::vector<float> frame(n * 4, 0.f);
    for (size_t i = 0; i < n; ++i) {
        frame[4 * i + 3] = 1.f;
        if (d.kind[i] != VolumeRenderCL::DEPTH_HIT) continue;
        const float g = t_max > t_min ? 1.f - (d.xyzt[4 * i + 3] - t_min) / (t_max - t_min) : 1.f;
        frame[4 * i] = frame[4 * i + 1] = frame[4 * i + 2] = g;
    }
    std::ofstream fx(out + ".depth.f32", std::ios::binary);
    fx.write(reinterpret_cast<const char *>(d.xyzt.data()), std::streamsize(d.xyzt.size() * sizeof(float)));
    std::ofstream fa(out + ".depth.aux.f32", std::ios::binary);
    fa.write(reinterpret_cast<const char *>(d.aux.data()), std::streamsize(d.aux.size() * sizeof(float)));
    std::ofstream fk(out + ".depth.kind.u8", std::ios::binary);
    fk.write(reinterpret_cast<const char *>(d.kind.data()), std::streamsize(d.kind.size()));
    write_ppm(out + ".ppm", frame, d.width, d.height);
    char t_lo[32] = "null", t_hi[32] = "null";
    if (hits) {
        std::snprintf(t_lo, sizeof t_lo, "%.9g", double(t_min));
        std::snprintf(t_hi, sizeof t_hi, "%.9g", double(t_max));
    }
    auto res = vr.getResolution();
    std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                "\"rect\": [%u, %u, %zu, %zu], \"mode\": \"%s\", \"hits\": %zu, \"t_min\": %s, \"t_max\": %s, "
                "\"out\": \"%s.depth.f32\"}\n",
                vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], o.view.W, o.view.H, rect[0], rect[1], d.width, d.height,
                de.mode.c_str(), hits, t_lo, t_hi, out.c_str());
}

int rank_device(const Options::Ranks &rk, int r) { return rk.loopback ? rk.device : rk.device + r; }

// --ranks with --frames-per-launch, the throughput path: K independent frames per exchange, one exchange in flight.
// Leaves the last batch in `frame`, every frame in `all_frames` unless --bench; returns the seconds from the first
// submit to the last assembled batch.
double run_ranks_batched(TileGather &tg, std::vector<std::unique_ptr<VolumeRenderCL>> &vrs, const Options &o, const CameraPath &path,
                         size_t K, std::vector<float> &frame, std::vector<float> &all_frames)
{
    const bool bench = o.batch.bench, use_path = path.used();
    const std::vector<PathSegment> &segs = path.segs;
    for (auto &v : vrs) { v->setRoundBudget(unsigned(o.batch.round_budget)); v->setFrameTiming(false); }
    std::vector<std::vector<unsigned int>> sets;
    std::vector<std::vector<std::array<float, 16>>> set_views;   // (camera path: per set)
    std::vector<size_t> set_seg;
    std::vector<unsigned int> seeds = vrs[0]->drawSeeds(size_t(o.batch.frames));
    if (!use_path) {
        for (size_t f0 = 0; f0 < seeds.size(); f0 += K)
            sets.emplace_back(seeds.begin() + long(f0), seeds.begin() + long(std::min(seeds.size(), f0 + K)));
    } else {   // sets of <= K frames that do not cross a change of transfer function or time step
        size_t at = 0;
        for (size_t sg = 0; sg < segs.size(); ++sg)
            for (size_t f0 = 0; f0 < segs[sg].views.size(); f0 += K) {
                const size_t f1 = std::min(segs[sg].views.size(), f0 + K);
                sets.emplace_back(seeds.begin() + long(at + f0), seeds.begin() + long(at + f1));
                set_views.emplace_back(segs[sg].views.begin() + long(f0), segs[sg].views.begin() + long(f1));
                set_seg.push_back(sg);
            }
        for (const PathSegment &sg : segs) at += sg.views.size();
    }
    if (bench) {   // untimed: buffers, work queues, cost maps, communicators
        std::mt19937 warm(20261004u);
        std::vector<unsigned int> ws(std::min(K, size_t(o.batch.frames)));
        for (int rep = 0; rep < 2; ++rep) {
            for (auto &x : ws) x = static_cast<unsigned int>(warm());
            if (use_path) tg.submitFrames(std::vector<unsigned int>(ws.begin(), ws.begin() + long(set_views[0].size())), set_views[0]);
            else tg.submitFrames(ws);
        }
        tg.collectFrames(nullptr);
        tg.collectFrames(nullptr);
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t k = 0; k < sets.size(); ++k) {
        if (use_path && (k == 0 || set_seg[k] != set_seg[k - 1])) {
            // a new transfer function / time step: the batches in flight are finished first
            while (tg.pending()) {
                tg.collectFrames(bench ? nullptr : &frame);
                if (!bench) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
            }
            for (auto &v : vrs) apply_segment(*v, o, path, set_seg[k]);
        }
        if (use_path) tg.submitFrames(sets[k], set_views[k]);
        else tg.submitFrames(sets[k]);
        if (tg.pending() == 2) {
            tg.collectFrames(bench ? nullptr : &frame);
            if (!bench) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
        }
    }
    while (tg.pending()) {
        tg.collectFrames(&frame);
        if (!bench) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
    }
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// ---- image-tile decomposition over --ranks GPUs: one renderer per rank, every one with the whole volume
// and the same settings; jitter seeds follow the same default-seeded mt19937 sequence in every renderer, frame by frame
void run_ranks(std::vector<std::unique_ptr<VolumeRenderCL>> &vrs, const Options &o, const CameraPath &path)
{
    const Options::Batch &ba = o.batch;
    const size_t W = o.view.W, H = o.view.H;
    const int frames = ba.frames;
    std::vector<VolumeRenderCL *> ptrs;
    std::vector<int> devs;
    for (size_t r = 0; r < vrs.size(); ++r) { ptrs.push_back(vrs[r].get()); devs.push_back(rank_device(o.ranks, int(r))); }
    const bool batched = ba.frames_per_launch > 0;
    if (batched && (o.tech.pathtrace || o.render.img_ess || o.render.ao))
        throw std::runtime_error("--frames-per-launch: ray caster only, no image-order ESS, no ambient occlusion");
    const size_t K = batched ? size_t(std::min(256, std::max(1, ba.frames_per_launch))) : 0;
    TileGather tg(ptrs, devs, W, H, o.ranks.tile, o.ranks.loopback, o.ranks.force_gather, o.ranks.root_share, K);
    std::vector<float> frame, all_frames;
    double secs = 0.0;
    const std::array<float, 16> view = the_view(o.view);
    if (batched) {
        secs = run_ranks_batched(tg, vrs, o, path, K, frame, all_frames);
        frame.erase(frame.begin(), frame.end() - long(W * H * 4));   // the last frame of the last batch
    } else {
        for (size_t sg = 0, in_seg = 0, f = 0; f < size_t(frames); ++f, ++in_seg) {
            const std::array<float, 16> *pv = &view;
            if (path.used()) {   // frame f of the path: frame in_seg of segment sg
                if (f == 0) for (auto &v : vrs) apply_segment(*v, o, path, 0);
                if (in_seg == path.segs[sg].views.size()) {
                    ++sg;
                    in_seg = 0;
                    for (auto &v : vrs) apply_segment(*v, o, path, sg);
                }
                pv = &path.segs[sg].views[in_seg];
            }
            if (ba.independent)
                for (auto &v : vrs) v->updateView(*pv);   // (resets the running mean: iteration 0)
            secs += tg.renderFrame(frame);
            if (ba.independent) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
        }
    }
    write_frames(o.out.prefix, frame, all_frames, W, H);
    auto res = vrs[0]->getResolution();
    const int exchanged = std::max(1, frames + (ba.bench ? 2 * int(std::min(K, size_t(frames))) : 0));
    std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                "\"frames\": %d, \"ranks\": %d, \"tile\": %zu, \"transport\": \"%s\", "
                "\"frames_per_exchange\": %zu, \"independent\": %s, \"sent_bytes_per_frame\": %.0f, "
                "\"dense_bytes_per_frame\": %.0f, \"frame_ms\": %.4f, \"ms_per_frame\": %.4f, "
                "\"clock\": \"host, first submit to last assembled batch\", \"out\": \"%s.rgba.f32\"}\n",
                vrs[0]->getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, frames, o.ranks.n, o.ranks.tile,
                tg.transport().c_str(), K, (batched || ba.independent) ? "true" : "false",
                batched ? tg.sentBytes() / exchanged : 0.0, batched ? tg.denseBytes() / exchanged : 0.0,
                secs / frames * 1e3, secs / frames * 1e3, o.out.prefix.c_str());
}

// launch sets of <= K frames per segment (one segment and no views without a path), as many per segment as a
// multiple of `mult` renderers and all of (nearly) one size
struct LaunchSet { std::vector<unsigned int> seeds; std::vector<std::array<float, 16>> views; size_t seg; };

std::vector<LaunchSet> make_sets(const CameraPath &path, const std::vector<unsigned int> &seeds, size_t K, size_t mult)
{
    std::vector<LaunchSet> sets;
    const size_t nseg = path.used() ? path.segs.size() : 1;
    size_t f0 = 0;
    for (size_t sg = 0; sg < nseg; ++sg) {
        const size_t nf = path.used() ? path.segs[sg].views.size() : seeds.size();
        size_t n_sets = (nf + K - 1) / K;
        n_sets = std::min(nf, (n_sets + mult - 1) / mult * mult);
        for (size_t i = 0; i < n_sets; ++i) {
            const size_t lo = size_t(std::llround(double(i) * double(nf) / double(n_sets)));
            const size_t hi = size_t(std::llround(double(i + 1) * double(nf) / double(n_sets)));
            if (hi <= lo) continue;
            LaunchSet ls;
            ls.seeds.assign(seeds.begin() + long(f0 + lo), seeds.begin() + long(f0 + hi));
            if (path.used()) ls.views.assign(path.segs[sg].views.begin() + long(lo), path.segs[sg].views.begin() + long(hi));
            ls.seg = sg;
            sets.push_back(ls);
        }
        f0 += nf;
    }
    return sets;
}

// ---- --frames-per-launch, the throughput path on one GPU: F renderers over one shared volume take launch sets of
// <= K independent frames in turn (what bench.py times; volumerenderwidget.cpp:464-486 is the one-frame-per-paintGL
// caller this replaces for a caller that has many frames to render)
void run_launch_sets(VolumeRenderCL &vr, const Options &o, const CameraPath &path)
{
    const Options::Batch &ba = o.batch;
    const size_t W = o.view.W, H = o.view.H;
    const int frames = ba.frames;
    const bool bench = ba.bench, rgba8 = o.out.rgba8, use_path = path.used();
    if (o.tech.pathtrace || o.render.img_ess || o.render.ao)
        throw std::runtime_error("--frames-per-launch: ray caster only, no image-order ESS, no ambient occlusion");
    const size_t K = size_t(std::min(256, std::max(1, ba.frames_per_launch)));
    // (a short run -- all the frames fit one launch set -- goes to ONE renderer as one set: two renderers with
    // half the frames each pay a set's ramp and tail side by side without hiding each other's; bench.py does
    // the same)
    const size_t F = size_t(frames) <= K ? 1 : size_t(std::max(1, ba.frames_in_flight));
    std::vector<std::unique_ptr<VolumeRenderCL>> twins;
    std::vector<VolumeRenderCL *> lanes{&vr};
    vr.setRoundBudget(unsigned(ba.round_budget));
    for (size_t j = 1; j < F; ++j) {
        twins.push_back(vr.shareVolumes());
        lanes.push_back(twins.back().get());
    }
    hip_ok(hipSetDevice(o.ranks.device), "hipSetDevice");
    std::vector<float *> blocks(F, nullptr);
    std::vector<unsigned char *> blocks8(F, nullptr);   // --rgba8: the 8-bit twins of a set's frames
    std::vector<hipStream_t> streams(F);
    for (size_t j = 0; j < F; ++j) {
        hip_ok(hipMalloc(reinterpret_cast<void **>(&blocks[j]), K * W * H * 4 * sizeof(float)), "hipMalloc frames");
        if (rgba8) hip_ok(hipMalloc(reinterpret_cast<void **>(&blocks8[j]), K * W * H * 4), "hipMalloc 8-bit frames");
        streams[j] = static_cast<hipStream_t>(lanes[j]->stream());
        lanes[j]->setFrameTiming(false);   // nobody reads a set's own time: the next set may start under its tail
    }
    const std::vector<unsigned int> seeds = vr.drawSeeds(size_t(frames));
    // (per segment of a camera path: a set never crosses a change of transfer function or time step)
    const std::vector<LaunchSet> sets = make_sets(path, seeds, K, F);
    std::vector<size_t> lane_seg(F, 0);
    if (use_path)
        for (size_t j = 0; j < F; ++j) apply_segment(*lanes[j], o, path, 0);
    auto submit = [&](size_t j, const LaunchSet &ls, const std::vector<unsigned int> &sd) {
        if (use_path && lane_seg[j] != ls.seg) {
            apply_segment(*lanes[j], o, path, ls.seg);   // (waits for the renderer's stream: its sets in flight)
            lane_seg[j] = ls.seg;
        }
        if (rgba8 && use_path) lanes[j]->renderFramesRGBA8(W, H, sd, ls.views, blocks[j], blocks8[j]);
        else if (rgba8) lanes[j]->renderFramesRGBA8(W, H, sd, blocks[j], blocks8[j]);
        else if (use_path) lanes[j]->renderFrames(W, H, sd, ls.views, blocks[j]);
        else lanes[j]->renderFrames(W, H, sd, blocks[j]);
    };
    if (bench) {   // every renderer once, untimed: buffers, work queue, skip bitmap, cell grid, cost map
        std::mt19937 warm(20261004u);
        for (size_t j = 0; j < F; ++j) {
            std::vector<unsigned int> ws(sets[0].seeds.size());
            for (auto &x : ws) x = static_cast<unsigned int>(warm());
            submit(j, sets[0], ws);
        }
        hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    hipEvent_t ev0, ev1;
    std::vector<hipEvent_t> done(F);
    hip_ok(hipEventCreate(&ev0), "hipEventCreate");
    hip_ok(hipEventCreate(&ev1), "hipEventCreate");
    for (auto &e : done) hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    std::vector<float> frame, all_frames;
    std::vector<unsigned char> frame8, all_frames8;
    all_frames.reserve(bench ? 0 : size_t(frames) * W * H * 4);
    const auto t0 = std::chrono::steady_clock::now();
    hip_ok(hipEventRecord(ev0, streams[0]), "hipEventRecord");
    for (size_t j = 1; j < F; ++j) hip_ok(hipStreamWaitEvent(streams[j], ev0, 0), "hipStreamWaitEvent");
    for (size_t i = 0; i < sets.size(); ++i) {
        submit(i % F, sets[i], sets[i].seeds);
        if (!bench && ((i + 1) % F == 0 || i + 1 == sets.size())) {
            // the frames of this round of sets to the host, in frame order, before their blocks are reused
            hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
            for (size_t k = i / F * F; k <= i; ++k) {
                const size_t at = all_frames.size(), nfl = sets[k].seeds.size() * W * H * 4;
                all_frames.resize(at + nfl);
                hip_ok(hipMemcpy(all_frames.data() + at, blocks[k % F], nfl * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
                if (rgba8) {
                    all_frames8.resize(at + nfl);
                    hip_ok(hipMemcpy(all_frames8.data() + at, blocks8[k % F], nfl, hipMemcpyDeviceToHost), "hipMemcpy");
                }
            }
        }
    }
    for (size_t j = 1; j < F; ++j) {
        hip_ok(hipEventRecord(done[j], streams[j]), "hipEventRecord");
        hip_ok(hipStreamWaitEvent(streams[0], done[j], 0), "hipStreamWaitEvent");
    }
    hip_ok(hipEventRecord(ev1, streams[0]), "hipEventRecord");
    hip_ok(hipEventSynchronize(ev1), "hipEventSynchronize");
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    float ms = 0.f;
    hip_ok(hipEventElapsedTime(&ms, ev0, ev1), "hipEventElapsedTime");
    // the last frame of the last set
    const size_t last = sets.size() - 1;
    frame.resize(W * H * 4);
    hip_ok(hipMemcpy(frame.data(), blocks[last % F] + (sets[last].seeds.size() - 1) * W * H * 4, frame.size() * sizeof(float),
                     hipMemcpyDeviceToHost), "hipMemcpy");
    vrhip_launch_info li;
    std::memset(&li, 0, sizeof li);
    (void)vrhip_last_launch_info(lanes[last % F]->handle(), &li);
    write_frames(o.out.prefix, frame, all_frames, W, H);
    if (rgba8) {
        frame8.resize(W * H * 4);
        hip_ok(hipMemcpy(frame8.data(), blocks8[last % F] + (sets[last].seeds.size() - 1) * W * H * 4, frame8.size(),
                         hipMemcpyDeviceToHost), "hipMemcpy");
        write_rgba8(o.out.prefix, frame8, all_frames8, W, H);
    }
    auto res = vr.getResolution();
    std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, \"frames\": %d, "
                "\"renderers\": %zu, \"launch_sets\": %zu, \"frames_per_launch_set\": %zu, \"round_budget\": %u, "
                "\"phase1_waves\": %u, \"phase2_waves\": %u, \"empty_skip\": %u, "
                "\"ms_per_frame\": %.5f, \"ms_per_frame_host_clock\": %.5f, \"bench\": %s, "
                "\"clock\": \"HIP events around the region on the first renderer's stream, the other renderers' "
                "streams joined before the second%s\", \"out\": \"%s.rgba.f32\"}\n",
                vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, frames, F, sets.size(),
                sets[0].seeds.size(), li.round_budget, li.phase1_waves, li.phase2_waves, li.empty_skip,
                double(ms) / frames, wall / frames * 1e3, bench ? "true" : "false",
                bench ? "" : " (frames copied to the host inside the region)", o.out.prefix.c_str());
    for (float *b : blocks) (void)hipFree(b);
    for (unsigned char *b : blocks8) (void)hipFree(b);
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    for (auto &e : done) (void)hipEventDestroy(e);
}

// ---- --pathtrace, the progressive image's N samples: in launch sets of K (VolumeRenderCL::renderSamples), or -- K = 1
// under --bench -- one launch per sample without the copy to the host between them.  The seeds are the ones the
// per-sample loop of run_frames draws: the written image is the same bit for bit.
void run_samples(VolumeRenderCL &vr, const Options &o)
{
    const size_t W = o.view.W, H = o.view.H;
    const int frames = o.batch.frames, per_launch = o.batch.samples_per_launch;
    const bool bench = o.batch.bench;
    const std::array<float, 16> view = the_view(o.view);
    const std::vector<unsigned int> seeds = vr.drawSeeds(size_t(frames));
    std::vector<float> frame;
    auto render = [&](bool to_host) {
        vr.updateView(view);   // iteration 0
        if (per_launch == 1) {
            for (size_t k = 0; k < seeds.size(); ++k) {
                vr.setSeed(seeds[k]);
                if (to_host && k + 1 == seeds.size()) vr.runRaycastNoGL(W, H, frame);
                else vr.runRaycast(W, H);
            }
        } else if (to_host) {
            vr.renderSamples(W, H, seeds, frame, unsigned(per_launch));
        } else {
            vr.renderSamples(W, H, seeds, static_cast<float *>(nullptr), unsigned(per_launch));
        }
    };
    double ms_per_sample = 0.0;
    if (bench) {
        render(false);   // untimed: buffers, work queue, cell grid, scratch
        hipStream_t st = static_cast<hipStream_t>(vr.stream());
        hipEvent_t e0, e1;
        hip_ok(hipEventCreate(&e0), "hipEventCreate");
        hip_ok(hipEventCreate(&e1), "hipEventCreate");
        hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
        hip_ok(hipEventRecord(e0, st), "hipEventRecord");
        render(false);
        hip_ok(hipEventRecord(e1, st), "hipEventRecord");
        hip_ok(hipEventSynchronize(e1), "hipEventSynchronize");
        float ms = 0.f;
        hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
        ms_per_sample = double(ms) / frames;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    render(true);
    vrhip_launch_info li;
    std::memset(&li, 0, sizeof li);
    (void)vrhip_last_launch_info(vr.handle(), &li);
    write_frames(o.out.prefix, frame, std::vector<float>(), W, H);
    if (o.out.rgba8) {   // the bytes of the image the frame buffer holds
        std::vector<unsigned char> frame8;
        vr.frameRGBA8(W, H, frame8);
        write_rgba8(o.out.prefix, frame8, std::vector<unsigned char>(), W, H);
    }
    auto res = vr.getResolution();
    std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                "\"samples\": %d, \"samples_per_launch\": %u, \"sample_kernel\": %s, \"bench\": %s, "
                "\"ms_per_sample\": %.5f, \"out\": \"%s.rgba.f32\"}\n",
                vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, frames, li.frames,
                li.samples ? "true" : "false", bench ? "true" : "false", ms_per_sample, o.out.prefix.c_str());
}

// ---- rendered frames on one GPU: launch sets, the path tracer's samples, or frame after frame -- a single frame,
// --frames N accumulated or --independent, one frame per camera of a path
void run_frames(VolumeRenderCL &vr, const Options &o, const CameraPath &path)
{
    const Options::Batch &ba = o.batch;
    if (ba.frames_per_launch > 0) return run_launch_sets(vr, o, path);
    if (o.tech.pathtrace && !ba.independent && !path.used() && ba.frames >= 1 && (ba.samples_per_launch != 1 || ba.bench))
        return run_samples(vr, o);
    const size_t W = o.view.W, H = o.view.H;
    const std::array<float, 16> view = the_view(o.view);
    std::vector<float> frame, all_frames;
    std::vector<unsigned char> frame8, all_frames8;   // --rgba8
    double kernel_s = 0.0;
    for (size_t sg = 0, in_seg = 0, f = 0; f < size_t(ba.frames); ++f, ++in_seg) {
        const std::array<float, 16> *pv = &view;
        if (path.used()) {   // frame f of the path: frame in_seg of segment sg
            if (f == 0) apply_segment(vr, o, path, 0);
            if (in_seg == path.segs[sg].views.size()) {
                apply_segment(vr, o, path, ++sg);
                in_seg = 0;
            }
            pv = &path.segs[sg].views[in_seg];
        }
        if (ba.independent) vr.updateView(*pv);   // (resets the running mean: iteration 0, volumerendercl.cpp:379-390)
        vr.runRaycastNoGL(W, H, frame);   // frames accumulate (running mean), like the reference
        kernel_s += vr.getLastExecTime();
        if (ba.independent) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
        if (o.out.rgba8) {   // the same frame's bytes, quantised on the GPU from the frame buffer
            vr.frameRGBA8(W, H, frame8);
            if (ba.independent) all_frames8.insert(all_frames8.end(), frame8.begin(), frame8.end());
        }
    }
    write_frames(o.out.prefix, frame, all_frames, W, H);
    if (o.out.rgba8) write_rgba8(o.out.prefix, frame8, all_frames8, W, H);
    auto res = vr.getResolution();
    std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                "\"frames\": %d, \"kernel_ms_per_frame\": %.4f, \"out\": \"%s.rgba.f32\"}\n",
                vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, ba.frames,
                kernel_s / ba.frames * 1e3, o.out.prefix.c_str());
}

} // namespace

// parse, validate, set up, dispatch
int main(int argc, char **argv)
{
    Options o = parse_args(argc, argv);
    validate(o);
    try {
        CameraPath path;
        const int ended = front_end(o, path);
        if (ended >= 0) return ended;
        if (o.mesh.on || o.stats.on) {
            VolumeRenderCL vr;
            setup_volume_only(vr, o);
            if (o.mesh.on) run_mesh(vr, o);
            else run_stats(vr, o);
            return 0;
        }
        if (o.ranks.n > 0 && o.render.img_ess) throw std::runtime_error("image-order ESS state crosses tile borders: not with --ranks");
        std::vector<std::unique_ptr<VolumeRenderCL>> vrs;   // one renderer, or one per rank
        for (int r = 0; r < std::max(1, o.ranks.n); ++r) {
            vrs.emplace_back(new VolumeRenderCL());
            if (!setup_renderer(*vrs.back(), o, o.ranks.n > 0 ? rank_device(o.ranks, r) : o.ranks.device)) return 0;
        }
        if (o.ranks.n > 0) run_ranks(vrs, o, path);
        else if (o.slice.any()) run_slices(*vrs[0], o);
        else if (o.depth.on) run_depth(*vrs[0], o);
        else run_frames(*vrs[0], o, path);
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}


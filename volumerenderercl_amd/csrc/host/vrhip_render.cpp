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

[[noreturn]] void usage()
{
    std::cerr <<
        "usage: vrhip_render (--dat FILE.dat | --synth sphere|shells N UCHAR|USHORT|FLOAT)\n"
        "         [--size W H] [--rotate AX AY AZ DEG] [--translate X Y Z] [--view M0..M15]\n"
        "         [--tf default|FILE] [--illum N] [--no-ess] [--ortho] [--nearest] [--rate R]\n"
        "         [--bg R G B] [--gradient-bg] [--seed S] [--frames N] [--device D] --out PREFIX\n"
        "         [--pathtrace] [--extinction E]   (technique 1; --frames = samples per pixel)\n"
        "         [--mip]                          (technique 2, maximum intensity projection: independent frames only --\n"
        "                                           one frame, --independent, --frames-per-launch, --camera-path / --orbit;\n"
        "                                           combines with --rgba8; not with --pathtrace, --ao, --show-ess, --img-ess,\n"
        "                                           --env)\n"
        "         [--iso V [--iso-refine N]]       (technique 4, first-hit isosurface at V -- in the units of the transfer\n"
        "                                           function's coordinate: normalised for UCHAR / USHORT, raw for FLOAT --\n"
        "                                           coloured TF(V), shaded with --illum 1 (the default) or flat with\n"
        "                                           --illum 0; N bisection rounds refine the hit, 0-16, default 4\n"
        "                                           (--iso-refine needs --iso);\n"
        "                                           independent frames like --mip; combines with --orbit, --camera-path,\n"
        "                                           --frames-per-launch, --rgba8 and --ranks; not with --pathtrace, --mip,\n"
        "                                           --ao, --show-ess, --img-ess, --env)\n"
        "         [--tf2d FILE NV NG GHI]          (technique 6, a two-dimensional transfer function TF2(value, gradient\n"
        "                                           magnitude): FILE holds NV x NG raw RGBA8 entries, value fastest; GHI is\n"
        "                                           the gradient magnitude at the table's upper edge -- the GHI of\n"
        "                                           --stats-window, whose histogram bins the entries are the centres of;\n"
        "                                           --illum 0 or 1; independent frames like --mip; combines with --orbit,\n"
        "                                           --camera-path, --frames-per-launch and --rgba8; not with --pathtrace,\n"
        "                                           --mip, --iso, --ao, --show-ess, --img-ess, --env, --ranks)\n"
        "         [--tf2d-ramp NG GHI G0 G1]       (the same from the command's 1-D table: NG rows of it, their opacity\n"
        "                                           scaled by a ramp over the gradient magnitude, 0 up to G0 and 1 from G1\n"
        "                                           on -- boundary emphasis)\n"
        "         [--samples-per-launch K]         (--pathtrace: the N samples in launch sets of K -- vrhip_render_samples,\n"
        "                                           the same image bit for bit; 0 = the library's default set size, the\n"
        "                                           default; 1 = one launch per sample, as before; with --bench: one\n"
        "                                           untimed image, then the N samples timed with HIP events, ms per sample)\n"
        "         [--device-ingest]                (--dat: the loader only reads the raw files; maximum, USHORT stretch /\n"
        "                                           FLOAT normalisation and histogram are computed on the GPU -- the same\n"
        "                                           voxels bit for bit)\n"
        "         [--downsample FACTOR]            (volumeDownsampling: writes <dat>_<N>.raw/.dat, no frame)\n"
        "         [--state FILE.json] [--tf-stops FILE.tff]   (files saved by the reference GUI)\n"
        "         [--tf-easing linear|quad|cubic] [--dump-tf FILE]   (interpolation between the stops; --dump-tf\n"
        "                                           writes the RGBA8 table the options select and exits, no GPU)\n"
        "         [--contours] [--aerial] [--ao] [--show-ess] [--img-ess]   (--img-ess: state carried over --frames)\n"
        "         [--env FILE.hdr]                 (createEnvironmentMap: Radiance RGBE environment map)\n"
        "         [--ranks N [--tile T] [--loopback] [--force-gather]]   (image tiles over N GPUs, devices D .. D+N-1,\n"
        "                                           volume replicated, RCCL gather to the first; --loopback: N\n"
        "                                           renderers on device D, device copies instead of RCCL;\n"
        "                                           --force-gather: the root sends its tiles to itself over RCCL\n"
        "                                           too -- with --ranks 1 the transport runs on one GPU)\n"
        "         [--independent]                  (--frames N independent frames -- iteration 0 each, jitter seeds = the\n"
        "                                           first N outputs of the default-seeded mt19937 -- instead of the\n"
        "                                           running mean; all of them go to PREFIX.frames.rgba.f32)\n"
        "         [--frames-per-launch K [--frames-in-flight F] [--round-budget B] [--bench] [--root-share X]]\n"
        "                                          (the throughput path: the N independent frames in launch sets of K\n"
        "                                           (vrhip_render_batch), F renderers over one shared volume taking the\n"
        "                                           sets in turn (default 2; with --ranks: one per rank, K frames per\n"
        "                                           exchange, sparse messages, one exchange in flight), phase-1 round\n"
        "                                           budget B (default 48); --bench: one untimed set per renderer, then\n"
        "                                           the N frames timed with HIP events, nothing copied or written but\n"
        "                                           the last frame; --root-share: rank 0's share of a peer's tiles)\n"
        "         [--camera-path FILE | --orbit AX AY AZ N] [--dump-views FILE]\n"
        "                                          (one independent frame per camera entry of a path the reference GUI\n"
        "                                           recorded -- FILE_quat.txt + FILE_trans.txt, or an interaction log\n"
        "                                           whose transferFunction / timestep lines apply to the frames after\n"
        "                                           them -- or of an N-view turntable about the axis from the start\n"
        "                                           camera; --frames is ignored, the frames go to PREFIX.frames.rgba.f32;\n"
        "                                           --dump-views writes the 16-float matrices and exits, no GPU)\n"
        "         [--rgba8]                        (also the frame as 8-bit RGBA, the reference's display format, quantised\n"
        "                                           on the GPU: PREFIX.rgba.u8 (W*H*4 bytes), with several frames\n"
        "                                           PREFIX.frames.rgba.u8, and PREFIX.ppm from those bytes; not with --ranks)\n"
        "         [--slice-axis X|Y|Z POS | --slice OX OY OZ UX UY UZ VX VY VZ]\n"
        "         [--slab T N max|min|mean] [--slice-stack N] [--slice-value]\n"
        "                                          (slice views instead of a rendered frame: the full cross-section of the\n"
        "                                           box [-1,1]^3 perpendicular to an axis at POS (Z: right +x, up +y; Y: right\n"
        "                                           -x, up +z; X: right +y, up +z), or the plane with centre O, O + U the\n"
        "                                           centre of the right edge and O + V of the top edge; --slab: max, min or\n"
        "                                           mean of N (1-256) parallel planes over thickness T along the normal;\n"
        "                                           --slice-stack: N such slices spanning the box along the normal, one\n"
        "                                           launch; --slice-value: the filtered value in r, g, b instead of the\n"
        "                                           transfer function's colour; uses --size, --tf, --bg, --nearest; the\n"
        "                                           slices go to PREFIX.frames.rgba.f32, the last to PREFIX.rgba.f32, with\n"
        "                                           --rgba8 also as bytes; not with --mip, --iso, --pathtrace, --orbit,\n"
        "                                           --camera-path, --ranks)\n"
        "         [--depth iso V | max | opacity A] [--depth-refine N] [--depth-rect X Y W H]\n"
        "                                          (a depth image instead of a rendered frame: per pixel of the camera's\n"
        "                                           frame the first sample at or above V, refined by N (0-16, default 4)\n"
        "                                           bisections (iso), the first sample that attains the ray's maximum (max),\n"
        "                                           or the sample at which the accumulated opacity reaches A (opacity);\n"
        "                                           --depth-rect: that rectangle of the frame only; writes\n"
        "                                           PREFIX.depth.f32 (x y z t per pixel: box-space position and ray\n"
        "                                           parameter, 0 0 0 inf without a hit), PREFIX.depth.aux.f32 (the value\n"
        "                                           found), PREFIX.depth.kind.u8 (0 miss, 1 no hit, 2 hit) and PREFIX.ppm\n"
        "                                           (grey: finite t between its minimum and maximum, non-hits black); not\n"
        "                                           with --pathtrace, --mip, --iso, the slice options, --ranks,\n"
        "                                           --frames-per-launch, --orbit, --camera-path, --frames, --rgba8,\n"
        "                                           --img-ess; --depth-refine and --depth-rect need --depth)\n"
        "         [--mesh V FILE.stl|.ply] [--mesh-normals] [--mesh-region X0 Y0 Z0 X1 Y1 Z1] [--timestep T]\n"
        "         [--mesh-indexed]\n"
        "                                          (the isosurface at V as triangles instead of a rendered frame: binary\n"
        "                                           STL, the triangle list as it is, or binary little-endian PLY, welded by\n"
        "                                           bit-equal positions; --mesh-normals: technique 4's shading normal per\n"
        "                                           vertex (PLY: nx ny nz); --mesh-region: the cubes between voxels\n"
        "                                           (X0, Y0, Z0) and (X1, Y1, Z1) only; --timestep: of that time step;\n"
        "                                           needs no --size, camera or --out; prints the triangle count, for\n"
        "                                           .ply the vertex count too; not with a render, slice or depth option,\n"
        "                                           --ranks, --frames, --rgba8, --downsample; --mesh-normals,\n"
        "                                           --mesh-region and --timestep need --mesh; --mesh-indexed, with a\n"
        "                                           .ply only: the indexed mesh as the device makes it, one vertex per\n"
        "                                           crossed lattice edge, no weld on the host)\n"
        "         [--stats FILE.json] [--stats-bins V G] [--stats-window LO HI GHI] [--stats-region X0 Y0 Z0 X1 Y1 Z1]\n"
        "         [--stats-moments] [--stats-hist FILE.u64] [--timestep T]\n"
        "                                          (what is in the volume instead of a rendered frame: the counts of the\n"
        "                                           normalised values of channel 0 -- voxels, nan, below, above,\n"
        "                                           gradient_nan, binned -- and the value x gradient-magnitude histogram,\n"
        "                                           V (1-4096, default 256) value bins over [LO, HI] (default 0 1) by G\n"
        "                                           (1-256, default 1) gradient bins over [0, GHI) (default 1), the top\n"
        "                                           one open-ended, V * G <= 65536, computed on the device, as JSON with\n"
        "                                           the table as rows of V counts; --stats-region: the voxels from\n"
        "                                           (X0, Y0, Z0) up to but not including (X1, Y1, Z1); --stats-moments:\n"
        "                                           min, max, sum, sum_sq, mean and std too; --stats-hist: the table as\n"
        "                                           G * V little-endian 64-bit counts; --timestep: of that time step;\n"
        "                                           needs no --size, camera or --out; not with a render, slice, depth or\n"
        "                                           mesh option, --ranks, --frames, --rgba8, --downsample; the other\n"
        "                                           --stats-* options need --stats)\n"
        "         [--filter gauss SIGMA [RADIUS]] [--filter median] [--filter taps FILE]\n"
        "                                          (filter the loaded time step on the device, in place, before whatever\n"
        "                                           else the command does -- a render, --mesh, --stats, slices, depth --\n"
        "                                           and rebuild the ESS bricks; repeatable, applied in order; gauss: a\n"
        "                                           normalised Gaussian of SIGMA voxels along x, scaled per axis by the\n"
        "                                           slice thickness, RADIUS 1-8 (default ceil(3 sigma), at most 8);\n"
        "                                           median: the 3x3x3 median; taps: FILE holds three lines, for x, y and\n"
        "                                           z, of 1 to 9 weights each, the weight at distance 0 first; honours\n"
        "                                           --timestep where that is allowed; not with --ranks, --downsample)\n"
        "writes PREFIX.rgba.f32 (W*H*4 float32, row 0 = top), PREFIX.ppm and prints one JSON line\n";
    std::exit(2);
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

// --filter: one entry per occurrence, in the order given
struct FilterSpec {
    enum { GAUSS, MEDIAN, TAPS } kind = GAUSS;
    double sigma = 1.0;
    unsigned radius = 0;                    // GAUSS: 0 = by sigma
    VolumeRenderCL::FilterParams taps;      // TAPS
};

// --filter taps FILE: three lines (x, y, z) of 1 to 9 finite weights, distance 0 first; '#' starts a comment line
bool read_filter_taps(const std::string &path, VolumeRenderCL::FilterParams &fp)
{
    std::ifstream f(path);
    if (!f) return false;
    std::string line;
    size_t axis = 0;
    while (std::getline(f, line)) {
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        if (axis == 3) return false;
        std::istringstream in(line);
        double w;
        size_t n = 0;
        while (in >> w) {
            if (n == 9 || !std::isfinite(float(w))) return false;
            fp.taps[axis][n++] = float(w);
        }
        if (!in.eof() || n == 0) return false;
        fp.radius[axis] = unsigned(n - 1);
        ++axis;
    }
    return axis == 3;
}

void apply_filters(VolumeRenderCL &vr, const std::vector<FilterSpec> &filters)
{
    for (const FilterSpec &fs : filters) {
        if (fs.kind == FilterSpec::GAUSS) vr.gaussianFilter(fs.sigma, fs.radius);
        else if (fs.kind == FilterSpec::MEDIAN) vr.medianFilter();
        else vr.filterVolume(fs.taps, vr.getTimestep());
    }
}

} // namespace

int main(int argc, char **argv)
{
    std::string dat, synth_kind, synth_fmt = "UCHAR", tf = "default", out, env_file;
    unsigned synth_n = 0;
    size_t W = 1024, H = 1024;
    double q[4] = {1, 0, 0, 0}, tr[3] = {0, 0, 2};
    bool have_view = false, ess = true, ortho = false, linear = true, gradient_bg = false, pin = false;
    bool pathtrace = false, mip = false, iso = false, device_ingest = false;
    double iso_value = 0.5;
    int iso_refine = 4;
    bool have_iso_refine = false;
    // technique 6 (--tf2d FILE NV NG GHI, --tf2d-ramp NG GHI G0 G1)
    bool tf2d = false, tf2d_ramp = false;
    std::string tf2d_file;
    long tf2d_nv = 0, tf2d_ng = 0;
    double tf2d_ghi = 0.0, tf2d_g0 = 0.0, tf2d_g1 = 0.0;
    double extinction = 100.0;
    int downsample = 0;
    std::string state_file, tf_stops, tf_easing = "linear", dump_tf;
    bool contours = false, aerial = false, use_ao_flag = false, show_ess_flag = false, img_ess = false;
    std::array<float, 16> view{};
    unsigned illum = 1, seed = 0;
    int frames = 1, device = 0, ranks = 0;
    size_t tile = 64;
    bool loopback = false, force_gather = false;
    bool independent = false, bench = false, rgba8 = false;
    int frames_per_launch = 0, frames_in_flight = 2, round_budget = 48, samples_per_launch = 0;
    double root_share = 1.0;
    double rate = 1.5;
    std::array<float, 4> bg = {{1, 1, 1, 1}};
    std::string camera_path, dump_views;
    bool have_path_arg = false, have_orbit = false;
    double orbit_axis[3] = {0, 1, 0};
    int orbit_n = 0;
    // slice views (--slice-axis / --slice, --slab, --slice-stack, --slice-value)
    bool have_slice_axis = false, have_slice_plane = false, have_slab = false, have_stack = false, slice_value = false;
    int slice_axis = 2, slab_n = 1, stack_n = 0;
    double slice_pos = 0.0, slice_vec[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, slab_t = 0.0;
    std::string slab_mode = "max";
    // depth images (--depth, --depth-refine, --depth-rect)
    bool depth = false, have_depth_refine = false, have_depth_rect = false;
    std::string depth_mode;
    double depth_threshold = 0.5;
    int depth_refine = 4;
    long depth_rect[4] = {0, 0, 0, 0};
    // isosurface extraction (--mesh, --mesh-normals, --mesh-region, --timestep)
    bool mesh = false, mesh_normals = false, have_mesh_region = false, have_timestep = false, mesh_indexed = false;
    double mesh_iso = 0.5;
    std::string mesh_file;
    long mesh_region[6] = {0, 0, 0, 0, 0, 0}, timestep = 0;
    // volume statistics (--stats, --stats-bins, --stats-window, --stats-region, --stats-moments, --stats-hist)
    bool stats = false, have_stats_opt = false, have_stats_region = false, stats_moments = false;
    std::string stats_file, stats_hist_file;
    long stats_bins[2] = {256, 1}, stats_region[6] = {0, 0, 0, 0, 0, 0};
    double stats_window[3] = {0.0, 1.0, 1.0};
    std::vector<FilterSpec> filters;   // --filter

    auto need = [&](int i, int n) { if (i + n >= argc) usage(); };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--dat") { need(i, 1); dat = argv[++i]; }
        else if (a == "--synth") { need(i, 3); synth_kind = argv[++i]; synth_n = unsigned(std::atoi(argv[++i])); synth_fmt = argv[++i]; }
        else if (a == "--size") { need(i, 2); W = size_t(std::atol(argv[++i])); H = size_t(std::atol(argv[++i])); }
        else if (a == "--rotate") {
            need(i, 4);
            double ax = std::atof(argv[++i]), ay = std::atof(argv[++i]), az = std::atof(argv[++i]);
            double half = std::atof(argv[++i]) * M_PI / 360.0, l = std::sqrt(ax * ax + ay * ay + az * az);
            q[0] = std::cos(half); q[1] = ax / l * std::sin(half); q[2] = ay / l * std::sin(half); q[3] = az / l * std::sin(half);
        }
        else if (a == "--translate") { need(i, 3); for (int k = 0; k < 3; ++k) tr[k] = std::atof(argv[++i]); }
        else if (a == "--view") { need(i, 16); for (int k = 0; k < 16; ++k) view[size_t(k)] = float(std::atof(argv[++i])); have_view = true; }
        else if (a == "--tf") { need(i, 1); tf = argv[++i]; }
        else if (a == "--illum") { need(i, 1); illum = unsigned(std::atoi(argv[++i])); }
        else if (a == "--no-ess") ess = false;
        else if (a == "--ortho") ortho = true;
        else if (a == "--nearest") linear = false;
        else if (a == "--gradient-bg") gradient_bg = true;
        else if (a == "--rate") { need(i, 1); rate = std::atof(argv[++i]); }
        else if (a == "--bg") { need(i, 3); for (int k = 0; k < 3; ++k) bg[size_t(k)] = float(std::atof(argv[++i])); }
        else if (a == "--seed") { need(i, 1); seed = unsigned(std::strtoul(argv[++i], nullptr, 10)); pin = true; }
        else if (a == "--frames") { need(i, 1); frames = std::atoi(argv[++i]); }
        else if (a == "--pathtrace") pathtrace = true;
        else if (a == "--mip") mip = true;
        else if (a == "--iso") { need(i, 1); iso = true; iso_value = std::atof(argv[++i]); }
        else if (a == "--iso-refine") { need(i, 1); have_iso_refine = true; iso_refine = std::atoi(argv[++i]); }
        else if (a == "--tf2d") {
            need(i, 4);
            tf2d = true;
            tf2d_file = argv[++i];
            tf2d_nv = std::atol(argv[++i]);
            tf2d_ng = std::atol(argv[++i]);
            tf2d_ghi = std::atof(argv[++i]);
        }
        else if (a == "--tf2d-ramp") {
            need(i, 4);
            tf2d_ramp = true;
            tf2d_ng = std::atol(argv[++i]);
            tf2d_ghi = std::atof(argv[++i]);
            tf2d_g0 = std::atof(argv[++i]);
            tf2d_g1 = std::atof(argv[++i]);
        }
        else if (a == "--device-ingest") device_ingest = true;
        else if (a == "--downsample") { need(i, 1); downsample = std::atoi(argv[++i]); }
        else if (a == "--state") { need(i, 1); state_file = argv[++i]; }
        else if (a == "--tf-stops") { need(i, 1); tf_stops = argv[++i]; }
        else if (a == "--tf-easing") { need(i, 1); tf_easing = argv[++i]; }
        else if (a == "--dump-tf") { need(i, 1); dump_tf = argv[++i]; }
        else if (a == "--contours") contours = true;
        else if (a == "--aerial") aerial = true;
        else if (a == "--ao") use_ao_flag = true;
        else if (a == "--show-ess") show_ess_flag = true;
        else if (a == "--img-ess") img_ess = true;
        else if (a == "--env") { need(i, 1); env_file = argv[++i]; }
        else if (a == "--extinction") { need(i, 1); extinction = std::atof(argv[++i]); }
        else if (a == "--device") { need(i, 1); device = std::atoi(argv[++i]); }
        else if (a == "--ranks") { need(i, 1); ranks = std::atoi(argv[++i]); }
        else if (a == "--tile") { need(i, 1); tile = size_t(std::atol(argv[++i])); }
        else if (a == "--loopback") loopback = true;
        else if (a == "--force-gather") force_gather = true;
        else if (a == "--independent") independent = true;
        else if (a == "--bench") bench = true;
        else if (a == "--rgba8") rgba8 = true;
        else if (a == "--frames-per-launch") { need(i, 1); frames_per_launch = std::atoi(argv[++i]); }
        else if (a == "--samples-per-launch") { need(i, 1); samples_per_launch = std::atoi(argv[++i]); if (samples_per_launch < 0) usage(); }
        else if (a == "--frames-in-flight") { need(i, 1); frames_in_flight = std::atoi(argv[++i]); }
        else if (a == "--round-budget") { need(i, 1); round_budget = std::atoi(argv[++i]); }
        else if (a == "--root-share") { need(i, 1); root_share = std::atof(argv[++i]); }
        else if (a == "--out") { need(i, 1); out = argv[++i]; }
        else if (a == "--camera-path") { need(i, 1); camera_path = argv[++i]; have_path_arg = true; }
        else if (a == "--orbit") {
            need(i, 4);
            for (int k = 0; k < 3; ++k) orbit_axis[k] = std::atof(argv[++i]);
            orbit_n = std::atoi(argv[++i]);
            have_orbit = true;
        }
        else if (a == "--slice-axis") {
            need(i, 2);
            const std::string ax = argv[++i];
            slice_axis = ax == "X" || ax == "x" ? 0 : ax == "Y" || ax == "y" ? 1 : ax == "Z" || ax == "z" ? 2 : -1;
            slice_pos = std::atof(argv[++i]);
            have_slice_axis = true;
        }
        else if (a == "--slice") { need(i, 9); for (int k = 0; k < 9; ++k) slice_vec[k] = std::atof(argv[++i]); have_slice_plane = true; }
        else if (a == "--slab") { need(i, 3); slab_t = std::atof(argv[++i]); slab_n = std::atoi(argv[++i]); slab_mode = argv[++i]; have_slab = true; }
        else if (a == "--slice-stack") { need(i, 1); stack_n = std::atoi(argv[++i]); have_stack = true; }
        else if (a == "--slice-value") slice_value = true;
        else if (a == "--dump-views") { need(i, 1); dump_views = argv[++i]; }
        else if (a == "--depth") {
            need(i, 1);
            depth = true;
            depth_mode = argv[++i];
            if (depth_mode == "iso" || depth_mode == "opacity") { need(i, 1); depth_threshold = std::atof(argv[++i]); }
        }
        else if (a == "--depth-refine") { need(i, 1); have_depth_refine = true; depth_refine = std::atoi(argv[++i]); }
        else if (a == "--depth-rect") { need(i, 4); for (int k = 0; k < 4; ++k) depth_rect[k] = std::atol(argv[++i]); have_depth_rect = true; }
        else if (a == "--mesh") { need(i, 2); mesh = true; mesh_iso = std::atof(argv[++i]); mesh_file = argv[++i]; }
        else if (a == "--mesh-normals") mesh_normals = true;
        else if (a == "--mesh-indexed") mesh_indexed = true;
        else if (a == "--mesh-region") { need(i, 6); for (int k = 0; k < 6; ++k) mesh_region[k] = std::atol(argv[++i]); have_mesh_region = true; }
        else if (a == "--stats") { need(i, 1); stats = true; stats_file = argv[++i]; }
        else if (a == "--stats-bins") { need(i, 2); for (int k = 0; k < 2; ++k) stats_bins[k] = std::atol(argv[++i]); have_stats_opt = true; }
        else if (a == "--stats-window") { need(i, 3); for (int k = 0; k < 3; ++k) stats_window[k] = std::atof(argv[++i]); have_stats_opt = true; }
        else if (a == "--stats-region") {
            need(i, 6);
            for (int k = 0; k < 6; ++k) stats_region[k] = std::atol(argv[++i]);
            have_stats_opt = have_stats_region = true;
        }
        else if (a == "--stats-moments") have_stats_opt = stats_moments = true;
        else if (a == "--stats-hist") { need(i, 1); stats_hist_file = argv[++i]; have_stats_opt = true; }
        else if (a == "--filter") {
            need(i, 1);
            const std::string what = argv[++i];
            FilterSpec fs;
            if (what == "gauss") {
                need(i, 1);
                fs.kind = FilterSpec::GAUSS;
                fs.sigma = std::atof(argv[++i]);
                if (!(std::isfinite(fs.sigma) && fs.sigma > 0.0)) usage();
                if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // (an option starts with '-')
                    const long rad = std::atol(argv[++i]);
                    if (rad < 1 || rad > 8) usage();
                    fs.radius = unsigned(rad);
                }
            } else if (what == "median") fs.kind = FilterSpec::MEDIAN;
            else if (what == "taps") {
                need(i, 1);
                fs.kind = FilterSpec::TAPS;
                if (!read_filter_taps(argv[++i], fs.taps)) {
                    std::fprintf(stderr, "--filter taps: %s does not hold three lines of 1 to 9 finite weights\n", argv[i]);
                    return 2;
                }
            } else usage();
            filters.push_back(fs);
        }
        else if (a == "--timestep") { need(i, 1); timestep = std::atol(argv[++i]); have_timestep = true; }
        else usage();
    }
    if (have_path_arg && (camera_path.empty() || have_orbit)) usage();
    if (mip && pathtrace) usage();
    if (iso && (pathtrace || mip || use_ao_flag || show_ess_flag || img_ess || !env_file.empty())) usage();
    if (have_iso_refine && (!iso || iso_refine < 0 || iso_refine > 16)) usage();
    if (tf2d || tf2d_ramp) {
        if (tf2d && tf2d_ramp) usage();
        if (pathtrace || mip || iso || use_ao_flag || show_ess_flag || img_ess || !env_file.empty() || ranks > 0) usage();
        if (tf2d && (tf2d_file.empty() || tf2d_nv < 1 || tf2d_nv > long(VRHIP_TF2D_MAX_NV))) usage();
        if (tf2d_ng < 1 || tf2d_ng > long(VRHIP_TF2D_MAX_NG) || (tf2d && tf2d_nv * tf2d_ng > long(VRHIP_TF2D_MAX_ENTRIES))) usage();
        if (!std::isfinite(tf2d_ghi) || !(float(tf2d_ghi) > 0.f)) usage();
        if (tf2d_ramp && (!std::isfinite(tf2d_g0) || !std::isfinite(tf2d_g1) || !(float(tf2d_g0) >= 0.f) ||
                          !(float(tf2d_g1) > float(tf2d_g0))))
            usage();
    }
    const bool tf2d_any = tf2d || tf2d_ramp;
    if (rgba8 && ranks > 0) {
        std::cerr << "--rgba8 cannot be combined with --ranks: the C++ tile gather carries float pixels "
                     "(8-bit frames over several GPUs: the Python TileDriver, pixel_format=\"rgba8\")" << std::endl;
        return 2;
    }
    const bool slicing = have_slice_axis || have_slice_plane;
    if ((have_slab || have_stack || slice_value) && !slicing) usage();
    if (slicing) {
        if (have_slice_axis && have_slice_plane) usage();
        if (mip || iso || tf2d_any || pathtrace || have_orbit || have_path_arg || ranks > 0) usage();
        if (have_slice_axis && (slice_axis < 0 || !std::isfinite(slice_pos))) usage();
        for (double c : slice_vec) if (!std::isfinite(c)) usage();
        if (have_slab && (slab_n < 1 || slab_n > int(VRHIP_SLICE_MAX_SAMPLES) || !std::isfinite(slab_t) ||
                          (slab_mode != "max" && slab_mode != "min" && slab_mode != "mean")))
            usage();
        if (have_stack && (stack_n < 1 || stack_n > 1 << 16)) usage();
        if (have_slice_plane && (have_slab || have_stack)) {   // these need the plane's normal
            const double *u = slice_vec + 3, *v = slice_vec + 6;
            const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            if (n[0] * n[0] + n[1] * n[1] + n[2] * n[2] == 0.0) usage();
        }
    }
    if ((have_depth_refine || have_depth_rect) && !depth) usage();
    if (depth) {
        if (depth_mode != "iso" && depth_mode != "max" && depth_mode != "opacity") usage();
        if (pathtrace || mip || iso || tf2d_any || slicing || have_slab || have_stack || slice_value || ranks > 0 ||
            frames_per_launch > 0)
            usage();
        // one depth image of one camera: what asks for several frames, or for a frame's own state, has nothing to act on
        if (have_orbit || have_path_arg || frames != 1 || rgba8 || img_ess) usage();
        if (!std::isfinite(depth_threshold) || depth_refine < 0 || depth_refine > 16) usage();
        if (have_depth_rect) {
            for (long c : depth_rect) if (c < 0 || c > 16384) usage();
            if (depth_rect[2] < 1 || depth_rect[3] < 1 || depth_rect[0] + depth_rect[2] > long(W) ||
                depth_rect[1] + depth_rect[3] > long(H))
                usage();
        }
    }
    if ((mesh_normals || have_mesh_region || mesh_indexed) && !mesh) usage();
    if (have_timestep && !mesh && !stats) usage();
    if (have_stats_opt && !stats) usage();
    if (!filters.empty() && (ranks > 0 || downsample)) usage();
    if (stats) {
        // numbers about the volume, not a picture of it: as for --mesh, and not with it
        if (mesh || pathtrace || mip || iso || tf2d_any || have_iso_refine || slicing || have_slab || have_stack || slice_value || depth ||
            ranks > 0 || frames_per_launch > 0 || have_orbit || have_path_arg || frames != 1 || rgba8 || img_ess || downsample ||
            !dump_tf.empty() || bench || independent)
            usage();
        if (stats_file.empty() || timestep < 0) usage();
        if (stats_bins[0] < 1 || stats_bins[0] > 4096 || stats_bins[1] < 1 || stats_bins[1] > 256 ||
            stats_bins[0] * stats_bins[1] > 65536)
            usage();
        if (!std::isfinite(stats_window[0]) || !std::isfinite(stats_window[1]) || !(float(stats_window[1]) > float(stats_window[0])))
            usage();
        if (stats_bins[1] > 1 && (!std::isfinite(stats_window[2]) || !(float(stats_window[2]) > 0.f))) usage();
        for (long c : stats_region) if (c < 0 || c > 8192) usage();
    }
    bool mesh_ply = false;
    if (mesh) {
        const size_t dot = mesh_file.rfind('.');
        const std::string ext = dot == std::string::npos ? "" : mesh_file.substr(dot);
        if (ext != ".stl" && ext != ".ply") usage();
        mesh_ply = ext == ".ply";
        if (mesh_indexed && !mesh_ply) usage();   // (STL is a triangle list)
        // triangles of the volume, not a picture of it: what selects, shapes or multiplies frames has nothing to act on
        if (pathtrace || mip || iso || tf2d_any || have_iso_refine || slicing || have_slab || have_stack || slice_value || depth || ranks > 0 ||
            frames_per_launch > 0 || have_orbit || have_path_arg || frames != 1 || rgba8 || img_ess || downsample ||
            !dump_tf.empty() || bench || independent)
            usage();
        if (!std::isfinite(mesh_iso) || timestep < 0) usage();
        for (long c : mesh_region) if (c < 0 || c > 8192) usage();
    }
    if (have_orbit && (orbit_n < 1 || orbit_n > 1 << 20 ||
                       orbit_axis[0] * orbit_axis[0] + orbit_axis[1] * orbit_axis[1] + orbit_axis[2] * orbit_axis[2] == 0.0))
        usage();
    if (!dump_views.empty() && !have_path_arg && !have_orbit) usage();
    // the camera path (--camera-path / --orbit), parsed before anything touches a GPU
    std::vector<PathEvent> path_events;
    std::vector<PathSegment> segs;
    try {
        if (have_path_arg) {
            std::ifstream probe(camera_path + "_quat.txt");
            path_events = probe ? read_view_record(camera_path) : read_interaction_log(camera_path);
        } else if (have_orbit) {
            if (!state_file.empty()) {   // (the orbit starts from the camera the options select, --state included)
                const CamState st = read_cam_state(state_file);
                if (st.has_rot) for (int k = 0; k < 4; ++k) q[k] = st.q[k];
                if (st.has_tr) for (int k = 0; k < 3; ++k) tr[k] = st.t[k];
            }
            path_events = orbit_views(orbit_axis, orbit_n, q, tr);
        }
        if (!dump_views.empty()) {   // front-end formula only: nothing below touches a GPU
            std::ofstream f(dump_views, std::ios::binary);
            for (const PathEvent &e : path_events)
                if (e.kind == PathEvent::CAMERA)
                    f.write(reinterpret_cast<const char *>(e.view.data()), std::streamsize(16 * sizeof(float)));
            return f ? 0 : 1;
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    const bool use_path = !path_events.empty();
    if (use_path) {
        segs = path_segments(path_events);
        frames = 0;
        for (const PathSegment &sg : segs) frames += int(sg.views.size());
        independent = true;
        if (pathtrace || img_ess) {
            std::cerr << "--camera-path / --orbit: ray caster only, no image-order ESS" << std::endl;
            return 1;
        }
    }
    if (tf_easing != "linear" && tf_easing != "quad" && tf_easing != "cubic") usage();
    // the transfer-function table the options select (TransferFunctionWidget's default stops,
    // transferfunctionwidget.cpp:338-346, unless a file is given)
    auto make_table = [&]() -> std::vector<unsigned char> {
        return !tf_stops.empty() ? tff_from_stops_file(tf_stops, tf_easing)
               : tf == "default" ? tff_from_stops({{0.0, {0, 0, 0, 0}}, {0.1, {125, 125, 125, 0}}, {1.0, {0, 0, 0, 255}}},
                                                  1024, tf_easing)
                                 : tff_from_raw_file(tf);
    };
    if (!dump_tf.empty()) {   // front-end formula only: nothing below touches a GPU
        try {
            const std::vector<unsigned char> table = make_table();
            std::ofstream f(dump_tf, std::ios::binary);
            f.write(reinterpret_cast<const char *>(table.data()), std::streamsize(table.size()));
            return f ? 0 : 1;
        } catch (const std::exception &e) {
            std::cerr << e.what() << std::endl;
            return 1;
        }
    }
    if ((dat.empty() && synth_kind.empty()) || (out.empty() && !downsample && !mesh && !stats)) usage();

    try {
        // everything the front end sets on a renderer; returns false when there is no frame to render
        auto setup = [&](VolumeRenderCL &vr, int dev) -> bool {
        vr.initialize(false, false, VENDOR_ANY, std::to_string(dev));
        if (!dat.empty()) {
            DatRawReader::Properties p;
            p.dat_file_name = dat;
            vr.setDeviceIngest(device_ingest);
            vr.loadVolumeData(p);
        } else {
            DatRawReader::data_format f = synth_fmt == "USHORT" ? DatRawReader::USHORT
                                          : synth_fmt == "FLOAT" ? DatRawReader::FLOAT : DatRawReader::UCHAR;
            vr.loadSyntheticVolume(synth_kind, synth_n, f);
        }
        if (!filters.empty()) {
            vr.setObjEss(ess);
            apply_filters(vr, filters);
        }
        if (downsample) {   // volumeDownsampling (volumerendercl.cpp:238-341) and nothing else
            const std::string base = vr.volumeDownsampling(0, downsample);
            std::printf("{\"downsampled\": \"%s\"}\n", base.c_str());
            return false;
        }
        bool use_ao = use_ao_flag, show_box = show_ess_flag;
        if (!state_file.empty()) {   // what the GUI's widgets would forward after loadCamState
            const CamState st = read_cam_state(state_file);
            if (st.has_rot) for (int k = 0; k < 4; ++k) q[k] = st.q[k];
            if (st.has_tr) for (int k = 0; k < 3; ++k) tr[k] = st.t[k];
            if (st.num.count("rayStepSize")) rate = st.num.at("rayStepSize");
            if (st.num.count("imgResFactor")) {
                W = size_t(std::floor(double(W) * st.num.at("imgResFactor")));
                H = size_t(std::floor(double(H) * st.num.at("imgResFactor")));
            }
            if (st.flag.count("useLerp")) linear = st.flag.at("useLerp");
            if (st.flag.count("useOrtho")) ortho = st.flag.at("useOrtho");
            if (st.flag.count("showContours")) contours = st.flag.at("showContours");
            if (st.flag.count("useAerial")) aerial = st.flag.at("useAerial");
            if (st.flag.count("useAO")) use_ao = st.flag.at("useAO");
            if (st.flag.count("showBox")) show_box = st.flag.at("showBox");
        }
        std::vector<unsigned char> table = make_table();
        vr.setTransferFunction(table);
        vr.setIllumination(illum);
        vr.setObjEss(ess);
        vr.setCamOrtho(ortho);
        vr.setLinearInterpolation(linear);
        vr.setUseGradient(gradient_bg);
        vr.setContours(contours);
        vr.setAerial(aerial);
        vr.setAmbientOcclusion(use_ao);
        if (show_box) vr.setShowESS(true);
        if (!env_file.empty()) vr.createEnvironmentMap(env_file);
        if (img_ess) vr.setImgEss(true);   // state carried from frame to frame (--frames N)
        vr.setBackground(bg);
        vr.updateSamplingRate(rate);
        if (pathtrace) {
            vr.setTechnique(VolumeRenderCL::TECH_PATHTRACE);
            vr.setExtinction(extinction);
        }
        if (mip) vr.setTechnique(VolumeRenderCL::TECH_MIP);
        if (iso) {
            vr.setTechnique(VolumeRenderCL::TECH_ISO);
            vr.setIsoValue(float(iso_value));
            vr.setIsoRefinement(unsigned(iso_refine));
        }
        if (tf2d_any) {
            std::vector<unsigned char> table2;
            unsigned nv = unsigned(tf2d_nv);
            if (tf2d) {
                std::ifstream f(tf2d_file, std::ios::binary);
                table2.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
                if (!f.good() && !f.eof()) table2.clear();
                if (table2.size() != size_t(4) * size_t(tf2d_nv) * size_t(tf2d_ng))
                    throw std::runtime_error("--tf2d: " + tf2d_file + " does not hold NV * NG RGBA8 entries");
            } else {
                nv = unsigned(table.size() / 4);
                table2 = VolumeRenderCL::rampTransferFunction2D(table, unsigned(tf2d_ng), float(tf2d_ghi), float(tf2d_g0),
                                                                float(tf2d_g1));
            }
            vr.setTechnique(VolumeRenderCL::TECH_TF2D);
            vr.setTransferFunction2D(table2, nv, unsigned(tf2d_ng), float(tf2d_ghi));
        }
        if (pin) vr.setSeed(seed);
        vr.updateOutputImg(W, H, 0);
        vr.updateView(have_view ? view : view_matrix(q, tr));
        return true;
        };
        // what segment s of the camera path has in force (transfer function, time step), on renderer vr
        auto apply_segment = [&](VolumeRenderCL &vr, size_t s) {
            std::vector<unsigned char> table = segs[s].tff ? *segs[s].tff : make_table();
            vr.setTransferFunction(table);
            vr.setTimestep(size_t(segs[s].timestep < 0 ? 0 : segs[s].timestep));
        };
        // launch sets of <= K frames per segment (one segment and no views without a path), as many per segment as a
        // multiple of `mult` renderers and all of (nearly) one size
        struct LaunchSet { std::vector<unsigned int> seeds; std::vector<std::array<float, 16>> views; size_t seg; };
        auto make_sets = [&](const std::vector<unsigned int> &seeds, size_t K, size_t mult) {
            std::vector<LaunchSet> sets;
            const size_t nseg = use_path ? segs.size() : 1;
            size_t f0 = 0;
            for (size_t sg = 0; sg < nseg; ++sg) {
                const size_t nf = use_path ? segs[sg].views.size() : seeds.size();
                size_t n_sets = (nf + K - 1) / K;
                n_sets = std::min(nf, (n_sets + mult - 1) / mult * mult);
                for (size_t i = 0; i < n_sets; ++i) {
                    const size_t lo = size_t(std::llround(double(i) * double(nf) / double(n_sets)));
                    const size_t hi = size_t(std::llround(double(i + 1) * double(nf) / double(n_sets)));
                    if (hi <= lo) continue;
                    LaunchSet ls;
                    ls.seeds.assign(seeds.begin() + long(f0 + lo), seeds.begin() + long(f0 + hi));
                    if (use_path) ls.views.assign(segs[sg].views.begin() + long(lo), segs[sg].views.begin() + long(hi));
                    ls.seg = sg;
                    sets.push_back(ls);
                }
                f0 += nf;
            }
            return sets;
        };

        if (mesh) {
            // ---- the isosurface as a file (VolumeRenderCL::extractIsosurface): the volume, the ESS switch, nothing else
            VolumeRenderCL vr;
            vr.initialize(false, false, VENDOR_ANY, std::to_string(device));
            if (!dat.empty()) {
                DatRawReader::Properties p;
                p.dat_file_name = dat;
                vr.setDeviceIngest(device_ingest);
                vr.loadVolumeData(p);
            } else {
                DatRawReader::data_format f = synth_fmt == "USHORT" ? DatRawReader::USHORT
                                              : synth_fmt == "FLOAT" ? DatRawReader::FLOAT : DatRawReader::UCHAR;
                vr.loadSyntheticVolume(synth_kind, synth_n, f);
            }
            vr.setObjEss(ess);
            if (have_timestep) vr.setTimestep(size_t(timestep));
            apply_filters(vr, filters);
            VolumeRenderCL::mesh_region region;
            if (have_mesh_region)
                for (size_t k = 0; k < 3; ++k) { region.lo[k] = unsigned(mesh_region[k]); region.hi[k] = unsigned(mesh_region[3 + k]); }
            if (mesh_indexed) {
                const VolumeRenderCL::welded_mesh im = vr.extractIsosurfaceIndexed(float(mesh_iso), mesh_normals, region);
                const size_t vertices = VolumeRenderCL::writePly(mesh_file, im);
                std::printf("{\"device\": \"%s\", \"mesh\": \"%s\", \"iso\": %.9g, \"triangles\": %zu, \"vertices\": %zu, "
                            "\"indexed\": true}\n",
                            vr.getCurrentDeviceName().c_str(), mesh_file.c_str(), mesh_iso, im.indices.size() / 3, vertices);
                return 0;
            }
            const VolumeRenderCL::iso_mesh m = vr.extractIsosurface(float(mesh_iso), mesh_normals, region);
            const size_t triangles = m.positions.size() / 9;
            if (mesh_ply) {
                const size_t vertices = VolumeRenderCL::writePly(mesh_file, m.positions, m.normals);
                std::printf("{\"device\": \"%s\", \"mesh\": \"%s\", \"iso\": %.9g, \"triangles\": %zu, \"vertices\": %zu}\n",
                            vr.getCurrentDeviceName().c_str(), mesh_file.c_str(), mesh_iso, triangles, vertices);
            } else {
                VolumeRenderCL::writeStl(mesh_file, m.positions);
                std::printf("{\"device\": \"%s\", \"mesh\": \"%s\", \"iso\": %.9g, \"triangles\": %zu}\n",
                            vr.getCurrentDeviceName().c_str(), mesh_file.c_str(), mesh_iso, triangles);
            }
            return 0;
        }
        if (stats) {
            // ---- what is in the volume (VolumeRenderCL::volumeStatistics): the volume, the ESS switch, nothing else
            VolumeRenderCL vr;
            vr.initialize(false, false, VENDOR_ANY, std::to_string(device));
            if (!dat.empty()) {
                DatRawReader::Properties p;
                p.dat_file_name = dat;
                vr.setDeviceIngest(device_ingest);
                vr.loadVolumeData(p);
            } else {
                DatRawReader::data_format f = synth_fmt == "USHORT" ? DatRawReader::USHORT
                                              : synth_fmt == "FLOAT" ? DatRawReader::FLOAT : DatRawReader::UCHAR;
                vr.loadSyntheticVolume(synth_kind, synth_n, f);
            }
            vr.setObjEss(ess);
            if (have_timestep) vr.setTimestep(size_t(timestep));
            apply_filters(vr, filters);
            VolumeRenderCL::stats_params sp;
            sp.vBins = unsigned(stats_bins[0]);
            sp.gBins = unsigned(stats_bins[1]);
            sp.vLo = float(stats_window[0]);
            sp.vHi = float(stats_window[1]);
            sp.gHi = float(stats_window[2]);
            sp.moments = stats_moments;
            if (have_stats_region)
                for (size_t k = 0; k < 3; ++k) { sp.region.lo[k] = unsigned(stats_region[k]); sp.region.hi[k] = unsigned(stats_region[3 + k]); }
            const VolumeRenderCL::volume_stats st = vr.volumeStatistics(sp);
            if (!write_stats_json(stats_file, sp, st)) throw std::runtime_error("cannot write " + stats_file);
            if (!stats_hist_file.empty()) {
                std::ofstream f(stats_hist_file, std::ios::binary);
                f.write(reinterpret_cast<const char *>(st.hist.data()), std::streamsize(st.hist.size() * sizeof(uint64_t)));
                if (!f) throw std::runtime_error("cannot write " + stats_hist_file);
            }
            std::printf("{\"device\": \"%s\", \"stats\": \"%s\", \"voxels\": %llu, \"binned\": %llu}\n",
                        vr.getCurrentDeviceName().c_str(), stats_file.c_str(), (unsigned long long)st.voxels,
                        (unsigned long long)st.binned);
            return 0;
        }
        if (ranks > 0) {
            // image-tile decomposition over `ranks` GPUs: one renderer per rank, every
            // one with the whole volume and the same settings; jitter seeds follow the same
            // default-seeded mt19937 sequence in every renderer, frame by frame
            if (img_ess) throw std::runtime_error("image-order ESS state crosses tile borders: not with --ranks");
            std::vector<std::unique_ptr<VolumeRenderCL>> vrs;
            std::vector<VolumeRenderCL *> ptrs;
            std::vector<int> devs;
            for (int r = 0; r < ranks; ++r) {
                vrs.emplace_back(new VolumeRenderCL());
                devs.push_back(loopback ? device : device + r);
                if (!setup(*vrs.back(), devs.back())) return 0;
                ptrs.push_back(vrs.back().get());
            }
            const bool batched = frames_per_launch > 0;
            if (batched && (pathtrace || img_ess || use_ao_flag))
                throw std::runtime_error("--frames-per-launch: ray caster only, no image-order ESS, no ambient occlusion");
            const size_t K = batched ? size_t(std::min(256, std::max(1, frames_per_launch))) : 0;
            TileGather tg(ptrs, devs, W, H, tile, loopback, force_gather, root_share, K);
            std::vector<float> frame, all_frames;
            double secs = 0.0;
            const std::array<float, 16> the_view = have_view ? view : view_matrix(q, tr);
            if (batched) {
                // the throughput path: K independent frames per exchange, one exchange in flight
                for (auto &v : vrs) { v->setRoundBudget(unsigned(round_budget)); v->setFrameTiming(false); }
                std::vector<std::vector<unsigned int>> sets;
                std::vector<std::vector<std::array<float, 16>>> set_views;   // (camera path: per set)
                std::vector<size_t> set_seg;
                std::vector<unsigned int> seeds = vrs[0]->drawSeeds(size_t(frames));
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
                    std::vector<unsigned int> ws(std::min(K, size_t(frames)));
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
                        for (auto &v : vrs) apply_segment(*v, set_seg[k]);
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
                secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                frame.erase(frame.begin(), frame.end() - long(W * H * 4));   // the last frame of the last batch
            } else {
                for (size_t sg = 0, in_seg = 0, f = 0; f < size_t(frames); ++f, ++in_seg) {
                    const std::array<float, 16> *pv = &the_view;
                    if (use_path) {   // frame f of the path: frame in_seg of segment sg
                        if (f == 0) for (auto &v : vrs) apply_segment(*v, 0);
                        if (in_seg == segs[sg].views.size()) {
                            ++sg;
                            in_seg = 0;
                            for (auto &v : vrs) apply_segment(*v, sg);
                        }
                        pv = &segs[sg].views[in_seg];
                    }
                    if (independent)
                        for (auto &v : vrs) v->updateView(*pv);   // (resets the running mean: iteration 0)
                    secs += tg.renderFrame(frame);
                    if (independent) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
                }
            }
            if (!all_frames.empty()) {
                std::ofstream af(out + ".frames.rgba.f32", std::ios::binary);
                af.write(reinterpret_cast<const char *>(all_frames.data()), std::streamsize(all_frames.size() * sizeof(float)));
            }
            std::ofstream raw(out + ".rgba.f32", std::ios::binary);
            raw.write(reinterpret_cast<const char *>(frame.data()), std::streamsize(frame.size() * sizeof(float)));
            write_ppm(out + ".ppm", frame, W, H);
            auto res = vrs[0]->getResolution();
            std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                        "\"frames\": %d, \"ranks\": %d, \"tile\": %zu, \"transport\": \"%s\", "
                        "\"frames_per_exchange\": %zu, \"independent\": %s, \"sent_bytes_per_frame\": %.0f, "
                        "\"dense_bytes_per_frame\": %.0f, \"frame_ms\": %.4f, \"ms_per_frame\": %.4f, "
                        "\"clock\": \"host, first submit to last assembled batch\", \"out\": \"%s.rgba.f32\"}\n",
                        vrs[0]->getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, frames, ranks, tile,
                        tg.transport().c_str(), K, (batched || independent) ? "true" : "false",
                        batched ? tg.sentBytes() / std::max(1, frames + (bench ? 2 * int(std::min(K, size_t(frames))) : 0)) : 0.0,
                        batched ? tg.denseBytes() / std::max(1, frames + (bench ? 2 * int(std::min(K, size_t(frames))) : 0)) : 0.0,
                        secs / frames * 1e3, secs / frames * 1e3, out.c_str());
            return 0;
        }

        VolumeRenderCL vr;
        if (!setup(vr, device)) return 0;
        std::vector<float> frame, all_frames;
        std::vector<unsigned char> frame8, all_frames8;   // --rgba8
        double kernel_s = 0.0;
        if (slicing) {
            // ---- slice views (VolumeRenderCL::renderSlices): the slices of the options in calls of <= 64, written like
            // the frames of --orbit
            const VolumeRenderCL::slice_mode mode = slab_mode == "min" ? VolumeRenderCL::SLICE_MIN
                                                    : slab_mode == "mean" ? VolumeRenderCL::SLICE_MEAN : VolumeRenderCL::SLICE_MAX;
            const VolumeRenderCL::slice_output output = slice_value ? VolumeRenderCL::SLICE_VALUE : VolumeRenderCL::SLICE_TF;
            VolumeRenderCL::slice_params sp;
            double nrm[3] = {0, 0, 0};   // the unit normal
            if (have_slice_axis) {
                sp = VolumeRenderCL::axisSlice(slice_axis, float(slice_pos), float(slab_t), unsigned(slab_n), mode, output);
                nrm[slice_axis] = 1.0;
            } else {
                std::memset(&sp, 0, sizeof sp);
                const double *u = slice_vec + 3, *v = slice_vec + 6;
                const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                const double l = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
                for (int k = 0; k < 3; ++k) {
                    nrm[k] = l > 0.0 ? c[k] / l : 0.0;
                    sp.origin[k] = float(slice_vec[k]);
                    sp.u[k] = float(u[k]);
                    sp.v[k] = float(v[k]);
                    sp.w[k] = float(slab_t * nrm[k]);
                }
                sp.samples = unsigned(slab_n);
                sp.mode = unsigned(mode);
                sp.output = unsigned(output);
            }
            std::vector<VolumeRenderCL::slice_params> slices{sp};
            if (have_stack) {
                // spanning the box along the normal: centred where the normal's line through the box centre meets the
                // plane's parallel through it, over the box's extent along the normal
                const double d = sp.origin[0] * nrm[0] + sp.origin[1] * nrm[1] + sp.origin[2] * nrm[2];
                VolumeRenderCL::slice_params base = sp;
                for (int k = 0; k < 3; ++k) base.origin[k] = float(double(sp.origin[k]) - d * nrm[k]);
                const double span = 2.0 * (std::fabs(nrm[0]) + std::fabs(nrm[1]) + std::fabs(nrm[2]));
                slices = VolumeRenderCL::sliceStack(base, unsigned(stack_n), float(span));
            }
            auto hip_ok = [](hipError_t e, const char *what) {
                if (e != hipSuccess) throw std::runtime_error(std::string("ERROR: ") + what + " (" + hipGetErrorString(e) + ")");
            };
            hip_ok(hipSetDevice(device), "hipSetDevice");
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
            frame.assign(all_frames.end() - long(px), all_frames.end());
            std::ofstream af(out + ".frames.rgba.f32", std::ios::binary);
            af.write(reinterpret_cast<const char *>(all_frames.data()), std::streamsize(all_frames.size() * sizeof(float)));
            std::ofstream raw(out + ".rgba.f32", std::ios::binary);
            raw.write(reinterpret_cast<const char *>(frame.data()), std::streamsize(frame.size() * sizeof(float)));
            write_ppm(out + ".ppm", frame, W, H);
            if (rgba8) {
                frame8.assign(all_frames8.end() - long(px), all_frames8.end());
                write_rgba8(out, frame8, all_frames8, W, H);
            }
            auto res = vr.getResolution();
            std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, \"slices\": %zu, "
                        "\"samples\": %d, \"mode\": \"%s\", \"output\": \"%s\", \"out\": \"%s.rgba.f32\"}\n",
                        vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, slices.size(), slab_n,
                        slab_mode.c_str(), slice_value ? "value" : "tf", out.c_str());
            return 0;
        }
        if (depth) {
            // ---- a depth image (VolumeRenderCL::renderDepth) of the options' camera
            const VolumeRenderCL::depth_mode mode = depth_mode == "max" ? VolumeRenderCL::DEPTH_MAX
                                                    : depth_mode == "opacity" ? VolumeRenderCL::DEPTH_OPACITY
                                                                              : VolumeRenderCL::DEPTH_ISO;
            VolumeRenderCL::depth_image d;
            std::array<unsigned int, 4> rect{{0, 0, 0, 0}};
            if (have_depth_rect) for (size_t k = 0; k < 4; ++k) rect[k] = unsigned(depth_rect[k]);
            vr.renderDepth(W, H, mode, float(depth_threshold), d, unsigned(depth_refine), rect);
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
            frame.assign(n * 4, 0.f);
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
                        vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, rect[0], rect[1], d.width, d.height,
                        depth_mode.c_str(), hits, t_lo, t_hi, out.c_str());
            return 0;
        }
        if (frames_per_launch > 0) {
            // ---- the throughput path on one GPU: F renderers over one shared volume take launch sets of <= K
            // independent frames in turn (what bench.py times; volumerenderwidget.cpp:464-486 is the one-frame-per-
            // paintGL caller this replaces for a caller that has many frames to render)
            if (pathtrace || img_ess || use_ao_flag)
                throw std::runtime_error("--frames-per-launch: ray caster only, no image-order ESS, no ambient occlusion");
            const size_t K = size_t(std::min(256, std::max(1, frames_per_launch)));
            // (a short run -- all the frames fit one launch set -- goes to ONE renderer as one set: two renderers with
            // half the frames each pay a set's ramp and tail side by side without hiding each other's; bench.py does
            // the same)
            const size_t F = size_t(frames) <= K ? 1 : size_t(std::max(1, frames_in_flight));
            std::vector<std::unique_ptr<VolumeRenderCL>> twins;
            std::vector<VolumeRenderCL *> lanes{&vr};
            vr.setRoundBudget(unsigned(round_budget));
            for (size_t j = 1; j < F; ++j) {
                twins.push_back(vr.shareVolumes());
                lanes.push_back(twins.back().get());
            }
            auto hip_ok = [](hipError_t e, const char *what) {
                if (e != hipSuccess) throw std::runtime_error(std::string("ERROR: ") + what + " (" + hipGetErrorString(e) + ")");
            };
            hip_ok(hipSetDevice(device), "hipSetDevice");
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
            // launch sets of <= K frames, as many as a multiple of the renderers and all of (nearly) one size (per
            // segment of a camera path: a set never crosses a change of transfer function or time step)
            const std::vector<LaunchSet> sets = make_sets(seeds, K, F);
            std::vector<size_t> lane_seg(F, 0);
            if (use_path)
                for (size_t j = 0; j < F; ++j) apply_segment(*lanes[j], 0);
            auto submit = [&](size_t j, const LaunchSet &ls, const std::vector<unsigned int> &sd) {
                if (use_path && lane_seg[j] != ls.seg) {
                    apply_segment(*lanes[j], ls.seg);   // (waits for the renderer's stream: its sets in flight)
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
            if (!all_frames.empty()) {
                std::ofstream af(out + ".frames.rgba.f32", std::ios::binary);
                af.write(reinterpret_cast<const char *>(all_frames.data()), std::streamsize(all_frames.size() * sizeof(float)));
            }
            std::ofstream raw(out + ".rgba.f32", std::ios::binary);
            raw.write(reinterpret_cast<const char *>(frame.data()), std::streamsize(frame.size() * sizeof(float)));
            write_ppm(out + ".ppm", frame, W, H);
            if (rgba8) {
                frame8.resize(W * H * 4);
                hip_ok(hipMemcpy(frame8.data(), blocks8[last % F] + (sets[last].seeds.size() - 1) * W * H * 4, frame8.size(),
                                 hipMemcpyDeviceToHost), "hipMemcpy");
                write_rgba8(out, frame8, all_frames8, W, H);
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
                        bench ? "" : " (frames copied to the host inside the region)", out.c_str());
            for (float *b : blocks) (void)hipFree(b);
            for (unsigned char *b : blocks8) (void)hipFree(b);
            (void)hipEventDestroy(ev0);
            (void)hipEventDestroy(ev1);
            for (auto &e : done) (void)hipEventDestroy(e);
            return 0;
        }
        const std::array<float, 16> the_view = have_view ? view : view_matrix(q, tr);
        if (pathtrace && !independent && !use_path && frames >= 1 && (samples_per_launch != 1 || bench)) {
            // the progressive image's N samples: in launch sets of K (VolumeRenderCL::renderSamples), or -- K = 1 under
            // --bench -- one launch per sample without the copy to the host between them.  The seeds are the ones the
            // per-sample loop below draws: the written image is the same bit for bit.
            const std::vector<unsigned int> seeds = vr.drawSeeds(size_t(frames));
            auto render = [&](bool to_host) {
                vr.updateView(the_view);   // iteration 0
                if (samples_per_launch == 1) {
                    for (size_t k = 0; k < seeds.size(); ++k) {
                        vr.setSeed(seeds[k]);
                        if (to_host && k + 1 == seeds.size()) vr.runRaycastNoGL(W, H, frame);
                        else vr.runRaycast(W, H);
                    }
                } else if (to_host) {
                    vr.renderSamples(W, H, seeds, frame, unsigned(samples_per_launch));
                } else {
                    vr.renderSamples(W, H, seeds, static_cast<float *>(nullptr), unsigned(samples_per_launch));
                }
            };
            double ms_per_sample = 0.0;
            if (bench) {
                auto hip_ok = [](hipError_t e, const char *what) {
                    if (e != hipSuccess) throw std::runtime_error(std::string("ERROR: ") + what + " (" + hipGetErrorString(e) + ")");
                };
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
            std::ofstream raw(out + ".rgba.f32", std::ios::binary);
            raw.write(reinterpret_cast<const char *>(frame.data()), std::streamsize(frame.size() * sizeof(float)));
            write_ppm(out + ".ppm", frame, W, H);
            if (rgba8) {   // the bytes of the image the frame buffer holds
                std::vector<unsigned char> frame8;
                vr.frameRGBA8(W, H, frame8);
                write_rgba8(out, frame8, std::vector<unsigned char>(), W, H);
            }
            auto res = vr.getResolution();
            std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                        "\"samples\": %d, \"samples_per_launch\": %u, \"sample_kernel\": %s, \"bench\": %s, "
                        "\"ms_per_sample\": %.5f, \"out\": \"%s.rgba.f32\"}\n",
                        vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, frames, li.frames,
                        li.samples ? "true" : "false", bench ? "true" : "false", ms_per_sample, out.c_str());
            return 0;
        }
        for (size_t sg = 0, in_seg = 0, f = 0; f < size_t(frames); ++f, ++in_seg) {
            const std::array<float, 16> *pv = &the_view;
            if (use_path) {   // frame f of the path: frame in_seg of segment sg
                if (f == 0) apply_segment(vr, 0);
                if (in_seg == segs[sg].views.size()) {
                    apply_segment(vr, ++sg);
                    in_seg = 0;
                }
                pv = &segs[sg].views[in_seg];
            }
            if (independent) vr.updateView(*pv);   // (resets the running mean: iteration 0, volumerendercl.cpp:379-390)
            vr.runRaycastNoGL(W, H, frame);   // frames accumulate (running mean), like the reference
            kernel_s += vr.getLastExecTime();
            if (independent) all_frames.insert(all_frames.end(), frame.begin(), frame.end());
            if (rgba8) {   // the same frame's bytes, quantised on the GPU from the frame buffer
                vr.frameRGBA8(W, H, frame8);
                if (independent) all_frames8.insert(all_frames8.end(), frame8.begin(), frame8.end());
            }
        }
        if (!all_frames.empty()) {
            std::ofstream af(out + ".frames.rgba.f32", std::ios::binary);
            af.write(reinterpret_cast<const char *>(all_frames.data()), std::streamsize(all_frames.size() * sizeof(float)));
        }
        std::ofstream raw(out + ".rgba.f32", std::ios::binary);
        raw.write(reinterpret_cast<const char *>(frame.data()), std::streamsize(frame.size() * sizeof(float)));
        write_ppm(out + ".ppm", frame, W, H);
        if (rgba8) write_rgba8(out, frame8, all_frames8, W, H);
        auto res = vr.getResolution();
        std::printf("{\"device\": \"%s\", \"volume\": [%u, %u, %u], \"width\": %zu, \"height\": %zu, "
                    "\"frames\": %d, \"kernel_ms_per_frame\": %.4f, \"out\": \"%s.rgba.f32\"}\n",
                    vr.getCurrentDeviceName().c_str(), res[0], res[1], res[2], W, H, frames,
                    kernel_s / frames * 1e3, out.c_str());
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

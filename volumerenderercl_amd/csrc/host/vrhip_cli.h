// The options of vrhip_render: one struct with a sub-struct per option group, the parser that fills it and the
// cross-option refusals.  Nothing here opens a device or creates a renderer, so this unit compiles and runs without a
// GPU (tests/cxx/cli_args_main.cpp runs it under the host sanitizers).
#pragma once

#include <array>
#include <string>
#include <vector>

#include "volumerendercl.h"

// --filter: one entry per occurrence, in the order given
struct FilterSpec {
    enum { GAUSS, MEDIAN, TAPS } kind = GAUSS;
    double sigma = 1.0;
    unsigned radius = 0;                    // GAUSS: 0 = by sigma
    VolumeRenderCL::FilterParams taps;      // TAPS
};

// --morph: one entry per occurrence, in the order given
struct MorphSpec {
    VolumeRenderCL::MorphParams params;
};

// --filter and --morph run in command-line order: entry k of that order is filters[index] or morphs[index]
struct VolumeStep {
    bool morph = false;
    size_t index = 0;
};

struct Options {
    struct Volume {      // volume source (--dat, --synth, --device-ingest, --downsample, --timestep)
        std::string dat, synth_kind, synth_fmt = "UCHAR";
        unsigned synth_n = 0;
        bool device_ingest = false, have_timestep = false;
        int downsample = 0;
        long timestep = 0;
    } volume;
    struct View {        // view / camera (--size, --rotate, --translate, --view, --state, --camera-path, --orbit)
        size_t W = 1024, H = 1024;
        double q[4] = {1, 0, 0, 0}, tr[3] = {0, 0, 2};
        bool have_view = false, have_path_arg = false, have_orbit = false;
        std::array<float, 16> view{};
        std::string state_file, camera_path;
        double orbit_axis[3] = {0, 1, 0};
        int orbit_n = 0;
    } view;
    struct Render {      // common rendering (--tf*, --illum, --rate, --bg, --seed, --env and the switches)
        std::string tf = "default", tf_stops, tf_easing = "linear", env_file;
        unsigned illum = 1, seed = 0;
        bool pin = false;   // --seed was given
        bool ess = true, ortho = false, linear = true, gradient_bg = false;
        bool contours = false, aerial = false, ao = false, show_ess = false, img_ess = false;
        double rate = 1.5;
        std::array<float, 4> bg = {{1, 1, 1, 1}};
    } render;
    struct Technique {   // --pathtrace, --extinction, --mip, --iso, --iso-refine, --preint
        bool pathtrace = false, mip = false, iso = false, have_iso_refine = false, preint = false;
        double extinction = 100.0, iso_value = 0.5;
        int iso_refine = 4;
    } tech;
    struct Tf2d {        // technique 6 (--tf2d FILE NV NG GHI, --tf2d-ramp NG GHI G0 G1)
        bool table = false, ramp = false;
        std::string file;
        long nv = 0, ng = 0;
        double ghi = 0.0, g0 = 0.0, g1 = 0.0;
        bool any() const { return table || ramp; }
    } tf2d;
    struct Slice {       // slice views (--slice-axis / --slice, --slab, --slice-stack, --slice-value)
        bool have_axis = false, have_plane = false, have_slab = false, have_stack = false, value = false;
        int axis = 2, slab_n = 1, stack_n = 0;
        double pos = 0.0, vec[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, slab_t = 0.0;
        std::string slab_mode = "max";
        bool any() const { return have_axis || have_plane; }
    } slice;
    struct Depth {       // depth images (--depth, --depth-refine, --depth-rect)
        bool on = false, have_refine = false, have_rect = false;
        std::string mode;
        double threshold = 0.5;
        int refine = 4;
        long rect[4] = {0, 0, 0, 0};
    } depth;
    struct Mesh {        // isosurface extraction (--mesh, --mesh-normals, --mesh-region, --mesh-indexed)
        bool on = false, normals = false, have_region = false, indexed = false;
        double iso = 0.5;
        std::string file;
        long region[6] = {0, 0, 0, 0, 0, 0};
        std::string ext() const { const size_t dot = file.rfind('.'); return dot == std::string::npos ? "" : file.substr(dot); }
    } mesh;
    struct Stats {       // volume statistics (--stats, --stats-bins, --stats-window, --stats-region, --stats-moments, --stats-hist)
        bool on = false, have_opt = false, have_region = false, moments = false;
        std::string file, hist_file;
        long bins[2] = {256, 1}, region[6] = {0, 0, 0, 0, 0, 0};
        double window[3] = {0.0, 1.0, 1.0};
    } stats;
    std::vector<FilterSpec> filters;   // --filter
    std::vector<MorphSpec> morphs;     // --morph
    std::vector<VolumeStep> steps;     // the two in command-line order
    struct Batch {       // batching / launch sets (--frames, --independent, --frames-per-launch ..., --samples-per-launch, --bench)
        int frames = 1, frames_per_launch = 0, frames_in_flight = 2, round_budget = 48, samples_per_launch = 0;
        bool independent = false, bench = false;
    } batch;
    struct Ranks {       // devices, ranks / tiles (--device, --ranks, --tile, --loopback, --force-gather, --root-share)
        int device = 0, n = 0;
        size_t tile = 64;
        bool loopback = false, force_gather = false;
        double root_share = 1.0;
    } ranks;
    struct Out {         // outputs (--out, --rgba8, --dump-tf, --dump-views)
        std::string prefix, dump_tf, dump_views;
        bool rgba8 = false;
    } out;
};

[[noreturn]] void usage();                        // the usage text to stderr, exit status 2
Options parse_args(int argc, char **argv);        // the option chain and nothing else
void validate(const Options &o);                  // the refusals that need the options alone
void validate_easing(const Options &o);           // --tf-easing: after the camera path is read (see validate)
void validate_source_and_output(const Options &o);   // --dat / --synth and --out: after --dump-views and --dump-tf

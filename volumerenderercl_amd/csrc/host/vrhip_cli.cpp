// vrhip_render's command line: the usage text, parse_args and the refusals (vrhip_cli.h).  No device is opened here.
#include "vrhip_cli.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

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
        "         [--preint]                       (technique 8, pre-integrated classification: the slab between two\n"
        "                                           samples is coloured by the transfer function integrated over the\n"
        "                                           values in between, so a narrow peak is never stepped over; the\n"
        "                                           command's 1-D table (--tf); --illum 0 or 1; independent frames like\n"
        "                                           --mip; combines with --orbit, --camera-path, --frames-per-launch and\n"
        "                                           --rgba8; not with --pathtrace, --mip, --iso, --tf2d, --tf2d-ramp, --ao,\n"
        "                                           --show-ess, --img-ess, --env, --ranks)\n"
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
        "         [--morph OP box|ball RX RY RZ]   (grey-scale morphology of the loaded time step on the device, in place:\n"
        "                                           OP erode, dilate, open, close, gradient, tophat or blackhat; the\n"
        "                                           structuring element a box or a ball of radius 0-8 voxels per axis;\n"
        "                                           repeatable; --filter and --morph steps run in command-line order,\n"
        "                                           under the rules of --filter)\n"
        "writes PREFIX.rgba.f32 (W*H*4 float32, row 0 = top), PREFIX.ppm and prints one JSON line\n";
    std::exit(2);
}

namespace {

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

} // namespace

Options parse_args(int argc, char **argv)
{
    Options o;
    Options::Volume &vol = o.volume;
    Options::View &vw = o.view;
    Options::Render &rn = o.render;
    Options::Technique &te = o.tech;
    Options::Tf2d &t2 = o.tf2d;
    Options::Slice &sl = o.slice;
    Options::Depth &de = o.depth;
    Options::Mesh &me = o.mesh;
    Options::Stats &st = o.stats;
    Options::Batch &ba = o.batch;
    Options::Ranks &rk = o.ranks;
    auto need = [&](int i, int n) { if (i + n >= argc) usage(); };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto num = [&]() { return std::atof(argv[++i]); };        // the next argument as a double, an int, a long
        auto integer = [&]() { return std::atoi(argv[++i]); };
        auto lng = [&]() { return std::atol(argv[++i]); };
        if (a == "--dat") { need(i, 1); vol.dat = argv[++i]; }
        else if (a == "--synth") { need(i, 3); vol.synth_kind = argv[++i]; vol.synth_n = unsigned(integer()); vol.synth_fmt = argv[++i]; }
        else if (a == "--device-ingest") vol.device_ingest = true;
        else if (a == "--downsample") { need(i, 1); vol.downsample = integer(); }
        else if (a == "--timestep") { need(i, 1); vol.timestep = lng(); vol.have_timestep = true; }
        else if (a == "--size") { need(i, 2); vw.W = size_t(lng()); vw.H = size_t(lng()); }
        else if (a == "--rotate") {
            need(i, 4);
            double ax = num(), ay = num(), az = num();
            double half = num() * M_PI / 360.0, l = std::sqrt(ax * ax + ay * ay + az * az);
            vw.q[0] = std::cos(half); vw.q[1] = ax / l * std::sin(half); vw.q[2] = ay / l * std::sin(half); vw.q[3] = az / l * std::sin(half);
        }
        else if (a == "--translate") { need(i, 3); for (double &c : vw.tr) c = num(); }
        else if (a == "--view") { need(i, 16); for (float &c : vw.view) c = float(num()); vw.have_view = true; }
        else if (a == "--state") { need(i, 1); vw.state_file = argv[++i]; }
        else if (a == "--camera-path") { need(i, 1); vw.camera_path = argv[++i]; vw.have_path_arg = true; }
        else if (a == "--orbit") { need(i, 4); for (double &c : vw.orbit_axis) c = num(); vw.orbit_n = integer(); vw.have_orbit = true; }
        else if (a == "--tf") { need(i, 1); rn.tf = argv[++i]; }
        else if (a == "--tf-stops") { need(i, 1); rn.tf_stops = argv[++i]; }
        else if (a == "--tf-easing") { need(i, 1); rn.tf_easing = argv[++i]; }
        else if (a == "--illum") { need(i, 1); rn.illum = unsigned(integer()); }
        else if (a == "--no-ess") rn.ess = false;
        else if (a == "--ortho") rn.ortho = true;
        else if (a == "--nearest") rn.linear = false;
        else if (a == "--gradient-bg") rn.gradient_bg = true;
        else if (a == "--rate") { need(i, 1); rn.rate = num(); }
        else if (a == "--bg") { need(i, 3); for (size_t k = 0; k < 3; ++k) rn.bg[k] = float(num()); }
        else if (a == "--seed") { need(i, 1); rn.seed = unsigned(std::strtoul(argv[++i], nullptr, 10)); rn.pin = true; }
        else if (a == "--contours") rn.contours = true;
        else if (a == "--aerial") rn.aerial = true;
        else if (a == "--ao") rn.ao = true;
        else if (a == "--show-ess") rn.show_ess = true;
        else if (a == "--img-ess") rn.img_ess = true;
        else if (a == "--env") { need(i, 1); rn.env_file = argv[++i]; }
        else if (a == "--pathtrace") te.pathtrace = true;
        else if (a == "--extinction") { need(i, 1); te.extinction = num(); }
        else if (a == "--mip") te.mip = true;
        else if (a == "--preint") te.preint = true;
        else if (a == "--iso") { need(i, 1); te.iso = true; te.iso_value = num(); }
        else if (a == "--iso-refine") { need(i, 1); te.have_iso_refine = true; te.iso_refine = integer(); }
        else if (a == "--tf2d") { need(i, 4); t2.table = true; t2.file = argv[++i]; t2.nv = lng(); t2.ng = lng(); t2.ghi = num(); }
        else if (a == "--tf2d-ramp") { need(i, 4); t2.ramp = true; t2.ng = lng(); t2.ghi = num(); t2.g0 = num(); t2.g1 = num(); }
        else if (a == "--slice-axis") {
            need(i, 2);
            const std::string ax = argv[++i];
            sl.axis = ax == "X" || ax == "x" ? 0 : ax == "Y" || ax == "y" ? 1 : ax == "Z" || ax == "z" ? 2 : -1;
            sl.pos = num();
            sl.have_axis = true;
        }
        else if (a == "--slice") { need(i, 9); for (double &c : sl.vec) c = num(); sl.have_plane = true; }
        else if (a == "--slab") { need(i, 3); sl.slab_t = num(); sl.slab_n = integer(); sl.slab_mode = argv[++i]; sl.have_slab = true; }
        else if (a == "--slice-stack") { need(i, 1); sl.stack_n = integer(); sl.have_stack = true; }
        else if (a == "--slice-value") sl.value = true;
        else if (a == "--depth") {
            need(i, 1);
            de.on = true;
            de.mode = argv[++i];
            if (de.mode == "iso" || de.mode == "opacity") { need(i, 1); de.threshold = num(); }
        }
        else if (a == "--depth-refine") { need(i, 1); de.have_refine = true; de.refine = integer(); }
        else if (a == "--depth-rect") { need(i, 4); for (long &c : de.rect) c = lng(); de.have_rect = true; }
        else if (a == "--mesh") { need(i, 2); me.on = true; me.iso = num(); me.file = argv[++i]; }
        else if (a == "--mesh-normals") me.normals = true;
        else if (a == "--mesh-indexed") me.indexed = true;
        else if (a == "--mesh-region") { need(i, 6); for (long &c : me.region) c = lng(); me.have_region = true; }
        else if (a == "--stats") { need(i, 1); st.on = true; st.file = argv[++i]; }
        else if (a == "--stats-bins") { need(i, 2); for (long &c : st.bins) c = lng(); st.have_opt = true; }
        else if (a == "--stats-window") { need(i, 3); for (double &c : st.window) c = num(); st.have_opt = true; }
        else if (a == "--stats-region") { need(i, 6); for (long &c : st.region) c = lng(); st.have_opt = st.have_region = true; }
        else if (a == "--stats-moments") st.have_opt = st.moments = true;
        else if (a == "--stats-hist") { need(i, 1); st.hist_file = argv[++i]; st.have_opt = true; }
        else if (a == "--filter") {
            need(i, 1);
            const std::string what = argv[++i];
            FilterSpec fs;
            if (what == "gauss") {
                need(i, 1);
                fs.kind = FilterSpec::GAUSS;
                fs.sigma = num();
                if (!(std::isfinite(fs.sigma) && fs.sigma > 0.0)) usage();
                if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {   // (an option starts with '-')
                    const long rad = lng();
                    if (rad < 1 || rad > 8) usage();
                    fs.radius = unsigned(rad);
                }
            } else if (what == "median") fs.kind = FilterSpec::MEDIAN;
            else if (what == "taps") {
                need(i, 1);
                fs.kind = FilterSpec::TAPS;
                if (!read_filter_taps(argv[++i], fs.taps)) {
                    std::fprintf(stderr, "--filter taps: %s does not hold three lines of 1 to 9 finite weights\n", argv[i]);
                    std::exit(2);
                }
            } else usage();
            o.steps.push_back(VolumeStep{false, o.filters.size()});
            o.filters.push_back(fs);
        }
        else if (a == "--morph") {
            need(i, 5);
            static const char *const ops[] = {"erode", "dilate", "open", "close", "gradient", "tophat", "blackhat"};
            const std::string op = argv[++i], shape = argv[++i];
            MorphSpec ms;
            size_t k = 0;
            while (k < 7 && op != ops[k]) ++k;
            if (k == 7 || (shape != "box" && shape != "ball")) usage();
            ms.params.op = VolumeRenderCL::MorphOp(k);
            ms.params.ball = shape == "ball";
            for (size_t ax = 0; ax < 3; ++ax) {
                const char *text = argv[++i];
                char *end = nullptr;
                const long rad = std::strtol(text, &end, 10);
                if (end == text || *end || rad < 0 || rad > 8) usage();
                ms.params.radius[ax] = unsigned(rad);
            }
            o.steps.push_back(VolumeStep{true, o.morphs.size()});
            o.morphs.push_back(ms);
        }
        else if (a == "--frames") { need(i, 1); ba.frames = integer(); }
        else if (a == "--independent") ba.independent = true;
        else if (a == "--bench") ba.bench = true;
        else if (a == "--frames-per-launch") { need(i, 1); ba.frames_per_launch = integer(); }
        else if (a == "--samples-per-launch") { need(i, 1); ba.samples_per_launch = integer(); if (ba.samples_per_launch < 0) usage(); }
        else if (a == "--frames-in-flight") { need(i, 1); ba.frames_in_flight = integer(); }
        else if (a == "--round-budget") { need(i, 1); ba.round_budget = integer(); }
        else if (a == "--device") { need(i, 1); rk.device = integer(); }
        else if (a == "--ranks") { need(i, 1); rk.n = integer(); }
        else if (a == "--tile") { need(i, 1); rk.tile = size_t(lng()); }
        else if (a == "--loopback") rk.loopback = true;
        else if (a == "--force-gather") rk.force_gather = true;
        else if (a == "--root-share") { need(i, 1); rk.root_share = num(); }
        else if (a == "--out") { need(i, 1); o.out.prefix = argv[++i]; }
        else if (a == "--rgba8") o.out.rgba8 = true;
        else if (a == "--dump-tf") { need(i, 1); o.out.dump_tf = argv[++i]; }
        else if (a == "--dump-views") { need(i, 1); o.out.dump_views = argv[++i]; }
        else usage();
    }
    return o;
}

// The refusals, in the order they have always been applied: the first that fails decides the message and the exit
// status.  All of them run before a device is opened; the ones that need a renderer are not here but with the mode
// that makes them (vrhip_render.cpp):
//   before VolumeRenderCL::initialize():
//     - while parsing: a missing argument, an unknown option, --samples-per-launch < 0, a --filter that is malformed
//       or whose taps file is (its own message, status 2)
//     - validate(): every check below
//     - the camera path is read (--camera-path / --orbit; status 1 with the reader's message), --dump-views writes
//       and ends the run; a path with --pathtrace or --img-ess is refused (status 1)
//     - validate_easing(); --dump-tf writes and ends the run; validate_source_and_output()
//     - --ranks with --img-ess (status 1)
//   after initialize() and the volume's load, as exceptions (status 1): --frames-per-launch with --pathtrace,
//   --img-ess or --ao; a --tf2d file of the wrong size; whatever the library refuses.
void validate(const Options &o)
{
    const Options::View &vw = o.view;
    const Options::Render &rn = o.render;
    const Options::Technique &te = o.tech;
    const Options::Tf2d &t2 = o.tf2d;
    const Options::Slice &sl = o.slice;
    const Options::Depth &de = o.depth;
    const Options::Mesh &me = o.mesh;
    const Options::Stats &st = o.stats;
    const Options::Batch &ba = o.batch;
    const int ranks = o.ranks.n;
    const bool ray_caster_extras = rn.ao || rn.show_ess || rn.img_ess || !rn.env_file.empty();
    if (vw.have_path_arg && (vw.camera_path.empty() || vw.have_orbit)) usage();
    if (te.mip && te.pathtrace) usage();
    if (te.iso && (te.pathtrace || te.mip || ray_caster_extras)) usage();
    if (te.have_iso_refine && (!te.iso || te.iso_refine < 0 || te.iso_refine > 16)) usage();
    if (t2.any()) {
        if (t2.table && t2.ramp) usage();
        if (te.pathtrace || te.mip || te.iso || ray_caster_extras || ranks > 0) usage();
        if (t2.table && (t2.file.empty() || t2.nv < 1 || t2.nv > long(VRHIP_TF2D_MAX_NV))) usage();
        if (t2.ng < 1 || t2.ng > long(VRHIP_TF2D_MAX_NG) || (t2.table && t2.nv * t2.ng > long(VRHIP_TF2D_MAX_ENTRIES))) usage();
        if (!std::isfinite(t2.ghi) || !(float(t2.ghi) > 0.f)) usage();
        if (t2.ramp && (!std::isfinite(t2.g0) || !std::isfinite(t2.g1) || !(float(t2.g0) >= 0.f) || !(float(t2.g1) > float(t2.g0))))
            usage();
    }
    // (--ranks: refused like technique 6's options, not wired through the C++ tile gather)
    if (te.preint && (te.pathtrace || te.mip || te.iso || t2.any() || ray_caster_extras || ranks > 0)) usage();
    if (o.out.rgba8 && ranks > 0) {
        std::cerr << "--rgba8 cannot be combined with --ranks: the C++ tile gather carries float pixels "
                     "(8-bit frames over several GPUs: the Python TileDriver, pixel_format=\"rgba8\")" << std::endl;
        std::exit(2);
    }
    const bool slice_opt = sl.have_slab || sl.have_stack || sl.value;
    if (slice_opt && !sl.any()) usage();
    if (sl.any()) {
        if (sl.have_axis && sl.have_plane) usage();
        if (te.mip || te.iso || t2.any() || te.preint || te.pathtrace || vw.have_orbit || vw.have_path_arg || ranks > 0) usage();
        if (sl.have_axis && (sl.axis < 0 || !std::isfinite(sl.pos))) usage();
        for (double c : sl.vec) if (!std::isfinite(c)) usage();
        if (sl.have_slab && (sl.slab_n < 1 || sl.slab_n > int(VRHIP_SLICE_MAX_SAMPLES) || !std::isfinite(sl.slab_t) ||
                             (sl.slab_mode != "max" && sl.slab_mode != "min" && sl.slab_mode != "mean")))
            usage();
        if (sl.have_stack && (sl.stack_n < 1 || sl.stack_n > 1 << 16)) usage();
        if (sl.have_plane && (sl.have_slab || sl.have_stack)) {   // these need the plane's normal
            const double *u = sl.vec + 3, *v = sl.vec + 6;
            const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            if (n[0] * n[0] + n[1] * n[1] + n[2] * n[2] == 0.0) usage();
        }
    }
    // what asks for several frames, or for a frame's own state: one depth image, a mesh or statistics have nothing
    // for it to act on
    const bool many_frames = vw.have_orbit || vw.have_path_arg || ba.frames != 1 || o.out.rgba8 || rn.img_ess;
    if ((de.have_refine || de.have_rect) && !de.on) usage();
    if (de.on) {
        if (de.mode != "iso" && de.mode != "max" && de.mode != "opacity") usage();
        if (te.pathtrace || te.mip || te.iso || t2.any() || te.preint || sl.any() || slice_opt || ranks > 0 || ba.frames_per_launch > 0)
            usage();
        if (many_frames) usage();
        if (!std::isfinite(de.threshold) || de.refine < 0 || de.refine > 16) usage();
        if (de.have_rect) {
            for (long c : de.rect) if (c < 0 || c > 16384) usage();
            if (de.rect[2] < 1 || de.rect[3] < 1 || de.rect[0] + de.rect[2] > long(vw.W) || de.rect[1] + de.rect[3] > long(vw.H))
                usage();
        }
    }
    if ((me.normals || me.have_region || me.indexed) && !me.on) usage();
    if (o.volume.have_timestep && !me.on && !st.on) usage();
    if (st.have_opt && !st.on) usage();
    if ((!o.filters.empty() || !o.morphs.empty()) && (ranks > 0 || o.volume.downsample)) usage();
    // numbers about the volume (--stats) or triangles of it (--mesh), not a picture: what selects, shapes or
    // multiplies frames has nothing to act on
    const bool a_picture = te.pathtrace || te.mip || te.iso || t2.any() || te.preint || te.have_iso_refine || sl.any() || slice_opt || de.on ||
                           ranks > 0 || ba.frames_per_launch > 0 || many_frames || o.volume.downsample || !o.out.dump_tf.empty() ||
                           ba.bench || ba.independent;
    if (st.on) {
        if (me.on || a_picture) usage();
        if (st.file.empty() || o.volume.timestep < 0) usage();
        if (st.bins[0] < 1 || st.bins[0] > 4096 || st.bins[1] < 1 || st.bins[1] > 256 || st.bins[0] * st.bins[1] > 65536) usage();
        if (!std::isfinite(st.window[0]) || !std::isfinite(st.window[1]) || !(float(st.window[1]) > float(st.window[0]))) usage();
        if (st.bins[1] > 1 && (!std::isfinite(st.window[2]) || !(float(st.window[2]) > 0.f))) usage();
        for (long c : st.region) if (c < 0 || c > 8192) usage();
    }
    if (me.on) {
        if (me.ext() != ".stl" && me.ext() != ".ply") usage();
        if (me.indexed && me.ext() != ".ply") usage();   // (STL is a triangle list)
        if (a_picture) usage();
        if (!std::isfinite(me.iso) || o.volume.timestep < 0) usage();
        for (long c : me.region) if (c < 0 || c > 8192) usage();
    }
    if (vw.have_orbit && (vw.orbit_n < 1 || vw.orbit_n > 1 << 20 ||
                          vw.orbit_axis[0] * vw.orbit_axis[0] + vw.orbit_axis[1] * vw.orbit_axis[1] +
                                  vw.orbit_axis[2] * vw.orbit_axis[2] == 0.0))
        usage();
    if (!o.out.dump_views.empty() && !vw.have_path_arg && !vw.have_orbit) usage();
}

void validate_easing(const Options &o)
{
    const std::string &e = o.render.tf_easing;
    if (e != "linear" && e != "quad" && e != "cubic") usage();
}

void validate_source_and_output(const Options &o)
{
    if (o.volume.dat.empty() && o.volume.synth_kind.empty()) usage();
    if (o.out.prefix.empty() && !o.volume.downsample && !o.mesh.on && !o.stats.on) usage();
}

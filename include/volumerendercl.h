// volumerendercl.h -- host-side C++ class with the public surface of the reference's
// `VolumeRenderCL` (/root/reference/src/core/volumerendercl.h:39-482), implemented on the
// C ABI of libvrhip.so (include/vrhip.h).  A caller of the reference class
// (volumerenderwidget.cpp) compiles against this header unchanged for the ray-cast path:
// same method names, argument meaning, call order and exception types.
//
// Differences, all deliberate:
//  * OpenCL types that leaked into the interface have local stand-ins (cl_vendor, cl_GLuint);
//  * runRaycastNoGL fills width*height*4 fp32 RGBA, row 0 = top, as documented there (:173)
//    (the reference reads an UNORM8 image into that vector);
//  * frames accumulate in fp32 and `iteration` advances in both run paths (C9, C10);
//  * ARGB / BGRA volumes (uploaded by the reference, never handled by its kernel) throw
//    std::runtime_error;
//  * `buildScaledVol` (declared but never defined in the reference, :221) is dropped.
#pragma once

#include <array>
#include <memory>
#include <random>
#include <string>
#include <valarray>
#include <vector>

#include "vrhip.h"
#include "datrawreader.h"

typedef unsigned int uint;
typedef unsigned int cl_GLuint;
// openclutilities.h:56-62
enum cl_vendor { VENDOR_ANY, VENDOR_NVIDIA, VENDOR_AMD, VENDOR_INTEL };

class VolumeRenderCL
{
public:
    typedef vrhip_camera_params camera_params;
    typedef vrhip_rendering_params rendering_params;
    typedef vrhip_raycast_params raycast_params;
    typedef vrhip_pathtrace_params pathtrace_params;

    enum kernel_arg {
        VOLUME = 0, BRICKS = 1, TFF = 2, OUTPUT, TFF_PREFIX, IN_ACCUMULATE, OUT_ACCUMULATE,
        IN_HIT_IMG, OUT_HIT_IMG, ENVIRONMENT, CAMERA, RENDERING, RAYCAST, PATHTRACE
    };
    enum scaling_metric { MIN = 0, MAX, AVG, DENSITY };
    // TECH_MIP: maximum intensity projection (VRHIP_TECHNIQUE_MIP, vrhip.h; no reference counterpart)
    // TECH_ISO: first-hit isosurface (VRHIP_TECHNIQUE_ISO, vrhip.h; no reference counterpart; 3 is unassigned)
    // TECH_TF2D: ray casting through a 2-D transfer function (VRHIP_TECHNIQUE_TF2D, vrhip.h; no reference counterpart;
    //   5 is unassigned)
    // TECH_PREINT: ray casting with pre-integrated classification of the 1-D transfer function
    //   (VRHIP_TECHNIQUE_PREINT, vrhip.h; no reference counterpart; 7 is unassigned)
    enum technique { TECH_RAYCAST = 0, TECH_PATHTRACE = 1, TECH_MIP = 2, TECH_ISO = 4, TECH_TF2D = 6, TECH_PREINT = 8 };

    VolumeRenderCL();
    ~VolumeRenderCL();
    VolumeRenderCL(const VolumeRenderCL &) = delete;
    VolumeRenderCL &operator=(const VolumeRenderCL &) = delete;

    // useGL / useCPU / vendor / platformId select OpenCL plumbing that does not exist here;
    // useCPU throws (there is no CPU path); deviceName "N" or platformId >= 0 pick HIP device N.
    void initialize(bool useGL = false, bool useCPU = false, cl_vendor vendor = VENDOR_ANY,
                    const std::string deviceName = "", const int platformId = -1);
    void updateView(const std::array<float, 16> viewMat);
    void updateSamplingRate(const double samplingRate);
    void updateOutputImg(const size_t width, const size_t height, cl_GLuint texId);
    void runRaycast(const size_t width, const size_t height);
    void runRaycastNoGL(const size_t width, const size_t height, std::vector<float> &output);
    size_t loadVolumeData(const DatRawReader::Properties volumeFileProps);
    bool hasData() const;
    const std::array<unsigned int, 4> getResolution() const;
    void setTransferFunction(std::vector<unsigned char> &tff);
    void setTffPrefixSum(std::vector<unsigned int> &tffPrefixSum);
    void scaleVolume(std::valarray<float> scale);

    void setCamOrtho(bool setCamOrtho);
    void setIllumination(unsigned int illum);
    void setShowESS(bool showESS);
    void setLinearInterpolation(bool linearSampling);
    void setContours(bool contours);
    void setAerial(bool aerial);
    void setImgEss(bool useEss);
    void setObjEss(bool useEss);
    void setBackground(std::array<float, 4> color);
    double getLastExecTime();
    const std::vector<std::string> getPlatformNames();
    const std::vector<std::string> getDeviceNames(size_t platformId, const std::string &type);
    const std::string getCurrentDeviceName();
    void setAmbientOcclusion(bool ao);
    const std::string volumeDownsampling(const size_t t, const int factor);
    const std::array<double, 256> &getHistogram(unsigned int timestep = 0);
    void createEnvironmentMap(const std::string &file_name);
    void setUseGradient(bool useGradient);
    void setTechnique(technique tech);
    void setExtinction(const double extinction);
    // TECH_ISO (no reference counterpart): the threshold, in the units of the transfer function's coordinate (default
    // 0.5), and the bisection rounds that refine the hit (0-16, default 4); vrhip_iso_params
    void setIsoValue(float isoValue);
    void setIsoRefinement(unsigned int refineSteps);
    // TECH_TF2D (no reference counterpart): the n_v x n_g RGBA8 table, value fastest, and the gradient magnitude of
    // its upper edge (vrhip_set_transfer_function_2d; the gHi of volumeStatistics' histogram).  Throws on a table of
    // another size than 4 * nV * nG bytes.
    void setTransferFunction2D(const std::vector<unsigned char> &table, unsigned int nV, unsigned int nG, float gHi);
    // ... and the one such table to be had without an editor: the rows are `tff` (4 * nV bytes), their alpha scaled by
    // a ramp over the gradient magnitude that is 0 up to g0 and 1 from g1 on (vrhip_tf2d_build_ramp).  Host only.
    static std::vector<unsigned char> rampTransferFunction2D(const std::vector<unsigned char> &tff, unsigned int nG,
                                                             float gHi, float g0, float g1);
    // TECH_PREINT (no parameters of its own): the classification of the slab between the sample values sf (front) and
    // sb (back) with the RGBA8 table `tff`: (Cbar.rgb, abar) (vrhip_preint_slab).  raw: a FLOAT volume's values.  Host
    // only.  Throws on a table that is empty, above 4096 entries or no multiple of 4 bytes, or a refused value.
    static std::array<float, 4> preintSlab(const std::vector<unsigned char> &tff, float sf, float sb, bool raw = false);
    void setBBox(float bl_x, float bl_y, float bl_z, float tr_x, float tr_y, float tr_z);
    void setTimestep(const size_t t);

    // ---- additions for the headless / multi-GPU host (no reference counterpart)
    // Synthetic input of SURVEY 8(d) generated in HBM: kind "sphere" | "shells".
    void loadSyntheticVolume(const std::string &kind, unsigned int res, DatRawReader::data_format f);
    // Image tiles: compact device buffer [n][tile_h][tile_w][4].
    void renderTiles(size_t width, size_t height, size_t tile_w, size_t tile_h,
                     const std::vector<unsigned int> &tile_ids, float *out_tiles_dev,
                     bool advanceIteration = false);   // true: the frame counts for the running mean (:540)
    // Device-side ingest (default off): loadVolumeData only reads the raw files; the maximum, the USHORT stretch /
    // FLOAT normalisation and the histogram are computed in HBM (vrhip_ingest_raw), bit for bit what the host
    // loader computes.  Set before loadVolumeData.  getHistogram answers for synthetic volumes either way.
    void setDeviceIngest(bool on);
    void setSeed(unsigned int seed);   // pin the per-frame jitter seed
    void clearSeed();                  // back to the std::mt19937 sequence
    vrhip_renderer *handle() { return _r; }
    const rendering_params &renderingParams() const { return _rendering_params; }

    // ---- the throughput path (no reference counterpart: runRaycast renders one frame per call and waits,
    // volumerendercl.cpp:506-558; a caller that wants independent frames -- a turntable, an image-tile share of a
    // multi-GPU split, a benchmark -- hands over several at once)
    // A second renderer on the same GPU that renders from THIS renderer's voxels, ESS bricks and footprint volume
    // (vrhip_share_volumes) with a stream, frame buffer and scratch of its own: two launch sets can be in flight over
    // one copy of the volume.  It starts with this renderer's transfer function and parameters; this renderer must
    // outlive it.
    std::unique_ptr<VolumeRenderCL> shareVolumes();
    // seeds.size() <= 256 INDEPENDENT frames (frame f jittered by seeds[f], iteration 0) in ONE set of launches
    // (vrhip_render_batch) into DEVICE memory dev_out[f][height][width][4]; returns without waiting.
    void renderFrames(size_t width, size_t height, const std::vector<unsigned int> &seeds, float *dev_out);
    // the same for a tile subset: dev_out[f][n_tiles][tile_h][tile_w][4]; frame_stride: pixels between the frames of
    // dev_out (0 = packed)
    void renderFramesTiles(size_t width, size_t height, size_t tile_w, size_t tile_h,
                           const std::vector<unsigned int> &tile_ids, const std::vector<unsigned int> &seeds,
                           float *dev_out, size_t frame_stride = 0);
    // per-frame cameras (vrhip_render_batch_views): frame f rendered from views[f] (row-major, as updateView takes it)
    // with this renderer's bbox and ortho setting -- a turntable, a fly-through, a replayed camera path;
    // views.size() == seeds.size()
    void renderFrames(size_t width, size_t height, const std::vector<unsigned int> &seeds,
                      const std::vector<std::array<float, 16>> &views, float *dev_out);
    void renderFramesTiles(size_t width, size_t height, size_t tile_w, size_t tile_h,
                           const std::vector<unsigned int> &tile_ids, const std::vector<unsigned int> &seeds,
                           const std::vector<std::array<float, 16>> &views, float *dev_out, size_t frame_stride = 0);
    // ---- 8-bit frames: the reference's output image is CL_UNORM_INT8 (volumerendercl.cpp:468-478), which is what its
    // runRaycastNoGL actually reads back (:568-607) and its GUI shows, saves and records.  Per channel 0 for a NaN, else
    // rint(clamp(f * 255.0f, 0, 255)), ties to even (vrhip.h "8-bit frames"); quantised on the GPU.
    // runRaycastNoGL with `output` resized to width*height*4 bytes, R G B A per pixel, row 0 = top.  The frame buffer
    // keeps the float frame: accumulation and image-order ESS carry on as with runRaycast.
    void runRaycastRGBA8(size_t width, size_t height, std::vector<unsigned char> &output);
    // the bytes of the frame the frame buffer holds (vrhip_frame_rgba8): what the last runRaycast / runRaycastNoGL /
    // runRaycastRGBA8 / whole-frame renderSamples of this size rendered; nothing is rendered, nothing advances
    void frameRGBA8(size_t width, size_t height, std::vector<unsigned char> &output);
    // renderFrames with the frames also as 8-bit pixels: the floats into DEVICE memory dev_frames[f][height][width][4]
    // as renderFrames writes them, their 8-bit twins into DEVICE memory dev_out[f][height][width][4] (bytes) on the
    // same stream; returns without waiting
    void renderFramesRGBA8(size_t width, size_t height, const std::vector<unsigned int> &seeds, float *dev_frames,
                           unsigned char *dev_out);
    void renderFramesRGBA8(size_t width, size_t height, const std::vector<unsigned int> &seeds,
                           const std::vector<std::array<float, 16>> &views, float *dev_frames, unsigned char *dev_out);
    // ---- slice views (no reference counterpart; vrhip.h "slice views"): 2-D cuts through the voxels -- a plane, or a
    // slab reduced by max / min / mean over parallel planes -- coloured by the transfer function or as the filtered
    // value itself.  One launch for all slices of a call.  Reads the volume of the current time step, the transfer
    // function, setLinearInterpolation and setBackground; camera, technique, iteration and seed are neither read nor
    // touched, so progressive frames carry on around a slice bit for bit.
    typedef vrhip_slice_params slice_params;
    enum slice_mode { SLICE_MAX = VRHIP_SLICE_MAX, SLICE_MIN = VRHIP_SLICE_MIN, SLICE_MEAN = VRHIP_SLICE_MEAN };
    enum slice_output { SLICE_TF = VRHIP_SLICE_TF, SLICE_VALUE = VRHIP_SLICE_VALUE };
    // The full cross-section of the box [-1, 1]^3 perpendicular to axis 0 | 1 | 2 (x | y | z) at `position` along it;
    // thickness (box units, along +axis, centred on position) and samples make it a slab.  Orientation: axis z: right
    // = +x, up = +y; axis y: right = -x, up = +z; axis x: right = +y, up = +z -- each seen from the positive side of its
    // axis, u x v = +axis.  The image spans the whole box whatever its size in pixels: the caller picks width : height
    // from the model scale.
    static slice_params axisSlice(int axis, float position, float thickness = 0.f, unsigned int samples = 1,
                                  slice_mode mode = SLICE_MAX, slice_output output = SLICE_TF);
    // An oblique plane through `origin` perpendicular to `normal`: v = halfHeight * the unit vector of `up` made
    // orthogonal to the normal, u = halfWidth * (v^ x n^), w = thickness * n^ (computed in double, stored as float).
    // Throws std::invalid_argument for a zero normal or an up vector parallel to it.
    static slice_params planeSlice(const std::array<float, 3> &origin, const std::array<float, 3> &normal,
                                   const std::array<float, 3> &up, float halfWidth, float halfHeight, float thickness = 0.f,
                                   unsigned int samples = 1, slice_mode mode = SLICE_MAX, slice_output output = SLICE_TF);
    // n parallel copies of `s` stepped along its normal (along w for a slab, else u x v) over `span` box units centred
    // on s.origin: copy k at origin + ((k + 0.5) / n - 0.5) * span * normal
    static std::vector<slice_params> sliceStack(const slice_params &s, unsigned int n, float span);
    // `output` receives slices.size() images of width*height*4 floats, row 0 = top ...
    void renderSlices(size_t width, size_t height, const std::vector<slice_params> &slices, std::vector<float> &output);
    // ... or DEVICE memory dev_out[n][height][width][4] does (16-byte aligned); returns without waiting
    void renderSlices(size_t width, size_t height, const std::vector<slice_params> &slices, float *dev_out);
    // the device form with the images also as 8-bit pixels (vrhip_quantise_rgba8 on the same stream): the floats into
    // DEVICE memory dev_frames[n][height][width][4], their bytes into out[n][height][width][4] -- device memory
    // (returns without waiting), or host memory with outIsDevice = false (returns when the bytes have arrived)
    void renderSlicesRGBA8(size_t width, size_t height, const std::vector<slice_params> &slices, float *dev_frames,
                           unsigned char *out, bool outIsDevice = true);
    // ---- depth images and picking (no reference counterpart; vrhip.h "depth images and picking"): where along its
    // ray each pixel's "thing" lies -- the first sample at or above a value (DEPTH_ISO, refined as technique 4 refines),
    // the first sample that attains the ray's maximum (DEPTH_MAX), or the sample at which the ray caster's accumulated
    // opacity reaches a threshold (DEPTH_OPACITY).  The rays are the current camera's, with the jitter seed of the frame
    // last rendered (or the one pinned with setSeed): a pick lands in the frame on the screen.  Technique, iteration and
    // frame buffer are neither read nor touched, so progressive frames carry on around a depth call bit for bit.
    enum depth_mode { DEPTH_ISO = VRHIP_DEPTH_ISO, DEPTH_MAX = VRHIP_DEPTH_MAX, DEPTH_OPACITY = VRHIP_DEPTH_OPACITY };
    enum depth_kind { DEPTH_MISS = VRHIP_DEPTH_MISS, DEPTH_NO_HIT = VRHIP_DEPTH_NO_HIT, DEPTH_HIT = VRHIP_DEPTH_HIT };
    struct depth_image {
        size_t width = 0, height = 0;      // of the rectangle answered
        std::vector<float> xyzt;           // [height][width][4]: hit position in box space ([-1, 1]^3) and ray parameter t;
                                           // (0, 0, 0, +inf) without a hit
        std::vector<float> aux;            // [height][width]: ISO the value at the hit, MAX the maximum, OPACITY the opacity reached
        std::vector<unsigned char> kind;   // [height][width]: depth_kind
    };
    // rect = {x0, y0, w, h}: that rectangle of the width x height frame; all zero: the whole frame.  Row 0 = top.
    void renderDepth(size_t width, size_t height, depth_mode mode, float threshold, depth_image &output,
                     unsigned int refineSteps = 4, const std::array<unsigned int, 4> &rect = {{0, 0, 0, 0}});
    struct pick_result {
        bool hit = false;
        std::array<float, 3> pos{{0.f, 0.f, 0.f}};     // box space
        float t = 0.f, aux = 0.f;
        std::array<double, 3> voxel{{0., 0., 0.}};     // (pos * 0.5 + 0.5) * resolution: continuous voxel coordinates
    };
    // the 3-D point under pixel (x, y) of the width x height frame: renderDepth on a 1 x 1 rectangle
    pick_result pick(size_t width, size_t height, unsigned int x, unsigned int y, depth_mode mode, float threshold = 0.5f,
                     unsigned int refineSteps = 4);
    // ---- isosurface extraction (no reference counterpart; vrhip.h "isosurface extraction"): the surface technique 4
    // draws at `iso`, as a triangle list in box space ([-1, 1]^3), nine floats a triangle, in the contract's order.
    // Shared vertices are bit-equal, so weldMesh turns the list into an indexed, watertight mesh.  normals: technique
    // 4's shading normal per vertex.  region: the cubes with lo <= corner and corner + 1 <= hi, in voxels; all zero:
    // the whole volume.  Camera, technique and frame buffer are neither read nor touched.
    struct mesh_region {
        std::array<unsigned int, 3> lo, hi;
        mesh_region() : lo{{0u, 0u, 0u}}, hi{{0u, 0u, 0u}} {}
    };
    struct iso_mesh {
        std::vector<float> positions, normals;   // [triangles][3][3]; normals empty unless asked for
    };
    iso_mesh extractIsosurface(float iso, bool normals = false, const mesh_region &region = mesh_region());
    // unique vertices by bit-equal position, in order of first occurrence; the first occurrence keeps its normal
    struct welded_mesh {
        std::vector<float> vertices, normals;    // [vertices][3]
        std::vector<uint32_t> indices;           // [triangles][3]
    };
    static welded_mesh weldMesh(const std::vector<float> &positions, const std::vector<float> &normals = {});
    // binary STL: the list as it is, each facet's normal from its winding
    static void writeStl(const std::string &path, const std::vector<float> &positions);
    // binary_little_endian PLY of the welded mesh: x y z, nx ny nz when normals are given, uchar-counted uint index
    // lists; returns the number of vertices written
    static size_t writePly(const std::string &path, const std::vector<float> &positions,
                           const std::vector<float> &normals = {});
    // ... of an indexed mesh as it is
    static size_t writePly(const std::string &path, const welded_mesh &mesh);
    // the same surface as an indexed mesh made on the device (vrhip.h "indexed isosurface extraction"): one vertex
    // per crossed lattice edge, vertices[indices] = extractIsosurface's list bit for bit.  Where a grid point equals
    // `iso` several vertices share a position, which weldMesh would merge; no host weld happens here.
    welded_mesh extractIsosurfaceIndexed(float iso, bool normals = false, const mesh_region &region = mesh_region());
    // ---- volume statistics (no reference counterpart; vrhip.h "volume statistics"): the counts, the moments and the
    // value x gradient-magnitude histogram of a region of the current time step, computed on the device.  s is the
    // normalised value isoValue is compared against; bins: vBins over [vLo, vHi] and gBins over [0, gHi), the top
    // gradient bin open-ended; region: the voxels lo <= v < hi, all zero: the whole volume; moments: min, max, sum and
    // sumSq of s as well (0 without).  hist is [gBins][vBins], value fastest.  Nothing a render call reads changes.
    struct stats_params {
        unsigned int vBins = 256, gBins = 1;
        float vLo = 0.f, vHi = 1.f, gHi = 1.f;
        mesh_region region;
        bool moments = false;
    };
    struct volume_stats {
        uint64_t voxels = 0, nan = 0, below = 0, above = 0, gradientNan = 0, binned = 0;
        float min = 0.f, max = 0.f;
        double sum = 0., sumSq = 0.;
        std::vector<uint64_t> hist;
    };
    volume_stats volumeStatistics(const stats_params &params);
    // ---- volume filters (no reference counterpart; vrhip.h "volume filters"): channel 0 of the current time step
    // filtered on the device into time step dstTimestep -- the current one: in place; the number of steps: a new one
    // (which getResolution() does not count).  Separable: per axis (x, y, z) the radius 0..8 and the weights
    // taps[axis][k] at distance k, three fp32 passes with neighbours clamped to the volume; median: the median of
    // the 3x3x3 neighbourhood.  The ESS bricks are rebuilt when a transfer function is set, as after a load.
    struct FilterParams {
        bool median = false;
        std::array<unsigned int, 3> radius = {{0, 0, 0}};
        std::array<std::array<float, 9>, 3> taps = {};
    };
    struct filter_info {
        uint64_t blocks = 0, blocksFetched = 0, blocksSkipped = 0, scratchBytes = 0;
        bool emptySkip = false, inPlace = false;
    };
    void filterVolume(const FilterParams &params, size_t dstTimestep);
    // the current step smoothed in place with a normalised Gaussian of `sigma` voxels along x; the other axes are
    // scaled by the slice thickness (sigma * thickness[0] / thickness[a]): isotropic in box space.  radius 0:
    // ceil(3 sigma) per axis, at most 8.
    void gaussianFilter(double sigma, unsigned int radius = 0);
    void medianFilter();   // the current step, in place
    size_t getTimestep() const { return _timestep; }   // the step setTimestep last selected
    filter_info lastFilterInfo();
    // ---- volume morphology (no reference counterpart; vrhip.h "volume morphology"): grey-scale erosion, dilation,
    // opening, closing, gradient and the top-hat transforms of channel 0 of the current time step, computed on the
    // device into time step dstTimestep -- the current one: in place; the number of steps: a new one (which
    // getResolution() does not count).  The structuring element is a box or a ball (an ellipsoid) of radius 0..8 per
    // axis (x, y, z); neighbours are clamped to the volume.  The ESS bricks are rebuilt when a transfer function is
    // set, as after a load.
    enum class MorphOp { Erode = 0, Dilate, Open, Close, Gradient, TopHat, BlackHat };
    struct MorphParams {
        MorphOp op = MorphOp::Erode;
        bool ball = true;
        std::array<unsigned int, 3> radius = {{1, 1, 1}};
    };
    struct morph_info {
        std::array<uint64_t, 2> blocks = {{0, 0}}, blocksFetched = {{0, 0}}, blocksSkipped = {{0, 0}};
        uint64_t scratchBytes = 0;
        unsigned int sweeps = 0;
        bool emptySkip = false, inPlace = false;
    };
    void morphVolume(const MorphParams &params, size_t dstTimestep);
    // the current step, in place, the same radius on every axis
    void erode(unsigned int radius, bool ball = true);
    void dilate(unsigned int radius, bool ball = true);
    void open(unsigned int radius, bool ball = true);
    void close(unsigned int radius, bool ball = true);
    morph_info lastMorphInfo();
    // ---- the progressive path tracer (technique 1), many samples per call (vrhip_render_samples): seeds.size()
    // consecutive iterations of the accumulated image -- sample k with jitter seed seeds[k] at iteration
    // (current iteration + k) -- in as few launch sets as possible, bit for bit what seeds.size() runRaycastNoGL calls
    // with those seeds leave in the frame buffer.  Advances the iteration by seeds.size(), as runRaycastNoGL advances
    // it by one.  samplesPerLaunch: samples per launch set (0 = the library's default).
    // `output` receives the accumulated frame (width*height*4 floats, row 0 = top) ...
    void renderSamples(size_t width, size_t height, const std::vector<unsigned int> &seeds, std::vector<float> &output,
                       unsigned int samplesPerLaunch = 0);
    // ... or DEVICE memory dev_out[height][width][4] does (nullptr: the image stays in the frame buffer); returns
    // without waiting
    void renderSamples(size_t width, size_t height, const std::vector<unsigned int> &seeds, float *dev_out,
                       unsigned int samplesPerLaunch = 0);
    // the same for a tile subset, as renderTiles: dev_out[n_tiles][tile_h][tile_w][4]
    void renderSamples(size_t width, size_t height, size_t tile_w, size_t tile_h,
                       const std::vector<unsigned int> &tile_ids, const std::vector<unsigned int> &seeds,
                       float *dev_out, unsigned int samplesPerLaunch = 0);
    // the jitter seeds the next n runRaycast calls would use (the default-seeded std::mt19937 member, or the pinned seed)
    std::vector<unsigned int> drawSeeds(size_t n);
    // phase-1 sample rounds per ray (vrhip_set_round_budget): 10 for one frame at a time, 48 for launch sets of
    // several frames; no effect on any pixel
    void setRoundBudget(unsigned int rounds);
    // the events around every launch set (what getLastExecTime reads): off for back-to-back launch sets
    void setFrameTiming(bool on);
    void *stream();   // the hipStream_t the renderer launches on

private:
    void generateBricks();
    void ingestTimestep(size_t t);
    void calcScaling();
    void pushParams();
    void beginFrame();
    void advanceIteration();
    [[noreturn]] void fail(const char *what, int rc);
    void check(const char *what, int rc);

    vrhip_renderer *_r = nullptr;
    bool _volLoaded = false;
    size_t _timestep = 0;
    std::valarray<float> _modelScale;
    std::string _currentDevice;
    std::mt19937 _generator;   // default-seeded, like the reference's member
    bool _seedPinned = false;
    unsigned int _pinnedSeed = 0;
    camera_params _camera_params;
    rendering_params _rendering_params;
    raycast_params _raycast_params;
    pathtrace_params _pathtrace_params;
    vrhip_iso_params _iso_params;
    DatRawReader _dr;
    bool _synthetic = false;
    bool _deviceIngest = false;
    std::vector<std::array<double, 256>> _deviceHistograms;   // of ingested or synthetic time steps
    int _channels = 1;          // 1 = R, 2 = RG, 4 = RGBA (volDataToCLmem, :697-705)
    std::vector<unsigned char> _tff;          // what setTransferFunction / setTffPrefixSum were last given
    std::vector<unsigned int> _tffPrefixSum;  // (shareVolumes hands them to the twin)
    std::vector<unsigned char> _tf2d;         // what setTransferFunction2D was last given (likewise)
    unsigned int _tf2dNV = 0, _tf2dNG = 0;
    float _tf2dGHi = 0.f;
    bool _objEss = true;
    int _device = 0;
    unsigned int _roundBudget = 0;            // 0 = the library's default
    std::array<unsigned int, 4> _synthRes = {{0, 0, 0, 1}};
};

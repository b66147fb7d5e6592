// volumerendercl.cpp -- VolumeRenderCL on libvrhip (see include/volumerendercl.h).  Each
// method cites the reference behaviour it reproduces
// (/root/reference/src/core/volumerendercl.cpp).
#include "hdrloader.h"
#include "volumerendercl.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <numeric>
#include <fstream>
#include <stdexcept>

VolumeRenderCL::VolumeRenderCL() : _modelScale{1.0f, 1.0f, 1.0f}
{
    // member defaults of volumerendercl.h:43-81
    std::memset(&_camera_params, 0, sizeof _camera_params);
    std::memset(&_rendering_params, 0, sizeof _rendering_params);
    std::memset(&_raycast_params, 0, sizeof _raycast_params);
    const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(_camera_params.viewMat, ident, sizeof ident);
    for (int i = 0; i < 3; ++i) { _camera_params.bbox_bl[i] = -1.f; _camera_params.bbox_tr[i] = 1.f; }
    for (int i = 0; i < 4; ++i) _rendering_params.backgroundColor[i] = 1.f;
    for (int i = 0; i < 3; ++i) _rendering_params.modelScale[i] = 1.f;
    _rendering_params.illumType = 1;
    _rendering_params.useLinear = 1;
    _rendering_params.seed = 42;
    _raycast_params.samplingRate = 1.5f;
    for (int i = 0; i < 3; ++i) _raycast_params.brickRes[i] = 1.f;
    _pathtrace_params.max_extinction = 100.f;
    _iso_params = vrhip_iso_params{0.5f, 4u, {0u, 0u}};
}

VolumeRenderCL::~VolumeRenderCL()
{
    if (_r) vrhip_destroy(_r);
}

// logCLerror (volumerendercl.cpp:83-89): failures surface as std::runtime_error
// "ERROR: <what> (<detail>)"; bad arguments as std::invalid_argument.
void VolumeRenderCL::fail(const char *what, int rc)
{
    const char *msg = vrhip_last_error(_r);
    std::string text = (msg && *msg) ? std::string(msg) : std::string("ERROR: ") + what;
    std::cerr << "Error in " << what << ": " << text << std::endl;
    if (rc == VRHIP_ERR_INVALID) throw std::invalid_argument(text);
    throw std::runtime_error(text);
}

void VolumeRenderCL::check(const char *what, int rc)
{
    if (rc != VRHIP_OK) fail(what, rc);
}

void VolumeRenderCL::initialize(bool useGL, bool useCPU, cl_vendor, const std::string deviceName,
                                const int platformId)
{
    if (useCPU)
        throw std::runtime_error("ERROR: no CPU device path; this renderer runs on MI355X only");
    if (useGL)
        std::cout << "OpenGL context sharing is not available in the headless build. "
                  << "Using buffer generation instead." << std::endl;
    int device = 0;
    if (!deviceName.empty() && deviceName.find_first_not_of("0123456789") == std::string::npos)
        device = std::stoi(deviceName);
    else if (platformId >= 0)
        device = platformId;
    if (_r) { vrhip_destroy(_r); _r = nullptr; }
    _device = device;
    int rc = vrhip_create(device, &_r);
    if (rc != VRHIP_OK) {
        const char *msg = vrhip_last_error(nullptr);
        throw std::runtime_error(msg && *msg ? msg : "ERROR: vrhip_create");
    }
    char name[256];
    vrhip_device_name(_r, name, sizeof name);
    _currentDevice = name;
    // upload volume data to the device if already loaded (:153-158)
    if (_dr.has_data()) {
        const auto &p = _dr.properties();
        for (size_t t = 0; t < _dr.data().size(); ++t)
            if (_deviceIngest)
                ingestTimestep(t);   // (the reader holds raw file bytes: they are converted on the device again)
            else
                check("volDataToCLmem",
                      vrhip_upload_volume_channels(_r, _dr.data()[t].data(), p.volume_res.data(),
                                                   int(p.format), _channels, uint32_t(t)));
    }
}

void VolumeRenderCL::setDeviceIngest(bool on) { _deviceIngest = on; }

// one time step of raw file bytes through vrhip_ingest_raw: histogram and value range as the host loader
// would have left them in the reader
void VolumeRenderCL::ingestTimestep(size_t t)
{
    const auto &p = _dr.properties();
    if (_deviceHistograms.size() <= t) _deviceHistograms.resize(t + 1);
    float maxValue = 0.f;
    int rc = vrhip_ingest_raw(_r, _dr.data()[t].data(), _dr.data()[t].size(), p.volume_res.data(), int(p.format),
                              _channels, p.endianness == DatRawReader::BIG ? 1 : 0, uint32_t(t),
                              _deviceHistograms[t].data(), &maxValue);
    if (rc == VRHIP_ERR_INVALID) {   // loadVolumeData's size check throws std::runtime_error (:740-742)
        const std::string text = vrhip_last_error(_r);
        _dr.clearData();
        throw std::runtime_error(text);
    }
    check("vrhip_ingest_raw", rc);
    _dr.set_value_range(0.f, maxValue);
}

void VolumeRenderCL::updateView(const std::array<float, 16> viewMat)   // :379-390
{
    if (!_volLoaded || _modelScale.size() < 3) return;
    for (size_t i = 0; i < 16; ++i) _camera_params.viewMat[i] = viewMat[i];
    _rendering_params.iteration = 0;
}

void VolumeRenderCL::updateSamplingRate(const double samplingRate)   // :397-401
{
    _raycast_params.samplingRate = static_cast<float>(samplingRate);
}

void VolumeRenderCL::updateOutputImg(const size_t, const size_t, cl_GLuint)
{
    // output / accumulate buffers are sized by the render call itself (:465-499); the hit images of
    // image-order ESS start over with their initial contents (:482-488)
    if (_r) check("updateOutputImg", vrhip_reset_image_ess(_r));
}

void VolumeRenderCL::pushParams()
{
    for (int i = 0; i < 3; ++i) _rendering_params.modelScale[i] = _modelScale[i];   // :206-207
    check("setCameraArgs", vrhip_set_camera_params(_r, &_camera_params));
    check("setRenderingArgs", vrhip_set_rendering_params(_r, &_rendering_params));
    check("setRaycastArgs", vrhip_set_raycast_params(_r, &_raycast_params));
    check("setPathtraceArgs", vrhip_set_pathtrace_params(_r, &_pathtrace_params));
    check("setIsoArgs", vrhip_set_iso_params(_r, &_iso_params));
}

void VolumeRenderCL::beginFrame()   // setMemObjectsRaycast (:194-218): fresh seed per frame
{
    _rendering_params.seed = _seedPinned ? _pinnedSeed : static_cast<unsigned int>(_generator());
    pushParams();
}

void VolumeRenderCL::runRaycast(const size_t width, const size_t height)   // :506-558
{
    if (!_volLoaded) return;
    beginFrame();
    check("runRaycast", vrhip_render_frame(_r, uint32_t(width), uint32_t(height), nullptr, 0));
    advanceIteration();   // :540
}

void VolumeRenderCL::runRaycastNoGL(const size_t width, const size_t height,
                                    std::vector<float> &output)   // :568-607
{
    if (!_volLoaded) return;
    beginFrame();
    output.resize(width * height * 4);   // :583
    check("runRaycastNoGL", vrhip_render_frame(_r, uint32_t(width), uint32_t(height),
                                               output.data(), 0));
    advanceIteration();
}

void VolumeRenderCL::renderTiles(size_t width, size_t height, size_t tile_w, size_t tile_h,
                                 const std::vector<unsigned int> &tile_ids, float *out_tiles_dev,
                                 bool advanceIteration)
{
    if (!_volLoaded) return;
    beginFrame();
    check("renderTiles", vrhip_render_tiles(_r, uint32_t(width), uint32_t(height), uint32_t(tile_w),
                                            uint32_t(tile_h), tile_ids.data(),
                                            uint32_t(tile_ids.size()), out_tiles_dev));
    if (advanceIteration) this->advanceIteration();
}

size_t VolumeRenderCL::loadVolumeData(const DatRawReader::Properties volumeFileProps)   // :765-805
{
    _volLoaded = false;
    _synthetic = false;
    if (volumeFileProps.dat_file_name.empty() && !volumeFileProps.raw_file_names.empty())
        std::cerr << "Loading raw volume data from " << volumeFileProps.raw_file_names.at(0)
                  << std::endl;
    else
        std::cout << "Loading volume data defined in " << volumeFileProps.dat_file_name << std::endl;
    try {
        _dr.read_files(volumeFileProps, !_deviceIngest);
        _deviceHistograms.clear();
        const auto &p = _dr.properties();
        std::cout << _dr.data().front().size() * _dr.data().size() << " bytes have been read from "
                  << _dr.data().size() << " file(s)." << std::endl;
        std::cout << p.to_string() << std::endl;
        // volDataToCLmem (:690-759)
        const std::string &co = p.image_channel_order;
        int channels = 1;
        if (co == "RG") channels = 2;
        else if (co == "RGBA") channels = 4;
        else if (co == "ARGB" || co == "BGRA")
            // accepted by the reference's upload (:706-709), but its kernel has no branch for these
            // orders and composites an unset colour (volumeraycast.cl:800-855)
            throw std::invalid_argument("ARGB / BGRA volumes are not supported.");
        else if (!(co == "R" || co == "" || co == "I" || co == "LUMINANCE"))
            throw std::invalid_argument("Unknown or invalid volume color format.");
        _channels = channels;
        if (p.format != DatRawReader::UCHAR && p.format != DatRawReader::USHORT &&
            p.format != DatRawReader::FLOAT)
            throw std::invalid_argument("Unknown or invalid volume data format.");
        const size_t bpv = p.format == DatRawReader::UCHAR ? 1 : p.format == DatRawReader::USHORT ? 2 : 4;
        check("clearVolumes", vrhip_clear_volumes(_r));
        for (size_t t = 0; t < _dr.data().size(); ++t) {
            if (_deviceIngest) {
                ingestTimestep(t);
                continue;
            }
            // (the reference checks one channel's worth, :740-742, and lets the image read beyond)
            if (size_t(p.volume_res[0]) * p.volume_res[1] * p.volume_res[2] * bpv * size_t(channels) >
                _dr.data()[t].size()) {
                _dr.clearData();
                throw std::runtime_error("Volume size does not match size specified in dat file.");
            }
            check("volDataToCLmem",
                  vrhip_upload_volume_channels(_r, _dr.data()[t].data(), p.volume_res.data(),
                                               int(p.format), _channels, uint32_t(t)));
        }
        calcScaling();
    } catch (std::invalid_argument &e) {
        throw std::runtime_error(e.what());   // :784-787
    }
    // default prefix sum of the linear ramp (:795-801)
    std::vector<unsigned int> prefixSum(1024, 0);
    for (size_t i = 0; i < prefixSum.size(); ++i) prefixSum[i] = static_cast<unsigned int>(i) * 4u;
    std::partial_sum(prefixSum.begin(), prefixSum.end(), prefixSum.begin());
    _volLoaded = true;
    setTffPrefixSum(prefixSum);
    return _dr.data().size();
}

void VolumeRenderCL::loadSyntheticVolume(const std::string &kind, unsigned int res,
                                         DatRawReader::data_format f)
{
    _volLoaded = false;
    const uint32_t r3[3] = {res, res, res};
    check("clearVolumes", vrhip_clear_volumes(_r));
    check("synthVolume", vrhip_synth_volume(_r, kind == "shells" ? 1 : 0, r3, int(f), 0));
    _synthetic = true;
    _synthRes = {{res, res, res, 1}};
    _modelScale = {1.f, 1.f, 1.f};
    std::vector<unsigned int> prefixSum(1024, 0);
    for (size_t i = 0; i < prefixSum.size(); ++i) prefixSum[i] = static_cast<unsigned int>(i) * 4u;
    std::partial_sum(prefixSum.begin(), prefixSum.end(), prefixSum.begin());
    _volLoaded = true;
    setTffPrefixSum(prefixSum);
}

void VolumeRenderCL::calcScaling()   // :347-362
{
    if (!_dr.has_data()) return;
    const auto &p = _dr.properties();
    _modelScale = {static_cast<float>(p.volume_res.at(0)), static_cast<float>(p.volume_res.at(1)),
                   static_cast<float>(p.volume_res.at(2))};
    std::valarray<float> thickness = {static_cast<float>(p.slice_thickness.at(0)),
                                      static_cast<float>(p.slice_thickness.at(1)),
                                      static_cast<float>(p.slice_thickness.at(2))};
    _modelScale *= thickness * (1.f / thickness[0]);
    _modelScale = _modelScale.max() / _modelScale;
}

void VolumeRenderCL::scaleVolume(std::valarray<float> scale) { _modelScale *= scale; }

bool VolumeRenderCL::hasData() const { return _volLoaded; }

const std::array<unsigned int, 4> VolumeRenderCL::getResolution() const   // :822-827
{
    if (_synthetic) return _synthRes;
    if (!_dr.has_data()) return std::array<unsigned int, 4>{{0, 0, 0, 1}};
    return _dr.properties().volume_res;
}

const std::array<double, 256> &VolumeRenderCL::getHistogram(unsigned int timestep)   // :853-858
{
    if (_synthetic && _volLoaded) {
        // a volume born in HBM has no loader histogram: the same binning over the stored voxels
        if (_deviceHistograms.size() <= timestep) _deviceHistograms.resize(timestep + 1);
        int rc = vrhip_volume_histogram(_r, timestep, _deviceHistograms[timestep].data());
        if (rc == VRHIP_ERR_NODATA) throw std::invalid_argument("Invalid timestep for histogram data.");
        check("vrhip_volume_histogram", rc);
        return _deviceHistograms[timestep];
    }
    if (!_dr.has_data()) throw std::invalid_argument("Invalid timestep for histogram data.");
    if (_deviceIngest) {
        if (timestep >= _deviceHistograms.size())
            throw std::invalid_argument("No histogram data for selected timestep available.");
        return _deviceHistograms[timestep];
    }
    return _dr.getHistogram(timestep);
}

void VolumeRenderCL::setTransferFunction(std::vector<unsigned char> &tff)   // :864-891
{
    if (!_volLoaded) return;
    _tff = tff;
    check("setTransferFunction",
          vrhip_set_transfer_function(_r, tff.data(), uint32_t(tff.size() / 4)));
    generateBricks();
    std::vector<unsigned int> prefixSum;
    for (size_t i = 3; i < tff.size(); i += 4) prefixSum.push_back(static_cast<unsigned int>(tff.at(i)));
    std::partial_sum(prefixSum.begin(), prefixSum.end(), prefixSum.begin());
    setTffPrefixSum(prefixSum);
    _rendering_params.iteration = 0;
}

void VolumeRenderCL::setTffPrefixSum(std::vector<unsigned int> &tffPrefixSum)   // :898-916
{
    if (!_volLoaded) return;
    _tffPrefixSum = tffPrefixSum;
    check("setTffPrefixSum",
          vrhip_set_tff_prefix_sum(_r, tffPrefixSum.data(), uint32_t(tffPrefixSum.size())));
}

void VolumeRenderCL::generateBricks()   // :614-684
{
    check("generateBricks", vrhip_build_bricks(_r));
    float brf[3];
    check("generateBricks", vrhip_get_brick_info(_r, nullptr, brf, nullptr));
    for (int i = 0; i < 3; ++i) _raycast_params.brickRes[i] = brf[i];   // :627-631
}

void VolumeRenderCL::setCamOrtho(bool v) { _camera_params.ortho = v ? 1u : 0u; }
void VolumeRenderCL::setIllumination(unsigned int illum) { _rendering_params.illumType = illum; }
void VolumeRenderCL::setAmbientOcclusion(bool ao) { _raycast_params.useAO = ao ? 1u : 0u; }
void VolumeRenderCL::setShowESS(bool v) { _rendering_params.showEss = v ? 1u : 0u; }
void VolumeRenderCL::setLinearInterpolation(bool v) { _rendering_params.useLinear = v ? 1u : 0u; }
void VolumeRenderCL::setContours(bool v) { _raycast_params.contours = v ? 1u : 0u; }
void VolumeRenderCL::setAerial(bool v) { _raycast_params.aerial = v ? 1u : 0u; }
void VolumeRenderCL::setImgEss(bool v) { _rendering_params.imgEss = v ? 1u : 0u; }
void VolumeRenderCL::setUseGradient(bool v) { _rendering_params.useGradient = v ? 1u : 0u; }

void VolumeRenderCL::setObjEss(bool useEss)   // :1006-1019: kernel-variant switch, no rebuild
{
    _objEss = useEss;
    check("setObjEss", vrhip_set_object_ess(_r, useEss ? 1 : 0));
}

void VolumeRenderCL::setBackground(std::array<float, 4> color)   // :1025-1030
{
    // the reference converts through cl_float3, which zeroes the 4th component
    _rendering_params.backgroundColor[0] = color[0];
    _rendering_params.backgroundColor[1] = color[1];
    _rendering_params.backgroundColor[2] = color[2];
    _rendering_params.backgroundColor[3] = 0.f;
}

// A frame was rendered: the accumulating techniques move on to the next iteration; a maximum intensity
// projection or an isosurface does not accumulate, every frame of it is iteration 0 (the library rejects anything else).
void VolumeRenderCL::advanceIteration()
{
    if (_rendering_params.technique != TECH_MIP && _rendering_params.technique != TECH_ISO &&
        _rendering_params.technique != TECH_TF2D && _rendering_params.technique != TECH_PREINT)
        _rendering_params.iteration++;
}

std::array<float, 4> VolumeRenderCL::preintSlab(const std::vector<unsigned char> &tff, float sf, float sb, bool raw)
{
    std::vector<float> entries(tff.size());
    for (size_t i = 0; i < tff.size(); ++i) entries[i] = static_cast<float>(tff[i]) / 255.0f;
    std::array<float, 4> out{};
    if (tff.empty() || tff.size() % 4 != 0 ||
        vrhip_preint_slab(entries.data(), static_cast<uint32_t>(tff.size() / 4), raw ? 1 : 0, sf, sb, out.data()) != VRHIP_OK)
        throw std::invalid_argument("preintSlab: invalid table size or sample value.");
    return out;
}

void VolumeRenderCL::setTransferFunction2D(const std::vector<unsigned char> &table, unsigned int nV, unsigned int nG,
                                           float gHi)
{
    if (table.size() != size_t(4) * nV * nG)
        throw std::invalid_argument("setTransferFunction2D: the table must hold 4 * nV * nG bytes.");
    check("setTransferFunction2D", vrhip_set_transfer_function_2d(_r, table.data(), nV, nG, gHi));
    _tf2d = table;
    _tf2dNV = nV;
    _tf2dNG = nG;
    _tf2dGHi = gHi;
    _rendering_params.iteration = 0;
}

std::vector<unsigned char> VolumeRenderCL::rampTransferFunction2D(const std::vector<unsigned char> &tff, unsigned int nG,
                                                                  float gHi, float g0, float g1)
{
    const unsigned int nV = static_cast<unsigned int>(tff.size() / 4);
    std::vector<unsigned char> out(size_t(4) * nV * nG);
    if (tff.size() % 4 != 0 || vrhip_tf2d_build_ramp(tff.data(), nV, nG, gHi, g0, g1, out.data()) != VRHIP_OK)
        throw std::invalid_argument("rampTransferFunction2D: invalid table size, gHi or ramp.");
    return out;
}

void VolumeRenderCL::setTechnique(technique tech)   // :1042-1047
{
    _rendering_params.technique = static_cast<uint>(tech);
    _rendering_params.iteration = 0;
}

void VolumeRenderCL::setIsoValue(float isoValue)
{
    _iso_params.isoValue = isoValue;
}

void VolumeRenderCL::setIsoRefinement(unsigned int refineSteps)
{
    _iso_params.refineSteps = refineSteps;
}

void VolumeRenderCL::setExtinction(const double extinction)
{
    _pathtrace_params.max_extinction = float(extinction);
}

void VolumeRenderCL::setBBox(float bl_x, float bl_y, float bl_z, float tr_x, float tr_y, float tr_z)
{
    _camera_params.bbox_bl[0] = bl_x; _camera_params.bbox_bl[1] = bl_y; _camera_params.bbox_bl[2] = bl_z;
    _camera_params.bbox_tr[0] = tr_x; _camera_params.bbox_tr[1] = tr_y; _camera_params.bbox_tr[2] = tr_z;
    _rendering_params.iteration = 0;
}

void VolumeRenderCL::setTimestep(const size_t t)   // :1167-1174
{
    if (_dr.has_data() && t >= _dr.properties().volume_res.at(3)) return;
    _timestep = t;
    check("setTimestep", vrhip_set_timestep(_r, uint32_t(t)));
    _rendering_params.iteration = 0;
}

double VolumeRenderCL::getLastExecTime() { return vrhip_last_kernel_seconds(_r); }

const std::vector<std::string> VolumeRenderCL::getPlatformNames() { return {"AMD HIP (ROCm)"}; }

const std::vector<std::string> VolumeRenderCL::getDeviceNames(size_t, const std::string &type)
{
    if (type == "CPU") return {};
    return {_currentDevice};
}

const std::string VolumeRenderCL::getCurrentDeviceName() { return _currentDevice; }

// volumerendercl.cpp:238-341: down-sample time step t on the GPU, write <dat name>_<N>.raw/.dat
// next to the loaded .dat, return the path without extension.  The .dat text is the reference's,
// including its quirks: `Format:` carries the enum's integer and `ObjectFileName:` is cut with
// substr(first + 1, lastindex) where lastindex is a position, not a length.
const std::string VolumeRenderCL::volumeDownsampling(const size_t t, const int factor)
{
    if (!_dr.has_data()) throw std::runtime_error("No volume data is loaded.");
    if (factor < 2) throw std::invalid_argument("Factor must be greater or equal 2.");
    uint32_t lo[3] = {0, 0, 0};
    int rc = vrhip_downsample_volume(_r, uint32_t(t), factor, nullptr, 0, lo);
    if (rc == VRHIP_ERR_INVALID) throw std::invalid_argument(vrhip_last_error(_r));
    check("vrhip_downsample_volume", rc);
    const DatRawReader::Properties &p = _dr.properties();
    const size_t mult = p.format == DatRawReader::UCHAR ? 1 : p.format == DatRawReader::USHORT ? 2 : 4;
    std::vector<unsigned char> outputData(size_t(lo[0]) * lo[1] * lo[2] * mult);
    check("vrhip_downsample_volume", vrhip_downsample_volume(_r, uint32_t(t), factor, outputData.data(),
                                                             outputData.size(), lo));
    size_t lastindex = p.dat_file_name.find_last_of(".");
    std::string rawname = p.dat_file_name.substr(0, lastindex);
    rawname += "_";
    rawname += std::to_string(lo[0]);
    std::ofstream file(rawname + ".raw", std::ios::out | std::ios::binary);
    file.write(reinterpret_cast<const char *>(outputData.data()), std::streamsize(outputData.size()));
    file.close();
    std::ofstream datFile(rawname + ".dat", std::ios::out);
    lastindex = rawname.find_last_of(".");
    size_t firstindex = rawname.find_last_of("/\\");
    std::string rawnameShort = rawname.substr(firstindex + 1, lastindex);
    datFile << "ObjectFileName: \t" << rawnameShort << ".raw\n";
    datFile << "Resolution: \t\t" << lo[0] << " " << lo[1] << " " << lo[2] << "\n";
    datFile << "SliceThickness: \t" << p.slice_thickness.at(0) << " " << p.slice_thickness.at(1) << " "
            << p.slice_thickness.at(2) << "\n";
    datFile << "Format: \t\t\t" << p.format << "\n";
    datFile.close();
    return rawname;
}

void VolumeRenderCL::createEnvironmentMap(const std::string &file_name)
{
    // an empty name installs the 1x1 white map, which the kernel never samples (:1130-1134, :655)
    if (file_name.empty()) {
        check("createEnvironmentMap", vrhip_set_environment_map(_r, nullptr, 0, 0));
        return;
    }
    vrhost::HdrImage img;
    if (!vrhost::load_hdr_float4(file_name, img))
        throw std::runtime_error("Error loading environment map file.");   // :1138
    check("createEnvironmentMap",
          vrhip_set_environment_map(_r, img.rgba.data(), img.width, img.height));
    std::cout << "Loaded environment map " << file_name << std::endl;
}

void VolumeRenderCL::setSeed(unsigned int seed) { _seedPinned = true; _pinnedSeed = seed; }
void VolumeRenderCL::clearSeed() { _seedPinned = false; }

// ---- the throughput path (include/volumerendercl.h "additions"): launch sets of independent frames on
// vrhip_share_volumes / vrhip_render_batch

std::unique_ptr<VolumeRenderCL> VolumeRenderCL::shareVolumes()
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    std::unique_ptr<VolumeRenderCL> twin(new VolumeRenderCL());
    int rc = vrhip_create(_device, &twin->_r);
    if (rc != VRHIP_OK) {
        const char *msg = vrhip_last_error(nullptr);
        throw std::runtime_error(msg && *msg ? msg : "ERROR: vrhip_create");
    }
    twin->_device = _device;
    twin->_currentDevice = _currentDevice;
    twin->check("shareVolumes", vrhip_share_volumes(twin->_r, _r));
    twin->_synthetic = true;          // (resolution from _synthRes: the twin holds no DatRawReader data)
    twin->_synthRes = getResolution();
    twin->_channels = _channels;
    twin->_modelScale = _modelScale;
    twin->_timestep = _timestep;
    twin->_camera_params = _camera_params;
    twin->_rendering_params = _rendering_params;
    twin->_raycast_params = _raycast_params;
    twin->_pathtrace_params = _pathtrace_params;
    twin->_iso_params = _iso_params;
    twin->_seedPinned = _seedPinned;
    twin->_pinnedSeed = _pinnedSeed;
    twin->_volLoaded = true;
    twin->check("setTimestep", vrhip_set_timestep(twin->_r, uint32_t(_timestep)));
    twin->setObjEss(_objEss);
    if (!_tff.empty()) {
        std::vector<unsigned char> tff = _tff;
        twin->setTransferFunction(tff);     // (takes the owner's bricks: vrhip_build_bricks on a sharer)
    }
    if (!_tffPrefixSum.empty()) {
        std::vector<unsigned int> prefix = _tffPrefixSum;
        twin->setTffPrefixSum(prefix);
    }
    if (!_tf2d.empty()) twin->setTransferFunction2D(_tf2d, _tf2dNV, _tf2dNG, _tf2dGHi);
    twin->_rendering_params.iteration = _rendering_params.iteration;
    if (_roundBudget) twin->setRoundBudget(_roundBudget);
    return twin;
}

void VolumeRenderCL::renderFrames(size_t width, size_t height, const std::vector<unsigned int> &seeds, float *dev_out)
{
    renderFramesTiles(width, height, 0, 0, std::vector<unsigned int>(), seeds, dev_out, 0);
}

void VolumeRenderCL::renderFramesTiles(size_t width, size_t height, size_t tile_w, size_t tile_h,
                                       const std::vector<unsigned int> &tile_ids,
                                       const std::vector<unsigned int> &seeds, float *dev_out, size_t frame_stride)
{
    if (!_volLoaded) return;
    _rendering_params.iteration = 0;   // the frames of a launch set are independent
    pushParams();
    check("renderFrames", vrhip_render_batch(_r, uint32_t(width), uint32_t(height), uint32_t(tile_w), uint32_t(tile_h),
                                             tile_ids.empty() ? nullptr : tile_ids.data(), uint32_t(tile_ids.size()),
                                             seeds.data(), uint32_t(seeds.size()), dev_out, uint32_t(frame_stride)));
}

void VolumeRenderCL::renderFrames(size_t width, size_t height, const std::vector<unsigned int> &seeds,
                                  const std::vector<std::array<float, 16>> &views, float *dev_out)
{
    renderFramesTiles(width, height, 0, 0, std::vector<unsigned int>(), seeds, views, dev_out, 0);
}

void VolumeRenderCL::renderFramesTiles(size_t width, size_t height, size_t tile_w, size_t tile_h,
                                       const std::vector<unsigned int> &tile_ids,
                                       const std::vector<unsigned int> &seeds,
                                       const std::vector<std::array<float, 16>> &views, float *dev_out,
                                       size_t frame_stride)
{
    if (!_volLoaded) return;
    if (views.size() != seeds.size()) throw std::invalid_argument("renderFrames: one view per frame");
    _rendering_params.iteration = 0;
    pushParams();
    std::vector<vrhip_camera_params> cams(views.size());
    for (size_t f = 0; f < views.size(); ++f) {
        std::memcpy(&cams[f], &_camera_params, sizeof(vrhip_camera_params));
        for (size_t i = 0; i < 16; ++i) cams[f].viewMat[i] = views[f][i];
    }
    check("renderFrames", vrhip_render_batch_views(_r, uint32_t(width), uint32_t(height), uint32_t(tile_w),
                                                   uint32_t(tile_h), tile_ids.empty() ? nullptr : tile_ids.data(),
                                                   uint32_t(tile_ids.size()), seeds.data(), cams.data(),
                                                   uint32_t(seeds.size()), dev_out, uint32_t(frame_stride)));
}

// ---- 8-bit frames (vrhip_render_frame_rgba8, vrhip_quantise_rgba8)

void VolumeRenderCL::runRaycastRGBA8(size_t width, size_t height, std::vector<unsigned char> &output)
{
    if (!_volLoaded) return;
    beginFrame();
    output.resize(width * height * 4);
    check("runRaycastRGBA8", vrhip_render_frame_rgba8(_r, uint32_t(width), uint32_t(height), output.data(), 0));
    advanceIteration();
}

void VolumeRenderCL::frameRGBA8(size_t width, size_t height, std::vector<unsigned char> &output)
{
    if (!_volLoaded) return;
    output.resize(width * height * 4);
    check("frameRGBA8", vrhip_frame_rgba8(_r, uint32_t(width), uint32_t(height), output.data(), 0));
}

void VolumeRenderCL::renderFramesRGBA8(size_t width, size_t height, const std::vector<unsigned int> &seeds,
                                       float *dev_frames, unsigned char *dev_out)
{
    if (!_volLoaded) return;
    renderFrames(width, height, seeds, dev_frames);
    check("renderFramesRGBA8", vrhip_quantise_rgba8(_r, stream(), dev_frames, uint32_t(seeds.size()), uint32_t(width * height),
                                                    uint32_t(width * height), dev_out, 1));
}

void VolumeRenderCL::renderFramesRGBA8(size_t width, size_t height, const std::vector<unsigned int> &seeds,
                                       const std::vector<std::array<float, 16>> &views, float *dev_frames,
                                       unsigned char *dev_out)
{
    if (!_volLoaded) return;
    renderFrames(width, height, seeds, views, dev_frames);
    check("renderFramesRGBA8", vrhip_quantise_rgba8(_r, stream(), dev_frames, uint32_t(seeds.size()), uint32_t(width * height),
                                                    uint32_t(width * height), dev_out, 1));
}

// ---- slice views (vrhip_render_slices; the helpers compute in double and store floats, as frontend.py's do)

namespace {

VolumeRenderCL::slice_params make_slice(const double o[3], const double u[3], const double v[3], const double w[3],
                                        unsigned int samples, unsigned int mode, unsigned int output)
{
    VolumeRenderCL::slice_params s;
    std::memset(&s, 0, sizeof s);
    for (int i = 0; i < 3; ++i) {
        s.origin[i] = float(o[i]);
        s.u[i] = float(u[i]);
        s.v[i] = float(v[i]);
        s.w[i] = float(w[i]);
    }
    s.samples = samples;
    s.mode = mode;
    s.output = output;
    return s;
}

} // namespace

VolumeRenderCL::slice_params VolumeRenderCL::axisSlice(int axis, float position, float thickness, unsigned int samples,
                                                       slice_mode mode, slice_output output)
{
    if (axis < 0 || axis > 2) throw std::invalid_argument("axisSlice: the axis is 0, 1 or 2");
    const int right = axis == 0 ? 1 : 0, up = axis == 2 ? 1 : 2;
    double o[3] = {0, 0, 0}, u[3] = {0, 0, 0}, v[3] = {0, 0, 0}, w[3] = {0, 0, 0};
    o[axis] = position;
    u[right] = axis == 1 ? -1.0 : 1.0;   // (u x v = +axis for all three)
    v[up] = 1.0;
    w[axis] = thickness;
    return make_slice(o, u, v, w, samples, mode, output);
}

VolumeRenderCL::slice_params VolumeRenderCL::planeSlice(const std::array<float, 3> &origin, const std::array<float, 3> &normal,
                                                        const std::array<float, 3> &up, float halfWidth, float halfHeight,
                                                        float thickness, unsigned int samples, slice_mode mode,
                                                        slice_output output)
{
    double n[3] = {normal[0], normal[1], normal[2]}, upv[3] = {up[0], up[1], up[2]};
    const double ln = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(ln > 0.0)) throw std::invalid_argument("planeSlice: the normal must not be zero");
    for (double &c : n) c /= ln;
    const double d = upv[0] * n[0] + upv[1] * n[1] + upv[2] * n[2];
    double vv[3] = {upv[0] - n[0] * d, upv[1] - n[1] * d, upv[2] - n[2] * d};
    const double lv = std::sqrt(vv[0] * vv[0] + vv[1] * vv[1] + vv[2] * vv[2]);
    const double lu = std::sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
    if (!(lv > 1e-12 * std::max(1.0, lu))) throw std::invalid_argument("planeSlice: up must not be parallel to the normal");
    for (double &c : vv) c /= lv;
    const double uu[3] = {vv[1] * n[2] - vv[2] * n[1], vv[2] * n[0] - vv[0] * n[2], vv[0] * n[1] - vv[1] * n[0]};   // v^ x n^
    double o[3], u[3], v[3], w[3];
    for (int i = 0; i < 3; ++i) {
        o[i] = origin[size_t(i)];
        u[i] = uu[i] * double(halfWidth);
        v[i] = vv[i] * double(halfHeight);
        w[i] = n[i] * double(thickness);
    }
    return make_slice(o, u, v, w, samples, mode, output);
}

std::vector<VolumeRenderCL::slice_params> VolumeRenderCL::sliceStack(const slice_params &s, unsigned int n, float span)
{
    if (n < 1) throw std::invalid_argument("sliceStack: n >= 1");
    double nrm[3] = {s.w[0], s.w[1], s.w[2]};
    if (nrm[0] == 0.0 && nrm[1] == 0.0 && nrm[2] == 0.0) {
        const double u[3] = {s.u[0], s.u[1], s.u[2]}, v[3] = {s.v[0], s.v[1], s.v[2]};
        nrm[0] = u[1] * v[2] - u[2] * v[1];
        nrm[1] = u[2] * v[0] - u[0] * v[2];
        nrm[2] = u[0] * v[1] - u[1] * v[0];
    }
    const double l = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    if (!(l > 0.0)) throw std::invalid_argument("sliceStack: the slice has no normal (u x v and w are zero)");
    std::vector<slice_params> out(n, s);
    for (unsigned int k = 0; k < n; ++k)
        for (int i = 0; i < 3; ++i)
            out[k].origin[i] = float(double(s.origin[i]) + ((double(k) + 0.5) / double(n) - 0.5) * double(span) * (nrm[i] / l));
    return out;
}

void VolumeRenderCL::renderSlices(size_t width, size_t height, const std::vector<slice_params> &slices,
                                  std::vector<float> &output)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    pushParams();
    output.resize(slices.size() * width * height * 4);
    check("renderSlices", vrhip_render_slices(_r, uint32_t(width), uint32_t(height), slices.data(), uint32_t(slices.size()),
                                              output.data(), 0));
}

void VolumeRenderCL::renderSlices(size_t width, size_t height, const std::vector<slice_params> &slices, float *dev_out)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    pushParams();
    check("renderSlices", vrhip_render_slices(_r, uint32_t(width), uint32_t(height), slices.data(), uint32_t(slices.size()),
                                              dev_out, 1));
}

void VolumeRenderCL::renderDepth(size_t width, size_t height, depth_mode mode, float threshold, depth_image &output,
                                 unsigned int refineSteps, const std::array<unsigned int, 4> &rect)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    vrhip_depth_params p{};
    p.mode = uint32_t(mode);
    p.threshold = threshold;
    p.refineSteps = refineSteps;
    p.x0 = rect[0]; p.y0 = rect[1]; p.w = rect[2]; p.h = rect[3];
    const bool whole = rect[2] == 0 && rect[3] == 0;
    output.width = whole ? width : rect[2];
    output.height = whole ? height : rect[3];
    const size_t n = output.width * output.height;
    output.xyzt.resize(n * 4);
    output.aux.resize(n);
    output.kind.resize(n);
    // the rays of the frame last rendered: its seed is still in the parameters; a pinned seed (setSeed) holds at once
    if (_seedPinned) _rendering_params.seed = _pinnedSeed;
    pushParams();
    // (an empty rectangle -- exactly one of w, h zero -- is the library's to refuse: the pointers only must not be null)
    float none_f[4];
    unsigned char none_k;
    check("renderDepth", vrhip_render_depth(_r, uint32_t(width), uint32_t(height), &p, n ? output.xyzt.data() : none_f,
                                            n ? output.aux.data() : none_f, n ? output.kind.data() : &none_k, 0));
}

VolumeRenderCL::pick_result VolumeRenderCL::pick(size_t width, size_t height, unsigned int x, unsigned int y,
                                                 depth_mode mode, float threshold, unsigned int refineSteps)
{
    depth_image d;
    renderDepth(width, height, mode, threshold, d, refineSteps, {{x, y, 1u, 1u}});
    pick_result res;
    res.hit = d.kind[0] == DEPTH_HIT;
    if (!res.hit) return res;
    uint32_t r4[4] = {0, 0, 0, 0};
    check("pick", vrhip_get_resolution(_r, r4));
    for (int i = 0; i < 3; ++i) {
        res.pos[i] = d.xyzt[i];
        res.voxel[i] = (double(d.xyzt[i]) * 0.5 + 0.5) * double(r4[i]);
    }
    res.t = d.xyzt[3];
    res.aux = d.aux[0];
    return res;
}

// (weldMesh, writeStl and writePly: meshio.cpp)
VolumeRenderCL::iso_mesh VolumeRenderCL::extractIsosurface(float iso, bool normals, const mesh_region &region)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    vrhip_mesh_params p{};
    p.isoValue = iso;
    p.normals = normals ? VRHIP_MESH_NORMALS_GRADIENT : VRHIP_MESH_NORMALS_NONE;
    for (int i = 0; i < 3; ++i) { p.lo[i] = region.lo[i]; p.hi[i] = region.hi[i]; }
    uint64_t n = 0;
    check("extractIsosurface", vrhip_isosurface_count(_r, &p, &n));
    iso_mesh m;
    m.positions.resize(size_t(n) * 9);
    if (normals) m.normals.resize(size_t(n) * 9);
    if (n == 0) return m;
    uint64_t got = 0;
    check("extractIsosurface", vrhip_isosurface_extract(_r, &p, m.positions.data(), normals ? m.normals.data() : nullptr, n,
                                                        &got, 0));
    if (got != n) throw std::runtime_error("ERROR: extractIsosurface (the volume changed between count and extraction)");
    return m;
}

VolumeRenderCL::welded_mesh VolumeRenderCL::extractIsosurfaceIndexed(float iso, bool normals, const mesh_region &region)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    vrhip_mesh_params p{};
    p.isoValue = iso;
    p.normals = normals ? VRHIP_MESH_NORMALS_GRADIENT : VRHIP_MESH_NORMALS_NONE;
    for (int i = 0; i < 3; ++i) { p.lo[i] = region.lo[i]; p.hi[i] = region.hi[i]; }
    uint64_t nv = 0, nt = 0;
    check("extractIsosurfaceIndexed", vrhip_isosurface_count_indexed(_r, &p, &nv, &nt));
    welded_mesh m;
    m.vertices.resize(size_t(nv) * 3);
    if (normals) m.normals.resize(size_t(nv) * 3);
    m.indices.resize(size_t(nt) * 3);
    if (nt == 0) return m;
    uint64_t got_v = 0, got_t = 0;
    check("extractIsosurfaceIndexed", vrhip_isosurface_extract_indexed(_r, &p, m.vertices.data(), normals ? m.normals.data() : nullptr,
                                                                       m.indices.data(), nv, nt, &got_v, &got_t, 0));
    if (got_v != nv || got_t != nt)
        throw std::runtime_error("ERROR: extractIsosurfaceIndexed (the volume changed between count and extraction)");
    return m;
}

VolumeRenderCL::volume_stats VolumeRenderCL::volumeStatistics(const stats_params &params)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    vrhip_stats_params p{};
    for (int i = 0; i < 3; ++i) { p.lo[i] = params.region.lo[i]; p.hi[i] = params.region.hi[i]; }
    p.bins_v = params.vBins;
    p.bins_g = params.gBins;
    p.v_lo = params.vLo;
    p.v_hi = params.vHi;
    p.g_hi = params.gHi;
    p.flags = params.moments ? VRHIP_STATS_MOMENTS : 0u;
    if (vrhip_stats_params_check(&p) != VRHIP_OK)   // (before the table is sized by the bins)
        throw std::invalid_argument("volumeStatistics: bins, window or gradient range out of range");
    volume_stats out;
    out.hist.resize(size_t(p.bins_v) * p.bins_g);
    vrhip_volume_stats st{};
    check("volumeStatistics", vrhip_volume_statistics(_r, &p, &st, out.hist.data(), 0));
    out.voxels = st.voxels;
    out.nan = st.nan;
    out.below = st.below;
    out.above = st.above;
    out.gradientNan = st.gradient_nan;
    out.binned = st.binned;
    out.min = st.min;
    out.max = st.max;
    out.sum = st.sum;
    out.sumSq = st.sum_sq;
    return out;
}

void VolumeRenderCL::filterVolume(const FilterParams &params, size_t dstTimestep)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    vrhip_filter_params p{};
    p.kind = params.median ? VRHIP_FILTER_MEDIAN3 : VRHIP_FILTER_SEPARABLE;
    for (size_t a = 0; a < 3; ++a) {
        p.radius[a] = params.radius[a];
        for (size_t k = 0; k <= VRHIP_FILTER_MAX_RADIUS; ++k) p.taps[a][k] = params.taps[a][k];
    }
    if (vrhip_filter_params_check(&p) != VRHIP_OK) throw std::invalid_argument("filterVolume: radius or taps out of range");
    check("filterVolume", vrhip_filter_volume(_r, &p, uint32_t(dstTimestep)));
    if (!_tff.empty()) generateBricks();
    if (dstTimestep == _timestep) _rendering_params.iteration = 0;
}

void VolumeRenderCL::gaussianFilter(double sigma, unsigned int radius)
{
    if (!(std::isfinite(sigma) && sigma > 0.0) || radius > VRHIP_FILTER_MAX_RADIUS)
        throw std::invalid_argument("gaussianFilter: sigma must be finite and positive, radius at most 8");
    double thickness[3] = {1.0, 1.0, 1.0};
    if (!_synthetic && _dr.has_data())
        for (size_t a = 0; a < 3; ++a) thickness[a] = _dr.properties().slice_thickness.at(a);
    FilterParams fp;
    for (size_t a = 0; a < 3; ++a) {
        const double s = thickness[a] > 0.0 ? sigma * thickness[0] / thickness[a] : sigma;
        const unsigned int r = radius ? radius : unsigned(std::min(std::ceil(3.0 * s), double(VRHIP_FILTER_MAX_RADIUS)));
        float w[VRHIP_FILTER_MAX_RADIUS + 1];
        if (vrhip_filter_gaussian_taps(s, r, w) != VRHIP_OK) throw std::invalid_argument("gaussianFilter: sigma out of range");
        fp.radius[a] = r;
        for (size_t k = 0; k <= VRHIP_FILTER_MAX_RADIUS; ++k) fp.taps[a][k] = w[k];
    }
    filterVolume(fp, _timestep);
}

void VolumeRenderCL::medianFilter()
{
    FilterParams fp;
    fp.median = true;
    filterVolume(fp, _timestep);
}

VolumeRenderCL::filter_info VolumeRenderCL::lastFilterInfo()
{
    vrhip_filter_info fi{};
    check("lastFilterInfo", vrhip_last_filter_info(_r, &fi));
    filter_info out;
    out.blocks = fi.blocks;
    out.blocksFetched = fi.blocks_fetched;
    out.blocksSkipped = fi.blocks_skipped;
    out.scratchBytes = fi.scratch_bytes;
    out.emptySkip = fi.empty_skip != 0;
    out.inPlace = fi.in_place != 0;
    return out;
}

void VolumeRenderCL::morphVolume(const MorphParams &params, size_t dstTimestep)
{
    if (!_volLoaded) throw std::runtime_error("No volume data is loaded.");
    vrhip_morph_params p{};
    p.op = uint32_t(params.op);
    p.shape = params.ball ? VRHIP_MORPH_BALL : VRHIP_MORPH_BOX;
    for (size_t a = 0; a < 3; ++a) p.radius[a] = params.radius[a];
    if (vrhip_morph_params_check(&p) != VRHIP_OK) throw std::invalid_argument("morphVolume: op or radius out of range");
    check("morphVolume", vrhip_morph_volume(_r, &p, uint32_t(dstTimestep)));
    if (!_tff.empty()) generateBricks();
    if (dstTimestep == _timestep) _rendering_params.iteration = 0;
}

void VolumeRenderCL::erode(unsigned int radius, bool ball)
{
    morphVolume(MorphParams{MorphOp::Erode, ball, {{radius, radius, radius}}}, _timestep);
}

void VolumeRenderCL::dilate(unsigned int radius, bool ball)
{
    morphVolume(MorphParams{MorphOp::Dilate, ball, {{radius, radius, radius}}}, _timestep);
}

void VolumeRenderCL::open(unsigned int radius, bool ball)
{
    morphVolume(MorphParams{MorphOp::Open, ball, {{radius, radius, radius}}}, _timestep);
}

void VolumeRenderCL::close(unsigned int radius, bool ball)
{
    morphVolume(MorphParams{MorphOp::Close, ball, {{radius, radius, radius}}}, _timestep);
}

VolumeRenderCL::morph_info VolumeRenderCL::lastMorphInfo()
{
    vrhip_morph_info mi{};
    check("lastMorphInfo", vrhip_last_morph_info(_r, &mi));
    morph_info out;
    for (size_t s = 0; s < 2; ++s) {
        out.blocks[s] = mi.sweep[s].blocks;
        out.blocksFetched[s] = mi.sweep[s].blocks_fetched;
        out.blocksSkipped[s] = mi.sweep[s].blocks_skipped;
    }
    out.scratchBytes = mi.scratch_bytes;
    out.sweeps = mi.sweeps;
    out.emptySkip = mi.empty_skip != 0;
    out.inPlace = mi.in_place != 0;
    return out;
}

void VolumeRenderCL::renderSlicesRGBA8(size_t width, size_t height, const std::vector<slice_params> &slices,
                                       float *dev_frames, unsigned char *out, bool outIsDevice)
{
    renderSlices(width, height, slices, dev_frames);
    check("renderSlicesRGBA8", vrhip_quantise_rgba8(_r, stream(), dev_frames, uint32_t(slices.size()), uint32_t(width * height),
                                                    uint32_t(width * height), out, outIsDevice ? 1 : 0));
}

// ---- the progressive path tracer, many samples per call (vrhip_render_samples)

void VolumeRenderCL::renderSamples(size_t width, size_t height, const std::vector<unsigned int> &seeds,
                                   std::vector<float> &output, unsigned int samplesPerLaunch)
{
    if (!_volLoaded) return;
    pushParams();
    output.resize(width * height * 4);
    check("renderSamples", vrhip_render_samples(_r, uint32_t(width), uint32_t(height), 0, 0, nullptr, 0, seeds.data(),
                                                uint32_t(seeds.size()), samplesPerLaunch, output.data(), 0));
    _rendering_params.iteration += static_cast<unsigned int>(seeds.size());
}

void VolumeRenderCL::renderSamples(size_t width, size_t height, const std::vector<unsigned int> &seeds, float *dev_out,
                                   unsigned int samplesPerLaunch)
{
    if (!_volLoaded) return;
    pushParams();
    check("renderSamples", vrhip_render_samples(_r, uint32_t(width), uint32_t(height), 0, 0, nullptr, 0, seeds.data(),
                                                uint32_t(seeds.size()), samplesPerLaunch, dev_out, 1));
    _rendering_params.iteration += static_cast<unsigned int>(seeds.size());
}

void VolumeRenderCL::renderSamples(size_t width, size_t height, size_t tile_w, size_t tile_h,
                                   const std::vector<unsigned int> &tile_ids, const std::vector<unsigned int> &seeds,
                                   float *dev_out, unsigned int samplesPerLaunch)
{
    if (!_volLoaded) return;
    pushParams();
    check("renderSamples", vrhip_render_samples(_r, uint32_t(width), uint32_t(height), uint32_t(tile_w), uint32_t(tile_h),
                                                tile_ids.data(), uint32_t(tile_ids.size()), seeds.data(),
                                                uint32_t(seeds.size()), samplesPerLaunch, dev_out, 1));
    _rendering_params.iteration += static_cast<unsigned int>(seeds.size());
}

std::vector<unsigned int> VolumeRenderCL::drawSeeds(size_t n)
{
    std::vector<unsigned int> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = _seedPinned ? _pinnedSeed : static_cast<unsigned int>(_generator());
    return out;
}

void VolumeRenderCL::setRoundBudget(unsigned int rounds)
{
    _roundBudget = rounds;
    check("setRoundBudget", vrhip_set_round_budget(_r, rounds));
}

void VolumeRenderCL::setFrameTiming(bool on) { check("setFrameTiming", vrhip_set_frame_timing(_r, on ? 1 : 0)); }

void *VolumeRenderCL::stream()
{
    void *s = nullptr;
    check("stream", vrhip_get_stream(_r, &s));
    return s;
}

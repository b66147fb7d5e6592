// A caller of the device-side ingest, compiled against include/ ALONE (tests/test_gpu_ingest.py): the same
// .dat file loaded by the host loader and with setDeviceIngest(true), a frame from each, the histograms of both,
// and the histogram of a synthetic volume.  Exit code 0: frames and histograms are bit-identical.
#include <volumerendercl.h>

#include <cstdio>
#include <cstring>

static std::vector<float> frame(VolumeRenderCL &vr, const char *dat, bool deviceIngest, std::array<double, 256> &hist)
{
    vr.initialize(false, false);
    vr.setDeviceIngest(deviceIngest);
    DatRawReader::Properties props;
    props.dat_file_name = dat;
    vr.loadVolumeData(props);
    std::vector<unsigned char> tff(1024 * 4, 0);
    for (size_t i = 0; i < 1024; ++i) {
        tff[4 * i] = (unsigned char)(i / 4);
        tff[4 * i + 3] = (unsigned char)(i / 8);
    }
    vr.setTransferFunction(tff);
    vr.setSeed(7u);
    vr.updateView({{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2, 0, 0, 0, 1}});
    std::vector<float> out;
    vr.runRaycastNoGL(64, 48, out);
    hist = vr.getHistogram(0);
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        VolumeRenderCL host, device, synth;
        std::array<double, 256> hh, hd;
        const std::vector<float> a = frame(host, argv[1], false, hh);
        const std::vector<float> b = frame(device, argv[1], true, hd);
        if (a.size() != b.size() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) != 0) {
            std::fprintf(stderr, "frames differ\n");
            return 1;
        }
        if (hh != hd) {
            std::fprintf(stderr, "histograms differ\n");
            return 1;
        }
        synth.initialize(false, false);
        synth.loadSyntheticVolume("shells", 24, DatRawReader::USHORT);
        double total = 0.0, synthTotal = 0.0;
        for (double v : hd) total += v;
        for (double v : synth.getHistogram(0)) synthTotal += v;
        std::printf("%zu floats identical, histogram total %.0f, synthetic total %.0f\n", a.size(), total, synthTotal);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

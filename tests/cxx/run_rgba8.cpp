// Runs the host class's 8-bit frame methods (tests/test_gpu_rgba8.py builds and starts it): two renderers draw the same
// jitter seeds from their default-seeded generators; A renders two accumulating path-tracer frames with
// runRaycastNoGL, B the same two with runRaycastRGBA8.  Writes A's floats (PREFIX.a<k>.f32), B's bytes (PREFIX.b<k>.u8),
// the bytes of A's last frame from its frame buffer (PREFIX.a1.u8, frameRGBA8) and a launch set's frames both ways
// (PREFIX.set.f32 / PREFIX.set.u8, renderFramesRGBA8); prints B's iteration count.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "volumerendercl.h"

template <class T>
static void dump(const std::string &path, const std::vector<T> &v)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char *>(v.data()), std::streamsize(v.size() * sizeof(T)));
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const std::string prefix = argv[1];
    const size_t W = 40, H = 24;
    try {
        std::vector<unsigned char> tff(1024 * 4);
        for (size_t i = 0; i < 1024; ++i) {
            tff[i * 4 + 0] = static_cast<unsigned char>(i / 4);
            tff[i * 4 + 1] = static_cast<unsigned char>(255 - i / 4);
            tff[i * 4 + 2] = 90;
            tff[i * 4 + 3] = static_cast<unsigned char>(i / 8);
        }
        VolumeRenderCL a, b;
        for (VolumeRenderCL *vr : {&a, &b}) {
            vr->initialize();
            vr->loadSyntheticVolume("sphere", 32, DatRawReader::UCHAR);
            vr->setTransferFunction(tff);
            vr->setTechnique(VolumeRenderCL::TECH_PATHTRACE);
        }
        std::vector<float> f32;
        std::vector<unsigned char> u8;
        for (int k = 0; k < 2; ++k) {
            a.runRaycastNoGL(W, H, f32);
            dump(prefix + ".a" + std::to_string(k) + ".f32", f32);
            b.runRaycastRGBA8(W, H, u8);
            dump(prefix + ".b" + std::to_string(k) + ".u8", u8);
        }
        a.frameRGBA8(W, H, u8);
        dump(prefix + ".a1.u8", u8);
        std::printf("iteration %u %u\n", a.renderingParams().iteration, b.renderingParams().iteration);
        // a launch set, floats and bytes from the same launches
        b.setTechnique(VolumeRenderCL::TECH_RAYCAST);
        const std::vector<unsigned int> seeds{11u, 22222u, 3333333u};
        const size_t n = seeds.size() * W * H * 4;
        float *dev32 = nullptr;
        unsigned char *dev8 = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&dev32), n * sizeof(float)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&dev8), n) != hipSuccess)
            return 3;
        b.renderFramesRGBA8(W, H, seeds, dev32, dev8);
        f32.resize(n);
        u8.resize(n);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(f32.data(), dev32, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(u8.data(), dev8, n, hipMemcpyDeviceToHost) != hipSuccess)
            return 3;
        dump(prefix + ".set.f32", f32);
        dump(prefix + ".set.u8", u8);
        (void)hipFree(dev32);
        (void)hipFree(dev8);
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}

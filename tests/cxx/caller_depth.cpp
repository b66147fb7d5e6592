// A caller of the depth images through the C++ class, compiled against include/ ALONE (tests/test_gpu_depth.py):
// VolumeRenderCL::renderDepth in the three modes and on a rectangle, and VolumeRenderCL::pick, between two progressive
// ray-cast frames of the same renderer.  Writes to argv[1], raw: the two frames (float32), then per depth image xyzt
// (float32), aux (float32), kind (bytes) -- ISO, MAX, OPACITY over the whole frame, ISO on the rectangle -- then the
// pick: hit (one float32, 0 or 1), pos[3], t, aux (float32) and voxel[3] (float64).
#include <volumerendercl.h>

#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    try {
        const size_t W = 45, H = 29;
        VolumeRenderCL vr;
        vr.initialize(false, false);
        vr.loadSyntheticVolume("sphere", 32, DatRawReader::UCHAR);
        std::vector<unsigned char> tff(256 * 4, 0);
        for (size_t i = 0; i < 256; ++i) {
            tff[4 * i] = (unsigned char)i;
            tff[4 * i + 1] = (unsigned char)(255 - i);
            tff[4 * i + 2] = 40;
            tff[4 * i + 3] = (unsigned char)i;
        }
        vr.setTransferFunction(tff);
        vr.updateSamplingRate(1.5);
        vr.updateOutputImg(W, H, 0);
        vr.updateView({{2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 2, 0, 0, 0, 1}});
        vr.setSeed(77);
        static_assert(sizeof(vrhip_depth_params) == 32 && sizeof(vrhip_depth_info) == 32, "32 bytes each");
        std::vector<float> a, b;
        VolumeRenderCL::depth_image iso, mx, op, part;
        vr.runRaycastNoGL(W, H, a);          // iteration 0
        vr.renderDepth(W, H, VolumeRenderCL::DEPTH_ISO, 0.4f, iso, 6);
        vr.renderDepth(W, H, VolumeRenderCL::DEPTH_MAX, 0.f, mx);
        vr.renderDepth(W, H, VolumeRenderCL::DEPTH_OPACITY, 0.6f, op);
        vr.renderDepth(W, H, VolumeRenderCL::DEPTH_ISO, 0.4f, part, 6, {{5, 3, 13, 9}});
        const VolumeRenderCL::pick_result p = vr.pick(W, H, 22, 14, VolumeRenderCL::DEPTH_ISO, 0.4f, 6);
        const VolumeRenderCL::pick_result none = vr.pick(W, H, 0, 0, VolumeRenderCL::DEPTH_ISO, 0.4f, 6);
        vr.setSeed(78);
        vr.runRaycastNoGL(W, H, b);          // iteration 1, another jitter: accumulates on a
        if (none.hit || !p.hit) return 5;
        if (iso.width != W || iso.height != H || part.width != 13 || part.height != 9) return 5;
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 3;
        for (const std::vector<float> *v : {&a, &b})
            if (v->size() != W * H * 4 || std::fwrite(v->data(), sizeof(float), v->size(), f) != v->size()) return 4;
        for (const VolumeRenderCL::depth_image *d : {&iso, &mx, &op, &part}) {
            const size_t n = d->width * d->height;
            if (d->xyzt.size() != 4 * n || d->aux.size() != n || d->kind.size() != n) return 4;
            if (std::fwrite(d->xyzt.data(), sizeof(float), 4 * n, f) != 4 * n) return 4;
            if (std::fwrite(d->aux.data(), sizeof(float), n, f) != n) return 4;
            if (std::fwrite(d->kind.data(), 1, n, f) != n) return 4;
        }
        const float pf[6] = {p.hit ? 1.f : 0.f, p.pos[0], p.pos[1], p.pos[2], p.t, p.aux};
        if (std::fwrite(pf, sizeof(float), 6, f) != 6 || std::fwrite(p.voxel.data(), sizeof(double), 3, f) != 3) return 4;
        std::fclose(f);
        std::printf("%zu pixels\n", W * H);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}

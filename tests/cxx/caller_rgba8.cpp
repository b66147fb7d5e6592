// A caller of the 8-bit frame interface, compiled against include/ alone (tests/test_rgba8_abi.py): the C ABI's four
// entry points and the host class's methods as a GUI, a recorder or a stream encoder would use them.
#include <cstdint>
#include <vector>

#include "volumerendercl.h"
#include "vrhip.h"

int main()
{
    const size_t W = 64, H = 48;
    VolumeRenderCL vr;
    std::vector<unsigned char> image;
    vr.runRaycastRGBA8(W, H, image);                      // width * height * 4 bytes, row 0 = top
    float *dev_frames = nullptr;      // (device memory in a real caller)
    unsigned char *dev = nullptr;
    const std::vector<unsigned int> seeds{1u, 2u, 3u};
    vr.renderFramesRGBA8(W, H, seeds, dev_frames, dev);
    const std::vector<std::array<float, 16>> views(seeds.size());
    vr.renderFramesRGBA8(W, H, seeds, views, dev_frames, dev);

    vrhip_renderer *r = nullptr;
    const float *src = nullptr;
    uint8_t *dst = nullptr;
    int rc = vrhip_quantise_rgba8(r, nullptr, src, 3u, 37u, 64u, dst, 1);
    rc |= vrhip_render_frame_rgba8(r, uint32_t(W), uint32_t(H), dst, 0);
    int32_t *scratch = nullptr;
    uint32_t *msg = nullptr, *count = nullptr;
    rc |= vrhip_pack_tiles_rgba8(r, nullptr, src, 6u, 256u, scratch, msg, count);
    const uint32_t *const *msgs = nullptr;
    const int32_t *pos = nullptr;
    const uint32_t *rank_slot = nullptr;
    rc |= vrhip_assemble_batch_rgba8(r, nullptr, msgs, 1u, 1u, 6u, 8u, pos, rank_slot, uint32_t(W), uint32_t(H), 16u, 16u, dst);
    return rc == VRHIP_OK ? 0 : 1;
}

// vr_raycast_kernels.h -- the per-pixel front-to-back ray march for gfx950 (CDNA4): device code, the kernel
// templates and their launcher.  Everything here is templated on the voxel type and is instantiated in two units that
// compile side by side: vr_raycast_int.hip (UCHAR and USHORT) and vr_raycast_f32.hip (FLOAT); vr_raycast.hip holds
// what does not depend on the voxel type and the format switch.
//
// Replaces the reference's OpenCL kernel `volumeRender`
// (/root/reference/src/kernel/volumeraycast.cl:589-926).  CDNA has no image/sampler
// hardware (__HIP_NO_IMAGE_SUPPORT), so every read_imagef of the reference is restated
// as explicit address arithmetic + loads following the OpenCL 1.2 image rules
// (vr_sampling.h).
//
// Execution design, four launches per frame on one stream:
//  * PRE-PASS (vr_dda_prepass_kernel, with ESS): one wave per 8x8-pixel patch (the reference's
//    work-group) at high occupancy: ray set-up and the reference's DDA up to the first brick the
//    ESS bitmap does not skip.  Rays that never reach one get their background pixel here; the
//    others go to a ray list with the DDA state they have reached.
//  * PHASE 1 (vr_raycast_rays_kernel on that list; vr_raycast_kernel on 8x8 patches for the
//    instrumented / XS variants and without ESS): one lane per ray in PERSISTENT waves.  The
//    transfer function (float4 table) and the ESS skip bitmap (1 bit per brick, precomputed from
//    bricks + TF + prefix sum) live in LDS: a DDA step touches no global memory.  The reference's
//    nested loops (DDA over bricks / samples inside a brick) are flattened into a per-lane state
//    machine driven by wave ballots; each sample round evaluates up to kBatch consecutive samples
//    of every ray as independent straight-line code.
//  * The frame time of a ray caster on a machine this wide is set by its LONGEST rays: their
//    samples form a serial chain.  So phase 1 marches a ray for at most `round_budget` sample
//    rounds; rays still alive are SUSPENDED (13 words of state), counting-sorted by the rounds
//    their pixel needed in the previous frame (longest first), and
//  * PHASE 2 (vr_raycast_split_kernel) resumes them with kSplit = 4 lanes per ray: each lane
//    evaluates 4 of the ray's next 16 consecutive samples, then the 16 contributions are
//    composited in ray order (in-quad DPP broadcasts).  The chain of a long ray shrinks 4x; the
//    16 ray slots of a wave draw their rays one by one from the sorted list.
//  Several independent frames (jitter seeds) can share one set of these launches: the work items
//  carry a frame index (vrhip_render_batch).
//  The per-ray sequence of t values and of fp32 operations is exactly the reference's in every
//  kernel, so the image is bit-identical whatever the schedule (budget, refill, batch, lists).
//  Where that is enforced: the kernels share one batch ladder (VR_BATCH_PARAMS, VR_BATCH_PARAMS_SPLIT), one ray record
//  (VR_PACK_RAY, VR_UNPACK_RAY) and one compositing step (composite, VR_COMPOSITE_QUAD), defined once below.
#pragma once
#include <algorithm>
#include <vector>

#include "vr_sampling.h"

// The units' entries: the ray-cast launches of one frame (or set of frames) for volumes of one voxel type, with the
// launch's camera or with per-frame cameras (FrameView::cams).  vr_launch_raycast picks one by RaycastLaunch::format.
hipError_t vr_launch_raycast_u8(const RaycastLaunch &a, hipStream_t stream);
hipError_t vr_launch_raycast_u16(const RaycastLaunch &a, hipStream_t stream);
hipError_t vr_launch_raycast_f32(const RaycastLaunch &a, hipStream_t stream);
// between the phases: the counting sort of the suspended rays (FrameView::order); vr_raycast.hip
hipError_t vr_launch_cont_sort(const FrameView &frame, hipStream_t stream);
// between the pre-pass and phase 1, pixel-major order only (FrameView::pm): the index into the ray lists; vr_raycast.hip
hipError_t vr_launch_regroup(const FrameView &frame, uint32_t group, hipStream_t stream);
#if defined(VR_MARCH_STATS) || defined(VR_STAMPS)
// Diagnostic builds: every unit has its own copy of the arrays its kernels write (g_march_stats, g_stamps,
// g_wave_span).  A unit's reader ADDS its copy of array `which` to sum[0, n) and clears the copy on request; the
// vrhip_debug_* entry points (vr_raycast.hip) add up the units'.
enum { VR_DEBUG_MARCH_STATS = 0, VR_DEBUG_STAMPS = 1, VR_DEBUG_WAVE_SPAN = 2 };
int vr_raycast_debug_int(int which, unsigned long long *sum, size_t n, int reset);
int vr_raycast_debug_f32(int which, unsigned long long *sum, size_t n, int reset);
#endif

namespace {

constexpr int kSplit = 4;           // lanes per ray in phase 2 (x kBatch samples per lane)

#ifdef VR_MARCH_STATS   // diagnostic build: what the waves of the marching kernels spend their rounds on
__device__ unsigned long long g_march_stats[32];   // [16, 26) phase 1 on the ray list, [28, 32) pre-pass; [0, 16) unused
#define VR_MS(i, v) ms_acc[i] += (unsigned long long)(v)
#else
#define VR_MS(i, v)
#endif
#ifdef VR_ISA_MARKS   // diagnostic: comments in the -S output that delimit the stages (tools/isa_marks.py)
#define VR_MARK(x) asm volatile("; VRMARK " x ::: "memory")
#else
#define VR_MARK(x)
#endif

// Occupancy experiments: -DVR_WAVES_PER_EU=N asks the compiler to fit N waves per SIMD
#ifdef VR_WAVES_PER_EU
#define VR_OCC __attribute__((amdgpu_waves_per_eu(VR_WAVES_PER_EU, VR_WAVES_PER_EU)))
#else
#define VR_OCC
#endif

struct RayCtx {   // per-ray invariants, recomputable from the pixel
    f3 cam, dir;
    float env0, env1, env2, env3;
    float tnear;      // clamped to >= 0 (:719)
    float tfar, sampleDist, stepSize, offset;
    f3 lgt, hv;       // illumination invariants (:280-303)
    bool hvalid;
    int stepv0, stepv1, stepv2, exit0, exit1, exit2;
    float dT0, dT1, dT2;
    bool valid;       // hits the clip box with sampleDist > 0
    bool miss;        // inside the image, misses the clip box (image-order ESS bookkeeping)
    float nominal;    // ceil(sampleDist / stepSize)
};

struct RayDyn {   // marching state
    int state;
    float t, t_exit, alpha, r0, r1, r2;
    int c0, c1, c2;
    float tv0, tv1, tv2;
    uint32_t cidx, skw;   // linear index of the current brick cell and its bitmap word
    float t_last;         // XS variants: ray parameter of the last sample taken, < 0 = none (showEss)
    float t_ert;          // ray parameter of the sample that triggered early ray termination
    bool ert;             // (ambient occlusion is applied there, :870-876)
#ifdef VR_RAYLEN          // diagnostic build: samples taken by the ray, written to the alpha channel
    uint32_t nsmp;
#endif
};
#ifdef VR_RAYLEN
#define VR_RAYLEN_INC(d) ((d).nsmp++)
#define VR_RAYLEN_PACK(r, d) (r).pad = (d).nsmp     // (the diagnostic build carries the sample count in the key's place)
#define VR_RAYLEN_UNPACK(rec, d) (d).nsmp = (rec).pad
#else
#define VR_RAYLEN_INC(d)
#define VR_RAYLEN_PACK(r, d)
#define VR_RAYLEN_UNPACK(rec, d)
#endif

// ---- The blocks the four kernels share, one definition each -- as MACROS, expanded in the kernel bodies.  As inlined
// functions each of them, tried alone, changed the device code of some kernels (other registers, another order of
// independent instructions: this compiler follows the order in which a kernel's locals come into being); expanded in
// place the kernels compile to what they were (DESIGN.md "Build").  They name the kernels' locals (d, c, fr, vv, ...)
// where the blocks did.

// The ray record: ContRec `r` from the ray's RayDyn d, its pixel, its frame of the batch (state >> 8: states fit 8 bits)
// and the sort key; and back: pixel and frame first, then the caller's setup_ray for that pixel (SETUP..., which leaves
// c and a fresh d), then the state the record holds.  The only code that names ContRec's fields (the sort reads pad).
#define VR_PACK_RAY(r, OUT_INDEX, FRAME, KEY)                 \
    ContRec r;                                                \
    r.pix = gx | (gy << 16);                                  \
    r.out_index = OUT_INDEX;                                  \
    r.state = d.state | (int32_t)(FRAME << 8);                \
    r.t = d.t; r.t_exit = d.t_exit; r.alpha = d.alpha;        \
    r.r0 = d.r0; r.r1 = d.r1; r.r2 = d.r2;                    \
    r.cx = d.c0; r.cy = d.c1; r.cz = d.c2;                    \
    r.tv0 = d.tv0; r.tv1 = d.tv1; r.tv2 = d.tv2;              \
    r.pad = KEY;                                              \
    VR_RAYLEN_PACK(r, d)
#define VR_UNPACK_RAY(rec, FRAME, ...)                        \
    gx = rec.pix & 0xffffu;                                   \
    gy = rec.pix >> 16;                                       \
    out_index = rec.out_index;                                \
    FRAME = (uint32_t)rec.state >> 8;                         \
    __VA_ARGS__                                               \
    d.state = rec.state & 0xff;                               \
    d.t = rec.t; d.t_exit = rec.t_exit; d.alpha = rec.alpha;  \
    d.r0 = rec.r0; d.r1 = rec.r1; d.r2 = rec.r2;              \
    d.c0 = rec.cx; d.c1 = rec.cy; d.c2 = rec.cz;              \
    d.tv0 = rec.tv0; d.tv1 = rec.tv1; d.tv2 = rec.tv2;        \
    VR_RAYLEN_UNPACK(rec, d)
#define VR_SORT_KEY (fr.cost ? (uint32_t)fr.cost[(size_t)gy * fr.W + gx] : 0u)   // last frame's phase-2 rounds of the pixel

// The wave-wide append: the first lane of MASK (not 0) moves the list's counter for all its lanes; `base` is the first
// slot, lane's slot is base + VR_LANE_RANK.
#define VR_WAVE_APPEND(base, COUNTER, MASK)                                    \
    uint32_t base = 0;                                                         \
    if (lane == (uint32_t)__builtin_ctzll(MASK))                               \
        base = atomicAdd(COUNTER, (uint32_t)__builtin_popcountll(MASK));       \
    base = __shfl(base, __builtin_ctzll(MASK), 64)
#define VR_LANE_RANK(MASK) ((uint32_t)__builtin_popcountll(MASK & ((1ull << lane) - 1ull)))
// Pixel-major order: the pre-pass's note for work item q -- the ballot of its live rays and the position of the first of
// their records in live_rays (vr_internal.h; vr_regroup_kernel reads them).  Every wave of the pre-pass leaves one,
// whichever way it ends: nothing else initialises the block.
#define VR_PM_NOTE(fr, q, MASK, FIRST)                                      \
    do {                                                                    \
        if ((fr).pm && lane == 0) {                                         \
            (fr).pm[2u * (q)] = (uint32_t)(MASK);                           \
            (fr).pm[2u * (q) + 1u] = (uint32_t)((MASK) >> 32);              \
            (fr).pm[2u * (fr).n_wave_tiles + (q)] = (FIRST);                \
        }                                                                   \
    } while (0)

struct Grid {     // wave-uniform brick-grid constants
    int bw, bh, bd;
    float bl0, bl1, bl2, brickDia;
    uint32_t oob_word;
};

// volumeraycast.cl:605-683 for one pixel: ray, background, clip.  The first half of setup_ray: all the
// pre-pass's patch culling needs (and all a ray that is never marched needs: write_pixel reads the
// background and the clip result).  SHADE: the illumination invariants (:280-303).
template <bool SHADE>
VR_DEV void setup_ray_head(uint32_t gx, uint32_t gy, bool inside, const FrameView &fr,
                           const vrhip_camera_params &cam, const vrhip_rendering_params &rp, RayCtx &c,
                           RayDyn &d, uint32_t seed, float &rnd)
{
    const Ray ray = make_ray(gx, gy, fr, cam, rp, seed);
    rnd = ray.rnd;
    c.cam = ray.cam;
    c.dir = ray.dir;
    c.env0 = ray.env[0]; c.env1 = ray.env[1]; c.env2 = ray.env[2]; c.env3 = ray.env[3];
    c.tfar = ray.tfar;
    c.sampleDist = ray.tfar - ray.tnear;
    c.valid = inside && ray.hit && c.sampleDist > 0.f;
    c.miss = inside && !ray.hit;
    c.tnear = ray.tnear;
    c.stepSize = 0.f; c.offset = 0.f; c.nominal = 0.f;
    c.stepv0 = c.stepv1 = c.stepv2 = 0;
    c.exit0 = c.exit1 = c.exit2 = 0;
    c.dT0 = c.dT1 = c.dT2 = 0.f;
    if (SHADE) {
        const f3 toLight = neg3(ray.dir);
        c.lgt = normalize3(toLight);
        f3 hv = add3(toLight, c.lgt);
        c.hvalid = !(dot3(hv, hv) < 1.e-6f);
        c.hv = normalize3(hv);
    } else {
        c.lgt = c.hv = mk3(0.f, 0.f, 0.f);
        c.hvalid = false;
    }

    d.state = S_DONE;
    d.t = 0.f; d.t_exit = ray.tfar; d.alpha = 0.f;
    d.r0 = c.env0; d.r1 = c.env1; d.r2 = c.env2;
    d.c0 = d.c1 = d.c2 = 0;
    d.tv0 = d.tv1 = d.tv2 = 0.f;
    d.cidx = 0; d.skw = 0;
    d.t_ert = 0.f; d.ert = false;
    d.t_last = -1.f;
#ifdef VR_RAYLEN
    d.nsmp = 0;
#endif
    if (c.valid) c.tnear = vmax(0.f, ray.tnear);   // :719 (the unclamped value is not needed again)
}

// volumeraycast.cl:709-760: step size, jitter offset, DDA set-up -- for rays that will be marched.
template <bool ESS>
VR_DEV void setup_ray_tail(const vrhip_raycast_params &rcp, f3 resf, f3 voxLen, const Grid &g, RayCtx &c,
                           RayDyn &d, float rnd)
{
    if (c.valid) {
        // volumeraycast.cl:709-733
        float stepSize = vmin(c.sampleDist,
                              c.sampleDist / (rcp.samplingRate *
                                              len3(mul3(scale3(c.dir, c.sampleDist), resf))));
        c.nominal = ceilf(c.sampleDist / stepSize);
        c.stepSize = c.sampleDist / c.nominal;
        d.t = c.tnear;
        c.offset = (len3(voxLen) * rnd) * 2.0f;
        d.state = ESS ? S_BRICK : S_SAMPLE;
        if (ESS) {   // 3-D DDA set-up (:737-760)
            const int bres[3] = {g.bw, g.bh, g.bd};
            const float bl[3] = {g.bl0, g.bl1, g.bl2};
            const float dirv[3] = {c.dir.x, c.dir.y, c.dir.z};
            const float camv[3] = {c.cam.x, c.cam.y, c.cam.z};
            int stepv[3], cell[3], exitc[3];
            float tv[3], dT[3];
            for (int i = 0; i < 3; ++i) {
                float invRay = 1.f / dirv[i];
                stepv[i] = dirv[i] > 0.f ? 1 : (dirv[i] < 0.f ? -1 : 0);
                dT[i] = (float)stepv[i] * ((bl[i] * 2.f) * invRay);
                float roc = (camv[i] + dirv[i] * c.tnear) - (-1.f);
                cell[i] = iclamp((int)floorf(roc / (2.f * bl[i])), 0, bres[i] - 1);
                int cadj = cell[i] - (dirv[i] >= 0.f ? -1 : 0);
                tv[i] = c.tnear + ((float)cadj * (2.f * bl[i]) - roc) * invRay;
                exitc[i] = stepv[i] * bres[i];
                if (exitc[i] < 0) exitc[i] = -1;
            }
            c.stepv0 = stepv[0]; c.stepv1 = stepv[1]; c.stepv2 = stepv[2];
            c.exit0 = exitc[0]; c.exit1 = exitc[1]; c.exit2 = exitc[2];
            c.dT0 = dT[0]; c.dT1 = dT[1]; c.dT2 = dT[2];
            d.c0 = cell[0]; d.c1 = cell[1]; d.c2 = cell[2];
            d.tv0 = tv[0]; d.tv1 = tv[1]; d.tv2 = tv[2];
        }
    }
}

// volumeraycast.cl:605-760 for one pixel: ray, background, clip, step size, DDA set-up.
template <bool ESS>
VR_DEV void setup_ray(uint32_t gx, uint32_t gy, bool inside, const FrameView &fr,
                      const vrhip_camera_params &cam, const vrhip_rendering_params &rp,
                      const vrhip_raycast_params &rcp, f3 resf, f3 voxLen, const Grid &g, RayCtx &c,
                      RayDyn &d, uint32_t seed)
{
    float rnd;
    setup_ray_head<true>(gx, gy, inside, fr, cam, rp, c, d, seed, rnd);
    setup_ray_tail<ESS>(rcp, resf, voxLen, g, c, d, rnd);
}

// Per-frame cameras (FrameView::cams, kernels instantiated with VIEWS = true): frame f's camera, the fields make_ray
// reads -- rows 0-2 of the view matrix, the box, ortho -- from the batch's table.  UNIFORM: f is the same in every lane
// (one patch of one frame per wave) and the values go to scalar registers, as the launch's by-value camera does.
// The VIEWS = false kernels never call this: they compile as they did before the table existed.
template <bool UNIFORM>
VR_DEV vrhip_camera_params load_frame_cam(const vrhip_camera_params *cams, uint32_t f)
{
    if (UNIFORM) f = __builtin_amdgcn_readfirstlane(f);
    const float4 *p = reinterpret_cast<const float4 *>(cams + f);
    vrhip_camera_params k;
    float v[18];
    for (int i = 0; i < 3; ++i) {
        const float4 row = p[i];
        v[4 * i] = row.x; v[4 * i + 1] = row.y; v[4 * i + 2] = row.z; v[4 * i + 3] = row.w;
    }
    const float4 bl = p[4], tr = p[5];
    v[12] = bl.x; v[13] = bl.y; v[14] = bl.z;
    v[15] = tr.x; v[16] = tr.y; v[17] = tr.z;
    uint32_t ortho = reinterpret_cast<const uint32_t *>(p)[24];
    if (UNIFORM) {
        for (int i = 0; i < 18; ++i)
            v[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v[i])));
        ortho = __builtin_amdgcn_readfirstlane(ortho);
    }
    for (int i = 0; i < 12; ++i) k.viewMat[i] = v[i];
    k.viewMat[12] = k.viewMat[13] = k.viewMat[14] = 0.f;
    k.viewMat[15] = 1.f;
    for (int i = 0; i < 3; ++i) { k.bbox_bl[i] = v[12 + i]; k.bbox_tr[i] = v[15 + i]; }
    k.bbox_bl[3] = k.bbox_tr[3] = 0.f;
    k.ortho = ortho;
    for (int i = 0; i < 7; ++i) k._pad[i] = 0u;
    return k;
}

// bitmap word of the cell the ray is in (out-of-range cells read the trailing word, which
// holds the (0,0) decision in every bit)
VR_DEV void fetch_skip_word(const uint32_t *sb, const Grid &g, RayDyn &d)
{
    const bool oob = (uint32_t)d.c0 >= (uint32_t)g.bw || (uint32_t)d.c1 >= (uint32_t)g.bh ||
                     (uint32_t)d.c2 >= (uint32_t)g.bd;
    d.cidx = __umul24(__umul24((uint32_t)d.c2, (uint32_t)g.bh) + (uint32_t)d.c1, (uint32_t)g.bw) +
             (uint32_t)d.c0;
    d.skw = sb[oob ? g.oob_word : (d.cidx >> 5)];
}

// One DDA step (:763-787) as branch-free predicated code (a lone wave pays ~60 cycles per
// ballot + scalar branch; tools/micro_issue.hip).  Every lane computes the step; `go` (lane is
// in S_BRICK and passes the outer loop condition t < tfar) gates what is committed.  The
// decision for the current cell comes from the bitmap word fetched one step ahead.
template <int INSTR>
VR_DEV void dda_step(const uint32_t *sb, const Grid &g, const RayCtx &c, RayDyn &d,
                     unsigned long long &c_bricks, unsigned long long &c_skipped)
{
    const bool inB = d.state == S_BRICK;
    const bool go = inB && (d.t < c.tfar);
    const bool skp = (d.skw >> (d.cidx & 31u)) & 1u;
    const bool m0 = (d.tv0 <= d.tv1) && (d.tv0 <= d.tv2);
    const bool m1 = (d.tv1 <= d.tv0) && (d.tv1 <= d.tv2);
    const bool m2 = (d.tv2 <= d.tv0) && (d.tv2 <= d.tv1);
    const float inc0 = m0 ? 1.f : 0.f, inc1 = m1 ? 1.f : 0.f, inc2 = m2 ? 1.f : 0.f;
    float te = ((d.tv0 * inc0) + (d.tv1 * inc1)) + (d.tv2 * inc2);
    te = vclamp(te, d.t + c.stepSize, d.t + g.brickDia);
    d.c0 += (go && m0) ? c.stepv0 : 0;
    d.c1 += (go && m1) ? c.stepv1 : 0;
    d.c2 += (go && m2) ? c.stepv2 : 0;
    d.tv0 = go ? d.tv0 + inc0 * c.dT0 : d.tv0;
    d.tv1 = go ? d.tv1 + inc1 * c.dT1 : d.tv1;
    d.tv2 = go ? d.tv2 + inc2 * c.dT2 : d.tv2;
    d.t_exit = go ? te : d.t_exit;
    fetch_skip_word(sb, g, d);
    if (INSTR) { c_bricks += go ? 1 : 0; c_skipped += (go && skp) ? 1 : 0; }
    d.t = (go && skp) ? te : d.t;   // :784-785 `continue`
    d.state = inB ? (go ? (skp ? S_BRICK : S_SAMPLE) : S_DONE) : d.state;
}

// The inner loop was left by its condition (:790): the checks after it (:882-884).
template <bool ESS>
VR_DEV void after_segment(const RayCtx &c, RayDyn &d)
{
    if (d.state == S_SAMPLE && !(d.t < d.t_exit)) {
        if (!ESS) d.state = S_DONE;
        else if (d.t >= c.tfar || d.alpha >= 0.98f) d.state = S_DONE;                       // :882
        else if (d.c0 == c.exit0 || d.c1 == c.exit1 || d.c2 == c.exit2) d.state = S_DONE;  // :883
        else { d.t = d.t_exit; d.state = S_BRICK; }                                         // :884
    }
}

// LDS staging of the gathered sample evaluation (eval_batch): one slot per sample of a wave's
// round (64 lanes x kBatch samples), for each of the 4 waves of a workgroup
constexpr int kSlotFloats = 5;   // eval_batch: in: pos.xyz, opacity, owner|flags   out: ndl, spec, contour, op
                                 // eval_front / eval_dense / eval_back: in: pos.xyz, density, owner|flags   out: colour.rgb, op
constexpr int kStageFloatsPerWave = 64 * kBatch * kSlotFloats;
// Dynamic LDS of the marching kernels: [a stage per wave][the transfer function, tff_n float4][the skip bitmap, n_words
// + 1 words, if it is kept there].  The host sizes a launch with march_lds_bytes; the workgroup (WAVES waves) takes its
// pointers and fills the two tables together with VR_MARCH_LDS, which ends with the barrier.
#define VR_MARCH_STAGE_F4(WAVES) ((WAVES) * kStageFloatsPerWave / 4)   // float4 units, whole workgroup
inline size_t march_lds_bytes(int waves, uint32_t tff_n, uint32_t n_words, bool keep_skip)
{
    return ((size_t)VR_MARCH_STAGE_F4(waves) + tff_n) * sizeof(float4) + (keep_skip ? ((size_t)n_words + 1) * sizeof(uint32_t) : 0);
}
#define VR_MARCH_LDS(WAVES, KEEP_SKIP)                                                                          \
    extern __shared__ float4 s_mem[];                                                                           \
    float *s_stage = reinterpret_cast<float *>(s_mem) + (threadIdx.x >> 6) * kStageFloatsPerWave;               \
    float4 *s_tff = s_mem + VR_MARCH_STAGE_F4(WAVES);                                                           \
    uint32_t *s_skip = reinterpret_cast<uint32_t *>(s_tff + tf.tff_n);                                          \
    for (uint32_t i = threadIdx.x; i < tf.tff_n; i += (WAVES) * 64) s_tff[i] = tf.tff[i];                       \
    if (KEEP_SKIP)                                                                                              \
        for (uint32_t i = threadIdx.x; i <= skip.n_words; i += (WAVES) * 64) s_skip[i] = skip.bits[i];          \
    __syncthreads()

// Up to kBatch consecutive samples of one ray (inner loop, :790-864): for each, the colour
// already multiplied by the sample's opacity and the opacity.  Neither depends on the running
// alpha, so the batch is independent straight-line code (the loads of all its fetches are in
// flight together) and only the cheap front-to-back compositing is sequential.  Samples past
// ERT / t_exit are speculative: fetched from clamped (always valid) addresses, never composited.
//
// The kernel is bound by VALU issue, and the expensive part of a sample -- opacity correction
// (powr), and for samples above the shading threshold the gradient (32 voxel loads), the
// Blinn-Phong terms and a second powr -- only matters for samples whose opacity is not 0:
// often a few per cent of them, scattered over lanes and batch slots.  Under per-slot divergent
// branches that code would run up to kBatch times per round for a handful of lanes each.
// Instead the wave GATHERS its non-zero samples into LDS slots, evaluates the expensive scalars
// over the dense slot list (usually one pass over the active lanes; per-ray constants come from
// the owner lane by ds_bpermute) and hands four scalars per sample back.  Every sample sees the
// same fp32 operations as before, in another lane.
// FP: the kernel variant that reads the footprint volume (VolView::fp) instead of the plain
// layout -- default kernels only (no instrumentation, no XS extras); see launch_typed.
template <typename VT, int INSTR, bool XS, bool FP, typename V>
VR_DEV void eval_batch(const V &vol, const float4 *s_tff, int tffn, float *s_stage,
                       const RayCtx &c, const vrhip_rendering_params &rp,
                       const vrhip_raycast_params &rcp, float refInterval,
                       const float (&tk)[kBatch], const bool (&vk)[kBatch], float (&p0)[kBatch],
                       float (&p1)[kBatch], float (&p2)[kBatch], float (&op)[kBatch],
                       bool (&shaded)[kBatch])
{
    VR_MARK("E_pos");
    f3 pk[kBatch];
    float dens[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        f3 pos = add3(c.cam, scale3(c.dir, tk[k] - c.offset));
        pk[k] = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
        dens[k] = 0.f;
    }
    VR_MARK("E_fetch");
    if (XS && rp.illumType == 4) {
        // handled below
    } else if (!XS || rp.useLinear) {   // (nearest filtering, contours and the depth cue: XS variants, see launch_typed)
#pragma unroll
        for (int k = 0; k < kBatch; ++k)
            if (INSTR != 2 || vk[k]) dens[k] = vol.linear(pk[k].x, pk[k].y, pk[k].z);
    } else {
#pragma unroll
        for (int k = 0; k < kBatch; ++k)
            if (INSTR != 2 || vk[k]) dens[k] = vol.nearest(pk[k].x, pk[k].y, pk[k].z);
    }
    if (XS && rp.illumType == 4) {
        // gradient magnitude through the transfer function (:796-799): no density fetch
#pragma unroll 1
        for (int k = 0; k < kBatch; ++k)
            dens[k] = (INSTR != 2 || vk[k]) ? vol.gradient_len(pk[k].x, pk[k].y, pk[k].z) : 0.f;
    }
    VR_MARK("E_tf");
    float4 tfc[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) tfc[k] = tff_linear<kRawDensity<VT>>(s_tff, tffn, dens[k]);

    // CL_RGBA / CL_RG volumes (:838-855): the voxel is the colour (RGBA) or (r, g) -> colour
    // (r, 0, 0) with opacity TF(|g|); neither is shaded.  dens[] holds channel 0 already.
    const bool multi = XS && vol.channels > 1 && rp.illumType != 4;
    if (multi) {
#pragma unroll 1
        for (int k = 0; k < kBatch; ++k) {
            if (INSTR == 2 && !vk[k]) continue;
            float ch[3] = {0.f, 0.f, 0.f};
            for (int j = 1; j < vol.channels; ++j) {
                const auto vc = vol.channel(j);
                ch[j - 1] = rp.useLinear ? vc.linear(pk[k].x, pk[k].y, pk[k].z)
                                         : vc.nearest(pk[k].x, pk[k].y, pk[k].z);
            }
            if (vol.channels == 4) tfc[k] = make_float4(dens[k], ch[0], ch[1], ch[2]);
            else tfc[k] = make_float4(dens[k], 0.f, 0.f, tff_linear<kRawDensity<VT>>(s_tff, tffn, fabsf(ch[0] / 1.f)).w);
        }
    }

    VR_MARK("E_slots");
    // ---- which samples need the expensive part, and their slots
    const bool shade_mode = XS ? (rp.illumType != 0 && rp.illumType != 4) : rp.illumType == 1;   // :809
    const bool want_grad = shade_mode || (XS && rcp.contours && !rp.illumType);
    const uint32_t lane = threadIdx.x & 63u;
    bool lit[kBatch], need[kBatch];
    uint32_t slot[kBatch];
    uint32_t n_slots = 0;
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        lit[k] = vk[k] && tfc[k].w > 0.1f && !(XS && rp.illumType == 4) && !multi;   // :809/:832, before the depth cue
        shaded[k] = lit[k] && shade_mode;
        if (XS && rcp.aerial) {                               // :858-862
            float depthCue = 1.f - (tk[k] - c.tnear) / c.sampleDist;
            tfc[k].w *= depthCue;
        }
        // opacity 0 gives op = 1 - powr(1, y) = 0 exactly: nothing of the sample survives
        need[k] = vk[k] && tfc[k].w != 0.f;
        const unsigned long long m = __ballot(need[k]);
        slot[k] = n_slots + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        n_slots += (uint32_t)__builtin_popcountll(m);
    }
    float ndl[kBatch], spc[kBatch], cnt[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) { ndl[k] = 0.f; spc[k] = 0.f; cnt[k] = 0.f; op[k] = 0.f; }

    VR_MARK("E_stage");
    if (n_slots) {   // wave-uniform
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (need[k]) {
                float *q = s_stage + kSlotFloats * slot[k];
                q[0] = pk[k].x; q[1] = pk[k].y; q[2] = pk[k].z;
                q[3] = tfc[k].w;
                q[4] = __uint_as_float(lane | ((lit[k] && want_grad) ? 64u : 0u));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // only the lanes inside this (divergent) call can work: slots go to them by rank
        const unsigned long long act = __ballot(true);
        const uint32_t n_act = (uint32_t)__builtin_popcountll(act);
        const uint32_t arank = __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
    VR_MARK("E_dense");
        for (uint32_t base = 0; base < n_slots; base += n_act) {
            const uint32_t sidx = base + arank;
            const bool mine = sidx < n_slots;
            float *q = s_stage + kSlotFloats * (mine ? sidx : 0u);
            const float qx = q[0], qy = q[1], qz = q[2], qw = q[3];
            const uint32_t tag = mine ? __float_as_uint(q[4]) : lane;
            const int owner = (int)(tag & 63u);
            const bool shade = mine && (tag & 64u);
            // the owner's per-ray constants (every lane takes part in the exchange)
            const f3 lgt = mk3(__shfl(c.lgt.x, owner, 64), __shfl(c.lgt.y, owner, 64),
                               __shfl(c.lgt.z, owner, 64));
            const f3 hv = mk3(__shfl(c.hv.x, owner, 64), __shfl(c.hv.y, owner, 64),
                              __shfl(c.hv.z, owner, 64));
            const int hvalid = __shfl(c.hvalid ? 1 : 0, owner, 64);
            f3 dirv = mk3(0.f, 0.f, 0.f);
            if (XS && rcp.contours)
                dirv = mk3(__shfl(c.dir.x, owner, 64), __shfl(c.dir.y, owner, 64),
                           __shfl(c.dir.z, owner, 64));
            float o_ndl = 0.f, o_sp = 0.f, o_cnt = 0.f, o_op = 0.f;
            if (__ballot(shade)) {
                if (shade) {
                    f3 g;
                    if (XS && rp.illumType == 2) {    // :816-818 central differences of TF opacities
                        const float4 gq = gradient_tff<VT, INSTR>(vol, s_tff, tffn, mk3(qx, qy, qz));
                        g = mk3(-gq.x, -gq.y, -gq.z);
                    } else if (XS && rp.illumType == 3) {   // :819-821 Sobel
                        g = vol.neg_sobel(qx, qy, qz);
                    } else {                          // 1, 5, and contours without illumination
                        g = vol.neg_gradient(qx, qy, qz);
                    }
                    // illumination (:294-303) with specularBlinnPhong (:280-291); cel shading
                    // (:306-319) only needs the diffuse term
                    o_ndl = vmax(0.f, dot3(g, lgt));
                    if (!(XS && rp.illumType == 5)) {
                        o_sp = hvalid ? vr_powr(vmax(dot3(g, hv), 0.f), 40.f) : 0.0f;
                        o_sp = o_sp * 0.15f;
                    }
                    o_cnt = fabsf(dot3(dirv, g));             // contours (:846-848)
                }
            }
            if (mine) {
                o_op = 1.f - vr_powr(1.f - qw, refInterval);  // opacity correction (:864)
                q[0] = o_ndl; q[1] = o_sp; q[2] = o_cnt; q[3] = o_op;
            }
        }
    VR_MARK("E_readback");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (need[k]) {
                const float *q = s_stage + kSlotFloats * slot[k];
                ndl[k] = q[0]; spc[k] = q[1]; cnt[k] = q[2]; op[k] = q[3];
            }
        }
    }

    VR_MARK("E_combine");
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        if (lit[k] && shade_mode && !(XS && rp.illumType == 5)) {
            tfc[k].x = ((tfc[k].x * 0.15f) + ((tfc[k].x * ndl[k]) * 0.7f)) + spc[k];
            tfc[k].y = ((tfc[k].y * 0.15f) + ((tfc[k].y * ndl[k]) * 0.7f)) + spc[k];
            tfc[k].z = ((tfc[k].z * 0.15f) + ((tfc[k].z * ndl[k]) * 0.7f)) + spc[k];
        }
        if (XS && lit[k] && rp.illumType == 5) {   // celShading (:306-319), intensity = ndl
            const float f = ndl[k] > 0.95f ? 1.0f : ndl[k] > 0.5f ? 0.6f : ndl[k] > 0.25f ? 0.4f : 0.2f;
            if (!(ndl[k] > 0.95f)) { tfc[k].x *= f; tfc[k].y *= f; tfc[k].z *= f; }
        }
        if (XS && lit[k] && rcp.contours) {
            tfc[k].x *= cnt[k]; tfc[k].y *= cnt[k]; tfc[k].z *= cnt[k];
        }
        tfc[k].x = c.env0 - tfc[k].x;
        tfc[k].y = c.env1 - tfc[k].y;
        tfc[k].z = c.env2 - tfc[k].z;
        p0[k] = tfc[k].x * op[k];
        p1[k] = tfc[k].y * op[k];
        p2[k] = tfc[k].z * op[k];
    }
}

// ---- eval_batch for the default kernels (no instrumentation, no XS extras), cut in three so that the dense
// pass over the gathered samples is run by ALL 64 lanes of the wave, not only by the lanes whose rays
// evaluate a batch this round.  A batch runs with ~30 of 64 lanes and gathers ~38 samples with a non-zero
// opacity on the headline: inside the divergent call that was two passes of the gradient / shading code
// more often than not; the wave's idle and empty-run-skipping lanes take the second half now.  The same
// operations per sample, in another lane (as before).
//
// The COLOUR of a sample is the dense pass's work too.  Only the TF's alpha decides `lit` and `need`; a sample
// without `need` composites to nothing whatever its colour is (op == 0: colour * op is a zero whose sign alone is the
// colour's doing, and r - (+-0) * oma is r for every r but -0, which the accumulator -- the environment colour less
// such products -- holds only where the background itself is -0), and two thirds of the headline's evaluated
// samples are such.  So eval_front reads the two table entries' alpha only (tff_linear_alpha: the index, entries and
// lerp of tff_linear's .w) and stages the DENSITY in the slot; eval_dense runs tff_linear on it -- the same fp32
// operations on the same operands, so the same alpha, now with the colour --, applies the shading terms to the
// colour right where it has computed them, and hands back colour and opacity: a slot stays 5 floats.  The colour
// that is no longer computed was finite (0 * colour cannot have been a NaN): the table holds bytes / 255 (TfView),
// and tff_coord's clamp keeps a FLOAT volume's inf and NaN voxels on its edge entries -- in both lookups.
struct EvalFront {
    bool lit[kBatch], need[kBatch];
    uint32_t slot[kBatch];
};

// divergent part 1: density, the transfer function's alpha, slots of the samples with an opacity, staged to LDS.
// Returns the number of slots (the same in every lane that calls).
template <typename VT, bool FP, typename V>
VR_DEV uint32_t eval_front(const V &vol, const float4 *s_tff, int tffn, float *s_stage, const RayCtx &c,
                           const vrhip_rendering_params &rp, const float (&tk)[kBatch], const bool (&vk)[kBatch],
                           bool ev, EvalFront &ef)
{
    // Called by the whole wave: a VALU instruction costs the same with 30 lanes as with 64, and straight
    // code spares the exec-mask bookkeeping of a divergent region around the batch.  Lanes whose ray does
    // not evaluate this round (ev false: every vk false) only skip the voxel loads.
    f3 pk[kBatch];
    float dens[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        f3 pos = add3(c.cam, scale3(c.dir, tk[k] - c.offset));
        pk[k] = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
        dens[k] = 0.f;
    }
    if (ev) {
#pragma unroll
        for (int k = 0; k < kBatch; ++k) dens[k] = vol.linear(pk[k].x, pk[k].y, pk[k].z);
    }
    float al[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) al[k] = tff_linear_alpha<kRawDensity<VT>>(s_tff, tffn, dens[k]);
    const bool shade_mode = rp.illumType == 1;   // :809
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_slots = 0;
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        ef.lit[k] = vk[k] && al[k] > 0.1f;   // :809/:832
        // opacity 0 gives op = 1 - powr(1, y) = 0 exactly: nothing of the sample survives
        ef.need[k] = vk[k] && al[k] != 0.f;
        const unsigned long long m = __ballot(ef.need[k]);
        ef.slot[k] = n_slots + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        n_slots += (uint32_t)__builtin_popcountll(m);
    }
    if (n_slots) {
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (ef.need[k]) {
                float *q = s_stage + kSlotFloats * ef.slot[k];
                q[0] = pk[k].x; q[1] = pk[k].y; q[2] = pk[k].z;
                q[3] = dens[k];
                q[4] = __uint_as_float(lane | ((ef.lit[k] && shade_mode) ? 64u : 0u));
            }
        }
    }
    return n_slots;
}

// wave-uniform part: every lane of the wave takes slots (n_slots > 0, the same in all 64 lanes)
template <typename VT, bool FP, typename V>
VR_DEV void eval_dense(const V &vol, const float4 *s_tff, int tffn, float *s_stage, const RayCtx &c, float refInterval,
                       uint32_t n_slots)
{
    const uint32_t lane = threadIdx.x & 63u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < n_slots; base += 64u) {
        const uint32_t sidx = base + lane;
        const bool mine = sidx < n_slots;
        float *q = s_stage + kSlotFloats * (mine ? sidx : 0u);
        const float qx = q[0], qy = q[1], qz = q[2];
        const float qd = mine ? q[3] : 0.f;   // (slot 0 holds a result from the second pass on: not a density)
        const uint32_t tag = mine ? __float_as_uint(q[4]) : lane;
        const int owner = (int)(tag & 63u);
        const bool shade = mine && (tag & 64u);
        // the owner's per-ray constants (every lane takes part in the exchange)
        const f3 lgt = mk3(__shfl(c.lgt.x, owner, 64), __shfl(c.lgt.y, owner, 64), __shfl(c.lgt.z, owner, 64));
        const f3 hv = mk3(__shfl(c.hv.x, owner, 64), __shfl(c.hv.y, owner, 64), __shfl(c.hv.z, owner, 64));
        const int hvalid = __shfl(c.hvalid ? 1 : 0, owner, 64);
        // colour and alpha of the sample: eval_front's lookup again, all four channels (its alpha bit for bit)
        float4 t = tff_linear<kRawDensity<VT>>(s_tff, tffn, qd);
        if (__ballot(shade)) {
            if (shade) {
                const f3 g = vol.neg_gradient(qx, qy, qz);
                // illumination (:294-303) with specularBlinnPhong (:280-291)
                const float o_ndl = vmax(0.f, dot3(g, lgt));
                float o_sp = hvalid ? vr_powr(vmax(dot3(g, hv), 0.f), 40.f) : 0.0f;
                o_sp = o_sp * 0.15f;
                t.x = ((t.x * 0.15f) + ((t.x * o_ndl) * 0.7f)) + o_sp;
                t.y = ((t.y * 0.15f) + ((t.y * o_ndl) * 0.7f)) + o_sp;
                t.z = ((t.z * 0.15f) + ((t.z * o_ndl) * 0.7f)) + o_sp;
            }
        }
        if (mine) {
            const float o_op = 1.f - vr_powr(1.f - t.w, refInterval);  // opacity correction (:864)
            q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = o_op;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// divergent part 2: the samples' (shaded) colour and opacity back from their slots, colour x opacity.  A sample without
// a slot has opacity 0 and any colour: 0.
VR_DEV void eval_back(const float *s_stage, const RayCtx &c, const EvalFront &ef, uint32_t n_slots,
                      float (&p0)[kBatch], float (&p1)[kBatch], float (&p2)[kBatch], float (&op)[kBatch])
{
    float t0[kBatch], t1[kBatch], t2[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) { t0[k] = 0.f; t1[k] = 0.f; t2[k] = 0.f; op[k] = 0.f; }
    if (n_slots) {
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (ef.need[k]) {
                const float *q = s_stage + kSlotFloats * ef.slot[k];
                t0[k] = q[0]; t1[k] = q[1]; t2[k] = q[2]; op[k] = q[3];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        p0[k] = (c.env0 - t0[k]) * op[k];
        p1[k] = (c.env1 - t1[k]) * op[k];
        p2[k] = (c.env2 - t2[k]) * op[k];
    }
}

#ifndef VR_LOOK1
#define VR_LOOK1 24
#endif
#ifndef VR_LOOK_NUM
#define VR_LOOK_NUM 2   // the lookahead runs when at least 1 / VR_LOOK_NUM of the sampling lanes expect an empty sample
#endif
#ifndef VR_LOOK2
#define VR_LOOK2 8
#endif
// samples looked ahead for empty runs per lane and round (<= 32): phase 1 (one lane per ray) and
// phase 2 (four lanes per ray, each with its own window)
constexpr int kLook1 = VR_LOOK1, kLook2 = VR_LOOK2;

// Bit k set: sample k of the run t0, t0 + stepSize, ... lies in an EMPTY cell (CellView): its
// fetch can only map to opacity 0, so compositing it changes nothing (:864-879 with alpha == 0).
// The cell of a sample comes from the ray's cell line (vr_sampling.h, "the cell of a point on a line": why the cell of
// floor(u') answers for the fetch's voxels, the signed clamp, positions outside the volume).  Three instructions per
// axis and sample, no voxel access.
template <typename VT, int INSTR, int kLook, typename V>
VR_DEV uint32_t empty_mask(const CellView &cv, const V &vol, const RayCtx &c, float t0)
{
    const CellLine line = cell_line_ray(add3(c.cam, scale3(c.dir, t0 - c.offset)), c.dir, c.stepSize, vol, cv.eshift,
                                        cv.ecx, cv.ecy, cv.ecz);
    uint32_t w[kLook], sh[kLook];
#pragma unroll
    for (int k = 0; k < kLook; ++k) {
        const uint32_t idx = cell_index_of(cell_at(line, (float)k), cv.ecx, cv.ecy);
        w[k] = cv.empty[idx >> 5];
        sh[k] = idx & 31u;
    }
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < kLook; ++k) m |= ((w[k] >> sh[k]) & 1u) << k;
    return m;
}

// Step over the leading empty samples of the run (the reference's own t sequence and loop
// exits, :790 and :868-879; nothing else of the loop body has an effect for them).  Returns
// true when all kLook1 samples were consumed and the run may continue.
//
// Branch-free (round 4): sample k of the run is stepped over when the samples before it were, its cell is empty
// (k < n1, the number of leading ones of the mask) and the inner loop's condition and the check after the sample
// let the ray go on -- t < t_exit (:790) and not t >= tfar (:868) -- i.e. t < lim = min(t_exit, tfar).  Once one of
// the two fails it fails for every later k (t stays), so the run needs no flag: one integer and one float compare,
// the add and a select per sample, where the nested ifs compiled to ~8 VALU and ~10 SALU instructions and a branch
// each.  The sample at which the run stops is looked at once, afterwards: still in an empty cell and t < t_exit, so
// t >= tfar -- the reference takes that sample (it composites nothing) and leaves the loop at :868.
template <int kLook>
VR_DEV uint32_t skip_empty_steps(uint32_t n1, const RayCtx &c, RayDyn &d, bool count, unsigned long long &c_taken)
{
    const float lim = vmin(d.t_exit, c.tfar);
    float tk = d.t;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kLook; ++k) {
        const bool adv = (uint32_t)k < n1 && tk < lim;
        n += adv ? 1u : 0u;
        tk = adv ? tk + c.stepSize : tk;
    }
    d.t = tk;
    const bool far_hit = n < (uint32_t)kLook && n < n1 && tk < d.t_exit;   // (t >= tfar: the sample is taken, then :868)
    if (count) c_taken += n + (far_hit ? 1u : 0u);
#ifdef VR_RAYLEN
    d.nsmp += n + (far_hit ? 1u : 0u);
#endif
    if (far_hit) d.state = S_DONE;
    return n;
}

// number of leading ones among the low kLook bits of a mask
template <int kLook>
VR_DEV uint32_t leading_ones(uint32_t mask)
{
    if (kLook < 32) return (uint32_t)__builtin_ctz(~mask | (1u << (kLook & 31)));
    return mask == 0xffffffffu ? 32u : (uint32_t)__builtin_ctz(~mask);
}

VR_DEV bool skip_empty_run(uint32_t mask, const RayCtx &c, RayDyn &d, bool count,
                           unsigned long long &c_taken)
{
    // leading samples in empty cells; a lane that is not sampling steps over nothing
    const uint32_t n1 = d.state == S_SAMPLE ? leading_ones<kLook1>(mask) : 0u;
    return skip_empty_steps<kLook1>(n1, c, d, count, c_taken) == (uint32_t)kLook1;
}

// Phase 2: the four lanes of a ray look at four consecutive windows of kLook2 samples; the run is
// then stepped over in chunks of kLook2 for as long as some ray of the wave is still skipping.
VR_DEV bool skip_empty_run_wide(const uint32_t (&masks)[4], const RayCtx &c, RayDyn &d, bool count,
                                unsigned long long &c_taken)
{
    bool run = d.state == S_SAMPLE;
#pragma unroll
    for (int chunk = 0; chunk < 4; ++chunk) {
        if (!__ballot(run)) break;
        const uint32_t n1 = run ? leading_ones<kLook2>(masks[chunk]) : 0u;
        run = skip_empty_steps<kLook2>(n1, c, d, count, c_taken) == (uint32_t)kLook2;
    }
    return run;
}

// Is the empty-run lookahead on for this launch?  It needs the empty bits and the linear sampler's footprint; the
// traffic-instrumented variant (INSTR 2) reproduces the reference's fetch set instead, and the XS modes that look at
// every sample stay out: illumType 4, and showEss, which tracks the last sample.  SHOW_ESS: false in the split kernel,
// which has no such term -- showEss renders in a single phase.  The three marching kernels and the host's launch info ask here.
#define VR_LOOKAHEAD_ON(INSTR, XS, SHOW_ESS, EMPTY, RP) \
    (INSTR != 2 && EMPTY != nullptr && RP.useLinear != 0 && !(XS && (RP.illumType == 4 || (SHOW_ESS && RP.showEss))))

// The lookahead costs a few hundred instructions for the whole wave: it runs when at least half
// of the sampling lanes expect their next sample to be empty (their last one was).
VR_DEV bool lookahead_pays(bool sampling, bool guess_empty)
{
    const int n_s = __builtin_popcountll(__ballot(sampling));
    const int n_g = __builtin_popcountll(__ballot(sampling && guess_empty));
    return n_g > 0 && VR_LOOK_NUM * n_g >= n_s;
}

// One front-to-back compositing step (:865-879) with the sample's colour*opacity (q0..q2),
// opacity qo and ray parameter ti.
VR_DEV void composite(const RayCtx &c, RayDyn &d, float q0, float q1, float q2, float qo, float ti)
{
    VR_RAYLEN_INC(d);
    float oma = 1.f - d.alpha;
    d.r0 = d.r0 - q0 * oma;
    d.r1 = d.r1 - q1 * oma;
    d.r2 = d.r2 - q2 * oma;
    d.alpha = d.alpha + qo * oma;
    // (double)alpha > 0.98 <=> alpha >= 0.98f (ERT_THRESHOLD, :28); `break`, then :882 breaks
    if (ti >= c.tfar || d.alpha >= 0.98f) {
        d.state = S_DONE;
        d.ert = !(ti >= c.tfar);   // :868 breaks before the ERT branch (:869-877) is looked at
        d.t_ert = ti;
    } else {
        d.t = ti + c.stepSize;
    }
}

// The batch ladder, where every kernel gets the reference's t sequence from: ray parameters (t += stepSize, :879) and
// validity -- the inner loop's condition (:790) and the break after a sample at or past tfar (:868) -- of the ray's next
// kBatch samples, one lane per ray.  FIRST_VALID: the loop condition for the first one (and what gates the lane);
// NO_SPECULATION: the traffic-instrumented variant must not touch speculative voxels.
#define VR_BATCH_PARAMS(FIRST_VALID, NO_SPECULATION)                            \
    tk[0] = d.t;                                                                \
    vk[0] = FIRST_VALID;                                                        \
    _Pragma("unroll")                                                           \
    for (int k = 1; k < kBatch; ++k) {                                          \
        tk[k] = tk[k - 1] + c.stepSize;                                         \
        vk[k] = vk[k - 1] && !(tk[k - 1] >= c.tfar) && (tk[k] < d.t_exit);      \
        if (NO_SPECULATION) vk[k] = false;                                      \
    }
// ... of the ray's next kSplit * kBatch samples, four lanes per ray (phase 2): lane `slot` of the quad keeps numbers
// kBatch * slot .. kBatch * slot + kBatch - 1
#define VR_BATCH_PARAMS_SPLIT(FIRST_VALID)                                              \
    float tk[kBatch] = {0.f, 0.f, 0.f, 0.f};                                            \
    bool vk[kBatch] = {false, false, false, false};                                     \
    float tc = d.t;                                                                     \
    bool v = FIRST_VALID;                                                               \
    _Pragma("unroll")                                                                   \
    for (int i = 0; i < kSplit * kBatch; ++i) {                                         \
        if ((int)slot == i / kBatch) { tk[i % kBatch] = tc; vk[i % kBatch] = v; }       \
        const float tn = tc + c.stepSize;                                               \
        v = v && !(tc >= c.tfar) && (tn < d.t_exit);                                    \
        tc = tn;                                                                        \
    }

// broadcast lane L of every quad (4 consecutive lanes): one DPP move, no LDS
template <int L> VR_DEV float quad_bcast(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), L * 0x55, 0xf, 0xf, true));
}
template <int L> VR_DEV int quad_bcast(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, L * 0x55, 0xf, 0xf, true);
}

// ------------------------------------------------------------------ ambient occlusion

// hybrid Tausworthe / LCG generator on the per-pixel uint4 state (:50-80); the constant is a
// double literal: product in double, rounded to float on return
VR_DEV uint32_t taus_step(uint32_t &z, int s1, int s2, int s3, uint32_t m)
{
    const uint32_t b = (((z << (uint32_t)s1) ^ z) >> (uint32_t)s2);
    z = (((z & m) << (uint32_t)s3) ^ b);
    return z;
}
VR_DEV float hybrid_rand(uint32_t (&st)[4])
{
    const uint32_t a = taus_step(st[0], 13, 19, 12, 4294967294u);
    const uint32_t b = taus_step(st[1], 2, 25, 4, 4294967288u);
    const uint32_t c = taus_step(st[2], 3, 11, 17, 4294967280u);
    const uint32_t d = st[3];
    st[3] = 1664525u * st[3] + 1013904223u;
    return (float)(2.3283064365387e-10 * (double)(float)(a ^ b ^ c ^ d));
}

// calcAO (:368-392) at the sample that triggered early ray termination, with
// getUniformRandomSampleDirectionUpper (:353-364); scales the ray's colour by 1 - ao / 2 (:875).
// Rare mode, rolled loops.
template <typename VT, int INSTR, typename V>
VR_DEV void apply_ao(const V &vol, const float4 *s_tff, int tffn, const RayCtx &c,
                     RayDyn &d, const vrhip_rendering_params &rp, uint32_t gx, uint32_t gy)
{
    const f3 p0 = add3(c.cam, scale3(c.dir, d.t_ert - c.offset));
    const f3 pos = mk3(p0.x * 0.5f + 0.5f, p0.y * 0.5f + 0.5f, p0.z * 0.5f + 0.5f);
    const f3 n = vol.neg_gradient(pos.x, pos.y, pos.z);
    const float vl = len3(mk3(1.f / vol.fw, 1.f / vol.fh, 1.f / vol.fd));
    const float stepSize = vl * 0.9f, r = vl * 5.f;
    uint32_t st[4];
    st[0] = st[1] = st[2] = st[3] = parallel_rng3(gx, gy, rp.seed);   // :611
    float ao = 0.f;
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
        const float z = (hybrid_rand(st) * 2.f) - 1.f;
        const float phi = (hybrid_rand(st) * 2.f) * 3.14159274101257f;
        float sn, cs;
        vr_sincosf(phi, &sn, &cs);
        const float rad = sqrtf(1.f - z * z);
        f3 dir = mk3(rad * sn, rad * cs, z);
        if (dot3(n, dir) < 0) dir = mk3(dir.x * -1.f, dir.y * -1.f, dir.z * -1.f);
        float sample = 0.f;
        int cnt = 0;
#pragma unroll 1
        while ((float)cnt * stepSize < r) {
            ++cnt;
            const f3 p = add3(pos, scale3(scale3(dir, (float)cnt), stepSize));
            sample += tff_linear_alpha<kRawDensity<VT>>(s_tff, tffn, vol.linear(p.x, p.y, p.z));
            if (sample > 0.98f) break;
        }
        sample /= (float)cnt;
        ao += sample;
    }
    ao = ao / 16.f;
    const float f = 1.f - 0.5f * ao;
    d.r0 *= f; d.r1 *= f; d.r2 *= f;
}

// ---- image-order ESS (volumeraycast.cl:659-670, :912-925) and showEss (:888-896)

// what the work-items of an 8x8 work-group (= patch) did, for vr_hit_resolve_kernel
enum { HIT_SKIPPED = 0, HIT_FIRST_ENDS = 1, HIT_FIRST_MISSES = 2 };

// volumeraycast.cl:323-343 with bound = (0, 1)
VR_DEV bool check_bounding_box(f3 pos, f3 voxLen)
{
    const bool xl = pos.x < voxLen.x, xh = pos.x > 1.f - voxLen.x;
    const bool yl = pos.y < voxLen.y, yh = pos.y > 1.f - voxLen.y;
    const bool zl = pos.z < 0.f + voxLen.z, zh = pos.z > 1.f - voxLen.z;
    return (xl && zl) || (xl && yl) || (yl && zl) || (xh && zl) || (yh && zl) || (xh && zh) ||
           (yh && zh) || (xl && zh) || (yl && zh) || (xh && yl) || (xh && yh) || (xl && yh);
}

// getLastHit (:513-526): true when nothing was hit in or around this work-group last frame.
// Lanes 0..8 read one texel each; texels outside the hit image count as 0.
VR_DEV bool group_unhit(const FrameView &fr, uint32_t tx8, uint32_t ty8, uint32_t lane)
{
    uint32_t v = 0;
    if (lane < 9u) {
        const int x = (int)tx8 + (int)(lane % 3u) - 1, y = (int)ty8 + (int)(lane / 3u) - 1;
        if (x >= 0 && y >= 0 && x < (int)fr.hit_w && y < (int)fr.hit_h)
            v = fr.hit_in[(size_t)y * fr.hit_w + (size_t)x];
    }
    return __ballot(v != 0u) == 0ull;
}

// Runs once per patch, after its rays are set up.  Records what the group's first work-item
// will do (it has the last word on the hit texel, :918-924) and, for a group that is skipped,
// writes the background (:664-668).  Returns true for a skipped group.
VR_DEV bool image_ess_patch(const FrameView &fr, const vrhip_rendering_params &rp, const RayCtx &c,
                            const WaveTile &wt, uint32_t lane, bool inside, uint32_t gx, uint32_t gy,
                            size_t out_index)
{
    const bool unhit = group_unhit(fr, wt_col(wt), wt_row(wt), lane);
    const unsigned long long valid = __ballot(c.valid);
    if (lane == 0)
        fr.hit_status[(size_t)wt_row(wt) * fr.hit_w + wt_col(wt)] =
            (uint8_t)(unhit ? HIT_SKIPPED : ((valid & 1ull) ? HIT_FIRST_ENDS : HIT_FIRST_MISSES));
    if (unhit && inside) {
        float4 o = make_float4(c.env0, c.env1, c.env2, c.env3);
        if (rp.showEss) o = make_float4(1.f - o.x, 1.f - o.y, 1.f - o.z, 1.f - o.w);
        fr.fb[(size_t)gy * fr.W + gx] = o;
        if (fr.out) fr.out[out_index] = o;
    }
    return unhit;
}

// showEss (:888-896), running mean over iterations (:898-909, fp32 accumulate buffer), the two
// writes, and the image-order ESS hit flag (:912-917).  EXTRAS = false: the default kernels,
// which are never launched with showEss / imgEss set.
template <bool EXTRAS>
VR_DEV void write_pixel(const FrameView &fr, const vrhip_rendering_params &rp, const RayCtx &c,
                        const RayDyn &d, f3 voxLen, uint32_t gx, uint32_t gy, size_t out_index)
{
    const size_t fi = (size_t)gy * fr.W + gx;
    float r0 = d.r0, r1 = d.r1, r2 = d.r2, alpha = d.alpha;
    if (EXTRAS && rp.showEss && c.valid) {
        f3 pk = mk3(0.f, 0.f, 0.f);   // :722: the position of a ray that never sampled
        if (d.t_last >= 0.f) {
            const f3 pos = add3(c.cam, scale3(c.dir, d.t_last - c.offset));
            pk = mk3(pos.x * 0.5f + 0.5f, pos.y * 0.5f + 0.5f, pos.z * 0.5f + 0.5f);
        }
        if (check_bounding_box(pk, voxLen)) {
            r0 = fabsf(1.f - rp.backgroundColor[0]);
            r1 = fabsf(1.f - rp.backgroundColor[1]);
            r2 = fabsf(1.f - rp.backgroundColor[2]);
            alpha = 1.f;
        }
    }
    if (rp.iteration != 0 && c.valid) {
        float4 prev = fr.fb[fi];
        float it1 = (float)(rp.iteration + 1u);
        r0 = prev.x + (r0 - prev.x) / it1;
        r1 = prev.y + (r1 - prev.y) / it1;
        r2 = prev.z + (r2 - prev.z) / it1;
    }
    float4 o = make_float4(r0, r1, r2, c.valid ? alpha : c.env3);
#ifdef VR_RAYLEN
    o.w = c.valid ? (float)d.nsmp : 0.f;
#endif
    fr.fb[fi] = o;
    if (fr.out) fr.out[out_index] = o;
    if (EXTRAS && rp.imgEss && c.valid && (r0 != c.env0 || r1 != c.env1 || r2 != c.env2))
        fr.hit_any[(size_t)(gy >> 3) * fr.hit_w + (gx >> 3)] = 1;
}

VR_DEV Grid make_grid(const BrickView &bricks, const vrhip_raycast_params &rcp, uint32_t oob_word,
                      bool ess)
{
    Grid g;
    g.bw = bricks.bw; g.bh = bricks.bh; g.bd = bricks.bd;
    g.bl0 = g.bl1 = g.bl2 = 0.f;
    g.brickDia = 0.f;
    g.oob_word = oob_word;
    if (ess) {
        g.bl0 = 1.f / rcp.brickRes[0];
        g.bl1 = 1.f / rcp.brickRes[1];
        g.bl2 = 1.f / rcp.brickRes[2];
        g.brickDia = sqrtf(((g.bl0 * g.bl0) + (g.bl1 * g.bl1)) + (g.bl2 * g.bl2)) * 2.f;
    }
    return g;
}

// make_grid(bricks, rc, n_words, true), computed once on the host with the same IEEE operations: for the kernels that
// take the grid as an argument (the pre-pass, the patch classes)
inline Grid make_grid_host(const RaycastLaunch &a)
{
    Grid hg;
    hg.bw = a.bricks.bw; hg.bh = a.bricks.bh; hg.bd = a.bricks.bd;
    hg.oob_word = a.skip.n_words;
    hg.bl0 = 1.f / a.raycast.brickRes[0];
    hg.bl1 = 1.f / a.raycast.brickRes[1];
    hg.bl2 = 1.f / a.raycast.brickRes[2];
    hg.brickDia = sqrtf(((hg.bl0 * hg.bl0) + (hg.bl1 * hg.bl1)) + (hg.bl2 * hg.bl2)) * 2.f;
    return hg;
}

// What a marching kernel derives once per launch from its arguments, the same in every ray.  (The pre-pass gets grid and
// voxLen from the host: see there.)  sb: the skip bitmap where this kernel reads it, LDS or global.
#define VR_MARCH_CONSTS(INSTR, ESS, TOUCHED)                                        \
    const Vol<VT, INSTR, FP> vol = make_vol<VT, INSTR, FP>(vv, TOUCHED);            \
    const f3 resf = mk3(vol.fw, vol.fh, vol.fd);                                    \
    const f3 voxLen = mk3(1.f / vol.fw, 1.f / vol.fh, 1.f / vol.fd);                \
    const float refInterval = 1.f / rc.samplingRate;                                \
    const Grid grid = make_grid(bricks, rc, skip.n_words, ESS);                     \
    const uint32_t *sb = SKIP_LDS ? s_skip : skip.bits

VR_DEV void flush_counters(DevStats *stats, uint32_t lane, const unsigned long long (&c)[6])
{
    for (int i = 0; i < 6; ++i) {
        unsigned long long s = wave_sum(c[i]);
        if (lane == 0 && s) atomicAdd(&stats->v[i], s);
    }
}

// ------------------------------------------------------------------ patch culling

// maximum over the 64 lanes (all of them active), in every lane: six DPP steps -- row_shr 1, 2, 4, 8 leave
// each row's maximum in its lane 15, row_bcast15 / row_bcast31 carry it on to lane 63 -- and a readlane
template <int CTRL, int ROW_MASK>
VR_DEV float dpp_max_step(float v)
{
    // lanes without a source (and rows outside ROW_MASK) keep their own value: `old` = v
    const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
    return vmax(v, o);
}
VR_DEV float wave_max_f(float v)
{
    v = dpp_max_step<0x111, 0xf>(v);   // row_shr:1
    v = dpp_max_step<0x112, 0xf>(v);   // row_shr:2
    v = dpp_max_step<0x114, 0xf>(v);   // row_shr:4
    v = dpp_max_step<0x118, 0xf>(v);   // row_shr:8
    v = dpp_max_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_max_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// True when NO ray of the wave's 8x8 patch can visit a brick that is not skipped (SkipView::near_bits).
// Every point of every valid ray i, cam_i + t dir_i with t in [tn, tf] (the patch's smallest tnear and
// largest tfar), lies within rho = max|cam_i - cam_r| + tf max|dir_i - dir_r| of the point with the
// same t on a reference ray r of the patch; 256 test points on r (four per lane) leave no point of r
// farther than h / 2 from one of them.  The reference DDA of a ray only visits bricks that touch the
// ray within one brick (its crossing times are accumulated sums, off by far less than a brick), so
// all it can visit lies within floor((rho + h / 2) / brick) + 2 bricks of a test point's (clamped) brick
// (+1 because the test points' bricks are found with a reciprocal, good to a brick).
// If that is within the radius the bitmap was dilated by and every test point reads 0, every brick
// any of the rays visits is skipped: the rays end as they started.  Out-of-range cells read the
// (0, 0) decision, which must be "skip" for any of this to hold.
VR_DEV bool patch_is_clear(const SkipView &skip, const Grid &g, const RayCtx &c, uint32_t lane)
{
    const unsigned long long vm = __ballot(c.valid);
    if (!vm) return false;                       // (nothing to walk anyway: the normal path writes the pixels)
    if (skip.bits[skip.n_words] != 0xffffffffu) return false;
    const int ref = ((vm >> 27) & 1ull) ? 27 : (int)__builtin_ctzll(vm);   // a ray in the middle of the patch, if it has one
    const f3 rc = mk3(__shfl(c.cam.x, ref, 64), __shfl(c.cam.y, ref, 64), __shfl(c.cam.z, ref, 64));
    const f3 rd = mk3(__shfl(c.dir.x, ref, 64), __shfl(c.dir.y, ref, 64), __shfl(c.dir.z, ref, 64));
    const float dc = wave_max_f(c.valid ? len3(sub3(c.cam, rc)) : 0.f);
    const float dd = wave_max_f(c.valid ? len3(sub3(c.dir, rd)) : 0.f);
    const float tf = wave_max_f(c.valid ? c.tfar : -3.0e38f);
    const float tn = -wave_max_f(c.valid ? -c.tnear : -3.0e38f);
    if (!(tf > tn) || !(tf < 1.0e30f)) return false;
    const float h = (tf - tn) * (1.0f / 256.0f);
    const float need = (dc + tf * dd + 0.5f * h) * 1.0001f;
    const float bl[3] = {g.bl0, g.bl1, g.bl2};
    const int bres[3] = {g.bw, g.bh, g.bd};
    // a point within `need` of a test point lies at most floor(need / brick) + 1 bricks from the test
    // point's brick; one more for bricks the DDA visits next to the ray
    float ibs[3];   // bricks per world unit
    for (int i = 0; i < 3; ++i) {
        ibs[i] = 0.5f / bl[i];
        // (+3: one brick more than the derivation needs, for the reciprocal in the test points' bricks)
        if (!(floorf(need / (2.f * bl[i])) + 3.f <= (float)skip.near_r)) return false;
    }
    bool live = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = tn + ((float)(lane + 64u * (uint32_t)k) + 0.5f) * h;
        const float p[3] = {rc.x + t * rd.x, rc.y + t * rd.y, rc.z + t * rd.z};
        int cell[3];   // (good to a brick: the radius test above has a brick to spare for it)
        for (int i = 0; i < 3; ++i) cell[i] = iclamp((int)floorf((p[i] + 1.f) * ibs[i]), 0, bres[i] - 1);
        const uint32_t idx = ((uint32_t)cell[2] * (uint32_t)g.bh + (uint32_t)cell[1]) * (uint32_t)g.bw + (uint32_t)cell[0];
        live = live || ((skip.near_bits[idx >> 5] >> (idx & 31u)) & 1u);
    }
    return __ballot(live) == 0ull;
}

// ------------------------------------------------------------------ DDA pre-pass

// Most rays of a typical frame cross the volume without ever meeting a brick the ESS bitmap
// does not skip: all they do is the DDA walk.  In the marching kernels (two waves per SIMD) that
// walk is a latency chain; here it runs alone in a kernel small enough for high occupancy (the
// bitmap is read through the caches).  One wave per 8x8 patch, same set-up and dda_step as the
// march, hence the same decisions.  Rays that end without a sample write their pixel here;
// patches with rays that reach a brick to sample go to the `live` list for phase 1.
template <typename VT, bool VIEWS = false>
__global__ __launch_bounds__(kBlockDim) void vr_dda_prepass_kernel(
    VolView vv, BrickView bricks, SkipView skip, FrameView fr, vrhip_camera_params cam,
    vrhip_rendering_params rp, vrhip_raycast_params rc, Grid grid, f3 voxLen)
{
    // (grid, voxLen: make_grid's and 1 / resolution's values, computed once on the host with the same
    // IEEE operations -- a wave lives for one patch here, and the divisions and the square root were
    // 90 of its ~1250 instructions)
    VR_ZERO_NEXT_CTRL(fr);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (kBlockDim / 64) + (threadIdx.x >> 6);
    if (q >= fr.n_wave_tiles) return;
    const WaveTile wt = fr.queue[q];
    const uint32_t lx = lane & 7u, ly = lane >> 3;
    const uint32_t gx = wt_col(wt) * 8u + lx, gy = wt_row(wt) * 8u + ly;
    const size_t out_index = (size_t)wt.out_base + (size_t)ly * fr.out_stride + lx;
    if (fr.patch_class && fr.patch_class[q / fr.set_frames]) {
        // class 1 (vr_patch_class_kernel): every ray of this patch -- in any frame of the set -- hits the box,
        // meets no brick to sample, and the background is one colour: what the walk would leave, without a ray
        const float4 o = make_float4(rp.backgroundColor[0], rp.backgroundColor[1], rp.backgroundColor[2], 0.f);
        fr.fb[(size_t)gy * fr.W + gx] = o;
        if (fr.out) fr.out[out_index] = o;
        VR_PM_NOTE(fr, q, 0ull, 0u);
        return;
    }
    const uint32_t seed = fr.seeds ? fr.seeds[wt_frame(wt)] : rp.seed;
    const bool inside = gx < fr.W && gy < fr.H;
    const f3 resf = mk3(vv.fw, vv.fh, vv.fd);
    RayCtx c;
    RayDyn d;
    float rnd;
    if constexpr (VIEWS) {
        const vrhip_camera_params fc = load_frame_cam<true>(fr.cams, wt_frame(wt));
        setup_ray_head<false>(gx, gy, inside, fr, fc, rp, c, d, seed, rnd);
    } else {
        setup_ray_head<false>(gx, gy, inside, fr, cam, rp, c, d, seed, rnd);   // (nothing is shaded here)
    }
    if (rp.imgEss && image_ess_patch(fr, rp, c, wt, lane, inside, gx, gy, out_index)) {
        VR_PM_NOTE(fr, q, 0ull, 0u);
        return;
    }
    if (skip.near_bits && patch_is_clear(skip, grid, c, lane)) {
        // no ray of this patch can meet a brick that is not skipped: what the walk would leave
        // (step size and DDA set-up are not needed for that)
        if (inside) write_pixel<true>(fr, rp, c, d, voxLen, gx, gy, out_index);
        VR_PM_NOTE(fr, q, 0ull, 0u);
        return;
    }
    setup_ray_tail<true>(rc, resf, voxLen, grid, c, d, rnd);
    fetch_skip_word(skip.bits, grid, d);
    unsigned long long n0 = 0, n1 = 0;
#ifdef VR_MARCH_STATS
    unsigned long long w_steps = 0, l_steps = 0;
    while (__ballot(d.state == S_BRICK)) {
        w_steps++;
        l_steps += __builtin_popcountll(__ballot(d.state == S_BRICK));
        dda_step<0>(skip.bits, grid, c, d, n0, n1);
    }
    if (lane == 0) {
        atomicAdd(&g_march_stats[28], 1ull);                                     // patches that walk
        atomicAdd(&g_march_stats[29], w_steps);                                  // DDA step executions
        atomicAdd(&g_march_stats[30], l_steps);                                  // lanes in them
        atomicAdd(&g_march_stats[31], (unsigned long long)__builtin_popcountll(__ballot(c.valid)));   // valid rays
    }
#else
    while (__ballot(d.state == S_BRICK)) dda_step<0>(skip.bits, grid, c, d, n0, n1);
#endif
    const bool live = d.state == S_SAMPLE;
    const unsigned long long m = __ballot(live);
    if (inside && !live) {
        // what the march would leave for a ray without samples: background colour, alpha 0
        write_pixel<true>(fr, rp, c, d, voxLen, gx, gy, out_index);
    }
    if (fr.live_rays) {
        // ray list for phase 1 (vr_raycast_rays_kernel): the live rays with the DDA state they have
        // reached, so that phase 1 neither repeats the walk nor carries the patch's dead lanes
        if (m) {
            // (list q % kLiveLists: vr_internal.h)
            const uint32_t list = q % kLiveLists;
            VR_WAVE_APPEND(base, fr.live_list_count + list * kLiveStride, m);
            base += list * live_list_cap(fr.n_wave_tiles);
            VR_PM_NOTE(fr, q, m, base);
            if (live) {
                VR_PACK_RAY(r, (uint32_t)out_index, wt_frame(wt), 0);
                fr.live_rays[base + VR_LANE_RANK(m)] = r;
            }
        } else {
            VR_PM_NOTE(fr, q, 0ull, 0u);
        }
        return;
    }
    if (m && lane == 0) {
        const uint32_t slot = atomicAdd(fr.live_count, 1u);
        LiveTile lt;
        lt.wt = wt;
        lt.mask_lo = (uint32_t)m;
        lt.mask_hi = (uint32_t)(m >> 32);
        fr.live[slot] = lt;
    }
}

// ------------------------------------------------------------------ phase 1 on the ray list

// Phase 1 for the default modes with ESS: one lane per ray, the rays taken from the pre-pass's ray
// list (FrameView::live_rays) with the DDA state reached there; a lane whose ray ends -- or is
// suspended for phase 2 after `round_budget` rounds of its own -- takes the next ray once
// 4 * refill_min lanes of the wave are idle (default 64: the whole wave, measured best).  Same per-ray operation sequence as the patch kernel above; no dead
// lanes carried through a patch, no second DDA walk.  Exit condition reached by every wave: the
// list head only grows, and every ray ends or is suspended.
// WAVES: waves per workgroup.  4 (256 threads): the compiler's register choice (184 VGPRs), two workgroups per CU by
// their 72 KiB of LDS = two waves per SIMD.  12 (768 threads): launch bounds that leave 170 VGPRs (168 used, three to
// six spilled), ONE workgroup per CU = three waves per SIMD that share one transfer function and one skip bitmap in
// LDS (60 + 16 + 32 KiB): pays where waves wait more than they issue -- launch sets of several frames, volumes whose
// ESS bricks are too small for the empty-run lookahead -- and not one frame at a time with the lookahead, where a
// third wave only stretches the chain of the longest rays.  See launch_variant.
constexpr int kWavesWide = 12;

template <typename VT, bool SKIP_LDS, bool FP, int WAVES = 4, bool VIEWS = false>
__global__ __launch_bounds__(WAVES * 64) void vr_raycast_rays_kernel(
    VolView vv, BrickView bricks, TfView tf, SkipView skip, CellView cells, FrameView fr,
    vrhip_camera_params cam, vrhip_rendering_params rp, vrhip_raycast_params rc)
{
    // The pre-pass (previous kernel on the stream) has written kLiveLists lists; they are read interleaved, 64 rays from
    // each in turn: virtual ray v is ray (v / 64 / kLiveLists) * 64 + v % 64 of list (v / 64) % kLiveLists, and there are
    // kLiveLists * 64 * ceil(longest list / 64) virtual rays (those beyond a list's end do not exist: idle lanes).
    // Pixel-major order (fr.pm, never with VIEWS): the same walk over the kLiveLists INDEX lists that vr_regroup_kernel
    // has written behind the pre-pass -- their counters sit kPmBase - kLiveBase control words behind the ray lists' --,
    // and a refill reads the index entry, then the record it names.
    const bool pm_order = !VIEWS && fr.pm != nullptr;
    const uint32_t *const list_count = fr.live_list_count + (pm_order ? kPmBase - kLiveBase : 0u);
    __shared__ uint32_t s_live_n[kLiveLists];
    uint32_t longest = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLiveLists; ++k) {
        const uint32_t n_k = list_count[k * kLiveStride];
        longest = n_k > longest ? n_k : longest;
        if (threadIdx.x == k) s_live_n[k] = n_k;
    }
    const uint32_t n_rays = ((longest + 63u) >> 6) * kLiveLists * 64u;
    if (n_rays == 0) return;
    const uint32_t list_cap = live_list_cap(fr.n_wave_tiles);
    VR_MARCH_LDS(WAVES, SKIP_LDS);

    const uint32_t lane = threadIdx.x & 63u;
    const int tffn = (int)tf.tff_n;
    VR_MARCH_CONSTS(0, true, nullptr);
    const bool skip_empty = VR_LOOKAHEAD_ON(0, false, true, cells.empty, rp);   // (this kernel has no INSTR or XS variants)
    const uint32_t budget = fr.round_budget ? fr.round_budget : 0xffffffffu;
    const uint32_t kRefillLanes = (fr.refill_min ? fr.refill_min : 16u) * 4u;   // idle lanes before a refill

    unsigned long long n0 = 0, n1 = 0;
    bool have = false, drained = false, first_draw = true;
    uint32_t gx = 0, gy = 0, out_index = 0, my_rounds = 0, frame_idx = 0;
    bool guess_empty = true;
    uint32_t cool = 0;   // evaluation batches before the ray guesses "empty" again (see the lookahead below)
#ifdef VR_MARCH_STATS
    unsigned long long ms_acc[16] = {0};
#endif
    RayCtx c;
    RayDyn d;
    setup_ray<true>(0u, 0u, false, fr, cam, rp, rc, resf, voxLen, grid, c, d, rp.seed);   // S_DONE

    for (;;) {
        VR_MARK("R_top");
        {
            const bool idle = d.state == S_DONE;
            const unsigned long long idle_m = __ballot(idle);
            const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle_m);
            const bool all_idle = idle_m == ~0ull;
            if ((!drained && n_idle >= kRefillLanes) || all_idle) {
                VR_MS(8, 1);                                                   // refills
                if (idle && have) {   // retire a finished ray (suspended ones have given up `have`)
                    write_pixel<false>(fr, rp, c, d, voxLen, gx, gy, (size_t)out_index);
                    have = false;
                }
                if (!drained) {
                    // a wave's FIRST 64 rays are its own by position -- no ticket: 2 048 - 3 072 waves drawing from one
                    // counter at the same instant is a queue at one L2 address before anything marches --, the
                    // later ones are drawn behind those
                    uint32_t base = 0;
                    if (first_draw) {
                        base = (blockIdx.x * (uint32_t)WAVES + (threadIdx.x >> 6)) * 64u;
                    } else {
                        if (lane == 0) base = atomicAdd(fr.queue_head, n_idle);
                        base = __builtin_amdgcn_readfirstlane(base) + gridDim.x * (uint32_t)WAVES * 64u;
                    }
                    first_draw = false;
                    if (base + n_idle >= n_rays) drained = true;
                    if (idle) {
                        const uint32_t v = base + (uint32_t)__builtin_popcountll(idle_m & ((1ull << lane) - 1ull));
                        const uint32_t chunk = v >> 6, list = chunk % kLiveLists;
                        const uint32_t pos = ((chunk / kLiveLists) << 6) | (v & 63u);
                        have = v < n_rays && pos < s_live_n[list];
                        uint32_t at = list * list_cap + pos;
                        if (pm_order) {   // (entries that pad a patch's group name no ray)
                            at = have ? fr.pm[3u * fr.n_wave_tiles + list * pm_list_cap(fr.n_wave_tiles, fr.set_frames) + pos] : kPmNone;
                            have = at != kPmNone;
                        }
                        if (have) {
                            const ContRec rec = fr.live_rays[at];
                            // (per lane: the lanes of a wave may hold rays of different frames)
                            VR_UNPACK_RAY(rec, frame_idx,
                                if constexpr (VIEWS) {
                                    const vrhip_camera_params fc = load_frame_cam<false>(fr.cams, frame_idx);
                                    setup_ray<true>(gx, gy, true, fr, fc, rp, rc, resf, voxLen, grid, c, d, fr.seeds ? fr.seeds[frame_idx] : rp.seed);
                                } else {
                                    setup_ray<true>(gx, gy, true, fr, cam, rp, rc, resf, voxLen, grid, c, d, fr.seeds ? fr.seeds[frame_idx] : rp.seed);
                                });
                            fetch_skip_word(sb, grid, d);
                            my_rounds = 0;
                            guess_empty = true;
                            cool = 0;
                        }
                    }
                }
                if (!__ballot(d.state != S_DONE)) {
                    if (drained) break;
                    continue;
                }
            }
        }
        VR_MARK("R_dda");
        // ---- one round (the patch kernel's)
        VR_MS(0, 1);                                                           // rounds
        VR_MS(1, __builtin_popcountll(__ballot(d.state != S_DONE)));           // live lanes, summed over rounds
        for (int it = 0;; ++it) {
            if (!__ballot(d.state == S_BRICK)) break;
            if (it >= kMaxBrickSteps && __ballot(d.state == S_SAMPLE)) break;
            VR_MS(2, 1);                                                       // DDA step executions
            VR_MS(3, __builtin_popcountll(__ballot(d.state == S_BRICK)));      // lanes in them
            dda_step<0>(sb, grid, c, d, n0, n1);
        }
        if (!__ballot(d.state != S_DONE)) continue;
        VR_MARK("R_susp");
        // a ray that has used its rounds goes to the continuation buffer (phase 2)
        {
            const bool susp = d.state != S_DONE && my_rounds >= budget;
            const unsigned long long cm = __ballot(susp);
            if (cm) {
                VR_WAVE_APPEND(base, fr.cont_count, cm);
                if (susp) {
                    VR_PACK_RAY(r, out_index, frame_idx, VR_SORT_KEY);
                    fr.cont[base + VR_LANE_RANK(cm)] = r;
                    d.state = S_DONE;
                    have = false;
                }
                if (!__ballot(d.state != S_DONE)) continue;
            }
        }
        VR_MARK("R_look");
        if (__ballot(d.state == S_SAMPLE)) my_rounds += d.state == S_SAMPLE ? 1u : 0u;
        bool more_empty = false;
        if (skip_empty && lookahead_pays(d.state == S_SAMPLE, guess_empty)) {
            VR_MS(4, 1);                                                       // lookahead executions
            VR_MS(5, __builtin_popcountll(__ballot(d.state == S_SAMPLE)));     // lanes in them
            if (d.state == S_SAMPLE) {
                const uint32_t em = empty_mask<VT, 0, kLook1>(cells, vol, c, d.t);
                more_empty = skip_empty_run(em, c, d, false, n0);
                guess_empty = (em & 1u) != 0u;
                // a transparent sample in a cell that is NOT empty (the rim of a structure) says little
                // about the samples behind it: no new guess for the next `cool` batches.  How long: as
                // many batches as the mask shows non-empty samples ahead
                if (!(em & 1u)) cool = (uint32_t)(__builtin_ctz(em | 0x10000u) / kBatch);
                after_segment<true>(c, d);
            }
        }
        VR_MARK("R_batch");
        if (__ballot(d.state == S_SAMPLE && !more_empty)) {
            VR_MS(6, 1);                                                       // evaluation batches
            VR_MS(7, __builtin_popcountll(__ballot(d.state == S_SAMPLE && !more_empty)));   // lanes in them
        }
        // the evaluation batch as wave-uniform code in three parts (eval_front / eval_dense / eval_back): every
        // lane of the wave works in the dense pass, whether its own ray evaluates this round or not
        const bool ev = d.state == S_SAMPLE && !more_empty;
        if (__ballot(ev)) {
            float tk[kBatch];
            bool vk[kBatch];
            VR_BATCH_PARAMS(ev && d.t < d.t_exit, false);
#ifdef VR_MARCH_STATS
            for (int k = 0; k < kBatch; ++k) ms_acc[9] += vk[k] ? 1 : 0;      // valid samples evaluated (per lane: summed below)
#endif
            EvalFront ef;
            const uint32_t ns = eval_front<VT, FP>(vol, s_tff, tffn, s_stage, c, rp, tk, vk, ev, ef);
            if (ns) eval_dense<VT, FP>(vol, s_tff, tffn, s_stage, c, refInterval, ns);
            VR_MARK("R_comp");
            float p0[kBatch], p1[kBatch], p2[kBatch], opk[kBatch];
            eval_back(s_stage, c, ef, ns, p0, p1, p2, opk);
#pragma unroll
            for (int k = 0; k < kBatch; ++k)
                if (vk[k] && d.state == S_SAMPLE) composite(c, d, p0[k], p1[k], p2[k], opk[k], tk[k]);
            if (ev) {
                if (vk[kBatch - 1]) guess_empty = opk[kBatch - 1] == 0.f && cool == 0u;
                if (cool) --cool;
                after_segment<true>(c, d);
            }
        }
    }
#ifdef VR_MARCH_STATS
    if (lane == 0)
        for (int i = 0; i < 9; ++i) atomicAdd(&g_march_stats[16 + i], ms_acc[i]);
    {
        unsigned long long w = wave_sum(ms_acc[9]);
        if (lane == 0) atomicAdd(&g_march_stats[16 + 9], w);
    }
#endif
}

// ------------------------------------------------------------------ phase 1

template <typename VT, bool ESS, int INSTR, bool SKIP_LDS, bool XS, bool FP, bool VIEWS = false>
__global__ __launch_bounds__(kBlockDim) VR_OCC void vr_raycast_kernel(
    VolView vv, BrickView bricks, TfView tf, SkipView skip, CellView cells, FrameView fr,
    vrhip_camera_params cam, vrhip_rendering_params rp, vrhip_raycast_params rc, DevStats *stats,
    uint32_t *touched)
{
    VR_ZERO_NEXT_CTRL(fr);   // (also when the pre-pass has done it: the block stays unused until the next set)
    VR_STAMP_DECL;
    VR_MARCH_LDS(kBlockDim / 64, ESS && SKIP_LDS);
    VR_STAMP(8);

    const uint32_t lane = threadIdx.x & 63u;
    const int tffn = (int)tf.tff_n;
    unsigned long long c_taken = 0, c_nominal = 0, c_shaded = 0, c_bricks = 0, c_skipped = 0,
                       c_hit = 0;
    VR_MARCH_CONSTS(INSTR, ESS, touched);
    const bool skip_empty = VR_LOOKAHEAD_ON(INSTR, XS, true, cells.empty, rp);

    // every wave pulls 8x8 patches until the queue is drained (exit condition reached by every
    // wave: the head only grows).  The next ticket is drawn while the current patch is marched,
    // which hides the contended atomic; every wave draws exactly one ticket past the end.
    const bool use_live = ESS && INSTR == 0 && fr.live != nullptr;
    const uint32_t n_tiles = use_live ? *fr.live_count : fr.n_wave_tiles;
    uint32_t q_next = 0;
    if (lane == 0) q_next = atomicAdd(fr.queue_head, 1u);
    for (;;) {
        const uint32_t q = __builtin_amdgcn_readfirstlane(q_next);
        if (q >= n_tiles) break;
        WaveTile wt;
        unsigned long long live_mask = ~0ull;
        if (use_live) {
            const LiveTile lt = fr.live[q];
            wt = lt.wt;
            live_mask = (unsigned long long)lt.mask_lo | ((unsigned long long)lt.mask_hi << 32);
        } else {
            wt = fr.queue[q];
        }
        if (lane == 0) q_next = atomicAdd(fr.queue_head, 1u);
        VR_STAMP(0);
        VR_COUNT(11);
        const uint32_t lx = lane & 7u, ly = lane >> 3;
        const uint32_t gx = wt_col(wt) * 8u + lx, gy = wt_row(wt) * 8u + ly;
        const uint32_t frame_idx = wt_frame(wt);
        const uint32_t seed = fr.seeds ? fr.seeds[frame_idx] : rp.seed;
        const bool inside = gx < fr.W && gy < fr.H;

        RayCtx c;
        RayDyn d;
        if constexpr (VIEWS) {
            const vrhip_camera_params fc = load_frame_cam<true>(fr.cams, frame_idx);
            setup_ray<ESS>(gx, gy, inside, fr, fc, rp, rc, resf, voxLen, grid, c, d, seed);
        } else {
            setup_ray<ESS>(gx, gy, inside, fr, cam, rp, rc, resf, voxLen, grid, c, d, seed);
        }
        if (XS && rp.imgEss && !use_live &&   // (with a live list the pre-pass has done this)
            image_ess_patch(fr, rp, c, wt, lane, inside, gx, gy,
                            (size_t)wt.out_base + (size_t)ly * fr.out_stride + lx))
            continue;
        // rays the pre-pass has finished (their pixel is written) stay out of the march
        const bool prepass_done = !((live_mask >> lane) & 1ull);
        if (prepass_done) d.state = S_DONE;
        if (ESS) fetch_skip_word(sb, grid, d);
        if (INSTR && c.valid) { c_hit++; c_nominal += (unsigned long long)c.nominal; }
        VR_STAMP(1);

        // ---- flattened DDA / sample state machine, at most round_budget sample rounds
        uint32_t rounds_left = fr.round_budget ? fr.round_budget : 0xffffffffu;
        bool suspended = false;
        bool guess_empty = true;   // this ray's next sample is expected to lie in an empty cell
        for (;;) {
            VR_COUNT(10);
            if (ESS) {
                for (int it = 0;; ++it) {
                    if (!__ballot(d.state == S_BRICK)) break;
                    if (it >= kMaxBrickSteps && __ballot(d.state == S_SAMPLE)) break;
                    VR_COUNT(9);
                    dda_step<INSTR>(sb, grid, c, d, c_bricks, c_skipped);
                }
            }
            VR_STAMP(2);
            if (!__ballot(d.state != S_DONE)) break;
            if (rounds_left == 0) { suspended = true; break; }
            if (__ballot(d.state == S_SAMPLE)) --rounds_left;
            bool more_empty = false;
            if (skip_empty && lookahead_pays(d.state == S_SAMPLE, guess_empty)) {
                if (d.state == S_SAMPLE) {
                    // ---- step over a run of up to kLook1 samples in empty cells
                    const uint32_t em = empty_mask<VT, INSTR, kLook1>(cells, vol, c, d.t);
                    more_empty = skip_empty_run(em, c, d, INSTR != 0, c_taken);
                    guess_empty = (em & 1u) != 0u;
                    after_segment<ESS>(c, d);
                }
            }
            VR_STAMP(4);
            if (d.state == S_SAMPLE && !more_empty) {
                // ---- up to kBatch consecutive samples of this ray per round
                float tk[kBatch];
                bool vk[kBatch], litk[kBatch];
                VR_BATCH_PARAMS(d.t < d.t_exit, INSTR == 2);
                float p0[kBatch], p1[kBatch], p2[kBatch], opk[kBatch];
                eval_batch<VT, INSTR, XS, FP>(vol, s_tff, tffn, s_stage, c, rp, rc, refInterval, tk, vk, p0, p1, p2,
                                      opk, litk);
                VR_STAMP(3);
                // sequential front-to-back compositing (:865-879)
#pragma unroll
                for (int k = 0; k < kBatch; ++k) {
                    if (vk[k] && d.state == S_SAMPLE) {
                        if (INSTR) { c_taken++; if (litk[k]) c_shaded++; }
                        if (XS) d.t_last = tk[k];
                        composite(c, d, p0[k], p1[k], p2[k], opk[k], tk[k]);
                    }
                }
                if (vk[kBatch - 1]) guess_empty = opk[kBatch - 1] == 0.f;
                after_segment<ESS>(c, d);
                VR_STAMP(6);
            }
        }

        // rays that outlived the budget go to the continuation buffer (phase 2)
        const bool cont = suspended && d.state != S_DONE;
        const unsigned long long cm = __ballot(cont);
        if (cm) {
            VR_WAVE_APPEND(base, fr.cont_count, cm);
            if (cont) {
                VR_PACK_RAY(r, wt.out_base + ly * fr.out_stride + lx, frame_idx, VR_SORT_KEY);
                const uint32_t rank = VR_LANE_RANK(cm);
                fr.cont[base + rank] = r;
            }
        }
        if (XS && rc.useAO && inside && !cont && !prepass_done && d.ert)
            apply_ao<VT, INSTR>(vol, s_tff, tffn, c, d, rp, gx, gy);
        if (inside && !cont && !prepass_done)
            write_pixel<XS>(fr, rp, c, d, voxLen, gx, gy,
                            (size_t)wt.out_base + (size_t)ly * fr.out_stride + lx);
        VR_STAMP(7);
    }
    VR_STAMP_FLUSH_AT(0);

    if (INSTR) {
        const unsigned long long cc[6] = {c_taken, c_nominal, c_shaded, c_bricks, c_skipped, c_hit};
        flush_counters(stats, lane, cc);
    }
}

// ------------------------------------------------------------------ phase 2

// composite the kBatch samples evaluated by lane O of every quad, in order
template <int O>
VR_DEV void composite_from(const RayCtx &c, RayDyn &d, const float (&p0)[kBatch],
                           const float (&p1)[kBatch], const float (&p2)[kBatch],
                           const float (&op)[kBatch], const float (&tk)[kBatch],
                           const int (&fl)[kBatch], bool count, unsigned long long &c_taken,
                           unsigned long long &c_shaded)
{
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        const float q0 = quad_bcast<O>(p0[k]), q1 = quad_bcast<O>(p1[k]), q2 = quad_bcast<O>(p2[k]);
        const float qo = quad_bcast<O>(op[k]), ti = quad_bcast<O>(tk[k]);
        const int f = quad_bcast<O>(fl[k]);
        if ((f & 1) && d.state == S_SAMPLE) {
            if (count) { c_taken++; if (f & 2) c_shaded++; }
            composite(c, d, q0, q1, q2, qo, ti);
        }
    }
}

// ... of the whole quad: the ray's kSplit * kBatch samples of this round in ray order; F_LAST, O_LAST: flag and opacity
// of the 16th of them (lane 3 of the quad, slot kBatch - 1), for the next round's guess
#define VR_COMPOSITE_QUAD(COUNT, F_LAST, O_LAST)                                    \
    composite_from<0>(c, d, p0, p1, p2, opk, tk, fl, COUNT, c_taken, c_shaded);     \
    composite_from<1>(c, d, p0, p1, p2, opk, tk, fl, COUNT, c_taken, c_shaded);     \
    composite_from<2>(c, d, p0, p1, p2, opk, tk, fl, COUNT, c_taken, c_shaded);     \
    composite_from<3>(c, d, p0, p1, p2, opk, tk, fl, COUNT, c_taken, c_shaded);     \
    const int F_LAST = quad_bcast<3>(fl[kBatch - 1]);                               \
    const float O_LAST = quad_bcast<3>(opk[kBatch - 1])

// Resumes suspended rays with kSplit = 4 lanes per ray (16 rays per wave).  The 4 lanes of a ray
// hold the same state and take the same decisions; lane `slot` evaluates samples
// 4*slot .. 4*slot+3 of the next 16 consecutive samples (same batch code as phase 1), then every
// lane replays the compositing of all 16 in ray order, fetching the other lanes' results with
// in-quad DPP broadcasts -- the fp32 operation sequence per ray is exactly phase 1's (and the
// reference's), the serial chain of a long ray is 4x shorter.
template <typename VT, bool ESS, int INSTR, bool SKIP_LDS, bool XS, bool FP, int WAVES = 4, bool VIEWS = false>
__global__ __launch_bounds__(WAVES * 64) void vr_raycast_split_kernel(
    VolView vv, BrickView bricks, TfView tf, SkipView skip, CellView cells, FrameView fr,
    vrhip_camera_params cam, vrhip_rendering_params rp, vrhip_raycast_params rc, DevStats *stats,
    uint32_t *touched)
{
    static_assert(kSplit == 4 && (kBatch == 4 || kBatch == 8), "phase 2 is written for 4 lanes x 4 (8: A/B build) samples");
    const uint32_t n_rays = *fr.cont_count;   // written by phase 1 (previous kernel on the stream)
    if (n_rays == 0) return;
    VR_STAMP_DECL;
    VR_MARCH_LDS(WAVES, ESS && SKIP_LDS);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = lane & (kSplit - 1);   // 16 rays per wave, 4 lanes each
    constexpr uint32_t kRaysPerWave = 64 / kSplit;
    const int tffn = (int)tf.tff_n;
    unsigned long long c_taken = 0, c_shaded = 0, c_bricks = 0, c_skipped = 0;
    VR_MARCH_CONSTS(INSTR, ESS, touched);
    const bool skip_empty = VR_LOOKAHEAD_ON(INSTR, XS, false, cells.empty, rp);
    // Rays are handed out one by one from the sorted list: when `refill_min` ray slots (quads) of
    // the wave are idle they retire their rays and take the next ones (their set-up runs
    // together).  With the default, 16, a wave refills when all its rays are done, but draws as
    // many rays as it has slots from wherever the list head is -- finer than fixed groups of 16,
    // and with the longest rays first the tail is made of the shortest ones.  Smaller values keep
    // the waves fuller at the price of more (divergent) set-ups: measured better by 2-3 % on the
    // "shells" volumes, worse by as much on dense ones.  Exit condition reached by every wave: the
    // list head only grows, and every ray ends.
    const uint32_t refill_min = fr.refill_min ? fr.refill_min : kRaysPerWave;
    unsigned long long dummy0 = 0, dummy1 = 0;
    const bool count = INSTR && slot == 0;
    bool have = false, drained = false, first_draw = true;
    uint32_t gx = 0, gy = 0, out_index = 0, my_rounds = 0;
    bool guess_empty = true;   // identical in the four lanes of a ray, like all of its state
    uint32_t cool = 0;         // evaluation batches before the ray guesses "empty" again
    RayCtx c;
    RayDyn d;
    setup_ray<ESS>(0u, 0u, false, fr, cam, rp, rc, resf, voxLen, grid, c, d, rp.seed);   // S_DONE

    for (;;) {
        {
            const bool idle = d.state == S_DONE;
            const unsigned long long idle_m = __ballot(idle);
            const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle_m) / kSplit;
            const bool all_idle = idle_m == ~0ull;
            if ((!drained && n_idle >= refill_min) || all_idle) {
                VR_COUNT(11);
                // retire the finished rays
                if (idle && have) {
                    if (XS && rc.useAO && slot == 0 && d.ert)
                        apply_ao<VT, INSTR>(vol, s_tff, tffn, c, d, rp, gx, gy);
                    if (slot == 0) {
                        write_pixel<XS>(fr, rp, c, d, voxLen, gx, gy, (size_t)out_index);
                        if (fr.cost)
                            fr.cost[(size_t)gy * fr.W + gx] = (uint16_t)(my_rounds < 65535u ? my_rounds : 65535u);
                    }
                    have = false;
                }
                if (!drained) {
                    // (a wave's first 16 rays are its own by position, the later ones are drawn behind those: see
                    // vr_raycast_rays_kernel)
                    uint32_t base = 0;
                    if (first_draw) {
                        base = (blockIdx.x * (uint32_t)WAVES + (threadIdx.x >> 6)) * kRaysPerWave;
                    } else {
                        if (lane == 0) base = atomicAdd(fr.cont_head, n_idle);
                        base = __builtin_amdgcn_readfirstlane(base) + gridDim.x * (uint32_t)WAVES * kRaysPerWave;
                    }
                    first_draw = false;
                    if (base + n_idle >= n_rays) drained = true;
                    if (idle) {
                        // my quad's rank among the idle quads (every lane of a quad is idle or none is)
                        const uint32_t below = (uint32_t)__builtin_popcountll(
                            idle_m & ((1ull << (lane & ~(uint64_t)(kSplit - 1))) - 1ull)) / kSplit;
                        const uint32_t ri = base + below;
                        have = ri < n_rays;
                        if (have) {
                            const uint32_t rix = fr.order ? fr.order[ri] : ri;
                            const ContRec rec = fr.cont[rix];
                            // (per lane: the quads of a wave may hold rays of different frames)
                            VR_UNPACK_RAY(rec, const uint32_t f,
                                if constexpr (VIEWS) {
                                    const vrhip_camera_params fc = load_frame_cam<false>(fr.cams, f);
                                    setup_ray<ESS>(gx, gy, true, fr, fc, rp, rc, resf, voxLen, grid, c, d, fr.seeds ? fr.seeds[f] : rp.seed);
                                } else {
                                    setup_ray<ESS>(gx, gy, true, fr, cam, rp, rc, resf, voxLen, grid, c, d, fr.seeds ? fr.seeds[f] : rp.seed);
                                });
                            if (ESS) fetch_skip_word(sb, grid, d);
                            my_rounds = 0;
                            guess_empty = true;
                            cool = 0;
                        }
                    }
                }
                VR_STAMP(1);
                if (!__ballot(d.state != S_DONE)) {
                    if (drained) break;
                    continue;
                }
            }
        }
        {   // ---- one round
            if (ESS) {
                for (int it = 0;; ++it) {
                    if (!__ballot(d.state == S_BRICK)) break;
                    if (it >= kMaxBrickSteps && __ballot(d.state == S_SAMPLE)) break;
                    VR_COUNT(9);
                    if (count) dda_step<INSTR>(sb, grid, c, d, c_bricks, c_skipped);
                    else dda_step<0>(sb, grid, c, d, dummy0, dummy1);
                }
            }
            VR_STAMP(2);
            if (!__ballot(d.state != S_DONE)) continue;
            VR_COUNT(10);
            my_rounds += d.state != S_DONE ? 1u : 0u;
            bool more_empty = false;
            if (skip_empty && lookahead_pays(d.state == S_SAMPLE, guess_empty)) {
                if (d.state == S_SAMPLE) {
                    // the four lanes of a ray hold the same state and take the same decisions;
                    // lane `slot` looks at samples [kLook2 * slot, kLook2 * (slot + 1)) of the run
                    // (its window start is approximate, which is all the cell lookup needs)
                    const float t_win = d.t + (float)(kLook2 * (int)slot) * c.stepSize;
                    const int em = (int)empty_mask<VT, INSTR, kLook2>(cells, vol, c, t_win);
                    const uint32_t m4[4] = {(uint32_t)quad_bcast<0>(em), (uint32_t)quad_bcast<1>(em),
                                            (uint32_t)quad_bcast<2>(em), (uint32_t)quad_bcast<3>(em)};
                    more_empty = skip_empty_run_wide(m4, c, d, count, c_taken);
                    guess_empty = (m4[0] & 1u) != 0u;
                    // (see phase 1: no new guess while the mask shows samples in cells that are not empty)
                    if (!(m4[0] & 1u)) {
                        const uint32_t all = m4[0] | (m4[1] << kLook2) | (m4[2] << (2 * kLook2)) | (m4[3] << (3 * kLook2));
                        cool = (uint32_t)((all ? __builtin_ctz(all) : 4 * kLook2) / (kSplit * kBatch));
                    }
                    after_segment<ESS>(c, d);
                }
            }
            VR_STAMP(4);
            const bool ev2 = d.state == S_SAMPLE && !more_empty;   // (the same in the four lanes of a ray)
            if (INSTR == 0 && !XS) {
                // default kernels: the batch as wave-uniform code (phase 1's eval_front / eval_dense /
                // eval_back): the dense pass over the gathered samples is run by all 64 lanes, also those
                // of rays that step over empty runs or have ended
                if (__ballot(ev2)) {
                    VR_BATCH_PARAMS_SPLIT(ev2 && d.t < d.t_exit);
                    EvalFront ef;
                    const uint32_t ns = eval_front<VT, FP>(vol, s_tff, tffn, s_stage, c, rp, tk, vk, ev2, ef);
                    if (ns) eval_dense<VT, FP>(vol, s_tff, tffn, s_stage, c, refInterval, ns);
                    float p0[kBatch], p1[kBatch], p2[kBatch], opk[kBatch];
                    eval_back(s_stage, c, ef, ns, p0, p1, p2, opk);
                    VR_STAMP(3);
                    int fl[kBatch];
#pragma unroll
                    for (int k = 0; k < kBatch; ++k) fl[k] = (vk[k] ? 1 : 0) | ((ef.lit[k] && rp.illumType == 1) ? 2 : 0);
                    {
                        VR_COMPOSITE_QUAD(false, f3v, o3);
                        if (ev2) {
                            if (f3v & 1) guess_empty = o3 == 0.f && cool == 0u;
                            if (cool) --cool;
                            after_segment<ESS>(c, d);
                        }
                    }
                    VR_STAMP(6);
                }
            } else
            if (d.state == S_SAMPLE && !more_empty) {
                VR_BATCH_PARAMS_SPLIT(d.t < d.t_exit);
                if (INSTR == 2) {   // no speculative voxel touches: one sample per round
#pragma unroll
                    for (int k = 0; k < kBatch; ++k) vk[k] = vk[k] && slot == 0 && k == 0;
                }
                float p0[kBatch], p1[kBatch], p2[kBatch], opk[kBatch];
                bool litk[kBatch];
                eval_batch<VT, INSTR, XS, FP>(vol, s_tff, tffn, s_stage, c, rp, rc, refInterval, tk, vk, p0, p1, p2,
                                      opk, litk);
                VR_STAMP(3);
                int fl[kBatch];
#pragma unroll
                for (int k = 0; k < kBatch; ++k) fl[k] = (vk[k] ? 1 : 0) | (litk[k] ? 2 : 0);
                {
                    VR_COMPOSITE_QUAD(count, f3v, o3);
                    if (f3v & 1) guess_empty = o3 == 0.f && cool == 0u;
                    if (cool) --cool;
                }
                after_segment<ESS>(c, d);
                VR_STAMP(6);
            }
        }
    }
    VR_STAMP_FLUSH_AT(16);

    if (INSTR) {
        const unsigned long long cc[6] = {c_taken, 0, c_shaded, c_bricks, c_skipped, 0};
        flush_counters(stats, lane, cc);
    }
}

template <typename K>
hipError_t prepare_variant(K kernel, size_t lds, int *nb_out, const char *what, int num_cus, int block_dim = kBlockDim)
{
    return vr_prepare_kernel(kernel, block_dim, lds, nb_out, what, num_cus);
}

// dynamic LDS of the marching kernels: a stage per wave, the transfer function, the skip bitmap if it is kept there
inline size_t march_lds(int waves, const RaycastLaunch &a, bool skip_lds) { return march_lds_bytes(waves, a.tf.tff_n, a.skip.n_words, skip_lds); }
// does a workgroup of kWavesWide waves with the skip bitmap fit a CU's LDS?
inline bool wide_fits_lds(const RaycastLaunch &a) { return march_lds(kWavesWide, a, true) <= (size_t)160 * 1024; }

// VIEWS: the kernels that take frame f's camera from FrameView::cams (a batch of per-frame views) instead of the
// launch's; the VIEWS = false instantiations are the ones every other launch runs, unchanged by the option.
template <typename VT, bool ESS, int INSTR, bool SKIP_LDS, bool XS, bool FP = false, bool VIEWS = false>
hipError_t launch_variant(const RaycastLaunch &a, hipStream_t stream)
{
    auto k1 = vr_raycast_kernel<VT, ESS, INSTR, SKIP_LDS, XS, FP, VIEWS>;
    auto k2 = vr_raycast_split_kernel<VT, ESS, INSTR, SKIP_LDS, XS, FP, 4, VIEWS>;
    // three waves per SIMD (RaycastLaunch::occ3 / occ3_split): the default kernels on the footprint volume as ONE
    // workgroup of kWavesWide waves per CU (launch_typed keeps SKIP_LDS for them when the bitmap fits beside 12 stages)
    constexpr bool kWide = ESS && INSTR == 0 && !XS && FP;
    const bool wide2 = kWide && a.occ3_split;
    if (wide2) k2 = vr_raycast_split_kernel<VT, ESS, INSTR, SKIP_LDS, XS, FP, kWide ? kWavesWide : 4, VIEWS>;
    const int waves2 = wide2 ? kWavesWide : 4;
    const size_t lds = march_lds(4, a, ESS && SKIP_LDS);
    const size_t lds2 = march_lds(waves2, a, ESS && SKIP_LDS);
    int nb1 = 0, nb2 = 0;
    {
        hipError_t e = prepare_variant(k1, lds, &nb1, "raycast phase 1", a.num_cus);
        if (e == hipSuccess) e = prepare_variant(k2, lds2, &nb2, "raycast phase 2", a.num_cus, waves2 * 64);
        if (e != hipSuccess) return e;
    }
    const uint32_t cus = (uint32_t)(a.num_cus > 0 ? a.num_cus : 256);
    uint32_t want = (a.frame.n_wave_tiles + 3u) / 4u;
    uint32_t cap = cus * (uint32_t)nb1;
    dim3 grid(want < cap ? want : cap), block(kBlockDim);
    if (grid.x == 0) return hipSuccess;
    FrameView frame = a.frame;
    if (XS || INSTR != 0 || !ESS) frame.live_rays = nullptr;   // the ray list serves the default kernels
    // ... and the pixel-major index is an index into that list, for the frames of one camera
    if (VIEWS || !frame.live || !frame.live_rays || frame.set_frames < 2u || frame.n_wave_tiles % frame.set_frames) frame.pm = nullptr;
    if (a.info) {   // what this call launches, for vrhip_last_launch_info (completed below)
        vrhip_launch_info &li = *a.info;
        li.technique = 0;
        li.work_items = a.frame.n_wave_tiles;
        li.round_budget = a.frame.round_budget;
        li.footprint = FP ? 1u : 0u;
        li.instrumented = (uint32_t)INSTR;
        li.extras = XS ? 1u : 0u;
        li.skip_in_lds = (ESS && SKIP_LDS) ? 1u : 0u;
        li.phase1_waves = 4;
        li.phase2_waves = a.frame.round_budget ? (uint32_t)waves2 : 0u;
        li.sorted_phase2 = (a.frame.round_budget && a.frame.order) ? 1u : 0u;
        li.empty_skip = VR_LOOKAHEAD_ON(INSTR, XS, true, a.cells.empty, a.render) ? 1u : 0u;
    }
    // the events of the frame's timing ride on the launches themselves (RaycastLaunch::stop_event, start_event)
    hipEvent_t start_ev = (a.bind_events && a.start_bound) ? a.start_event : nullptr;
    if (ESS && INSTR == 0 && frame.live) {
        const Grid hg = make_grid_host(a);
        f3 hv;
        hv.x = 1.f / a.vol.fw; hv.y = 1.f / a.vol.fh; hv.z = 1.f / a.vol.fd;
        vr_launch_kernel(vr_dda_prepass_kernel<VT, VIEWS>, dim3(want), block, 0, stream, start_ev, nullptr, a.vol, a.bricks,
                         a.skip, frame, a.cam, a.render, a.raycast, hg, hv);
        hipError_t pe = hipGetLastError();
        if (pe != hipSuccess) return pe;
        if (start_ev) { *a.start_bound = true; start_ev = nullptr; }
        if (a.info) { a.info->prepass = 1; a.info->patch_classes = frame.patch_class ? 1u : 0u; }
        if (VIEWS && frame.patch_class) return hipErrorInvalidValue;   // (classes hold for one camera: the host turns them off)
        if (frame.pm) {
            pe = vr_launch_regroup(frame, a.pm_group, stream);
            if (pe != hipSuccess) return pe;
            if (a.info) a.info->pixel_major = 1;
        }
    } else {
        frame.live = nullptr;
        frame.pm = nullptr;
    }
    hipError_t e;
    const bool resolve_follows = a.render.imgEss && a.hit_out && a.frame.n_wave_tiles;
    const bool bind_stop = a.bind_events && a.stop_event && a.stop_bound && !resolve_follows;
    const bool p1_last = a.frame.round_budget == 0;
    const hipEvent_t p1_ev = !a.bind_events ? nullptr : (p1_last && bind_stop) ? a.stop_event : a.mid_event;
    if (ESS && INSTR == 0 && !XS && frame.live && frame.live_rays) {   // phase 1 on the ray list
        // phase 1 picks its own schedule: two or three waves per SIMD (three: footprint volume only), the skip
        // bitmap in LDS whenever it fits
        constexpr int kWavesR3 = FP ? kWavesWide : 4;   // (r3 only with FP)
        const bool r3 = FP && a.occ3;
        const bool rlds = a.skip.in_lds != 0 && (!r3 || wide_fits_lds(a));
        const int waves_r = r3 ? kWavesWide : 4;
        const auto kr = r3 ? (rlds ? vr_raycast_rays_kernel<VT, /*SKIP_LDS*/ true, FP, kWavesR3, VIEWS>
                                   : vr_raycast_rays_kernel<VT, /*SKIP_LDS*/ false, FP, kWavesR3, VIEWS>)
                           : (rlds ? vr_raycast_rays_kernel<VT, /*SKIP_LDS*/ true, FP, 4, VIEWS>
                                   : vr_raycast_rays_kernel<VT, /*SKIP_LDS*/ false, FP, 4, VIEWS>);
        const size_t lds_r = march_lds(waves_r, a, rlds);
        int nbr = 0;
        e = prepare_variant(kr, lds_r, &nbr, "raycast phase 1 (ray list)", a.num_cus, waves_r * 64);
        if (e != hipSuccess) return e;
        vr_launch_kernel(kr, dim3(cus * (uint32_t)nbr), dim3(waves_r * 64), lds_r, stream, start_ev, p1_ev, a.vol, a.bricks,
                         a.tf, a.skip, a.cells, frame, a.cam, a.render, a.raycast);
        if (a.info) { a.info->ray_list = 1; a.info->phase1_waves = (uint32_t)waves_r; a.info->skip_in_lds = rlds ? 1u : 0u; }
    } else {
        vr_launch_kernel(k1, grid, block, lds, stream, start_ev, p1_ev, a.vol, a.bricks, a.tf, a.skip, a.cells, frame, a.cam,
                         a.render, a.raycast, a.stats, a.touched);
    }
    e = hipGetLastError();
    if (e == hipSuccess && start_ev) *a.start_bound = true;
    if (e == hipSuccess && p1_ev && p1_ev == a.stop_event) *a.stop_bound = true;
    if (e == hipSuccess && a.mid_event && p1_ev != a.mid_event) e = hipEventRecord(a.mid_event, stream);
    if (e != hipSuccess || p1_last) return e;
    if (a.frame.order) {   // longest rays first (keys: last frame's phase-2 rounds per pixel)
        e = vr_launch_cont_sort(a.frame, stream);
        if (e != hipSuccess) return e;
    }
    // phase 2: persistent grid; exits at once when nothing was suspended
    dim3 grid2(cus * (uint32_t)nb2);
    vr_launch_kernel(k2, grid2, dim3(waves2 * 64), lds2, stream, nullptr, bind_stop ? a.stop_event : nullptr, a.vol, a.bricks,
                     a.tf, a.skip, a.cells, frame, a.cam, a.render, a.raycast, a.stats, a.touched);
    e = hipGetLastError();
    if (e == hipSuccess && bind_stop) *a.stop_bound = true;
    return e;
}

// The variant table: the instantiations of launch_variant that exist, one row each.  INSTR 2 (the traffic pass) renders
// one camera: its rows are never instantiated with VIEWS.
//      ESS    INSTR  SKIP_LDS  XS     FP
#define VR_RAYCAST_VARIANTS(ROW) \
    ROW(false, 0,     false,    false, true ) \
    ROW(true,  0,     false,    false, true ) \
    ROW(true,  0,     true,     false, true ) \
    ROW(false, 0,     false,    false, false) \
    ROW(false, 0,     false,    true,  false) \
    ROW(false, 1,     false,    false, false) \
    ROW(false, 1,     false,    true,  false) \
    ROW(false, 2,     false,    false, false) \
    ROW(false, 2,     false,    true,  false) \
    ROW(true,  0,     false,    false, false) \
    ROW(true,  0,     false,    true,  false) \
    ROW(true,  1,     false,    false, false) \
    ROW(true,  1,     false,    true,  false) \
    ROW(true,  2,     false,    false, false) \
    ROW(true,  2,     false,    true,  false) \
    ROW(true,  0,     true,     false, false) \
    ROW(true,  0,     true,     true,  false) \
    ROW(true,  1,     true,     false, false) \
    ROW(true,  1,     true,     true,  false) \
    ROW(true,  2,     true,     false, false) \
    ROW(true,  2,     true,     true,  false)

constexpr uint32_t variant_key(bool ess, int instr, bool skip_lds, bool xs, bool fp)
{
    return (uint32_t)ess | (uint32_t)instr << 1 | (uint32_t)skip_lds << 3 | (uint32_t)xs << 4 | (uint32_t)fp << 5;
}

template <typename VT, bool VIEWS>
hipError_t launch_typed(const RaycastLaunch &a, hipStream_t stream)
{
    // the traffic pass (instr 2: vrhip_count_touched) renders one camera
    if (VIEWS && a.instr >= 2) return hipErrorNotSupported;
    const bool ess = a.use_ess != 0;
    const int instr = a.instr == 0 ? 0 : a.instr == 1 ? 1 : 2;
    // the skip bitmap in LDS (phase 2 and the patch kernels; phase 1 on the ray list: launch_variant)
    const bool skip_lds = ess && a.skip.in_lds != 0 && (!a.occ3_split || wide_fits_lds(a));
    // the rarely used shading modes 2-5, contours, the depth cue and nearest filtering live in kernel
    // variants of their own (XS), so that their code and registers do not tax the default ones
    const bool xs = a.render.illumType >= 2 || a.raycast.useAO != 0 || a.render.showEss != 0 ||
                    a.render.imgEss != 0 || a.vol.channels > 1 || a.raycast.contours != 0 ||
                    a.raycast.aerial != 0 || a.render.useLinear == 0;
    // the default kernels read the footprint volume when the host has provided one for this frame
    const bool fp = !xs && instr == 0 && a.vol.fp;
    switch (variant_key(ess, instr, skip_lds, xs, fp)) {
#define VR_ROW(ESS, INSTR, SKIP_LDS, XS, FP) \
    case variant_key(ESS, INSTR, SKIP_LDS, XS, FP): \
        return launch_variant<VT, ESS, INSTR, SKIP_LDS, XS, FP, VIEWS && INSTR != 2>(a, stream);
        VR_RAYCAST_VARIANTS(VR_ROW)
#undef VR_ROW
    }
    return hipErrorInvalidValue;   // (no such row)
}

#if defined(VR_MARCH_STATS) || defined(VR_STAMPS)
// this unit's copy of diagnostic array `which`, added to sum[0, n) and cleared on request (vr_raycast_debug_*)
inline int debug_add(int which, unsigned long long *sum, size_t n, int reset)
{
    const void *sym = nullptr;
    size_t len = 0;
#ifdef VR_MARCH_STATS
    if (which == VR_DEBUG_MARCH_STATS) { sym = &g_march_stats; len = 32; }
#endif
#ifdef VR_STAMPS
    if (which == VR_DEBUG_STAMPS) { sym = &g_stamps; len = 32; }
    if (which == VR_DEBUG_WAVE_SPAN) { sym = &g_wave_span; len = 2 * 2 * 8192; }
#endif
    if (!sym || n != len) return -1;
    std::vector<unsigned long long> v(n);
    if (hipMemcpyFromSymbol(v.data(), sym, n * sizeof v[0]) != hipSuccess) return -1;
    for (size_t i = 0; i < n; ++i) sum[i] += v[i];
    if (!reset) return 0;
    std::fill(v.begin(), v.end(), 0ull);
    return hipMemcpyToSymbol(sym, v.data(), n * sizeof v[0]) == hipSuccess ? 0 : -1;
}
#endif

} // namespace

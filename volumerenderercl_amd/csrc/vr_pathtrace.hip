// vr_pathtrace.hip -- the Woodcock-tracking path-tracing mode of the reference kernel
// (/root/reference/src/kernel/volumeraycast.cl:686-706 with trace_volume :463-503,
// sample_interaction :407-437, get_dir_phase_function :453-460, gradientCentralDiffTff
// :181-206) for gfx950.
//
// One sample per pixel and launch; the caller accumulates over `iteration` (running mean in
// the fp32 frame buffer, as the ray caster does).  A pixel is up to three tracking walks --
// primary, optional scatter, shadow -- each a chain of up to 513 steps with a PER-CALL CONSTANT
// stride and acceptance threshold (`rand2 = ParallelRNG(rand)` is loop-invariant, :423-424;
// SURVEY A.8), so a walk is a strided march whose length differs wildly between neighbouring
// pixels (exponentially distributed stride, uniformly distributed threshold).
//
// Execution design: persistent workgroups, transfer function in LDS, and LANE-LEVEL work
// refill: every lane runs a small state machine (fetch pixel -> primary walk -> shade ->
// scatter walk -> shadow walk -> write) and draws its next pixel as soon as its current one is
// written, instead of waiting for the longest walk of an 8x8 patch.  Pixels are handed out in
// blocks of 64 from the same centre-first queue of 8x8 patches the ray caster uses, so a wave
// still works on neighbouring pixels most of the time.  Each round evaluates kPtBatch
// consecutive tracking steps of the lane's walk as independent straight-line code (addresses
// are clamped, so steps past the end of the walk are harmless speculation) and then resolves
// the walk's sequential exit conditions in order: the per-pixel operation sequence is the
// reference's.
//
// The kernel body is that loop -- draw, step, leap, shade, exit -- and the stages are defined once above it, as blocks
// expanded in place (as functions, or on structs, they change the kernel's register allocation):
//   draw   VR_PT_REFILL: VR_PT_DRAW_PATCH (the wave's next patch), VR_PT_START_PIXEL (make_ray to P_PRIMARY)
//   step   VR_PT_POSITIONS, VR_PT_CULL (bounds, the leap's seed), VR_PT_FETCH, VR_PT_RESOLVE (the exit conditions)
//   leap   VR_PT_LEAP: VR_PT_LEAP_STEPS (how many), VR_PT_LEAP_ADVANCE (on the bit pattern of t), VR_PT_LEAP_LAND
//   shade  VR_PT_WALK_ENDED (trace_volume's transitions), VR_PT_WRITE_PIXEL (VR_PT_RUNNING_MEAN, shared with the fold)
#include "vr_sampling.h"

namespace {

// Diagnostic build only (-DVR_STAMPS, tools/pt_stamps.py): where a wave of the path tracer spends its time -- summed shader
// clock per stage (a stamp waits for the memory queue, so a stage owns the latency of what it issued), calls, lifetime.
#ifdef VR_STAMPS
__device__ unsigned long long g_pt_stamps[16];
#define PT_STAMP(i) do { const unsigned long long n_ = vr_stamp(); pt_acc[i] += n_ - pt_last; pt_last = n_; } while (0)
#define PT_COUNT(i) pt_acc[i] += 1
#else
#define PT_STAMP(i)
#define PT_COUNT(i)
#endif

#ifndef VR_PT_BATCH
#define VR_PT_BATCH 6
#endif
constexpr int kPtBatch = VR_PT_BATCH;

enum : int { P_FETCH = 0, P_PRIMARY = 1, P_SCATTER = 2, P_SHADOW = 3, P_WRITE = 4, P_ENDED = 8 };
#ifndef VR_PT_STAGE_MIN
#define VR_PT_STAGE_MIN 16
#endif
// lanes that must wait for the (divergent) refill / shading code before it is worth running
constexpr int kStageMin = VR_PT_STAGE_MIN;
#ifndef VR_LEAP_MARGIN
#define VR_LEAP_MARGIN 1.f
#endif
#ifndef VR_LEAP_PIECES
#define VR_LEAP_PIECES 1
#endif
constexpr int kLeapPieces = VR_LEAP_PIECES;   // closed-form stretches of a leap (one binade each)
#ifndef VR_LEAP_CHAIN
#define VR_LEAP_CHAIN 1
#endif
constexpr int kLeapChain = VR_LEAP_CHAIN;     // leaps of a walk per round, each from the landing of the one before
#ifndef VR_PT_SHADE_MIN
#define VR_PT_SHADE_MIN VR_PT_STAGE_MIN
#endif
constexpr int kShadeMin = VR_PT_SHADE_MIN;   // the same for stage 3 (walk ends: shading, next walk, pixel write)

VR_DEV bool in_volume(f3 p)   // volumeraycast.cl:93-96
{
    return vmax(fabsf(p.x), vmax(fabsf(p.y), fabsf(p.z))) < 1.f;
}

// get_dir_phase_function, volumeraycast.cl:453-460
VR_DEV f3 dir_phase_function(uint32_t rnd)
{
    const uint32_t rand2 = parallel_rng(rnd);
    const float phi = (float)(2.0 * (double)3.14159274101257f) * map_uint_float(rand2);
    const float cos_theta = 1.0f - 2.0f * map_uint_float(parallel_rng(rand2));
    const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
    float s, c;
    vr_sincosf(phi, &s, &c);
    return mk3(c * sin_theta, s * sin_theta, cos_theta);
}

// illumination (:294-303) with specularBlinnPhong (:280-291)
VR_DEV f3 illumination(f3 color, f3 toLightDir, f3 n)
{
    const f3 l = normalize3(toLightDir);
    const float ndl = vmax(0.f, dot3(n, l));
    f3 h = add3(toLightDir, l);
    float sp = 0.0f;
    if (!(dot3(h, h) < 1.e-6f)) {
        h = normalize3(h);
        sp = vr_powr(vmax(dot3(n, h), 0.f), 40.f);
    }
    sp = sp * 0.15f;
    return mk3(((color.x * 0.15f) + ((color.x * ndl) * 0.7f)) + sp,
               ((color.y * 0.15f) + ((color.y * ndl) * 0.7f)) + sp,
               ((color.z * 0.15f) + ((color.z * ndl) * 0.7f)) + sp);
}

struct PtPixel {   // the pixel a lane is working on
    uint32_t gx, gy, out_index;
    uint32_t rnd;           // ParallelRNG3(x, y, seed), :688
    float dt, thr;          // stride (log(1-u)/max_extinction) and acceptance threshold of every walk
    float env0, env1, env2, env3;
    f3 dir;                 // primary ray direction
    f3 hit_pos;             // position of the primary interaction
    float c0, c1, c2;       // colour carried through trace_volume
    // current walk
    f3 org, wdir;
    float t;
    uint32_t cnt;
    // how it ended
    bool accepted;
    f3 apos;
    float adens;
};

struct PtCounters {   // INSTR builds
    unsigned long long taken, hit, culled, leaped;
};

// ---- draw: the wave's next patch, when the current one is handed out.  A wave's first patch is its own by position,
// the later ones are drawn behind those (no queue of 3 072 waves at one counter when the kernel starts -- see
// vr_raycast_rays_kernel) through one of kDrawCounters counters (a cache line each): counter k hands out the patches
// G + 8 j + k, a wave starts at k = its number mod 8 and moves on to the next counter when one has run out.  (One
// counter for 3 072 waves: +7 % on the sphere, +12 % on the shells.)  Queue empty: sets drained and leaves the
// refill loop it is expanded in.
// in: fr, lane, first_patch, sub, sub_tried.  out: patch_taken = 0, wt, seed -- or drained and a `break`.
#define VR_PT_DRAW_PATCH                                                                                              \
    if (patch_taken >= 64) {                                                                                          \
        uint32_t q = 0;                                                                                               \
        if (first_patch) {                                                                                            \
            q = blockIdx.x * (kBlockDim / 64u) + (threadIdx.x >> 6);                                                  \
        } else {                                                                                                      \
            const uint32_t G = gridDim.x * (kBlockDim / 64u);                                                         \
            for (;;) {                                                                                                \
                uint32_t j = 0;                                                                                       \
                if (lane == 0) j = atomicAdd(fr.draw_count + sub * kLiveStride, 1u);                                  \
                j = __builtin_amdgcn_readfirstlane(j);                                                                \
                q = G + j * kDrawCounters + sub;                                                                      \
                if (q < fr.n_wave_tiles || ++sub_tried >= kDrawCounters) break;                                       \
                sub = (sub + 1u) % kDrawCounters;                                                                     \
            }                                                                                                         \
        }                                                                                                             \
        first_patch = false;                                                                                          \
        if (q >= fr.n_wave_tiles) { drained = true; break; }                                                          \
        patch_taken = 0;                                                                                              \
        wt = fr.queue[q];                                                                                             \
        if (SAMPLES) seed = fr.seeds[wt_frame(wt)];                                                                   \
    }

// ---- pixel start: the lanes ranked below n_take take pixel patch_taken + rank of the patch, from make_ray to the
// start of the primary walk (P_PRIMARY, :473, :688, :423).  A pixel outside the frame (ragged right / bottom patches)
// is dropped, one whose ray misses the box is written here (:677-683): both leave the lane idle.
// in: rank, n_take (VR_PT_REFILL), patch_taken, wt, seed, fr, cam, rp, pt.  out: px, state, cn.hit.
#define VR_PT_START_PIXEL                                                                                             \
    if (state == P_FETCH && rank < n_take) {                                                                          \
        const uint32_t pi = patch_taken + rank;                                                                       \
        const uint32_t lx = pi & 7u, ly = pi >> 3;                                                                    \
        px.gx = wt_col(wt) * 8u + lx;                                                                                 \
        px.gy = wt_row(wt) * 8u + ly;                                                                                 \
        px.out_index = wt.out_base + ly * fr.out_stride + lx;                                                         \
        if (px.gx < fr.W && px.gy < fr.H) {                                                                           \
            const Ray ray = make_ray(px.gx, px.gy, fr, cam, rp, seed);                                                \
            px.env0 = ray.env[0]; px.env1 = ray.env[1];                                                               \
            px.env2 = ray.env[2]; px.env3 = ray.env[3];                                                               \
            if (!ray.hit) {                                                                                           \
                const float4 o = make_float4(px.env0, px.env1, px.env2, px.env3);                                     \
                if (SAMPLES) {                                                                                        \
                    fr.out[px.out_index] = o;                                                                         \
                    fr.sample_mark[px.out_index] = 0;                                                                 \
                } else {                                                                                              \
                    fr.fb[(size_t)px.gy * fr.W + px.gx] = o;                                                          \
                    if (fr.out) fr.out[px.out_index] = o;                                                             \
                }                                                                                                     \
            } else {                                                                                                  \
                if (INSTR) cn.hit++;                                                                                  \
                px.rnd = parallel_rng3(px.gx, px.gy, seed);                                                           \
                const uint32_t rand2 = parallel_rng(px.rnd);                                                          \
                px.dt = vr_logf(1.f - map_uint_float(rand2)) / pt.max_extinction;                                     \
                px.thr = map_uint_float(px.rnd);                                                                      \
                px.dir = ray.dir;                                                                                     \
                px.c0 = px.env0; px.c1 = px.env1; px.c2 = px.env2;                                                    \
                px.org = add3(ray.cam, scale3(ray.dir, ray.tnear));                                                   \
                px.wdir = ray.dir;                                                                                    \
                px.t = 0.f;                                                                                           \
                px.cnt = 0;                                                                                           \
                state = P_PRIMARY;                                                                                    \
            }                                                                                                         \
        }                                                                                                             \
    }

// ---- stage 1: hand out pixels to the idle lanes, patch by patch, until none is idle or the queue is empty
// in: idle_m, lane and the inputs of the two blocks inside it.  out: idle_m, patch_taken, drained, px, state.
#define VR_PT_REFILL                                                                                                  \
    {                                                                                                                 \
        unsigned long long idle = idle_m;                                                                             \
        while (idle && !drained) {                                                                                    \
            VR_PT_DRAW_PATCH                                                                                          \
            /* the i-th idle lane takes pixel patch_taken + i of the patch */                                         \
            const uint32_t rank = (uint32_t)__builtin_popcountll(idle & ((1ull << lane) - 1ull));                     \
            const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle);                                             \
            const uint32_t avail = 64u - patch_taken;                                                                 \
            const uint32_t n_take = n_idle < avail ? n_idle : avail;                                                  \
            VR_PT_START_PIXEL                                                                                         \
            patch_taken += n_take;                                                                                    \
            idle = __ballot(state == P_FETCH);                                                                        \
        }                                                                                                             \
        idle_m = idle;                                                                                                \
    }

// ---- stage 2, positions: the next B steps of the walk (:419-431), as if none of them ended it
// in: px, walking.  out: tk[], pk[], ink[], need[] (declared by the kernel).
#define VR_PT_POSITIONS                                                                                               \
    float tc = px.t;                                                                                                  \
    _Pragma("unroll")                                                                                                 \
    for (int k = 0; k < B; ++k) {                                                                                     \
        tc = tc - px.dt;                                                                                              \
        tk[k] = tc;                                                                                                   \
        pk[k] = add3(px.org, scale3(px.wdir, tc));                                                                    \
        ink[k] = in_volume(pk[k]);                                                                                    \
        need[k] = walking && ink[k];                                                                                  \
    }

// ---- stage 2, majorant cull: no value a fetch in this cell can return maps to an opacity that reaches the walk's
// threshold -> the step is a rejection whatever the voxels hold.  The cell of step k is the walk's cell line at tk[k]
// (vr_sampling.h, "the cell of a point on a line": VR_CELL_LINE_WALK, VR_CELL_AXIS -- cell_at's own text -- and the
// proofs (1)-(5)).  Steps outside the volume (never fetched: `ink`) clamp to a cell inside.  With `leap`, the line, the
// macro cell of the batch's last step, its bound and -- from CellView::cdist -- how far the macro cells around are free
// at the level below the walk's threshold go to the leap.
// in: cull, leap, px, vol, grid, tk[].  out: need[]; for the leap la*, lb* (the line), lc* (macro cell), lcb, lrad,
// llev.
#define VR_PT_CULL                                                                                                    \
    if (cull) {                                                                                                       \
        VR_CELL_LINE_WALK(px.org, px.wdir, vol, grid.shift, grid.cx, grid.cy, grid.cz);                               \
        float bnd[B];                                                                                                 \
        _Pragma("unroll")                                                                                             \
        for (int k = 0; k < B; ++k) {                                                                                 \
            Cell c;                                                                                                   \
            c.x = VR_CELL_AXIS(ax, bx, tk[k], mx);                                                                    \
            c.y = VR_CELL_AXIS(ay, by, tk[k], my);                                                                    \
            c.z = VR_CELL_AXIS(az, bz, tk[k], mz);                                                                    \
            bnd[k] = grid.bound[cell_index_of(c, grid.cx, grid.cy)];                                                  \
            if (k == B - 1 && leap) {                                                                                 \
                lcx = c.x >> kLeapShift; lcy = c.y >> kLeapShift; lcz = c.z >> kLeapShift;                            \
                const uint32_t ci = (lcz * (uint32_t)grid.ccy + lcy) * (uint32_t)grid.ccx + lcx;                      \
                lcb = grid.cbound[ci];                                                                                \
                if (grid.cdist) {                                                                                     \
                    const uint32_t j = (uint32_t)(px.thr * 8.f);   /* tau_j = j / 8 <= thr (exact: a power of two) */ \
                    const uint32_t jj = j < (uint32_t)kLeapLevels ? j : (uint32_t)kLeapLevels;                        \
                    if (jj) {                                                                                         \
                        llev = (jj - 1u) * (uint32_t)(grid.ccx * grid.ccy * grid.ccz);                                \
                        lrad = grid.cdist[llev + ci];                                                                 \
                    }                                                                                                 \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
        lax = ax; lbx = bx; lay = ay; lby = by; laz = az; lbz = bz;                                                   \
        _Pragma("unroll")                                                                                             \
        for (int k = 0; k < B; ++k) need[k] = need[k] && !(bnd[k] < px.thr);                                          \
    }

// ---- stage 2, fetch and transfer function -- behind ONE wave-uniform test: with the cull, seven rounds in eight need
// neither for any lane, and a guard per step is a handful of scalar instructions each.  (The opacity only matters
// where the step was fetched: the exit resolution tests `need` first, :432.)
// in: cull, need[], pk[], vol, s_tff, tffn.  out: dens[], al[].
#define VR_PT_FETCH                                                                                                   \
    bool any_need = !cull;                                                                                            \
    _Pragma("unroll")                                                                                                 \
    for (int k = 0; k < B; ++k) {                                                                                     \
        dens[k] = 0.f;                                                                                                \
        al[k] = 0.f;                                                                                                  \
        any_need = any_need || need[k];                                                                               \
    }                                                                                                                 \
    if (__ballot(any_need)) {                                                                                         \
        _Pragma("unroll")                                                                                             \
        for (int k = 0; k < B; ++k)                                                                                   \
            if (need[k] || (INSTR < 2 && !cull))                                                                      \
                dens[k] = vol.linear(pk[k].x * 0.5f + 0.5f, pk[k].y * 0.5f + 0.5f, pk[k].z * 0.5f + 0.5f);            \
        _Pragma("unroll")                                                                                             \
        for (int k = 0; k < B; ++k)                                                                                   \
            if (need[k] || !cull) al[k] = tff_linear_alpha<kRawDensity<VT>>(s_tff, tffn, dens[k]);                    \
    }

// ---- stage 2, exit resolution: the walk's exit conditions, in step order -- as selects, not branches (the bodies are
// assignments; as nested ifs they were ~25 scalar mask instructions per step): step k happens while `run`; it leaves
// the volume (:426-427), exceeds the step limit (:430-431) or is accepted (:432), in that order.  Declares `run`: the
// walk goes on behind the batch.
// in: walking, tk[], pk[], ink[], need[], al[], dens[].  out: run (declared here), px.t, px.cnt, px.accepted,
// px.apos, px.adens, cn.taken, cn.culled.
#define VR_PT_RESOLVE                                                                                                 \
    bool run = walking;                                                                                               \
    _Pragma("unroll")                                                                                                 \
    for (int k = 0; k < B; ++k) {                                                                                     \
        const bool st = run;                                                                                          \
        px.cnt += st ? 1u : 0u;                                                                                       \
        px.t = st ? tk[k] : px.t;                                                                                     \
        const bool out = !ink[k];                                                                                     \
        const bool over = px.cnt > 512u;                                                                              \
        const bool acc = need[k] && !(al[k] < px.thr);                                                                \
        const bool accept = st && !out && !over && acc;                                                               \
        const bool stop = st && (out || over || acc);                                                                 \
        if (INSTR) {                                                                                                  \
            cn.taken += (st && !out) ? 1u : 0u;                                                                       \
            cn.culled += (st && !out && !need[k]) ? 1u : 0u;                                                          \
        }                                                                                                             \
        px.accepted = stop ? accept : px.accepted;                                                                    \
        px.apos.x = accept ? pk[k].x : px.apos.x;                                                                     \
        px.apos.y = accept ? pk[k].y : px.apos.y;                                                                     \
        px.apos.z = accept ? pk[k].z : px.apos.z;                                                                     \
        px.adens = accept ? dens[k] : px.adens;                                                                       \
        run = st && !stop;                                                                                            \
    }

// ---- the leap, how many steps (`left`): to where the line leaves the cube of macro cells [C - R, C + R] per axis, in
// cells (R = 0: the macro cell [4 C, 4 C + 4) itself), cut at the volume's own faces (cell coordinate 0 and res / E: a
// walk that leaves the volume inside the cube lands just before it does, instead of failing the landing check and
// taking no leap at all) -- and within the step limit (cnt <= 512 while `run`).  An estimate, from reciprocals.
// in: can, sst (VR_PT_LEAP), la*, lb*, lc*, lrad, px.t, px.cnt, vol, grid.  out: R, left (declared here).
#define VR_PT_LEAP_STEPS                                                                                              \
    const int R = lrad ? (int)lrad - 1 : 0;                                                                           \
    const float inv_e = __uint_as_float((uint32_t)(127 - grid.shift) << 23);                                          \
    const float ux = vol.fw * inv_e, uy = vol.fh * inv_e, uz = vol.fd * inv_e;                                        \
    const float ex = __builtin_amdgcn_fmed3f((float)(((int)lcx + (lbx > 0.f ? R + 1 : -R)) * (1 << kLeapShift)), 0.f, ux); \
    const float ey = __builtin_amdgcn_fmed3f((float)(((int)lcy + (lby > 0.f ? R + 1 : -R)) * (1 << kLeapShift)), 0.f, uy); \
    const float ez = __builtin_amdgcn_fmed3f((float)(((int)lcz + (lbz > 0.f ? R + 1 : -R)) * (1 << kLeapShift)), 0.f, uz); \
    const float tx = lbx != 0.f ? (ex - lax) * __builtin_amdgcn_rcpf(lbx) : 3.0e38f;                                  \
    const float ty = lby != 0.f ? (ey - lay) * __builtin_amdgcn_rcpf(lby) : 3.0e38f;                                  \
    const float tz = lbz != 0.f ? (ez - laz) * __builtin_amdgcn_rcpf(lbz) : 3.0e38f;                                  \
    const float t_out = vmin(tx, vmin(ty, tz));                                                                       \
    const float n_cell = (t_out - px.t) * __builtin_amdgcn_rcpf(sst);                                                 \
    const float n_f = vmin(n_cell - VR_LEAP_MARGIN, (float)(512u - px.cnt));                                          \
    uint32_t left = (can && n_f >= 1.f) ? (uint32_t)n_f : 0u;

// ---- the leap, the steps themselves, on the bit pattern of t: (ti, left, si) -> (tb, n), n <= left steps of sst taken
// from the float with bits ti, tb the bits after them.  kLeapPieces stretches in closed form, each within the binade t
// is in, with one real step t + s between two of them -- the step that crosses into the next binade when the stretch
// before it reached the top.  Within a binade t + s is rounded to a multiple of ulp(t), s / ulp(t) = q + f with the
// same q and f at every step, so every step adds inc = q (f < 1/2) or q + 1 (f > 1/2) ulps to the bit pattern (f = 1/2
// -- a tie, resolved by the parity of the sum -- has no closed form and ends the stretch).  A stretch takes
// k = min(left, floor(room / inc)) steps, room = the ulps to the top of the binade: the quotient from a reciprocal,
// exact after one correction each way when it matters (quotients up to left + 4 <= 516; a larger estimate is >= left
// for sure).  Integer and bit arithmetic only.
// in: ti, si, es, sst (VR_PT_LEAP), left (VR_PT_LEAP_STEPS; used up).  out: tb, n (declared here).
#define VR_PT_LEAP_ADVANCE                                                                                            \
    const uint32_t ms = (si & 0x7fffffu) | 0x800000u;                                                                 \
    uint32_t tb = ti, n = 0;                                                                                          \
    _Pragma("unroll")                                                                                                 \
    for (int piece = 0; piece < kLeapPieces; ++piece) {                                                               \
        const int e_t = (int)(tb >> 23), dsh = e_t - es;                                                              \
        const bool closed = dsh >= 1 && dsh <= 24 && e_t < 255;                                                       \
        const uint32_t sh = (uint32_t)dsh & 31u;                                                                      \
        const uint32_t q = ms >> sh, rem = ms & ((1u << sh) - 1u), half = (1u << sh) >> 1;                            \
        const uint32_t inc = q + (rem > half ? 1u : 0u);                                                              \
        const uint32_t room = (tb | 0x7fffffu) - tb;                                                                  \
        uint32_t k = (uint32_t)((float)room * __builtin_amdgcn_rcpf((float)(inc ? inc : 1u)));                        \
        if (k > left + 4u) {                                                                                          \
            k = left;                                                                                                 \
        } else {                                                                                                      \
            k -= (k * inc > room) ? 1u : 0u;                                                                          \
            k += ((k + 1u) * inc <= room) ? 1u : 0u;                                                                  \
            k = k < left ? k : left;                                                                                  \
        }                                                                                                             \
        k = (closed && rem != half && __umulhi(k, inc) == 0u && k * inc <= room) ? k : 0u;                            \
        tb += k * inc;                                                                                                \
        left -= k;                                                                                                    \
        n += k;                                                                                                       \
        if (piece + 1 < kLeapPieces) {                                                                                \
            const bool one = left != 0u;                                                                              \
            tb = one ? __float_as_uint(__uint_as_float(tb) + sst) : tb;                                               \
            left -= one ? 1u : 0u;                                                                                    \
            n += one ? 1u : 0u;                                                                                       \
        }                                                                                                             \
    }

// ---- the leap, landing check: the landing step is inside the volume, inside the cube (its cell from the cull's own
// line la*, lb* through the same VR_CELL_AXIS: the stepping code's arithmetic by construction) and within the step
// limit -- then the walk is there.
// in: tb, n (VR_PT_LEAP_ADVANCE), R (VR_PT_LEAP_STEPS), can, la*, lb*, lc*, px, grid.  out: ok, cl (the landing's cell;
// declared here), px.t, px.cnt, cn.
#define VR_PT_LEAP_LAND                                                                                               \
    const float tn = __uint_as_float(tb);                                                                             \
    const f3 pn = add3(px.org, scale3(px.wdir, tn));                                                                  \
    const float gmx = VR_CELL_MAX(grid.cx), gmy = VR_CELL_MAX(grid.cy), gmz = VR_CELL_MAX(grid.cz);                   \
    Cell cl;                                                                                                          \
    cl.x = VR_CELL_AXIS(lax, lbx, tn, gmx);                                                                           \
    cl.y = VR_CELL_AXIS(lay, lby, tn, gmy);                                                                           \
    cl.z = VR_CELL_AXIS(laz, lbz, tn, gmz);                                                                           \
    const int ddx = (int)(cl.x >> kLeapShift) - (int)lcx, ddy = (int)(cl.y >> kLeapShift) - (int)lcy,                 \
              ddz = (int)(cl.z >> kLeapShift) - (int)lcz;                                                             \
    const bool ok = can && n != 0u && px.cnt + n <= 512u && in_volume(pn) && ddx >= -R && ddx <= R &&                 \
                    ddy >= -R && ddy <= R && ddz >= -R && ddz <= R;                                                   \
    px.t = ok ? tn : px.t;                                                                                            \
    px.cnt += ok ? n : 0u;                                                                                            \
    if (INSTR) {                                                                                                      \
        cn.taken += ok ? n : 0u;                                                                                      \
        cn.culled += ok ? n : 0u;                                                                                     \
        cn.leaped += ok ? n : 0u;                                                                                     \
    }

// ---- the leap: a walk whose batch ended with a rejected step in a macro cell (4^3 cells) whose bound is below its
// threshold takes ALL its further steps inside that macro cell at once -- or inside the cube of macro cells around it
// that CellView::cdist says are free as well.  Exact, because
//  * every one of those steps is a rejection: its cell lies in the macro cell (the cube), so its bound is below the
//    threshold -- and it lies in there because the last step taken does, the landing step does (VR_PT_LEAP_LAND) and a
//    step's cell is monotone in t (vr_sampling.h, (5)), as is its position org + wdir * t, axis by axis: what holds at
//    both ends of a stretch of the walk (the same macro cell, inside the volume) holds in between;
//  * t after n steps is known in closed form while it stays in its binade (VR_PT_LEAP_ADVANCE); at the binade's top
//    one real step t + s crosses over, and the next stretch has its own inc;
//  * the step counter stays within the limit of 512 (:430).
// The number of steps comes from the macro cell's exit along the walk's line in cell space and the room in the binade,
// both estimated and then VERIFIED: landing cell, landing position, bit pattern.
// A leap that lands (one step short of its cube's face) in a macro cell with free macro cells around it starts the
// next one from there -- the landing step is a rejected step in a known macro cell like the batch's last one -- for
// the price of that macro cell's two table entries (a dependent load, but from tables of a few hundred KB) instead of
// a whole round: kLeapChain hops at most.
// in: leap, run (VR_PT_RESOLVE), the cull's la*, lb*, lc*, lcb, lrad, llev, px, vol, grid.  out: px.t, px.cnt, cn;
// lc*, lcb, lrad move on with the hops.  Inside a hop: sst, ti, si, es, can, then what the three blocks above declare.
#define VR_PT_LEAP                                                                                                    \
    bool go = run;                                                                                                    \
    _Pragma("unroll 1")                                                                                               \
    for (int hop = 0; leap && hop < kLeapChain; ++hop) {                                                              \
        const float sst = -px.dt;                                                                                     \
        const uint32_t ti = __float_as_uint(px.t), si = __float_as_uint(sst);                                         \
        const int et = (int)(ti >> 23), es = (int)(si >> 23);   /* (a sign bit makes the exponent >= 256) */          \
        /* (rad != 0: the macro cell and those within rad - 1 around it have bounds < tau_j <= thr) */                \
        const bool can = go && (lrad != 0u || lcb < px.thr) && et > 0 && et < 255 && es > 0 && es < 255;              \
        if (!__ballot(can)) break;                                                                                    \
        {                                                                                                             \
            VR_PT_LEAP_STEPS                                                                                          \
            VR_PT_LEAP_ADVANCE                                                                                        \
            VR_PT_LEAP_LAND                                                                                           \
            /* the next hop: from the landing's macro cell, if the tables say there is room around it */              \
            go = false;                                                                                               \
            if (hop + 1 < kLeapChain && grid.cdist) {                                                                 \
                const bool more = ok && px.cnt < 512u && llev != 0xffffffffu;                                         \
                if (!__ballot(more)) break;                                                                           \
                if (more) {                                                                                           \
                    lcx = cl.x >> kLeapShift; lcy = cl.y >> kLeapShift; lcz = cl.z >> kLeapShift;                     \
                    const uint32_t ci = (lcz * (uint32_t)grid.ccy + lcy) * (uint32_t)grid.ccx + lcx;                  \
                    lrad = grid.cdist[llev + ci];                                                                     \
                    lcb = 0.f;                 /* (rad != 0 says the cell is free at the walk's level; 0: no hop) */  \
                    /* a cube of radius >= 1: further than the one step left in this cell */                          \
                    go = lrad >= 2u;                                                                                  \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
    }

// ---- stage 3, trace_volume's transitions (:463-503) for a lane whose walk ended: the primary walk's end shades the
// interaction (:483-486 high gradient: Phong, then the shadow walk; :487-494 low gradient: a second, scatter walk), the
// scatter walk's end mixes its colour in (:493) and starts the shadow walk (:496-497, towards the light, from the
// interaction), the shadow walk's end dims the colour (:497-499).  Leaves `state` at the next walk, or at P_WRITE.
// in: state (P_ENDED set), px, vol, s_tff, tffn.  out: state, px (colour, hit_pos, the next walk).
#define VR_PT_WALK_ENDED                                                                                              \
    const int ended = state & ~P_ENDED;                                                                               \
    bool start_shadow = false;                                                                                        \
    if (ended == P_PRIMARY) {                                                                                         \
        if (!px.accepted) {                                                                                           \
            state = P_WRITE;                                                                                          \
        } else {                                                                                                      \
            const float4 col = tff_linear<kRawDensity<VT>>(s_tff, tffn, px.adens);                                    \
            px.c0 = col.x; px.c1 = col.y; px.c2 = col.z;                                                              \
            px.hit_pos = px.apos;                                                                                     \
            const f3 sp = mk3(px.apos.x * 0.5f + 0.5f, px.apos.y * 0.5f + 0.5f,                                       \
                              px.apos.z * 0.5f + 0.5f);                                                               \
            const float4 gq = gradient_tff<VT, VI>(vol, s_tff, tffn, sp);                                             \
            const float g0 = -gq.x, g1 = -gq.y, g2 = -gq.z, g3 = -gq.w;                                               \
            const float glen = sqrtf((((g0 * g0) + (g1 * g1)) + (g2 * g2)) + (g3 * g3));                              \
            if (glen > 0.5f) {                                                                                        \
                const f3 light = add3(neg3(px.dir), mk3(0.5f, 0.5f, 0.f));                                            \
                const f3 c = illumination(mk3(px.c0, px.c1, px.c2), light, mk3(g0, g1, g2));                          \
                px.c0 = c.x; px.c1 = c.y; px.c2 = c.z;                                                                \
                start_shadow = true;                                                                                  \
            } else {                                                                                                  \
                px.org = px.apos;                                                                                     \
                px.wdir = dir_phase_function(px.rnd);                                                                 \
                px.t = 0.f;                                                                                           \
                px.cnt = 0;                                                                                           \
                state = P_SCATTER;                                                                                    \
            }                                                                                                         \
        }                                                                                                             \
    } else if (ended == P_SCATTER) {                                                                                  \
        float s0 = px.env0, s1 = px.env1, s2 = px.env2;                                                               \
        if (px.accepted) {                                                                                            \
            const float4 col = tff_linear<kRawDensity<VT>>(s_tff, tffn, px.adens);                                    \
            s0 = col.x; s1 = col.y; s2 = col.z;                                                                       \
        }                                                                                                             \
        px.c0 = px.c0 + (s0 - px.c0) * 0.5f;                                                                          \
        px.c1 = px.c1 + (s1 - px.c1) * 0.5f;                                                                          \
        px.c2 = px.c2 + (s2 - px.c2) * 0.5f;                                                                          \
        start_shadow = true;                                                                                          \
    } else {                                                                                                          \
        const float w = px.accepted ? 0.6f : 1.f;                                                                     \
        px.c0 = px.c0 * w; px.c1 = px.c1 * w; px.c2 = px.c2 * w;                                                      \
        state = P_WRITE;                                                                                              \
    }                                                                                                                 \
    if (start_shadow) {                                                                                               \
        px.org = px.hit_pos;                                                                                          \
        px.wdir = add3(neg3(px.dir), mk3(0.5f, 0.5f, 0.f));                                                           \
        px.t = 0.f;                                                                                                   \
        px.cnt = 0;                                                                                                   \
        state = P_SHADOW;                                                                                             \
    }

// The progressive image's running mean (:689-704) on r0, r1, r2: the sample joins PREV (read only then) with iteration
// IT; the sample of iteration 0 is written, never averaged -- what the frame buffer held does not leak in.
// in: r0, r1, r2 (the sample), PREV, IT.  out: r0, r1, r2.
#define VR_PT_RUNNING_MEAN(PREV, IT)                                                                                  \
    if ((IT) != 0) {                                                                                                  \
        const float4 prev = PREV;                                                                                     \
        const float it1 = (float)((IT) + 1u);                                                                         \
        r0 = prev.x + (r0 - prev.x) / it1;                                                                            \
        r1 = prev.y + (r1 - prev.y) / it1;                                                                            \
        r2 = prev.z + (r2 - prev.z) / it1;                                                                            \
    }

// ---- stage 3, pixel write (:689-704): a set's sample as it is (the fold accumulates), else accumulated into the frame
// in: state, px, fr, rp.iteration.  out: the pixel; state = P_FETCH where it was P_WRITE.
#define VR_PT_WRITE_PIXEL                                                                                             \
    if (SAMPLES && state == P_WRITE) {                                                                                \
        fr.out[px.out_index] = make_float4(px.c0, px.c1, px.c2, 1.f);                                                 \
        fr.sample_mark[px.out_index] = 1;                                                                             \
        state = P_FETCH;                                                                                              \
    }                                                                                                                 \
    if (state == P_WRITE) {                                                                                           \
        const size_t fi = (size_t)px.gy * fr.W + px.gx;                                                               \
        float r0 = px.c0, r1 = px.c1, r2 = px.c2;                                                                     \
        VR_PT_RUNNING_MEAN(fr.fb[fi], rp.iteration);                                                                  \
        const float4 o = make_float4(r0, r1, r2, 1.f);                                                                \
        fr.fb[fi] = o;                                                                                                \
        if (fr.out) fr.out[px.out_index] = o;                                                                         \
        state = P_FETCH;                                                                                              \
    }

#ifdef VR_PT_WAVES_PER_EU   // A/B builds: more waves per SIMD at fewer registers
#define VR_PT_OCC __attribute__((amdgpu_waves_per_eu(VR_PT_WAVES_PER_EU, VR_PT_WAVES_PER_EU)))
#else
#define VR_PT_OCC
#endif
// SAMPLES (vrhip_render_samples): the work queue holds every patch once per SAMPLE of a set of consecutive iterations
// of the progressive image (the sample's index rides in the patch's frame bits, its seed is fr.seeds[index]), so the
// launch, an idle wave's ray set-up and the tail of lanes finishing one by one are paid once per set.  The running
// mean is order-dependent fp32 arithmetic and a pixel's samples end in any order, on any wave: this variant never
// touches fr.fb.  It writes every sample's raw colour to its plane of a scratch buffer (fr.out, which the queue's
// out_base already addresses plane by plane) and one byte beside it (fr.sample_mark: 1 traced, 0 the ray missed the
// box and the record is the background) -- a background's alpha may be any float, 1 included, so no alpha value can
// carry that mark.  vr_pt_fold_kernel below then folds the planes into the frame buffer in sample order.
template <typename VT, int INSTR, bool SAMPLES = false>
__global__ __launch_bounds__(kBlockDim) VR_PT_OCC void vr_pathtrace_kernel(
    VolView vv, TfView tf, CellView grid, FrameView fr, vrhip_camera_params cam,
    vrhip_rendering_params rp, vrhip_pathtrace_params pt, DevStats *stats, uint32_t *touched)
{
    VR_ZERO_NEXT_CTRL(fr);
    extern __shared__ float4 s_mem[];
    float4 *s_tff = s_mem;
    for (uint32_t i = threadIdx.x; i < tf.tff_n; i += kBlockDim) s_tff[i] = tf.tff[i];
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const int tffn = (int)tf.tff_n;
    PtCounters cn = {0, 0, 0, 0};
    // The instrumented traffic variant (INSTR 2) reproduces the reference's fetch set: no culling.
    // INSTR 3 records the micro-bricks of the fetches the culling lets through -- what the production
    // kernel needs from the volume (vrhip_count_fetched).
    const bool cull = INSTR != 2 && grid.bound != nullptr;
    constexpr int VI = INSTR == 3 ? 2 : INSTR;   // the sampler's instrumentation level
    const Vol<VT, VI> vol = make_vol<VT, VI, false>(vv, touched);
    // the traffic-instrumented variant must not touch speculative voxels: one step per round
    constexpr int B = INSTR >= 2 ? 1 : kPtBatch;
    const bool leap = cull && grid.cbound != nullptr;   // leaps over macro cells (stage 2)

    PtPixel px = {};
    int state = P_FETCH;
    uint32_t patch_taken = 64;         // pixels of the current patch already handed out (wave-uniform)
    bool drained = false;              // queue exhausted (wave-uniform)
    bool first_patch = true;
    uint32_t sub = (blockIdx.x * (kBlockDim / 64u) + (threadIdx.x >> 6)) % kDrawCounters, sub_tried = 0;   // (the draw's counters)
    WaveTile wt = {0, 0, 0};
    uint32_t seed = rp.seed;           // of the current patch (wave-uniform): its sample's own with SAMPLES

    // Exit condition reached by every wave: the queue head only grows, every walk ends after at
    // most 513 steps, and the refill / transition stages run unconditionally once no lane walks.
    // The lanes by state, as wave masks kept across the rounds (a round in which nobody is handed a pixel or shaded --
    // most rounds -- recomputes only the two that stage 2 changes): idle (P_FETCH), walking, walk ended (P_ENDED).
    unsigned long long idle_m = ~0ull, walk_m = 0ull;
#ifdef VR_STAMPS
    unsigned long long pt_acc[16] = {0}, pt_last = vr_stamp(), pt_first = pt_last, pt_drained = 0;
#endif
    for (;;) {
        PT_STAMP(6);   // loop control
        // ---- stage 1, draw: hand out pixels to idle lanes -- when enough lanes are idle to pay for the
        //      ray set-up code, or when nothing else is left to do
        if (!drained && idle_m && ((int)__builtin_popcountll(idle_m) >= kStageMin || !walk_m)) {
            VR_PT_REFILL
            walk_m = __ballot(state >= P_PRIMARY && state <= P_SHADOW);
            PT_STAMP(0);
            PT_COUNT(8);
#ifdef VR_STAMPS
            if (drained && !pt_drained) pt_drained = pt_last;
#endif
        }

        // ---- stage 2, step: kPtBatch consecutive tracking steps of every walking lane (:419-431), then the leap
        const bool walking = state >= P_PRIMARY && state <= P_SHADOW;
        if (walk_m) {
            float tk[B], dens[B], al[B];
            f3 pk[B];
            bool ink[B], need[B];
            // what the cull hands to the leap: the walk's cell line (offset la*, slope lb*), the macro cell of the batch's
            // last step (lc*), its bound (lcb), its free radius at the walk's level (lrad) and that level's offset (llev)
            float lax = 0.f, lbx = 0.f, lay = 0.f, lby = 0.f, laz = 0.f, lbz = 0.f, lcb = 0.f;
            uint32_t lcx = 0, lcy = 0, lcz = 0, lrad = 0, llev = 0xffffffffu;
            VR_PT_POSITIONS
            VR_PT_CULL
            PT_STAMP(1);   // positions, cells, bound loads
            PT_COUNT(9);
            VR_PT_FETCH
            PT_STAMP(2);   // fetch + TF
            VR_PT_RESOLVE
            if (walking && !run) state |= P_ENDED;
            PT_STAMP(3);   // exit conditions
            VR_PT_LEAP
        }

        PT_STAMP(4);   // leap
        // ---- stage 3, shade: trace_volume's control flow (:463-503) for lanes whose walk ended -- again
        //      only when enough lanes wait, or no lane walks any more
        const unsigned long long pend = __ballot((state & P_ENDED) != 0);
        walk_m = __ballot(state >= P_PRIMARY && state <= P_SHADOW);
        // (once the queue is empty nothing new will join the lanes that wait: a walk's end is handled at once, or its
        // pixel's next walk would start only when every other walk of the wave has ended -- walks in series, not side by side)
#ifndef VR_PT_DRAIN_SHADE_MIN
#define VR_PT_DRAIN_SHADE_MIN 1
#endif
        // (A wave learns that the queue is empty when it next draws from it, not before.  Looking at the queue's head
        // every few rounds instead -- thousands of waves reading the one address the draws update -- was measured at 2.4x
        // the kernel's time.)
        const int shade_min = drained ? VR_PT_DRAIN_SHADE_MIN : kShadeMin;
        const bool shade = pend && ((int)__builtin_popcountll(pend) >= shade_min || !walk_m);
        if (shade && (state & P_ENDED)) {
            VR_PT_WALK_ENDED
            VR_PT_WRITE_PIXEL
        }
        if (shade) {
            idle_m = __ballot(state == P_FETCH);
            walk_m = __ballot(state >= P_PRIMARY && state <= P_SHADOW);
            PT_STAMP(5);   // walk ends: shading, next walk, pixel write
            PT_COUNT(10);
        }
        // ---- exit: the queue is empty and every lane has written its pixel
        if (drained && idle_m == ~0ull) break;
    }

#ifdef VR_STAMPS
    if (lane == 0) {
        const unsigned long long end_ = vr_stamp();
        for (int i_ = 0; i_ < 11; ++i_) atomicAdd(&g_pt_stamps[i_], pt_acc[i_]);
        atomicAdd(&g_pt_stamps[11], end_ - pt_first);                              // wave lifetime
        atomicAdd(&g_pt_stamps[12], pt_drained ? end_ - pt_drained : 0ull);        // ... of it after the queue was empty
        atomicMax(&g_pt_stamps[13], end_ - pt_first);                              // the longest wave
        atomicAdd(&g_pt_stamps[14], 1ull);
    }
#endif
    if (INSTR) {
        unsigned long long s = wave_sum(cn.taken);
        if (lane == 0 && s) atomicAdd(&stats->v[0], s);
        s = wave_sum(cn.hit);
        if (lane == 0 && s) atomicAdd(&stats->v[5], s);
        // technique 1 reuses the two brick counters: steps whose bound was consulted / culled
        s = wave_sum(cn.culled);
        if (lane == 0 && s) atomicAdd(&stats->v[4], s);
        s = wave_sum(cn.leaped);   // samples_nominal: the steps taken in leaps (among the culled ones)
        if (lane == 0 && s) atomicAdd(&stats->v[1], s);
        s = wave_sum(cull ? cn.taken : 0ull);
        if (lane == 0 && s) atomicAdd(&stats->v[3], s);
    }
}

// The fold of a set of samples (vr_pathtrace_kernel with SAMPLES): one thread per pixel of the set's patches -- the
// patches of sample 0, every n-th queue entry -- walks the pixel's n records in sample order and applies what the
// one-sample kernel applies per launch (:689-704 and :677-683): a traced sample enters the running mean with
// iteration first + k (the sample of iteration 0 is written, never averaged: what the frame buffer held does not
// leak in), a missed one replaces the pixel, alpha included.  A patch row is 128 contiguous bytes of a plane.
__global__ __launch_bounds__(kBlockDim) void vr_pt_fold_kernel(FrameView fr, const float4 *planes, const uint8_t *mark,
                                                               uint32_t n, uint32_t plane, uint32_t first, float4 *out)
{
    const uint32_t p = blockIdx.x * (kBlockDim / 64u) + (threadIdx.x >> 6);
    if (p >= fr.n_wave_tiles / n) return;
    const WaveTile wt = fr.queue[(size_t)p * n];
    const uint32_t lx = threadIdx.x & 7u, ly = (threadIdx.x >> 3) & 7u;
    const uint32_t gx = wt_col(wt) * 8u + lx, gy = wt_row(wt) * 8u + ly;
    if (gx >= fr.W || gy >= fr.H) return;
    const size_t oi = (size_t)wt.out_base + ly * fr.out_stride + lx, fi = (size_t)gy * fr.W + gx;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (first != 0) acc = fr.fb[fi];
#pragma unroll 4
    for (uint32_t k = 0; k < n; ++k) {
        const float4 s = planes[(size_t)k * plane + oi];
        const uint32_t iteration = first + k;
        if (!mark[(size_t)k * plane + oi]) {
            acc = s;
        } else {
            float r0 = s.x, r1 = s.y, r2 = s.z;
            VR_PT_RUNNING_MEAN(acc, iteration);
            acc = make_float4(r0, r1, r2, 1.f);
        }
    }
    fr.fb[fi] = acc;
    if (out) out[oi] = acc;
}

template <typename VT, int INSTR, bool SAMPLES = false>
hipError_t launch_pt(const RaycastLaunch &a, hipStream_t stream)
{
    auto k = vr_pathtrace_kernel<VT, INSTR, SAMPLES>;
    const size_t lds = (size_t)a.tf.tff_n * sizeof(float4);
    int nb = 0;
    {
        hipError_t e = vr_prepare_kernel(k, kBlockDim, lds, &nb, "pathtrace", a.num_cus);
        if (e != hipSuccess) return e;
    }
    const uint32_t cus = (uint32_t)(a.num_cus > 0 ? a.num_cus : 256);
    const uint32_t want = (a.frame.n_wave_tiles + 3u) / 4u;
    const uint32_t cap = cus * (uint32_t)nb;
    dim3 grid(want < cap ? want : cap), block(kBlockDim);
    if (grid.x == 0) return hipSuccess;
    // (a set of samples ends with its fold: that launch carries the set's end, the event between the two is the phases')
    return vr_launch_bound(
        a, stream, SAMPLES,
        [&](hipEvent_t start, hipEvent_t stop) {
            vr_launch_kernel(k, grid, block, lds, stream, start, stop, a.vol, a.tf, a.cells, a.frame, a.cam, a.render,
                             a.pathtrace, a.stats, a.touched);
        },
        [&](hipEvent_t stop) {
            const uint32_t n = a.frame.set_frames, n_patches = a.frame.n_wave_tiles / n;
            vr_launch_kernel(vr_pt_fold_kernel, dim3((n_patches + kBlockDim / 64u - 1u) / (kBlockDim / 64u)), block, 0, stream,
                             nullptr, stop, a.frame, (const float4 *)a.frame.out, (const uint8_t *)a.frame.sample_mark, n,
                             a.sample_plane, a.render.iteration, a.fold_out);
        });
}

#ifdef VR_STAMPS
} // namespace
extern "C" int vrhip_debug_pt_stamps(unsigned long long out[16], int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pt_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_pt_stamps), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
namespace {
#endif

template <typename VT>
hipError_t launch_pt_typed(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.instr == 0) return launch_pt<VT, 0>(a, stream);
    if (a.instr == 1) return launch_pt<VT, 1>(a, stream);
    if (a.instr == 3) return launch_pt<VT, 3>(a, stream);
    return launch_pt<VT, 2>(a, stream);
}

// a set of samples: production and stats builds (the touched-bitmap variants count one frame's traffic)
template <typename VT>
hipError_t launch_pt_samples(const RaycastLaunch &a, hipStream_t stream)
{
    if (!a.frame.out || !a.frame.sample_mark || !a.frame.seeds || !a.frame.set_frames || !a.sample_plane ||
        a.frame.n_wave_tiles % a.frame.set_frames)
        return hipErrorInvalidValue;
    if (a.instr == 0) return launch_pt<VT, 0, true>(a, stream);
    if (a.instr == 1) return launch_pt<VT, 1, true>(a, stream);
    return hipErrorInvalidValue;
}

} // namespace

hipError_t vr_launch_pathtrace(const RaycastLaunch &a, hipStream_t stream)
{
    if (a.info) {
        a.info->technique = 1;
        a.info->work_items = a.frame.n_wave_tiles;
        a.info->instrumented = (uint32_t)a.instr;
        a.info->samples = a.samples ? 1u : 0u;
    }
    // (two dispatches, not one that branches inside: the kernels keep their order in the code object)
    if (a.samples)
        return vr_for_format(a.format, [&](auto vt) { return launch_pt_samples<typename decltype(vt)::type>(a, stream); });
    return vr_for_format(a.format, [&](auto vt) { return launch_pt_typed<typename decltype(vt)::type>(a, stream); });
}

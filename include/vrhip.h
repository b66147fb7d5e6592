/*
 * vrhip.h -- C ABI of the MI355X-native volume ray-caster (libvrhip.so).
 *
 * This is the drop-in boundary underneath the reference's C++ class
 * `VolumeRenderCL` (/root/reference/src/core/volumerendercl.h:39-482): every entry
 * point below replaces one OpenCL-side action of that class and cites it.  Plain
 * pointers and sizes only; no C++/torch types.  All functions return VRHIP_OK (0)
 * or an error code; vrhip_last_error() gives the message (the host class turns it
 * into the std::runtime_error the reference throws, volumerendercl.cpp:83-89).
 *
 * Not thread-safe per renderer (like the reference's single in-order queue,
 * volumerendercl.cpp:140).  One renderer == one GPU.
 */
#ifndef VRHIP_H
#define VRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRHIP_ABI_VERSION 1

enum vrhip_status {
    VRHIP_OK = 0,
    VRHIP_ERR_INVALID = 1,     /* bad argument (reference: std::invalid_argument)          */
    VRHIP_ERR_HIP = 2,         /* HIP runtime failure (reference: cl::Error -> runtime_error) */
    VRHIP_ERR_NODATA = 3,      /* no volume / TF / bricks yet                               */
    VRHIP_ERR_UNSUPPORTED = 4  /* feature outside the hot path                  */
};

/* DatRawReader::data_format, src/io/datrawreader.h:41-48 */
enum vrhip_format { VRHIP_UCHAR = 0, VRHIP_USHORT = 1, VRHIP_FLOAT = 2 };

/* Kernel-argument structs: byte-identical to the reference's
 * camera_params / rendering_params / raycast_params / pathtrace_params
 * (src/core/volumerendercl.h:43-81 == src/kernel/volumeraycast.cl:540-582). */
typedef struct vrhip_camera_params {
    float viewMat[16];   /* row-major 4x4 (updateView, volumerendercl.cpp:379-390) */
    float bbox_bl[4];    /* cl_float3 in a 16-byte slot */
    float bbox_tr[4];
    uint32_t ortho;
    uint32_t _pad[7];
} vrhip_camera_params;   /* 128 bytes */

typedef struct vrhip_rendering_params {
    float backgroundColor[4];
    float modelScale[4]; /* cl_float3 in a 16-byte slot */
    uint32_t illumType;  /* 0 off, 1 central differences, 2 TF-opacity differences, 3 Sobel,
                            4 gradient magnitude through the TF, 5 cel (volumeraycast.cl:796-830) */
    uint32_t imgEss;
    uint32_t showEss;
    uint32_t useLinear;
    uint32_t useGradient;
    uint32_t technique;  /* 0 ray cast, 1 path tracing, 2 maximum intensity projection (VRHIP_TECHNIQUE_MIP),
                            4 first-hit isosurface (VRHIP_TECHNIQUE_ISO), 6 two-dimensional transfer function
                            (VRHIP_TECHNIQUE_TF2D), 8 pre-integrated classification (VRHIP_TECHNIQUE_PREINT);
                            3, 5 and 7 are unassigned and rejected */
    uint32_t seed;
    uint32_t iteration;
} vrhip_rendering_params; /* 64 bytes */

/* rendering_params.technique == 2: maximum intensity projection (no reference counterpart; DESIGN.md "Maximum
 * intensity projection").
 *  Ray: exactly technique 0's -- view matrix, ortho switch, bbox_bl / bbox_tr, step length from samplingRate, start
 *   jitter from the seed -- and technique 0's sample positions with object-order ESS off: t_0 = max(0, tnear),
 *   t_{k+1} = t_k + stepSize while t_k < tfar (a step that no longer changes t ends the sequence).
 *  Value: m = the maximum over those samples of the normalised, filtered channel-0 value (useLinear: trilinear or
 *   nearest); a sample replaces m only when s > m, so a NaN sample never does; m starts at -inf.
 *  Pixel: c = TF(m), the transfer-function read of the ray caster, no opacity correction, no shading;
 *   rgb = c.rgb * c.a + bg.rgb * (1 - c.a), a = c.a + bg.a * (1 - c.a), bg = backgroundColor, every product and sum
 *   one rounded fp32 operation in this order.  A ray that misses the box or takes no sample: bg unchanged.
 *  Ignored: illumType, useGradient, contours, aerial.  VRHIP_ERR_UNSUPPORTED: imgEss, showEss, useAO, iteration > 0,
 *   RG / RGBA volumes, a set environment map, vrhip_render_samples, vrhip_count_touched*, vrhip_count_fetched.
 *  vrhip_set_object_ess: on, samples that provably cannot raise m are not fetched (cell grid, vrhip_download_cells);
 *   no pixel changes.  Needs neither ESS bricks nor the prefix sum.  vrhip_get_stats: zeros. */
#define VRHIP_TECHNIQUE_MIP 2u

/* rendering_params.technique == 4: first-hit isosurface rendering (no reference counterpart; DESIGN.md "First-hit
 * isosurface").  The value 3 is unassigned: it answers "Unknown rendering technique." like every other value.
 *  Parameters: vrhip_iso_params below (vrhip_set_iso_params), since rendering_params mirrors the reference's layout.
 *   isoValue is in the units of the transfer function's coordinate: the normalised channel-0 value for UCHAR and
 *   USHORT volumes, the raw value for FLOAT.  Defaults: isoValue 0.5, refineSteps 4.  A non-finite isoValue or
 *   refineSteps > 16: VRHIP_ERR_INVALID from the render calls while technique 4 is selected.
 *  Ray: exactly technique 0's with object-order ESS off, as for technique 2: t_0 = max(0, tnear),
 *   t_{k+1} = t_k + stepSize while t_k < tfar, sample k at cam + dir * (t_k - offset); a step that no longer changes t
 *   ends the sequence.
 *  Hit: the first k whose normalised, filtered channel-0 value (useLinear: trilinear or nearest) satisfies
 *   s_k >= isoValue.  A NaN sample never hits.  A ray that starts inside the solid hits at k = 0: the clip box caps
 *   the surface.
 *  Refinement (skipped when k = 0 or refineSteps = 0): ta = t_{k-1}, tb = t_k; refineSteps times tm = (ta + tb) * 0.5f,
 *   s = the fetch at tm (always taken), s >= isoValue ? tb = tm : ta = tm; then t_hit = tb.  One rounded fp32
 *   operation each.
 *  Pixel: c = TF(isoValue), the transfer-function read of the ray caster; the surface is opaque, c.a is not used.
 *   illumType 0: rgb = c.rgb.  illumType 1: g = the ray caster's negated central-difference gradient at the hit
 *   position, ndl = max(0, g . lgt), spec = hvalid ? powr(max(g . hv, 0), 40) * 0.15 : 0 (lgt, hv, hvalid: the ray
 *   caster's light and half vector), rgb = ((c * 0.15) + ((c * ndl) * 0.7)) + spec per channel, in this order.
 *   a = 1.  A ray that misses the box or finds no hit: backgroundColor unchanged, alpha included.
 *  Ignored: useGradient, contours, aerial.  VRHIP_ERR_UNSUPPORTED: illumType 2-5, imgEss, showEss, useAO,
 *   iteration > 0, RG / RGBA volumes, a set environment map, vrhip_render_samples, vrhip_count_touched*,
 *   vrhip_count_fetched.
 *  vrhip_set_object_ess: on, march samples that provably lie below isoValue are not fetched (cell grid,
 *   vrhip_download_cells); no pixel changes.  Needs neither ESS bricks nor the prefix sum.  vrhip_get_stats: zeros. */
#define VRHIP_TECHNIQUE_ISO 4u

typedef struct vrhip_iso_params {
    float isoValue;
    uint32_t refineSteps;
    uint32_t reserved[2];
} vrhip_iso_params; /* 16 bytes */

/* rendering_params.technique == 6: emission-absorption ray casting through a TWO-DIMENSIONAL transfer function,
 * TF2(value, gradient magnitude) (Kniss et al.; no reference counterpart).  The values 3 and 5 are
 * unassigned: they answer "Unknown rendering technique." like every other value.
 *  Table (vrhip_set_transfer_function_2d): n_v x n_g RGBA8 entries, value fastest: T[j * n_v + i].  1 <= n_v <= 4096,
 *   1 <= n_g <= 256, n_v * n_g <= 65536 -- the limits of the statistics histogram; g_hi finite and > 0: the gradient
 *   magnitude that maps to the upper edge of the table, the same axis as vrhip_stats_params.g_hi.  Texel (i, j) is
 *   the colour at the CENTRE of histogram bin (i, j) of vrhip_volume_statistics called with the window [0, 1],
 *   bins_v = n_v, bins_g = n_g and the same g_hi: a lookup there returns the entry exactly.
 *  Ray: exactly technique 0's with object-order ESS off, as for techniques 2 and 4: t_0 = max(0, tnear), sample k at
 *   cam + dir * (t_k - offset), and the reference's loop: composite sample k; stop when the accumulated alpha, as a
 *   double, exceeds 0.98; t_{k+1} = t_k + stepSize; go on while t_{k+1} < tfar (a step that no longer changes t ends
 *   the sequence).
 *  Sample: s = the filtered, normalised channel-0 value (useLinear: trilinear or nearest; FLOAT: the raw value);
 *   G = s2 - s1, the ray caster's six-tap central difference (texel space, the centre's trilinear weights on indices
 *   shifted by -+1 and clamped to the edge, whatever useLinear says); m = 0.5f * sqrtf((G.x * G.x + G.y * G.y) + G.z *
 *   G.z): at a grid point the m of vrhip_volume_statistics.
 *  Lookup (vrhip_tf2d_lookup is this on the host), coord(x) = x > -1 ? (x < 2 ? x : 2) : -1 (a NaN reads -1):
 *   ub = coord(s) * (float)n_v - 0.5f, fu = floorf(ub), a = ub - fu, i0 = clamp((int)fu, 0, n_v - 1),
 *   i1 = clamp((int)fu + 1, 0, n_v - 1); inv_ghi = 1.0f / g_hi once, y = m * inv_ghi, vb = coord(y) * (float)n_g - 0.5f,
 *   fv = floorf(vb), b = vb - fv, j0, j1 likewise on n_g; per channel e(j, i) = (float)T[j * n_v + i] / 255.0f,
 *   r0 = lerpf(e(j0, i0), e(j0, i1), a), r1 = lerpf(e(j1, i0), e(j1, i1), a), c = lerpf(r0, r1, b), with
 *   lerpf(p, q, w) = fmaf(w, q - p, p).
 *  Shading and compositing: technique 0's lines.  illumType 1 and c.a > 0.1f: c.rgb = ((c * 0.15) + ((c * ndl) * 0.7))
 *   + spec per channel with n = -normalize(G) -- (0.57735, 0.57735, 0.57735) negated when G == 0 -- from the taps that
 *   gave m, ndl = max(0, n . lgt), spec = hvalid ? powr(max(n . hv, 0), 40) * 0.15 : 0.  Then x = bg.rgb - c.rgb,
 *   opacity = 1 - powr(1 - c.a, 1 / samplingRate), result.rgb -= (x * opacity) * (1 - alpha), alpha += opacity *
 *   (1 - alpha), from result = bg = backgroundColor and alpha = 0.  Pixel: (result.rgb, alpha), the accumulated alpha
 *   (as the ray caster reports it).  A ray that misses the box: backgroundColor unchanged, alpha included.
 *  Ignored: useGradient, contours, aerial, the 1-D transfer function and its prefix sum (neither read nor required).
 *   VRHIP_ERR_UNSUPPORTED: illumType 2-5, imgEss, showEss, useAO, iteration > 0, RG / RGBA volumes, a set environment
 *   map, vrhip_render_samples, vrhip_count_touched*, vrhip_count_fetched.  VRHIP_ERR_NODATA "No 2-D transfer function
 *   set." from the render calls while technique 6 is selected and none is.
 *  Cost: a sample whose value can only read table columns that are transparent in every row takes neither the
 *   gradient nor the lookup; vrhip_set_object_ess: on, samples whose cell of the cell grid (vrhip_download_cells)
 *   proves that are not fetched at all.  No bit of a pixel changes either way (backgroundColor finite).  Needs neither
 *   ESS bricks nor the prefix sum.
 *  vrhip_get_stats (vrhip_set_stats_enabled): samples_taken = values fetched, samples_shaded = gradient evaluations,
 *   bricks_skipped = samples stepped over by the cell bound, rays_hit = rays with alpha > 0; the rest 0.
 *  State: the 2-D table is state of its own.  Setting it touches nothing a technique 0-4 frame, a slice, depth, mesh,
 *   statistics or filter call reads; vrhip_set_transfer_function does not touch it. */
#define VRHIP_TECHNIQUE_TF2D 6u
#define VRHIP_TF2D_MAX_NV 4096u
#define VRHIP_TF2D_MAX_NG 256u
#define VRHIP_TF2D_MAX_ENTRIES 65536u

/* rendering_params.technique == 8: emission-absorption ray casting with PRE-INTEGRATED classification (Engel, Kraus,
 * Ertl 2001, by integral functions; no reference counterpart).  Techniques 0 and 6 classify a ray by
 * point samples and never see what the transfer function does between two of them; this one classifies the SLAB
 * between two consecutive samples by the transfer function integrated over the values in between, so a narrow peak
 * that the data crosses between two samples is always seen.  No new parameters: it reads the 1-D transfer function of
 * vrhip_set_transfer_function.  The values 3, 5 and 7 are unassigned: "Unknown rendering technique.".
 *  Ray: exactly technique 0's with object-order ESS off, as for technique 6: t_0 = max(0, tnear), sample k at
 *   cam + dir * (t_k - offset); composite slab k; stop when the accumulated alpha >= 0.98f; t_{k+1} = t_k + stepSize;
 *   go on while t_{k+1} < tfar (a step that no longer changes t ends the sequence).
 *  Sample value: s_k = the filtered, normalised channel-0 value (useLinear: trilinear or nearest; FLOAT: the raw
 *   value); its table coordinate u_k = coord(s_k) * (float)n - 0.5f, fp32, with coord(x) = x for UCHAR / USHORT and
 *   x > -1 ? (x < 2 ? x : 2) : -1 for FLOAT (a NaN reads -1): the ray caster's read.  Entry i of the n-entry table
 *   E (c / 255.0f) sits at u = i.
 *  c(u): the ray caster's read as a function of a real u -- linear on every segment j = [j, j + 1], 0 <= j <= n - 2,
 *   between E[j] and E[j + 1]; constant E[0] on the tail (-inf, 0] (segment -1) and E[n - 1] on [n - 1, +inf)
 *   (segment n - 1).  Segment j has the end entries p = E[clamp(j, 0, n - 1)], q = E[clamp(j + 1, 0, n - 1)].
 *  Slab k: uf = u_{k-1}, ub = u_k; for k = 0 uf = ub.
 *   uf == ub (fp32 compare): the slab's colour IS the ray caster's read at s_k: fu = floorf(ub), a = ub - fu,
 *    lerpf(E[i0], E[i1], a) per channel with i0 = clamp((int)fu, 0, n - 1), i1 = clamp((int)fu + 1, 0, n - 1),
 *    lerpf(p, q, w) = fmaf(w, q - p, p).  A volume that is constant along a ray renders technique 0's pixel bit for
 *    bit.
 *   else, with lo = min(uf, ub), hi = max(uf, ub): abar = the mean of c.a over [lo, hi]; Cbar = the mean of
 *    c.rgb * c.a over [lo, hi] divided by abar -- the opacity-weighted colour -- and 0 where abar is 0.
 *   Self-attenuation INSIDE a slab is not modelled (the paper's approximation by integral functions; the full 2-D
 *   table depends on the step length): a slab that crosses a peak of opacity 1 gets the peak's share of the value
 *   interval as its opacity, not 1.
 *  Arithmetic of the means, ONE evaluation order, in double until stated otherwise (each operation rounded on its own,
 *   no contraction).  part(j, u0, u1), the integral over [u0, u1] inside segment j: h = u1 - u0; on a tail w0 = w1 = 0,
 *   else w0 = u0 - j, w1 = u1 - j; wm = 0.5 * (w0 + w1); v = 1 - w for each; a(w) = p.a * v + q.a * w,
 *   c(w) = p.c * v + q.c * w per colour channel;
 *     A = h * a(wm);   M_c = (h * (1.0 / 6.0)) * ((c(w0) * a(w0) + 4.0 * (c(wm) * a(wm))) + c(w1) * a(w1))
 *   (midpoint and Simpson's rule: exact for the linear and the quadratic integrand).  Prefix table, n entries of four
 *   doubles: P[0] = 0, P[i] = P[i - 1] + part(i - 1, i - 1, i).  jl = clamp((int)floorf(lo), -1, n - 1), jh likewise:
 *     jl == jh: S = part(jl, lo, hi)         -- an interval inside one segment is the closed form alone; two nearly
 *                                               equal prefix values are never subtracted to get a short interval
 *     else:     S = (part(jl, lo, jl + 1) + (P[jh] - P[jl + 1])) + part(jh, jh, hi)   per component
 *   r = 1.0 / (hi - lo); abar = (float)(S.A * r), m_c = (float)(S.M_c * r); from here fp32: Cbar_c = abar > 0 ?
 *   m_c / abar : 0.  Every term is a sum of products of non-negative numbers, so an interval over which every entry
 *   that c reads (clamp(jl, 0, n - 1) .. clamp(jh + 1, 0, n - 1)) has alpha 0 gives abar = +0 EXACTLY, whatever the
 *   colours: leaving such slabs out rests on it.
 *  Shading and compositing: technique 0's lines on (Cbar, abar).  illumType 1 and abar > 0.1f: C = ((C * 0.15) +
 *   ((C * ndl) * 0.7)) + spec per channel with the ray caster's central-difference normal at sample k's position
 *   (technique 6's wording).  opacity = 1 - powr(1 - abar, 1 / samplingRate), result.rgb -= ((bg.rgb - C) * opacity)
 *   * (1 - alpha), alpha += opacity * (1 - alpha), from result = bg = backgroundColor and alpha = 0.  Pixel:
 *   (result.rgb, alpha).  A ray that misses the box: backgroundColor unchanged, alpha included.
 *  Ignored: useGradient, contours, aerial, the prefix sum of vrhip_set_tff_prefix_sum (not required).
 *   VRHIP_ERR_UNSUPPORTED: illumType 2-5, imgEss, showEss, useAO, iteration > 0, RG / RGBA volumes, a set environment
 *   map, vrhip_render_samples, vrhip_count_touched*, vrhip_count_fetched.  VRHIP_ERR_NODATA "No transfer function
 *   set." while none is.
 *  Cost: a slab that can only read transparent entries is neither classified nor composited; vrhip_set_object_ess: on,
 *   a sample is not fetched when the cell grid (vrhip_download_cells) proves the slab before it and the slab after it
 *   transparent: both of a slab's cells have usable bounds and the HULL of their two value ranges reads transparent
 *   entries only (two transparent ranges on either side of a peak do not make a transparent slab).  No bit of a
 *   pixel changes either way (backgroundColor finite).  Needs neither ESS bricks nor the prefix sum.
 *  vrhip_get_stats (vrhip_set_stats_enabled): samples_taken = values fetched, samples_shaded = slabs classified --
 *   those that can read an entry which is not transparent, whether or not their abar turns out 0 --
 *   bricks_skipped = samples stepped over without a fetch, rays_hit = rays with alpha > 0; the rest 0.
 *  State: the integral table and the prefix count are made on the host from the 1-D table when a technique-8 frame
 *   first needs them after vrhip_set_transfer_function, and read by technique 8 alone.  Selecting the technique or
 *   building them touches nothing that any other technique, a slice, depth, mesh, statistics or filter call reads --
 *   with the one exception every frame of every technique shares: the renderer has ONE frame buffer, which a frame
 *   overwrites and which technique 0 at iteration k > 0 accumulates onto.  A progressive accumulation that is
 *   started after a technique-8 frame is unchanged bit for bit; one that CONTINUES across a technique-8 frame (or a
 *   technique 2, 4 or 6 frame) accumulates onto that frame.  Restart it (iteration 0), as the C++ and Python
 *   setTechnique do. */
#define VRHIP_TECHNIQUE_PREINT 8u
#define VRHIP_PREINT_MAX_ENTRIES 4096u   /* the limit of vrhip_set_transfer_function */

typedef struct vrhip_raycast_params {
    float samplingRate;
    uint32_t useAO;
    uint32_t contours;
    uint32_t aerial;
    float brickRes[4];   /* volume_res / brick_edge; written by vrhip_build_bricks */
} vrhip_raycast_params;  /* 32 bytes */

typedef struct vrhip_pathtrace_params {
    float max_extinction;
} vrhip_pathtrace_params;

/* Work counters of the last instrumented render (SURVEY 8d "sample" definitions).
 * technique 0: samples = executions of the inner loop body (volumeraycast.cl:790-880), bricks =
 * DDA steps / steps skipped by ESS.  technique 1: samples_taken = tracking steps inside the
 * volume (sample_interaction :419-431); the two brick counters are reused for the opacity-bound
 * culling: bricks_visited = steps whose bound was consulted (their cell's or, in a leap, their
 * macro cell's), bricks_skipped = steps whose voxel fetch was skipped, samples_nominal = those of
 * them that were taken in leaps over a macro cell; samples_shaded stays 0. */
typedef struct vrhip_stats {
    uint64_t samples_taken;
    uint64_t samples_nominal;
    uint64_t samples_shaded;
    uint64_t bricks_visited;
    uint64_t bricks_skipped;
    uint64_t rays_hit;
} vrhip_stats;

typedef struct vrhip_renderer vrhip_renderer;

/* ---- life cycle: VolumeRenderCL::initialize (volumerendercl.cpp:95-159) -------- */
int vrhip_abi_version(void);
int vrhip_create(int device_id, vrhip_renderer **out);
void vrhip_destroy(vrhip_renderer *r);
/* message of the last failing call on `r` (or of vrhip_create when r == NULL) */
const char *vrhip_last_error(const vrhip_renderer *r);
/* getCurrentDeviceName (volumerendercl.cpp:1114-1117) */
int vrhip_device_name(const vrhip_renderer *r, char *buf, size_t buf_len);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream; NULL is the legacy
 * default stream) instead of the renderer's own stream; use_own != 0 restores the latter. */
int vrhip_set_stream(vrhip_renderer *r, void *hip_stream, int use_own);
/* The hipStream_t the renderer launches on right now (its own stream unless vrhip_set_stream
 * gave it another): render calls return without synchronising, so whoever consumes a frame on
 * another stream (a collective, a copy) orders that stream behind this one. */
int vrhip_get_stream(const vrhip_renderer *r, void **hip_stream);

/* ---- volume: volDataToCLmem (volumerendercl.cpp:690-759) ----------------------- */
/* Dense x-fastest scalar field (CL_R image) of `format`, host memory. */
int vrhip_upload_volume(vrhip_renderer *r, const void *host_voxels, const uint32_t res[3],
                        int format, uint32_t timestep);
/* CL_RG / CL_RGBA volumes (volumerendercl.cpp:697-705; kernel volumeraycast.cl:838-855):
 * `channels` interleaved values of `format` per voxel, 2 = RG (colour (r,0,0), opacity TF(|g|)),
 * 4 = RGBA (the voxel is the sample's colour and opacity), 1 = vrhip_upload_volume.  Everything
 * that reads `.x` in the reference -- bricks, gradients, the path tracer, down-sampling -- sees
 * channel 0.  Other counts: VRHIP_ERR_INVALID ("Unknown or invalid volume color format."). */
int vrhip_upload_volume_channels(vrhip_renderer *r, const void *host_voxels, const uint32_t res[3],
                                 int format, int channels, uint32_t timestep);
/* Same, source already in device memory (HBM). */
int vrhip_upload_volume_device(vrhip_renderer *r, const void *dev_voxels, const uint32_t res[3],
                               int format, uint32_t timestep);
/* Synthetic inputs of SURVEY 8(d), generated on the GPU: kind 0 sphere, 1 shells. */
int vrhip_synth_volume(vrhip_renderer *r, int kind, const uint32_t res[3], int format,
                       uint32_t timestep);
/* Device-side ingest: the bytes of a .raw file as they are (`raw`, host memory) become time step `timestep`
 * with everything the host loader does per voxel (DatRawReader::read_raw) done in HBM, bit for bit
 * the loader's: the maximum over every whole word of the file (FLOAT words byte-swapped first when
 * big_endian, USHORT words compared unswapped whatever the endianness, as the reference does), USHORT
 * stretched by 65535.f / max and stored byte-swapped for big-endian files, FLOAT divided by the maximum, and
 * the 256-bin histogram.  `raw` is uploaded slab by slab through a bounded staging buffer (environment
 * variable VRHIP_INGEST_SLAB_BYTES, read by vrhip_create: rounded down to whole multiples of 4 slices, at
 * least 4; default 256 MiB; no effect on any stored byte), de-interleaved on the device for `channels` = 2
 * or 4, re-tiled raw, then converted in place.  hist: the loader's counts, over every scalar of every channel;
 * *max_value: the loader's Properties::max_value (255 for UCHAR).  Bytes beyond res[0] * res[1] * res[2] *
 * bytes per value * channels are not stored but do enter the maximum and the histogram (the loader's loops
 * run over the whole file); fewer bytes: VRHIP_ERR_INVALID ("Volume size does not match size specified in
 * dat file.").  A USHORT step of zeros only: the loader multiplies 0 by 65535 / FLT_MIN = inf and converts
 * the NaN to an integer, which C++ leaves undefined; here the zeros stay zeros and are counted in bin 0. */
int vrhip_ingest_raw(vrhip_renderer *r, const void *raw, size_t bytes, const uint32_t res[3], int format,
                     int channels, int big_endian, uint32_t timestep, double hist[256], float *max_value);
/* The loader's binning applied to the STORED values of time step `timestep`, however it got there (synthetic,
 * device or host upload, ingest), every channel; nothing is converted: UCHAR bin = the byte, USHORT
 * bin = value / 256, FLOAT bin = round(value * 255) if that lies in [0, 255], else 255.  For a step ingested
 * from little-endian data this is the histogram vrhip_ingest_raw returned. */
int vrhip_volume_histogram(vrhip_renderer *r, uint32_t timestep, double hist[256]);
/* HIP-event seconds of the kernels of the last vrhip_ingest_raw (the host-to-device copies between them
 * excluded), like vrhip_last_bricks_seconds. */
double vrhip_last_ingest_seconds(const vrhip_renderer *r);
/* Copy timestep `t` back as a dense x-fastest array (bytes must equal its size). */
int vrhip_download_volume(vrhip_renderer *r, uint32_t timestep, void *host_dst, size_t bytes);
/* volumeDownsampling's device part (volumerendercl.cpp:238-300 + kernel `downsampling`,
 * volumeraycast.cl:966-994): low-res size = ceil(res / factor) per axis; the low-res volume of
 * timestep `t` is copied to host_dst as a dense x-fastest array in the volume's type.  Call with
 * host_dst == NULL to query out_res only.  factor < 2 -> VRHIP_ERR_INVALID ("Factor must be
 * greater or equal 2."); low-res x size < 64 -> VRHIP_ERR_INVALID (the reference's minimum). */
int vrhip_downsample_volume(vrhip_renderer *r, uint32_t timestep, int factor, void *host_dst,
                            size_t bytes, uint32_t out_res[3]);
/* Scheduling of the two-phase march (no effect on any pixel): sample rounds (4 samples each) a ray
 * marches with one lane in phase 1 before it is suspended and resumed with four lanes in phase 2;
 * 0 = single phase.  The default, 10, minimises the time of ONE frame (long rays get the short
 * 4-lane chains early); with several frames in flight (vrhip_share_volumes) latency is hidden by
 * the other frames and the leaner 1-lane march should keep its rays longer: 32 renders the 2048^3
 * headline at 0.38 ms per frame instead of 0.45 (four in flight), but 0.80 instead of 0.70 alone. */
int vrhip_set_round_budget(vrhip_renderer *r, uint32_t rounds);
/* Frames in flight: renderer `r` (same device) renders from `owner`'s voxels and ESS bricks
 * instead of holding copies -- everything else (transfer function, parameters, frame and scratch
 * buffers, footprint volume, stream) is its own, so two renderers on two streams can
 * have one frame each in flight over one 8 GiB volume.  The owner keeps a list of its sharers:
 * when it clears its volumes, is destroyed, or uploads a volume of another size or a new time step,
 * the sharers are detached first (they wait for their streams, drop the borrowed volumes and answer
 * "No volume data is loaded." until they share again); an upload into an existing time step of the
 * same size overwrites the shared voxels in place after the sharers' streams have drained, and the
 * sharers rebuild what they had derived from them (the owner calls vrhip_build_bricks first).  `r`
 * gives the volumes back with vrhip_clear_volumes or by uploading its own.  vrhip_build_bricks on `r`
 * takes the owner's bricks, and on the owner it never moves them: a brick grid is allocated once per
 * time step and rebuilt only after that step's voxels were uploaded again, so transfer-function edits
 * on either renderer are safe. */
int vrhip_share_volumes(vrhip_renderer *r, vrhip_renderer *owner);
int vrhip_clear_volumes(vrhip_renderer *r);
/* setTimestep (volumerendercl.cpp:1167-1174) */
int vrhip_set_timestep(vrhip_renderer *r, uint32_t timestep);
int vrhip_get_resolution(const vrhip_renderer *r, uint32_t res_xyzt[4]);

/* ---- transfer function + ESS bricks: setTransferFunction (volumerendercl.cpp:864-891) */
/* RGBA8 table upload only (:870-876); n_entries <= 4096. */
int vrhip_set_transfer_function(vrhip_renderer *r, const uint8_t *rgba8, uint32_t n_entries);
/* setTffPrefixSum (:898-916) */
int vrhip_set_tff_prefix_sum(vrhip_renderer *r, const uint32_t *prefix, uint32_t n);
/* The 2-D transfer function of technique 6 (VRHIP_TECHNIQUE_TF2D above): n_v * n_g RGBA8 entries, value fastest.
 * VRHIP_ERR_INVALID: a NULL table, or what vrhip_tf2d_params_check refuses.  The table is converted (c / 255.0f) and
 * its per-column opacity summary made on the host here; nothing else of the renderer changes. */
int vrhip_set_transfer_function_2d(vrhip_renderer *r, const uint8_t *rgba8, uint32_t n_v, uint32_t n_g, float g_hi);
/* host only, no renderer: VRHIP_OK, or VRHIP_ERR_INVALID for n_v outside 1..4096, n_g outside 1..256, n_v * n_g above
 * 65536, or a g_hi that is not finite and > 0 */
int vrhip_tf2d_params_check(uint32_t n_v, uint32_t n_g, float g_hi);
/* host only: technique 6's lookup of (s, m) in the table, as stated above, four floats.  VRHIP_ERR_INVALID: a NULL
 * pointer or refused parameters (out_rgba is not written). */
int vrhip_tf2d_lookup(const uint8_t *rgba8, uint32_t n_v, uint32_t n_g, float g_hi, float s, float m, float out_rgba[4]);
/* host only: boundary emphasis from a 1-D table of n_v RGBA8 entries -- the one 2-D table to be had without an
 * editor.  Row j of out_rgba8 (n_v * n_g entries) is the 1-D table with its alpha scaled by the ramp
 *   g_j = (((float)j + 0.5f) * g_hi) / (float)n_g,  w = (g_j - g0) / (g1 - g0),  w_j = w < 0 ? 0 : (w > 1 ? 1 : w),
 *   x = (float)alpha * w_j,  q = floorf(x),  out alpha = (uint8_t)(q + (x - q >= 0.5f ? 1.0f : 0.0f))
 * (fp32, each operation rounded on its own; x - q is exact: round to nearest, ties away from zero).  rgb is copied.
 * VRHIP_ERR_INVALID: a NULL pointer, refused n_v / n_g / g_hi, g0 or g1 not finite, g0 < 0 or g1 <= g0. */
int vrhip_tf2d_build_ramp(const uint8_t *tf1d_rgba8, uint32_t n_v, uint32_t n_g, float g_hi, float g0, float g1,
                          uint8_t *out_rgba8);
/* Technique 8 (VRHIP_TECHNIQUE_PREINT above) on the host: no renderer, no device.
 * vrhip_preint_slab: the slab classification of the n-entry table tff_rgba (4 n floats in [0, 1], the renderer's
 * c / 255.0f) between the sample values sf (front, s_{k-1}) and sb (back, s_k): out = (Cbar.rgb, abar), the device's
 * result bit for bit.  raw != 0: FLOAT-volume values (any float, NaN included); raw == 0: normalised values, which
 * must lie in [-1, 2].  VRHIP_ERR_INVALID: a NULL pointer, n outside 1..4096, an entry outside [0, 1] or a refused
 * value (out is not written).  It builds the tables on every call.
 * vrhip_preint_tables: what the renderer uploads -- prefix: the n x 4 doubles P above; nz: n + 1 words, nz[i] = the
 * number of entries i' < i with alpha != 0 (entries i0..i1 all transparent <=> nz[i1 + 1] == nz[i0]). */
int vrhip_preint_slab(const float *tff_rgba, uint32_t n, int raw, float sf, float sb, float out[4]);
int vrhip_preint_tables(const float *tff_rgba, uint32_t n, double *prefix, uint32_t *nz);
/* generateBricks host part + kernel for every timestep (:614-684, volumeraycast.cl:932-961);
 * also stores raycast.brickRes like :627-631. */
int vrhip_build_bricks(vrhip_renderer *r);
int vrhip_get_brick_info(const vrhip_renderer *r, uint32_t tex[3], float brick_res[3],
                         uint32_t edge[3]);
/* (min,max) pairs in the volume's own type, x-fastest; for tests. */
int vrhip_download_bricks(vrhip_renderer *r, uint32_t timestep, void *host_dst, size_t bytes);
double vrhip_last_bricks_seconds(const vrhip_renderer *r);

/* ---- kernel arguments: setCameraArgs/.. (volumerendercl.cpp:406-449) ----------- */
int vrhip_set_camera_params(vrhip_renderer *r, const vrhip_camera_params *p);
int vrhip_set_rendering_params(vrhip_renderer *r, const vrhip_rendering_params *p);
int vrhip_set_raycast_params(vrhip_renderer *r, const vrhip_raycast_params *p);
int vrhip_set_pathtrace_params(vrhip_renderer *r, const vrhip_pathtrace_params *p);
/* technique 4 (VRHIP_TECHNIQUE_ISO above); stored as given, checked by the render calls */
int vrhip_set_iso_params(vrhip_renderer *r, const vrhip_iso_params *p);
/* setObjEss (volumerendercl.cpp:1006-1019): the reference recompiles with/without -DESS;
 * here it selects the kernel variant. Default on (:150). */
int vrhip_set_object_ess(vrhip_renderer *r, int enabled);

/* ---- render: runRaycast / runRaycastNoGL (volumerendercl.cpp:506-607) ---------- */
/* Renders the whole width x height frame (launch grid padded like :513-514).
 * out_rgba: width*height*4 floats, row 0 = top, or NULL to keep the frame on the GPU.
 * out_is_device != 0: out_rgba is device memory. */
int vrhip_render_frame(vrhip_renderer *r, uint32_t width, uint32_t height, float *out_rgba,
                       int out_is_device);
/* Image-tile decomposition for multi-GPU: renders n_tiles tiles of
 * tile_w x tile_h pixels (tile id = ty * ceil(width/tile_w) + tx) into the compact
 * DEVICE buffer out_tiles[n_tiles][tile_h][tile_w][4].  Pixels outside the frame are
 * left untouched.  tile_w, tile_h must be multiples of 16. */
int vrhip_render_tiles(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                       uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                       float *out_tiles_dev);
/* ---- slice views: oblique planes and thick slabs through the voxels (no reference counterpart; DESIGN.md "Slice
 * views").  An entry point of its own, not a technique: it casts no ray and reads no camera.
 *  All arithmetic is fp32, every operation below rounded on its own, in the order written.
 *  Pixel position: pixel (gx, gy) of a width x height image, row 0 at the top:
 *   sx = (2.f * ((float)gx + 0.5f)) / (float)W - 1.f,  sy = 1.f - (2.f * ((float)gy + 0.5f)) / (float)H,
 *   p = (origin + sx * u) + sy * v per component, in box space: the volume is [-1, 1]^3.
 *  Samples: k = 0 .. N - 1: a_k = ((float)k + 0.5f) / (float)N - 0.5f, q_k = p + a_k * w, tex = q_k * 0.5f + 0.5f.
 *   A sample is TAKEN when 0 <= tex <= 1 holds for all three components (a NaN fails).  Its value s_k is the
 *   normalised, filtered channel-0 value at tex of the current time step, exactly what techniques 2 and 4 see
 *   (useLinear: trilinear, clamp to edge; else nearest).
 *  Reduction over the taken samples, in order of k: VRHIP_SLICE_MAX `s > m ? s : m` from -inf, VRHIP_SLICE_MIN
 *   `s < m ? s : m` from +inf (a NaN never replaces either), VRHIP_SLICE_MEAN sum = sum + s from 0.f, then
 *   sum / (float)count.  With N = 1 the three modes give the same bits.
 *  Pixel: no sample taken: backgroundColor, all four components.  VRHIP_SLICE_TF: technique 2's pixel, c = TF(val),
 *   rgb = c.rgb * c.a + bg.rgb * (1 - c.a), a = c.a + bg.a * (1 - c.a).  VRHIP_SLICE_VALUE: (val, val, val, 1), the
 *   data readout; a NaN val is written as the quiet NaN 0x7fc00000 whatever its sign and payload (fp32 arithmetic
 *   defines neither: a NaN pixel does not depend on how the hardware negates or hands on a NaN).
 *  Output: slice i goes to out_rgba + i * W * H * 4: device memory when out_is_device != 0 (16-byte aligned; the
 *   call returns without synchronising), else host memory through a staging buffer the renderer owns (the call
 *   returns after the copy has completed).
 *  State: reads the volume, the time step, the transfer function, useLinear and backgroundColor -- no camera,
 *   technique, illumination, ESS switch, iteration, seed or environment map -- and writes nothing a render entry
 *   point reads later: not the frame buffer, the hit images, the launch sets' control words or
 *   vrhip_last_launch_info.  A slice between two progressive frames does not disturb them.
 *  VRHIP_ERR_INVALID: n_slices == 0, NULL pointers, samples 0 or above VRHIP_SLICE_MAX_SAMPLES, mode > 2,
 *   output > 1, reserved != 0, a non-finite component of origin, u, v or w, a width or height vrhip_render_frame
 *   refuses, more than 2^32 - 1 patches of 8 x 8 pixels in all.  VRHIP_ERR_UNSUPPORTED: RG / RGBA volumes.
 *   VRHIP_ERR_NODATA as from vrhip_render_frame: no volume; no transfer function while a slice has output TF. */
#define VRHIP_SLICE_MAX_SAMPLES 256u
enum { VRHIP_SLICE_MAX = 0, VRHIP_SLICE_MIN = 1, VRHIP_SLICE_MEAN = 2 };   /* mode   */
enum { VRHIP_SLICE_TF = 0, VRHIP_SLICE_VALUE = 1 };                        /* output */
typedef struct vrhip_slice_params {
    float origin[4];   /* image centre in box space: the volume is [-1,1]^3 (texture coordinate = q*0.5+0.5); [3] unused */
    float u[4];        /* image centre -> centre of the right edge  */
    float v[4];        /* image centre -> centre of the top edge    */
    float w[4];        /* slab: from its first to its last face, across the plane; all zero for a thin slice */
    uint32_t samples;  /* N: 1 .. VRHIP_SLICE_MAX_SAMPLES */
    uint32_t mode, output, reserved;   /* reserved must be 0 */
} vrhip_slice_params;   /* 80 bytes */
int vrhip_render_slices(vrhip_renderer *r, uint32_t width, uint32_t height, const vrhip_slice_params *slices,
                        uint32_t n_slices, float *out_rgba, int out_is_device);

/* ---- depth images and picking: where along its ray a pixel's "thing" lies (no reference counterpart; DESIGN.md
 * "Depth images and picking").  An entry point of its own, not a technique: values 3 and 5 of
 * rendering_params.technique stay unassigned.  All arithmetic is fp32, every operation rounded on its own, in the
 * order written.
 *  Ray: exactly technique 0's ray for pixel (gx, gy) of the width x height frame with object-order ESS off, as for
 *   techniques 2 and 4: the renderer's camera, ortho, bbox_bl / bbox_tr, rendering_params.seed (jitter) and
 *   raycast_params.samplingRate.  Samples: t_0 = max(0, tnear), t_{k+1} = t_k + stepSize while t_k < tfar; a step
 *   that no longer changes t ends the sequence.  Sample k sits at cam + dir * (t_k - offset); its value s_k is the
 *   normalised, filtered channel-0 value of the current time step (useLinear: trilinear, else nearest).
 *  Hit, by mode:
 *   VRHIP_DEPTH_ISO: technique 4's hit and refinement, word for word, with isoValue = threshold: the first k with
 *    s_k >= isoValue (a NaN never hits); unless k = 0 or refineSteps = 0, ta = t_{k-1}, tb = t_k, refineSteps times
 *    tm = (ta + tb) * 0.5f, s = the fetch at tm, s >= isoValue ? tb = tm : ta = tm; t = tb.
 *   VRHIP_DEPTH_MAX: m starts at -inf and sample k replaces it only when s_k > m; t is the t_k of the last
 *    replacement, i.e. of the first sample that attains the maximum.  A ray whose samples never replace m (all NaN
 *    or -inf) is NO_HIT.
 *   VRHIP_DEPTH_OPACITY: technique 0's accumulated opacity without the aerial depth cue: c = TF(s_k), the ray
 *    caster's transfer-function read; refInterval = 1.f / samplingRate; opacity = 1.f - powr(1.f - c.a, refInterval)
 *    with the ray caster's powr; alpha = alpha + opacity * (1.f - alpha) from alpha = 0.  The hit is the first k with
 *    alpha >= threshold after sample k's update, t = t_k.  Threshold 0 hits at k = 0; a threshold above 1 never hits.
 *  Outputs, each dense over the w x h rectangle, row 0 at the top; any may be NULL, not all three:
 *   out_xyzt, four floats per pixel.  HIT: d = t - offset, then (cam.x + dir.x * d, cam.y + dir.y * d,
 *    cam.z + dir.z * d, t): the position in box space, the volume being [-1, 1]^3 (texture coordinate = p * 0.5 + 0.5),
 *    and the ray parameter.  NO_HIT and MISS: (0, 0, 0, +inf).
 *   out_aux, one float per pixel.  ISO: the value fetched at t -- the fetch that last answered >= isoValue, sample
 *    k's when nothing was refined.  MAX: m.  OPACITY: alpha where the ray stopped, whether it hit or ran out of
 *    samples.  MISS in any mode, and NO_HIT in ISO: 0.
 *   out_kind, one byte per pixel: VRHIP_DEPTH_MISS when the ray misses the box, else VRHIP_DEPTH_NO_HIT or
 *    VRHIP_DEPTH_HIT.
 *   Host memory goes through a staging block the renderer owns and the call returns after the copy; with
 *   out_is_device != 0 the three pointers are device memory, out_xyzt 16-byte aligned, and the call returns without
 *   synchronising.
 *  vrhip_set_object_ess: on, samples whose outcome is known from the cell grid are not fetched -- ISO and MAX as
 *   techniques 4 and 2, OPACITY samples in cells whose every fetch maps to opacity exactly 0; no output bit changes.
 *  State: reads the volume, the time step, the camera, seed, useLinear, samplingRate and the object-ESS switch, in
 *   OPACITY mode the transfer function -- not the technique, illumination, aerial, imgEss, showEss, useAO, iteration,
 *   vrhip_iso_params or the environment map -- and writes nothing a render entry point reads later: not the frame
 *   buffer, the hit images, the launch sets' control words or vrhip_last_launch_info.
 *  VRHIP_ERR_INVALID: a NULL r or p, all outputs NULL, mode > 2, reserved != 0, a non-finite threshold in ISO or
 *   OPACITY, refineSteps > 16 in ISO, a width or height vrhip_render_frame refuses, a rectangle that is not inside
 *   the frame or has exactly one of w, h zero.  VRHIP_ERR_UNSUPPORTED: RG / RGBA volumes.  VRHIP_ERR_NODATA: no
 *   volume; no transfer function in OPACITY mode. */
enum { VRHIP_DEPTH_ISO = 0, VRHIP_DEPTH_MAX = 1, VRHIP_DEPTH_OPACITY = 2 };   /* mode */
enum { VRHIP_DEPTH_MISS = 0, VRHIP_DEPTH_NO_HIT = 1, VRHIP_DEPTH_HIT = 2 };   /* kind */
typedef struct vrhip_depth_params {
    uint32_t mode;
    float threshold;       /* ISO: isoValue, in the transfer function's coordinate, as vrhip_iso_params.isoValue;
                              OPACITY: the accumulated opacity to reach; MAX: not read */
    uint32_t refineSteps;  /* ISO only, <= 16 */
    uint32_t x0, y0, w, h; /* the rectangle of the width x height frame to answer; w == h == 0: the whole frame */
    uint32_t reserved;     /* must be 0 */
} vrhip_depth_params;      /* 32 bytes */
int vrhip_render_depth(vrhip_renderer *r, uint32_t width, uint32_t height, const vrhip_depth_params *p,
                       float *out_xyzt, float *out_aux, uint8_t *out_kind, int out_is_device);
/* What the last vrhip_render_depth launched: its mode, the 8 x 8 patches of its rectangle, and whether the kernel
 * was handed the cell grid (1) or fetched every sample (0).  VRHIP_ERR_NODATA before the first call. */
typedef struct vrhip_depth_info {
    uint32_t mode, work_items, empty_skip, reserved[5];
} vrhip_depth_info;        /* 32 bytes */
int vrhip_last_depth_info(const vrhip_renderer *r, vrhip_depth_info *out);

/* ---- isosurface extraction: the surface technique 4 draws, as a triangle list (no reference counterpart; DESIGN.md
 * "Isosurface extraction").  An entry point of its own, not a technique.  All arithmetic is fp32, every operation
 * rounded on its own, in the order written.
 *  Grid: the grid points are the voxel centres of channel 0 of the current time step; a point's value is
 *   s = (float)raw * inv_max, the normalised value techniques 2 and 4 filter (FLOAT volumes: the raw value).  A point
 *   is inside when s >= isoValue; a NaN is outside.  A cube is the eight points (x + dx, y + dy, z + dz), its corner
 *   j = dx + 2 dy + 4 dz; a W x H x D volume has (W-1)(H-1)(D-1) cubes, an axis of length 1 gives none (zero
 *   triangles, VRHIP_OK).  The surface is open where it leaves the volume or the region: no caps.
 *  Tetrahedra: every cube is cut into the six tetrahedra of the Kuhn triangulation around the diagonal from corner 0
 *   to corner 7.  Tetrahedron k = 0..5 belongs to the axis order xyz, xzy, yxz, yzx, zxy, zyx; for the order (a, b, c)
 *   its vertices are v0 = (0,0,0), v1 = v0 + e_a, v2 = v1 + e_b, v3 = (1,1,1): the cube corners {0,1,3,7}, {0,1,5,7},
 *   {0,2,3,7}, {0,2,6,7}, {0,4,5,7}, {0,4,6,7}.  The cut is the same in every cube and neighbouring cubes agree on
 *   their shared faces.
 *  Triangles of a tetrahedron, from the inside mask m = sum of (v_i inside) << i; an edge vertex is named by the two
 *   tetrahedron vertices of its edge.  m = 0 or 15: none.  One vertex inside, or one outside: one triangle on the
 *   three edges at that vertex.  Two inside i0 < i1 and two outside o0 < o1: the quad (i0,o0), (i0,o1), (i1,o1),
 *   (i1,o0) as the triangles [(i0,o0), (i0,o1), (i1,o1)] and [(i0,o0), (i1,o1), (i1,o0)].  The first edge vertex of a
 *   triangle is the one named first here (edges at a lone vertex: by ascending other vertex); the other two are
 *   ordered so that the right-hand normal points to the outside vertices.  The table, masks 0..15 from left to right,
 *   triangles of a mask separated by |:
 *   xyz, yzx, zxy (tetrahedra 0, 3, 4):
 *     -, 01 02 03, 01 13 12, 02 03 13|02 13 12, 02 12 23, 01 23 03|01 12 23, 01 13 23|01 23 02, 03 13 23,
 *     03 23 13, 01 02 23|01 23 13, 01 23 12|01 03 23, 02 23 12, 02 12 13|02 13 03, 01 12 13, 01 03 02, -
 *   xzy, yxz, zyx (tetrahedra 1, 2, 5; the mirror images: every triangle above with its last two vertices swapped):
 *     -, 01 03 02, 01 12 13, 02 13 03|02 12 13, 02 23 12, 01 03 23|01 23 12, 01 23 13|01 02 23, 03 23 13,
 *     03 13 23, 01 23 02|01 13 23, 01 12 23|01 23 03, 02 12 23, 02 13 12|02 03 13, 01 13 12, 01 02 03, -
 *  Edge vertex: edge (i, j), i < j, runs from the grid point P = cube corner 0 + v_i to Q = cube corner 0 + v_j, so
 *   Q - P is in {0,1}^3 and P is the end nearer corner 0.  t = (isoValue - sP) / (sQ - sP); if (!(t >= 0.f)) t = 0.f;
 *   if (t > 1.f) t = 1.f; per axis g = (float)P + (float)(Q - P) * t and the box-space coordinate is
 *   (g + 0.5f) / (float)res * 2.f - 1.f -- the volume is [-1, 1]^3, texture coordinate = p * 0.5 + 0.5, as for the
 *   slice views and depth images.  A vertex depends on its edge's two points alone: every tetrahedron and cube that
 *   shares the edge writes the same bits, so the list welds by bit-equality into a watertight mesh.  NaN and
 *   infinite values give finite positions.  Degenerate triangles (a point equal to isoValue) are emitted like any
 *   other: the count depends on the inside masks alone.
 *  Normals (VRHIP_MESH_NORMALS_GRADIENT), per vertex: technique 4's shading normal at the vertex's texture coordinate
 *   (p * 0.5f + 0.5f per axis): the six trilinear taps one texel either side of it, s2 - s1 = g, the normal
 *   -g * (1.f / sqrtf(g . g)), whatever useLinear says.  g . g == 0 or a non-finite component: (0, 0, 0).
 *  Order: cubes are grouped into blocks of VRHIP_MESH_BLOCK^3 cubes anchored at voxel (0,0,0) (not at lo); blocks x
 *   fastest, cubes within a block x fastest, tetrahedra 0..5 within a cube, triangles within a tetrahedron in table
 *   order.  The output is that list, nine floats a triangle, and nothing else; two calls give the same bytes, and a
 *   region's list is the whole volume's with the cubes outside the region removed.
 *  Region: the cubes with lo <= corner 0 and corner 0 + 1 <= hi per axis, in voxels; all six values 0: the whole volume.
 *  vrhip_isosurface_count: the number of triangles.  vrhip_isosurface_extract: writes them when capacity_triangles
 *   is at least that number; else it writes nothing, sets *n_triangles to the number needed and returns
 *   VRHIP_ERR_INVALID.  Host destinations go through staging the renderer owns and the call returns after the copy;
 *   with out_is_device != 0 they are device memory, 16-byte aligned, and the call returns once the count is known and
 *   the last kernel is queued on the renderer's stream.
 *  vrhip_set_object_ess: on, a block whose cell of the cell grid proves every point outside (fl(max * inv_max) <
 *   isoValue) or every point inside (fl(min * inv_max) >= isoValue) is neither fetched nor classified; no output byte
 *   changes.  vrhip_last_mesh_info: the blocks of the last call that hold a cube of the region, how many of them
 *   were skipped so, and whether the cell grid was handed over.
 *  State: reads the volume, the time step and the object-ESS switch -- not the camera, technique, transfer function,
 *   seed, iteration, vrhip_iso_params or the environment map -- and writes nothing a render entry point reads later.
 *  VRHIP_ERR_INVALID: a NULL r, p or n_triangles; normals > 1; reserved != 0; a non-finite isoValue; extract with
 *   out_positions NULL, with out_normals set and normals == 0 or NULL and normals == 1, or with a device destination
 *   that is not 16-byte aligned; a region that is not all zero with hi > res, lo > hi or hi == 0 on an axis.
 *   VRHIP_ERR_UNSUPPORTED: RG / RGBA volumes.  VRHIP_ERR_NODATA: no volume; vrhip_last_mesh_info before the first call. */
#define VRHIP_MESH_BLOCK 8u
enum { VRHIP_MESH_NORMALS_NONE = 0, VRHIP_MESH_NORMALS_GRADIENT = 1 };
typedef struct vrhip_mesh_params {
    float    isoValue;      /* units of vrhip_iso_params.isoValue */
    uint32_t normals;       /* VRHIP_MESH_NORMALS_* */
    uint32_t lo[3], hi[3];  /* region in voxels; all six 0: the whole volume */
    uint32_t reserved[4];   /* must be 0 */
} vrhip_mesh_params;        /* 48 bytes */
int vrhip_isosurface_count(vrhip_renderer *r, const vrhip_mesh_params *p, uint64_t *n_triangles);
int vrhip_isosurface_extract(vrhip_renderer *r, const vrhip_mesh_params *p, float *out_positions,
                             float *out_normals, uint64_t capacity_triangles, uint64_t *n_triangles,
                             int out_is_device);
typedef struct vrhip_mesh_info {
    uint64_t triangles, blocks, blocks_skipped;
    uint32_t empty_skip, reserved;
} vrhip_mesh_info;          /* 32 bytes */
int vrhip_last_mesh_info(const vrhip_renderer *r, vrhip_mesh_info *out);

/* ---- indexed isosurface extraction: the same surface as unique vertices and an index list (DESIGN.md "Indexed
 * isosurface extraction").  vrhip_mesh_params means what it means above -- grid, inside test, tetrahedra, table, edge
 * vertex, normals, region, skipping -- and is checked and refused as there.  fp32, every operation rounded on its own.
 *  Edges: the lattice edges are (P, d), P a grid point and d = dx + 2 dy + 4 dz in 1..7, from P to Q = P + (dx, dy, dz),
 *   Q a point of the volume: exactly the edges of the Kuhn tetrahedra (any two cube corners u, v with u's bits among
 *   v's are an edge of some tetrahedron of that cube), P the end nearer corner 0 as in the edge vertex formula.
 *  Eligible: edge (P, d) is eligible when a cube of the effective region contains it.  The effective region is lo, hi
 *   of the calls above after hi = min(hi, res - 1); on an axis whose bit of d is set lo <= P < hi, on one whose bit
 *   is clear lo <= P <= hi.  A region that holds no cube has no eligible edge.
 *  Crossed: inside(P) != inside(Q), inside being s >= isoValue (a NaN is outside).
 *  Vertices: one per eligible crossed edge and nothing else; its position is the edge vertex formula on (P, Q), its
 *   normal the normals formula at that position.  Identity is the edge, not the float: two edges whose positions are
 *   bit-equal (a grid point equal to isoValue: t = 0 on all of its edges) stay two vertices, where a weld by
 *   bit-equality makes them one.
 *  Vertex order: ascending by the owning point P's block -- blocks of VRHIP_MESH_BLOCK^3 grid points anchored at voxel
 *   (0,0,0), x fastest; per axis there may be one more of them than of the cube blocks (9 points: one cube block, two
 *   point blocks) --, then by the point within the block, x fastest, then by d.
 *  Triangles: the list of vrhip_isosurface_extract, in its order, each triangle's three vertices in its order, each
 *   entry the number of the vertex of the edge that vertex lies on.  out_vertices[out_indices] is that call's
 *   out_positions byte for byte, out_normals[out_indices] its out_normals, and *n_triangles is vrhip_isosurface_count's.
 *  vrhip_isosurface_count_indexed: both numbers.  vrhip_isosurface_extract_indexed: writes three floats a vertex
 *   (and a normal), three 32-bit words a triangle, when both capacities suffice; else it writes nothing to any
 *   destination, sets both counts to the numbers needed and returns VRHIP_ERR_INVALID.  More than 2^32 - 1 vertices:
 *   VRHIP_ERR_UNSUPPORTED from the extraction, the counts set, nothing written.  Host destinations go through
 *   staging the renderer owns and the call returns after the copy; with out_is_device != 0 all of them are device
 *   memory, 16-byte aligned, and the call returns once the counts are known and the last kernel is queued on the
 *   renderer's stream.
 *  vrhip_set_object_ess: on, a point block whose cell of the cell grid proves its points 8 b .. 8 b + 8 all outside or
 *   all inside -- the test and the argument of a cube block, which covers those nine points per axis -- is neither
 *   fetched nor classified; cube blocks are skipped as above; no output byte changes.
 *  vrhip_last_indexed_mesh_info: the last indexed call's counts; the point blocks that own an eligible edge and how
 *   many of them were skipped; the cube blocks as vrhip_mesh_info; scratch_bytes, the device memory an extraction of
 *   that surface holds beyond the destinations (for a count: what the count held; the staging of host destinations
 *   is not in it); whether the cell grid was handed over.
 *  State: two calls give the same bytes.  Reads what the calls above read; writes nothing a render entry point, a
 *   slice, a depth call or vrhip_last_mesh_info reads later.
 *  VRHIP_ERR_INVALID: as above, n_vertices and out_vertices / out_indices in the places of n_triangles and
 *   out_positions.  VRHIP_ERR_UNSUPPORTED: RG / RGBA volumes.  VRHIP_ERR_NODATA: no volume;
 *   vrhip_last_indexed_mesh_info before the first indexed call. */
int vrhip_isosurface_count_indexed(vrhip_renderer *r, const vrhip_mesh_params *p, uint64_t *n_vertices,
                                   uint64_t *n_triangles);
int vrhip_isosurface_extract_indexed(vrhip_renderer *r, const vrhip_mesh_params *p, float *out_vertices,
                                     float *out_normals, uint32_t *out_indices, uint64_t capacity_vertices,
                                     uint64_t capacity_triangles, uint64_t *n_vertices, uint64_t *n_triangles,
                                     int out_is_device);
typedef struct vrhip_indexed_mesh_info {
    uint64_t vertices, triangles;
    uint64_t point_blocks, point_blocks_skipped;
    uint64_t blocks, blocks_skipped;
    uint64_t scratch_bytes;
    uint32_t empty_skip, reserved;
} vrhip_indexed_mesh_info;  /* 64 bytes */
int vrhip_last_indexed_mesh_info(const vrhip_renderer *r, vrhip_indexed_mesh_info *out);

/* ---- volume statistics: counts, moments and the value x gradient-magnitude histogram of a region (DESIGN.md "Volume
 * statistics").  Not a technique: it reads the volume and writes the caller's destinations.  fp32, every operation
 * rounded on its own, no contraction; tests/ref/stats_ref.c restates it on the CPU.
 *  Value: s = (float)raw * inv_max of channel 0 of the current time step (FLOAT: the raw value) -- the grid-point
 *   value of the isosurface extraction, the s techniques 2 and 4 and the slices compare against.
 *  Region: the voxels lo <= v < hi per axis; all six values 0: the whole volume.  lo == hi on an axis: no voxel.
 *  A voxel of the region is classified in this order: a NaN s counts in `nan`; s < v_lo in `below`; s > v_hi in
 *   `above`; else it has the value bin i: k_v = (float)bins_v / (v_hi - v_lo) once, u = (s - v_lo) * k_v,
 *   i = u >= (float)bins_v ? bins_v - 1 : (uint32_t)u (s == v_hi lies in the last bin).
 *  Gradient, for voxels with a value bin and bins_g > 1 (else j = 0): per axis g_a = s(p + e_a) - s(p - e_a), the
 *   neighbour's coordinate clamped to the VOLUME (not the region: histograms of disjoint regions add up), in index
 *   space (slice thickness is ignored); m = 0.5f * sqrtf((gx * gx + gy * gy) + gz * gz).  A NaN m counts in
 *   `gradient_nan` and the voxel is not binned; else k_g = (float)bins_g / g_hi once, w = m * k_g,
 *   j = w >= (float)bins_g ? bins_g - 1 : (uint32_t)w: the top gradient bin is open-ended.
 *  hist[j * bins_v + i] += 1: bins_g * bins_v 64-bit counts, value fastest, written whole (zeros included).
 *   voxels == nan + below + above + gradient_nan + binned, binned == the sum of hist.
 *  Moments (VRHIP_STATS_MOMENTS; without it min, max, sum and sum_sq are 0): min and max over the non-NaN s of the
 *   region, compared with < and >, +inf and -inf where there is none, a zero of either sign reported as +0; sum and
 *   sum_sq of (double)s and (double)s * (double)s over the same voxels, in this order, which is part of the contract:
 *   blocks of VRHIP_MESH_BLOCK^3 voxels anchored at voxel (0,0,0); lane x + 8 y of a block adds the voxels of its
 *   column z = 0..7 ascending, from 0.0 (voxels outside the region and NaNs add nothing); then over the 64 lanes
 *   v += v[lane ^ k] for k = 1, 2, 4, 8, 16, 32; the block sums of the call's block grid (the blocks that hold a
 *   voxel of the region, x fastest) are added from 0.0 in ascending order within chunks of VRHIP_STATS_SUM_CHUNK
 *   consecutive blocks, and the chunk sums from 0.0 in ascending order.  No floating-point atomic anywhere: two calls
 *   give the same bits, whatever the object-ESS switch says.
 *  vrhip_set_object_ess: on, a block whose cell of the cell grid proves the outcome is not fetched.  Constant block
 *   (min == max, finite): every voxel of it in the region has the value bin (or below / above) of fl(min * inv_max)
 *   and gradient bin 0.  Out of window (without VRHIP_STATS_MOMENTS only): fl(max * inv_max) < v_lo or
 *   fl(min * inv_max) > v_hi, every voxel below or above.  With VRHIP_STATS_MOMENTS a constant block is skipped only
 *   where min == max == 0: its block sums are +0.0 and its min and max 0 on either path (n * c is exact in double
 *   for n <= 512, n * c * c is not in general, so other constants are fetched).  A cell with a NaN holds
 *   (-inf, +inf) and proves nothing.  No count and no bit of the output changes with the switch.
 *  hist: host memory, or with hist_is_device != 0 device memory, 16-byte aligned; either way the call returns after
 *   the counts have reached *out, so the histogram is complete then.
 *  vrhip_last_stats_info: the blocks of the last call that hold a voxel of the region, how many were fetched, skipped
 *   as constant and skipped as out of window, whether the cell grid was handed over, which histogram path ran
 *   (VRHIP_STATS_PATH_*: per-workgroup tables in LDS flushed with 64-bit integer atomics, or atomics straight to the
 *   global table) and the scratch the call held in device memory beyond the histogram.
 *  State: reads the volume, the time step and the object-ESS switch; writes nothing a render, slice, depth or mesh
 *   call or their last_*_info reads later.
 *  VRHIP_ERR_INVALID: a NULL r, p, out or hist; bins_v outside 1..4096, bins_g outside 1..256 or their product above
 *   65536; v_lo or v_hi not finite, v_hi <= v_lo, or k_v not finite; bins_g > 1 with g_hi not finite, g_hi <= 0 or
 *   k_g not finite; flags other than VRHIP_STATS_MOMENTS; reserved != 0; a region that is not all zero with hi > res,
 *   lo > hi or hi == 0 on an axis; a device hist that is not 16-byte aligned.  VRHIP_ERR_UNSUPPORTED: RG / RGBA
 *   volumes.  VRHIP_ERR_NODATA: no volume; vrhip_last_stats_info before the first call. */
#define VRHIP_STATS_MOMENTS 1u
#define VRHIP_STATS_SUM_CHUNK 256u
#define VRHIP_STATS_MAX_BINS_V 4096u
#define VRHIP_STATS_MAX_BINS_G 256u
#define VRHIP_STATS_MAX_BINS 65536u
enum { VRHIP_STATS_PATH_LDS = 0, VRHIP_STATS_PATH_GLOBAL = 1 };
typedef struct vrhip_stats_params {
    uint32_t lo[3], hi[3];  /* region in voxels; all six 0: the whole volume */
    uint32_t bins_v, bins_g;
    float    v_lo, v_hi, g_hi;
    uint32_t flags;         /* VRHIP_STATS_MOMENTS */
    uint32_t reserved[4];   /* must be 0 */
} vrhip_stats_params;       /* 64 bytes */
typedef struct vrhip_volume_stats {
    uint64_t voxels, nan, below, above, gradient_nan, binned;
    float    min, max;
    double   sum, sum_sq;
} vrhip_volume_stats;       /* 72 bytes */
int vrhip_volume_statistics(vrhip_renderer *r, const vrhip_stats_params *p, vrhip_volume_stats *out, uint64_t *hist,
                            int hist_is_device);
typedef struct vrhip_stats_info {
    uint64_t blocks, blocks_fetched, blocks_skipped_constant, blocks_skipped_window;
    uint64_t scratch_bytes;
    uint32_t empty_skip, hist_path;
} vrhip_stats_info;         /* 48 bytes */
int vrhip_last_stats_info(const vrhip_renderer *r, vrhip_stats_info *out);
/* the checks of vrhip_volume_statistics that need neither a renderer nor a volume -- bins, window, g_hi, flags,
 * reserved -- for callers that validate before they have a device: VRHIP_OK or VRHIP_ERR_INVALID (a NULL p too) */
int vrhip_stats_params_check(const vrhip_stats_params *p);

/* ---- volume filters: separable smoothing and the 3x3x3 median, computed on the device (DESIGN.md "Volume filters").
 * Not a technique: vrhip_filter_volume reads channel 0 of the CURRENT time step and writes the whole of time step
 * dst_timestep, in the volume's own format and resolution.  fp32, every operation rounded on its own, no contraction;
 * tests/ref/filter_ref.c restates it on the CPU.
 *  Value: s = (float)raw * inv_max (FLOAT: the raw value) -- the s of the statistics and the isosurface extraction.
 *  Neighbours: a neighbour's coordinate is clamped to the volume on each axis.
 *  VRHIP_FILTER_SEPARABLE: three passes on full fp32 fields, x on s gives A, y on A gives B, z on B gives C.  A pass
 *   along axis a with radius R = radius[a] and taps w = taps[a] computes at point p: acc = w[0] * f(p); then for
 *   k = 1 .. R ascending acc = acc + w[k] * (f(p - k e_a) + f(p + k e_a)).  A radius-0 axis still multiplies by w[0].
 *   The taps within the radius must be finite and need not sum to 1; those beyond it are not read.
 *  VRHIP_FILTER_MEDIAN3: the 14th smallest of the 27 clamped neighbours (the voxel included).  UCHAR and USHORT: of
 *   the raw integers, stored as it is.  FLOAT: of the order-preserving 32-bit keys of the raw words -- the sign bit
 *   flipped for words with a clear sign bit, all bits for the others, every NaN mapped to 0xffffffff, above +inf --
 *   and the word of that key is stored.
 *  Store.  FLOAT: C (or the median); a zero of either sign is stored as +0, a NaN as 0x7fc00000.  UCHAR / USHORT,
 *   SEPARABLE: q = C * 255.f (65535.f); q = q > 0.f ? q : 0.f; q = q < 255.f ? q : 255.f (65535.f) -- a NaN, which
 *   only overflowing taps can make, becomes 0 --; the voxel is (integer)rintf(q), round half to even.
 *  Destination: dst_timestep is an existing step (the current one: in place) or the number of steps, which appends
 *   one.  Afterwards it is a step like an uploaded one: its bricks, cells and footprint are stale and
 *   vrhip_build_bricks is due as after an upload; renderers that share this one's volumes are treated as by an upload
 *   (an overwritten step: they drop what they derived; an appended step: they are detached).  In place the result is
 *   written to a scratch of the volume's size and type and then takes the slot's place (swapped in; copied where
 *   other renderers hold the slot's address); it is the only full-size scratch, and it is freed before the call
 *   returns.  No full-size fp32 intermediate exists: the passes run on tiles in LDS.
 *  vrhip_set_object_ess: work goes by blocks of VRHIP_MESH_BLOCK^3 voxels anchored at voxel (0,0,0).  On, a block is
 *   not fetched where the coarse cells that cover the block dilated by radius[a] voxels per axis (by 1 for the median)
 *   and clamped to the volume all hold the same finite min == max == c.  SEPARABLE skips only c == 0: every product
 *   and sum is a zero and a zero is stored as +0 (other constants are fetched: sum(w) * c is not c in fp32).  MEDIAN3
 *   skips any c and stores it (c == 0: +0).  A cell with a NaN holds (-inf, +inf) and proves nothing.  No byte of the
 *   destination changes with the switch.
 *  vrhip_last_filter_info: the blocks of the last call, how many were fetched and skipped, the device scratch the
 *   call held (the in-place copy; 16 bytes of counters), whether the cell grid was handed over, whether it ran in place.
 *  vrhip_filter_gaussian_taps, in double: t_k = exp(-(k * k) / (2 sigma^2)), S = t_0 + 2 * (t_1 + ... + t_R) added in
 *   ascending order, taps[k] = (float)(t_k / S) for k <= radius and 0 above.  A convenience: taps are inputs.
 *  State: reads the volume, the time step and the object-ESS switch.  Nothing that a render, slice, depth, mesh or
 *   statistics call of ANOTHER step reads later changes, beyond what an upload into dst_timestep changes.
 *  VRHIP_ERR_INVALID: a NULL r or p (the tap helper: NULL taps, sigma not finite or <= 0, radius > 8); an unknown
 *   kind; a radius above VRHIP_FILTER_MAX_RADIUS, or a non-zero radius with MEDIAN3; a non-finite tap within the
 *   radius (SEPARABLE); reserved != 0; dst_timestep above the number of steps.  VRHIP_ERR_UNSUPPORTED: RG / RGBA
 *   volumes; a renderer whose volumes are borrowed (vrhip_share_volumes) -- checked before anything is touched.
 *   VRHIP_ERR_NODATA: no volume; vrhip_last_filter_info before the first call. */
#define VRHIP_FILTER_MAX_RADIUS 8u
enum { VRHIP_FILTER_SEPARABLE = 0, VRHIP_FILTER_MEDIAN3 = 1 };
typedef struct vrhip_filter_params {
    uint32_t kind;                                   /* VRHIP_FILTER_* */
    uint32_t radius[3];                              /* SEPARABLE: 0..8 per axis (x, y, z); MEDIAN3: must be 0 */
    float    taps[3][VRHIP_FILTER_MAX_RADIUS + 1];   /* taps[a][k] = weight at distance k on axis a, symmetric */
    uint32_t reserved[4];                            /* must be 0 */
} vrhip_filter_params;                               /* 140 bytes */
int vrhip_filter_volume(vrhip_renderer *r, const vrhip_filter_params *p, uint32_t dst_timestep);
/* the checks of vrhip_filter_volume that need neither a renderer nor a volume -- kind, radii, taps, reserved:
 * VRHIP_OK or VRHIP_ERR_INVALID (a NULL p too) */
int vrhip_filter_params_check(const vrhip_filter_params *p);
int vrhip_filter_gaussian_taps(double sigma, uint32_t radius, float taps[VRHIP_FILTER_MAX_RADIUS + 1]);
typedef struct vrhip_filter_info {
    uint64_t blocks, blocks_fetched, blocks_skipped;
    uint64_t scratch_bytes;
    uint32_t empty_skip, in_place;
} vrhip_filter_info;                                 /* 40 bytes */
int vrhip_last_filter_info(const vrhip_renderer *r, vrhip_filter_info *out);

/* ---- volume morphology: grey-scale erosion, dilation, opening, closing, gradient and the top-hat transforms, computed
 * on the device (DESIGN.md "Volume morphology").  Not a technique: vrhip_morph_volume reads channel 0 of the CURRENT
 * time step and writes the whole of time step dst_timestep, in the volume's own format and resolution.  Minimum and
 * maximum are exact and independent of the order of evaluation; tests/ref/morph_ref.c restates the contract on the CPU.
 *  Structuring element B: the integer offsets (dx, dy, dz) with |d_a| <= R_a = radius[a].  VRHIP_MORPH_BOX takes all
 *   of them; VRHIP_MORPH_BALL those with dx^2 R'y^2 R'z^2 + dy^2 R'x^2 R'z^2 + dz^2 R'x^2 R'y^2 <= R'x^2 R'y^2 R'z^2,
 *   R'_a = max(R_a, 1), in integer arithmetic: radius (1,1,1) is the 6-neighbourhood and the centre, 7 offsets;
 *   (2,2,2) has 33, (4,4,4) 257, (8,8,8) 2109, (2,0,3) 19.  Radius (0,0,0) is the identity element.
 *   vrhip_morph_element lists B as triples (dx, dy, dz), z, then y, then x ascending; *n is the number of offsets
 *   whatever the capacity (in triples), and VRHIP_ERR_INVALID is returned, with nothing written to offsets_xyz, where
 *   it is below *n (offsets_xyz may be NULL with capacity 0).
 *  Keys: UCHAR and USHORT compare the raw integer.  FLOAT compares the order-preserving 32-bit key of the raw word
 *   that the volume filters' median uses -- the sign bit flipped for words with a clear sign bit, all bits for the
 *   others, every NaN mapped to 0xffffffff: every NaN is the largest key.
 *  Erosion at p is the smallest key, dilation the largest, over the clamped positions clamp(p + o), o in B.  B is
 *   symmetric and down-closed in |o|, so these are the voxels p + o that lie inside the volume.
 *  Ops: ERODE; DILATE; OPEN = dilation of the erosion; CLOSE = erosion of the dilation; GRADIENT = dilation - erosion;
 *   TOPHAT = f - OPEN; BLACKHAT = CLOSE - f (f the source).  With this border rule erosion <= open <= f <= close <=
 *   dilation at every voxel, so on UCHAR / USHORT the three differences are plain unsigned subtractions of the raw
 *   integers and never wrap; on FLOAT each is one fp32 subtraction of the two stored words read as floats (for f the
 *   source's raw word).
 *  Store.  UCHAR / USHORT: the integer.  FLOAT: the word of the key, or the difference; a zero of either sign is
 *   stored as +0 and any NaN as 0x7fc00000 (the filters' store).  The intermediate of a two-sweep op is stored by the
 *   same rule and the second sweep reads those stored words.  Voxels of an existing micro-brick beyond the volume are
 *   written 0, as an upload does; no sweep reads them as data.
 *  Sweeps and scratch.  ERODE, DILATE and GRADIENT take one sweep over the blocks of VRHIP_MESH_BLOCK^3 voxels (the
 *   gradient takes both extremes from one staged tile); the others two, through one full-size intermediate in the
 *   volume's own type; the second sweep of TOPHAT / BLACKHAT reads the intermediate for the extreme and the source for
 *   f.  In place the result goes to a scratch that takes the slot's place (swapped in; copied where other renderers
 *   hold the slot's address), except that OPEN / CLOSE in place without sharers write their second sweep straight
 *   into the slot.  Full-size scratches held at once: into another step 0 (one sweep) or 1 (two); in place 1 or 2
 *   (OPEN / CLOSE without sharers: 1).  All of it is freed before the call returns.
 *  Destination, sharers and staleness: as vrhip_filter_volume.  dst_timestep is an existing step (the current one: in
 *   place) or the number of steps, which appends one.  Afterwards it is a step like an uploaded one: its bricks, cells
 *   and footprint are stale and vrhip_build_bricks is due as after an upload; renderers that share this one's volumes
 *   are treated as by an upload.
 *  vrhip_set_object_ess: on, the first sweep does not fetch a block where the coarse cells that cover the block
 *   dilated by R_a voxels per axis and clamped to the volume all hold the same finite min == max == c; the second
 *   sweep asks the same of the block dilated by 2 R_a (the intermediate is then c on everything it reads, and so is
 *   f).  A skipped block is written c for ERODE / DILATE / OPEN / CLOSE and for the intermediate (FLOAT, c == 0: +0)
 *   and 0 for GRADIENT / TOPHAT / BLACKHAT.  A cell with a NaN holds (-inf, +inf) and proves nothing.  No byte of the
 *   destination changes with the switch.
 *  vrhip_last_morph_info: per sweep the blocks, how many were fetched and skipped (sweep[1] is 0 for a one-sweep op);
 *   the sweeps; the device scratch the call held at its peak (full-size scratches and 32 bytes of counters); whether
 *   the cell grid was handed over; whether it ran in place.
 *  State: reads the volume, the time step and the object-ESS switch.  Nothing that a render, slice, depth, mesh,
 *   statistics or filter call of ANOTHER step reads later changes, beyond what an upload into dst_timestep changes.
 *  VRHIP_ERR_INVALID: a NULL argument; an unknown op or shape; a radius above VRHIP_MORPH_MAX_RADIUS; reserved != 0;
 *   dst_timestep above the number of steps.  VRHIP_ERR_UNSUPPORTED: RG / RGBA volumes; a renderer whose volumes are
 *   borrowed (vrhip_share_volumes) -- checked before anything is touched.  VRHIP_ERR_NODATA: no volume;
 *   vrhip_last_morph_info before the first call. */
enum { VRHIP_MORPH_ERODE = 0, VRHIP_MORPH_DILATE = 1, VRHIP_MORPH_OPEN = 2, VRHIP_MORPH_CLOSE = 3,
       VRHIP_MORPH_GRADIENT = 4, VRHIP_MORPH_TOPHAT = 5, VRHIP_MORPH_BLACKHAT = 6 };
enum { VRHIP_MORPH_BOX = 0, VRHIP_MORPH_BALL = 1 };
#define VRHIP_MORPH_MAX_RADIUS 8u
typedef struct vrhip_morph_params {
    uint32_t op, shape;      /* VRHIP_MORPH_* */
    uint32_t radius[3];      /* x, y, z: 0..8 */
    uint32_t reserved[3];    /* must be 0 */
} vrhip_morph_params;                                /* 32 bytes */
int vrhip_morph_volume(vrhip_renderer *r, const vrhip_morph_params *p, uint32_t dst_timestep);
/* the checks of vrhip_morph_volume that need neither a renderer nor a volume -- op, shape, radii, reserved: VRHIP_OK
 * or VRHIP_ERR_INVALID (a NULL p too).  Host only. */
int vrhip_morph_params_check(const vrhip_morph_params *p);
/* the offsets of B, 3 int8 per offset.  Host only. */
int vrhip_morph_element(const vrhip_morph_params *p, int8_t *offsets_xyz, uint32_t capacity, uint32_t *n);
typedef struct vrhip_morph_sweep_info {
    uint64_t blocks, blocks_fetched, blocks_skipped;
} vrhip_morph_sweep_info;                            /* 24 bytes */
typedef struct vrhip_morph_info {
    vrhip_morph_sweep_info sweep[2];
    uint64_t scratch_bytes;
    uint32_t sweeps, empty_skip, in_place, reserved;
} vrhip_morph_info;                                  /* 72 bytes */
int vrhip_last_morph_info(const vrhip_renderer *r, vrhip_morph_info *out);

/* createEnvironmentMap (volumerendercl.cpp:1121-1150): float RGBA texels, row-major, width*height*4
 * floats (the host layer decodes the Radiance .hdr file).  The kernel samples it in place of the
 * background colour when it is wider than one texel (volumeraycast.cl:506-510, :655-656);
 * rgba == NULL or width <= 1 removes it. */
int vrhip_set_environment_map(vrhip_renderer *r, const float *rgba, uint32_t width,
                              uint32_t height);

/* ---- image-order ESS (rendering_params.imgEss; volumeraycast.cl:659-670, :912-925) --------
 * The renderer keeps the reference's two hit images, (width/8 + 1) x (height/8 + 1) texels of one
 * byte, creates them on the first imgEss frame of a size with updateOutputImg's initial contents
 * (volumerendercl.cpp:482-488) and swaps them after every imgEss frame (:524-530).  A tile render
 * only updates the texels of its own 8x8 work-groups: with several GPUs the caller merges the
 * images between frames (get on every rank, exchange, set; volumerenderercl_amd/tiles.py).
 * vrhip_reset_image_ess: what updateOutputImg does to them (re-created on the next frame).
 * get/set: hit_in = the image the next frame reads, hit_out = the one it writes; either may be
 * NULL.  Not supported together with technique 1. */
int vrhip_reset_image_ess(vrhip_renderer *r);
int vrhip_get_image_ess(vrhip_renderer *r, uint32_t width, uint32_t height, uint8_t *hit_in,
                        uint8_t *hit_out);
int vrhip_set_image_ess(vrhip_renderer *r, uint32_t width, uint32_t height, const uint8_t *hit_in,
                        const uint8_t *hit_out);
/* The cell grid behind empty-run skipping and the path tracer's culling (no reference counterpart;
 * DESIGN.md "Kernels"): per cell of 2^shift voxels the (min, max) of the raw voxel values a fetch in
 * or within one texel of the cell can read, as pairs of floats, x fastest.  Builds the grid of the
 * current time step if need be.  out == NULL: dims / shift only.  For tests. */
int vrhip_download_cells(vrhip_renderer *r, float *out_minmax, size_t n_floats, uint32_t dims[3],
                         uint32_t *shift);
/* The same for the finer grid the ray caster's empty bits live on (cells of 4 voxels up to 2048^3;
 * the grid above where the two coincide). */
int vrhip_download_empty_cells(vrhip_renderer *r, float *out_minmax, size_t n_floats, uint32_t dims[3],
                               uint32_t *shift);
/* What the renderer derives from those grids and the transfer function (vr_cells.hip), rebuilt for the current time
 * step and transfer function and copied out; any output may be NULL.  For tests (tests/test_gpu_cell_tables.py).
 *   out_bound  n_bound = cx*cy*cz floats: the opacity bound of every cell of the grid of vrhip_download_cells
 *   out_macro  n_macro = ccx*ccy*ccz floats: the bound of every macro cell of 4 x 4 x 4 cells
 *   out_leap   n_leap = 7 * n_macro bytes: level j = 1..7 (threshold j / 8) at [(j - 1) * n_macro + C]: 0 when macro
 *              cell C is not free at that level, else 1 + the radius (<= 15) of the free cube of macro cells around it
 *   out_empty  n_empty = (ecx*ecy*ecz + 31) / 32 words: bit (c & 31) of word c >> 5 = cell c of the grid of
 *              vrhip_download_empty_cells is empty (every fetch in it reads opacity exactly 0)
 *   dims       {cx, cy, cz, ccx, ccy, ccz, ecx, ecy, ecz};  shifts  {shift, eshift}
 * All outputs NULL: dims / shifts only.  A size that does not match is VRHIP_ERR_INVALID. */
int vrhip_download_cell_tables(vrhip_renderer *r, float *out_bound, size_t n_bound, float *out_macro, size_t n_macro,
                               uint8_t *out_leap, size_t n_leap, uint32_t *out_empty, size_t n_empty, uint32_t dims[9],
                               uint32_t shifts[2]);

/* Image-tile gather, root side: the frame from the gathered tiles.  `staging_dev` holds
 * tile slots of tile_w x tile_h RGBA float pixels (the peers' blocks as received, one after the
 * other); slot_of_tile_dev[t] is the slot of tile t (tiles numbered row-major over the frame).
 * One thread per pixel, enqueued on the renderer's stream; frame_dev = width x height x 4 floats. */
int vrhip_assemble_frame(vrhip_renderer *r, const float *staging_dev, const uint32_t *slot_of_tile_dev,
                         uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h,
                         float *frame_dev);

/* Multi-GPU, rank 0: assemble the n_frames frames of a batch straight from the ranks' gather messages
 * (tiles.py TileDriver, sparse gather: a tile of one colour travels as one pixel).  msgs_dev: HOST array
 * of `world` (<= 64) device pointers, message r = [maxc floats: slot numbers of rank r's whole tiles |
 * S = n_frames x cap RGBA pixels, one per tile slot | maxc whole tiles of tile_w x tile_h RGBA pixels]
 * (16-byte aligned, maxc a multiple of 4); pos_dev[r * S + row] = -1 (one colour: that pixel) or the
 * position of row = frame x cap + slot among rank r's whole tiles; rank_slot_of_tile_dev[t] = rank << 16 |
 * slot of tile t (tiles numbered row-major over the frame).  One thread per pixel of frames_dev
 * [n_frames][height][width][4], enqueued on hip_stream (a hipStream_t; NULL = legacy default stream). */
int vrhip_assemble_batch(vrhip_renderer *r, void *hip_stream, const float *const *msgs_dev, uint32_t world,
                         uint32_t n_frames, uint32_t cap, uint32_t maxc, const int32_t *pos_dev,
                         const uint32_t *rank_slot_of_tile_dev, uint32_t width, uint32_t height, uint32_t tile_w,
                         uint32_t tile_h, float *frames_dev);

/* Multi-GPU, every rank: pack the n_slots tile slots of a batch (tile_pixels RGBA float pixels each, one after the
 * other in tiles_dev: a rank's output of vrhip_render_batch with a tile subset) into the sparse gather message
 * [spad slot numbers of the whole tiles (int32 bits) | n_slots pixels, one per slot | the whole tiles], spad =
 * n_slots rounded up to a multiple of 4: a tile whose pixels are all bit-identical travels as its one pixel.  Pure
 * data compression (no notion of a background).  msg_dev holds spad + 4 n_slots + 4 n_slots tile_pixels floats (the
 * worst case); count_dev receives the number c of whole tiles: the first spad + 4 n_slots + 4 c tile_pixels floats
 * are what has to travel.  scratch_dev: n_slots int32.  All device memory, 16-byte aligned; three small kernels on
 * hip_stream.  The root reads the messages with vrhip_message_positions + vrhip_assemble_batch (maxc = spad). */
int vrhip_pack_tiles(vrhip_renderer *r, void *hip_stream, const float *tiles_dev, uint32_t n_slots,
                     uint32_t tile_pixels, int32_t *scratch_dev, float *msg_dev, uint32_t *count_dev);
/* Multi-GPU, rank 0: pos_dev[rank * n_slots + row] (what vrhip_assemble_batch reads) from the slot lists at the
 * head of the `world` received messages; counts_host[rank] = that rank's number of whole tiles.  msgs_dev: HOST
 * array of device pointers. */
int vrhip_message_positions(vrhip_renderer *r, void *hip_stream, const float *const *msgs_dev,
                            const uint32_t *counts_host, uint32_t world, uint32_t n_slots, int32_t *pos_dev);

/* ---- 8-bit frames (the reference's output image is CL_UNORM_INT8, volumerendercl.cpp:468-478: what its GUI shows,
 * saves and records; the float frame above stays the parity surface) -------------------------------------------
 * One conversion everywhere, per channel of an fp32 pixel: q(f) = 0 for a NaN, else (uint8) rint(clamp(f * 255.0f,
 * 0, 255)) -- ONE rounded fp32 multiply, a clamp, round-half-to-even: OpenCL's convert_uchar_sat_rte(f * 255.0f),
 * what write_imagef does on such an image.  +inf gives 255; -inf, negatives and -0.0 give 0.  A pixel is the bytes
 * R, G, B, A in memory order, i.e. the word r | g << 8 | b << 16 | a << 24.  (numpy: frontend.quantise_rgba8.) */
/* Quantise `rows` blocks of `row_pixels` RGBA float pixels, `src_stride` (>= row_pixels) pixels apart in src_dev
 * (device memory, 16-byte aligned) and dense in dst: a frame (rows = 1), the frames of a batch rendered with
 * out_frame_stride, a tile layout.  One kernel on hip_stream (a hipStream_t; NULL = legacy default stream).
 * dst_is_device != 0: dst is device memory (4-byte aligned) and the call returns without synchronising; else dst is
 * host memory: the bytes travel through a pinned staging block the renderer owns (grown on demand, freed with the
 * renderer) and the call returns after the copy has completed.  A NULL pointer, src_stride < row_pixels or
 * rows x row_pixels >= 2^32: VRHIP_ERR_INVALID. */
int vrhip_quantise_rgba8(vrhip_renderer *r, void *hip_stream, const float *src_dev, uint32_t rows,
                         uint32_t row_pixels, uint32_t src_stride, uint8_t *dst, int dst_is_device);
/* runRaycastNoGL as the reference reads it back (volumerendercl.cpp:568-607): exactly vrhip_render_frame with
 * out_rgba == NULL, then the renderer's frame buffer quantised on the same stream into out_rgba8 (width * height * 4
 * bytes, row 0 = top; host memory, or device memory when out_is_device != 0).  The float frame buffer keeps the
 * unquantised frame: progressive accumulation and image-order ESS carry on across calls bit for bit as with
 * vrhip_render_frame. */
int vrhip_render_frame_rgba8(vrhip_renderer *r, uint32_t width, uint32_t height, uint8_t *out_rgba8,
                             int out_is_device);
/* The second half of it alone: the frame the renderer's frame buffer holds -- what the last vrhip_render_frame
 * (with out_rgba NULL or host memory), vrhip_render_frame_rgba8 or whole-frame vrhip_render_samples of this size
 * left there -- quantised on the renderer's stream into out_rgba8; nothing is rendered.  For a caller that has the
 * float frame already and wants its bytes too (a screenshot of what is shown).  No frame of width x height in the
 * frame buffer: VRHIP_ERR_NODATA. */
int vrhip_frame_rgba8(vrhip_renderer *r, uint32_t width, uint32_t height, uint8_t *out_rgba8, int out_is_device);
/* Multi-GPU, every rank: the 8-bit twin of vrhip_pack_tiles.  tiles_dev holds the FLOAT tiles the rank has rendered;
 * the message is [spad slot numbers of the whole tiles (int32) | n_slots pixels, one word each | the whole tiles,
 * tile_pixels words each], spad = n_slots rounded up to a multiple of 4: a tile travels as its one pixel when its
 * QUANTISED pixels are all equal (so also one whose floats differ only below the rounding).  msg_dev holds spad +
 * n_slots + n_slots tile_pixels words (the worst case); count_dev receives the number c of whole tiles: the first
 * spad + n_slots + c tile_pixels words are what has to travel.  scratch_dev: n_slots int32.  All device memory,
 * tiles_dev and msg_dev 16-byte aligned; three small kernels on hip_stream.  The head is the float message's:
 * vrhip_message_positions reads both formats. */
int vrhip_pack_tiles_rgba8(vrhip_renderer *r, void *hip_stream, const float *tiles_dev, uint32_t n_slots,
                           uint32_t tile_pixels, int32_t *scratch_dev, uint32_t *msg_dev, uint32_t *count_dev);
/* Multi-GPU, rank 0: the 8-bit twin of vrhip_assemble_batch.  Arguments as there, with message r = [maxc slot
 * numbers | S = n_frames x cap words, one per tile slot | whole tiles of tile_w x tile_h words] (16-byte aligned,
 * maxc a multiple of 4) and frames_dev[n_frames][height][width] words (4-byte aligned). */
int vrhip_assemble_batch_rgba8(vrhip_renderer *r, void *hip_stream, const uint32_t *const *msgs_dev, uint32_t world,
                               uint32_t n_frames, uint32_t cap, uint32_t maxc, const int32_t *pos_dev,
                               const uint32_t *rank_slot_of_tile_dev, uint32_t width, uint32_t height,
                               uint32_t tile_w, uint32_t tile_h, uint8_t *frames_dev);

/* A batch of n_frames <= 256 INDEPENDENT frames (n_frames x pixels per frame < 2^32) -- same camera and parameters, frame f with jitter
 * seed seeds[f] (rendering_params.seed is not used) -- in ONE set of launches: the work queue holds
 * every patch once per frame, so a small tile share still fills the GPU and the latency chain of
 * a frame (pre-pass, phase-1 rounds, sort, the longest rays of phase 2) is paid once per batch.
 * tile_ids == NULL: whole frames, out_dev[n_frames][height][width][4]; else the tile subset like
 * vrhip_render_tiles, out_dev[n_frames][n_tiles][tile_h][tile_w][4]; out_frame_stride != 0 gives the
 * distance between the frames of out_dev in pixels (>= one frame).  DEVICE output only (the
 * renderer's own frame buffer is not meaningful afterwards).  Ray caster, maximum intensity
 * projection or first-hit isosurface (technique 0, 2 or 4), iteration 0, no image-order ESS, no ambient
 * occlusion: anything else is VRHIP_ERR_UNSUPPORTED. */
int vrhip_render_batch(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                       uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                       const uint32_t *seeds, uint32_t n_frames, float *out_dev,
                       uint32_t out_frame_stride);
/* The same with a camera per frame: frame f is rendered with cams[f] (n_frames HOST structs: view matrix,
 * bbox, ortho) instead of the renderer's camera -- a turntable, a fly-through, a replayed camera path in one
 * set of launches.  Everything else (transfer function, parameters, restrictions) is shared by the frames as
 * in vrhip_render_batch; cams == NULL is exactly vrhip_render_batch. */
int vrhip_render_batch_views(vrhip_renderer *r, uint32_t width, uint32_t height, uint32_t tile_w,
                             uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                             const uint32_t *seeds, const vrhip_camera_params *cams, uint32_t n_frames,
                             float *out_dev, uint32_t out_frame_stride);
/* Progressive path tracer (technique 1): n_samples CONSECUTIVE iterations of the accumulated image in as few sets
 * of launches as possible.  Sample k is traced with jitter seed seeds[k] (rendering_params.seed is not used) at
 * iteration rendering_params.iteration + k, and the renderer's frame buffer ends up bit for bit where n_samples
 * calls of vrhip_render_frame with those seeds and iterations would have left it: the running mean
 * prev + (cur - prev) / (iteration + 1) per colour channel, alpha 1, a sample whose ray misses the box replacing
 * the pixel with the background (volumeraycast.cl:677-704).  With iteration 0 the first sample is written, not
 * averaged; with iteration > 0 the call carries on from the frame buffer as it stands.  Like every entry point
 * here it does NOT advance rendering_params.iteration.
 * A set holds samples_per_launch samples (0: the default; at most 256, and fewer where a set would exceed 2^32
 * pixels): one launch of the sample kernel -- the work queue holds every 8x8 patch once per sample -- and one
 * streaming fold, in sample order, of the set's per-sample records (17 bytes per pixel and sample of scratch,
 * allocated on first use, kept, freed with the renderer).  A larger n_samples is a chain of such sets.
 * tile_ids == NULL: the whole frame, out_rgba[height][width][4]; else the tile subset as in vrhip_render_tiles,
 * out_rgba[n_tiles][tile_h][tile_w][4].  out_rgba may be NULL (the image stays in the frame buffer), host memory or
 * (out_is_device) device memory.  vrhip_get_stats: the sums over all samples; vrhip_last_kernel_seconds and
 * vrhip_last_launch_info: the last set, its fold included (with phase timing on, phase 2 is the fold).
 * Technique 0, 2 or 4: VRHIP_ERR_UNSUPPORTED.  n_samples == 0 or seeds == NULL: VRHIP_ERR_INVALID. */
int vrhip_render_samples(vrhip_renderer *r, uint32_t width, uint32_t height,
                         uint32_t tile_w, uint32_t tile_h, const uint32_t *tile_ids, uint32_t n_tiles,
                         const uint32_t *seeds, uint32_t n_samples, uint32_t samples_per_launch /* 0 = default */,
                         float *out_rgba, int out_is_device);
/* getLastExecTime (volumerendercl.cpp:1053-1056): HIP-event time of the last ray-cast
 * kernel launch, seconds. */
double vrhip_last_kernel_seconds(const vrhip_renderer *r);
/* The ray-cast pass is two back-to-back launches (budgeted march of every ray, then the
 * suspended long rays with 4 lanes per ray): HIP-event seconds of each. */
int vrhip_last_phase_seconds(const vrhip_renderer *r, double *phase1, double *phase2);
/* The event between the two phases costs a few microseconds of GPU time per frame (a barrier packet
 * between two launches): it is recorded only while this is enabled (default off; then
 * vrhip_last_phase_seconds answers VRHIP_ERR_NODATA). */
int vrhip_set_phase_timing(vrhip_renderer *r, int enabled);
/* The two events around a frame's launches (what vrhip_last_kernel_seconds reads; the reference times every frame
 * with CL profiling events, volumerendercl.cpp:545-551) cost GPU time of their own when frames follow each other
 * without a wait in between.  Default on; off: vrhip_last_kernel_seconds answers 0 and vrhip_last_phase_seconds
 * VRHIP_ERR_NODATA. */
int vrhip_set_frame_timing(vrhip_renderer *r, int enabled);

/* What the last render call launched (no reference counterpart; filled by the launchers themselves, not
 * re-derived): the tests and bench.py assert that the kernel instantiation and schedule they mean to check
 * are the ones that ran -- e.g. that the timed frames of the benchmark and the frames compared with the
 * oracle came out of the same kernels. */
typedef struct vrhip_launch_info {
    uint32_t technique;      /* 0 ray caster, 1 path tracer, 2 maximum intensity projection, 4 first-   */
                             /* hit isosurface (2 and 4: only frames, work_items, empty_skip and views  */
                             /* are filled, the rest is 0)                                              */
    uint32_t frames;         /* frames of the launch set (vrhip_render_batch), else 1                   */
    uint32_t work_items;     /* 8x8 patches in the work queue, all frames                               */
    uint32_t prepass;        /* 1: vr_dda_prepass_kernel ran                                            */
    uint32_t ray_list;       /* 1: phase 1 = vr_raycast_rays_kernel on the pre-pass's ray list          */
    uint32_t phase1_waves;   /* waves per workgroup of the phase-1 kernel: 4, or 12 (three per SIMD)    */
    uint32_t phase2_waves;   /* the same for vr_raycast_split_kernel; 0: single phase                   */
    uint32_t round_budget;   /* phase-1 sample rounds per ray, 0 = single phase                         */
    uint32_t footprint;      /* 1: the kernels read the footprint volume                                */
    uint32_t empty_skip;     /* 1: the empty-run lookahead is on (cell grid handed to the kernels);     */
                             /* technique 2: samples below the running maximum are skipped by that grid */
                             /* technique 4: march samples below isoValue are                           */
    uint32_t skip_in_lds;    /* 1: the ESS skip bitmap is staged in LDS (phase 1)                       */
    uint32_t instrumented;   /* 0 production kernels, 1 work counters, 2 / 3 + touched bitmap           */
    uint32_t extras;         /* 1: the variants with the rarer modes (illumType 2-5, AO, contours, ...) */
    uint32_t patch_classes;  /* 1: the pre-pass used per-patch classes                                  */
    uint32_t sorted_phase2;  /* 1: suspended rays were counting-sorted, longest first                   */
    uint32_t views;          /* 1: per-frame cameras (vrhip_render_batch_views with cams != NULL)       */
    uint32_t samples;        /* 1: the sample variant of the path tracer and its fold (vrhip_render_samples) */
    uint32_t reserved[14];
    uint32_t pixel_major;    /* 1: phase 1 drew the set's rays pixel by pixel across its frames (vr_regroup_kernel  */
                             /* ran: vrhip_render_batch sets of >= 2 frames), 0: in the pre-pass's order            */
} vrhip_launch_info;
/* VRHIP_ERR_NODATA before the first render call. */
int vrhip_last_launch_info(const vrhip_renderer *r, vrhip_launch_info *out);

/* The per-pixel cost map of the two-phase march (no reference counterpart; a schedule, not a result): for every
 * pixel of the last width x height frame the 4-lane rounds (16 samples each) its ray needed when it last reached
 * the 4-lane kernel -- the key suspended rays are sorted by.  n = width * height.  For tools (tools/costmap.py). */
int vrhip_download_cost_map(vrhip_renderer *r, uint16_t *out, size_t n);

/* The pixel-major ray order of the launch set just rendered (no reference counterpart; a schedule, not a result):
 * what the pre-pass noted, the ray records it appended and the index vr_regroup_kernel made of them, copied out
 * as they lie in device memory.  VRHIP_ERR_NODATA unless the last render call on this renderer was a launch set
 * whose launch info says pixel_major == 1.  Synchronises the renderer's stream; launches nothing and changes
 * nothing.  For tests (tests/test_gpu_ray_order.py).
 *   sizes        {set_frames, n = work items, group, live_list_cap(n), pm_list_cap(n, set_frames),
 *                 R = records of the eight ray lists together, E = entries of the eight index lists together, 0};
 *                R and E count at most a list's capacity per list (a counter beyond it is reported as it is in
 *                out_counters, and the copy stops at the capacity)
 *   out_items    3 n words: (patch column, patch row, frame) of every work item, in queue order
 *   out_notes    3 n words as the pre-pass left them: the live ballot of item q at [2 q] (pixels 0-31 of the
 *                patch, bit = 8 * row + column) and [2 q + 1] (pixels 32-63), the position of its first record
 *                in the ray lists at [2 n + q]
 *   out_counters 16 words: the eight ray-list counters, then the eight index-list counters
 *   out_records  4 R words: (gx, gy, frame, position in the ray lists) of every record, list 0 first
 *   out_index    E words: the entries of the index lists, list 0 first: a position in the ray lists, or
 *                0xffffffff where an entry pads a patch's run to a multiple of the group
 * Any output may be NULL; all NULL: sizes only.  A size that does not match is VRHIP_ERR_INVALID. */
int vrhip_download_ray_order(vrhip_renderer *r, uint32_t sizes[8], uint32_t *out_items, size_t n_items,
                             uint32_t *out_notes, size_t n_notes, uint32_t out_counters[16], uint32_t *out_records,
                             size_t n_records, uint32_t *out_index, size_t n_index);

/* ---- measurement helpers ------------------------------------------- */
/* When enabled, render calls run the instrumented kernel variant that accumulates
 * vrhip_stats (one atomic per wave). */
int vrhip_set_stats_enabled(vrhip_renderer *r, int enabled);
int vrhip_get_stats(const vrhip_renderer *r, vrhip_stats *out);
/* Untimed instrumentation pass over the current frame set-up: number of distinct
 * 4x4x4-voxel micro-bricks touched by at least one voxel fetch (compulsory traffic,
 * SURVEY 8d B_frame). Optionally returns the bitmap (ceil(res/4)^3 bits). */
int vrhip_count_touched(vrhip_renderer *r, uint32_t width, uint32_t height,
                        uint64_t *microbricks_touched, uint8_t *bitmap_host, size_t bitmap_bytes);
/* Path tracer (technique 1): the micro-bricks touched by the voxel fetches the PRODUCT issues -- tracking
 * steps the opacity bound of their cell cannot rule out (the others are rejections whatever the voxels
 * hold and are never fetched) plus the gradient at the primary interaction; speculative steps of a batch
 * excluded.  vrhip_count_touched counts the reference's fetch set (every step inside the volume).  The
 * difference is the traffic the culling removes; bench.py prices the kernel against THIS set. */
int vrhip_count_fetched(vrhip_renderer *r, uint32_t width, uint32_t height, uint64_t *microbricks_fetched);
/* Same for a tile subset (arguments as vrhip_render_tiles); also fills vrhip_get_stats. */
int vrhip_count_touched_tiles(vrhip_renderer *r, uint32_t width, uint32_t height,
                              uint32_t tile_w, uint32_t tile_h, const uint32_t *tile_ids,
                              uint32_t n_tiles, uint64_t *microbricks_touched);

/* Hash (16 hex digits) of the kernel sources this library was built from (the .hip and .h files of csrc/ and this header,
 * volumerenderercl_amd/_srchash.py): bench.py compares it with the tree's before it measures, so that a stale build
 * is never measured under the tree's name.  No reference counterpart. */
const char *vrhip_build_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* VRHIP_H */

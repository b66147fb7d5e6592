"""Analytic closed forms that pin the oracle's march loop independently of any reference
run: empty volume -> background; constant-density volume ->
alpha = 1 - (1-a)^(n/rate) with n = number of samples the step rule yields."""
import numpy as np

from oracle import vro
from volumerenderercl_amd import frontend


def _params(view=None, illum=0, rate=1.5, seed=3499211612, res=(32, 32, 32)):
    cam = vro.CameraParams()
    cam.viewMat[:] = view or frontend.view_matrix()
    cam.bbox_bl[:] = [-1, -1, -1, 0]
    cam.bbox_tr[:] = [1, 1, 1, 0]
    rp = vro.RenderingParams()
    rp.backgroundColor[:] = [1, 1, 1, 1]
    rp.modelScale[:] = [1, 1, 1, 0]
    rp.illumType, rp.useLinear, rp.seed = illum, 1, seed
    rc = vro.RaycastParams()
    rc.samplingRate = rate
    _, brf, _ = vro.brick_layout(res)
    rc.brickRes[:] = brf + [0]
    return cam, rp, rc


def test_empty_volume_gives_background():
    vol = np.zeros((32, 32, 32), np.uint8)
    cam, rp, rc = _params()
    for ess in (True, False):
        img, st, _ = vro.render_tile(vol, vro.UCHAR, frontend.tff_from_stops(), cam, rp, rc,
                                     use_ess=ess, W=48, H=40)
        assert np.all(img[..., :3] == 1.0) and np.all(img[..., 3] == 0.0)
        if ess:
            assert st["samples_taken"] == 0 and st["bricks_skipped"] == st["bricks_visited"] > 0


def test_constant_density_closed_form():
    """Constant voxel value v, constant TF alpha a, no ESS: every ray takes n samples and
    ends with alpha = 1 - (1-a)^(n/rate) (or stops once alpha > 0.98)."""
    vol = np.full((24, 24, 24), 128, np.uint8)
    tff = np.zeros((1024, 4), np.uint8)
    a8 = 5
    tff[:, 3] = a8
    tff[:, 0] = 255   # colour: result = bg - (bg - c) * alpha
    cam, rp, rc = _params(rate=1.5, res=(24, 24, 24))
    img, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=40, H=40)
    a = np.float64(np.float32(a8) / np.float32(255))
    hit = img[..., 3] > 0
    assert hit.sum() == st["rays_hit"] > 0
    n = st["samples_taken"] / st["rays_hit"]
    # per-ray check: alpha determines n_ray, and colour follows from alpha
    alpha = img[..., 3][hit].astype(np.float64)
    n_ray = np.log1p(-alpha) / np.log1p(-a) * 1.5
    assert np.all(np.abs(n_ray - np.round(n_ray)) < 2e-3)      # integer sample counts
    assert abs(n_ray.mean() - n) < 1e-2
    # colour: bg=1, tf colour (1,0,0): result = 1 - (1 - c) * alpha
    np.testing.assert_allclose(img[..., 0][hit], 1.0, atol=1e-6)
    np.testing.assert_allclose(img[..., 1][hit], 1.0 - alpha, atol=2e-6)
    np.testing.assert_allclose(img[..., 2][hit], 1.0 - alpha, atol=2e-6)


def test_ert_stops_rays():
    vol = np.full((24, 24, 24), 255, np.uint8)
    tff = np.zeros((1024, 4), np.uint8)
    tff[:, 3] = 200
    cam, rp, rc = _params(res=(24, 24, 24))
    img, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=32, H=32)
    hit = img[..., 3] > 0
    # grazing rays at the box silhouette take a single sample; all others terminate early
    assert np.mean(img[..., 3][hit] >= np.float32(0.98)) > 0.9
    assert st["samples_taken"] < 8 * st["rays_hit"]


def test_tile_equals_full_frame_crop():
    vol = vro.synth_volume("sphere", [32, 32, 32], vro.UCHAR)
    cam, rp, rc = _params(view=frontend.view_matrix(frontend.quat_from_axis_angle((1, 1, 0), 30)),
                          illum=1)
    tff = frontend.tff_from_stops()
    full, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=70, H=50)
    part, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=70, H=50, tile=(16, 8, 33, 21))
    np.testing.assert_array_equal(part, full[8:29, 16:49])


def test_pathtrace_empty_volume_gives_background():
    """technique 1: zero opacity everywhere -> no walk ever accepts an interaction -> every
    pixel that hits the box keeps the background colour with alpha 1 (volumeraycast.cl:
    463-503 with isInteraction == false, :689-704)."""
    vol = np.zeros((24, 24, 24), np.float32)
    cam, rp, rc = _params(res=(24, 24, 24))
    rp.technique = 1
    img, st, _ = vro.render_tile(vol, vro.FLOAT, frontend.tff_from_stops(), cam, rp, rc,
                                 pt=vro.PathtraceParams(50.0), W=48, H=40)
    assert np.all(img[..., :3] == 1.0)
    hit = img[..., 3] == 1.0          # misses carry the background alpha (1 here as well)
    assert hit.all() and st["rays_hit"] > 0
    # every primary walk runs until it leaves the box or for 513 steps, and is the only walk
    assert st["rays_hit"] <= st["samples_taken"] <= 513 * st["rays_hit"]


def test_pathtrace_opaque_volume_closed_form():
    """technique 1, opacity 1 everywhere, TF colour (1, 0, 0): the primary walk accepts its
    first step inside the box; the TF-opacity gradient is 0 -> the fallback normal with
    |(-n, 0)| = 1 > 0.5 -> Phong branch; the shadow walk accepts its first step -> w = 0.6.
    So G == B == 0.6 * 0.15 * spec and R - G = 0.6 * (0.15 + 0.7 * max(0, n.l))."""
    vol = np.full((24, 24, 24), 0.5, np.float32)
    tff = np.zeros((256, 4), np.uint8)
    tff[:, 0] = 255
    tff[:, 3] = 255
    cam, rp, rc = _params(res=(24, 24, 24))
    rp.technique = 1
    rp.backgroundColor[:] = [0.25, 0.5, 0.75, 1.0]
    img, st, _ = vro.render_tile(vol, vro.FLOAT, tff, cam, rp, rc, pt=vro.PathtraceParams(100.0),
                                 W=64, H=64)
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    traced = np.any(img[..., :3] != bg, axis=-1)
    assert traced.sum() > 0.3 * traced.size
    r, g, b = (img[..., i][traced].astype(np.float64) for i in range(3))
    np.testing.assert_array_equal(g, b)
    d = r - g
    # w is 0.6 when the shadow walk interacts (its first step stays inside the box) else 1
    assert np.all((d >= 0.6 * 0.15 - 1e-6) & (d <= 0.85 + 1e-6))
    assert np.all(g <= 0.15 + 1e-6)
    # 1 primary + 1 shadow step for interior hits; grazing rays leave the box on the first step
    assert st["samples_taken"] <= 2 * st["rays_hit"]


def test_downsample_box_mean():
    """downsampling (volumeraycast.cl:966-994): box sums over ceil(res/lowres)^3 voxels divided
    by the full box volume, UNORM written with round-to-nearest-even; constant volumes stay
    constant where the box is complete and fade at a clipped border."""
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 256, size=(8, 6, 10), dtype=np.uint8)       # z, y, x
    lo = vro.downsample(vol, vro.UCHAR, 2)
    assert lo.shape == (4, 3, 5)
    blocks = vol.reshape(4, 2, 3, 2, 5, 2).astype(np.float64).mean(axis=(1, 3, 5))
    assert np.abs(lo.astype(np.float64) - blocks).max() <= 0.5 + 1e-3
    const = np.full((6, 6, 7), 200, np.uint8)                          # x = 7: last box clipped
    lo = vro.downsample(const, vro.UCHAR, 2)
    assert lo.shape == (3, 3, 4)
    assert np.all(lo[:, :, :3] == 200) and np.all(lo[:, :, 3] == 100)
    f = np.linspace(0, 1, 4 * 4 * 6, dtype=np.float32).reshape(4, 4, 6)
    lo = vro.downsample(f, vro.FLOAT, 3)                               # res (6,4,4) -> (2,2,2)
    assert lo.shape == (2, 2, 2)
    np.testing.assert_allclose(lo[0, 0, 0], f[:2, :2, :3].sum() / 12.0, rtol=1e-6)


def test_show_ess_marks_skipped_rays_and_box_edges():
    """showEss (:888-896): rays that never sample keep pos = 0 and get |1 - background| with
    alpha 1; so do rays whose last sample lies next to an edge of the box."""
    vol = np.zeros((32, 32, 32), np.uint8)
    vol[8:24, 8:24, 8:24] = 200
    cam, rp, rc = _params(illum=0)
    rp.backgroundColor[:] = [0.25, 0.5, 1.0, 1.0]
    tff = frontend.tff_from_stops()
    plain, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=64, H=64)
    rp.showEss = 1
    shown, st, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=64, H=64)
    marked = np.all(shown[..., :3] == np.float32([0.75, 0.5, 0.0]), axis=-1) & (shown[..., 3] == 1)
    hit_box = plain[..., 3] != 1.0          # missed rays carry the background alpha (1)
    # rays that meet the box but no brick to sample are marked: all of them for an empty volume
    assert (marked & hit_box).sum() > 0 and st["samples_taken"] > 0
    rp.showEss = 1
    empty, st0, _ = vro.render_tile(np.zeros_like(vol), vro.UCHAR, tff, cam, rp, rc, W=64, H=64)
    assert st0["samples_taken"] == 0
    m0 = np.all(empty[..., :3] == np.float32([0.75, 0.5, 0.0]), axis=-1) & (empty[..., 3] == 1)
    assert np.array_equal(m0, hit_box)
    # unmarked pixels are those of the plain frame
    assert np.array_equal(shown[~marked], plain[~marked])
    assert not marked[~hit_box].any()


def test_image_order_ess_sequence():
    """imgEss (:659-670, :912-925): groups without a hit in their 3x3 neighbourhood last frame
    are filled with the background; the hit image converges to the footprint of the volume."""
    vol = np.zeros((32, 32, 32), np.uint8)
    vol[12:20, 12:20, 12:20] = 255
    cam, rp, rc = _params(illum=0)
    tff = frontend.tff_from_stops()
    W, H = 96, 80
    plain, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H)
    rp.imgEss = 1
    hin, hout = vro.hit_image_init(W, H)
    assert hin.shape == (H // 8 + 1, W // 8 + 1) and hin.reshape(-1)[:8].tolist() == [1, 0, 0, 0] * 2
    frames = []
    for _ in range(4):
        img, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H, hit_in=hin,
                                    hit_out=hout)
        frames.append((img, hin.copy(), hout.copy()))
        hin, hout = hout, hin        # runRaycast's swap (volumerendercl.cpp:524-530)
    changed = np.any(plain[..., :3] != 1.0, axis=-1)
    for img, h_in, h_out in frames:
        for gy in range(H // 8):
            for gx in range(W // 8):
                nb = h_in[max(gy - 1, 0):gy + 2, max(gx - 1, 0):gx + 2].sum()
                blk = (slice(gy * 8, gy * 8 + 8), slice(gx * 8, gx * 8 + 8))
                if nb == 0:
                    assert np.all(img[blk][..., :3] == 1.0) and h_out[gy, gx] == 0
                else:
                    assert np.array_equal(img[blk], plain[blk])
    # the first frame starts from the reference's 1,0,0,0 byte pattern: with 13 groups per row
    # every group has a set neighbour, so the whole image is rendered and the hit image is exact
    h1 = frames[0][2]
    want = np.zeros_like(h1)
    for gy in range(H // 8):
        for gx in range(W // 8):
            want[gy, gx] = changed[gy * 8:gy * 8 + 8, gx * 8:gx * 8 + 8].any()
    assert np.array_equal(h1, want)
    # steady state: the colours equal the plain frame's (hit groups have their neighbours
    # rendered; skipped pixels carry the background's alpha instead of 0)
    assert np.array_equal(frames[-1][0][..., :3], plain[..., :3])
    assert frames[-1][1].sum() < frames[0][1].size // 2
    # a tile of whole groups gives the same pixels and hit texels as the full frame
    hin, hout = vro.hit_image_init(W, H)
    hout2 = hout.copy()
    full, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H, hit_in=hin, hit_out=hout)
    part, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=W, H=H, tile=(32, 16, 40, 48),
                                 hit_in=hin, hit_out=hout2)
    assert np.array_equal(part, full[16:64, 32:72])
    assert np.array_equal(hout2[2:8, 4:9], hout[2:8, 4:9]) and hout2.sum() == hout[2:8, 4:9].sum()


def test_environment_map_replaces_background():
    """:506-510, :655-656: a map wider than one texel is sampled (linear, clamp to edge) in the
    ray's direction and used wherever the background colour was; a constant map equals a
    constant background; a 1-texel-wide map is ignored."""
    vol = vro.synth_volume("sphere", [24, 24, 24], vro.UCHAR)
    cam, rp, rc = _params(illum=1, res=(24, 24, 24))
    tff = frontend.tff_from_stops()
    rp.backgroundColor[:] = [0.2, 0.4, 0.6, 0.5]
    plain, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=56, H=40)
    const = np.tile(np.float32([0.2, 0.4, 0.6, 0.5]), (4, 8, 1))
    rp.backgroundColor[:] = [1, 1, 1, 1]
    img, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=56, H=40, env=const)
    assert np.array_equal(img, plain)
    one, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=56, H=40, env=const[:, :1])
    white, _, _ = vro.render_tile(vol, vro.UCHAR, tff, cam, rp, rc, W=56, H=40)
    assert np.array_equal(one, white)
    # a map that encodes its own texture coordinates: missed rays return (s, t) of their direction
    h, w = 64, 128
    env = np.zeros((h, w, 4), np.float32)
    env[..., 0] = (np.arange(w, dtype=np.float32) + 0.5) / w
    env[..., 1] = ((np.arange(h, dtype=np.float32) + 0.5) / h)[:, None]
    vol0 = np.zeros_like(vol)
    img, _, _ = vro.render_tile(vol0, vro.UCHAR, tff, cam, rp, rc, W=56, H=40, env=env)
    # default camera looks down -z: atan2(z, x) in (-pi, 0) -> s in (0, 0.5); centre ray s = 0.25
    assert abs(img[20, 28, 0] - 0.25) < 0.06 and abs(img[20, 28, 1] - 0.5) < 0.06
    assert np.all(np.diff(img[20, :, 0]) > 0)       # s grows with x, t with y (image row 0 = top)
    assert np.all(np.diff(img[:, 28, 1]) > 0)


def test_rgba_and_rg_volumes_closed_form():
    """CL_RGBA volumes (:840-845): the voxel is the sample's colour and opacity, the TF is not
    used; CL_RG (:846-855): colour (r, 0, 0), opacity TF(|g|).alpha.  Constant volumes give the
    same closed form as test_constant_density_closed_form."""
    rgba = np.zeros((20, 20, 20, 4), np.uint8)
    rgba[...] = [255, 0, 51, 5]
    cam, rp, rc = _params(rate=1.5, res=(20, 20, 20))
    tff = np.zeros((1024, 4), np.uint8)          # TF with alpha 0 everywhere: must not matter
    img, st, _ = vro.render_tile(rgba, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=40, H=40)
    hit = img[..., 3] > 0
    assert hit.sum() == st["rays_hit"] > 0
    alpha = img[..., 3][hit].astype(np.float64)
    a = np.float64(np.float32(5) / np.float32(255))
    n_ray = np.log1p(-alpha) / np.log1p(-a) * 1.5
    assert np.all(np.abs(n_ray - np.round(n_ray)) < 2e-3)
    np.testing.assert_allclose(img[..., 0][hit], 1.0, atol=1e-6)                 # c = 1
    np.testing.assert_allclose(img[..., 1][hit], 1.0 - alpha, atol=2e-6)         # c = 0
    np.testing.assert_allclose(img[..., 2][hit], 1.0 - 0.8 * alpha, atol=2e-6)   # c = 0.2
    # RG: opacity comes from the TF at |g|, colour is (r, 0, 0)
    rg = np.zeros((20, 20, 20, 2), np.uint8)
    rg[...] = [128, 255]
    tff[:, 3] = np.arange(1024) // 128           # alpha byte 7 at the top of the table
    img2, _, _ = vro.render_tile(rg, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=40, H=40)
    hit2 = img2[..., 3] > 0
    assert np.array_equal(hit2, hit)
    alpha2 = img2[..., 3][hit2].astype(np.float64)
    a2 = np.float64(np.float32(7) / np.float32(255))
    n2 = np.log1p(-alpha2) / np.log1p(-a2) * 1.5
    assert np.all(np.abs(n2 - np.round(n2)) < 2e-3)
    r = np.float64(np.float32(128) / np.float32(255))
    np.testing.assert_allclose(img2[..., 0][hit2], 1.0 - (1.0 - r) * alpha2, atol=2e-6)
    np.testing.assert_allclose(img2[..., 1][hit2], 1.0 - alpha2, atol=2e-6)
    # ESS decisions come from channel 0 through the TF (generateBricks reads .x): where the TF is
    # empty at channel 0's value every brick is skipped, whatever the opacity from |g| would be
    tff[:, 3] = np.where(np.arange(1024) < 900, 0, 7)
    on, st_on, _ = vro.render_tile(rg, vro.UCHAR, tff, cam, rp, rc, use_ess=True, W=40, H=40)
    off, _, _ = vro.render_tile(rg, vro.UCHAR, tff, cam, rp, rc, use_ess=False, W=40, H=40)
    assert st_on["samples_taken"] == 0 and np.all(on[..., :3] == 1.0)
    assert np.array_equal(off, img2)


def test_float_outside_unit_range_reads_tf_edges():
    """FLOAT volumes are raw values (a CT volume in Hounsfield units reaches the kernel as it is).
    read_imagef(tffData, linearSmp, x) with CLAMP_TO_EDGE (OpenCL 1.2 8.2) gives TF[n-1] for every
    x >= 1 and TF[0] for every x <= 0.  A constant volume of such a value then follows the closed form
    of test_constant_density_closed_form with that entry's colour and opacity -- also where x * n
    passes 2^31, which an unclamped float -> int index conversion wraps -- and equals the frame of a
    constant 1.0 or 0.0 volume, with ESS on and off and for tables of 1024 and 4096 entries."""
    flt_max = float(np.finfo(np.float32).max)
    high = [1.0, 1.7, 1e3, 2.0e6, 2.2e6, 5e6, 1e30, flt_max]
    low = [0.0, -0.0, -3.0, -5e6, -flt_max]
    res = (16, 16, 16)
    cam, rp, rc = _params(rate=1.5, res=res)
    for n in (1024, 4096):
        tff = np.zeros((n, 4), np.uint8)
        tff[:] = [0, 0, 255, 3]          # interior: never read by these volumes
        tff[0] = [0, 255, 0, 5]          # TF[0]: green, alpha 5 / 255
        tff[-1] = [255, 0, 0, 9]         # TF[n-1]: red, alpha 9 / 255
        for ess in (True, False):
            for values, a8, rgb in ((high, 9, (1, 0, 0)), (low, 5, (0, 1, 0))):
                frames = {}
                for v in values:
                    vol = np.full(res[::-1], v, np.float32)
                    img, st, _ = vro.render_tile(vol, vro.FLOAT, tff, cam, rp, rc, use_ess=ess, W=32, H=32)
                    frames[v] = img
                    hit = img[..., 3] > 0
                    assert hit.sum() == st["rays_hit"] > 0, (n, ess, v)
                    a = np.float64(np.float32(a8) / np.float32(255))
                    alpha = img[..., 3][hit].astype(np.float64)
                    n_ray = np.log1p(-alpha) / np.log1p(-a) * 1.5
                    assert np.all(np.abs(n_ray - np.round(n_ray)) < 2e-3), (n, ess, v)
                    for c in range(3):   # background 1: 1 - (1 - c) * alpha
                        np.testing.assert_allclose(img[..., c][hit], 1.0 - (1.0 - rgb[c]) * alpha, atol=2e-6,
                                                   err_msg="n=%d ess=%s v=%r" % (n, ess, v))
                for v in values[1:]:
                    np.testing.assert_array_equal(frames[v], frames[values[0]], err_msg="n=%d ess=%s v=%r" % (n, ess, v))

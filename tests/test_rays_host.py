"""Ray lists without a GPU: the equirectangular table, the argument checks of the three entry points (every one is made before any device
call), and the yardstick of tests/test_rays_gpu.py itself -- the oracle called once per ray through a one-pixel camera (rays_ref.oracle_rays)
on the pinhole rays of a frame reproduces the oracle's frame bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cases
import rays_ref


def _ulps(a, b):
    """distance in binary32 steps between two float32 arrays (same sign or across zero)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("w,h", [(1, 1), (8, 4), (75, 41), (1920, 1080), (4096, 2048)])
def test_equirect_tables_within_one_ulp_of_float64(mnv, w, h):
    """Two correctly-rounded-ish binary64 sines differ by binary64 ulps, which moves the binary32 rounding by at most one step."""
    got = mnv.equirect_tables(w, h)
    want = rays_ref.equirect_tables64(w, h)
    assert got.shape == (w + h, 2) and got.dtype == np.float32
    assert int(_ulps(got, want).max()) <= 1
    # the layout: columns first (longitude -pi .. pi: cos < 0 at both ends, sin changes sign), then rows (latitude: cos >= 0)
    if w >= 8:
        assert got[0, 0] < 0 < got[w - 1, 0] and got[0, 1] < 0 and got[w - 1, 1] < 0
    assert (got[w:, 1] >= 0).all() and (h < 2 or got[w, 0] > 0 > got[w + h - 1, 0])


def test_equirect_tables_argument_checks(mnv):
    out = np.zeros((4, 2), np.float32)
    for w, h, p in ((0, 2, out.ctypes.data), (2, 0, out.ctypes.data), (-1, 2, out.ctypes.data), (2, 2, None)):
        assert mnv.lib().mnv_equirect_tables(w, h, p) == mnv.MNV_E_INVALID


def test_generate_rays_argument_checks_need_no_gpu(mnv):
    """Every check returns its code before any device call: the pointers are never dereferenced here."""
    cam = mnv.Camera(32, 16, 100.0)
    fake = C.c_void_p(0x1000)   # never used: each call is refused
    gen = mnv.lib().mnv_generate_rays
    inv = mnv.MNV_E_INVALID
    rect = mnv.Rect(0, 0, 32, 16)
    assert gen(3, C.byref(cam.c), rect, None, fake, fake, None) == inv              # unknown projection
    assert gen(-1, C.byref(cam.c), rect, None, fake, fake, None) == inv
    assert gen(mnv.PROJ_PINHOLE, None, rect, None, fake, fake, None) == inv         # null camera
    assert gen(mnv.PROJ_PINHOLE, C.byref(cam.c), rect, None, None, fake, None) == inv   # null outputs
    assert gen(mnv.PROJ_ORTHO, C.byref(cam.c), rect, None, fake, None, None) == inv
    assert gen(mnv.PROJ_EQUIRECT, C.byref(cam.c), rect, None, fake, fake, None) == inv  # EQUIRECT without its table
    for bad in ((0, 0, 0, 16), (0, 0, 32, 0), (0, 0, -1, 4), (-1, 0, 8, 8), (0, 0, 33, 16), (30, 0, 3, 16), (0, 10, 32, 7)):
        assert gen(mnv.PROJ_PINHOLE, C.byref(cam.c), mnv.Rect(*bad), None, fake, fake, None) == inv, bad
    big = mnv.Camera(1 << 15, 1 << 14, 100.0)                                        # 2^29 pixels
    assert gen(mnv.PROJ_PINHOLE, C.byref(big.c), mnv.Rect(0, 0, 1 << 15, 1 << 14), None, fake, fake, None) == inv
    assert gen(mnv.PROJ_PINHOLE, C.byref(cam.c), rect, None, C.c_void_p(0x1002), fake, None) == inv   # misaligned output
    assert b"mnv_generate_rays" in mnv.lib().mnv_last_error()


def test_render_rays_argument_checks_need_no_gpu(mnv):
    opt = mnv.RenderOptions.defaults()
    fake = C.c_void_p(0x1000)
    fn = mnv.lib().mnv_render_rays_accel
    inv = mnv.MNV_E_INVALID
    # (the accel is checked last of the plain arguments, so each of these is refused for the argument it names)
    assert fn(None, None, fake, 4, 4, C.byref(opt), None, fake, None, None) == inv      # null origins
    assert fn(None, fake, None, 4, 4, C.byref(opt), None, fake, None, None) == inv      # null dirs
    assert fn(None, fake, fake, 4, 4, C.byref(opt), None, None, None, None) == inv      # both outputs null
    assert b"outputs" in mnv.lib().mnv_last_error()
    assert fn(None, fake, fake, 0, 4, C.byref(opt), None, fake, None, None) == inv      # width < 1
    assert fn(None, fake, fake, 4, 0, C.byref(opt), None, None, fake, None) == inv      # height < 1
    assert fn(None, fake, fake, (1 << 28) + 1, 1, C.byref(opt), None, fake, None, None) == inv   # more than 2^28 rays
    assert fn(None, fake, fake, 1 << 15, 1 << 14, C.byref(opt), None, fake, None, None) == inv
    assert b"2^28" in mnv.lib().mnv_last_error()
    assert fn(None, fake, fake, 4, 4, None, None, fake, None, None) == inv              # null options
    assert fn(None, fake, fake, 4, 4, C.byref(opt), None, fake, None, None) == inv      # null accel
    assert b"accel" in mnv.lib().mnv_last_error()


def test_python_wrappers_check_shapes_and_types(mnv):
    """Shape / dtype checks of the binding (the style of render_voxels_accel): raised before the library is called."""
    opt = mnv.RenderOptions.defaults()
    with pytest.raises(mnv.MnvError) as e:
        mnv.render_rays_accel(0, np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), opt)
    assert e.value.code == mnv.MNV_E_INVALID
    with pytest.raises(mnv.MnvError) as e:
        mnv.render_rays_accel(0, None, None, opt)
    assert e.value.code == mnv.MNV_E_INVALID
    r = mnv.lib().mnv_renderer_set_projection(None, mnv.PROJ_ORTHO)
    assert r == mnv.MNV_E_INVALID
    assert (mnv.PROJ_PINHOLE, mnv.PROJ_ORTHO, mnv.PROJ_EQUIRECT) == (0, 1, 2)


def test_one_pixel_cameras_reproduce_the_oracle_frame(mnv, orc):
    """The yardstick: case rot_dirs at its own camera, a 40 x 30 tile, with a depth image and an image under the volume -- the pinhole rays
    of rays_ref through oracle_rays equal the oracle's frame of that tile in every float bit and every byte."""
    spec = cases.CASES["rot_dirs"]
    tree = cases.make_tree(mnv, spec["tree"])
    cam = cases.make_camera(mnv, spec["camera"])
    opt = cases.make_options(mnv, spec["options"])
    tile = (53, 41, 40, 30)
    x0, y0, w, h = tile
    rng = np.random.default_rng(11)
    dist = float(np.linalg.norm(np.array(list(cam.c.c2w))[9:12]))
    tmax = (dist * rng.uniform(0.55, 1.35, size=(h, w))).astype(np.float32)
    u = rng.uniform(size=(h, w))
    tmax[u < 0.15] = np.float32(1e9)
    tmax[u > 0.95] = np.float32(0.0)
    image = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    t = orc.tree_from_view(tree.host_view())
    want = orc.render(t, cam.c, opt, tile=tile, want_rgba8=True, tmax_px=tmax, rgba8_init=image, n_threads=1)
    assert (want["rgba"][..., 3] > 0).mean() > 0.2, "the tile sees too little of the tree to test anything"
    o, d = rays_ref.pinhole_rays(cam.c, tile)
    assert o.shape == (h, w, 3) and not np.any((d == 0) & np.signbit(d))
    got, got8 = rays_ref.oracle_rays(orc, t, o, d, opt, tmax, image)
    assert np.array_equal(cases.bits(got), cases.bits(want["rgba"])), f"{int((cases.bits(got) != cases.bits(want['rgba'])).any(axis=-1).sum())} rays differ"
    assert np.array_equal(got8, want["rgba8"])

"""Reference side of the ray-list tests (tests/test_rays_host.py, tests/test_rays_gpu.py).

* oracle_rays: the oracle renders through a camera, and a 1 x 1 camera is a ray.  With width = height = 1, cx = cy = 0.5, fx = fy = 1 the
  camera-space vector of the only pixel is (0, -0, -1); with the c2w columns right = (1,0,0), up = (0,1,0), back = -d, centre = o the
  oracle computes dir = 1*0 + 0*(-0) + (-d)*(-1) = d exactly (an exactly zero component of d must be +0.0: the sum turns -0 into +0),
  and from there the 1 / sqrtf normalisation, the rodrigues block, the origin transform, the per-ray t_max and the pixel under the
  volume of the ray march's contract (include/mnv.h, mnv_render_rays_accel).
* pinhole_rays / ortho_rays / equirect_rays: the three generators of mnv_generate_rays restated in numpy binary32, every sum left to
  right, every product and sum rounded separately.
"""
import ctypes as C

import numpy as np

f32 = np.float32


def oracle_rays(orc, tree, origins, dirs, opt, tmax=None, rgba8_init=None):
    """origins / dirs: float32 [..., 3]; tmax float32 [...] or None; rgba8_init uint8 [..., 4] or None.
    -> (rgba float32 [..., 4], rgba8 uint8 [..., 4]) of one oracle call per ray, n_threads = 1."""
    o = np.ascontiguousarray(origins, f32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    assert o.shape == d.shape
    assert not np.any((d == 0) & np.signbit(d)), "an exactly zero direction component must be +0.0"
    n = o.shape[0]
    t = None if tmax is None else np.ascontiguousarray(tmax, f32).reshape(n)
    px = None if rgba8_init is None else np.ascontiguousarray(rgba8_init, np.uint8).reshape(n, 4)
    cam = orc.OrcCamera()
    cam.width = cam.height = 1
    cam.fx = cam.fy = 1.0
    cam.cx = cam.cy = 0.5
    o_opt = orc._copy_struct(orc.OrcOptions(), opt)
    ctr = orc.OrcCounters()
    rgba = np.empty((n, 4), f32)
    rgba8 = np.empty((n, 4), np.uint8)
    fn = orc.lib().orc_render_voxels_ex
    m = np.zeros(12, f32)
    m[0] = m[4] = 1.0
    for i in range(n):
        m[6:9] = -d[i]
        m[9:12] = o[i]
        for k in range(12):
            cam.c2w[k] = m[k]
        rc = fn(C.byref(tree), C.byref(cam), C.byref(o_opt), 0, 0, 1, 1, t[i:].ctypes.data if t is not None else None,
                px[i:].ctypes.data if px is not None else None, rgba[i:].ctypes.data, rgba8[i:].ctypes.data, None, None, None, 0, None,
                C.byref(ctr), 1)
        assert rc == 0
    shape = np.shape(origins)[:-1]
    return rgba.reshape(shape + (4,)), rgba8.reshape(shape + (4,))


def _uv(cam, tile):
    x0, y0, w, h = tile
    ix = np.arange(x0, x0 + w, dtype=np.int32).astype(f32)
    iy = np.arange(y0, y0 + h, dtype=np.int32).astype(f32)
    u = ((ix + f32(0.5)) - f32(cam.cx)) / f32(cam.fx)
    v = -(((iy + f32(0.5)) - f32(cam.cy)) / f32(cam.fy))
    return np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))


def _m(cam):
    return np.array(list(cam.c2w), f32)


def _tile(cam, tile):
    return (0, 0, cam.width, cam.height) if tile is None else tuple(tile)


def pinhole_rays(cam, tile=None):
    """cam: CameraStruct.  -> origins, dirs float32 [h, w, 3] (MNV_PROJ_PINHOLE)."""
    tile = _tile(cam, tile)
    m = _m(cam)
    u, v = _uv(cam, tile)
    h, w = u.shape
    o = np.empty((h, w, 3), f32)
    d = np.empty((h, w, 3), f32)
    for k in range(3):
        o[..., k] = m[9 + k]
        d[..., k] = ((m[k] * u).astype(f32) + (m[3 + k] * v).astype(f32)).astype(f32) + f32(m[6 + k] * f32(-1.0))
    return o, d


def ortho_rays(cam, tile=None):
    """MNV_PROJ_ORTHO: fx, fy are pixels per world unit; rays start on the camera plane."""
    tile = _tile(cam, tile)
    m = _m(cam)
    u, v = _uv(cam, tile)
    h, w = u.shape
    o = np.empty((h, w, 3), f32)
    d = np.empty((h, w, 3), f32)
    for k in range(3):
        o[..., k] = (m[9 + k] + (m[k] * u).astype(f32)).astype(f32) + (m[3 + k] * v).astype(f32)
        d[..., k] = f32(m[6 + k] * f32(-1.0))
    return o, d


def equirect_rays(cam, tables, tile=None):
    """MNV_PROJ_EQUIRECT: tables float32 [width + height, 2] = (sin, cos) of the columns' longitudes, then of the rows' latitudes."""
    x0, y0, w, h = _tile(cam, tile)
    m = _m(cam)
    tables = np.asarray(tables, f32)
    lon = tables[x0:x0 + w]
    lat = tables[cam.width + y0:cam.width + y0 + h]
    so, co = lon[None, :, 0], lon[None, :, 1]
    sl, cl = lat[:, None, 0], lat[:, None, 1]
    dx = (cl * so).astype(f32)
    dy = np.broadcast_to(sl, (h, w)).astype(f32)
    dz = -((cl * co).astype(f32))
    o = np.empty((h, w, 3), f32)
    d = np.empty((h, w, 3), f32)
    for k in range(3):
        o[..., k] = m[9 + k]
        d[..., k] = ((m[k] * dx).astype(f32) + (m[3 + k] * dy).astype(f32)).astype(f32) + (m[6 + k] * dz).astype(f32)
    return o, d


def equirect_tables64(width, height):
    """numpy float64 sin / cos of the table's angles, rounded to binary32: what mnv_equirect_tables is compared with."""
    lon = ((np.arange(width, dtype=np.float64) + 0.5) / width - 0.5) * (2.0 * np.pi)
    lat = (0.5 - (np.arange(height, dtype=np.float64) + 0.5) / height) * np.pi
    a = np.concatenate([lon, lat])
    return np.stack([np.sin(a), np.cos(a)], axis=1).astype(f32)

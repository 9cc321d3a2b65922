"""The mesh pass on the device (mnv_render_meshes): against the grid pass on line meshes, against analytic coverage and depth, against its
own draw-over rule, against the numpy restatement of its raster contract bit for bit, and VolumeRenderer frames with meshes against the
oracle's frame over the pass's two images."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aa_ref
import cases
import mesh_ref
import wireframe_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mega-nerf-viewer_amd")
F = np.float32


# ------------------------------------------------------------------------------------------------ helpers

def _verts(pos, col=(1.0, 1.0, 1.0), nrm=(0.0, 0.0, 1.0)):
    pos = np.asarray(pos, F).reshape(-1, 3)
    v = np.empty((pos.shape[0], 9), F)
    v[:, 0:3] = pos
    v[:, 3:6] = np.asarray(col, F)
    v[:, 6:9] = np.asarray(nrm, F)
    return v


def uv_sphere(n_lat, n_lon, radius=1.0, center=(0.0, 0.0, 0.0)):
    """2 * n_lon * (n_lat - 1) triangles, smooth normals, a colour that varies over the surface; indexed."""
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    n = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], axis=-1).reshape(-1, 3)
    col = 0.5 + 0.5 * n * [1.0, -1.0, 0.6]
    v = _verts(n * radius + np.asarray(center), col, n)
    f = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            c, d = a + n_lon, b + n_lon
            if i > 0:
                f.append((a, c, b))
            if i < n_lat - 1:
                f.append((b, c, d))
    return v, np.asarray(f, np.uint32)


class Pair:
    """One mesh on the device and in the restatement."""

    def __init__(self, mnv, vert, faces=None, face_size=3, unlit=False, transform=None, visible=True):
        self.dev = mnv.Mesh(vert, faces, face_size, unlit)
        matrix = None
        if transform is not None:
            matrix = mnv.model_matrix(*transform)
            self.dev.set_matrix(matrix)
        self.dev.visible = visible
        self.ref = mesh_ref.RefMesh(vert, faces, face_size, unlit, matrix, visible)


def _look(mnv, w, h, fx, center=(0.0, 0.0, 5.0), back=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), **kw):
    """A camera at `center` looking along -back; the default looks down -z with x right and y up: the world point (X, Y, 5 - Z) is the
    camera-space point (X, Y, Z)."""
    return mnv.Camera(w, h, fx, **kw).set_pose(center, back, up)


def _gpu(mnv, torch, pairs, cam, opt, tile=None, under=None):
    t, i = mnv.render_meshes([p.dev for p in pairs], cam, opt, tile, under)
    torch.cuda.synchronize()
    return t.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def _assert_contract(mnv, torch, pairs, cam, opt, tile=None, min_hits=1, under=None):
    """mnv_render_meshes == mesh_ref on both images, twice (the per-stream scratch is reused)."""
    tile = tile or (0, 0, cam.width, cam.height)
    want = mesh_ref.render([p.ref for p in pairs], cam.c, tile, opt.background_brightness, under)
    for again in range(2):
        under_dev = None if under is None else tuple(None if u is None else torch.from_numpy(np.ascontiguousarray(u)).cuda() for u in under)
        got = _gpu(mnv, torch, pairs, cam, opt, tile, under_dev)
        bad = (got[0].view(np.uint32) != want[0].view(np.uint32)) | (got[1] != want[1]).any(axis=-1)
        assert not bad.any(), f"run {again}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"
    hits = int((want[0] != F(1e9)).sum())
    assert hits >= min_hits, hits
    return want


def _opt(mnv, bg=0.25):
    opt = mnv.RenderOptions.cli_defaults()
    opt.background_brightness = bg
    return opt


def _at(cam, px, py, Z):
    """world position (for _look's default pose) of the point that projects to pixel coordinates (px, py) at depth Z"""
    px, py, Z = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(Z, np.float64))
    return np.stack([(px - cam.c.cx) * Z / cam.c.fx, (cam.c.cy - py) * Z / cam.c.fy, 5.0 - Z], axis=-1)


# ------------------------------------------------------------------------------------------------ 1. against the grid pass

@pytest.mark.parametrize("name", ["sh4_d6", "terrain_d7_aniso"])
def test_line_mesh_equals_the_wireframe_pass(mnv, torch_gpu, name):
    spec = cases.CASES[name]
    tree = cases.make_tree(mnv, spec["tree"])
    tree.move_to_device()
    opt = cases.make_options(mnv, spec["options"])
    total = 0
    for (w, h), tile in (((75, 53), None), ((96, 64), (5, 3, 70, 45))):
        cs = dict(spec["camera"], width=w, height=h, fx=spec["camera"]["fx"] * w / spec["camera"]["width"])
        cam = cases.make_camera(mnv, cs)
        for depth in (0, 3, 100):
            wire = mnv.Wireframe(tree.device_view(), depth)
            want_t, want_i = wire.render(cam, opt, tile)
            torch_gpu.cuda.synchronize()
            want = (want_t.cpu().numpy(), want_i.cpu().numpy())
            line = Pair(mnv, tree.gen_wireframe(depth), None, 2, unlit=True)
            assert line.dev.face_count * 2 == line.dev.vertex_count == wire.cube_count * 24
            got = _gpu(mnv, torch_gpu, [line], cam, opt, tile)
            assert _same(got, want), (w, h, depth)
            total += int((want[0] != F(1e9)).sum())
    assert total > 1000


# ------------------------------------------------------------------------------------------------ 2. analytic quad

def test_camera_facing_quad_coverage_depth_and_colour(mnv, torch_gpu):
    """75 x 53, fx 60, cx 37, cy 26, the quad at depth 5: px = 37 + 12 X, py = 26 - 12 Y.  Its edges X = -1.02, 1.27, Y = -0.73, 0.93 project to
    24.76, 52.24, 34.76, 14.84: strictly between pixel centres, so the covered pixels are x 25 .. 51, y 15 .. 34."""
    cam = _look(mnv, 75, 53, 60.0)
    assert (cam.c.cx, cam.c.cy) == (37.0, 26.0)
    col = (0.2, 0.6, 0.8)     # c * 255 is an integer for each: the pack is far from a rounding boundary
    quad = Pair(mnv, _verts([[-1.02, -0.73, 0], [1.27, -0.73, 0], [1.27, 0.93, 0], [-1.02, 0.93, 0]], col), [[0, 1, 2], [0, 2, 3]], 3, unlit=True)
    opt = _opt(mnv, 0.5)
    for tile in ((0, 0, 75, 53), (7, 5, 60, 40)):
        t, img = _gpu(mnv, torch_gpu, [quad], cam, opt, tile)
        x0, y0, w, h = tile
        ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
        inside = (xs >= 25) & (xs <= 51) & (ys >= 15) & (ys <= 34)
        assert np.array_equal(t != F(1e9), inside)
        X = (xs + 0.5 - 37.0) / 60.0 * 5.0
        Y = (26.0 - (ys + 0.5)) / 60.0 * 5.0
        want = np.sqrt(X * X + Y * Y + 25.0)
        rel = np.abs(t.astype(np.float64) - want)[inside] / want[inside]
        assert rel.max() <= 1e-5, rel.max()
        assert (img[inside] == (51, 153, 204, 255)).all() and (img[~inside] == (128, 128, 128, 255)).all()


# ------------------------------------------------------------------------------------------------ 3. watertightness and ordering

def test_shared_diagonals_through_pixel_centres_leave_no_hole(mnv, torch_gpu):
    """A plane of 2 x (8 x 8) triangles at depth 4 with fx 64: vertices every 0.25 units = 4 pixels, at integer pixel coordinates, so every
    shared diagonal runs exactly through pixel centres.  All of x 21 .. 52, y 10 .. 41 is covered and nothing else."""
    cam = _look(mnv, 75, 53, 64.0, center=(0.0, 0.0, 4.0))
    k = np.arange(-4, 5) * 0.25
    gx, gy = np.meshgrid(k, k)
    pos = np.stack([gx.ravel(), gy.ravel(), np.zeros(81)], axis=1)
    faces = []
    for j in range(8):
        for i in range(8):
            a = j * 9 + i
            faces += [(a, a + 1, a + 10), (a, a + 10, a + 9)] if (i + j) % 2 == 0 else [(a, a + 1, a + 9), (a + 1, a + 10, a + 9)]
    rng = np.random.default_rng(3)
    for lit in (False, True):
        plane = Pair(mnv, _verts(pos, rng.uniform(0.1, 0.9, size=(81, 3))), faces, 3, unlit=not lit)
        t, _ = _assert_contract(mnv, torch_gpu, [plane], cam, _opt(mnv))
        ys, xs = np.mgrid[0:53, 0:75]
        inside = (xs >= 21) & (xs <= 52) & (ys >= 10) & (ys <= 41)
        assert np.array_equal(t != F(1e9), inside)


def _quad(cam, x0, x1, y0, y1, Z, col):
    return _verts(_at(cam, [x0, x1, x1, x0], [y0, y0, y1, y1], Z), col), np.uint32([[0, 1, 2], [0, 2, 3]])


def test_nearer_wins_first_drawn_wins_ties_invisible_changes_nothing(mnv, torch_gpu):
    cam = _look(mnv, 96, 64, 80.0)
    opt = _opt(mnv, 0.0)
    far = Pair(mnv, *_quad(cam, 10.3, 60.7, 8.2, 50.6, 5.0, (1.0, 0.0, 0.0)), 3, unlit=True)
    near = Pair(mnv, *_quad(cam, 40.4, 90.1, 20.7, 60.2, 4.0, (0.0, 1.0, 0.0)), 3, unlit=True)
    a = _gpu(mnv, torch_gpu, [far, near], cam, opt)
    b = _gpu(mnv, torch_gpu, [near, far], cam, opt)
    assert _same(a, b)
    assert tuple(a[1][30, 50]) == (0, 255, 0, 255) and tuple(a[1][15, 20]) == (255, 0, 0, 255) and tuple(a[1][2, 2]) == (0, 0, 0, 255)
    assert a[0][30, 50] < a[0][15, 20] < F(1e9)
    _assert_contract(mnv, torch_gpu, [far, near], cam, opt)
    # coincident quads: the colour of the one drawn first, whichever that is; as two meshes and as two faces of one mesh
    v1, f = _quad(cam, 10.3, 60.7, 8.2, 50.6, 5.0, (1.0, 0.0, 0.0))
    v2, _ = _quad(cam, 10.3, 60.7, 8.2, 50.6, 5.0, (0.0, 0.0, 1.0))
    red, blue = Pair(mnv, v1, f, 3, unlit=True), Pair(mnv, v2, f, 3, unlit=True)
    rb, br = _gpu(mnv, torch_gpu, [red, blue], cam, opt), _gpu(mnv, torch_gpu, [blue, red], cam, opt)
    covered = rb[0] != F(1e9)
    assert covered.sum() > 1000 and np.array_equal(rb[0].view(np.uint32), br[0].view(np.uint32))
    assert (rb[1][covered] == (255, 0, 0, 255)).all() and (br[1][covered] == (0, 0, 255, 255)).all()
    both = Pair(mnv, np.concatenate([v2, v1]), np.concatenate([f, f + 4]), 3, unlit=True)
    assert _same(_gpu(mnv, torch_gpu, [both], cam, opt), br)
    _assert_contract(mnv, torch_gpu, [blue, red], cam, opt)
    # an invisible mesh changes nothing
    hidden = Pair(mnv, *_quad(cam, 0.0, 96.0, 0.0, 64.0, 2.0, (1.0, 1.0, 1.0)), 3, unlit=True, visible=False)
    assert not hidden.dev.visible
    assert _same(_gpu(mnv, torch_gpu, [hidden, far, hidden, near], cam, opt), a)
    hidden.dev.visible = True
    assert not _same(_gpu(mnv, torch_gpu, [hidden, far, near], cam, opt), a)
    # no mesh at all: the cleared images
    t, img = _gpu(mnv, torch_gpu, [], cam, _opt(mnv, 0.5))
    assert (t == F(1e9)).all() and (img == (128, 128, 128, 255)).all()


# ------------------------------------------------------------------------------------------------ 4. draw-over

def test_draw_over_the_grid_in_place(mnv, torch_gpu):
    torch = torch_gpu
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    tree.move_to_device()
    opt = cases.make_options(mnv, spec["options"])
    opt.background_brightness = 0.5
    cam = cases.make_camera(mnv, dict(spec["camera"], width=96, height=64, fx=spec["camera"]["fx"] * 96 / 200))
    v, f = uv_sphere(12, 16, 0.3)
    ball = Pair(mnv, v, f, 3, transform=((0.2, 0.1, -0.3), (0.1, 0.0, -0.1), 1.0))
    wire = mnv.Wireframe(tree.device_view(), 3)
    for tile in (None, (5, 3, 70, 45)):
        gt, gi = wire.render(cam, opt, tile)
        torch.cuda.synchronize()
        grid = (gt.cpu().numpy(), gi.cpu().numpy())
        alone = _gpu(mnv, torch, [ball], cam, opt, tile)
        mnv.render_meshes([ball.dev], cam, opt, tile, under=(gt, gi), tmax_px=gt, rgba8=gi)     # in place
        torch.cuda.synchronize()
        t, img = gt.cpu().numpy(), gi.cpu().numpy()
        assert np.array_equal(t.view(np.uint32), np.minimum(grid[0], alone[0]).view(np.uint32))
        mesh_wins = alone[0] < grid[0]
        assert mesh_wins.sum() > 200 and ((grid[0] < alone[0]) & (alone[0] != F(1e9))).sum() > 20      # both orders occur on the ball
        assert np.array_equal(img[mesh_wins], alone[1][mesh_wins]) and np.array_equal(img[~mesh_wins], grid[1][~mesh_wins])
        # ... and the restatement agrees, also with one member of `under` missing
        _assert_contract(mnv, torch, [ball], cam, opt, tile, under=grid)
        _assert_contract(mnv, torch, [ball], cam, opt, tile, under=(grid[0], None))
        _assert_contract(mnv, torch, [ball], cam, opt, tile, under=(None, grid[1]))


# ------------------------------------------------------------------------------------------------ 5. the contract

def test_contract_lit_sphere_with_a_model_matrix(mnv, torch_gpu):
    cam = _look(mnv, 96, 64, 90.0, center=(0.4, -0.3, 5.0), back=(0.1, -0.05, 0.99))
    v, f = uv_sphere(32, 33, 1.0)
    assert 2000 <= f.shape[0] <= 2100
    ball = Pair(mnv, v, f, 3, transform=((0.3, -0.5, 0.8), (0.1, -0.05, 0.2), 1.7))
    for tile in (None, (5, 3, 70, 45)):
        _assert_contract(mnv, torch_gpu, [ball], cam, _opt(mnv), tile, min_hits=1500)
    # the frame 75 x 53 with an off-centre principal point
    cam = _look(mnv, 75, 53, 70.0, cx=30.25, cy=29.5)
    _assert_contract(mnv, torch_gpu, [ball], cam, _opt(mnv), min_hits=1500)
    # indexed and non-indexed copies give identical bytes
    flat = Pair(mnv, v[f.reshape(-1)], None, 3, transform=((0.3, -0.5, 0.8), (0.1, -0.05, 0.2), 1.7))
    assert flat.dev.face_count == ball.dev.face_count == f.shape[0] and flat.dev.vertex_count == 3 * f.shape[0]
    assert _same(_gpu(mnv, torch_gpu, [flat], cam, _opt(mnv)), _gpu(mnv, torch_gpu, [ball], cam, _opt(mnv)))
    # unlit: the interpolated colour alone
    _assert_contract(mnv, torch_gpu, [Pair(mnv, v, f, 3, unlit=True, transform=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.5))], cam, _opt(mnv), min_hits=1500)


def test_contract_vertices_behind_the_camera_and_a_frame_filling_triangle(mnv, torch_gpu):
    opt = _opt(mnv)
    for w, h in ((96, 64), (75, 53)):
        cam = _look(mnv, w, h, 80.0)
        col = [(1.0, 0.2, 0.1), (0.1, 1.0, 0.3), (0.2, 0.3, 1.0)]
        n = [(0.0, 0.0, 1.0), (0.3, 0.1, 0.9), (-0.2, 0.4, 0.8)]
        # world z > 5 - 1e-3 is behind the near plane
        one = Pair(mnv, _verts([[-1.5, -1.0, 2.0], [1.6, -0.9, 1.0], [0.2, 0.9, 7.0]], col, n))
        two = Pair(mnv, _verts([[-0.4, -0.3, 3.0], [2.5, 0.4, 9.0], [-1.0, 2.0, 6.0]], col, n))
        allb = Pair(mnv, _verts([[-0.4, -0.3, 5.5], [2.5, 0.4, 9.0], [-1.0, 2.0, 6.0]], col, n))
        full = Pair(mnv, _verts([[-40.0, -30.0, -1.0], [45.0, -28.0, 0.5], [1.0, 60.0, 0.0]], col, n))
        _assert_contract(mnv, torch_gpu, [one], cam, opt, min_hits=300)
        _assert_contract(mnv, torch_gpu, [two], cam, opt, min_hits=100)
        t, _ = _assert_contract(mnv, torch_gpu, [allb], cam, opt, min_hits=0)
        assert (t == F(1e9)).all()
        t, _ = _assert_contract(mnv, torch_gpu, [full], cam, opt, min_hits=w * h)
        _assert_contract(mnv, torch_gpu, [full, one, two], cam, opt, (3, 2, w - 9, h - 7), min_hits=1000)


def test_contract_sub_pixel_triangles(mnv, torch_gpu):
    cam = _look(mnv, 96, 64, 80.0)
    rng = np.random.default_rng(5)
    n = 3000
    c = np.stack([rng.uniform(-2, 98, n), rng.uniform(-2, 66, n)], axis=1)
    Z = rng.uniform(2.0, 6.0, (n, 1))
    corners = c[:, None, :] + rng.uniform(-0.45, 0.45, (n, 3, 2))
    pos = _at(cam, corners[..., 0], corners[..., 1], Z + rng.uniform(-0.05, 0.05, (n, 3)))
    v = _verts(pos.reshape(-1, 3), rng.uniform(0, 1, (3 * n, 3)), rng.normal(size=(3 * n, 3)))
    t, _ = _assert_contract(mnv, torch_gpu, [Pair(mnv, v)], cam, _opt(mnv), min_hits=100)
    assert int((t != F(1e9)).sum()) < n // 2          # most of them cover no centre


def test_contract_six_thousand_triangles_in_one_tile(mnv, torch_gpu):
    """Tile (1, 1) of the 96 x 64 frame (pixels 32 .. 63 both ways) receives 6000 triangles: its list is walked in 24 chunks of 256, and
    triangles of 1 to 9 pixels across take both the thread-per-triangle and the shared path."""
    cam = _look(mnv, 96, 64, 80.0)
    rng = np.random.default_rng(6)
    n = 6000
    c = rng.uniform(37, 58, (n, 2))
    size = rng.uniform(0.5, 4.5, (n, 1, 1))
    corners = c[:, None, :] + size * rng.uniform(-1, 1, (n, 3, 2))
    assert corners.min() > 32 and corners.max() < 63
    pos = _at(cam, corners[..., 0], corners[..., 1], rng.uniform(2.0, 6.0, (n, 1)) + rng.uniform(-0.3, 0.3, (n, 3)))
    v = _verts(pos.reshape(-1, 3), rng.uniform(0, 1, (3 * n, 3)), rng.normal(size=(3 * n, 3)))
    idx = rng.permutation(3 * n).astype(np.uint32).reshape(-1, 3)        # indexed, vertices shared at random: slivers and large triangles too
    _assert_contract(mnv, torch_gpu, [Pair(mnv, v)], cam, _opt(mnv), min_hits=400)
    _assert_contract(mnv, torch_gpu, [Pair(mnv, v, idx[:2000])], cam, _opt(mnv), min_hits=400)


def test_contract_points_and_a_mixed_list(mnv, torch_gpu):
    cam = _look(mnv, 75, 53, 70.0)
    rng = np.random.default_rng(8)
    n = 600
    pos = _at(cam, rng.uniform(-5, 80, n), rng.uniform(-5, 58, n), rng.uniform(-1.0, 6.0, n))      # some behind the camera, some off the frame
    pos[:40] = pos[40:80]                                                                           # coincident points: the first-drawn colour
    pv = _verts(pos, rng.uniform(0, 1, (n, 3)), rng.normal(size=(n, 3)))
    for unlit in (True, False):
        t, _ = _assert_contract(mnv, torch_gpu, [Pair(mnv, pv, None, 1, unlit=unlit)], cam, _opt(mnv), min_hits=200)
    pts = Pair(mnv, pv, rng.permutation(n).astype(np.uint32)[:300], 1)
    # lit, coloured lines through the frame, some crossing the near plane
    m = 80
    a = _at(cam, rng.uniform(-20, 95, m), rng.uniform(-20, 73, m), rng.uniform(-0.5, 6.0, m))
    b = _at(cam, rng.uniform(-20, 95, m), rng.uniform(-20, 73, m), rng.uniform(1.0, 6.0, m))
    lv = _verts(np.stack([a, b], axis=1).reshape(-1, 3), rng.uniform(0, 1, (2 * m, 3)), rng.normal(size=(2 * m, 3)))
    lines = Pair(mnv, lv, None, 2, transform=((0.0, 0.0, 0.2), (0.05, 0.0, 0.0), 1.0))
    _assert_contract(mnv, torch_gpu, [lines], cam, _opt(mnv), min_hits=500)
    v, f = uv_sphere(10, 12, 0.8)
    ball = Pair(mnv, v, f, 3, transform=((0.0, 0.4, 0.0), (0.0, 0.0, 1.0), 1.0))
    for order in ([pts, lines, ball], [ball, pts, lines]):
        _assert_contract(mnv, torch_gpu, order, cam, _opt(mnv), min_hits=1500)
        _assert_contract(mnv, torch_gpu, order, cam, _opt(mnv), (7, 5, 60, 40), min_hits=1000)


def test_mesh_update_in_place_and_counts(mnv, torch_gpu):
    cam = _look(mnv, 75, 53, 70.0)
    v, f = uv_sphere(8, 9, 0.9)
    p = Pair(mnv, v, f)
    assert (p.dev.vertex_count, p.dev.face_count, p.dev.face_size) == (v.shape[0], f.shape[0], 3)
    a = _gpu(mnv, torch_gpu, [p], cam, _opt(mnv))
    v2 = v.copy()
    v2[:, 0:3] *= 0.5
    assert mnv.lib().mnv_mesh_update(p.dev._h, v2.ctypes.data, v2.shape[0], f.ctypes.data, f.size, 3, 0) == mnv.MNV_OK
    b = _gpu(mnv, torch_gpu, [p], cam, _opt(mnv))
    assert not _same(a, b) and _same(b, _gpu(mnv, torch_gpu, [Pair(mnv, v2, f)], cam, _opt(mnv)))
    assert mnv.lib().mnv_mesh_update(p.dev._h, v2.ctypes.data, v2.shape[0], f.ctypes.data, f.size - 1, 3, 0) == mnv.MNV_E_INVALID
    assert _same(b, _gpu(mnv, torch_gpu, [p], cam, _opt(mnv)))                        # a refused update leaves the mesh as it was


# ------------------------------------------------------------------------------------------------ 6. whole frames

BALL_TRANSFORM = ((0.3, -0.5, 0.8), (0.1, -0.2, 0.05), 0.55)


@pytest.fixture(scope="module")
def ball():
    return uv_sphere(24, 28, 1.0)


def _renderer(mnv, tree, spec, opt, **over):
    r = mnv.Renderer()
    cs = spec["camera"]
    r.resize(cs["width"], cs["height"])
    r.set(tree, tree.capacity)
    r.set_camera(cs["center"], cs["back"], fx=cs["fx"], up=cs.get("up", (0.0, 0.0, 1.0)))
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    for k, v in over.items():
        setattr(r.options, k, v)
    return r


def _inputs(tree, cam, opt, pairs, grid_depth=None):
    """the two images the frame must have been marched over: the restatements of the grid pass and of the mesh pass over it"""
    full = (0, 0, cam.width, cam.height)
    under = None
    if grid_depth is not None:
        under = wireframe_ref.raster(wireframe_ref.segments_from_vertices(tree.gen_wireframe(grid_depth)), cam, full, opt.background_brightness)
    return mesh_ref.render([p.ref for p in pairs], cam, full, opt.background_brightness, under)


def _scene(mnv, name):
    spec = cases.CASES[name]
    tree = cases.make_tree(mnv, spec["tree"])
    v = tree.host_view()
    opt = cases.make_options(mnv, spec["options"])
    opt.basis_minmax[0], opt.basis_minmax[1] = 0, max(v.basis_dim - 1, 0)
    return spec, tree, v, opt


@pytest.mark.parametrize("grid_depth", [None, 3])
def test_renderer_mesh_frame_equals_the_oracle(mnv, orc, torch_gpu, ball, grid_depth):
    spec, tree, v, opt = _scene(mnv, "sh9_d7_aniso")
    p = Pair(mnv, *ball, 3, transform=BALL_TRANSFORM)
    plain = orc.render(orc.tree_from_view(v), cases.make_camera(mnv, spec["camera"]).c, opt, want_rgba8=True)
    for in_flight in (1, 3):          # slot 0's path and a slot in flight
        over = dict(show_grid=True, grid_max_depth=grid_depth) if grid_depth is not None else {}
        r = _renderer(mnv, tree, spec, opt, **over)
        r.set_frames_in_flight(in_flight)
        r.add_mesh(p.dev)
        assert r.mesh_count == 1
        for f in range(2):
            st = r.render()
            f32, u8 = r.download(want_rgba8=True)
            t, img = _inputs(tree, r.last_camera(), opt, [p], grid_depth)
            want = orc.render(orc.tree_from_view(v), r.last_camera(), opt, want_rgba8=True, tmax_px=t, rgba8_init=img)
            assert st["used_accel"]
            assert np.array_equal(cases.bits(f32), cases.bits(want["rgba"])) and np.array_equal(u8, want["rgba8"]), (in_flight, f)
        assert int((cases.bits(f32) != cases.bits(plain["rgba"])).any(axis=-1).sum()) > 300      # the ball shows
        # an invisible mesh, or none: the frame without the feature, for the camera of that frame (Camera::_update renormalises v_back on
        # every call, so the matrix may move by an ulp between frames)
        for step in ("invisible", "cleared"):
            if step == "invisible":
                p.dev.visible = False
            else:
                p.dev.visible = True
                r.clear_meshes()
                assert r.mesh_count == 0
            r.render()
            g32, g8 = r.download(want_rgba8=True)
            cam = r.last_camera()
            if grid_depth is None:
                want = orc.render(orc.tree_from_view(v), cam, opt, want_rgba8=True)
            else:
                t, img = _inputs(tree, cam, opt, [], grid_depth)
                want = orc.render(orc.tree_from_view(v), cam, opt, want_rgba8=True, tmax_px=t, rgba8_init=img)
            assert np.array_equal(cases.bits(g32), cases.bits(want["rgba"])) and np.array_equal(g8, want["rgba8"]), (in_flight, step)


def test_renderer_mesh_tracker_and_guided_frames(mnv, orc, torch_gpu, ball):
    """As test_renderer_grid_tracker_and_guided_frames: the refinement frame equals the oracle's frame over the mesh pass's images; the
    guided-sampling frame, fused and four-step, equals mnv_render_guided_fused called with the mesh pass's depth image."""
    import mlp_cases
    from test_renderer_refine_gpu import make_grid
    torch = torch_gpu
    spec, tree, v, opt = _scene(mnv, "sh4_d6")
    desc = mnv.mlp_desc(n_clusters=6, pos_octaves=4, dir_octaves=2, need_viewdir=False, hidden_width=64, hidden_layers=2, out_dim=v.data_dim + 1)
    params, grid = mlp_cases.make_params(mnv, desc, seed=21), make_grid(mnv)
    p = Pair(mnv, *ball, 3, transform=BALL_TRANSFORM)
    r = _renderer(mnv, tree, spec, opt)
    r.set(tree, v.capacity * 4)
    r.set_model(desc, params, grid)
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.use_splitting, r.options.split_batch_size, r.options.max_depth = True, 64, 8
    r.add_mesh(p.dev)
    st = r.render()
    f32, u8 = r.download(want_rgba8=True)
    assert st["used_accel"] and not st["fused"]
    cam = r.last_camera()
    t, img = _inputs(tree, cam, opt, [p])
    want = orc.render(orc.tree_from_view(v), cam, opt, want_rgba8=True, tmax_px=t, rgba8_init=img)
    assert np.array_equal(cases.bits(f32), cases.bits(want["rgba"])) and np.array_equal(u8, want["rgba8"])
    tree = cases.make_tree(mnv, spec["tree"])
    for fused in (True, False):
        r = _renderer(mnv, tree, spec, opt)
        r.set_model(desc, params, grid)
        r.options.use_guided_sampling, r.options.max_guided_samples = True, 16
        r.set_fused_guided(fused)
        r.add_mesh(p.dev)
        st = r.render()
        assert bool(st["fused"]) == fused
        got = r.download()
        cam = r.last_camera()
        t, _ = _inputs(tree, cam, opt, [p])
        opt2 = mnv.RenderOptions()
        C.memmove(C.byref(opt2), C.byref(r.options), C.sizeof(opt2))
        cam_obj = mnv.Camera(cam.width, cam.height, cam.fx)
        C.memmove(C.byref(cam_obj.c), C.byref(cam), C.sizeof(cam))
        out = torch.empty((cam.height, cam.width, 4), dtype=torch.float32, device="cuda")
        mnv.render_guided_fused(tree.accel, cam_obj, opt2, mnv.Mlp(desc, params), grid, rgba=out, tmax_px=torch.from_numpy(t).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(cases.bits(got), cases.bits(out.cpu().numpy())), f"guided frame (fused {fused})"
        mnv.render_guided_fused(tree.accel, cam_obj, opt2, mnv.Mlp(desc, params), grid, rgba=out)
        torch.cuda.synchronize()
        assert (cases.bits(got) != cases.bits(out.cpu().numpy())).any()          # the mesh's depth image matters


def test_frames_in_flight_3_equal_1_with_meshes(mnv, torch_gpu, ball):
    spec, tree, v, opt = _scene(mnv, "terrain_d7_aniso")
    frames = {}
    for k in (1, 3):
        p = Pair(mnv, *ball, 3, transform=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.5))
        r = _renderer(mnv, tree, spec, opt, show_grid=True, grid_max_depth=3)
        r.set_frames_in_flight(k)
        r.add_mesh(p.dev)
        out = []
        for f in range(6):
            p.dev.set_transform((0.1 * f, 0.0, 0.2), (0.05 * f, 0.1, 0.0), 0.5 + 0.05 * f)     # the mesh moves between frames in flight
            r.options.show_grid = f != 4
            r.render()
            out.append(r.download_slot(r.last_slot(), want_rgba8=True))
        frames[k] = out
        r.clear_meshes()
    for (a, a8), (b, b8) in zip(frames[1], frames[3]):
        assert np.array_equal(cases.bits(a), cases.bits(b)) and np.array_equal(a8, b8)
    assert (cases.bits(frames[1][0][0]) != cases.bits(frames[1][5][0])).any()


def test_antialiased_mesh_frame_equals_the_resolve_of_single_frames(mnv, torch_gpu, ball):
    torch = torch_gpu
    W, H = 96, 64
    tree = mnv.N3Tree.synth_random(depth=4, basis_dim=4, seed=11)
    p = Pair(mnv, *ball, 3, transform=((0.3, 0.0, 0.2), (0.0, 0.0, 0.0), 0.6))
    for grid_depth in (None, 2):
        r = mnv.Renderer()
        r.resize(W, H)
        r.set(tree, tree.capacity)
        r.set_camera((-3.5, 0.0, 3.5), (-0.7071068, 0.0, 0.7071068), fx=150.0)
        r.options.background_brightness = 1.0
        if grid_depth is not None:
            r.options.show_grid, r.options.grid_max_depth = True, grid_depth
        r.add_mesh(p.dev)
        r.set_antialiasing(4, mnv.AA_TENT)
        r.render()
        f32, u8 = r.download(want_rgba8=True)
        off = aa_ref.pattern(4)
        lc = r.last_camera()
        wire = mnv.Wireframe(tree.device_view(), grid_depth) if grid_depth is not None else None
        sub = np.empty((4, H, W, 4), F)
        for i in range(4):
            cam = mnv.Camera(lc.width, lc.height, lc.fx)
            C.memmove(C.byref(cam.c), C.byref(lc), C.sizeof(lc))
            cam.c.cx = float(F(lc.cx) - F(off[i, 0]))
            cam.c.cy = float(F(lc.cy) - F(off[i, 1]))
            under = wire.render(cam, r.options) if wire is not None else None
            tmax, img = mnv.render_meshes([p.dev], cam, r.options, under=under)
            out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
            mnv.render_voxels_accel(tree.accel, cam, r.options, rgba=out, tmax_px=tmax, rgba8_init=img)
            torch.cuda.synchronize()
            sub[i] = out.cpu().numpy()
        table = aa_ref.weights(aa_ref.AA_TENT, off)
        want_f32, want_u8 = aa_ref.resolve(sub, table, table.shape[1] // 2)
        assert np.array_equal(cases.bits(f32), cases.bits(want_f32)) and np.array_equal(u8, want_u8), grid_depth
        assert (cases.bits(sub[0]) != cases.bits(sub[1])).any()


def test_meshes_refuse_frame_inputs_and_ranks(mnv, torch_gpu, ball):
    torch = torch_gpu
    spec, tree, v, opt = _scene(mnv, "sh4_d6")
    p = Pair(mnv, *ball, 3, transform=BALL_TRANSFORM)
    r = _renderer(mnv, tree, spec, opt)
    r.add_mesh(p.dev)
    cs = spec["camera"]
    t = torch.zeros((cs["height"], cs["width"]), dtype=torch.float32, device="cuda")
    r.set_frame_inputs(t, None)
    with pytest.raises(mnv.MnvError) as e:
        r.render()
    assert e.value.code == mnv.MNV_E_INVALID and "set_frame_inputs" in str(e.value)
    p.dev.visible = False
    r.render()                                              # an invisible mesh asks for nothing
    p.dev.visible = True
    r.set_frame_inputs(None, None)
    r.render()
    comm = mnv.Comm(mnv.comm_get_unique_id(), 1, 0)         # one rank through RCCL
    try:
        r.set_ranks(comm)
        with pytest.raises(mnv.MnvError) as e:
            r.render()
        assert e.value.code == mnv.MNV_E_INVALID and "set_ranks" in str(e.value)
        r.set_ranks(None)
        r.render()
    finally:
        r.set_ranks(None)
        comm.close()


# ------------------------------------------------------------------------------------------------ 7. the CLI

def _ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_cli_mesh(mnv, torch_gpu, tmp_path):
    spec = cases.CASES["sh4_d6"]
    tree = cases.make_tree(mnv, spec["tree"])
    path = str(tmp_path / "t.npz")
    tree.save_npz(path)
    v, f = uv_sphere(10, 12, 0.8)
    obj = tmp_path / "ball.obj"
    with open(obj, "w") as fh:
        for row in v:
            fh.write("v %.9g %.9g %.9g\n" % tuple(row[0:3]))
        for row in v:
            fh.write("vn %.9g %.9g %.9g\n" % tuple(row[6:9]))
        for a, b, c in f + 1:
            fh.write(f"f {a}//{a} {b}//{b} {c}//{c}\n")
    tri = tmp_path / "tri.obj"
    tri.write_text("v -1 -1 -0.5 1 0 0\nv 1 -1 -0.5 0 1 0\nv 0 1.2 -0.5 0 0 1\nf 1 2 3\n")
    exe = os.path.join(PKG, "mnv_render")
    base = [exe, path, "-w", "96", "-h", "80", "--fx", "150", "--in_flight", "1"]
    flags = ["--mesh", str(obj), "--mesh_color", "0.9,0.5,0.2", "--mesh_rotate", "0.2,0.3,-0.4", "--mesh_translate", "0.1,-0.2,0.3", "--mesh_scale", "0.8",
             "--mesh", str(tri) + ",unlit", "--mesh_translate", "0,0.3,0"]
    out = str(tmp_path / "m")
    res = subprocess.run(base + flags + ["--out", out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    got = _ppm(out + "_0000.ppm")
    res = subprocess.run(base + ["--out", str(tmp_path / "p")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert (got != _ppm(str(tmp_path / "p_0000.ppm"))).any(axis=-1).sum() > 200
    # the same frame through the Python renderer
    t2 = mnv.N3Tree.open(path)
    opt = mnv.RenderOptions.cli_defaults()
    r = mnv.Renderer()
    r.resize(96, 80)
    r.set(t2, t2.capacity)
    r.set_camera((-3.5, 0.0, 3.5), (-0.7071068, 0.0, 0.7071068), fx=150.0)
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    m1 = mnv.Mesh.from_obj(str(obj), color=(0.9, 0.5, 0.2))
    m1.set_transform((0.2, 0.3, -0.4), (0.1, -0.2, 0.3), 0.8)
    m2 = mnv.Mesh.from_obj(str(tri), unlit=True)
    m2.set_transform(translation=(0.0, 0.3, 0.0))
    assert m1.face_count == f.shape[0] and m2.face_count == 1
    r.add_mesh(m1)
    r.add_mesh(m2)
    r.render()
    _, u8 = r.download(want_rgba8=True)
    assert np.array_equal(u8[..., :3], got)
    res = subprocess.run([exe, path, "--mesh", str(obj), "--gpus", "1"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "--mesh" in res.stderr
    res = subprocess.run([exe, path, "--mesh_scale", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "--mesh" in res.stderr


# ------------------------------------------------------------------------------------------------ 8. one full-size frame

def test_1080p_sphere_of_20k_triangles_on_a_tile(mnv, torch_gpu):
    cam = cases.cfg2_camera(mnv)
    v, f = uv_sphere(100, 101, 0.45)
    assert 19500 <= f.shape[0] <= 20500
    p = Pair(mnv, v, f, 3, transform=((0.2, -0.1, 0.4), (0.05, 0.0, -0.02), 1.0))
    opt = mnv.RenderOptions.cli_defaults()
    full = _gpu(mnv, torch_gpu, [p], cam, opt)
    tile = (1060, 412, 256, 256)
    want = mesh_ref.render([p.ref], cam.c, tile, opt.background_brightness)
    x0, y0, w, h = tile
    got = (full[0][y0:y0 + h, x0:x0 + w], full[1][y0:y0 + h, x0:x0 + w])
    hit = want[0] != F(1e9)
    assert hit.sum() > 20000 and (~hit).sum() > 1000            # the tile straddles the ball's outline
    assert _same(got, want)
    assert _same(_gpu(mnv, torch_gpu, [p], cam, opt, tile), want)

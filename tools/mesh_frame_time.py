"""The mesh pass's cost on one GPU (1920x1080, cfg2's camera orbit): python tools/mesh_frame_time.py [--out FILE] [--reps N]

Every figure is the median over `reps` launches of the time between two HIP events around ONE call on one stream, after a warm-up call
(mnv_render_meshes waits once per call for the size of its tile lists, so the events bracket the whole pass, host wait included).
  (a) lines_ms / wireframe_ms   the grid-depth-4 edges of the cfg2 tree as a non-indexed unlit line mesh (72 bytes per segment) next to
                                mnv_render_wireframe on the same edges (16 bytes per cube), same run
  (b) quad_ms                   a full-frame quad of two triangles, lit
  (c) sphere20k_ms / sphere200k_ms   lit UV spheres of about 20 k and 200 k triangles filling a third of the frame's height
  frame_ms / frame_sphere20k_ms / frame_sphere200k_ms   a whole cfg2 frame through Renderer (frames in flight 1, a wait per frame, wall
                                clock median) without meshes and with each sphere
One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

W, H, FX = 1920, 1080, 1600.0


def median_ms(fn, reps, stream):
    fn(0)
    torch.cuda.synchronize()
    out = []
    for i in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(stream)
        fn(i)
        e.record(stream)
        e.synchronize()
        out.append(s.elapsed_time(e))
    return round(float(np.median(out)), 4)


def uv_sphere(n_lat, n_lon, radius):
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    n = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], axis=-1).reshape(-1, 3)
    v = np.concatenate([n * radius, 0.5 + 0.5 * n, n], axis=1).astype(np.float32)
    a = (np.arange(n_lat)[:, None] * n_lon + np.arange(n_lon)[None, :])
    b = (np.arange(n_lat)[:, None] * n_lon + (np.arange(n_lon)[None, :] + 1) % n_lon)
    c, d = a + n_lon, b + n_lon
    up = np.stack([a, c, b], axis=-1)[1:].reshape(-1, 3)
    down = np.stack([b, c, d], axis=-1)[:-1].reshape(-1, 3)
    return v, np.concatenate([up, down]).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tree = cases.make_tree(mnv, cases.CFG2_TREE)
    tree.move_to_device()
    cams = [cases.cfg2_camera(mnv, p, W, H, FX) for p in range(16)]
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    tmax = torch.empty((H, W), dtype=torch.float32, device="cuda")
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    line = dict(tree="cfg2", width=W, height=H, reps=a.reps)

    def covered():
        return int((tmax.cpu().numpy() != np.float32(1e9)).sum())

    # (a) the grid as a line mesh, next to the grid pass
    wire = mnv.Wireframe(tree.device_view(), 4, stream=sp)
    wire.set_method(mnv.WIREFRAME_BINNED)
    lines = mnv.Mesh(tree.gen_wireframe(4), None, 2, unlit=True)
    line.update(segments=lines.face_count)
    line["wireframe_ms"] = median_ms(lambda i: wire.render(cams[i % 16], opt, tmax_px=tmax, rgba8=img, stream=sp), a.reps, st)
    line["lines_ms"] = median_ms(lambda i: mnv.render_meshes([lines], cams[i % 16], opt, tmax_px=tmax, rgba8=img, stream=sp), a.reps, st)
    line["lines_covered_px"] = covered()
    # (b) a full-frame quad: in front of cfg2's pose-0 camera, facing it
    c2w = np.array(cams[0].c.c2w[:], np.float64)
    r, u, b, c = c2w[0:3], c2w[3:6], c2w[6:9], c2w[9:12]
    corners = [c - 2.0 * b + sx * 1.5 * r + sy * 1.0 * u for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    qv = np.zeros((4, 9), np.float32)
    qv[:, 0:3], qv[:, 3:6], qv[:, 6:9] = corners, (0.8, 0.7, 0.6), b
    quad = mnv.Mesh(qv, np.uint32([[0, 1, 2], [0, 2, 3]]))
    line["quad_ms"] = median_ms(lambda i: mnv.render_meshes([quad], cams[0], opt, tmax_px=tmax, rgba8=img, stream=sp), a.reps, st)
    line["quad_covered_px"] = covered()
    # (c) spheres
    spheres = {}
    for name, (n_lat, n_lon) in (("sphere20k", (100, 101)), ("sphere200k", (316, 317))):
        v, f = uv_sphere(n_lat, n_lon, 0.3)
        m = mnv.Mesh(v, f)
        spheres[name] = m
        line[name + "_triangles"] = m.face_count
        line[name + "_ms"] = median_ms(lambda i: mnv.render_meshes([m], cams[i % 16], opt, tmax_px=tmax, rgba8=img, stream=sp), a.reps, st)
        line[name + "_covered_px"] = covered()
    # whole frames
    for name in ("", "sphere20k", "sphere200k"):
        r = mnv.Renderer()
        r.resize(W, H)
        r.set(tree, tree.capacity)
        r.set_frames_in_flight(1)
        pose = cams[0].c
        r.set_camera(tuple(pose.c2w[9:12]), tuple(pose.c2w[6:9]), fx=FX)
        if name:
            r.add_mesh(spheres[name])
        out = []
        for i in range(a.reps + 1):
            t0 = time.perf_counter()
            r.render()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        line["frame_" + name + "_ms" if name else "frame_ms"] = round(float(np.median(out[1:])), 4)
        r.clear_meshes()
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

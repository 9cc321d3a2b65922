"""What ray lists cost on one GPU (cfg2 tree, 1920x1080): python tools/rays_bench.py [--out FILE] [--min_ms 1000]

  (a) frame_ms          mnv_render_voxels_accel_ex on the camera: the yardstick (the frame kernel, unchanged by ray lists)
  (b) generate_<p>_ms   mnv_generate_rays alone for the pinhole, orthographic and equirectangular projection: ms and bytes written over the time
  (c) rays_pinhole_ms   mnv_render_rays_accel on the pinhole rays of the same camera (the same pixels as (a), bit for bit: checked here), and
                        its ratio to (a); rays_flat_ms the same rays as a flat list (64 x 1 tiles instead of 8 x 8)
  (d) frame_<p>_<n>     whole orthographic / equirectangular frames through Renderer (generator + march) with n = 1 and n = 3 frames in flight

(a)-(c): HIP events on one stream around `reps` back-to-back calls after a warm-up, reps chosen so that every figure covers at least
--min_ms of device work; the median of five such figures.  (d): the Renderer owns its streams, so it is the wall time of `reps` render()
calls and the wait for the last frame, same rule for reps, median of five.  Prints a table and one JSON line; --out writes the table."""
import argparse, ctypes as C, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

W, H, FX = 1920, 1080, 1600.0
PEAK = 8e12
ROUNDS = 5


def events_ms(fn, reps, stream):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(reps):
        fn()
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) / reps


def measure(fn, stream, min_ms):
    for _ in range(3):
        fn()
    pilot = events_ms(fn, 5, stream)
    reps = max(10, int(math.ceil(min_ms / max(pilot, 1e-3))))
    return statistics.median(events_ms(fn, reps, stream) for _ in range(ROUNDS)), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--min_ms", type=float, default=1000.0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tree = cases.make_tree(mnv, cases.CFG2_TREE)
    tree.move_to_device()
    cam = cases.cfg2_camera(mnv, 0, W, H, FX)
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    res, rows = {}, []
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    u8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    g32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    g8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    d = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    n = W * H

    ms, reps = measure(lambda: mnv.render_voxels_accel(tree.accel, cam, opt, rgba=f32, rgba8=u8, stream=sp), st, a.min_ms)
    res["frame_ms"] = ms
    rows.append(f"(a) mnv_render_voxels_accel_ex, the camera frame     {ms:8.4f} ms   {n / ms / 1e3:7.1f} Mrays/s   reps {reps}")

    ray_bytes = 2 * n * 12
    ortho = mnv.Camera(W, H, 700.0).set_pose((2.6, 0.4, 0.3), (0.985, 0.15, 0.09))   # 700 pixels per world unit: the unit cube's shell fills the frame
    inside = mnv.Camera(W, H, FX).set_pose((0.05, 0.02, 0.01), (0.985, 0.15, 0.09))     # a panorama from inside the shell: every ray meets it
    for name, code, c in (("pinhole", mnv.PROJ_PINHOLE, cam), ("ortho", mnv.PROJ_ORTHO, ortho), ("equirect", mnv.PROJ_EQUIRECT, inside)):
        ms, reps = measure(lambda: mnv.generate_rays(code, c, origins=o, dirs=d, stream=sp), st, a.min_ms)
        res[f"generate_{name}_ms"] = ms
        rate = ray_bytes / (ms * 1e-3)
        rows.append(f"(b) mnv_generate_rays {name:<8s} ({ray_bytes / 1e6:5.1f} MB written)   {ms:8.4f} ms   {rate / 1e12:5.2f} TB/s ({rate / PEAK:5.1%} of peak)   reps {reps}")

    mnv.generate_rays(mnv.PROJ_PINHOLE, cam, origins=o, dirs=d, stream=sp)
    ms, reps = measure(lambda: mnv.render_rays_accel(tree.accel, o, d, opt, rgba=g32, rgba8=g8, stream=sp), st, a.min_ms)
    torch.cuda.synchronize()
    same = bool(torch.equal(f32.view(torch.int32), g32.view(torch.int32)) and torch.equal(u8, g8))
    res["rays_pinhole_ms"] = ms
    res["rays_equal_frame"] = same
    rows.append(f"(c) mnv_render_rays_accel, the pinhole rays          {ms:8.4f} ms   {n / ms / 1e3:7.1f} Mrays/s   {ms / res['frame_ms']:5.3f} x (a)   "
                f"pixels {'equal' if same else 'DIFFER FROM'} the frame's   reps {reps}")
    of, df = o.view(n, 3), d.view(n, 3)
    ms, reps = measure(lambda: mnv.render_rays_accel(tree.accel, of, df, opt, rgba=g32, rgba8=g8, stream=sp), st, a.min_ms)
    torch.cuda.synchronize()
    res["rays_flat_ms"] = ms
    res["rays_flat_equal_frame"] = bool(torch.equal(f32.view(torch.int32), g32.view(torch.int32)))
    rows.append(f"(c) ... the same rays as a flat list (64 x 1 tiles)   {ms:8.4f} ms   {n / ms / 1e3:7.1f} Mrays/s   {ms / res['frame_ms']:5.3f} x (a)   reps {reps}")

    for name, code, c in (("ortho", mnv.PROJ_ORTHO, ortho), ("equirect", mnv.PROJ_EQUIRECT, inside)):
        for k in (1, 3):
            r = mnv.Renderer()
            r.resize(W, H)
            r.set(tree, tree.capacity)
            bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
            C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
            r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
            c2w = c.c2w
            r.set_camera(tuple(c2w[9:12]), tuple(c2w[6:9]), up=(0.0, 0.0, 1.0), fx=float(c.c.fx))
            r.set_frames_in_flight(k)
            r.set_projection(code)

            def run(reps):
                t0 = time.perf_counter()
                for _ in range(reps):
                    r.render()
                for s in range(k):
                    try:
                        r.download_slot(s)
                    except mnv.MnvError:
                        pass
                return (time.perf_counter() - t0) * 1e3 / reps

            run(3)
            pilot = run(5)
            reps = max(10, int(math.ceil(a.min_ms / pilot)))
            ms = statistics.median(run(reps) for _ in range(ROUNDS))
            hit = float((torch.from_numpy(r.download())[..., 3] > 0).float().mean())
            res[f"frame_{name}_{k}_ms"] = ms
            rows.append(f"(d) Renderer {name:<8s} frame, {k} in flight            {ms:8.4f} ms wall per frame (generator + march; the last download included; "
                        f"{hit:4.0%} of the pixels see the shell)   reps {reps}")
            del r
    head = f"ray lists on the cfg2 tree, {W}x{H}, {torch.cuda.get_device_name(0)}; peak = 8 TB/s; every figure the median of {ROUNDS} over >= {a.min_ms:.0f} ms of work each"
    text = "\n".join([head] + rows)
    print(text)
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

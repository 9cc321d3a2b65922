"""The grid overlay's cost on one GPU (cfg2 tree, 1920x1080, grid depths 4 and 10 = every leaf): python tools/grid_frame_time.py [--out FILE]

  raster_<method>_ms   mnv_render_wireframe alone, warm, HIP events around `reps` calls on one stream (16 orbit poses), for each raster
                       method: binned (pairs per 32x32 tile, LDS resolve) and global (64-bit atomicMin per fragment into a key image)
  live_call_ms         the reference's literal per-frame call (bench.py's `live_call` on the packed accel): clear the image to the background
                       and the depth image to 1e9, fill both trackers with -1, the tracker march with offscreen == false; one stream, a wait
                       per frame
  live_call_grid_ms    the same frame with the grid pass (auto method) writing the image and the depth image instead of the two clears
  regen_ms             mnv_wireframe_update of the whole tree (wall, includes one wait per tree level); regen_after_split_ms: the same after
                       512 leaves of the deepest chunk level were given children (as mnv_add_children_and_generate_samples appends them)
One JSON line per grid depth."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

W, H, FX = 1920, 1080, 1600.0


def timed(fn, n, stream):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for i in range(n):
        fn(i)
    e.record(stream)
    e.synchronize()
    return s.elapsed_time(e) / n


def chunk_levels(child, cap):
    """Level of every chunk (root 0), from the child links."""
    lvl = np.full(cap, -1, np.int64)
    nodes, d = np.zeros(1, np.int64), 0
    while nodes.size:
        lvl[nodes] = d
        ch = child[nodes]
        nodes = (nodes[:, None] + ch)[ch != 0]
        d += 1
    return lvl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tree = cases.make_tree(mnv, cases.CFG2_TREE)
    cap = tree.capacity
    tree.move_to_device(max_capacity=cap + 8 * 512, need_parent=True, need_sample_counts=True)
    dv = tree.device_view()
    cams = [cases.cfg2_camera(mnv, p, W, H, FX) for p in range(16)]
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    tmax = torch.empty((H, W), dtype=torch.float32, device="cuda")
    img = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    split = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    sample = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
    counts = torch.from_numpy(tree.host_arrays()[1].copy() * 0 + 8).to(torch.int16).cuda()
    c = int(np.floor(np.float32(min(max(opt.background_brightness, 0.0), 1.0)) * np.float32(255) + np.float32(0.5)))
    clear_word = int(np.array([c | c << 8 | c << 16 | 255 << 24], np.uint32).view(np.int32)[0])
    lines = []
    for depth in (4, 10):
        t0 = time.perf_counter()
        w = mnv.Wireframe(dv, depth, stream=sp)
        regen_first = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        w.update(dv, depth, stream=sp)
        regen = (time.perf_counter() - t0) * 1e3
        raster = lambda i: w.render(cams[i % 16], opt, tmax_px=tmax, rgba8=img, stream=sp)
        line = dict(tree="cfg2", capacity=cap, width=W, height=H, grid_depth=depth, cubes=w.cube_count, segments=w.cube_count * 12)
        for name, method in (("binned", mnv.WIREFRAME_BINNED), ("global", mnv.WIREFRAME_GLOBAL)):
            w.set_method(method)
            raster(0)
            torch.cuda.synchronize()
            line[f"raster_{name}_ms"] = round(timed(raster, a.reps, st), 4)
        w.set_method(mnv.WIREFRAME_AUTO)
        line["covered_px_pose15"] = int((tmax.cpu().numpy() != np.float32(1e9)).sum())

        def frame(i, grid):
            if grid:
                raster(i)
            else:
                img.view(torch.int32).fill_(clear_word)
                tmax.fill_(1e9)
            split.fill_(-1)
            sample.fill_(-1)
            mnv.render_voxels_accel_visit(tree.accel, cams[i % 16], opt, None, None, rgba8=img, split_track=split, sample_track=sample,
                                          sample_counts=counts, stream=sp, tmax_px=tmax, rgba8_init=img)
            st.synchronize()

        for g in (False, True):
            frame(0, g)
            t0 = time.perf_counter()
            for i in range(a.reps):
                frame(i, g)
            line["live_call_grid_ms" if g else "live_call_ms"] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
        line.update(regen_create_ms=round(regen_first, 2), regen_ms=round(regen, 2))
        lines.append(line)
        del w
    # regeneration after a split: 512 leaves of the deepest chunk level get a child chunk each
    host_child = tree.host_arrays()[1][:cap]
    lvl = chunk_levels(host_child, cap)
    deepest = np.flatnonzero(lvl == lvl.max())
    slots = np.argwhere(host_child[deepest] == 0)[:512]
    new = np.zeros((cap + len(slots), 8), np.int32)
    new[:cap] = host_child
    for n, (row, c8) in enumerate(slots):
        chunk = deepest[row]
        new[chunk, c8] = cap + n - chunk
    torch_child = torch.from_numpy(new.reshape(-1)).cuda()
    v2 = mnv.TreeView()
    C.memmove(C.byref(v2), C.byref(dv), C.sizeof(dv))
    v2.child = torch_child.data_ptr()
    v2.capacity = cap + len(slots)
    for line in lines:
        w = mnv.Wireframe(dv, line["grid_depth"], stream=sp)
        t0 = time.perf_counter()
        w.update(v2, line["grid_depth"], stream=sp)
        line["regen_after_split_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        line["cubes_after_split"] = w.cube_count
        line["split_chunk_level"] = int(lvl.max())
        del w
    text = "\n".join(json.dumps(l) for l in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""What a level of detail costs and buys on one GPU: python tools/lod_bench.py [--out FILE] [--reps 5] [--trees cfg2,cfg3] [--depths 10,9,8,7]

For cfg2's depth-10 shell and the cfg3 terrain of bench.py (tests/cases.py: CFG2_TREE, CFG3_FULL), one process per tree:
  mip ms        host clock around mnv_tree_mip_rows (the call waits for the stream: the level walk with one wait per level, one launch per
                depth, the scratch allocation), median over the reps; next to it a device-to-device copy of as many bytes as the tree's
                `data` array (HIP events around torch's copy_): the pass reads and writes about those bytes once
  truncate ms   HIP events around mnv_tree_truncate at each depth (the scan, the topology pass, the row gather), median over the reps
  frame ms      plain 1080p frames through Renderer (three in flight, the 16-pose orbit / the aerial poses of bench.py), host clock around
                `frames` render() calls ending in a device synchronise, for the full tree and for each depth in the same run, alternating
  psnr          of each depth's frame at pose 0 against the full tree's frame at pose 0, through Renderer.set_target (METRIC_QUANTISED)
  accel bytes   mnv_accel_device_bytes of the truncated tree's accel, chunks of the truncated tree
Every step is a child process under its own `timeout`; the driver itself never opens the GPU and stops at the first step that fails, is
killed or times out.  Prints a table and one JSON line per step; --out writes the table."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STEP_TIMEOUT_S = 540
W, H = 1920, 1080


def _events_ms(torch, fn, reps):
    out = []
    for _ in range(reps + 1):                               # the first round warms up and is dropped
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:])


def step(tree_name, depths, reps, frames):
    import torch, cases, mega_nerf_viewer_amd as mnv

    torch.cuda.set_device(0)
    spec = {"cfg2": cases.CFG2_TREE, "cfg3": cases.CFG3_FULL}[tree_name]
    camera = {"cfg2": cases.cfg2_camera, "cfg3": cases.cfg3_camera}[tree_name]
    note = lambda text: print(f"[{tree_name}] {text}", file=sys.stderr, flush=True)  # noqa: E731
    tree = cases.make_tree(mnv, spec)
    note(f"tree built: {tree.capacity} chunks")
    r = mnv.Renderer()
    r.resize(W, H)
    r.set(tree, tree.capacity)                              # uploads the tree: parent, sample counts, the packed accel
    dv = tree.device_view()
    cap, dd = dv.capacity, dv.data_dim
    data_bytes = cap * 16 * dd
    res = {"tree": tree_name, "chunks": cap, "data_bytes": data_bytes, "device": torch.cuda.get_device_name(0), "reps": reps, "frames": frames,
           "full_accel_bytes": int(mnv.lib().mnv_accel_device_bytes(tree.accel))}

    # 1. the mip pass next to a copy of the same bytes
    mipped = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    depth_t = torch.empty((cap,), dtype=torch.int32, device="cuda")
    scratch = torch.empty_like(mipped)
    mip_ms, counts = [], None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = mnv.tree_mip_rows(dv, mipped, depth_t)
        mip_ms.append((time.perf_counter() - t0) * 1e3)
    note("mip pass timed")
    res["mip_ms"] = statistics.median(mip_ms[1:])
    res["mip_ms_min"], res["mip_ms_max"] = min(mip_ms[1:]), max(mip_ms[1:])
    res["copy_ms"] = _events_ms(torch, lambda: scratch.copy_(mipped), reps)
    res["levels"] = int(max(d for d in range(24) if counts[d]))
    res["chunks_at_depth"] = [int(x) for x in counts[:res["levels"] + 1]]
    del scratch

    # 2. truncation at each depth (the rows to carry are the mipped ones)
    view = mnv.TreeView()
    import ctypes as C
    C.memmove(C.byref(view), C.byref(dv), C.sizeof(view))
    view.data = mipped.data_ptr()
    res["truncate"] = {}
    for d in depths:
        n = int(counts[1:d + 1].sum())
        o_child = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        o_data = torch.empty((n, 8, dd), dtype=torch.int16, device="cuda")
        o_parent = torch.empty((n,), dtype=torch.int32, device="cuda")
        o_sc = torch.empty((n, 8), dtype=torch.int16, device="cuda")
        ms = _events_ms(torch, lambda: mnv.tree_truncate(view, depth_t, d, n, o_child, o_data, o_parent, o_sc), reps)
        res["truncate"][str(d)] = {"ms": ms, "chunks": n}
        del o_child, o_data, o_parent, o_sc
    del mipped, depth_t
    note("truncation timed")

    # 3. frames, 4. psnr, 5. accel bytes
    opt = mnv.RenderOptions.cli_defaults()
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    r.set_frames_in_flight(3)
    poses = [camera(mnv, p, W, H) for p in range(16)]

    world_up = {"cfg2": (0.0, 0.0, 1.0), "cfg3": (1.0, 0.0, 0.0)}[tree_name]

    def pose(p):
        c2w = poses[p % 16].c2w
        cam = poses[p % 16].c
        r.set_camera(tuple(c2w[9:12]), tuple(c2w[6:9]), up=world_up, fx=cam.fx, fy=cam.fy)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(n):
            pose(f)
            r.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    levels = [0] + list(depths)
    times = {d: [] for d in levels}
    for d in levels:                                        # builds each truncated tree, warms each shape up
        r.set_lod(d)
        run(6)
    for i in range(reps):
        note(f"frames, round {i}")
        for d in levels:                                    # alternating
            r.set_lod(d)
            times[d].append(run(frames))
    res["frame_ms"] = {str(d): statistics.median(times[d]) for d in levels}
    res["frame_ms_spread"] = {str(d): [min(times[d]), max(times[d])] for d in levels}
    r.set_frames_in_flight(1)
    r.set_lod(0)
    pose(0)
    r.render()
    _, full8 = r.download(want_rgba8=True)
    target = torch.from_numpy(full8).cuda()
    r.set_target(target, mnv.METRIC_QUANTISED)
    res["psnr"], res["accel_bytes"] = {}, {}
    for d in depths:
        r.set_lod(d)
        pose(0)
        r.render()
        res["psnr"][str(d)] = r.metrics()["psnr"]
    r.set_target(None)
    r.set_lod(0)
    for d in depths:
        cut = tree.make_lod(d)
        res["accel_bytes"][str(d)] = int(mnv.lib().mnv_accel_device_bytes(cut.accel))
        del cut
    print("STEP " + json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--trees", default="cfg2,cfg3")
    ap.add_argument("--depths", default="10,9,8,7")
    ap.add_argument("--step", default="", help="internal: TREE, run in this process")
    a = ap.parse_args()
    depths = [int(x) for x in a.depths.split(",")]
    if a.step:
        return step(a.step, depths, a.reps, a.frames)
    rows = []
    for name in a.trees.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", name, "--depths", a.depths, "--reps", str(a.reps),
               "--frames", str(a.frames)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)      # (the step's progress lines go to stderr as they come)
        line = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
        if p.returncode != 0 or not line:
            print(f"step {name} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}")
            return 1
        print(line[0], flush=True)
        m = json.loads(line[0][5:])
        gb = m["data_bytes"] / 1e9
        rows.append(f"{name}: {m['chunks']} chunks, {m['levels']} levels, rows {gb:.3f} GB, accel {m['full_accel_bytes'] / 1e9:.3f} GB, {m['device']}; medians over {m['reps']} rounds")
        rows.append(f"  mnv_tree_mip_rows {m['mip_ms']:8.3f} ms [{m['mip_ms_min']:.3f} .. {m['mip_ms_max']:.3f}] (call, host clock)   copy of the same bytes {m['copy_ms']:8.3f} ms "
                    f"({2 * gb / m['copy_ms'] * 1e3:.0f} GB/s read + written)   mip / copy {m['mip_ms'] / m['copy_ms']:.2f}")
        rows.append(f"  full tree: frame {m['frame_ms']['0']:.3f} ms [{m['frame_ms_spread']['0'][0]:.3f} .. {m['frame_ms_spread']['0'][1]:.3f}]")
        for d in depths:
            k = str(d)
            rows.append(f"  depth {d:2d}: {m['truncate'][k]['chunks']:9d} chunks   truncate {m['truncate'][k]['ms']:8.3f} ms   frame {m['frame_ms'][k]:.3f} ms "
                        f"[{m['frame_ms_spread'][k][0]:.3f} .. {m['frame_ms_spread'][k][1]:.3f}]   psnr against the full tree {m['psnr'][k]:.2f} dB   "
                        f"accel {m['accel_bytes'][k] / 1e9:.3f} GB")
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

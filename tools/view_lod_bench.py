"""What a view-dependent cut costs and buys on one GPU, beside the uniform levels of tools/lod_bench.py:
python tools/view_lod_bench.py [--out FILE] [--reps 3] [--frames 32] [--trees cfg2,cfg3] [--pixels 0.5,1,2,4] [--depths 10,9,8,7]

For cfg2's depth-10 shell and the cfg3 terrain of bench.py (tests/cases.py: CFG2_TREE, CFG3_FULL), one process per tree.  The views are the
eyes of bench.py's 16 poses (the orbit / the aerial poses) with focal length max(fx, fy).  Per `pixels` value:
  select ms     HIP events around mnv_tree_select_cut (the level walk over kept chunks with one wait per level), median over the reps
  cut ms        HIP events around mnv_tree_cut (the scan, the topology pass, the row gather), median over the reps
  kept          kept chunks per depth
  accel bytes   mnv_accel_device_bytes of the cut tree's accel
  frame ms      plain 1080p frames through Renderer (three in flight, the 16 poses in turn), host clock around `frames` render() calls ending in
                a device synchronise; the full tree, every uniform depth and every `pixels` value in the same run, alternating, each after
                warm-up frames (a switch between view cuts rebuilds the tree: that is outside the timed window)
  psnr          of the frame at each of the 16 poses against the full tree's frame at that pose, through Renderer.set_target
                (METRIC_QUANTISED): mean and minimum over the poses
and the same frame ms / psnr / accel bytes for each uniform depth (Renderer.set_lod), so that a cut can be read against the depth of about
the same accel size.  Every step is a child process under its own `timeout`; the driver itself never opens the GPU and stops at the first
step that fails, is killed or times out.  Prints a table and one JSON line per step; --out writes the table."""
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


def step(tree_name, pixels, depths, reps, frames):
    import ctypes as C
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
    poses = [camera(mnv, p, W, H) for p in range(16)]
    views = [(tuple(float(x) for x in c.c2w[9:12]), float(max(c.c.fx, c.c.fy))) for c in poses]
    res = {"tree": tree_name, "chunks": cap, "device": torch.cuda.get_device_name(0), "reps": reps, "frames": frames,
           "full_accel_bytes": int(mnv.lib().mnv_accel_device_bytes(tree.accel)), "select_ms": {}, "cut_ms": {}, "kept": {}, "accel_bytes": {}}

    # 1. select_cut and cut per `pixels` (the rows to carry are the mipped ones), accel bytes per setting
    mipped = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    counts = mnv.tree_mip_rows(dv, mipped)
    res["levels"] = int(max(d for d in range(24) if counts[d]))
    res["chunks_at_depth"] = [int(x) for x in counts[:res["levels"] + 1]]
    view = mnv.TreeView()
    C.memmove(C.byref(view), C.byref(dv), C.sizeof(view))
    view.data = mipped.data_ptr()
    keep = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    for p in pixels:
        k = f"px{p:g}"
        kept = [None]

        def select():
            kept[0] = mnv.tree_select_cut(view, views, p, 1, 23, keep)

        res["select_ms"][k] = _events_ms(torch, select, reps)
        n = int(kept[0].sum())
        res["kept"][k] = [int(x) for x in kept[0][:res["levels"] + 1]]
        o_child = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        o_data = torch.empty((n, 8, dd), dtype=torch.int16, device="cuda")
        o_parent = torch.empty((n,), dtype=torch.int32, device="cuda")
        o_sc = torch.empty((n, 8), dtype=torch.int16, device="cuda")
        res["cut_ms"][k] = _events_ms(torch, lambda: mnv.tree_cut(view, keep, n, o_child, o_data, o_parent, o_sc), reps)
        del o_child, o_data, o_parent, o_sc
        cut = tree.make_view_lod(views, p)
        assert cut.capacity == n
        res["accel_bytes"][k] = int(mnv.lib().mnv_accel_device_bytes(cut.accel))
        del cut
    del mipped, keep
    for d in depths:
        cut = tree.make_lod(d)
        res["kept"][f"d{d}"] = [int(x) for x in counts[:d + 1]]
        res["accel_bytes"][f"d{d}"] = int(mnv.lib().mnv_accel_device_bytes(cut.accel))
        del cut
    note("select_cut and cut timed")

    # 2. frames and psnr: the full tree, every uniform depth, every `pixels`
    opt = mnv.RenderOptions.cli_defaults()
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    world_up = {"cfg2": (0.0, 0.0, 1.0), "cfg3": (1.0, 0.0, 0.0)}[tree_name]

    def pose(p):
        c2w = poses[p % 16].c2w
        cam = poses[p % 16].c
        r.set_camera(tuple(c2w[9:12]), tuple(c2w[6:9]), up=world_up, fx=cam.fx, fy=cam.fy)

    def choose(setting):
        kind, value = setting
        r.set_lod(value if kind == "d" else 0)
        r.set_view_lod(views if kind == "px" else [], value if kind == "px" else 1.0)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(n):
            pose(f)
            r.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    settings = [("full", 0)] + [("d", d) for d in depths] + [("px", p) for p in pixels]
    name = lambda s: "full" if s[0] == "full" else f"{s[0]}{s[1]:g}"  # noqa: E731
    r.set_frames_in_flight(3)
    times = {name(s): [] for s in settings}
    for i in range(reps):
        note(f"frames, round {i}")
        for s in settings:                                   # alternating
            choose(s)
            run(6)                                           # builds the tree where the setting changed it, warms the shape up
            times[name(s)].append(run(frames))
    res["frame_ms"] = {k: statistics.median(v) for k, v in times.items()}
    res["frame_ms_spread"] = {k: [min(v), max(v)] for k, v in times.items()}
    r.set_frames_in_flight(1)
    choose(("full", 0))
    targets = []
    for p in range(16):
        pose(p)
        r.render()
        _, full8 = r.download(want_rgba8=True)
        targets.append(torch.from_numpy(full8).cuda())
    res["psnr_mean"], res["psnr_min"] = {}, {}
    for s in settings[1:]:
        choose(s)
        vals = []
        for p in range(16):
            r.set_target(targets[p], mnv.METRIC_QUANTISED)
            pose(p)
            r.render()
            vals.append(r.metrics()["psnr"])
        r.set_target(None)
        res["psnr_mean"][name(s)], res["psnr_min"][name(s)] = statistics.mean(vals), min(vals)
    choose(("full", 0))
    print("STEP " + json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--trees", default="cfg2,cfg3")
    ap.add_argument("--pixels", default="0.5,1,2,4")
    ap.add_argument("--depths", default="10,9,8,7")
    ap.add_argument("--step", default="", help="internal: TREE, run in this process")
    a = ap.parse_args()
    pixels, depths = [float(x) for x in a.pixels.split(",")], [int(x) for x in a.depths.split(",")]
    if a.step:
        return step(a.step, pixels, depths, a.reps, a.frames)
    rows = []
    for tree in a.trees.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", tree, "--pixels", a.pixels, "--depths", a.depths,
               "--reps", str(a.reps), "--frames", str(a.frames)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)      # (the step's progress lines go to stderr as they come)
        line = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
        if p.returncode != 0 or not line:
            print(f"step {tree} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}")
            return 1
        print(line[0], flush=True)
        m = json.loads(line[0][5:])
        rows.append(f"{tree}: {m['chunks']} chunks {m['chunks_at_depth'][1:]}, accel {m['full_accel_bytes'] / 1e9:.3f} GB, {m['device']}; 16 views; medians over {m['reps']} rounds")
        rows.append(f"  full tree : frame {m['frame_ms']['full']:.3f} ms [{m['frame_ms_spread']['full'][0]:.3f} .. {m['frame_ms_spread']['full'][1]:.3f}]")
        for k in [f"d{d}" for d in depths] + [f"px{p:g}" for p in pixels]:
            label = f"depth {k[1:]:>4s}" if k[0] == "d" else f"pixels {k[2:]:>3s}"
            cost = f"   select {m['select_ms'][k]:7.3f} ms   cut {m['cut_ms'][k]:7.3f} ms" if k in m["select_ms"] else ""
            rows.append(f"  {label}: {sum(m['kept'][k]):9d} chunks   accel {m['accel_bytes'][k] / 1e9:.3f} GB   frame {m['frame_ms'][k]:.3f} ms "
                        f"[{m['frame_ms_spread'][k][0]:.3f} .. {m['frame_ms_spread'][k][1]:.3f}]   psnr against the full tree: mean {m['psnr_mean'][k]:.2f} dB, "
                        f"min {m['psnr_min'][k]:.2f} dB{cost}")
            if k[0] == "p":
                rows.append(f"              kept per depth {m['kept'][k][1:]}")
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

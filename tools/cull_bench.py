"""What culling a tree to a pose set costs and buys on one GPU (csrc/mnv_visibility.hip; N3Tree.make_culled, Renderer.set_cull):
python tools/cull_bench.py [--out FILE] [--reps 3] [--frames 32] [--trees cfg2,cfg3,fog] [--thresholds 0,1e-3,1e-2,1e-1]

For cfg2's depth-10 shell, the cfg3 terrain and the fog shell of bench.py (tests/cases.py: CFG2_TREE, CFG3_FULL, FOG_TREE), one process per
tree.  The tree is culled with the EVEN poses of bench.py's 16 and scored on the even and on the ODD poses: a tree culled to views can
only lose on views it was not shown, so the held-out number is the honest one.
  visibility ms  HIP events around mnv_rays_visibility on the 1080p rays of pose 0: into a cleared wmax (`first`: every sample takes its
                 atomic) and after all eight poses went in (`later`: the plain load skips nearly all of them); beside them
                 mnv_render_rays_accel on the same rays.  Medians over the reps after a warm-up round.
  cull / cut ms  HIP events around mnv_tree_cull and mnv_tree_cut at the second threshold, beside mnv_tree_mip_rows on the same tree
  per threshold  kept chunks per depth, accel bytes, plain 1080p frame time through Renderer (three in flight, the 16 poses in turn, host
                 clock around `frames` render() calls ending in a device synchronise; the full tree and every threshold in the same
                 process, alternating, each after warm-up frames), psnr against the full tree's frame through Renderer.set_target
                 (METRIC_QUANTISED): mean and minimum over the even and over the odd poses
Every step is a child process under its own `timeout`; the driver itself never opens the GPU and stops at the first step that fails, is
killed or times out.  Prints a table and one JSON line per step; --out writes the table."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STEP_TIMEOUT_S = 540
W, H = 1920, 1080


def _events_ms(torch, fn, reps, before=None):
    out = []
    for _ in range(reps + 1):                               # the first round warms up and is dropped
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:])


def step(tree_name, thresholds, reps, frames):
    import ctypes as C
    import torch, cases, mega_nerf_viewer_amd as mnv

    torch.cuda.set_device(0)
    spec = {"cfg2": cases.CFG2_TREE, "cfg3": cases.CFG3_FULL, "fog": cases.FOG_TREE}[tree_name]
    camera = cases.cfg3_camera if tree_name == "cfg3" else cases.cfg2_camera
    note = lambda text: print(f"[{tree_name}] {text}", file=sys.stderr, flush=True)  # noqa: E731
    tree = cases.make_tree(mnv, spec)
    note(f"tree built: {tree.capacity} chunks")
    r = mnv.Renderer()
    r.resize(W, H)
    r.set(tree, tree.capacity)                              # uploads the tree: parent, sample counts, the packed accel
    opt = mnv.RenderOptions.cli_defaults()
    bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
    C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
    r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
    dv = tree.device_view()
    cap, dd = dv.capacity, dv.data_dim
    poses = [camera(mnv, p, W, H) for p in range(16)]
    even = poses[0::2]
    res = {"tree": tree_name, "chunks": cap, "device": torch.cuda.get_device_name(0), "reps": reps, "frames": frames,
           "full_accel_bytes": int(mnv.lib().mnv_accel_device_bytes(tree.accel))}

    # 1. the visibility march per 1080p view, beside the tuned ray march on the same rays
    wmax = torch.zeros((cap * 8,), dtype=torch.int32, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    o, d = mnv.generate_rays(mnv.PROJ_PINHOLE, even[0])
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    vis = lambda: mnv.rays_visibility(dv, o, d, r.options, wmax, sums)  # noqa: E731
    res["vis_first_ms"] = _events_ms(torch, vis, reps, before=lambda: wmax.zero_())
    wmax.zero_()
    sums.zero_()
    for c in even:
        oc, dc = mnv.generate_rays(mnv.PROJ_PINHOLE, c)
        mnv.rays_visibility(dv, oc, dc, r.options, wmax, sums)
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    res["rays"], res["samples"], res["skipped"] = int(s[0]), int(s[2]), int(s[3])
    res["words_set"] = int((wmax != 0).sum().item())
    res["vis_later_ms"] = _events_ms(torch, vis, reps)
    res["rays_accel_ms"] = _events_ms(torch, lambda: mnv.render_rays_accel(tree.accel, o, d, r.options, rgba=rgba), reps)
    del oc, dc, rgba
    note("visibility timed")

    # 2. the cull and the cut at one threshold, beside the mip pass
    rows = torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda")
    keep = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    at_depth = [None]

    def mip():
        at_depth[0] = mnv.tree_mip_rows(dv, rows)

    res["mip_ms"] = _events_ms(torch, mip, reps)
    res["levels"] = int(max(k for k in range(24) if at_depth[0][k]))
    res["chunks_at_depth"] = [int(x) for x in at_depth[0][:res["levels"] + 1]]
    th = thresholds[min(1, len(thresholds) - 1)]
    kept = [None]

    def cull():
        kept[0] = mnv.tree_cull(dv, wmax, th, rows, keep)[0]

    res["cull_ms"] = _events_ms(torch, cull, reps)
    n = int(kept[0].sum())
    view = mnv.TreeView()
    C.memmove(C.byref(view), C.byref(dv), C.sizeof(view))
    view.data = rows.data_ptr()
    o_child = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    o_data = torch.empty((n, 8, dd), dtype=torch.int16, device="cuda")
    res["cut_ms"] = _events_ms(torch, lambda: mnv.tree_cut(view, keep, n, o_child, o_data), reps)
    res["cull_cut_thresh"] = th
    del rows, keep, o_child, o_data, wmax, o, d
    note("cull and cut timed")

    # 3. per threshold: sizes, frames, psnr on the poses shown and on the poses held out
    res["kept"], res["counts"], res["accel_bytes"] = {}, {}, {}
    for th in thresholds:
        cut, kept_d, counts = tree.make_culled(even, r.options, th)
        res["kept"][f"{th:g}"] = [int(x) for x in kept_d[:res["levels"] + 1]]
        res["counts"][f"{th:g}"] = counts
        res["accel_bytes"][f"{th:g}"] = int(mnv.lib().mnv_accel_device_bytes(cut.accel))
        del cut
    world_up = (1.0, 0.0, 0.0) if tree_name == "cfg3" else (0.0, 0.0, 1.0)

    def pose(p):
        c2w, cam = poses[p % 16].c2w, poses[p % 16].c
        r.set_camera(tuple(c2w[9:12]), tuple(c2w[6:9]), up=world_up, fx=cam.fx, fy=cam.fy)

    def choose(th):
        r.set_cull([] if th is None else even, 0.0 if th is None else th)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(n):
            pose(f)
            r.render()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    settings = [None] + list(thresholds)
    name = lambda th: "full" if th is None else f"{th:g}"  # noqa: E731
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
    choose(None)
    targets = []
    for p in range(16):
        pose(p)
        r.render()
        _, full8 = r.download(want_rgba8=True)
        targets.append(torch.from_numpy(full8).cuda())
    res["psnr_shown"], res["psnr_held_out"] = {}, {}
    for th in thresholds:
        choose(th)
        vals = []
        for p in range(16):
            r.set_target(targets[p], mnv.METRIC_QUANTISED)
            pose(p)
            r.render()
            vals.append(r.metrics()["psnr"])
        r.set_target(None)
        res["psnr_shown"][name(th)] = [statistics.mean(vals[0::2]), min(vals[0::2])]
        res["psnr_held_out"][name(th)] = [statistics.mean(vals[1::2]), min(vals[1::2])]
    choose(None)
    print("STEP " + json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--trees", default="cfg2,cfg3,fog")
    ap.add_argument("--thresholds", default="0,1e-3,1e-2,1e-1")
    ap.add_argument("--step", default="", help="internal: TREE, run in this process")
    a = ap.parse_args()
    thresholds = [float(x) for x in a.thresholds.split(",")]
    if a.step:
        return step(a.step, thresholds, a.reps, a.frames)
    rows = []
    for tree in a.trees.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", tree, "--thresholds", a.thresholds,
               "--reps", str(a.reps), "--frames", str(a.frames)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)      # (the step's progress lines go to stderr as they come)
        line = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
        if p.returncode != 0 or not line:
            print(f"step {tree} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}")
            return 1
        print(line[0], flush=True)
        m = json.loads(line[0][5:])
        rows.append(f"{tree}: {m['chunks']} chunks {m['chunks_at_depth'][1:]}, accel {m['full_accel_bytes'] / 1e9:.3f} GB, {m['device']}; culled with the 8 even poses; "
                    f"medians over {m['reps']} rounds")
        rows.append(f"  mnv_rays_visibility per 1080p view: first {m['vis_first_ms']:.3f} ms, later {m['vis_later_ms']:.3f} ms; mnv_render_rays_accel on the same rays "
                    f"{m['rays_accel_ms']:.3f} ms; 8 views: {m['rays']} rays, {m['samples']} samples, {m['skipped']} skipped, {m['words_set']} words set")
        rows.append(f"  mnv_tree_cull {m['cull_ms']:.3f} ms, mnv_tree_cut {m['cut_ms']:.3f} ms (weight_thresh {m['cull_cut_thresh']:g}); mnv_tree_mip_rows {m['mip_ms']:.3f} ms")
        rows.append(f"  full tree  : frame {m['frame_ms']['full']:.3f} ms [{m['frame_ms_spread']['full'][0]:.3f} .. {m['frame_ms_spread']['full'][1]:.3f}]")
        for th in thresholds:
            k = f"{th:g}"
            c = m["counts"][k]
            rows.append(f"  thresh {k:>5s}: {sum(m['kept'][k]):9d} chunks   accel {m['accel_bytes'][k] / 1e9:.3f} GB   frame {m['frame_ms'][k]:.3f} ms "
                        f"[{m['frame_ms_spread'][k][0]:.3f} .. {m['frame_ms_spread'][k][1]:.3f}]   psnr against the full tree: shown poses mean {m['psnr_shown'][k][0]:.2f} dB, "
                        f"min {m['psnr_shown'][k][1]:.2f} dB; held-out poses mean {m['psnr_held_out'][k][0]:.2f} dB, min {m['psnr_held_out'][k][1]:.2f} dB")
            rows.append(f"                kept per depth {m['kept'][k][1:]}; leaves seen {c['leaves_seen']}, non-empty leaves culled {c['leaves_culled']}, dead chunks {c['dead_chunks']}")
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

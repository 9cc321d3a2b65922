"""What Adam and ray batches cost and buy on one GPU (1920x1080): python tools/fit_adam_bench.py [--configs cfg2,cfg3] [--out FILE] [--steps 10]

Per configuration (the trees and pose rings of bench.py's cfg2 and cfg3), next to tools/fit_bench.py's figures:
  (a) rows      mnv_rows_adam_step and mnv_rows_sgd_step, alternated, each behind the same mnv_rays_grad launch (pose 0, grey target): time,
                touched words, bytes by the header's counts (42 / 26 per touched word, 8 per untouched one) and the ratio held against
                (Adam's bytes / SGD's bytes) x 1.25
  (b) batcher   mnv_ray_batcher_draw of 2^21 rays (32768 tiles / 2097152 pixels) over the 16 poses' frames with tile 8 and tile 1: time
                and bytes (56 per ray: 16 read, 40 written) next to a device copy of the same bytes
  (c) gradient  mnv_rays_grad on such a tile-8 batch, on a tile-1 batch and on a whole image of the same ray count (a 2048 x 1024 frame
                of pose 0's camera): the price of spreading a batch over the set
  (d) psnr      levels of detail (--lod 9; cfg3 also one level down) fitted on the EVEN poses, scored on the ODD ones (mnv_frame_metrics,
                quantised): `steps` SGD steps (tools/fit_bench.py's path, re-measured here), `steps` full-batch Adam steps, and Adam on
                batches of 2^21 rays for the same number of rays.
Then the step `points`: the occupied leaf centres of cfg2's depth-10 shell as a white point cloud, N3Tree.from_points at D = 9 with SH9 rows
and one density, fitted to the full tree's frames of the even poses with Adam on 2^21-ray batches from that constant start: PSNR of the
fitted and of the held-out (odd) poses before and after 10, 100 and 1000 steps, each from the same start.
Every step (cfg2, cfg3, points) is a child process under its own `timeout`; the driver itself never opens the GPU and stops at the first
step that fails.  HIP events on one stream, medians of five figures.  Prints a table and one JSON line."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

STEP_TIMEOUT_S = 540
BATCH = 1 << 21


def run(name, a, res, rows):
    import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv
    from fit_bench import W, H, ROUNDS, events_ms, measure, psnr_on

    spec, camera = (cases.CFG2_TREE, cases.cfg2_camera) if name == "cfg2" else (cases.CFG3_FULL, cases.cfg3_camera)
    tree = cases.make_tree(mnv, spec)
    tree.move_to_device()
    v = tree.device_view()
    n_words = v.capacity * 8 * v.data_dim
    rows.append(f"--- {name}: {v.capacity} chunks, data_dim {v.data_dim}, {n_words / 1e6:.1f} M words")
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    cams = [camera(mnv, p, W, H) for p in range(16)]
    o, d = mnv.generate_rays(mnv.PROJ_PINHOLE, cams[0])
    grey = torch.full((H, W, 4), 0.5, dtype=torch.float32, device="cuda")
    grey[..., 3] = 1.0
    # (a) the two row kernels behind the same launch, alternated; rates 0 keep the rows (and with them the launch) what they are
    acc = torch.zeros((v.capacity * 8, v.data_dim), dtype=torch.int64, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    master = torch.empty((v.capacity * 8, v.data_dim), dtype=torch.float32, device="cuda")
    mnv.lib().mnv_rows_master_init(v.data, n_words, master.data_ptr(), None)
    m1, m2 = torch.zeros_like(master), torch.zeros_like(master)
    mnv.rays_grad(v, o, d, grey, opt, acc, sums, stream=sp)
    torch.cuda.synchronize()
    touched = int((acc != 0).any(dim=1).sum().item()) * v.data_dim
    acc.zero_()
    t_sgd, t_adam = [], []
    for i in range(ROUNDS + 1):
        for which in ("sgd", "adam"):
            mnv.rays_grad(v, o, d, grey, opt, acc, sums, stream=sp)
            if which == "sgd":
                ms = events_ms(lambda: mnv.rows_sgd_step(v.data, master, acc, v.data_dim, 0.0, 0.0, stream=sp), 1, st)
            else:
                ms = events_ms(lambda: mnv.rows_adam_step(v.data, master, m1, m2, acc, v.data_dim, i + 1, 0.0, 0.0, stream=sp), 1, st)
            if i > 0:                                      # (the first pair warms up)
                (t_sgd if which == "sgd" else t_adam).append(ms)
    ms_sgd, ms_adam = statistics.median(t_sgd), statistics.median(t_adam)
    b_sgd, b_adam = touched * 26 + (n_words - touched) * 8, touched * 42 + (n_words - touched) * 8
    bound = b_adam / b_sgd * 1.25
    rows.append(f"(a) {touched / 1e6:.1f} M touched words of {n_words / 1e6:.1f} M: mnv_rows_sgd_step {ms_sgd:8.4f} ms ({b_sgd / 1e9:.2f} GB, {b_sgd / ms_sgd / 1e9:.2f} TB/s); "
                f"mnv_rows_adam_step {ms_adam:8.4f} ms ({b_adam / 1e9:.2f} GB, {b_adam / ms_adam / 1e9:.2f} TB/s): {ms_adam / ms_sgd:.2f} x, target <= {bound:.2f} x: "
                f"{'met' if ms_adam / ms_sgd <= bound else 'MISSED'}")
    res.update({f"{name}_sgd_ms": ms_sgd, f"{name}_adam_ms": ms_adam, f"{name}_touched_words": touched, f"{name}_adam_bound": bound})
    del master, m1, m2
    # (b) the batcher over the 16 poses' frames (the full tree's own frames)
    frames = []
    for c in cams:
        f = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        mnv.render_voxels_accel(tree.accel, c, opt, rgba=f)
        frames.append(f)
    n = BATCH
    bo, bd, bt = (torch.empty((n, k), dtype=torch.float32, device="cuda") for k in (3, 3, 4))
    src, dst = torch.empty(n * 14, dtype=torch.float32, device="cuda"), torch.empty(n * 14, dtype=torch.float32, device="cuda")
    ms_copy, _ = measure(lambda: dst.copy_(src), st, a.min_ms)
    batches = {}
    for tile in (8, 1):
        b = mnv.RayBatcher(cams, frames, tile=tile, seed=1)
        count = n // (tile * tile)
        ms, reps = measure(lambda: b.draw(0, 0, count, bo, bd, bt, stream=sp), st, a.min_ms)
        rows.append(f"(b) mnv_ray_batcher_draw, tile {tile}: {n} rays of {b.units} units over 16 poses {ms:8.4f} ms ({n * 56 / ms / 1e9:.2f} TB/s of 56 B per ray); "
                    f"a device copy of the same bytes {ms_copy:8.4f} ms   reps {reps}")
        res[f"{name}_draw_tile{tile}_ms"] = ms
        # (c) the gradient on that batch
        acc.zero_()
        msg, reps = measure(lambda: mnv.rays_grad(v, bo, bd, bt, opt, acc, sums, stream=sp), st, a.min_ms)
        batches[tile] = msg
        b.close()
    res[f"{name}_copy_ms"] = ms_copy
    acc.zero_()
    wide = camera(mnv, 0, 2048, 1024)
    wo, wd = mnv.generate_rays(mnv.PROJ_PINHOLE, wide)
    wf = torch.empty((1024, 2048, 4), dtype=torch.float32, device="cuda")
    mnv.render_voxels_accel(tree.accel, wide, opt, rgba=wf)
    ms_img, reps = measure(lambda: mnv.rays_grad(v, wo, wd, wf, opt, acc, sums, stream=sp), st, a.min_ms)
    rows.append(f"(c) mnv_rays_grad on {n} rays: a whole 2048 x 1024 image of pose 0 {ms_img:8.4f} ms; a tile-8 batch over 16 poses {batches[8]:8.4f} ms ({batches[8] / ms_img:.2f} x); "
                f"a tile-1 batch {batches[1]:8.4f} ms ({batches[1] / ms_img:.2f} x)")
    res.update({f"{name}_grad_image_ms": ms_img, f"{name}_grad_tile8_ms": batches[8], f"{name}_grad_tile1_ms": batches[1]})
    del acc, bo, bd, bt, src, dst, frames, wo, wd, wf
    torch.cuda.empty_cache()
    # (d) fit on the even poses, score on the odd ones
    even, odd = cams[0::2], cams[1::2]
    full8 = []
    for c in odd:
        u8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        mnv.render_voxels_accel(tree.accel, c, opt, rgba8=u8)
        full8.append(u8)
    batch = BATCH
    batched_steps = -(-a.steps * len(even) * W * H // batch)
    for depth in ([9] if name == "cfg2" else [9, spec["depth"] - 1]):
        variants = (("sgd", dict(lr_colour=1.0, lr_sigma=20.0), a.steps), ("adam", dict(optimizer="adam"), a.steps),
                    ("adam_batched", dict(optimizer="adam", batch_rays=batch, tile=8, seed=1), batched_steps))
        for label, kw, steps in variants:
            lod = tree.make_lod(depth)
            before = psnr_on(lod, full8, odd, opt)
            t0 = time.time()
            lod.fit_to(tree, even, opt, steps, **kw)
            wall = time.time() - t0
            after = psnr_on(lod, full8, odd, opt)
            rows.append(f"(d) --lod {depth:2d}, {label:12s} {steps:4d} steps on the even poses: PSNR on the odd poses {before:6.2f} dB -> {after:6.2f} dB ({wall:.1f} s wall)")
            res.update({f"{name}_lod{depth}_{label}_psnr_before": before, f"{name}_lod{depth}_{label}_psnr_after": after})
            del lod
    del tree


def points(a, res, rows):
    """the experiment DESIGN.md 5.18 names: a tree built from a point cloud, fitted to frames from a constant-density start"""
    import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv
    from fit_bench import W, H, psnr_on
    from points_bench import leaf_centres

    full = cases.make_tree(mnv, cases.CFG2_TREE)
    data, child, _ = full.host_arrays()
    hv = full.host_view()
    offset, scale = [float(x) for x in hv.offset], [float(x) for x in hv.scale]
    centres = leaf_centres(np, data, child)
    world = torch.from_numpy(((centres - np.array(offset)) / np.array(scale)).astype(np.float32)).cuda()
    full.move_to_device()
    opt = mnv.RenderOptions.cli_defaults()
    cams = [cases.cfg2_camera(mnv, p, W, H) for p in range(16)]
    even, odd = cams[0::2], cams[1::2]
    frames, full8 = [], {}
    for c in even:
        f = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        mnv.render_voxels_accel(full.accel, c, opt, rgba=f)
        f[..., 3] = 1.0                                      # (a photograph has no alpha: every pixel counts, the background too)
        frames.append(f)
    for label, group in (("train", even), ("held", odd)):
        full8[label] = []
        for c in group:
            u8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
            mnv.render_voxels_accel(full.accel, c, opt, rgba8=u8)
            full8[label].append(u8)
    rows.append(f"--- points: {world.shape[0]} leaf centres of cfg2's shell, from_points at D = 9 (SH9 rows, white, sigma 100), fitted on the 8 even poses with "
                f"Adam (default rates) on 2^21-ray tile-8 batches")
    for steps in (10, 100, 1000):
        tree = mnv.N3Tree.from_points(world, None, depth=9, data_format="SH9", cube=(offset, scale))
        before = {k: psnr_on(tree, full8[k], g, opt) for k, g in (("train", even), ("held", odd))}
        t0 = time.time()
        tree.fit(even, frames, opt, steps, optimizer="adam", batch_rays=BATCH, tile=8, seed=1)
        wall = time.time() - t0
        after = {k: psnr_on(tree, full8[k], g, opt) for k, g in (("train", even), ("held", odd))}
        rows.append(f"(e) {steps:4d} steps: {tree.capacity} chunks; PSNR of the fitted poses {before['train']:6.2f} -> {after['train']:6.2f} dB, of the held-out poses "
                    f"{before['held']:6.2f} -> {after['held']:6.2f} dB ({wall:.1f} s wall)")
        res.update({f"points_{steps}_train_before": before["train"], f"points_{steps}_train_after": after["train"], f"points_{steps}_held_before": before["held"],
                    f"points_{steps}_held_after": after["held"]})
        del tree


def step(name, a):
    import torch

    torch.cuda.set_device(0)
    res, rows = {}, []
    if name == "points":
        points(a, res, rows)
    else:
        run(name, a, res, rows)
    for r in rows:
        print("ROW " + r)
    print("STEP " + json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3,points")
    ap.add_argument("--out", default="")
    ap.add_argument("--min_ms", type=float, default=300.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step", default="", help="internal: cfg2 | cfg3 | points, run in this process")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a)
    res, rows = {}, ["Adam and ray batches, 1920x1080; medians of five figures"]
    for name in a.configs.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", name, "--min_ms", str(a.min_ms), "--steps", str(a.steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        done = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
        rows += [t[4:] for t in p.stdout.splitlines() if t.startswith("ROW ")]
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(rows) + "\n")
        if p.returncode != 0 or not done:
            print("\n".join(rows))
            print(f"step {name} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}")
            return 1
        res.update(json.loads(done[0][5:]))
    print("\n".join(rows))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())

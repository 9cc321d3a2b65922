"""What fitting costs and buys on one GPU (1920x1080): python tools/fit_bench.py [--configs cfg2,cfg3] [--out FILE] [--min_ms 300]

Per configuration (the trees and pose rings of bench.py's cfg2 and cfg3):
  (a) rays_ms       mnv_render_rays_accel on the pinhole rays of pose 0: the yardstick (unchanged by this feature)
  (b) grad_ms       mnv_rays_grad on the same rays against a grey target (every dense sample then has terms to add), its ratio to (a), and
                    the integer-atomic bytes it delivers per second: n_samples * unmasked words * 8 over the launch time -- the rate of the
                    kernel as a whole, a LOWER bound of what the atomic path sustains (the two marches share the time)
      grad_fwd_ms   the same launch with every ray excluded (alpha 0): the forward march of this kernel alone
  (c) sgd_ms        mnv_rows_sgd_step behind such a launch (all rows read, the touched ones updated and cleared)
  (d) psnr          levels of detail (--lod 9; cfg3 also one level down from the full tree) against the full tree before and after
                    N3Tree.fit_to: fitted on the EVEN poses of the ring, scored on the ODD ones with mnv_frame_metrics (quantised).
HIP events on one stream around `reps` back-to-back calls after a warm-up, the median of five figures.  Prints a table and one JSON line."""
import argparse, json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

W, H = 1920, 1080
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
    for _ in range(2):
        fn()
    pilot = events_ms(fn, 3, stream)
    reps = max(5, int(math.ceil(min_ms / max(pilot, 1e-3))))
    return statistics.median(events_ms(fn, reps, stream) for _ in range(ROUNDS)), reps


def psnr_on(tree, full_frames8, cams, opt):
    """mean PSNR of `tree`'s frames at cams against the full tree's RGBA8 frames"""
    out = []
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    for cam, t8 in zip(cams, full_frames8):
        mnv.render_voxels_accel(tree.accel, cam, opt, rgba=f32)
        sums = mnv.frame_metrics(f32, t8, mnv.METRIC_QUANTISED)
        torch.cuda.synchronize()
        out.append(mnv.metrics_finish(sums)["psnr"])
    return float(np.mean(out))


def run(name, a, res, rows):
    spec, camera = (cases.CFG2_TREE, cases.cfg2_camera) if name == "cfg2" else (cases.CFG3_FULL, cases.cfg3_camera)
    t0 = time.time()
    tree = cases.make_tree(mnv, spec)
    tree.move_to_device()
    v = tree.device_view()
    rows.append(f"--- {name}: {v.capacity} chunks, data_dim {v.data_dim} (built in {time.time() - t0:.0f} s)")
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    n = W * H
    cam = camera(mnv, 0, W, H)
    o, d = mnv.generate_rays(mnv.PROJ_PINHOLE, cam)
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    ms_rays, reps = measure(lambda: mnv.render_rays_accel(tree.accel, o, d, opt, rgba=f32, stream=sp), st, a.min_ms)
    rows.append(f"(a) mnv_render_rays_accel, pose 0                    {ms_rays:8.4f} ms   {n / ms_rays / 1e3:7.1f} Mrays/s   reps {reps}")
    acc = torch.zeros((v.capacity * 8, v.data_dim), dtype=torch.int64, device="cuda")
    sums = torch.zeros(8, dtype=torch.int64, device="cuda")
    grey = torch.full((H, W, 4), 0.5, dtype=torch.float32, device="cuda")
    grey[..., 3] = 1.0
    ms_grad, reps = measure(lambda: mnv.rays_grad(v, o, d, grey, opt, acc, sums, stream=sp), st, a.min_ms)
    sums.zero_()
    mnv.rays_grad(v, o, d, grey, opt, acc, sums, rgba=f32, stream=sp)
    torch.cuda.synchronize()
    s = dict(zip(mnv.FIT_SUMS, sums.cpu().numpy()[:5].tolist()))
    words = s["n_samples"] * v.data_dim
    rate = words * 8 / (ms_grad * 1e-3)
    rows.append(f"(b) mnv_rays_grad, the same rays, grey target         {ms_grad:8.4f} ms   {ms_grad / ms_rays:5.2f} x (a)   {s['n_samples']} dense samples of {s['n_rays']} rays "
                f"({s['n_stopped']} stopped, {s['n_skipped']} skipped), {words * 8 / 1e6:.1f} MB of 64-bit atomic adds: {rate / 1e9:.1f} GB/s (whole-kernel rate)   reps {reps}")
    none = grey.clone()
    none[..., 3] = 0.0
    ms_fwd, reps = measure(lambda: mnv.rays_grad(v, o, d, none, opt, acc, sums, stream=sp), st, a.min_ms)
    rows.append(f"    ... every ray excluded: this kernel's forward alone  {ms_fwd:8.4f} ms   {ms_fwd / ms_rays:5.2f} x (a)   reps {reps}")
    master = torch.empty((v.capacity * 8, v.data_dim), dtype=torch.float32, device="cuda")
    mnv.lib().mnv_rows_master_init(v.data, v.capacity * 8 * v.data_dim, master.data_ptr(), None)
    acc.zero_()
    step_ms = []
    for _ in range(ROUNDS):
        mnv.rays_grad(v, o, d, grey, opt, acc, sums, stream=sp)
        step_ms.append(events_ms(lambda: mnv.rows_sgd_step(v.data, master, acc, v.data_dim, 0.0, 0.0, stream=sp), 1, st))   # (rates 0: the rows keep their values)
    ms_sgd = statistics.median(step_ms)
    sgd_bytes = v.capacity * 8 * v.data_dim * 8
    rows.append(f"(c) mnv_rows_sgd_step behind one launch               {ms_sgd:8.4f} ms   ({sgd_bytes / 1e9:.2f} GB of accumulators read: {sgd_bytes / ms_sgd / 1e9:.2f} TB/s)")
    res.update({f"{name}_rays_ms": ms_rays, f"{name}_grad_ms": ms_grad, f"{name}_grad_fwd_ms": ms_fwd, f"{name}_sgd_ms": ms_sgd, f"{name}_atomic_GBps": rate / 1e9,
                f"{name}_n_samples": s["n_samples"]})
    del acc, master
    torch.cuda.empty_cache()
    # (d) fit on the even poses, score on the odd ones
    even = [camera(mnv, p, W, H) for p in range(0, 16, 2)]
    odd = [camera(mnv, p, W, H) for p in range(1, 16, 2)]
    full8 = []
    for c in odd:
        u8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
        mnv.render_voxels_accel(tree.accel, c, opt, rgba8=u8)
        full8.append(u8)
    depths = [9] if name == "cfg2" else [9, spec["depth"] - 1]
    for depth in depths:
        lod = tree.make_lod(depth)
        before = psnr_on(lod, full8, odd, opt)
        t0 = time.time()
        se = lod.fit_to(tree, even, opt, a.iterations, a.lr_colour, a.lr_sigma)
        wall = time.time() - t0
        after = psnr_on(lod, full8, odd, opt)
        mono = all(y < x for x, y in zip(se, se[1:]))
        rows.append(f"(d) --lod {depth:2d}: {lod.capacity} chunks; PSNR on the odd poses {before:6.2f} dB -> {after:6.2f} dB after {a.iterations} steps on the even poses "
                    f"(lr {a.lr_colour:g} / {a.lr_sigma:g}; training loss {'fell at every step' if mono else 'did NOT fall at every step'}: "
                    f"{se[0] / 2**32:.1f} -> {se[-1] / 2**32:.1f}; {wall:.1f} s wall, teacher frames and accel rebuild included)")
        res.update({f"{name}_lod{depth}_psnr_before": before, f"{name}_lod{depth}_psnr_after": after, f"{name}_lod{depth}_monotone": mono})
        del lod
    del tree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--out", default="")
    ap.add_argument("--min_ms", type=float, default=300.0)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--lr_colour", type=float, default=1.0)
    ap.add_argument("--lr_sigma", type=float, default=20.0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res, rows = {}, [f"fitting, {W}x{H}, {torch.cuda.get_device_name(0)}; medians of {ROUNDS} figures over >= {a.min_ms:.0f} ms of work each"]
    for name in a.configs.split(","):
        run(name, a, res, rows)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(rows) + "\n")
    print("\n".join(rows))
    print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()

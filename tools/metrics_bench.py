"""What scoring a frame on the device costs on one GPU (cfg2 tree, 1920x1080): python tools/metrics_bench.py [--out FILE] [--min_ms 1000] [--no_frames]

  (a) se_ms             mnv_frame_metrics without MNV_METRIC_SSIM (the streaming squared-error pass) on a rendered frame against the packed
                        frame of the next pose: ms, the 20 bytes per pixel it reads over the time, and that rate relative to (c)
  (b) ssim_ms           the same with MNV_METRIC_SSIM (the tiled pass: squared error and SSIM in one launch)
  (c) copy_ms           a device-to-device copy (torch's, contiguous) of W * H * 20 bytes in the same run (reads AND writes that many bytes:
                        its rate is given as bytes copied over time, the yardstick for a streaming read of this memory system)
  (d) frame_<t>_3       whole plain frames through Renderer with three in flight, t = plain (no target), se and ssim (set_target)

(a)-(c): HIP events on one stream around `reps` back-to-back calls after a warm-up, reps chosen so that every figure covers at least
--min_ms of device work.  (d): the Renderer owns its streams, so it is the wall time of `reps` render() calls and the wait for the last
frame, same rule for reps.  Prints a table and one JSON line; --out writes the table.
A call of (a) / (b) is a memset of the sums and one kernel issued from Python: where the figure is the same for both, it is the rate at which
the host issues calls, not the kernels.  For the kernels' own times run (a)-(c) alone under the profiler, in a run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/metrics_bench.py --no_frames --min_ms 20; python tools/kstats.py DIR"""
import argparse, ctypes as C, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch, cases, mega_nerf_viewer_amd as mnv

W, H, FX = 1920, 1080, 1600.0
PEAK = 8e12


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
    return events_ms(fn, reps, stream), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--min_ms", type=float, default=1000.0)
    ap.add_argument("--no_frames", action="store_true", help="skip (d)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tree = cases.make_tree(mnv, cases.CFG2_TREE)
    tree.move_to_device()
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    res, rows = {}, []
    nbytes = W * H * 20
    # a real frame, and the packed frame of the next pose as its target
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    target = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    mnv.render_voxels_accel(tree.accel, cases.cfg2_camera(mnv, 0, W, H, FX), opt, rgba=f32, stream=sp)
    mnv.render_voxels_accel(tree.accel, cases.cfg2_camera(mnv, 1, W, H, FX), opt, rgba8=target, stream=sp)
    sums = torch.zeros(5, dtype=torch.int64, device="cuda")

    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cms, reps = measure(lambda: dst.copy_(src), st, a.min_ms)
    crate = nbytes / (cms * 1e-3)
    res["copy_ms"] = cms
    rows.append(f"(c) copy ({nbytes / 1e6:5.1f} MB)                  {cms:8.4f} ms   {crate / 1e12:5.2f} TB/s copied ({crate / PEAK:5.1%} of peak)   reps {reps}")
    for key, name, flags in (("se_ms", "(a) squared error", mnv.METRIC_QUANTISED), ("ssim_ms", "(b) squared error + SSIM", mnv.METRIC_QUANTISED | mnv.METRIC_SSIM)):
        ms, reps = measure(lambda: mnv.frame_metrics(f32, target, flags, sums=sums, stream=sp), st, a.min_ms)
        rate = nbytes / (ms * 1e-3)
        res[key] = ms
        v = mnv.metrics_finish(sums.cpu())
        rows.append(f"{name:<32s}   {ms:8.4f} ms   {rate / 1e12:5.2f} TB/s read   ({rate / PEAK:5.1%} of peak, {rate / crate:4.2f} x the copy's rate)   "
                    f"reps {reps}   psnr {v['psnr']:.3f} ssim {v['ssim']:.4f}")

    # (d) whole frames through the Renderer, three in flight
    del src, dst
    cam0 = cases.cfg2_camera(mnv, 0, W, H, FX)
    for kind, flags in () if a.no_frames else (("plain", None), ("se", mnv.METRIC_QUANTISED), ("ssim", mnv.METRIC_QUANTISED | mnv.METRIC_SSIM)):
        r = mnv.Renderer()
        r.resize(W, H)
        r.set(tree, tree.capacity)
        bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
        C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
        r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
        c2w = cam0.c2w
        r.set_camera(tuple(c2w[9:12]), tuple(c2w[6:9]), up=(0.0, 0.0, 1.0), fx=FX)
        r.set_frames_in_flight(3)
        if flags is not None:
            r.set_target(target, flags)

        def run(reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                r.render()
            for s in range(3):
                try:
                    r.download_slot(s)
                except mnv.MnvError:
                    pass
            return (time.perf_counter() - t0) * 1e3 / reps

        run(3)
        pilot = run(5)
        reps = max(10, int(math.ceil(a.min_ms / pilot)))
        ms = run(reps)
        res[f"frame_{kind}_3_ms"] = ms
        rows.append(f"(d) Renderer frame, {kind:<5s} 3 in flight   {ms:8.4f} ms wall per frame (the last downloads included)   reps {reps}")
        del r
    head = f"frame metrics on the cfg2 tree, {W}x{H}, {torch.cuda.get_device_name(0)}; peak = 8 TB/s; every figure over >= {a.min_ms:.0f} ms of work"
    text = "\n".join([head] + rows)
    print(text)
    print(json.dumps({k: round(v, 5) for k, v in res.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

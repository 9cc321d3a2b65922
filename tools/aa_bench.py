"""What anti-aliased frames cost on one GPU (cfg2 tree, 1920x1080): python tools/aa_bench.py [--out FILE] [--min_ms 1000]

  (a) batch16_ms        one mnv_render_voxels_accel_batch launch of the 16 jittered cameras of a K = 16 frame (float sub-frames only)
  (b) resolve_<f>_K     mnv_resolve_samples alone for K in {4, 16, 64}, box (r = 0) and tent (r = 1): ms, bytes of sub-frames read over the
                        time, that rate as a fraction of the 8 TB/s HBM peak and relative to (c)
  (c) copy_K            a device-to-device copy (torch's, contiguous) of the same K * W * H * 16 bytes in the same run (reads AND writes that many
                        bytes: its rate is given as bytes copied over time, the yardstick for a streaming read of this memory system)
  (d) frame16_tent_<n>  a whole K = 16 tent frame through Renderer (march + resolve) with n = 1 and n = 3 frames in flight

(a)-(c): HIP events on one stream around `reps` back-to-back calls after a warm-up, reps chosen so that every figure covers at least
--min_ms of device work.  (d): the Renderer owns its streams, so it is the wall time of `reps` render() calls and the wait for the last
frame, same rule for reps.  Prints a table and one JSON line; --out writes the table."""
import argparse, ctypes as C, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

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
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tree = cases.make_tree(mnv, cases.CFG2_TREE)
    tree.move_to_device()
    cam0 = cases.cfg2_camera(mnv, 0, W, H, FX)
    opt = mnv.RenderOptions.cli_defaults()
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    res, rows = {}, []
    frame_bytes = W * H * 16
    sub = torch.zeros((64, H, W, 4), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(sub)
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    u8 = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")

    # (a) the K = 16 batch launch (real sub-frames: the resolves below read them)
    off = mnv.aa_pattern(16)
    cams = []
    for dx, dy in off:
        c = cases.cfg2_camera(mnv, 0, W, H, FX)
        c.c.cx = float(np.float32(cam0.c.cx) - dx)
        c.c.cy = float(np.float32(cam0.c.cy) - dy)
        cams.append(c)
    ms, reps = measure(lambda: mnv.render_voxels_accel_batch(tree.accel, cams, opt, rgba=sub[:16], stream=sp), st, a.min_ms)
    res["batch16_ms"] = ms
    rows.append(f"(a) batch launch, 16 cameras            {ms:8.4f} ms   {16 * W * H / ms / 1e6:6.2f} Grays/s   reps {reps}")
    for k in (1, 2, 3):   # fill the rest of the 64 sub-frames with pictures too
        sub[16 * k:16 * (k + 1)].copy_(sub[:16])

    # (c) then (b) per K: the copy first, so that every resolve has its yardstick from the same run
    for k in (4, 16, 64):
        nbytes = k * frame_bytes
        cms, reps = measure(lambda: dst[:k].copy_(sub[:k]), st, a.min_ms)   # (a contiguous device-to-device copy on this stream)
        crate = nbytes / (cms * 1e-3)
        res[f"copy_{k}_ms"] = cms
        rows.append(f"(c) copy K={k:<2d} ({nbytes / 1e6:7.1f} MB)              {cms:8.4f} ms   {crate / 1e12:5.2f} TB/s copied ({crate / PEAK:5.1%} of peak)   reps {reps}")
        offk = mnv.aa_pattern(k)
        for name, filt in (("box", mnv.AA_BOX), ("tent", mnv.AA_TENT)):
            table = mnv.aa_weights(filt, offk)
            wt = torch.from_numpy(table).cuda()
            r = table.shape[1] // 2
            ms, reps = measure(lambda: mnv.resolve_samples(sub[:k], wt, r, rgba=f32, rgba8=u8, stream=sp), st, a.min_ms)
            rate = nbytes / (ms * 1e-3)
            res[f"resolve_{name}_{k}_ms"] = ms
            rows.append(f"(b) resolve {name:<4s} K={k:<2d}                   {ms:8.4f} ms   {rate / 1e12:5.2f} TB/s read   ({rate / PEAK:5.1%} of peak, "
                        f"{rate / crate:4.2f} x the copy's rate, {ms / res['batch16_ms']:5.1%} of (a))   reps {reps}")

    # (d) whole frames through the Renderer
    del dst
    for n in (1, 3):
        r = mnv.Renderer()
        r.resize(W, H)
        r.set(tree, tree.capacity)
        bm = (r.options.basis_minmax[0], r.options.basis_minmax[1])
        C.memmove(C.byref(r.options), C.byref(opt), C.sizeof(opt))
        r.options.basis_minmax[0], r.options.basis_minmax[1] = bm
        c2w = cam0.c2w
        r.set_camera(tuple(c2w[9:12]), tuple(c2w[6:9]), up=(0.0, 0.0, 1.0), fx=FX)
        r.set_frames_in_flight(n)
        r.set_antialiasing(16, mnv.AA_TENT)

        def run(reps):
            t0 = time.perf_counter()
            for _ in range(reps):
                r.render()
            for s in range(n):
                try:
                    r.download_slot(s)
                except mnv.MnvError:
                    pass
            return (time.perf_counter() - t0) * 1e3 / reps

        run(3)
        pilot = run(5)
        reps = max(10, int(math.ceil(a.min_ms / pilot)))
        ms = run(reps)
        res[f"frame16_tent_{n}_ms"] = ms
        rows.append(f"(d) Renderer frame K=16 tent, {n} in flight  {ms:8.4f} ms wall per frame (march + resolve; the last download included)   reps {reps}")
        del r
    head = f"anti-aliasing on the cfg2 tree, {W}x{H}, {torch.cuda.get_device_name(0)}; peak = 8 TB/s; every figure over >= {a.min_ms:.0f} ms of work"
    text = "\n".join([head] + rows)
    print(text)
    print(json.dumps({k: round(v, 5) for k, v in res.items()}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""What building a tree from a point cloud costs on one GPU: python tools/points_bench.py [--out FILE] [--reps 5] [--cases LIST]

Clouds are made on the device: the occupied leaf centres of cfg2's depth-10 shell / the cfg3 terrain of bench.py (tests/cases.py: CFG2_TREE,
CFG3_FULL), drawn with a seeded generator and jittered by half a depth-10 voxel, colours from the position.  A case is TREE:POINTS:DEPTH[:CALLS]
(default: cfg2 and cfg3 at 10 M and 100 M points, D = 10 and 11, one add; cfg2 at 10 M, D = 10, as ten adds).  Per case, medians over the
reps after a warm-up round, HIP events on the null stream:
  add / finish / write ms   a fresh handle per round; add includes its waits (it reads the record count back), write fills all five arrays
  points per second         accepted + dropped points over add + finish + write
  sort ms                   the same keys (the Morton codes, computed here with torch) and 32-bit payloads through rocprim::radix_sort_pairs
                            alone over the same 3 D bits, in the double-buffer form add uses (mnv_hook_points_sort_pairs of the test-hook
                            build): the yardstick for add
  copy ms                   a device-to-device copy of the input bytes (15 per point)
  device bytes              what the handle and its scratch hold after write (hipMemGetInfo before create and after write, torch's cache emptied)
Every case is a child process under its own `timeout`; the driver itself never opens the GPU and stops at the first case that fails, is
killed or times out.  Prints a table and one JSON line per case; --out writes the table."""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STEP_TIMEOUT_S = 540
DEFAULT_CASES = "cfg2:10000000:10,cfg2:10000000:11,cfg3:10000000:10,cfg3:10000000:11,cfg2:100000000:10,cfg2:100000000:11,cfg3:100000000:10,cfg3:100000000:11,cfg2:10000000:10:10"


def leaf_centres(np, data, child):
    """Tree-space centres float64 [m, 3] of the leaves whose sigma is positive: one level-synchronous walk."""
    dd = data.shape[2]
    digit = np.array([[j >> 2, (j >> 1) & 1, j & 1] for j in range(8)], np.int64)
    chunks, corners, depth, out = np.zeros(1, np.int64), np.zeros((1, 3), np.int64), 1, []
    while chunks.size:
        ch = child[chunks].astype(np.int64)
        cells = corners[:, None, :] * 2 + digit[None, :, :]
        lit = (ch == 0) & (data[chunks, :, dd - 1].view(np.float16) > 0)
        out.append((cells[lit] + 0.5) / 2.0 ** depth)
        go = ch != 0
        chunks, corners, depth = (chunks[:, None] + ch)[go], cells[go], depth + 1
    return np.concatenate(out)


def _events_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def morton(torch, xyz, offset, scale, depth):
    """int64 [n]: the contract's voxel code of every point (points outside get the all-ones key), computed with torch."""
    q = torch.tensor(offset, device="cuda") + torch.tensor(scale, device="cuda") * xyz
    ok = (torch.isfinite(q) & (q >= 0) & (q < 1)).all(dim=1)
    cell = torch.floor(q * float(2 ** depth)).long().clamp_(0, 2 ** depth - 1)
    code = torch.zeros(xyz.shape[0], dtype=torch.int64, device="cuda")
    for level in range(depth):
        for k in range(3):
            code |= ((cell[:, k] >> level) & 1) << (3 * level + (2 - k))
    return torch.where(ok, code, torch.full_like(code, -1))


def step(case, reps):
    import ctypes as C
    import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

    torch.cuda.set_device(0)
    name, n, depth, calls = (case.split(":") + ["1"])[:4]
    n, depth, calls = int(n), int(depth), int(calls)
    note = lambda text: print(f"[{case}] {text}", file=sys.stderr, flush=True)  # noqa: E731
    tree = cases.make_tree(mnv, {"cfg2": cases.CFG2_TREE, "cfg3": cases.CFG3_FULL}[name])
    data, child, _ = tree.host_arrays()
    hv = tree.host_view()
    offset, scale = [float(x) for x in hv.offset], [float(x) for x in hv.scale]
    centres = leaf_centres(np, data, child)
    note(f"source tree: {tree.capacity} chunks, {centres.shape[0]} lit leaves")
    world = torch.from_numpy(((centres - np.array(offset)) / np.array(scale)).astype(np.float32)).cuda()
    del tree, data, child
    gen = torch.Generator(device="cuda").manual_seed(1234)
    pick = torch.randint(world.shape[0], (n,), generator=gen, device="cuda")
    jitter = (torch.rand((n, 3), generator=gen, device="cuda") - 0.5) * torch.tensor([2.0 ** -10 / s for s in scale], device="cuda")
    xyz = (world[pick] + jitter).contiguous()
    rgb = ((xyz * torch.tensor(scale, device="cuda") + torch.tensor(offset, device="cuda")).clamp(0, 1) * 255).to(torch.uint8).contiguous()
    del pick, jitter, world
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    res = {"case": case, "points": n, "depth": depth, "calls": calls, "device": torch.cuda.get_device_name(0), "reps": reps}

    cuts = [n * i // calls for i in range(calls + 1)]
    t_add, t_finish, t_write, stats, held = [], [], [], None, 0
    for rnd in range(reps + 1):                                # the first round warms up and is dropped
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        pt = mnv.PointTree(offset, scale, depth, 100.0, 1, "SH9")
        add = _events_ms(torch, lambda: [pt.add(xyz[a:b], rgb[a:b], n=b - a) for a, b in zip(cuts[:-1], cuts[1:])])
        box = {}
        fin = _events_ms(torch, lambda: box.setdefault("st", pt.finish()))
        stats = box["st"]
        cap = stats.capacity
        o_child = torch.empty((cap, 8), dtype=torch.int32, device="cuda")
        o_data = torch.empty((cap, 8, pt.data_dim), dtype=torch.int16, device="cuda")
        o_parent = torch.empty((cap,), dtype=torch.int32, device="cuda")
        o_sc = torch.empty((cap, 8), dtype=torch.int16, device="cuda")
        o_counts = torch.empty((cap, 8), dtype=torch.int32, device="cuda")
        wr = _events_ms(torch, lambda: pt.write(o_child, o_data, o_parent, o_sc, o_counts))
        del o_child, o_data, o_parent, o_sc, o_counts
        torch.cuda.empty_cache()
        held = free0 - torch.cuda.mem_get_info()[0]
        del pt
        if rnd:
            t_add.append(add), t_finish.append(fin), t_write.append(wr)
        note(f"round {rnd}: add {add:.3f} ms, finish {fin:.3f} ms, write {wr:.3f} ms")
    res.update(add_ms=statistics.median(t_add), finish_ms=statistics.median(t_finish), write_ms=statistics.median(t_write),
               add_ms_spread=[min(t_add), max(t_add)], device_bytes=int(held), stats=stats.as_dict())
    res["points_per_s"] = n / ((res["add_ms"] + res["finish_ms"] + res["write_ms"]) * 1e-3)

    # the sort alone over the same keys, and a copy of the input bytes
    keys0 = morton(torch, xyz, offset, scale, depth)
    vals0 = torch.arange(n, dtype=torch.int32, device="cuda")
    keys, vals, keys_spare, vals_spare = torch.empty_like(keys0), torch.empty_like(vals0), torch.empty_like(keys0), torch.empty_like(vals0)
    h = mnv.hooks_lib()
    need, where = C.c_size_t(0), C.c_int32(0)
    assert h.mnv_hook_points_sort_pairs(None, None, None, None, n, 3 * depth, None, C.byref(need), None, None) == 0
    tmp = torch.empty((need.value + 256,), dtype=torch.uint8, device="cuda")

    def sort():
        size = C.c_size_t(need.value)
        assert h.mnv_hook_points_sort_pairs(keys.data_ptr(), keys_spare.data_ptr(), vals.data_ptr(), vals_spare.data_ptr(), n, 3 * depth, tmp.data_ptr(),
                                            C.byref(size), C.byref(where), None) == 0

    t_sort = []
    for _ in range(reps + 1):                                  # the sort overwrites both halves: the keys are put back outside the timed span
        keys.copy_(keys0), vals.copy_(vals0)
        t_sort.append(_events_ms(torch, sort))
    t_sort = t_sort[1:]
    low = (keys_spare if where.value else keys).bitwise_and((1 << (3 * depth)) - 1)
    assert bool((low[1:] >= low[:-1]).all())
    del low, keys0, vals0, keys, vals, keys_spare, vals_spare
    xyz2, rgb2 = torch.empty_like(xyz), torch.empty_like(rgb)
    t_copy = [_events_ms(torch, lambda: (xyz2.copy_(xyz), rgb2.copy_(rgb))) for _ in range(reps + 1)][1:]
    res.update(sort_ms=statistics.median(t_sort), sort_tmp_bytes=int(need.value), copy_ms=statistics.median(t_copy))
    res["add_over_sort"] = res["add_ms"] / res["sort_ms"]
    print("STEP " + json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--step", default="", help="internal: CASE, run in this process")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps)
    rows = []
    for case in a.cases.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", case, "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)      # (the step's progress lines go to stderr as they come)
        line = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
        if p.returncode != 0 or not line:
            print(f"case {case} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}")
            return 1
        print(line[0], flush=True)
        m = json.loads(line[0][5:])
        s = m["stats"]
        rows.append(f"{case}: {m['points'] / 1e6:.0f} M points in {m['calls']} add(s), D = {m['depth']}, {s['distinct_voxels']} distinct voxels, {s['capacity']} chunks, "
                    f"{s['dropped']} dropped, {m['device']}; medians over {m['reps']} rounds")
        rows.append(f"  add {m['add_ms']:9.3f} ms [{m['add_ms_spread'][0]:.3f} .. {m['add_ms_spread'][1]:.3f}]   finish {m['finish_ms']:8.3f} ms   write {m['write_ms']:8.3f} ms   "
                    f"{m['points_per_s'] / 1e9:.3f} G points/s   sort alone {m['sort_ms']:9.3f} ms   add / sort {m['add_over_sort']:.2f}   "
                    f"copy of the input {m['copy_ms']:.3f} ms   held {m['device_bytes'] / 1e9:.3f} GB ({m['device_bytes'] / m['points']:.1f} B per point)")
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

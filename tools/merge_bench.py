"""What merging two trees costs on one GPU: python tools/merge_bench.py [--out FILE] [--reps 5] [--small]

Three merges of the trees of bench.py (tests/cases.py: CFG3_FULL, the terrain that stands for a merged Mega-NeRF octree, and CFG2_TREE, the
depth-10 shell), in one process:
  renumber      cfg3 merged with the one-chunk empty tree: pure renumbering into the canonical order, every chunk moved whole
  place         cfg3 with cfg2's shell placed at level 1, corner (0, 0, 0), mode over
  blend         two cfg2 shells under mode add, the second with its radius shifted by one depth-10 voxel (2^-10) and other rows: the
                shells overlap in part, so rows are blended and chunks mix rows of both sides
For each: plan ms (HIP events around mnv_tree_merge_plan and, next to it, the host clock: the call waits for the stream once per level),
write ms (HIP events around mnv_tree_merge_write with all six outputs), medians over the reps after one warm-up round; in the same run
  copy          a device-to-device copy of as many bytes as the merged `data` array (HIP events around torch's copy_)
  cut           mnv_tree_cut with keep = 1 everywhere on the merge's base tree: the existing pass that moves the same rows
and the ratios write / copy and write / cut.  --small uses CFG3_SMALL and a depth-7 shell (a rehearsal of the script, not a measurement).
The work runs in a child process under its own `timeout`; the driver itself never opens the GPU.  A kernel trace is a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/merge_bench.py --step run  (kernels merge_level_kernel, merge_emit_kernel, rocPRIM's scan
kernels, merge_write_kernel).  Prints a table and one JSON line; --out writes the table."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STEP_TIMEOUT_S = 900


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


def step(reps, small):
    import numpy as np, torch, cases, mega_nerf_viewer_amd as mnv

    torch.cuda.set_device(0)
    note = lambda text: print(f"[merge_bench] {text}", file=sys.stderr, flush=True)  # noqa: E731
    shell_spec = dict(cases.CFG2_TREE, depth=7, half_thickness=1.5 / 128) if small else cases.CFG2_TREE
    shift = 2.0 ** -shell_spec["depth"]
    cfg3 = cases.make_tree(mnv, cases.CFG3_SMALL if small else cases.CFG3_FULL)
    shell = cases.make_tree(mnv, shell_spec)
    shifted = cases.make_tree(mnv, dict(shell_spec, radius=shell_spec["radius"] + shift, seed=1))
    dd = cfg3.host_view().data_dim
    empty = mnv.N3Tree.from_arrays(np.zeros((1, 8, dd), np.uint16), np.zeros((1, 8), np.int32), data_format=cfg3.data_format)
    for t in (cfg3, shell, shifted, empty):
        t.move_to_device(need_sample_counts=True)
    note(f"trees on the device: cfg3 {cfg3.capacity}, shell {shell.capacity}, shifted shell {shifted.capacity} chunks")
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "small": bool(small), "data_dim": dd, "merges": {}}
    for name, a, b, level, mode in (("renumber", cfg3, empty, 0, "over"), ("place", cfg3, shell, 1, "over"), ("blend", shell, shifted, 0, "add")):
        va, vb = a.device_view(), b.device_view()
        plan, plan_host = None, []

        def make_plan():
            nonlocal plan
            t0 = time.perf_counter()
            plan = mnv.TreeMerge(va, vb, level, (0, 0, 0), mode)
            plan_host.append((time.perf_counter() - t0) * 1e3)

        plan_ms = _events_ms(torch, make_plan, reps)
        st = plan.stats.as_dict()
        cap = st["capacity"]
        out = dict(child=torch.empty((cap, 8), dtype=torch.int32, device="cuda"), data=torch.empty((cap, 8, dd), dtype=torch.int16, device="cuda"),
                   parent=torch.empty((cap,), dtype=torch.int32, device="cuda"), counts=torch.empty((cap, 8), dtype=torch.int16, device="cuda"),
                   src_a=torch.empty((cap, 8), dtype=torch.int32, device="cuda"), src_b=torch.empty((cap, 8), dtype=torch.int32, device="cuda"))
        write_ms = _events_ms(torch, lambda: plan.write(out["child"], out["data"], out["parent"], out["counts"], out["src_a"], out["src_b"]), reps)
        scratch = torch.empty_like(out["data"])
        copy_ms = _events_ms(torch, lambda: scratch.copy_(out["data"]), reps)
        del scratch, out, plan
        n = va.capacity
        keep = torch.ones((n,), dtype=torch.uint8, device="cuda")
        o_child, o_data = torch.empty((n, 8), dtype=torch.int32, device="cuda"), torch.empty((n, 8, dd), dtype=torch.int16, device="cuda")
        o_parent, o_sc = torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((n, 8), dtype=torch.int16, device="cuda")
        cut_ms = _events_ms(torch, lambda: mnv.tree_cut(va, keep, n, o_child, o_data, o_parent, o_sc), reps)
        del keep, o_child, o_data, o_parent, o_sc
        levels = max(d for d in range(24) if st["chunks_at_depth"][d])
        res["merges"][name] = dict(a_chunks=int(va.capacity), b_chunks=int(vb.capacity), level=level, mode=mode, chunks=cap, levels=levels, data_bytes=cap * 16 * dd,
                                   base_data_bytes=int(va.capacity) * 16 * dd, plan_ms=plan_ms, plan_host_ms=statistics.median(plan_host[1:]), write_ms=write_ms,
                                   copy_ms=copy_ms, cut_ms=cut_ms, stats={k: v for k, v in st.items() if k != "chunks_at_depth"})
        note(f"{name} timed")
    print("STEP " + json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--step", default="", help="internal: run in this process")
    a = ap.parse_args()
    if a.step:
        return step(a.reps, a.small)
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "run", "--reps", str(a.reps)] + (["--small"] if a.small else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)          # (the step's progress lines go to stderr as they come)
    line = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
    if p.returncode != 0 or not line:
        print(f"the step ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}")
        return 1
    print(line[0], flush=True)
    m = json.loads(line[0][5:])
    rows = [f"{m['device']}; data_dim {m['data_dim']}; medians over {m['reps']} rounds" + ("; SMALL trees: a rehearsal, not a measurement" if m["small"] else "")]
    for name, r in m["merges"].items():
        gb = r["data_bytes"] / 1e9
        s = r["stats"]
        rows.append(f"{name}: {r['a_chunks']} + {r['b_chunks']} -> {r['chunks']} chunks, {r['levels']} levels, level {r['level']}, {r['mode']}; rows {gb:.3f} GB; "
                    f"rows from A {s['rows_from_a']}, from B {s['rows_from_b']}, blended {s['rows_blended']}")
        rows.append(f"  plan {r['plan_ms']:8.3f} ms (events; host clock {r['plan_host_ms']:.3f})   write {r['write_ms']:8.3f} ms ({2 * gb / r['write_ms'] * 1e3:.0f} GB/s rows read + written)   "
                    f"copy of the merged rows {r['copy_ms']:8.3f} ms ({2 * gb / r['copy_ms'] * 1e3:.0f} GB/s)   write / copy {r['write_ms'] / r['copy_ms']:.2f}")
        rows.append(f"  mnv_tree_cut, keep all, on the base tree ({r['base_data_bytes'] / 1e9:.3f} GB of rows) {r['cut_ms']:8.3f} ms   write / cut {r['write_ms'] / r['cut_ms']:.2f}   "
                    f"per GB of rows: write {r['write_ms'] / gb:.3f}, cut {r['cut_ms'] / (r['base_data_bytes'] / 1e9):.3f} ms")
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

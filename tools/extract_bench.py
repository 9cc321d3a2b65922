"""What extracting a surface costs on one GPU: python tools/extract_bench.py [--out FILE] [--reps 5] [--trees cfg2,cfg3] [--levels 8,9,10] [--iso 10]

For cfg2's depth-10 shell and the cfg3 terrain (tests/cases.py) at each level, with the empty-space skip and with MNV_EXTRACT_ALL_BRICKS, in
one process per (tree, level) so that both modes are measured on the same device in the same run, alternating:
  candidates   bricks the passes visit / bricks of the lattice (the candidate-brick share)
  vertices, triangles
  ms per pass  candidates, count, scans, emit, colour: HIP events on the stream inside the call (mnv_surface_stats), median over the reps
  call ms      host clock around mnv_extract_surface, which waits for the stream: scratch allocation, the two size read-backs and the
               output allocation included; median over the reps
  samples/s    2^(3 level) lattice samples over the call time
  identical    the two modes returned the same bytes
Every step is a child process under its own `timeout`; the driver itself never opens the GPU and stops at the first step that fails, is
killed or times out.  Prints a table and one JSON line per step; --out writes the table."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PASSES = ("ms_candidates", "ms_count", "ms_scan", "ms_emit", "ms_colour")
STEP_TIMEOUT_S = 420


def step(tree_name, level, iso, reps):
    import hashlib
    import torch, cases, mega_nerf_viewer_amd as mnv

    torch.cuda.set_device(0)
    spec = {"cfg2": cases.CFG2_TREE, "cfg3": cases.CFG3_TREE}[tree_name]
    tree = cases.make_tree(mnv, spec)
    tree.move_to_device()
    res = {"tree": tree_name, "level": level, "iso": iso, "reps": reps, "device": torch.cuda.get_device_name(0), "chunks": tree.capacity}
    runs = {False: [], True: []}
    digest = {}
    for rep in range(reps + 1):                             # the first round warms up (code objects, rocPRIM's choices) and is dropped
        for all_bricks in (False, True):                    # alternating
            t0 = time.perf_counter()
            s = mnv.extract_surface(tree.accel, level, iso, colour=True, all_bricks=all_bricks)
            call_ms = (time.perf_counter() - t0) * 1e3      # the call has waited for the stream
            st = s.stats()
            st["call_ms"] = call_ms
            st["vertices"], st["indices"] = s.counts()
            if rep == 0:
                h = hashlib.sha256()
                h.update(s.vertices().tobytes())
                h.update(s.faces().tobytes())
                digest[all_bricks] = h.hexdigest()
            else:
                runs[all_bricks].append(st)
            del s
    for all_bricks, key in ((False, "skip"), (True, "all_bricks")):
        r = runs[all_bricks]
        out = {k: statistics.median(x[k] for x in r) for k in PASSES + ("ms_total", "call_ms")}
        out["call_ms_min"], out["call_ms_max"] = min(x["call_ms"] for x in r), max(x["call_ms"] for x in r)
        out.update(bricks=r[0]["bricks"], candidate_bricks=r[0]["candidate_bricks"], vertices=r[0]["vertices"], triangles=r[0]["indices"] // 3)
        out["samples_per_s"] = float(8 ** level) / (out["call_ms"] * 1e-3)
        res[key] = out
    res["identical"] = digest[False] == digest[True]
    print("STEP " + json.dumps(res))
    return 0 if res["identical"] else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trees", default="cfg2,cfg3")
    ap.add_argument("--levels", default="8,9,10")
    ap.add_argument("--iso", type=float, default=10.0)
    ap.add_argument("--step", default="", help="internal: TREE:LEVEL, run in this process")
    a = ap.parse_args()
    if a.step:
        name, level = a.step.split(":")
        return step(name, int(level), a.iso, a.reps)
    rows = []
    for name in a.trees.split(","):
        for level in (int(x) for x in a.levels.split(",")):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", f"{name}:{level}", "--iso", str(a.iso),
                   "--reps", str(a.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            line = [t for t in p.stdout.splitlines() if t.startswith("STEP ")]
            if p.returncode != 0 or not line:
                print(f"step {name}:{level} ended with status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
                return 1
            print(line[0], flush=True)
            r = json.loads(line[0][5:])
            if not rows:
                rows.append(f"surface extraction, iso {a.iso:g}, with colour, {r['device']}; medians over {a.reps} calls per mode, modes alternating in one process")
            for key in ("skip", "all_bricks"):
                m = r[key]
                rows.append(f"{name} ({r['chunks']} chunks) level {level:2d} {key:<10s} candidates {m['candidate_bricks']:8d} / {m['bricks']:8d} ({m['candidate_bricks'] / m['bricks']:6.2%})   "
                            f"vertices {m['vertices']:9d} triangles {m['triangles']:9d}   passes ms: candidates {m['ms_candidates']:8.3f} count {m['ms_count']:8.3f} "
                            f"scans {m['ms_scan']:7.3f} emit {m['ms_emit']:8.3f} colour {m['ms_colour']:7.3f} (sum of events {m['ms_total']:8.3f})   "
                            f"call {m['call_ms']:9.3f} ms [{m['call_ms_min']:.3f} .. {m['call_ms_max']:.3f}]   {m['samples_per_s'] / 1e9:7.3f} G samples/s")
            rows.append(f"{name} level {level:2d}: the call with the skip takes {r['skip']['call_ms'] / r['all_bricks']['call_ms']:.3f} x the call without; same bytes: {r['identical']}")
    text = "\n".join(rows)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

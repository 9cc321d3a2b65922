"""Static instruction counts of a range of basic blocks of one kernel in a `hipcc --cuda-device-only -S` listing: the ruler of
LAB_NOTEBOOK round 10 for "what one iteration of the march loop holds".

Without a range: one row per loop the compiler annotated (blocks "in Loop: Header=X Depth=n", the header block included; a nested loop's
blocks count for the nested loop only), so the labels of a loop's first and last block can be read off.  With FROM and TO (labels without
the leading dot, e.g. LBB25_95 LBB25_181): the blocks from FROM to TO in layout order, both included.

Columns: instructions (no labels, no directives), VALU (v_*), v_mov* among them, SALU (s_* but s_waitcnt / s_nop / s_cbranch* / s_branch /
s_barrier / s_endpgm), branches (s_cbranch* + s_branch), v_readlane + v_writelane, scratch accesses, waits (s_waitcnt + s_nop).
usage: isa_loop_counts.py file.s mangled-name-substring [FROM TO]"""
import collections
import re
import sys

COLS = ("instr", "valu", "v_mov", "salu", "branch", "lane", "scratch", "wait")


def classify(op):
    out = ["instr"]
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        out += ["valu", "lane"]
    elif op.startswith("v_"):
        out.append("valu")
        if op.startswith("v_mov") or op.startswith("v_accvgpr"):
            out.append("v_mov")
    elif op.startswith(("s_cbranch", "s_branch")):
        out.append("branch")
    elif op.startswith(("s_waitcnt", "s_nop")):
        out.append("wait")
    elif op.startswith("s_") and not op.startswith(("s_barrier", "s_endpgm")):
        out.append("salu")
    elif op.startswith("scratch_"):
        out.append("scratch")
    return out


def blocks_of(path, key):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and ":" in l.split(";")[0])
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    blocks, cur = [], dict(label="entry", loop="", n=collections.Counter())
    for i in range(start + 1, end + 1):
        t = lines[i].strip()
        m = re.match(r"^\.(LBB\d+_\d+):", t)
        if m:
            blocks.append(cur)
            cur = dict(label=m.group(1), loop="", n=collections.Counter())
        loop = re.search(r"in Loop: Header=(\S+) Depth=(\d+)|Loop Header: Depth=(\d+)", lines[i])
        if loop and not cur["loop"]:
            cur["loop"] = f"{loop.group(1)} depth {loop.group(2)}" if loop.group(1) else f"{cur['label'][1:]} depth {loop.group(3)}"
        if m or not t or t.startswith((";", ".", "//")):
            continue
        cur["n"].update(classify(t.split()[0]))
    blocks.append(cur)
    return blocks


def row(name, n):
    return f"{name:34s}" + "".join(f"{n[c]:>8d}" for c in COLS)


def main():
    blocks = blocks_of(sys.argv[1], sys.argv[2])
    print(f"{'':34s}" + "".join(f"{c:>8s}" for c in COLS))
    if len(sys.argv) >= 5:
        labels = [b["label"] for b in blocks]
        a, z = labels.index(sys.argv[3]), labels.index(sys.argv[4])
        tot = collections.Counter()
        for b in blocks[a:z + 1]:
            tot.update(b["n"])
        print(row(f"{sys.argv[3]} .. {sys.argv[4]} ({z - a + 1} blocks)", tot))
        return
    loops, first, last = collections.defaultdict(collections.Counter), {}, {}
    for b in blocks:
        loops[b["loop"]].update(b["n"])
        first.setdefault(b["loop"], b["label"])
        last[b["loop"]] = b["label"]
    for k, n in loops.items():
        print(row((k or "outside every loop") + f" [{first[k]} .. {last[k]}]", n))


if __name__ == "__main__":
    main()

"""Which kernels of two `hipcc --cuda-device-only -S` listings of one unit differ.
A kernel is the lines from its label to s_endpgm plus its .amdhsa_kernel block, compared as a sorted multiset (instruction order is not
compared; lines with the per-build __hip_cuid symbol are dropped).  Exit status 1 if a kernel differs or exists in one listing only.
usage: isa_diff.py old.s new.s [-v]    (-v: the lines each side has alone)"""
import collections
import re
import sys


def kernels(path):
    lines = [l.rstrip() for l in open(path) if "__hip_cuid" not in l]
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out = collections.defaultdict(collections.Counter)
    i = 0
    while i < len(lines):
        m = re.match(r"(\S+):", lines[i])     # `name:    ; @name`
        label = m.group(1) if m else None
        head = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if label in names or head:
            name, last = (label, "s_endpgm") if label in names else (head.group(1), ".end_amdhsa_kernel")
            j = i
            while last not in lines[j]:
                j += 1
            out[name].update(l.strip() for l in lines[i:j + 1] if l.strip())
            i = j
        i += 1
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"only in {'new' if name in new else 'old'}: {name}")
            bad += 1
        elif old[name] != new[name]:
            gone, come = old[name] - new[name], new[name] - old[name]
            print(f"differs (-{sum(gone.values())} +{sum(come.values())} lines): {name}")
            if "-v" in sys.argv[3:]:
                for l, n in sorted(gone.items()):
                    print(f"    - {n} x {l}")
                for l, n in sorted(come.items()):
                    print(f"    + {n} x {l}")
            bad += 1
    print(f"{len(set(old) | set(new))} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

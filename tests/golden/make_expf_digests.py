"""Regenerate tests/golden/expf_digests.npz: the definition of "exact" for the device exponentials.

primitives_ref.expf (glibc 2.35's algorithm restated in numpy) is evaluated on all 2^32 binary32 bit patterns, in 4,096 blocks of 2^20
consecutive patterns.  NaN results become 0x7fc00000; per block two 64-bit words are kept, both mod 2^64: sum(bits) and
sum(bits * (i + 1)), i the index in the block.  tests/test_primitives_gpu.py asks the same two words of exact_expf and
exact_expf_select on the device.

    python tests/golden/make_expf_digests.py [--workers 16] [--out tests/golden/expf_digests.npz]

About 12 core-minutes.  The file is written with fixed zip metadata, so a rerun reproduces it byte for byte."""
import argparse
import io
import os
import sys
import zipfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N_BLOCKS = 4096
BATCH = 16   # blocks per task


def _task(first):
    import primitives_ref

    return first, primitives_ref.expf_block_digests(first, BATCH)


def write_npz(path, digests):
    buf = io.BytesIO()
    np.lib.format.write_array(buf, np.ascontiguousarray(digests, dtype="<u8"), version=(1, 0))
    info = zipfile.ZipInfo("digests.npy", date_time=(1980, 1, 1, 0, 0, 0))
    info.compress_type = zipfile.ZIP_STORED   # 64 KB; stored, so the bytes do not depend on the zlib at hand
    info.external_attr = 0o644 << 16
    with zipfile.ZipFile(path, "w") as z:
        z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(HERE, "expf_digests.npz"))
    args = ap.parse_args()
    digests = np.zeros((N_BLOCKS, 2), np.uint64)
    with ProcessPoolExecutor(max_workers=max(1, min(16, args.workers))) as pool:
        for first, d in pool.map(_task, range(0, N_BLOCKS, BATCH)):
            digests[first:first + BATCH] = d
    write_npz(args.out, digests)
    print(f"{args.out}: {N_BLOCKS} blocks, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()

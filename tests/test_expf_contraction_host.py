"""The host proof behind exact_expf's Horner polynomial (csrc/mnv_device.h): tools/expf_contraction_proof.cpp visits all 2^32 binary32
patterns and compares glibc 2.35's unfused evaluation of the polynomial with its fused variants, the kernels' Horner form among them, on
every input that reaches the polynomial.  CPU only, about ten seconds on 16 threads (the program sizes itself by OMP_NUM_THREADS)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.path.dirname(HERE), "tools", "expf_contraction_proof.cpp")
VARIANTS = ("fma_z", "fma_y", "fma_last", "fma_all", "horner")


def test_fused_polynomial_gives_glibc_bits_on_every_input(tmp_path):
    exe = str(tmp_path / "expf_contraction_proof")
    # -ffp-contract=off: the unfused evaluation must stay unfused; -march=native: std::fma is the hardware instruction where there is one
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=native", "-pthread", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(min(16, os.cpu_count() or 1)))
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    counts = dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2 and line.split()[1].isdigit())
    print(r.stdout)
    assert int(counts["patterns"]) == 1 << 32
    # every input but the special cases of |x| >= 88 (NaN, +-inf, overflow, underflow) reaches the polynomial: more than half of all patterns
    assert int(counts["main_path"]) == 2239849421
    for v in VARIANTS:
        assert int(counts["mismatch_" + v]) == 0, f"{v}: {counts['mismatch_' + v]} inputs differ from the unfused evaluation"
    # the comparison is live: the same polynomial on r rounded to binary32 does differ
    assert int(counts["mismatch_control_r_binary32"]) > 0
    assert r.returncode == 0 and "PROOF HOLDS" in r.stdout

"""The list of march_accel_kernel instantiations that tests/test_march_matrix_gpu.py must reach (march_matrix.VARIANTS) against the three
units that instantiate the kernel: a BASIS added to or dropped from one of their switches changes the list, and this test says so without a GPU."""
import os
import re

import march_matrix as mm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mega-nerf-viewer_amd", "csrc")


def instantiated_triples():
    """(BASIS, BRICK, RAYS) of every launch_march_mode<...> the three units name (the ray unit's template parameter BRICK is both)"""
    out = set()
    for unit in ("mnv_accel_march.hip", "mnv_accel_march_brick.hip", "mnv_accel_march_rays.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        found = re.findall(r"launch_march_mode<(-?\d+), (true|false|BRICK), (true|false)>", text)
        assert found, unit
        for b, brick, rays in found:
            for br in ((0, 1) if brick == "BRICK" else (int(brick == "true"),)):
                out.add((int(b), br, int(rays == "true")))
    return out


def test_the_variant_list_is_what_the_three_units_instantiate():
    # the MODEs of csrc/mnv_march_launch.h (launch_march_mode) per triple, MODE 1 (diagnostics) left out: frames have the tracked march,
    # BASIS 9 the colourless ones (samples: frames only; depth image), SH rows of frames the fast colour math
    want = set()
    for b, brick, rays in instantiated_triples():
        modes = {0} | (set() if rays else {2}) | ({5} if b == 9 else set()) | ({3} if b == 9 and not rays else set()) | ({4} if b >= 1 and not rays else set())
        want |= {(b, m, brick, rays) for m in modes}
    assert want == set(mm.VARIANTS), sorted(want ^ set(mm.VARIANTS))
    assert mm.planned_variants() == set(mm.VARIANTS), sorted(mm.planned_variants() ^ set(mm.VARIANTS))

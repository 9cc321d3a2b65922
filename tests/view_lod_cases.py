"""The scenes tests/test_view_lod_ref.py and tests/test_view_lod_gpu.py share: trees from test_lod_gpu's generators (offset 0.5 unless a
case says otherwise), viewpoints, and the counts tests/view_lod_ref.py gives for them."""
import numpy as np

from test_lod_gpu import _chain as chain, _random_tree as random_tree, _renumbered as renumbered, _with_unreached as with_unreached  # noqa: F401

# "mixed cut" scenes: tree = (seed, levels, data_dim, p); kept / partial are what the restatement gives (test_view_lod_ref asserts the
# conditions that make them mixed: more than the floor, less than the tree, partially kept levels at three depths or more)
MIXED = {
    "isotropic": dict(tree=(2, 7, 4, 0.35), total=1085, views=[((-0.25, 0.125, 0.0), 64.0)], pixels=8.0, scale=(1.0, 1.0, 1.0), min_depth=1,
                      kept=256, partial=[5, 6, 7]),
    "anisotropic": dict(tree=(2, 7, 4, 0.35), total=1085, views=[((-1.0, -0.25, 0.1), 48.0)], pixels=6.0, scale=(0.5, 1.0, 2.0), min_depth=1,
                        kept=294, partial=[5, 6, 7]),
    "anisotropic_deep": dict(tree=(3, 8, 4, 0.30), total=1180, views=[((-1.0, -0.25, 0.1), 48.0)], pixels=6.0, scale=(0.5, 1.0, 2.0), min_depth=1,
                             kept=136, partial=[5, 6, 7, 8]),
}
TWO_VIEWS = dict(tree=(2, 7, 4, 0.35), views=[((-0.5, -0.5, -0.5), 64.0), ((0.5, 0.5, 0.25), 32.0)], pixels=8.0, kept=65, kept_first=59)


def tie_chain():
    """(data, child, offset, scale, views, pixels): six chunks in a chain through the voxels 4, 0, 4, 0, 0 -- integer x corners 1, 2, 5,
    10, 20 at depths 1 .. 5, y and z corners 0 -- seen from (0.5, 0, 0) with focal_px / pixels == 1 in a tree whose space is the world's."""
    child = np.zeros((6, 8), np.int32)
    for c, j in enumerate((4, 0, 4, 0, 0)):
        child[c, j] = 1
    data = np.random.default_rng(6).uniform(0.1, 9, size=(6, 8, 4)).astype(np.float16).view(np.uint16)
    return np.ascontiguousarray(data), child, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), [((0.5, 0.0, 0.0), 4.0)], 4.0

"""The host half of anti-aliased frames (no GPU): mnv_aa_pattern and mnv_aa_weights equal the restatements of tests/aa_ref.py bit for
bit, refuse what include/mnv.h says they refuse, and follow the size-query convention of mnv_n3tree_gen_wireframe."""
import ctypes as C

import numpy as np
import pytest

import aa_ref

KS = [1, 2, 3, 4, 8, 16, 64]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("k", KS)
def test_pattern_equals_the_restatement(mnv, k):
    got = mnv.aa_pattern(k)
    assert got.shape == (k, 2) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(aa_ref.pattern(k)))
    assert (got >= -0.5).all() and (got < 0.5).all()
    if k == 1:
        assert np.array_equal(bits(got), bits(np.zeros((1, 2), np.float32)))   # +0, +0
    else:
        assert len({tuple(p) for p in got.tolist()}) == k                      # distinct points
        assert np.array_equal(bits(got[:2]), bits(np.array([[0.0, 1 / 3 - 0.5], [-0.25, 2 / 3 - 0.5]], np.float64).astype(np.float32)))


def test_pattern_refuses_bad_counts(mnv):
    buf = np.full((66, 2), 7.0, np.float32)
    for k in (0, 65, -1):
        assert mnv.lib().mnv_aa_pattern(k, buf.ctypes.data) == mnv.MNV_E_INVALID
        with pytest.raises(mnv.MnvError) as e:
            mnv.aa_pattern(k)
        assert e.value.code == mnv.MNV_E_INVALID
    assert (buf == 7.0).all()                                                  # nothing was written
    assert mnv.lib().mnv_aa_pattern(4, None) == mnv.MNV_E_INVALID
    assert mnv.MAX_BATCH == 64 and (mnv.AA_BOX, mnv.AA_TENT) == (aa_ref.AA_BOX, aa_ref.AA_TENT)


@pytest.mark.parametrize("k", KS)
def test_weight_tables_equal_the_restatement(mnv, k):
    off = mnv.aa_pattern(k)
    box = mnv.aa_weights(mnv.AA_BOX, off)
    assert box.shape == (k, 1, 1) and np.array_equal(bits(box), bits(np.ones((k, 1, 1), np.float32)))
    assert np.array_equal(bits(box), bits(aa_ref.weights(aa_ref.AA_BOX, off)))
    tent = mnv.aa_weights(mnv.AA_TENT, off)
    assert tent.shape == (k, 3, 3) and tent.dtype == np.float32
    assert np.array_equal(bits(tent), bits(aa_ref.weights(aa_ref.AA_TENT, off)))
    # a tent of one pixel radius is a partition of unity over the pixel grid: every sample hands out weight 1 in all
    assert np.allclose(tent.reshape(k, 9).sum(axis=1), 1.0, atol=1e-6)
    if k == 1:
        centre = np.zeros((3, 3), np.float32)
        centre[1, 1] = 1.0
        assert np.array_equal(bits(tent[0]), bits(centre))                     # the sample at the pixel centre belongs to its pixel alone


def test_weight_tables_of_arbitrary_offsets(mnv):
    """Offsets that are not the pattern's, both ends of the range included."""
    off = np.array([[-0.5, -0.5], [0.49999997, 0.25], [0.0, -0.125], [0.3, -0.3]], np.float32)
    assert np.array_equal(bits(mnv.aa_weights(mnv.AA_TENT, off)), bits(aa_ref.weights(aa_ref.AA_TENT, off)))
    w = mnv.aa_weights(mnv.AA_TENT, off[:1])[0]
    assert np.array_equal(bits(w), bits(np.array([[0, 0, 0], [0, 0.25, 0.25], [0, 0.25, 0.25]], np.float32)))   # a sample on a pixel's upper left corner
    w = mnv.aa_weights(mnv.AA_TENT, off[3:])[0]                                 # (0.3, -0.3): i along x (last index), j along y
    assert w[1, 0] > 0 and w[1, 2] == 0 and w[2, 1] > 0 and w[0, 1] == 0        # the left / lower neighbour's sample lies within one pixel


def test_weights_size_query_and_refusals(mnv):
    lib = mnv.lib()
    off = mnv.aa_pattern(5)
    r, n = C.c_int32(-1), C.c_int64(-1)
    assert lib.mnv_aa_weights(mnv.AA_TENT, 5, off.ctypes.data, C.byref(r), None, 0, C.byref(n)) == mnv.MNV_OK
    assert (r.value, n.value) == (1, 45)
    assert lib.mnv_aa_weights(mnv.AA_BOX, 5, off.ctypes.data, C.byref(r), None, 0, C.byref(n)) == mnv.MNV_OK
    assert (r.value, n.value) == (0, 5)
    assert lib.mnv_aa_weights(mnv.AA_TENT, 5, off.ctypes.data, None, None, 0, None) == mnv.MNV_OK         # both may be null
    short = np.full(44, 7.0, np.float32)
    n.value = -1
    assert lib.mnv_aa_weights(mnv.AA_TENT, 5, off.ctypes.data, C.byref(r), short.ctypes.data, 44, C.byref(n)) == mnv.MNV_E_INVALID
    assert n.value == 45 and (short == 7.0).all()                              # says what it needs, writes nothing
    roomy = np.full(50, 7.0, np.float32)
    assert lib.mnv_aa_weights(mnv.AA_TENT, 5, off.ctypes.data, C.byref(r), roomy.ctypes.data, 50, C.byref(n)) == mnv.MNV_OK
    assert np.array_equal(bits(roomy[:45]), bits(aa_ref.weights(aa_ref.AA_TENT, off)).reshape(-1)) and (roomy[45:] == 7.0).all()
    for args in ((2, 5, off.ctypes.data), (-1, 5, off.ctypes.data), (mnv.AA_TENT, 0, off.ctypes.data), (mnv.AA_TENT, 65, off.ctypes.data),
                 (mnv.AA_TENT, 5, None)):
        assert lib.mnv_aa_weights(args[0], args[1], args[2], C.byref(r), None, 0, C.byref(n)) == mnv.MNV_E_INVALID, args
    assert lib.mnv_aa_weights(mnv.AA_TENT, 5, off.ctypes.data, C.byref(r), None, 45, C.byref(n)) == mnv.MNV_E_INVALID   # a capacity without a buffer
    assert lib.mnv_aa_weights(mnv.AA_TENT, 5, off.ctypes.data, C.byref(r), roomy.ctypes.data, -1, C.byref(n)) == mnv.MNV_E_INVALID


def test_restated_resolve_on_a_case_worked_by_hand():
    """aa_ref.resolve itself: two samples, radius 1, a 2 x 1 frame; the border renormalises over what exists."""
    sub = np.zeros((2, 1, 2, 4), np.float32)
    sub[0, 0, 0], sub[0, 0, 1] = 1.0, 3.0
    sub[1, 0, 0], sub[1, 0, 1] = 5.0, 7.0
    w = np.zeros((2, 3, 3), np.float32)
    w[0, 1, 1], w[0, 1, 2] = 2.0, 1.0        # sample 0: own pixel 2, right neighbour 1
    w[1, 1, 0] = 4.0                         # sample 1: left neighbour 4
    out, u8 = aa_ref.resolve(sub, w, 1)
    assert out[0, 0, 0] == np.float32((2 * 1 + 1 * 3) / 3)            # no left neighbour: the term and its weight are missing
    assert out[0, 1, 0] == np.float32((2 * 3 + 4 * 5) / 6)            # no right neighbour
    assert np.array_equal(u8, np.full((1, 2, 4), 255, np.uint8))
    zero, z8 = aa_ref.resolve(sub, np.zeros((2, 3, 3), np.float32), 1)
    assert not zero.any() and not z8.any()
    assert np.array_equal(aa_ref.pack_u8(np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 0.999], np.float32)), np.array([0, 0, 127, 255, 255, 254], np.uint8))

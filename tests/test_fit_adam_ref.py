"""The numpy restatement of "fitting on a photo set" (tests/fit_adam_ref.py) held on the CPU: (a) the batcher's permutation is a bijection
that changes with seed and epoch; (b) the batches of an epoch partition the cameras' pixels, the padded lanes being exactly the edge
tiles' outside lanes; (c) the restated rays are tests/rays_ref.py's pinhole rays at those pixels, bit for bit; (d) the binary32 Adam step
stays within a measured bound of the same step in binary64; (e) on the fit scene of tests/fit_cases.py full-batch Adam at its default rates
falls at every step and ends below SGD, and mini-batch Adam brings the full loss down.  tests/test_fit_adam_gpu.py holds the device against
the same restatement.  These are property tests of the restatement, which ships with them: they need the library's cameras and the oracle
but none of its new entry points, so they hold on any commit that has tests/fit_adam_ref.py; the tests that fail without the feature
are the device's."""
import numpy as np
import pytest

import cases
import fit_adam_ref as far
import fit_cases
import fit_ref
import rays_ref

bits = cases.bits
F = np.float32

# (d): measured here on 4000 x 13 random words per step number (1, 2, 1000): the largest error of the new master, relative to the larger of
# |master| and the update's scale, was 3.24e-7 (step 1; 2.99e-7 and 2.64e-7 at steps 2 and 1000); of the first moment, relative to
# |m1 beta1| + |g (1 - beta1)|, 1.50e-7; of the second moment 2.49e-7 -- three to nine binary32 roundings of 2^-24 = 6e-8 each.  Rounding
# differs per input, hence 4 x the maximum.
ADAM_F32_BOUND = 4 * 3.24e-7

@pytest.mark.parametrize("units", [1, 2, 3, 4, 5, 63, 64, 65, 1000, 65537])
def test_perm_is_a_bijection_that_changes_with_seed_and_epoch(units):
    orders = {}
    for seed in (0, 0x123456789ABCDEF):
        for epoch in (0, 1):
            p = far.perm(units, seed, epoch, np.arange(units))
            assert np.array_equal(np.sort(p), np.arange(units)), (seed, epoch)
            orders[(seed, epoch)] = p
    if units >= 64:
        keys = list(orders)
        for i, a in enumerate(keys):
            assert not np.array_equal(orders[a], np.arange(units))
            for b in keys[i + 1:]:
                assert not np.array_equal(orders[a], orders[b]), (a, b)


def test_perm_takes_single_places_and_the_last_epoch():
    whole = far.perm(1000, 7, 2 ** 31 - 1, np.arange(1000))
    assert np.array_equal(np.sort(whole), np.arange(1000))
    assert np.array_equal(far.perm(1000, 7, 2 ** 31 - 1, [999, 5, 6]), whole[[999, 5, 6]])
    assert not np.array_equal(whole, far.perm(1000, 7, 0, np.arange(1000)))


@pytest.mark.parametrize("tile", [8, 1])
def test_batches_of_an_epoch_partition_the_pixels_and_rays_are_the_pinhole_rays(mnv, tile):
    cams = [c.c for c in far.batch_cameras(mnv)]
    targets = far.batch_targets(cams)
    prefix = far.unit_table(cams, tile)
    total = int(prefix[-1])
    assert total == (4 * 3 + 2 * 3 + 1 if tile == 8 else sum(w * h for w, h in far.SIZES))
    per_batch = 5 if tile == 8 else 97          # (neither divides U: the last batch is short)
    seen = [np.zeros((c.height, c.width), np.int64) for c in cams]
    full = [rays_ref.pinhole_rays(c) for c in cams]
    padded = 0
    for first in range(0, total, per_batch):
        D = far.draw(cams, targets, tile, 11, 3, first, min(per_batch, total - first))
        for ci, c in enumerate(cams):
            s = (D["cam"] == ci) & D["inside"]
            np.add.at(seen[ci], (D["iy"][s], D["ix"][s]), 1)
            # (c) rays and targets of the inside lanes: gathered from the whole image's
            assert np.array_equal(bits(D["o"][s]), bits(full[ci][0][D["iy"][s], D["ix"][s]]))
            assert np.array_equal(bits(D["d"][s]), bits(full[ci][1][D["iy"][s], D["ix"][s]]))
            assert np.array_equal(bits(D["target"][s]), bits(targets[ci][D["iy"][s], D["ix"][s]]))
            out = (D["cam"] == ci) & ~D["inside"]
            assert (D["ix"][out] >= c.width).__or__(D["iy"][out] >= c.height).all()
            assert not D["d"][out].any() and not D["target"][out].any()
            assert np.array_equal(bits(D["o"][out]), bits(np.broadcast_to(np.array(list(c.c2w), F)[9:12], D["o"][out].shape)))
        padded += int((~D["inside"]).sum())
    assert all((s == 1).all() for s in seen)
    # the padded lanes are exactly the edge tiles' outside lanes: 32 x 20 -> 4 tiles x 4 rows; 9 x 17 -> a 16 x 24 frame of tiles
    assert padded == ((32 * 24 - 32 * 20) + (16 * 24 - 9 * 17) if tile == 8 else 0)


def test_restated_lane_order_within_a_tile(mnv):
    cams = [c.c for c in far.batch_cameras(mnv)]
    cam, ix, iy, inside = far.unit_pixels(cams, 8, [5])          # camera 0's tile (1, 1)
    assert cam.tolist() == [0] * 64 and ix[:9].tolist() == [8, 9, 10, 11, 12, 13, 14, 15, 8] and iy[:9].tolist() == [8] * 8 + [9]
    assert inside.sum() == 64
    cam, ix, iy, inside = far.unit_pixels(cams, 8, [12 + 1])     # camera 1 (9 x 17): tile (1, 0) holds column 8 alone
    assert cam[0] == 1 and inside.reshape(8, 8)[:, 0].all() and not inside.reshape(8, 8)[:, 1:].any()


def _random_rows(rng, n_rows, dd):
    master = (rng.normal(size=(n_rows, dd)) * 10.0 ** rng.uniform(-3, 2, size=(n_rows, dd))).astype(F)
    m1 = (rng.normal(size=(n_rows, dd)) * 10.0 ** rng.uniform(-4, 1, size=(n_rows, dd))).astype(F)
    m2 = (rng.normal(size=(n_rows, dd)) ** 2 * 10.0 ** rng.uniform(-8, 2, size=(n_rows, dd))).astype(F)
    acc = (rng.normal(size=(n_rows, dd)) * 10.0 ** rng.uniform(-4, 1, size=(n_rows, dd)) * far.Q32).astype(np.int64)
    acc[rng.uniform(size=n_rows) < 0.3] = 0
    return master, m1, m2, acc


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_step_against_binary64(step):
    rng = np.random.default_rng(100 + step)
    n_rows, dd = 4000, 13
    master, m1, m2, acc = _random_rows(rng, n_rows, dd)
    p = far.ADAM
    args = (p["lr_colour"], p["lr_sigma"], p["beta1"], p["beta2"], p["eps"])
    want_m, want_a, want_v = far.adam_step64(master, m1, m2, acc, step, *args)
    data = np.zeros((n_rows, dd), np.uint16)
    got_m, got_a, got_v, left = master.copy(), m1.copy(), m2.copy(), acc.copy()
    far.adam_step(data, got_m, got_a, got_v, left, step, *args)
    touched = acc.any(axis=1)
    assert not left.any() and touched.sum() > 2000
    assert np.array_equal(bits(got_m[~touched]), bits(master[~touched])) and not data[~touched].any()
    g = acc.astype(np.float64) / far.Q32
    b1, b2 = float(F(p["beta1"])), float(F(p["beta2"]))
    # the update's scale with the two terms of the first moment taken by magnitude: where they cancel, the update inherits the moment's
    # rounding error, which is relative to the terms and not to their difference
    lr = np.full(dd, float(F(p["lr_colour"])))
    lr[dd - 1] = float(F(p["lr_sigma"]))
    a_mag = np.abs(m1 * b1) + np.abs(g * (1 - b1))
    upd = lr[None, :] * (a_mag / (1 - b1 ** step)) / (np.sqrt(want_v / (1 - b2 ** step)) + float(F(p["eps"])))
    clamped = np.zeros(acc.shape, bool)
    clamped[:, dd - 1] = want_m[:, dd - 1] == 0.0                       # (the clamp discards the update: no relative error there)
    sel = touched[:, None] & ~clamped
    err_m = (np.abs(got_m - want_m) / np.maximum(np.abs(master.astype(np.float64)), upd))[sel].max()
    err_a = (np.abs(got_a - want_a) / (np.abs(m1 * b1) + np.abs(g * (1 - b1))))[touched].max()
    err_v = (np.abs(got_v - want_v) / (m2 * b2 + g * g * (1 - b2)))[touched].max()
    print(f"step {step}: relative error master {err_m:.3e}, m1 {err_a:.3e}, m2 {err_v:.3e}")
    assert max(err_m, err_a, err_v) < ADAM_F32_BOUND
    assert np.array_equal(data[touched], fit_ref.half_sat(got_m[touched]))


def test_adam_consts_and_special_rows():
    omb1, omb2, c1, c2 = far.adam_consts(0.9, 0.999, 1)
    assert bits(omb1) == bits(F(1.0) - F(0.9)) and c1 == F(1.0 / (1.0 - float(F(0.9)))) and c2 == F(1.0 / (1.0 - float(F(0.999))))
    assert far.adam_consts(0.9, 0.999, 100000)[2:] == (F(1.0), F(1.0))
    # a first step from zero moments moves every touched word by lr (|a c1| / sqrt(v c2) is 1 up to rounding), whatever the gradient's size
    data = np.zeros((3, 4), np.uint16)
    master = np.full((3, 4), 2.0, F)
    m1, m2 = np.zeros((3, 4), F), np.zeros((3, 4), F)
    acc = np.zeros((3, 4), np.int64)
    acc[0] = [1 << 30, -(1 << 40), 1 << 50, -(1 << 33)]
    acc[2] = [0, 0, 0, 1 << 62]
    far.adam_step(data, master, m1, m2, acc, 1, 0.5, 4.0)
    assert np.allclose(master[0], [1.5, 2.5, 1.5, 6.0], rtol=1e-6) and np.array_equal(master[1], np.full(4, 2.0, F))
    assert master[2].tolist() == [2.0, 2.0, 2.0, 0.0]                  # zero words of a touched row: a = 0, no move; the density is clamped
    assert data[1].tolist() == [0, 0, 0, 0] and data[2].tolist() == [0x4000, 0x4000, 0x4000, 0]
    assert not acc.any()


@pytest.fixture(scope="module")
def scene(mnv, orc):
    return far.fit_scene(mnv, orc)


def _fresh(scene):
    return dict(scene["T"], data=scene["T"]["data"].copy())


def test_full_batch_adam_falls_at_every_step_and_beats_sgd(scene):
    S, s = fit_cases.FIT, scene
    se, n_rays = far.fit_ex(_fresh(s), s["opt"], s["cams"], s["targets"], S["iterations"], "adam", rays=s["rays"])
    sgd = fit_ref.fit(_fresh(s), s["opt"], s["rays"], s["targets"], S["iterations"], S["lr_colour"], S["lr_sigma"])
    print("adam se_q32 / 2^32 per step:", " ".join(f"{x / far.Q32:.4f}" for x in se))
    print("sgd  se_q32 / 2^32 per step:", " ".join(f"{x / far.Q32:.4f}" for x in sgd))
    assert len(se) == S["iterations"] and all(b < a for a, b in zip(se, se[1:])), se
    assert se[-1] < 0.75 * se[0]
    assert se[-1] < sgd[-1] and se[0] == sgd[0]
    assert len(set(n_rays)) == 1 and 0 < n_rays[0] <= S["cameras"] * S["size"] ** 2
    # SGD with full batch through the new loop is fit_ref.fit
    se2, _ = far.fit_ex(_fresh(s), s["opt"], s["cams"], s["targets"], 2, "sgd", S["lr_colour"], S["lr_sigma"], rays=s["rays"])
    assert se2 == sgd[:2]


def test_mini_batch_adam_brings_the_full_loss_down(scene):
    s = scene
    T = _fresh(s)
    before = far.full_loss(T, s["opt"], s["cams"], s["targets"], s["rays"])
    units = int(far.unit_table(s["cams"], 8)[-1])
    assert units == 12                                                     # three 16 x 16 cameras: three batches of 4 tiles per epoch
    se, n_rays = far.fit_ex(T, s["opt"], s["cams"], s["targets"], 8 * 3, "adam", batch_rays=4 * 64, tile=8, seed=1)
    after = far.full_loss(T, s["opt"], s["cams"], s["targets"], s["rays"])
    print(f"full loss / 2^32: {before / far.Q32:.4f} -> {after / far.Q32:.4f} ({after / before:.3f})")
    assert after < 0.75 * before
    assert all(0 < n <= 256 for n in n_rays) and sum(n_rays[:3]) == sum(n_rays[3:6])    # an epoch holds every counted ray once

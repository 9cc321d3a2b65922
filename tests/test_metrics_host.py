"""Frame metrics, the host half (no GPU): the SSIM window, mnv_metrics_finish, the argument checks of mnv_frame_metrics (which return before
any device call) and the PNM reader of `mnv_render --target`."""
import ctypes as C
import math

import numpy as np
import pytest

import metrics_ref as ref


def test_ssim_window_is_symmetric_normalised_and_numpys(mnv):
    g = mnv.ssim_window()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert np.array_equal(g, g[::-1])
    assert abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-6
    e = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / 4.5)
    want = (e / e.sum()).astype(np.float32)
    for got, w in zip(g, want):
        assert abs(float(got) - float(w)) <= float(np.spacing(w)), (got, w)
    assert np.array_equal(g, ref.ssim_window())       # the restatement takes the sum in index order, as the library does


@pytest.mark.parametrize("words", [(100, 3 << 30, 40, 5 << 31), (7, 1, 1, -12345), (1 << 28, 3 << 59, 1 << 27, 3 << 58)])
def test_metrics_finish_arithmetic(mnv, words):
    n_px, se, n_win, ss = words
    got = mnv.metrics_finish(words)
    mse = se / 4294967296.0 / (3.0 * n_px)
    assert got["mse"] == mse and got["psnr"] == -10.0 * math.log10(mse)
    assert got["ssim"] == ss / 4294967296.0 / (3.0 * n_win)
    assert (got["n_px"], got["n_win"]) == (n_px, n_win)
    assert got == ref.finish(words)


def test_metrics_finish_inf_and_nan(mnv):
    same = mnv.metrics_finish((50, 0, 4, 12 << 32))     # a frame against itself
    assert same["mse"] == 0.0 and same["psnr"] == math.inf and same["ssim"] == 1.0
    no_window = mnv.metrics_finish((50, 1 << 32, 0, 0))
    assert math.isnan(no_window["ssim"]) and no_window["n_win"] == 0 and math.isfinite(no_window["psnr"])
    nothing = mnv.metrics_finish((0, 0, 0, 0))          # every pixel masked out
    assert math.isnan(nothing["mse"]) and math.isnan(nothing["psnr"]) and math.isnan(nothing["ssim"])
    assert mnv.lib().mnv_metrics_finish(None, None) == mnv.MNV_E_INVALID
    assert mnv.lib().mnv_ssim_window(None) == mnv.MNV_E_INVALID


def test_frame_metrics_refuses_bad_arguments_before_any_device_call(mnv):
    """Fake (never dereferenced) addresses with the alignment under test: every case returns MNV_E_INVALID on a machine without a GPU."""
    fm = mnv.lib().mnv_frame_metrics
    rgba, tgt, sums, amap = 0x10000, 0x20000, 0x30000, 0x40000
    ok = dict(rgba=rgba, tgt=tgt, w=16, h=16, flags=7, win=None, sums=sums, se=None, ss=None)

    def call(**kw):
        a = dict(ok, **kw)
        return fm(a["rgba"], a["tgt"], a["w"], a["h"], a["flags"], a["win"], a["sums"], a["se"], a["ss"], None)

    bad = [dict(rgba=None), dict(tgt=None), dict(sums=None), dict(w=0), dict(h=0), dict(w=-3), dict(h=-1),
           dict(w=1 << 14, h=(1 << 14) + 1),                       # 2^28 + 2^14 pixels
           dict(rgba=rgba + 8), dict(rgba=rgba + 4), dict(tgt=tgt + 1), dict(tgt=tgt + 2), dict(sums=sums + 4),
           dict(se=amap + 2), dict(ss=amap + 1), dict(flags=8), dict(flags=-1), dict(flags=1 << 20)]
    for kw in bad:
        assert call(**kw) == mnv.MNV_E_INVALID, kw
        assert mnv.lib().mnv_last_error().decode().startswith("mnv_frame_metrics"), kw


def _write(path, header: bytes, data: bytes):
    with open(path, "wb") as f:
        f.write(header + data)
    return str(path)


def test_pnm_read_good_files(mnv, tmp_path):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    p6 = _write(tmp_path / "a.ppm", b"P6\n13 7\n255\n", rgb.tobytes())       # byte for byte what mnv_render --out writes
    got = mnv.pnm_read(p6)
    assert got.shape == (7, 13, 3) and np.array_equal(got, rgb)
    assert np.array_equal(mnv.pnm_read(p6, 13, 7), rgb)
    grey = rng.integers(0, 256, (5, 9, 1), dtype=np.uint8)
    p5 = _write(tmp_path / "m.pgm", b"P5 9 5 255\n", grey.tobytes())
    assert np.array_equal(mnv.pnm_read(p5), grey)
    # the size query alone, and a buffer that is too short
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    rd = mnv.lib().mnv_pnm_read
    assert rd(p6.encode(), 0, 0, None, 0, C.byref(w), C.byref(h), C.byref(ch)) == 0 and (w.value, h.value, ch.value) == (13, 7, 3)
    buf = np.zeros(13 * 7 * 3 - 1, np.uint8)
    assert rd(p6.encode(), 0, 0, buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ch)) == mnv.MNV_E_INVALID
    assert (w.value, h.value, ch.value) == (13, 7, 3)
    assert rd(None, 0, 0, None, 0, None, None, None) == mnv.MNV_E_INVALID


def test_pnm_read_comment_lines(mnv, tmp_path):
    """`#` comments are part of the format: anywhere in the header before the maxval's terminator, to the end of the line."""
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    p = _write(tmp_path / "c.ppm", b"P6\n# made by a tool\n3 # the width\n# and the height:\n2\n#255\n255\n", rgb.tobytes())
    assert np.array_equal(mnv.pnm_read(p), rgb)
    # a comment that never ends, and data that happens to start with '#': the header ends after ONE white-space byte
    with pytest.raises(mnv.MnvError) as e:
        mnv.pnm_read(_write(tmp_path / "d.ppm", b"P6\n3 2\n# 255", b""))
    assert e.value.code == mnv.MNV_E_IO
    data = b"#" + bytes(range(17))
    assert mnv.pnm_read(_write(tmp_path / "e.ppm", b"P6 3 2 255 ", data)).tobytes() == data


@pytest.mark.parametrize("name,blob,kw", [
    ("truncated header", b"P6\n13 7\n", {}),
    ("truncated header in a number", b"P6\n13 7\n25", {}),
    ("empty file", b"", {}),
    ("wrong magic", b"P3\n1 1\n255\n0 0 0\n", {}),
    ("wrong magic, short", b"P", {}),
    ("maxval 65535", b"P6\n2 2\n65535\n" + bytes(24), {}),
    ("maxval 254", b"P5\n2 2\n254\n" + bytes(4), {}),
    ("zero width", b"P5\n0 2\n255\n", {}),
    ("a number of twenty digits", b"P5\n11111111111111111111 2\n255\n", {}),
    ("letters in the header", b"P6\n13 x7\n255\n" + bytes(300), {}),
    ("no separator", b"P5\n1 1\n255", {}),
    ("short data", b"P6\n13 7\n255\n" + bytes(13 * 7 * 3 - 1), {}),
    ("wrong size", b"P6\n13 7\n255\n" + bytes(13 * 7 * 3), dict(expect_width=7, expect_height=13)),
    ("wrong height", b"P6\n13 7\n255\n" + bytes(13 * 7 * 3), dict(expect_width=13, expect_height=8)),
])
def test_pnm_read_refuses(mnv, tmp_path, name, blob, kw):
    p = _write(tmp_path / "bad.pnm", blob, b"")
    with pytest.raises(mnv.MnvError) as e:
        mnv.pnm_read(p, **kw)
    assert e.value.code == mnv.MNV_E_IO, name
    assert "bad.pnm" in str(e.value)


def test_pnm_read_missing_file(mnv, tmp_path):
    with pytest.raises(mnv.MnvError) as e:
        mnv.pnm_read(str(tmp_path / "nothing.ppm"))
    assert e.value.code == mnv.MNV_E_IO


def test_restatement_on_known_values():
    """The numpy restatement itself: a frame that equals its target scores 0 / 1, one changed pixel changes exactly the windows over it."""
    rng = np.random.default_rng(1)
    f = rng.random((20, 24, 4), dtype=np.float32)
    t8 = np.concatenate([ref.pack(f[..., :3]), np.full((20, 24, 1), 255, np.uint8)], axis=2)
    sums, se_map, ssim_map = ref.frame_metrics(f, t8, ref.QUANTISED | ref.SSIM)
    assert list(sums) == [480, 0, 140, 3 * 140 << 32, 0] and not se_map.any() and (ssim_map == 1).all()
    t8[10, 12, 0] ^= 0x80
    sums2, se2, ssim2 = ref.frame_metrics(f, t8, ref.QUANTISED | ref.SSIM)
    assert np.count_nonzero(se2) == 1 and sums2[1] == int(np.rint(float(se2[10, 12]) * 2.0 ** 32))
    changed = np.argwhere((ssim2 != 1).any(axis=2))
    assert changed[:, 0].min() == 0 and changed[:, 0].max() == 9 and changed[:, 1].min() == 2 and changed[:, 1].max() == 12
    masked = t8.copy()
    masked[10, 12, 3] = 0
    sums3, _, _ = ref.frame_metrics(f, masked, ref.QUANTISED | ref.SSIM | ref.MASK_ALPHA)
    assert list(sums3[:3]) == [479, 0, 140 - len(changed)] and sums3[3] == 3 * sums3[2] << 32

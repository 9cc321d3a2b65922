"""The metric contract of include/mnv.h (mnv_frame_metrics) restated in numpy: float32 arrays, the same operations in the same order, every
product and sum rounded separately, IEEE division; np.rint on float64 for the 2^-32 fixed-point words; int64 sums.  No GPU, no tolerance: the
kernel's sums and maps equal these bit for bit."""
import math

import numpy as np

QUANTISED, MASK_ALPHA, SSIM = 1, 2, 4
F = np.float32
C1, C2 = F(1e-4), F(9e-4)
TWO32 = 4294967296.0


def ssim_window() -> np.ndarray:
    """mnv_ssim_window: exp(-(i - 5)^2 / 4.5) in double, divided by the sum taken in index order, rounded to float."""
    e = [math.exp(-float((i - 5) * (i - 5)) / 4.5) for i in range(11)]
    s = 0.0
    for v in e:
        s = s + v
    return np.array([v / s for v in e], np.float64).astype(F)


def pack(v: np.ndarray) -> np.ndarray:
    """The truncating pack of mnv_resolve_samples: s = v * 255; 0 unless s > 0, 255 if s >= 255, else (uint8)s."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = v.astype(F) * F(255)
        out = np.zeros(s.shape, np.uint8)
        mid = (s > 0) & (s < 255)
        out[mid] = s[mid].astype(np.uint8)
        out[s >= 255] = 255
    return out


def frame_values(rgba: np.ndarray, flags: int) -> np.ndarray:
    """x of the three colour channels, float32 [h, w, 3]."""
    v = rgba[..., :3].astype(F)
    if flags & QUANTISED:
        return pack(v).astype(F) / F(255)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.where(v < 1, v, F(1)), F(0)).astype(F)


def q32(term: np.ndarray) -> np.ndarray:
    return np.rint(term.astype(np.float64) * TWO32).astype(np.int64)


def _filter(v: np.ndarray, g: np.ndarray) -> np.ndarray:
    """[h, w, 3] -> [h - 10, w - 10, 3]: along x, then along y, each h = 0; h = h + g[i] * v in index order."""
    h, w = v.shape[:2]
    row = np.zeros((h, w - 10, 3), F)
    for i in range(11):
        row = row + g[i] * v[:, i:i + w - 10]
    out = np.zeros((h - 10, w - 10, 3), F)
    for j in range(11):
        out = out + g[j] * row[j:j + h - 10]
    return out


def frame_metrics(rgba: np.ndarray, target8: np.ndarray, flags: int = 0, window=None):
    """(sums int64 [5], se_map float32 [h, w], ssim_map float32 [h - 10, w - 10, 3] or None when the frame has no window or MNV_METRIC_SSIM
    is not set) of a float32 [h, w, 4] frame against a uint8 [h, w, 4] target."""
    h, w = rgba.shape[:2]
    x = frame_values(rgba, flags)
    t = target8[..., :3].astype(F) / F(255)
    included = (target8[..., 3] != 0) if flags & MASK_ALPHA else np.ones((h, w), bool)
    e = x - t
    se = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    sums = np.zeros(5, np.int64)
    sums[0] = int(included.sum())
    sums[1] = int(q32(se)[included].sum(dtype=np.int64))
    se_map = np.where(included, se, F(0)).astype(F)
    ssim_map = None
    if flags & SSIM and w >= 11 and h >= 11:
        g = ssim_window() if window is None else np.asarray(window, F)
        mx, my = _filter(x, g), _filter(t, g)
        exx, eyy, exy = _filter(x * x, g), _filter(t * t, g), _filter(x * t, g)
        mxx, myy, mxy = mx * mx, my * my, mx * my
        sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
        num = (F(2) * mxy + C1) * (F(2) * sxy + C2)
        den = ((mxx + myy) + C1) * ((sxx + syy) + C2)
        s = (num / den).astype(F)
        count = np.zeros((h - 10, w - 10), np.int64)
        for j in range(11):
            for i in range(11):
                count += included[j:j + h - 10, i:i + w - 10]
        win_in = count == 121
        sums[2] = int(win_in.sum())
        sums[3] = int(q32(s)[win_in].sum(dtype=np.int64))
        ssim_map = np.where(win_in[..., None], s, F(0)).astype(F)
    return sums, se_map, ssim_map


def finish(sums) -> dict:
    """mnv_metrics_finish in Python floats (IEEE double, the C library's log10)."""
    n_px, se, n_win, ss = (int(v) for v in list(sums)[:4])
    nan = float("nan")
    mse = se / TWO32 / (3.0 * n_px) if n_px > 0 else nan
    psnr = (-10.0 * math.log10(mse) if mse > 0 else float("inf")) if n_px > 0 else nan
    ssim = ss / TWO32 / (3.0 * n_win) if n_win > 0 else nan
    return {"mse": mse, "psnr": psnr, "ssim": ssim, "n_px": n_px, "n_win": n_win}


def random_frame(rng, h: int, w: int) -> np.ndarray:
    """Random floats in [0, 1) with 5 % exact 0, 5 % exact 1, 5 % 1.5, 2 % -0.25 and a few NaN / inf."""
    f = rng.random((h, w, 4), dtype=F)
    u = rng.random((h, w, 4))
    f[u < 0.05] = 0.0
    f[(u >= 0.05) & (u < 0.10)] = 1.0
    f[(u >= 0.10) & (u < 0.15)] = 1.5
    f[(u >= 0.15) & (u < 0.17)] = -0.25
    f[(u >= 0.17) & (u < 0.175)] = np.nan
    f[(u >= 0.175) & (u < 0.18)] = np.inf
    f[(u >= 0.18) & (u < 0.182)] = -np.inf
    return f

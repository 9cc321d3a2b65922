"""numpy restatements of the anti-aliasing recipes stated in include/mnv.h: the sample pattern (mnv_aa_pattern), the filter tables
(mnv_aa_weights) and the resolve contract (mnv_resolve_samples).  Every float operation of the resolve is a float32 numpy operation, in
the contract's order per pixel: vectorised over pixels, looped over (k, j, i)."""
import numpy as np

AA_BOX, AA_TENT = 0, 1


def radical_inverse(i: int, b: int) -> float:
    f, r = 1.0, 0.0
    while i > 0:
        f = f / b
        r = r + f * (i % b)
        i = i // b
    return r


def pattern(n: int) -> np.ndarray:
    """float32 [n, 2]: (0, 0) for n == 1, else (H2(k + 1) - 0.5, H3(k + 1) - 0.5) in python doubles, rounded to float32."""
    if n == 1:
        return np.zeros((1, 2), np.float32)
    return np.array([[radical_inverse(k + 1, 2) - 0.5, radical_inverse(k + 1, 3) - 0.5] for k in range(n)], np.float64).astype(np.float32)


def weights(filt: int, offsets: np.ndarray) -> np.ndarray:
    """float32 [n, 2r + 1, 2r + 1], weights[k, j + r, i + r] (i along x).  Box: r = 0, all ones.  Tent: r = 1,
    max(0, 1 - |i + dx_k|) * max(0, 1 - |j + dy_k|) in double from the float32 offsets, rounded to float32."""
    off = np.asarray(offsets, np.float32).reshape(-1, 2)
    n = off.shape[0]
    if filt == AA_BOX:
        return np.ones((n, 1, 1), np.float32)
    assert filt == AA_TENT
    out = np.empty((n, 3, 3), np.float32)
    for k in range(n):
        dx, dy = float(off[k, 0]), float(off[k, 1])   # float32 -> double, exact
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                out[k, j + 1, i + 1] = np.float32(max(0.0, 1.0 - abs(i + dx)) * max(0.0, 1.0 - abs(j + dy)))
    return out


def pack_u8(v: np.ndarray) -> np.ndarray:
    """The truncating pack of the march's composite: s = v * 255 (float32); 0 unless s > 0, 255 if s >= 255, else uint8(s)."""
    s = v.astype(np.float32) * np.float32(255.0)
    out = np.zeros(s.shape, np.uint8)
    mid = (s > 0) & (s < np.float32(255.0))
    out[mid] = s[mid].astype(np.uint8)
    out[s >= np.float32(255.0)] = 255
    return out


def resolve(sub: np.ndarray, w: np.ndarray, r: int):
    """sub float32 [n, h, w, 4], w float32 [n, 2r + 1, 2r + 1] -> (rgba float32 [h, w, 4], rgba8 uint8 [h, w, 4])."""
    sub = np.ascontiguousarray(sub, np.float32)
    w = np.asarray(w, np.float32).reshape(sub.shape[0], 2 * r + 1, 2 * r + 1)
    n, H, W, _ = sub.shape
    acc = np.zeros((H, W, 4), np.float32)
    wsum = np.zeros((H, W), np.float32)
    for k in range(n):
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                wt = w[k, j + r, i + r]
                if wt == 0:
                    continue
                # pixels (x, y) for which (x + i, y + j) is inside the frame
                ys, ye = max(0, -j), min(H, H - j)
                xs, xe = max(0, -i), min(W, W - i)
                if ys >= ye or xs >= xe:
                    continue
                term = wt * sub[k, ys + j:ye + j, xs + i:xe + i, :]          # float32 product, rounded
                acc[ys:ye, xs:xe, :] = acc[ys:ye, xs:xe, :] + term          # float32 sum, rounded
                wsum[ys:ye, xs:xe] = wsum[ys:ye, xs:xe] + wt
    out = np.zeros((H, W, 4), np.float32)
    pos = wsum > 0
    out[pos] = acc[pos] / wsum[pos][:, None]                                # float32 division, correctly rounded
    return out, pack_u8(out)

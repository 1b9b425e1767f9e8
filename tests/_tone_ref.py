"""numpy restatement of the tone perturbations (include/vipcup_hip.h: vip_tone_hist_u8, vip_tone_lut_u8, vip_tone_apply_rgb_u8), written
from the arithmetic stated there, in plain Python integers and float64: auto-contrast per channel and from the luma, equalisation, and
the project's integer CLAHE.  tests/test_tone_cpu.py holds the first three against Pillow bit for bit; tests/test_gpu_tone.py holds the
kernels against this file."""
import numpy as np

MODES = ("autocontrast", "autocontrast_luma", "equalize", "clahe")


def luma(a):
    """Pillow's convert("L") of uint8 ``[..., 3]``, as int64"""
    a = a.astype(np.int64)
    return (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16


def grid(h, w, G=8):
    return min(G, max(1, h // 16)), min(G, max(1, w // 16))


def bounds(side, g):
    return [(k * side) // g for k in range(g + 1)]


def hist256(v):
    return np.bincount(np.asarray(v).ravel().astype(np.int64), minlength=256).astype(np.int64)


def tile_histograms(a, G, channels):
    """``[gy * gx, channels, 256]``: per tile (row-major) the histograms of R, G, B (channels 3) or of the luma (1)"""
    h, w, _ = a.shape
    gy, gx = grid(h, w, G)
    by, bx = bounds(h, gy), bounds(w, gx)
    src = a.astype(np.int64) if channels == 3 else luma(a)[..., None]
    out = np.zeros((gy * gx, channels, 256), np.int64)
    for j in range(gy):
        for i in range(gx):
            t = src[by[j]:by[j + 1], bx[i]:bx[i + 1]]
            for c in range(channels):
                out[j * gx + i, c] = hist256(t[..., c])
    return out


def autocontrast_table_lo_hi(lo, hi):
    """Pillow's float expression for the levels lo < hi: one division, two products, one sum in float64, int() towards zero"""
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(max(int(i * scale + offset), 0), 255) for i in range(256)]


def autocontrast_tables_all_pairs():
    """``(pairs [32640, 2], tables uint8 [32640, 256])``: the table of every 0 <= lo < hi <= 255, in numpy float64 - elementwise
    products and sums, each rounded on its own, like the scalar expression (tests/test_tone_cpu.py holds the two against each other)"""
    lo, hi = np.triu_indices(256, 1)
    scale = 255.0 / (hi - lo).astype(np.float64)
    offset = (-lo).astype(np.float64) * scale
    x = np.arange(256, dtype=np.float64)[None, :] * scale[:, None] + offset[:, None]
    return np.stack([lo, hi], axis=1), np.clip(np.trunc(x), 0, 255).astype(np.uint8)


def autocontrast_table(h, cutoff):
    h = [int(v) for v in h]
    n = sum(h)
    cut = (n * int(cutoff)) // 100
    lo = hi = 0
    acc = 0
    for i in range(256):
        acc += h[i]
        if acc > cut:
            lo = i
            break
    acc = 0
    for i in range(255, -1, -1):
        acc += h[i]
        if acc > cut:
            hi = i
            break
    if n == 0 or hi <= lo:
        return list(range(256))
    return autocontrast_table_lo_hi(lo, hi)


def equalize_table(h):
    h = [int(v) for v in h]
    nz = [v for v in h if v]
    if len(nz) < 2:
        return list(range(256))
    step = (sum(h) - nz[-1]) // 255
    if step == 0:
        return list(range(256))
    out, acc = [], step // 2
    for i in range(256):
        out.append(min(acc // step, 255))
        acc += h[i]
    return out


def clahe_redistribute(h, tt):
    """the clipped and refilled histogram h'' of a tile histogram h (sum A > 0) at ten times the clip limit ``tt``"""
    h = [int(v) for v in h]
    A = sum(h)
    clip = max(1, (int(tt) * A) // 2560)
    hc = [min(v, clip) for v in h]
    E = A - sum(hc)
    q, rem = E // 256, E % 256
    return [hc[i] + q + int((i * rem) // 256 != ((i + 1) * rem) // 256) for i in range(256)]


def clahe_table(h, tt):
    A = sum(int(v) for v in h)
    if A == 0:
        return list(range(256))
    out, acc = [], 0
    for v in clahe_redistribute(h, tt):
        acc += v
        out.append((acc * 255 + A // 2) // A)
    return out


def table(h, mode, param):
    """the 256 entries of ``mode`` (a name of MODES) from one histogram"""
    if mode in ("autocontrast", "autocontrast_luma"):
        return autocontrast_table(h, param)
    if mode == "equalize":
        return equalize_table(h)
    return clahe_table(h, param)


def axis_neighbours(side, g):
    """per pixel of an axis: the two neighbouring tiles and the weight of the second in 1 / 256"""
    b = bounds(side, g)
    c2 = [b[k] + b[k + 1] for k in range(g)]
    k0, k1, wq = np.zeros(side, np.int64), np.zeros(side, np.int64), np.zeros(side, np.int64)
    for x in range(side):
        X2 = 2 * x + 1
        if X2 < c2[0]:
            continue
        if X2 >= c2[g - 1]:
            k0[x] = k1[x] = g - 1
            continue
        k = max(j for j in range(g - 1) if c2[j] <= X2)
        k0[x], k1[x], wq[x] = k, k + 1, ((X2 - c2[k]) << 8) // (c2[k + 1] - c2[k])
    return k0, k1, wq


def clahe(a, tt, G=8):
    h, w, _ = a.shape
    gy, gx = grid(h, w, G)
    hists = tile_histograms(a, G, 1)
    T = np.array([clahe_table(hists[t, 0], tt) for t in range(gy * gx)], np.int64).reshape(gy, gx, 256)
    Y = luma(a)
    ky0, ky1, wy = axis_neighbours(h, gy)
    kx0, kx1, wx = axis_neighbours(w, gx)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    t00, t01 = T[ky0[yy], kx0[xx], Y], T[ky0[yy], kx1[xx], Y]
    t10, t11 = T[ky1[yy], kx0[xx], Y], T[ky1[yy], kx1[xx], Y]
    WX, WY = wx[xx], wy[yy]
    V = ((256 - WY) * ((256 - WX) * t00 + WX * t01) + WY * ((256 - WX) * t10 + WX * t11) + 32768) >> 16
    return np.clip(a.astype(np.int64) + (V - Y)[..., None], 0, 255).astype(np.uint8)


def tone(a, mode, param=None, G=8):
    """uint8 ``[h, w, 3]`` -> the image under ``mode`` (a name of MODES); ``param``: the cutoff percent, None, or ten times the clip limit"""
    if mode == "clahe":
        return clahe(a, param, G)
    if mode == "autocontrast_luma":
        lut = np.array(autocontrast_table(hist256(luma(a)), param), np.uint8)
        return lut[a]
    out = np.empty_like(a)
    for c in range(3):
        out[..., c] = np.array(table(hist256(a[..., c]), mode, param), np.uint8)[a[..., c]]
    return out

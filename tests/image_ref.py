"""Plain numpy statements of the small image kernels (img_kernels.hip, the image helpers of pm_kernels.hip, point_colors_kernel of
fuse_kernels.hip): what the device and the CPU oracle are both held to.  Every statement is written from the published definition
the kernel's header comment cites -- OpenCV's resize.cpp (computeResizeAreaTab, ResizeAreaFast, interpolateCubic), cvtColor's 8-bit
fixed point, Sobel + convertScaleAbs + addWeighted, MVS::EstimatePointColors -- not from the oracle's C.  Sums are taken in float64,
so a resize comes with the magnitude sum its float32 rounding bound needs; the integer statements are exact.  No ctypes here."""
import numpy as np

F32 = np.float32


# ---- cv::resize on an f32 image (DepthData::ViewData::ScaleImage) ---------------------------------------

def resize_size(shape, scale):
    """dsize = cvRound(size * scale): the scale is a float, the product a double, ties go to even"""
    s = float(F32(scale))
    return int(np.rint(shape[0] * s)), int(np.rint(shape[1] * s))


def area_tab(ssize, dsize, scale):
    """computeResizeAreaTab for one axis: per destination index the list of (source index, float32 weight); scale = source pixels per
    destination pixel"""
    tab = []
    for d in range(dsize):
        fs1 = d * scale
        fs2 = fs1 + scale
        cell = min(scale, ssize - fs1)
        s1 = int(np.ceil(fs1))
        s2 = min(int(np.floor(fs2)), ssize - 1)
        s1 = min(s1, s2)
        e = []
        if s1 - fs1 > 1e-3:
            e.append((s1 - 1, F32((s1 - fs1) / cell)))
        for s in range(s1, s2):
            e.append((s, F32(1.0 / cell)))
        if fs2 - s2 > 1e-3:
            e.append((s2, F32(min(min(fs2 - s2, 1.0), cell) / cell)))
        tab.append(e)
    return tab


def _tab_matrix(tab, ssize):
    m = np.zeros((len(tab), ssize), np.float64)
    for d, e in enumerate(tab):
        for s, a in e:
            m[d, s] += float(a)
    return m


def resize_area(src, scale):
    """INTER_AREA, shrinking.  Returns (out64, mag64, taps, path): the float64 sum, the same sum over |src| (the weights are positive),
    the largest number of terms of any output pixel and "fast" (integer factor that fits: the block mean) or "general" (the tables)"""
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.ndim == 2
    sh, sw = src.shape
    dh, dw = resize_size(src.shape, scale)
    factor = 1.0 / float(F32(scale))
    s64 = src.astype(np.float64)
    f = int(factor)
    if float(f) == factor and f >= 1 and dw * f <= sw and dh * f <= sh:
        blocks = lambda a: a[:dh * f, :dw * f].reshape(dh, f, dw, f)   # noqa: E731
        return blocks(s64).sum((1, 3)) / (f * f), blocks(np.abs(s64)).sum((1, 3)) / (f * f), f * f, "fast"
    ty, tx = area_tab(sh, dh, factor), area_tab(sw, dw, factor)
    wy, wx = _tab_matrix(ty, sh), _tab_matrix(tx, sw)
    taps = max(len(e) for e in ty) * max(len(e) for e in tx)
    return wy @ s64 @ wx.T, wy @ np.abs(s64) @ wx.T, taps, "general"


def cubic_weights(t):
    """interpolateCubic with A = -0.75 on float32 fractions, every operation in float32"""
    t = np.asarray(t, F32)
    A, one = F32(-0.75), F32(1)
    w0 = ((A * (t + one) - F32(5) * A) * (t + one) + F32(8) * A) * (t + one) - F32(4) * A
    w1 = ((A + F32(2)) * t - (A + F32(3))) * t * t + one
    u = one - t
    w2 = ((A + F32(2)) * u - (A + F32(3))) * u * u + one
    w3 = one - w0 - w1 - w2
    w = np.stack([w0, w1, w2, w3], -1)
    assert w.dtype == np.float32
    return w


def _cubic_axis(ssize, dsize, scale):
    f = (((np.arange(dsize, dtype=np.float64) + 0.5) / scale) - 0.5).astype(F32)
    i = np.floor(f)
    w = cubic_weights(f - i)
    taps = np.clip(i.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, ssize - 1)
    return taps, w.astype(np.float64)


def resize_cubic(src, scale):
    """INTER_CUBIC, enlarging.  Returns (out64, mag64): the 16 products summed in float64, and the same over absolute values"""
    src = np.asarray(src)
    assert src.dtype == np.float32 and src.ndim == 2
    sh, sw = src.shape
    dh, dw = resize_size(src.shape, scale)
    s = float(F32(scale))
    ty, wy = _cubic_axis(sh, dh, s)
    tx, wx = _cubic_axis(sw, dw, s)
    g = src.astype(np.float64)[ty[:, :, None, None], tx[None, None, :, :]]         # (dh, 4, dw, 4)
    out = np.einsum("yj,yjxi,xi->yx", wy, g, wx)
    mag = np.einsum("yj,yjxi,xi->yx", np.abs(wy), np.abs(g), np.abs(wx))
    return out, mag


def resize_gray(src, scale):
    """what ScaleImage computes: (out64, mag64, T, path) with T the number of float32 roundings a plain left-to-right evaluation
    of the sum can make"""
    if float(F32(scale)) > 1.0:
        out, mag = resize_cubic(src, scale)
        return out, mag, 16, "cubic"
    return resize_area(src, scale)


def resize_bound(mag64, T):
    """the standard bound of a length-T float32 sum of products against its exact value, per pixel"""
    return (T + 2) * 2.0 ** -24 * mag64


# ---- 8-bit conversions and the gradient map (InitGraMap) ------------------------------------------------

def gray_to_u8(gray):
    """the f32 gray image times 255 in float32, rounded half to even, saturated"""
    g = np.asarray(gray, F32) * F32(255)
    assert g.dtype == np.float32
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def bgr_to_u8(bgr):
    """cv::cvtColor BGR2GRAY on 8 bits: fixed point with 14 fractional bits"""
    b = np.asarray(bgr).astype(np.int64)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def sobel_abs(g8):
    """(|gx|, |gy|) of the 3 x 3 Sobel operator with reflect-101 borders, unclamped"""
    p = np.pad(np.asarray(g8).astype(np.int64), 1, mode="reflect")
    h, w = p.shape[0] - 2, p.shape[1] - 2
    v = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]   # noqa: E731
    gx = (v(-1, 1) + 2 * v(0, 1) + v(1, 1)) - (v(-1, -1) + 2 * v(0, -1) + v(1, -1))
    gy = (v(1, -1) + 2 * v(1, 0) + v(1, 1)) - (v(-1, -1) + 2 * v(-1, 0) + v(-1, 1))
    return np.abs(gx), np.abs(gy)


def gradient_u8(g8):
    """convertScaleAbs of both Sobel responses (saturated at 255), then addWeighted(0.5, 0.5): half of their sum, ties to even"""
    ax, ay = sobel_abs(g8)
    s = np.minimum(ax, 255) + np.minimum(ay, 255)
    return ((s + ((s >> 1) & 1)) >> 1).astype(np.uint8)


def gradient_branches(g8):
    """what an 8-bit image reaches of gradient_kernel: pixels with a clamped response, with an odd sum rounded up / down"""
    ax, ay = sobel_abs(g8)
    s = np.minimum(ax, 255) + np.minimum(ay, 255)
    odd = (s & 1) == 1
    return dict(clamped=int(((ax > 255) | (ay > 255)).sum()), up=int((odd & ((s >> 1) & 1 == 1)).sum()), down=int((odd & ((s >> 1) & 1 == 0)).sum()))


# ---- MVS::EstimatePointColors ---------------------------------------------------------------------------

def projection_matrix(v):
    K, R, Cc = (np.asarray(v[k], np.float64) for k in ("K", "R", "C"))
    return K @ np.concatenate([R, (-(R @ Cc))[:, None]], 1)


def closest_view(views, X, ids):
    """the view of ids with the smallest Camera::PointDepth (float64) among those with a colour image, or -1.  A negative depth is
    smaller than any positive one: a view behind the point wins, as in the reference"""
    best, img = float(np.finfo(np.float32).max), -1
    for i in ids:
        if views[i].get("bgr") is None:
            continue
        P = projection_matrix(views[i])
        d = P[2, 0] * X[0] + P[2, 1] * X[1] + P[2, 2] * X[2] + P[2, 3]
        if best > d:
            best, img = d, int(i)
    return img


def project_f32(view, X):
    """the float32 image position of X (three float64 values) in view: the homogeneous point rounded to float32, then 1 / z and two
    products in float32"""
    P = projection_matrix(view)
    with np.errstate(all="ignore"):
        q = [F32(P[r, 0] * X[0] + P[r, 1] * X[1] + P[r, 2] * X[2] + P[r, 3]) for r in range(3)]
        iz = F32(1) / q[2]
        return q[0] * iz, q[1] * iz


def sample_u8(img, px, py):
    """TImage<Pixel8U>::sample: bilinear, every product and every sum truncated back to 8 bits"""
    lx, ly = int(px), int(py)
    x = F32(px) - F32(lx); x1 = F32(1) - x
    y = F32(py) - F32(ly); y1 = F32(1) - y
    u8 = lambda f: int(f) & 255   # noqa: E731  (the products lie in 0 .. 255: the cast truncates; a sum wraps)
    out = []
    for k in range(3):
        p00, p01, p10, p11 = (F32(img[ly + j, lx + i, k]) for j in (0, 1) for i in (0, 1))
        top = (u8(x1 * p00) + u8(x * p01)) & 255
        bot = (u8(x1 * p10) + u8(x * p11)) & 255
        out.append((u8(F32(top) * y1) + u8(F32(bot) * y)) & 255)
    return out


def point_colors(views, xyz, n_views, view_ids, detail=None):
    """per point the colour of its closest view at its float32 projection when that lies inside the image with a border of 1
    (inclusive), white otherwise.  views: list indexed by view id of dicts (K, R, C, bgr or None).  detail, a list, receives per point
    (view or -1, px, py, inside)"""
    xyz = np.asarray(xyz, F32)
    out = np.full((len(xyz), 3), 255, np.uint8)
    off = 0
    for i in range(len(xyz)):
        ids = [int(v) for v in view_ids[off:off + int(n_views[i])]]
        off += int(n_views[i])
        X = xyz[i].astype(np.float64)
        img = closest_view(views, X, ids)
        px = py = F32(np.nan)
        inside = False
        if img >= 0:
            bgr = np.asarray(views[img]["bgr"])
            h, w = bgr.shape[:2]
            px, py = project_f32(views[img], X)
            inside = bool(px >= F32(1) and py >= F32(1) and px <= F32(w - 2) and py <= F32(h - 2))
            if inside:
                out[i] = sample_u8(bgr, px, py)
        if detail is not None:
            detail.append((img, px, py, inside))
    return out

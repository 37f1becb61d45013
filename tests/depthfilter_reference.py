"""NumPy restatement of the depth-refinement contract in include/uzl_mi355x.h ("Depth refinement and 3-D keypoint lifting"), written
from the contract alone: every f32 / f64 cast explicit, whole-image array operations in the contract's tap order (NumPy rounds
every elementwise operation on its own, so nothing is fused).  `refine` mirrors uzl_depthfilter_refine for one image and `lift`
uzl_depthfilter_lift; the other functions are the contract's steps."""
import math

import numpy as np

import laserline_reference as LR

DEFAULTS = dict(radius=3, nearest_radius=2, sigma_space=3.0, sigma_color=5.0, depth_scale=1.0, use_bilateral_filter=1)
F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(F32).max


def depth_values(depth, depth_scale=1.0):
    """step 1 -> float32 (the laser line's step 2)"""
    return LR.depth_values(depth, depth_scale)[0]


def tables(radius, sigma_space, sigma_color):
    """step 2 -> (cw[0..255], sw[-R..R]) float32, the host's libm (math, not np)"""
    ss = 1.0 if sigma_space <= 0 else float(sigma_space)
    sc = 1.0 if sigma_color <= 0 else float(sigma_color)
    cc, cs = -0.5 / (sc * sc), -0.5 / (ss * ss)
    cw = np.array([F32(math.exp(float(i * i) * cc)) for i in range(256)], F32)
    sw = np.array([F32(math.exp(float(abs(k)) * float(abs(k)) * cs)) for k in range(-radius, radius + 1)], F32)
    return cw, sw


def joint_pass(src, guide, cw, sw, radius, axis):
    """steps 3 (axis = 1: over columns) and 4 (axis = 0: over rows): src float32, guide integer, both (h, w) -> float32"""
    assert src.dtype == F32 and cw.dtype == F32 and sw.dtype == F32
    g = guide.astype(np.int64)
    n = src.shape[axis]
    t, ws = np.zeros(src.shape, F32), np.zeros(src.shape, F32)
    with np.errstate(all="ignore"):
        for k in range(-radius, radius + 1):
            at = np.clip(np.arange(n) + k, 0, n - 1)                      # BORDER_REPLICATE
            w = sw[k + radius] * cw[np.abs(np.take(g, at, axis) - g)]
            t = t + w * np.take(src, at, axis)
            ws = ws + w
        w = F32(0.0) * cw[0]                                              # the reference's one tap too many, at the centre
        t = t + w * src
        ws = ws + w
        out = t / ws
    assert out.dtype == F32
    return out


def reflect101(p, n):
    """BORDER_REFLECT_101 in closed form: the index has period 2 n - 2 and is mirrored in its second half"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q < n, q, 2 * n - 2 - q)


def disc(nearest_radius):
    """step 5's taps in order"""
    P = nearest_radius
    return [(i, j) for i in range(-P, P + 1) for j in range(-P, P + 1) if math.sqrt(float(i * i + j * j)) <= P]


def snap(filtered, before, nearest_radius):
    """step 5"""
    h, w = before.shape
    minv, out = np.full((h, w), FLT_MAX, F32), np.zeros((h, w), F32)
    with np.errstate(all="ignore"):
        for i, j in disc(nearest_radius):
            b = before[reflect101(np.arange(h) + i, h)[:, None], reflect101(np.arange(w) + j, w)[None, :]]
            a = np.abs(b - filtered)
            win = a < minv
            minv, out = np.where(win, a, minv), np.where(win, b, out)
    assert out.dtype == F32
    return out


def stages(depth, guide, **cfg):
    """-> dict of the step-1 image, the horizontal pass, the vertical pass and the snapped image"""
    cfg = dict(DEFAULTS, **cfg)
    d = depth_values(depth, cfg["depth_scale"])
    guide = np.asarray(guide)
    assert guide.dtype == np.uint8 and guide.shape == d.shape
    cw, sw = tables(cfg["radius"], cfg["sigma_space"], cfg["sigma_color"])
    hor = joint_pass(d, guide, cw, sw, cfg["radius"], 1)
    ver = joint_pass(hor, guide, cw, sw, cfg["radius"], 0)
    return dict(depth=d, horizontal=hor, vertical=ver, snapped=snap(ver, d, cfg["nearest_radius"]))


def refine(depth, guide=None, **cfg):
    """uzl_depthfilter_refine for one image -> float32 (height, width)"""
    cfg = dict(DEFAULTS, **cfg)
    depth = np.asarray(depth)
    if depth.size == 0:
        return np.zeros(depth.shape, F32)
    if not cfg["use_bilateral_filter"]:
        return depth_values(depth, cfg["depth_scale"])                    # step 6
    return stages(depth, guide, **cfg)["snapped"]


def lift(image, u, v, fx, fy, cx, cy, max_depth=0.0):
    """step 7 -> (pos float64 (3, n), valid uint8 (n))"""
    image = np.asarray(image)
    assert image.dtype == F32
    h, w = image.shape
    u = np.clip(np.asarray(u, np.int64).reshape(-1), 0, w - 1)
    v = np.clip(np.asarray(v, np.int64).reshape(-1), 0, h - 1)
    d = image[v, u].astype(F64)
    with np.errstate(all="ignore"):
        valid = (d != 0) & ~np.isnan(d) & ((max_depth == 0.0) | (d <= float(max_depth)))
        x = ((u.astype(F64) - float(cx)) * d) / float(fx)
        y = ((v.astype(F64) - float(cy)) * d) / float(fy)
    pos = np.zeros((3, len(u)), F64)
    pos[2] = -1.0
    pos[0, valid], pos[1, valid], pos[2, valid] = x[valid], y[valid], d[valid]
    return pos, valid.astype(np.uint8)

"""Deterministic edge scenes for the parity tests: the branches of the per-gaussian and binning kernels that the benchmark
scene (scene.make_gaussians: centres at most 5 % past the image edge, depths in [2, 12], splats of ~1.5 px) barely or
never reaches, but a training view takes all the time.

make_edge_scene starts from make_gaussians and overwrites disjoint row ranges, one per population:

  clamp_x, clamp_y, clamp_corner  centres with |x/z| or |y/z| (or both) past 1.3 tan(fov) but inside the cull padding,
                                  left / right / top / bottom, some large enough to reach into the image, some not
  clamp_boundary                  x/z or y/z within a few ulp of +-1.3 tan(fov), on either side, at the forward's limit
                                  (W / 2 fx) and at the backward's (tan(atan(.)) rounded as the library's host does)
  near                            z in [0.3, 0.45], large splats (large J), over many tiles
  near_edge                       z exactly near_thresh (kept) and the float just below it (culled)
  tiny                            scales 1e-5 .. 1e-4: lambda2 < 0, a NaN minor radius (SURVEY 8a hazard 2)
  needle, flat                    one scale 100 - 1000x the others (or one 1/100 - 1/1000 of them), at rotations that
                                  include 45 degrees: the coarse rectangle truncates the OBB (hazard 1)
  quat_small, quat_large          unnormalised quaternions, norms ~1e-3 and ~1e3
  saturated                       opacity logits 6 .. 20 (the alpha clamp at 0.99; sigmoid rounds to 1 in float)
  gate                            peak alpha within a few percent of 1/255
  vanishing                       logits -30 .. -12: on the lists, never above the gate
  culled                          every fourth row of `base` moved behind the camera: culled rows interleave with the
                                  rest, M < N
  base                            the benchmark scene's rows

The camera is view 0 (the identity pose) so that a camera-space coordinate IS the parameter: the boundary rows sit at
exact float ratios.  Every value is a pure function of (seed, size), generated with scene.uniform24.
"""
import ctypes
import ctypes.util
import math

import numpy as np

from conftest import pkg

NEAR = 0.3
FRACTIONS = dict(clamp_x=0.032, clamp_y=0.024, clamp_corner=0.024, near=0.06, tiny=0.06, needle=0.04, flat=0.03,
                 quat_small=0.02, quat_large=0.02, saturated=0.05, gate=0.04, vanishing=0.03)
SIZES = {"small": (5000, 256, 144, 3), "large": (16000, 640, 360, 1)}
# the near population of the larger scene: more of them, over the middle of the image, fainter -- tile lists beyond
# the 1488 entries from which the backward (and, two forwards later, the forward) splits lists into segments
NEAR_SHAPE = {"small": dict(fraction=0.06, sigma_px=(2.0, 40.0), spread=1.2, opacity=(-4.0, 0.0)),
              "large": dict(fraction=0.16, sigma_px=(15.0, 120.0), spread=0.7, opacity=(-6.5, -4.0))}


def _u(seed, stream, n):
    return pkg("scene").uniform24(seed, stream, n)


def forward_tan_fov(cam):
    """tan(fov / 2) of the forward (cuda/raster.cu:92-93): W / (2 fx) in float."""
    f = np.float32
    return f(cam["width"]) / (f(2.0) * f(cam["fx"])), f(cam["height"]) / (f(2.0) * f(cam["fy"]))


def backward_tan_fov(cam):
    """tan(fov / 2) as the library's backward computes it on the host (cuda/trainer.cu:992-995): the field of view in
    double, rounded to float, tanf of half of it."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.tanf.restype, libm.tanf.argtypes = ctypes.c_float, [ctypes.c_float]
    out = []
    for n, f in ((cam["width"], cam["fx"]), (cam["height"], cam["fy"])):
        fov = np.float32(2.0 * math.atan(float(n) / (2.0 * float(np.float32(f)))))
        out.append(np.float32(libm.tanf(float(fov * np.float32(0.5)))))
    return tuple(out)


def _ratio_rows(limit, z, backward, reach=3):
    """Coordinates c (float32) whose ratio c / z (forward) or c * (1 / (z + 1e-6)) (backward, H1) lies within a few ulp
    of `limit`: the floats around the one nearest limit * z; both sides of the limit are included."""
    f = np.float32
    z = f(z)
    zi = f(1.0) / (z + f(1e-6))
    ratio = (lambda c: f(c) * zi) if backward else (lambda c: f(c) / z)
    c = f(limit / zi) if backward else f(limit * z)
    out = [c]
    for direction in (np.inf, -np.inf):
        x = c
        for _ in range(reach):
            x = np.nextafter(x, f(direction))
            out.append(x)
    r = np.array([ratio(x) for x in out])
    assert (r < limit).any() and (r > limit).any(), (limit, z)
    return sorted(out)


def make_edge_scene(size="small", seed=None):
    """(params, camera, populations): populations maps a name to the sorted global row indices of that population."""
    scene = pkg("scene")
    seed = scene.SEED + 101 if seed is None else seed
    N, W, H, L = SIZES[size]
    params = scene.make_gaussians(N, W, H, L, seed)
    cam = scene.make_camera(W, H, 0)
    fx, fy = float(cam["fx"]), float(cam["fy"])
    xyz, scale, quat, opa = params["xyz"], params["scale"], params["quaternion"], params["opacity"]
    near_shape = NEAR_SHAPE[size]
    pops, start = {}, 0
    for name, frac in dict(FRACTIONS, near=near_shape["fraction"]).items():
        n = int(round(frac * N))
        pops[name] = np.arange(start, start + n)
        start += n
    s_ = 200  # stream offset for this module's draws

    def place(rows, u, v, z):
        xyz[rows, 0] = (u - W / 2.0) * z / fx
        xyz[rows, 1] = (v - H / 2.0) * z / fy
        xyz[rows, 2] = z

    def px_scale(rows, sigma_px, z, stream):
        """log-scales whose projected sigma is sigma_px pixels at depth z, jittered per axis by up to 30 %."""
        j = 0.7 + 0.6 * _u(seed, stream, 3 * len(rows)).reshape(-1, 3)
        scale[rows] = np.log(sigma_px[:, None] * z[:, None] / fx * j)

    # ---- clamp band: u in [-98, -40] or [296, 354] at 256 px (scaled with W), v likewise; sizes 1 .. 60 px
    limx_px, limy_px = 1.3 * W / 2.0, 1.3 * H / 2.0
    def band(n, lim_px, half, stream):
        t = _u(seed, stream, n)
        side = np.where(_u(seed, stream + 1, n) < 0.5, -1.0, 1.0)
        off = lim_px + 2.0 + t * (half + 98.0 - lim_px - 2.0)  # from 2 px past the clamp limit to 2 px inside the padding
        return half + side * off
    for name, stream in (("clamp_x", 0), ("clamp_y", 10), ("clamp_corner", 20)):
        rows = pops[name]
        n = len(rows)
        z = 2.0 + 10.0 * _u(seed, s_ + stream + 2, n)
        u = band(n, limx_px, W / 2.0, s_ + stream + 3) if name != "clamp_y" else W * _u(seed, s_ + stream + 4, n)
        v = band(n, limy_px, H / 2.0, s_ + stream + 5) if name != "clamp_x" else H * _u(seed, s_ + stream + 6, n)
        place(rows, u, v, z)
        px_scale(rows, np.exp(np.log(1.0) + np.log(60.0) * _u(seed, s_ + stream + 7, n)), z, s_ + stream + 8)

    # ---- clamp boundary: both axes, both signs, at the forward's and the backward's limit, a few ulp either side
    tfx, tfy = forward_tan_fov(cam)
    bfx, bfy = backward_tan_fov(cam)
    rows_b = []
    for axis, (tf, tb) in enumerate(((tfx, bfx), (tfy, bfy))):
        for backward, t in ((False, tf), (True, tb)):
            lim = np.float32(1.3) * t
            for sign in (1.0, -1.0):
                for z in (2.5, 4.0, 7.0):
                    for c in _ratio_rows(lim, z, backward):
                        rows_b.append((axis, np.float32(sign) * c, z))
    nb = len(rows_b)
    pops["clamp_boundary"] = np.arange(start, start + nb)
    start += nb
    for r, (axis, c, z) in zip(pops["clamp_boundary"], rows_b):
        other = (0.3 * (W if axis else H)) * (1 if r % 2 else -1) * z / (fy if axis else fx)  # inside along the other axis
        xyz[r, axis], xyz[r, 1 - axis], xyz[r, 2] = c, np.float32(other), np.float32(z)
    zb = xyz[pops["clamp_boundary"], 2].astype(np.float64)
    px_scale(pops["clamp_boundary"], 10.0 + 20.0 * _u(seed, s_ + 30, nb), zb, s_ + 31)  # they reach into the image

    # ---- near plane: z in [0.3, 0.45], large splats; plus z == near_thresh and the float below it
    rows = pops["near"]
    n = len(rows)
    z = NEAR + 0.15 * _u(seed, s_ + 40, n)
    sp = near_shape["spread"]
    place(rows, W * (0.5 + sp * (_u(seed, s_ + 41, n) - 0.5)), H * (0.5 + sp * (_u(seed, s_ + 42, n) - 0.5)), z)
    lo, hi = near_shape["sigma_px"]
    px_scale(rows, lo * np.exp(np.log(hi / lo) * _u(seed, s_ + 43, n)), z, s_ + 44)
    lo, hi = near_shape["opacity"]
    opa[rows] = lo + (hi - lo) * _u(seed, s_ + 45, n)
    edge = [np.float32(NEAR), np.nextafter(np.float32(NEAR), np.float32(0.0))] * 4
    pops["near_edge"] = np.arange(start, start + len(edge))
    start += len(edge)
    for k, (r, z) in enumerate(zip(pops["near_edge"], edge)):
        xyz[r] = [np.float32((0.2 + 0.08 * k) * W - W / 2.0) * z / np.float32(fx), np.float32(0.1 * H) * z / np.float32(fy), z]
        scale[r] = np.log(np.float32(6.0) * z / np.float32(fx) * np.array([1.0, 1.6, 0.6]))
        opa[r] = 0.5
    assert start <= 0.6 * N, "the populations leave most of the benchmark rows as they are"

    # ---- tiny: 1e-5 .. 1e-4 world units (a few thousandths of a pixel)
    rows = pops["tiny"]
    scale[rows] = np.log(1e-5 * np.exp(np.log(10.0) * _u(seed, s_ + 50, 3 * len(rows)))).reshape(-1, 3)

    # ---- needle (one axis 100 - 1000x) and flat (one axis 1/100 - 1/1000), rotations with 45 degrees
    c45, s45 = math.cos(math.pi / 8), math.sin(math.pi / 8)  # half-angle: a 45 degree rotation
    turns = np.array([[c45, 0, 0, s45], [c45, 0, 0, -s45], [c45, s45, 0, 0], [c45, 0, s45, 0],
                      [0.5, 0.5, 0.5, 0.5], [1, 0, 0, 0]], np.float64)
    for name, stream, long_axis in (("needle", 60, True), ("flat", 70, False)):
        rows = pops[name]
        n = len(rows)
        z = xyz[rows, 2].astype(np.float64)
        # thin axes of 0.005 - 0.02 px: the long axes end at 0.5 - 20 px, so the screen covariance (which holds 0.3 px^2
        # on both axes) stays within a condition number of ~1e3 and float32 parity keeps its meaning
        base_px = 0.005 + 0.015 * _u(seed, s_ + stream, n)
        ratio = np.exp(np.log(100.0) + np.log(10.0) * _u(seed, s_ + stream + 1, n))
        ax = (np.arange(n) % 3)
        s = np.repeat((base_px * z / fx)[:, None], 3, 1)
        if long_axis:
            s[np.arange(n), ax] *= ratio
        else:
            s *= np.sqrt(ratio)[:, None]
            s[np.arange(n), ax] /= ratio
        scale[rows] = np.log(s)
        q = turns[np.arange(n) % len(turns)]
        rnd = np.arange(n) % 4 == 3  # a quarter at random orientations
        q[rnd] = quat[rows][rnd]
        quat[rows] = q
        opa[rows] = -3.0 + 3.0 * _u(seed, s_ + stream + 2, n)  # faint: the long splats do not hide the rest

    # ---- unnormalised quaternions
    for name, norm in (("quat_small", 1e-3), ("quat_large", 1e3)):
        rows = pops[name]
        q = quat[rows].astype(np.float64)
        quat[rows] = q / np.linalg.norm(q, axis=1, keepdims=True) * norm * (0.5 + _u(seed, s_ + 80, len(rows)))[:, None]

    # ---- opacity: saturated, at the 1/255 gate, vanishing
    rows = pops["saturated"]
    opa[rows] = 6.0 + 14.0 * _u(seed, s_ + 90, len(rows))
    opa[rows[::5]] = 20.0
    rows = pops["gate"]
    logit = math.log((1.0 / 255.0) / (1.0 - 1.0 / 255.0))
    opa[rows] = logit + 0.05 * (2.0 * _u(seed, s_ + 91, len(rows)) - 1.0)
    rows = pops["vanishing"]
    opa[rows] = -30.0 + 18.0 * _u(seed, s_ + 92, len(rows))

    # ---- the rest: the benchmark scene, every fourth row behind the camera
    pops["base"] = np.arange(start, N)
    pops["culled"] = pops["base"][::4]
    xyz[pops["culled"], 2] = -np.abs(xyz[pops["culled"], 2])
    pops["base"] = np.setdiff1d(pops["base"], pops["culled"])
    return params, cam, pops


def compact_populations(pops, mask):
    """The populations in the forward's compacted order (culled rows dropped)."""
    slot = np.cumsum(mask) - 1
    return {k: slot[v[mask[v]]] for k, v in pops.items()}

"""CPU checks of the normal map from rendered depth: the float64 reference (tests/normal_reference.py) against central
differences of its own forward, a tilted plane's known normal, ops.pixel_intrinsics against the oracle's projection, the
validity rule, and the drop-in boundary of the four new entry points (no compute calls: there is no GPU here)."""
import os
import re

import numpy as np
import pytest

import normal_reference as nr
from conftest import ROOT, pkg

NAMES = ("gsplat_depth_to_normal", "gsplat_depth_to_normal_backward", "gsplat_normal_prior_loss",
         "gsplat_normal_smoothness_loss")
INTR = (41.5, 39.25, 3.75, 2.5)  # (fx, fy, cx, cy): float32 values, off-centre


def synthetic(H, W, seed, inverse):
    """(depth, T) float32 with mixed validity and no borderline decision: A is >= 0.55 or 0.1 against alpha_min = 0.5."""
    rng = np.random.default_rng(seed)
    T = rng.uniform(0.0, 0.45, (H, W)).astype(np.float32)
    T[rng.uniform(size=(H, W)) < 0.08] = 0.9
    s = rng.uniform(0.08, 0.5, (H, W))
    return ((1.0 - T.astype(np.float64)) * s).astype(np.float32), T


def _central(f, v, idx):
    """Central difference of f at element idx of array v with delta = 1e-6 |value|."""
    lo, hi = v.copy(), v.copy()
    delta = 1e-6 * abs(v[idx])
    lo[idx], hi[idx] = v[idx] - delta, v[idx] + delta
    return (f(hi) - f(lo)) / (hi[idx] - lo[idx])


def _difference_rounding(loss, v, idx):
    """What the rounding of the two float64 loss values can add to _central's quotient: each is a sum of positive terms
    known to a few 2^-52 of itself (taken as 8: 2^-49), and their difference is divided by 2e-6 |value|."""
    return 2.0 * 2.0 ** -49 * abs(loss) / (2e-6 * abs(v[idx]))


@pytest.mark.parametrize("inverse", (0, 1))
def test_reference_backward_is_the_derivative_of_its_forward(inverse):
    H, W = 7, 9
    depth, T = synthetic(H, W, 5, inverse)
    depth, A = depth.astype(np.float64), 1.0 - T.astype(np.float64)
    G = np.random.default_rng(1).normal(size=(H, W, 3))
    valid = nr.tangents(depth, 1.0 - A, INTR, inverse)["valid"]
    assert valid.any() and not valid[1:-1, 1:-1].all()
    g_depth, g_alpha, a_depth, a_alpha = nr.depth_to_normal_backward(depth, 1.0 - A, INTR, inverse, G)
    loss_of_depth = lambda d: float((G * nr.depth_to_normal(d, 1.0 - A, INTR, inverse)).sum())
    loss_of_alpha = lambda a: float((G * nr.depth_to_normal(depth, 1.0 - a, INTR, inverse)).sum())
    worst = 0.0
    for y in range(H):
        for x in range(W):
            for got, absolute, f, v in ((g_depth, a_depth, loss_of_depth, depth), (g_alpha, a_alpha, loss_of_alpha, A)):
                fd = _central(f, v, (y, x))
                if absolute[y, x] == 0.0:
                    assert got[y, x] == 0.0 and fd == 0.0, (y, x)
                    continue
                assert abs(got[y, x]) <= absolute[y, x] * (1 + 1e-12)
                err = abs(got[y, x] - fd) / absolute[y, x]
                worst = max(worst, err)
                assert err <= 1e-6, (y, x, got[y, x], fd, absolute[y, x])
    print(f"inverse={inverse}: worst |analytic - central| / absolute = {worst:.2e}")
    # a pixel no valid normal reads: exactly 0
    read = np.zeros((H, W), bool)
    read[:, 1:] |= valid[:, :-1]; read[:, :-1] |= valid[:, 1:]; read[1:] |= valid[:-1]; read[:-1] |= valid[1:]
    assert (~read).any() and (g_depth[~read] == 0).all() and (g_alpha[~read] == 0).all()


def test_reference_loss_gradients_are_the_derivatives():
    H, W = 7, 9
    rng = np.random.default_rng(3)
    depth, T = synthetic(H, W, 5, 0)
    n = nr.depth_to_normal(depth, T, INTR, 0)
    assert nr.has_normal(n).any() and not nr.has_normal(n).all()
    prior = rng.normal(size=(H, W, 3)) * rng.uniform(0.5, 2.0, (H, W, 1))
    prior[rng.uniform(size=(H, W)) < 0.3] = 0.0
    image = rng.uniform(0, 1, (H, W, 3))
    cases = (("prior", lambda m: nr.normal_prior_loss(m, prior, 0.75)),
             ("smooth", lambda m: nr.normal_smoothness_loss(m, image, 1.5, 2.0)),
             ("smooth, no image", lambda m: nr.normal_smoothness_loss(m, None, 1.5)))
    for what, fn in cases:
        loss, grad, absolute = fn(n)
        assert loss > 0 and (np.abs(grad) <= absolute * (1 + 1e-12)).all()
        for idx in zip(*np.nonzero(n)):  # (a zero component stays zero: the marker is not a value)
            fd = _central(lambda m: fn(m)[0], n, idx)
            # (both losses are sums over the whole map: a small component's step is small against the sum's own rounding)
            assert abs(grad[idx] - fd) <= 1e-6 * absolute[idx] + _difference_rounding(loss, n, idx), (what, idx, grad[idx], fd)
        assert (grad[~nr.has_normal(n)] == 0).all(), what
    # pixels without a prior take no part
    assert (nr.normal_prior_loss(n, prior, 0.75)[1][(prior == 0).all(-1)] == 0).all()


@pytest.mark.parametrize("inverse", (0, 1))
def test_plane_known_answer(inverse):
    """z = d / (m . ray) through float32 depth = A z (or A / z) at 33x19: n = m within what the rounding of depth allows,
    2 u z / min(|tx|, |ty|) with u = 2^-24."""
    W, H = 33, 19
    intr = (30.0, 28.0, 15.5, 9.25)
    rx, ry = nr.rays(H, W, intr)
    ray = np.stack([np.broadcast_to(rx[None, :], (H, W)), np.broadcast_to(ry[:, None], (H, W)), np.ones((H, W))], -1)
    m = np.array([0.3, -0.2, -1.0])
    m /= np.linalg.norm(m)
    z = -3.0 / (ray @ m)
    assert (z > 0).all()
    T = np.random.default_rng(7).uniform(0.0, 0.4, (H, W)).astype(np.float32)
    A = 1.0 - T.astype(np.float64)
    depth = ((A / z) if inverse else (A * z)).astype(np.float32)
    t = nr.tangents(depth, T, intr, inverse)
    assert t["valid"][1:-1, 1:-1].all() and not t["valid"][0].any() and not t["valid"][:, 0].any()
    n = nr.depth_to_normal(depth, T, intr, inverse)[1:-1, 1:-1]
    shortest = min(np.linalg.norm(t["tx"][1:-1, 1:-1], axis=-1).min(), np.linalg.norm(t["ty"][1:-1, 1:-1], axis=-1).min())
    bar = 2.0 * 2.0 ** -24 * z.max() / shortest
    err = np.abs(n - m).max()
    print(f"inverse={inverse}: max |n - m| = {err:.2e}, bar {bar:.2e}")
    assert err <= bar
    # fronto-parallel, exactly representable: (0, 0, -1) exactly
    flat = nr.depth_to_normal(np.full((H, W), 0.5 if inverse else 2.0, np.float32), np.zeros((H, W), np.float32), intr, inverse)
    assert np.array_equal(flat[1:-1, 1:-1], np.broadcast_to(np.array([0.0, 0.0, -1.0]), (H - 2, W - 2, 3)))
    assert (flat[0] == 0).all() and (flat[-1] == 0).all() and (flat[:, 0] == 0).all() and (flat[:, -1] == 0).all()


def _colmap_camera():
    app = pkg("app")
    cam = dict(width=97, height=61, params=[88.5, 91.25, 48.5, 30.5])
    img = dict(qvec=[0.9238795325, 0.0, 0.3826834324, 0.0], tvec=[0.1, -0.2, 0.3], id=1, name="a.png")
    return app.camera_from_colmap(cam, img)


@pytest.mark.parametrize("which", ("scene", "colmap"))
def test_pixel_intrinsics_invert_the_projection(scene, orc, which):
    ops = pkg("ops")
    cam = scene.make_camera(160, 96, 2) if which == "scene" else _colmap_camera()
    W, H = int(cam["width"]), int(cam["height"])
    intr = ops.pixel_intrinsics(cam)
    assert all(isinstance(v, float) and v == float(np.float32(v)) for v in intr)
    ref = nr.pixel_intrinsics(cam)
    assert np.allclose(intr, ref, rtol=2.0 ** -23, atol=0)
    rx, ry = nr.rays(H, W, intr)
    z = np.random.default_rng(0).uniform(0.5, 20.0, (H, W))
    P = z[..., None] * np.stack([np.broadcast_to(rx[None, :], (H, W)), np.broadcast_to(ry[:, None], (H, W)), np.ones((H, W))], -1)
    uv = orc.project_to_screen(P.reshape(-1, 3), cam["proj"], W, H, np.float64).reshape(H, W, 2)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).astype(np.float64)
    # the projection divides by w + 1e-6, not by w (cuda/projection.cu): a point at depth z lands 1e-6 / z of its
    # distance from the principal point short of its pixel, whatever the intrinsics.  Taken out, a few float32 ulp remain.
    centre = np.array([intr[2], intr[3]])
    err = np.abs(uv - xy) - np.abs(xy - centre) * (1e-6 / z[..., None])
    ulp = float(np.spacing(np.float32(max(W, H))))
    print(f"{which}: max |project_to_screen(P(p)) - p| = {np.abs(uv - xy).max():.2e} px, "
          f"{err.max() / ulp:.2f} ulp of {max(W, H)} beyond the projection's own 1e-6")
    assert err.max() <= 4 * ulp


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("damage", ("hole", "zero depth", "negative depth", "nan depth", "nan T"))
def test_validity(inverse, damage):
    """A pixel that is not ok zeroes exactly the normals that read it: its own and its four neighbours'."""
    H, W = 7, 9
    rng = np.random.default_rng(11)
    T = rng.uniform(0.0, 0.45, (H, W)).astype(np.float32)
    depth = ((1.0 - T.astype(np.float64)) * rng.uniform(0.08, 0.5, (H, W))).astype(np.float32)
    clean = nr.depth_to_normal(depth, T, INTR, inverse)
    assert nr.has_normal(clean)[1:-1, 1:-1].all()
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert (clean[border] == 0).all()
    y, x = 3, 4
    if damage == "hole":
        T[y, x] = 0.9
    elif damage == "nan T":
        T[y, x] = np.nan
    else:
        depth[y, x] = dict([("zero depth", 0.0), ("negative depth", -0.25), ("nan depth", np.nan)])[damage]
    n = nr.depth_to_normal(depth, T, INTR, inverse)
    readers = np.zeros((H, W), bool)
    for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
        readers[y + dy, x + dx] = True
    assert (n[readers] == 0).all()
    assert np.array_equal(n[~readers], clean[~readers]) and np.isfinite(n).all()
    # ... and the backward sends nothing through them
    G = rng.normal(size=(H, W, 3))
    g_depth, g_alpha, _, _ = nr.depth_to_normal_backward(depth, T, INTR, inverse, G)
    assert np.isfinite(g_depth).all() and np.isfinite(g_alpha).all() and g_depth[y, x] == 0 and g_alpha[y, x] == 0


def test_small_maps_have_no_normal():
    for H, W in ((1, 1), (2, 2), (2, 5), (5, 2)):
        depth, T = np.full((H, W), 2.0, np.float32), np.zeros((H, W), np.float32)
        assert (nr.depth_to_normal(depth, T, INTR, 0) == 0).all()
        assert all((m == 0).all() for m in nr.depth_to_normal_backward(depth, T, INTR, 0, np.ones((H, W, 3))))
    one = nr.depth_to_normal(np.full((3, 3), 2.0, np.float32), np.zeros((3, 3), np.float32), INTR, 0)
    assert nr.has_normal(one).sum() == 1 and np.array_equal(one[1, 1], [0.0, 0.0, -1.0])


def _declarations():
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(gsplat_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_entry_points_are_declared_bound_and_exported():
    lib_mod = pkg("_lib")
    text, decl = _declarations()
    assert re.search(r"#define\s+GSPLAT_ABI_VERSION\s+9\b", text) and lib_mod.ABI_VERSION == 9
    for name in NAMES:
        assert name in decl, f"{name} is not declared in gsplat_hip.h"
        assert name in lib_mod.SIGNATURES, f"{name} is not bound in _lib.py"
        assert len(lib_mod.SIGNATURES[name][1]) == decl[name].count(",") + 1, name
    assert len(lib_mod.SIGNATURES["gsplat_depth_to_normal"][1]) == 12
    assert len(lib_mod.SIGNATURES["gsplat_depth_to_normal_backward"][1]) == 15
    assert len(lib_mod.SIGNATURES["gsplat_normal_prior_loss"][1]) == 9
    assert len(lib_mod.SIGNATURES["gsplat_normal_smoothness_loss"][1]) == 10
    lib_mod.build()
    lib = lib_mod.load()
    assert lib.gsplat_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
    assert "gs_normal.hip" in open(os.path.join(ROOT, "3dgs_amd", "csrc", "Makefile")).read()
    ops = pkg("ops")
    for fn in ("pixel_intrinsics", "depth_to_normal", "depth_to_normal_backward", "normal_prior_loss", "normal_smoothness_loss"):
        assert callable(getattr(ops, fn))


def test_python_refusals_need_no_gpu():
    """The argument checks raise ValueError before anything is launched (here: before anything could be)."""
    ops = pkg("ops")
    import torch
    m = torch.zeros(5, 4)  # not on the device
    with pytest.raises(ValueError):
        ops.depth_to_normal(dict(T=m, depth=m), INTR, 0)
    with pytest.raises(ValueError):
        ops.depth_to_normal(dict(T=m), INTR, 0)
    with pytest.raises(ValueError):
        ops.normal_prior_loss(torch.zeros(5, 4, 3), torch.zeros(5, 4, 3), 1.0, None)

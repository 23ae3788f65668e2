"""The bilateral grid without a GPU: tests/bilagrid_reference.py against torch's grid_sample with autograd in float64 and
against central differences, the identity grid, the refusals (which need no device) and the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

import bilagrid_reference as bgr
from conftest import ROOT, pkg

INVALID_ARG = -3
GRIDS = ((1, 1, 1), (2, 2, 2), (3, 5, 4), (16, 16, 8), (64, 64, 16))  # (Wg, Hg, L)
IMAGES = ((1, 1), (1, 67), (35, 67))                                  # (H, W)
ENTRY_POINTS = {"gsplat_bilagrid_slice": 9, "gsplat_bilagrid_slice_backward": 12, "gsplat_bilagrid_tv_loss": 9}


def _case(Wg, Hg, L, H, W, seed=0):
    rng = np.random.default_rng([seed, Wg, Hg, L, H, W])
    grid = (bgr.identity_grid(Wg, Hg, L) + rng.uniform(-0.5, 0.5, (12, L, Hg, Wg))).astype(np.float32)
    image = rng.uniform(-0.2, 1.3, (H, W, 3)).astype(np.float32)  # 8-13 % of the pixels clamp at either end
    grad_out = rng.uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)
    return grid, image, grad_out


def _torch_slice(torch, grid, image):
    """grid_sample(bilinear, align_corners, border) of the grid at (x, y, luma), then the 3x4 product; float64."""
    H, W, _ = image.shape
    g = image[..., 0] * 0.299 + image[..., 1] * 0.587 + image[..., 2] * 0.114
    xs = (torch.arange(W, dtype=torch.float64) + 0.5) / W
    ys = (torch.arange(H, dtype=torch.float64) + 0.5) / H
    gx, gy = xs[None, :].expand(H, W), ys[:, None].expand(H, W)
    coords = torch.stack([gx, gy, g.clamp(0.0, 1.0)], -1) * 2.0 - 1.0
    A = torch.nn.functional.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True,
                                        padding_mode="border")  # [1,12,1,H,W]
    A = A[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (A[..., :3] * image[:, :, None, :]).sum(-1) + A[..., 3]


@pytest.mark.parametrize("size", IMAGES)
@pytest.mark.parametrize("shape", GRIDS)
def test_reference_is_grid_sample_with_autograd(shape, size):
    import torch
    grid, image, grad_out = _case(*shape, *size)
    tg = torch.from_numpy(grid).double().requires_grad_(True)
    ti = torch.from_numpy(image).double().requires_grad_(True)
    out = _torch_slice(torch, tg, ti)
    out.backward(torch.from_numpy(grad_out).double())
    ref_out, out_abs = bgr.slice_image(grid, image)
    grad_image, gi_abs, grad_grid, gg_abs, mask = bgr.slice_backward(grid, image, grad_out)
    assert mask.mean() <= 1e-3
    np.testing.assert_allclose(ref_out, out.detach().numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(grad_grid, tg.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(grad_image[~mask], ti.grad.numpy()[~mask], rtol=0, atol=1e-12)
    # a condition sum bounds its value, and is zero only where the value is
    assert (np.abs(ref_out) <= out_abs * (1 + 1e-12)).all() and (np.abs(grad_grid) <= gg_abs * (1 + 1e-12) + 1e-300).all()
    assert (np.abs(grad_image) <= gi_abs * (1 + 1e-12) + 1e-300).all()
    if shape == (64, 64, 16) and size == (1, 1):
        assert (gg_abs == 0).mean() > 0.99  # a grid far finer than the image: almost every vertex sees no pixel


def test_guidance_part_is_zero_where_it_clamps_and_without_a_z_axis():
    grid, image, grad_out = _case(3, 5, 4, 35, 67)
    flat = bgr.identity_grid(3, 5, 1) + grid[:, :1] * 0.1
    r = image.astype(np.float64)
    g = 0.299 * r[..., 0] + 0.587 * r[..., 1] + 0.114 * r[..., 2]
    clamped = (g < 0) | (g > 1)
    assert 0.05 < clamped.mean() < 0.3
    for gr in (grid, flat):
        grad_image, gi_abs, *_ = bgr.slice_backward(gr, image, grad_out)
        # there, the gradient is the direct part alone: A[:, :3]^T G of the reference's own coefficients
        flatg, rr, _, corners = bgr._pixels(gr, image)
        A, _ = bgr._coefficients(flatg, corners)
        direct = (A.reshape(-1, 3, 4)[:, :, :3] * grad_out.reshape(-1, 3).astype(np.float64)[:, :, None]).sum(1)
        where = clamped.reshape(-1) if gr is grid else np.ones(g.size, bool)
        assert (grad_image.reshape(-1, 3)[where] == direct[where]).all()


@pytest.mark.parametrize("shape", GRIDS[:4] + ((1, 4, 1), (5, 1, 3)))
def test_tv_reference_against_central_differences(shape):
    Wg, Hg, L = shape
    rng = np.random.default_rng([1, Wg, Hg, L])
    grid = rng.uniform(-1, 1, (12, L, Hg, Wg))
    weight = 10.0
    loss, grad, grad_abs, loss_abs = bgr.tv_loss(grid, weight)
    assert loss_abs == loss and (np.abs(grad) <= grad_abs * (1 + 1e-12)).all()
    if shape == (1, 1, 1):
        assert loss == 0.0 and (grad == 0).all()
    # by hand, axis by axis
    by_hand = 0.0
    for axis in (1, 2, 3):
        if grid.shape[axis] > 1:
            d = np.diff(grid, axis=axis)
            by_hand += (d ** 2).mean()
    assert abs(loss - weight * by_hand) <= 1e-12 * max(loss, 1.0)
    h = 1e-5
    for idx in rng.integers(0, grid.size, 12):
        e = np.zeros(grid.size)
        e[idx] = h
        e = e.reshape(grid.shape)
        numeric = (bgr.tv_loss(grid + e, weight)[0] - bgr.tv_loss(grid - e, weight)[0]) / (2 * h)
        assert abs(numeric - grad.reshape(-1)[idx]) <= 1e-7 * max(1.0, grad_abs.reshape(-1)[idx])


@pytest.mark.parametrize("shape", GRIDS)
def test_identity_grid_gives_the_image_back(shape):
    _, image, grad_out = _case(*shape, 35, 67)
    ident = bgr.identity_grid(*shape)
    out, _ = bgr.slice_image(ident, image)
    assert out.astype(np.float32).tobytes() == image.tobytes()
    grad_image, *_ = bgr.slice_backward(ident, image, grad_out)
    assert grad_image.astype(np.float32).tobytes() == grad_out.tobytes()


def test_entry_points_are_declared_and_bound():
    lib_mod, ops, trainer_mod = pkg("_lib"), pkg("ops"), pkg("trainer")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    lib = lib_mod.load()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(lib_mod.SIGNATURES[name][1]) == nargs and callable(getattr(lib, name))
    assert lib_mod.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    for fn in ("bilagrid_slice", "bilagrid_slice_backward", "bilagrid_tv_loss"):
        assert callable(getattr(ops, fn))
    assert callable(trainer_mod.Trainer.render_corrected)
    cfg = trainer_mod.DEFAULT_CONFIG
    assert (cfg["bilagrid"], tuple(cfg["bilagrid_shape"]), cfg["bilagrid_lr"], cfg["bilagrid_tv_weight"],
            cfg["bilagrid_start"]) == (False, (16, 16, 8), 0.002, 10.0, 0)
    assert "gs_bilagrid.hip" in open(os.path.join(ROOT, "3dgs_amd", "csrc", "Makefile")).read()


def test_refusals_need_no_device():
    """The limits, a null required pointer, both gradient outputs null and an aliased grad_image are refused with
    GSPLAT_ERR_INVALID_ARG before any pointer is looked at (the non-null pointers here are host addresses that must never
    be dereferenced or asked about)."""
    lib = pkg("_lib").load()
    bufs = [(ctypes.c_float * 64)() for _ in range(5)]
    g, im, go, gi, gg = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    fwd = lambda grid, w, h, l, image, rows, cols, out: lib.gsplat_bilagrid_slice(grid, w, h, l, image, rows, cols, out, None)
    bwd = lambda grid, w, h, l, image, grad_out, rows, cols, grad_image, grad_grid: lib.gsplat_bilagrid_slice_backward(
        grid, w, h, l, image, grad_out, rows, cols, 0, grad_image, grad_grid, None)
    tv = lambda grid, w, h, l, grad, loss: lib.gsplat_bilagrid_tv_loss(grid, w, h, l, 1.0, 0, grad, loss, None)
    # 1. the limits
    for w, h, l in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65, 1, 1), (1, 65, 1), (1, 1, 17), (-1, 2, 2)):
        assert fwd(g, w, h, l, im, 1, 1, go) == INVALID_ARG
        assert bwd(g, w, h, l, im, go, 1, 1, gi, gg) == INVALID_ARG
        assert tv(g, w, h, l, gg, None) == INVALID_ARG
    for rows, cols in ((0, 1), (1, 0), (-2, 3)):
        assert fwd(g, 1, 1, 1, im, rows, cols, go) == INVALID_ARG
        assert bwd(g, 1, 1, 1, im, go, rows, cols, gi, gg) == INVALID_ARG
    # 2. a null required pointer
    assert fwd(None, 1, 1, 1, im, 1, 1, go) == fwd(g, 1, 1, 1, None, 1, 1, go) == fwd(g, 1, 1, 1, im, 1, 1, None) == INVALID_ARG
    assert bwd(None, 1, 1, 1, im, go, 1, 1, gi, gg) == bwd(g, 1, 1, 1, None, go, 1, 1, gi, gg) == INVALID_ARG
    assert bwd(g, 1, 1, 1, im, None, 1, 1, gi, gg) == INVALID_ARG
    assert tv(None, 1, 1, 1, gg, None) == INVALID_ARG
    # 3. both gradient outputs null
    assert bwd(g, 1, 1, 1, im, go, 1, 1, None, None) == INVALID_ARG
    assert tv(g, 1, 1, 1, None, None) == INVALID_ARG
    # 4. grad_image aliasing grad_out or image (the same pointer, or overlapping it)
    assert bwd(g, 1, 1, 1, im, go, 1, 1, go, gg) == INVALID_ARG
    assert bwd(g, 1, 1, 1, im, go, 1, 1, im, gg) == INVALID_ARG
    inside = ctypes.c_void_p(go.value + 8)
    assert bwd(g, 1, 1, 1, im, go, 2, 2, inside, gg) == INVALID_ARG

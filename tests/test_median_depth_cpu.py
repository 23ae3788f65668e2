"""CPU tests of the median depth: the numpy reference (tests/median_depth_reference.py) on the oracle's forward and on
known answers, the width of its band, the declared entry points, and the Python argument checks that need no device."""
import os
import re

import numpy as np
import pytest

import median_depth_reference as mdr
from conftest import PIXEL_L1_TOL, ROOT, pkg


def _oracle(orc, scene, name):
    if name == "partial":  # 70 x 45: partial tiles in both directions
        N, W, H, L = 300, 70, 45, 1
    else:
        N, W, H, L = scene.WORKLOADS[name][:4]
    c = scene.CONFIG
    params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
    return W, H, orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, L, threads=4)


@pytest.mark.parametrize("name", ["tiny", "small", "partial"])
def test_the_band_is_one_position_almost_everywhere(orc, scene, name):
    """The band [lo, hi] must not be able to hide a failure: at most 0.5 % of the pixels may have lo != hi.  And both
    outcomes occur at the median: pixels with a surface and pixels without."""
    assert mdr.EPS == PIXEL_L1_TOL
    W, H, ref = _oracle(orc, scene, name)
    T = np.asarray(ref["T"], np.float64).reshape(H, W)
    for threshold in (0.5, 0.1, 0.9):
        lo, hi = mdr.median_band(ref, W, H, threshold)
        wide = int((lo != hi).sum())
        print(f"{name}, threshold {threshold}: lo != hi on {wide} of {W * H} pixels; {int((hi >= 0).sum())} have a surface")
        assert wide <= 0.005 * W * H
        assert ((lo <= hi) | (hi < 0)).all() and ((lo >= 0) | (hi < 0)).all()
        assert (lo < np.asarray(ref["n"]).reshape(H, W)).all()
        # the forward's final T decides whether there is a surface, away from the band's edges
        assert (hi[T <= threshold * (1 - 2 * mdr.EPS)] >= 0).all() and (lo[T > threshold * (1 + 2 * mdr.EPS)] < 0).all()
        if threshold == 0.5:
            assert 0 < int((hi >= 0).sum()) < W * H
    a, b, c = (mdr.median_band(ref, W, H, t)[0] for t in (0.9, 0.5, 0.1))
    all3 = (a >= 0) & (b >= 0) & (c >= 0)
    assert all3.any() and (a[all3] <= b[all3]).all() and (b[all3] <= c[all3]).all()


def _forward(orc, uv, logit, conic, sorted_ids, ranges, W, H):
    uv, conic = np.asarray(uv, np.float32).reshape(-1, 2), np.asarray(conic, np.float32).reshape(-1, 3)
    logit = np.asarray(logit, np.float32)
    rgb = np.ones((len(logit), 3), np.float32)
    sorted_ids, ranges = np.asarray(sorted_ids, np.int32), np.asarray(ranges, np.int32)
    n, T, _ = orc.render_image(uv, logit, conic, rgb, 0.0, sorted_ids, ranges, W, H)
    return dict(uv=uv, opacity=logit, conic=conic, sorted=sorted_ids, ranges=ranges, n=n, T=T)


def test_three_stacked_gaussians_cross_the_threshold_where_the_product_says(orc):
    W = H = 32
    u, v, k, logit = 16.0, 16.0, 0.03, 0.0  # alpha 0.5 exp(-0.015 r^2)
    fwd = _forward(orc, [u, v] * 3, [logit] * 3, [k, 0.0, k] * 3, [0, 1, 2] * 4, [0, 3, 6, 9, 12], W, H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.minimum(0.99, 0.5 * np.exp(-0.5 * np.float64(np.float32(k)) * ((x - u) ** 2 + (y - v) ** 2)))
    a = np.where(a > np.float32(0.00392156862), a, 0.0)
    for threshold in (0.6, 0.3, 0.2):
        after = np.stack([(1 - a) ** (i + 1) for i in range(3)])
        want = np.where((after <= threshold).any(0), (after <= threshold).argmax(0), -1)
        want = np.where(a > 0, want, -1)
        lo, hi = mdr.median_band(fwd, W, H, threshold)
        near = (np.abs(after / threshold - 1.0) < 3 * mdr.EPS).any(0)
        assert np.array_equal(lo[~near], want[~near]) and np.array_equal(hi[~near], want[~near])
        assert not mdr.outside_band(want, lo, hi)[~near].any()
    assert mdr.median_band(fwd, W, H, 0.6)[0][16, 16] == 0 and mdr.median_band(fwd, W, H, 0.2)[0][16, 16] == 2
    assert mdr.median_band(fwd, W, H, 0.1)[1].max() == -1  # 0.125 is as far as three halves go


def test_outside_band_counts_minus_one_as_infinity():
    lo, hi = np.array([[2, 2, -1, 3]]), np.array([[3, -1, -1, 3]])
    assert mdr.outside_band(np.array([[2, 7, -1, 3]]), lo, hi).tolist() == [[False, False, False, False]]
    assert mdr.outside_band(np.array([[1, 1, 5, -1]]), lo, hi).tolist() == [[True, True, True, True]]
    assert mdr.outside_band(np.array([[-1, -1, 0, 4]]), lo, hi).tolist() == [[True, False, True, True]]
    assert mdr.tile_of_pixels(33, 17)[16, 32] == 3 + 2 and mdr.tile_of_pixels(33, 17)[15, 15] == 0


def test_abi_declares_the_entry_points():
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(gsplat_\w+)\s*\(([^;]*)\)\s*;", header)}
    for name in ("gsplat_context_median_depth", "gsplat_tsdf_integrate_surface"):
        assert name in decl, name
        args = re.sub(r"/\*.*?\*/", "", decl[name], flags=re.S)
        assert len(lib_mod.SIGNATURES[name][1]) == args.count(",") + 1, name
        assert callable(getattr(lib, name))
    assert len(lib_mod.SIGNATURES["gsplat_context_median_depth"][1]) == 6
    assert len(lib_mod.SIGNATURES["gsplat_tsdf_integrate_surface"][1]) == len(lib_mod.SIGNATURES["gsplat_tsdf_integrate"][1]) - 1
    assert lib_mod.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    # the library refuses what it can judge without a device
    assert lib.gsplat_context_median_depth(None, 1, 0.5, None, None, None) == -3


def test_python_argument_checks_need_no_device():
    import torch
    raster, ops, lib_mod = pkg("raster"), pkg("ops"), pkg("_lib")
    ctx = raster.RasterContext.__new__(raster.RasterContext)  # no device: the checks come before the library is called
    ctx._last = ctx._last_size = None
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ctx.median_depth(bad)
    with pytest.raises(lib_mod.GsplatError):
        ctx.median_depth(0.5)  # no forward yet
    ctx._last, ctx._last_size = (10, 10, 0), (4, 6)
    for kw in (dict(out=torch.zeros(4, 6)), dict(out=np.zeros((4, 6), np.float32)), dict(index=torch.zeros(4, 6, dtype=torch.int32)),
               dict(out=torch.zeros(4, 6, dtype=torch.float64)), dict(out=torch.zeros(6, 4))):
        with pytest.raises(ValueError):
            ctx.median_depth(0.5, **kw)
    vol = dict(tsdf=None, weight=None, color=None, origin=(0, 0, 0), voxel=1.0, dims=(2, 2, 2))
    with pytest.raises(ValueError, match="inverse must be False"):
        ops.tsdf_integrate(vol, None, None, None, None, surface=True, inverse=True)
    with pytest.raises(ValueError, match="only with surface=True"):
        ops.tsdf_integrate(vol, None, None, None, None)
    t = pkg("trainer").Trainer.__new__(pkg("trainer").Trainer)
    t.world = 1
    with pytest.raises(ValueError):
        t.extract_mesh(depth="mode")
    with pytest.raises(ValueError):
        t.extract_mesh(depth="median", median_threshold=1.0)
    with pytest.raises(ValueError):
        t.extract_mesh(keep_largest=-1)

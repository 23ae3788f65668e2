"""CPU tests of the feature maps: the declared entry points, and the numpy reference (tests/feature_reference.py) against
the oracle's own image and against its adjoint."""
import os
import re

import numpy as np
import pytest

import feature_reference as fr
from conftest import ROOT, pkg


def _oracle(orc, scene, name, view=0):
    N, W, H, L = scene.WORKLOADS[name][:4]
    c = scene.CONFIG
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, view)
    return W, H, orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, L, threads=4)


def test_abi_declares_both_entry_points_and_stays_at_9():
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gsplat_context_render_features", "gsplat_context_lift_features"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert len(lib.SIGNATURES[name][1]) == 6, name
    assert lib.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    raster = pkg("raster")
    assert callable(raster.RasterContext.render_features) and callable(raster.RasterContext.lift_features)
    trainer = pkg("trainer")
    assert callable(trainer.Trainer.render_features) and callable(trainer.Trainer.lift_maps)


def test_the_reference_map_of_the_colours_is_the_oracle_image(orc, scene):
    """The oracle's float32 image is the running sum of n(p) terms w c, all of them within (1 - T(p)) max|rgb| in total;
    each addition rounds by at most 2^-24 of the partial sum, and the weights themselves (alpha and T in float32 against
    float64 on the same float32 inputs) by a few 2^-24 relative each: n(p) 2^-23 (1 - T(p)) max|rgb| per pixel."""
    W, H, ref = _oracle(orc, scene, "tiny")
    got = fr.feature_maps(ref, W, H, features=ref["rgb"])["out"]
    n = np.asarray(ref["n"], np.float64).reshape(H, W)
    T = np.asarray(ref["T"], np.float64).reshape(H, W)
    bound = n * 2.0 ** -23 * (1.0 - T) * np.abs(ref["rgb"]).max()
    err = np.abs(got - np.asarray(ref["image"], np.float64).reshape(H, W, 3))
    worst = (err / np.maximum(bound, 1e-300)[:, :, None])[bound > 0].max()
    print(f"tiny: reference map of rgb against the oracle image: largest error {err.max():.2e}, worst error / bound {worst:.3f}")
    assert (err <= bound[:, :, None]).all()
    assert (err[bound == 0] == 0).all() and (got != 0).any()


@pytest.mark.parametrize("channels", [1, 5])
def test_the_reference_is_its_own_adjoint(orc, scene, channels):
    W, H, ref = _oracle(orc, scene, "tiny")
    M = len(ref["uv"])
    f = fr.seeded_rows(M, channels, 3).astype(np.float64)
    g = fr.seeded_rows(H * W, channels, 4).astype(np.float64).reshape(H, W, channels)
    r = fr.feature_maps(ref, W, H, features=f, fmap=g)
    lhs, rhs = (r["out"] * g).sum(), (f * r["lifted"]).sum()
    scale = (r["out_abs"] * np.abs(g)).sum()
    print(f"C = {channels}: <F f, g> = {lhs:.12e}, <f, Ft g> = {rhs:.12e}, scale {scale:.3e}")
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * min(abs(lhs), abs(rhs))
    # the condition sums bound their sums, and a gaussian no pixel composites lifts nothing
    assert (np.abs(r["out"]) <= r["out_abs"] * (1 + 1e-12)).all() and (np.abs(r["lifted"]) <= r["lifted_abs"] * (1 + 1e-12)).all()
    assert (r["lifted"][r["pixels"] == 0] == 0).all() and (r["pixels"] == 0).any() and (r["pixels"] > 0).any()


def test_global_order_keeps_the_fill_on_culled_rows():
    rows = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert fr.to_global(rows, [3, 0], 4, fill=7.0).tolist() == [[3, 4], [7, 7], [7, 7], [1, 2]]

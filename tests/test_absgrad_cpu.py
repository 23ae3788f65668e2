"""Absgrad mode without a GPU: the ABI carries the three entry points, and the numpy reference the GPU tests compare
against (tests/absgrad_reference.py) is itself checked against the float64 oracle -- its signed sums are the oracle's
grad_uv, its absolute sums are the sum over single-pixel calls of |grad_uv| -- and says what the mode is for: on a random
scene the absolute statistic is several times the signed one."""
import os
import re

import numpy as np
import pytest

import absgrad_reference
from conftest import ROOT, pkg

ENTRY_POINTS = ("gsplat_context_set_absgrad", "gsplat_context_absgrad_uv", "gsplat_pack_absgrad_norm")

# Both identities compare two float64 evaluations of the same expressions that differ only in the order of their sums
# (per pixel, then over up to 1024 pixels and a list of a few hundred entries): every term carries a few dozen
# roundings of 1.1e-16 and a sum of 1e3..1e4 terms of one sign keeps a relative error of at most terms x eps ~ 1e-12.
# The bar is that figure, relative to the largest entry (the signed identity measures 2e-15).
F64_BAR = 1e-12


def test_abi_declares_the_entry_points():
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
    assert lib.SIGNATURES["gsplat_context_set_absgrad"][1] == lib.SIGNATURES["gsplat_context_set_depth"][1]
    assert len(lib.SIGNATURES["gsplat_context_absgrad_uv"][1]) == 3
    assert len(lib.SIGNATURES["gsplat_pack_absgrad_norm"][1]) == 4
    assert lib.ABI_VERSION == 9 and re.search(r"#define\s+GSPLAT_ABI_VERSION\s+9\b", header)


def test_config_key_is_optional_and_off_by_default(tmp_path):
    trainer_src = open(os.path.join(ROOT, "3dgs_amd", "trainer.py")).read()
    assert re.search(r"\babsgrad=False\b", trainer_src)
    ds = pkg("dataset")
    f = tmp_path / "c.yaml"
    f.write_text("num_iters: 5\nabsgrad: true  # comment\n")
    assert ds.parseExtensions(f) == {"absgrad": True}
    f.write_text("num_iters: 5\n")
    assert ds.parseExtensions(f) == {}


def _forward(scene, orc, N, W, H, bg, saturate=0):
    params = scene.make_gaussians(N, W, H, 0)
    if saturate:
        # sigma(40) is exactly 1 in float64 too: the gaussians in front of the camera with the largest footprint
        order = np.argsort(-np.asarray(params["scale"]).sum(1))
        params["opacity"][order[:saturate]] = 40.0
    cam = scene.make_camera(W, H, 1)
    c = scene.CONFIG
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], bg, 0, dtype=np.float64, threads=8)
    return ref


def _oracle_uv(orc, ref, gi, W, H, bg):
    return orc.render_image_backward(ref["uv"], ref["opacity"], ref["conic"], ref["rgb"], bg, ref["sorted"], ref["ranges"],
                                     ref["n"], ref["T"], gi, W, H, np.float64, 1)[2]


@pytest.mark.parametrize("bg,saturate", [(0.0, 0), (0.5, 0), (0.5, 6)], ids=["bg0", "bg05", "saturated"])
def test_reference_is_the_sum_of_single_pixel_calls(scene, orc, bg, saturate):
    N, W, H = 200, 48, 32
    ref = _forward(scene, orc, N, W, H, bg, saturate)
    gi = np.asarray(scene.make_grad_image(W, H), np.float64)
    signed, absolute = absgrad_reference.absgrad_sums(ref, gi, W, H, bg, dtype=np.float64)
    full = np.asarray(_oracle_uv(orc, ref, gi, W, H, bg)).reshape(-1, 2)
    err_s = np.abs(signed - full).max() / np.abs(full).max()
    print(f"signed identity: {err_s:.2e} of the largest entry")
    assert err_s <= F64_BAR
    total = np.zeros_like(full)
    for p in range(W * H):
        one = np.zeros((H, W, 3))
        one[p // W, p % W] = gi[p // W, p % W]
        total += np.abs(np.asarray(_oracle_uv(orc, ref, one, W, H, bg)).reshape(-1, 2))
    err_a = np.abs(absolute - total).max() / total.max()
    print(f"absolute identity: {err_a:.2e} of the largest entry")
    assert err_a <= F64_BAR
    assert (absolute >= np.abs(signed) - F64_BAR * total.max()).all()
    if saturate:
        opaque = np.asarray(ref["opacity"]) == 40.0
        assert opaque.any(), "no saturated gaussian survived the cull"
        assert (absolute[opaque] == 0).all() and (total[opaque] == 0).all()
        assert (absolute[~opaque] > 0).any()


@pytest.mark.parametrize("N,W,H", [(1500, 96, 64), (200, 48, 32)])
def test_the_two_criteria_differ(scene, orc, N, W, H):
    """abs >= |signed| componentwise, and the median ratio of the norms is well above 1 (measured 5.6 and 6.0)."""
    ref = _forward(scene, orc, N, W, H, 0.0)
    gi = np.asarray(scene.make_grad_image(W, H), np.float64)
    signed, absolute = absgrad_reference.absgrad_sums(ref, gi, W, H, 0.0, dtype=np.float64)
    assert (absolute >= np.abs(signed) - F64_BAR * absolute.max()).all()
    ns, na = np.linalg.norm(signed, axis=1), np.linalg.norm(absolute, axis=1)
    seen = ns > 0
    ratio = float(np.median(na[seen] / ns[seen]))
    print(f"median absnorm / |grad_uv| = {ratio:.2f} over {int(seen.sum())} gaussians")
    assert ratio > 2.0

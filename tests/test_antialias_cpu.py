"""Anti-aliased mode without a GPU: the ABI and the configuration carry it, and the numpy reference the GPU tests compare
against (tests/antialias_reference.py) is checked against central differences of its own float64 forward and against the
rules of the definition (0 <= rho <= 1, rho == 0, 1 - o == 0).  All on `tiny` with splat_scale = 0.25."""
import os
import re

import numpy as np
import pytest

import antialias_reference as aa
from conftest import ROOT, pkg

ENTRY_POINTS = ("gsplat_context_set_antialiased", "gsplat_compute_conic_antialiased",
                "gsplat_compute_conic_antialiased_backward")


def test_abi_declares_the_entry_points():
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
    assert lib.SIGNATURES["gsplat_context_set_antialiased"][1] == lib.SIGNATURES["gsplat_context_set_depth"][1]
    # one more array than the plain operators, in front of N / the stream
    assert len(lib.SIGNATURES["gsplat_compute_conic_antialiased"][1]) == len(lib.SIGNATURES["gsplat_compute_conic"][1]) + 1
    assert len(lib.SIGNATURES["gsplat_compute_conic_antialiased_backward"][1]) == \
        len(lib.SIGNATURES["gsplat_compute_conic_backward"][1]) + 1
    assert lib.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1))


def test_config_key_is_optional_and_off_by_default(tmp_path):
    trainer_src = open(os.path.join(ROOT, "3dgs_amd", "trainer.py")).read()
    assert re.search(r"\bantialiased=False\b", trainer_src)
    ds = pkg("dataset")
    f = tmp_path / "c.yaml"
    f.write_text("num_iters: 5\nantialiased: true  # comment\n")
    assert ds.parseExtensions(f) == {"antialiased": True}
    f.write_text("num_iters: 5\nabsgrad: false\n")
    assert ds.parseExtensions(f) == {"absgrad": False}


@pytest.fixture(scope="module")
def tiny(scene, orc):
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    params = scene.make_gaussians(N, W, H, L, splat_scale=0.25)
    cam = scene.make_camera(W, H, 2)
    c = scene.CONFIG
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L)
    return dict(params=params, cam=cam, ref=ref, J=np.asarray(ref["J"], np.float64), S=np.asarray(ref["sigma"], np.float64))


def test_rho_is_a_fraction_and_far_from_one(tiny):
    rho = aa.compensation(tiny["J"], tiny["S"], tiny["cam"]["view"])
    assert rho.shape == (tiny["ref"]["num_culled"],)
    assert ((rho >= 0) & (rho <= 1)).all()
    print(f"tiny, splat_scale 0.25: median rho {np.median(rho):.3f}, min {rho.min():.3f}")
    assert np.median(rho) < 0.6  # sub-pixel splats: the mode matters here


def test_conic_route_agrees_within_its_cancellation(tiny):
    """rho from the stored float32 conic (inverse of the blurred covariance) against rho from J and Sigma: a = a' - 0.3
    keeps an absolute error of a few float32 roundings of a' (conic entries, their determinant and the inverse: ~8), so
    rho = sqrt(a c / ..) moves by about that over the smaller of a, c -- a bar of 8 eps32 (a' / a + c' / c) rho, no tighter:
    the reason the reference does not take this route."""
    view = tiny["cam"]["view"]
    rho = aa.compensation(tiny["J"], tiny["S"], view)
    via = aa.compensation_from_conic(tiny["ref"]["conic"])
    _, _, a, b, c = aa.covariance(tiny["J"], tiny["S"], view)
    eps = float(np.finfo(np.float32).eps)
    # along the minor axis of an elongated splat the relevant size is the smaller eigenvalue of the unblurred covariance
    lam = 0.5 * (a + c) - np.sqrt(0.25 * (a - c) ** 2 + b * b)
    bar = 8 * eps * ((lam + aa.BLUR) / lam) * 2 * rho
    print(f"conic route: largest relative difference {np.max(np.abs(via - rho) / rho):.2e}")
    assert (np.abs(via - rho) <= bar).all()


def _central(f, x, col, h):
    xp, xm = x.copy(), x.copy()
    xp[:, col] += h
    xm[:, col] -= h
    return (f(xp) - f(xm)) / (2 * h)


def test_compensation_backward_matches_central_differences(tiny):
    """Central differences of the reference's own float64 rho, one input column at a time (the gaussians are independent).
    Step 1e-6 of the column's scale: truncation ~ step^2 times the third derivative and rounding ~ 1e-16 / 1e-6 leave
    1e-9 .. 1e-8 of the column's largest derivative; the bar is 1e-6 of it."""
    view, J, S = tiny["cam"]["view"], tiny["J"], tiny["S"]
    w = np.random.default_rng(1).uniform(0.5, 1.5, len(J))  # dL/d rho
    dJ, dS = aa.compensation_backward(J, S, view, w)
    assert np.isfinite(dJ).all() and np.isfinite(dS).all() and np.abs(dJ).max() > 0 and np.abs(dS).max() > 0
    for k in range(6):
        hJ = 1e-6 * np.abs(J).mean()
        num = w * _central(lambda x: aa.compensation(x, S, view), J, k, hJ)
        assert np.abs(num - dJ[:, k]).max() <= 1e-6 * np.abs(dJ).max(), ("J", k)
        hS = 1e-6 * np.abs(S).mean()
        num = w * _central(lambda x: aa.compensation(J, x, view), S, k, hS)
        assert np.abs(num - dS[:, k]).max() <= 1e-6 * np.abs(dS).max(), ("sigma", k)


def test_split_of_the_effective_gradient_matches_central_differences(tiny):
    """dL/d logit and dL/d rho for L = logit(sigmoid(l) rho), i.e. g_eff = 1, against central differences (float64,
    step 1e-6: the same 1e-6 bar, relative to each value)."""
    logit = np.asarray(tiny["ref"]["opacity"], np.float64)
    rho = aa.compensation(tiny["J"], tiny["S"], tiny["cam"]["view"])

    def eff(l, r):
        o = aa.sigmoid(l) * r
        return np.log(o) - np.log1p(-o)

    d_l, d_r = aa.split_effective(np.ones_like(logit), logit, rho)
    h = 1e-6
    num_l = (eff(logit + h, rho) - eff(logit - h, rho)) / (2 * h)
    num_r = (eff(logit, rho * (1 + h)) - eff(logit, rho * (1 - h))) / (2 * h * rho)
    assert np.abs(num_l - d_l).max() <= 1e-6 * np.abs(d_l).max()
    assert (np.abs(num_r - d_r) <= 1e-6 * np.abs(d_r)).all()
    # and the effective logit the forward substitutes is that function in float32
    sub = aa.effective_logit(logit.astype(np.float32), rho)
    assert np.abs(sub - eff(logit, rho)).max() <= 2 * np.finfo(np.float32).eps * np.abs(sub).max()


def test_rho_zero_contributes_nothing_and_receives_no_gradient(scene, orc, tiny):
    """Every fifth gaussian flattened to Sigma == 0 (exp(-60)^2 underflows in float32): det0 == 0, rho == 0, its effective
    logit is -inf, the oracle composites nothing of it, and every gradient of it is an exact, finite zero."""
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    params = {k: v.copy() for k, v in tiny["params"].items()}
    params["scale"][::5] = -60.0
    cam, c = tiny["cam"], scene.CONFIG
    plain, ref = aa.forward(orc, params, cam, c, c["bg"], L)
    flat = (np.asarray(ref["sigma"]) == 0).all(1)
    assert flat.any() and (ref["rho"][flat] == 0).all() and (ref["rho"][~flat] > 0).all()
    assert np.isneginf(ref["opacity"][flat]).all()
    kept = np.flatnonzero(~flat)
    remap = np.full(len(flat), -1)
    remap[kept] = np.arange(len(kept))
    # the same image without them (their list entries removed)
    keep_entry = ~flat[ref["sorted"]]
    ranges = np.concatenate([[0], np.cumsum(keep_entry)])[np.asarray(ref["ranges"])].astype(np.int32)
    _, _, without = orc.render_image(ref["uv"][kept], ref["opacity"][kept], ref["conic"][kept], ref["rgb"][kept], c["bg"],
                                     remap[ref["sorted"][keep_entry]].astype(np.int32), ranges, W, H)
    assert np.array_equal(without, ref["image"])
    g = aa.backward(orc, ref, cam, scene.make_grad_image(W, H), c["bg"], L)
    for k in ("opacity", "rho", "J", "sigma", "xyz_c", "scale", "quaternion", "uv", "conic"):
        v = np.asarray(g[k]).reshape(len(flat), -1)
        assert np.isfinite(v).all(), k
        assert (v[flat] == 0).all(), k
    assert np.abs(g["rho"][~flat]).max() > 0


def test_saturated_effective_opacity_gets_no_gradient():
    """1 - o == 0 (sigma(40) == 1 in float64, rho == 1): k = 0, nothing is divided by zero."""
    d_l, d_r = aa.split_effective(np.array([1.0, 1.0]), np.array([40.0, 40.0]), np.array([1.0, 0.5]))
    assert d_l[0] == 0 and d_r[0] == 0
    assert np.isfinite(d_l).all() and np.isfinite(d_r).all() and d_r[1] == 4.0  # k = 1 / 0.5, k / rho

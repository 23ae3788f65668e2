"""CPU checks of the depth / opacity maps (gsplat_context_set_depth): the C ABI declares and binds the new entry points,
and the reference the GPU tests compare against (tests/depth_reference.py, composed from the oracle's operators) holds up
against central finite differences of L = sum G_D depth + sum G_A alpha in float64."""
import os
import re

import numpy as np

import depth_reference
from conftest import ROOT, pkg

NEW = ("gsplat_context_set_depth", "gsplat_context_depth_map", "gsplat_backward_render_depth", "gsplat_backward_pass_depth")


def test_header_declares_and_binding_binds_the_depth_entry_points():
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define GSPLAT_ABI_VERSION 9\b", text)
    lib_mod = pkg("_lib")
    assert lib_mod.ABI_VERSION == 9
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in lib_mod.SIGNATURES, name
    # the superset of gsplat_backward_render_split: its seven arguments with the two gradient maps after grad_image
    split = lib_mod.SIGNATURES["gsplat_backward_render_split"][1]
    depth = lib_mod.SIGNATURES["gsplat_backward_render_depth"][1]
    assert len(depth) == len(split) + 2 and depth[:2] == split[:2] and depth[4:] == split[2:]


def _scene(scene):
    N, W, H = 20, 48, 32
    params = scene.make_gaussians(N, W, H, 0)
    cam = scene.make_camera(W, H, 0)
    # spread the gaussians over distinct depths: a finite-difference step must not reorder the depth sort
    rng = np.random.default_rng(5)
    z = np.linspace(2.0, 6.0, N) + rng.uniform(-0.05, 0.05, N)
    u, v = rng.uniform(6, W - 6, N), rng.uniform(5, H - 5, N)
    params["xyz"][:, 0] = (u - W / 2) * z / cam["fx"]
    params["xyz"][:, 1] = (v - H / 2) * z / cam["fy"]
    params["xyz"][:, 2] = z
    params["scale"][:] = np.log(rng.uniform(0.05, 0.15, (N, 3)))
    params["opacity"][:] = rng.uniform(-1.5, 2.5, N)
    return {k: np.asarray(v, np.float64) for k, v in params.items()}, cam, W, H


def test_composed_reference_matches_finite_differences(scene, orc):
    """The reference's per-gaussian chain keeps the reference rasterizer's conventions (d/d uv carries the {W,H}/2 of its
    pixel mapping, the covariance backward its own approximations), so its xyz / scale / quaternion gradients are not
    central differences of its forward to begin with -- that chain is the oracle's, tested on its own.  What is new here
    is checked where it is exact: d/d opacity at the leaves, and d/d z, d/d conic and d/d uv at the compositing's
    inputs -- the composed pixel gradient (G_D, G_A) through render_image_backward, and dL/dz = its grad_rgb[:, 0]."""
    params, cam, W, H = _scene(scene)
    c = scene.CONFIG
    rng = np.random.default_rng(7)
    gd, ga = rng.uniform(-1, 1, (H, W)), rng.uniform(-1, 1, (H, W))
    f64 = np.float64

    def rasterize(p):
        return orc.rasterize(p, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, 0, f64)

    def loss_of(ref):
        d, a = depth_reference.depth_alpha(orc, ref, W, H, f64)
        return float((gd * d).sum() + (ga * a).sum())

    ref = rasterize(params)
    assert ref["num_culled"] == len(params["opacity"]), "every gaussian in view"
    d, a = depth_reference.depth_alpha(orc, ref, W, H, f64)
    assert np.allclose(a, 1.0 - ref["T"], rtol=0, atol=1e-14)
    assert (d > 0).mean() > 0.3 and a.max() > 0.5, "the scene must cover the image"
    g = depth_reference.backward_pass(orc, ref, cam, np.zeros((H, W, 3)), gd, ga, 0.0, 0, f64)

    def central(f, x, h):
        numeric = np.zeros(x.size)
        for i in range(x.size):
            lo, hi = x.copy(), x.copy()
            lo.reshape(-1)[i] -= h
            hi.reshape(-1)[i] += h
            numeric[i] = (f(hi) - f(lo)) / (2 * h)
        return numeric.reshape(x.shape)

    def close(analytic, numeric, what):
        analytic = np.asarray(analytic, f64).reshape(numeric.shape)
        assert np.linalg.norm(numeric) > 0, what
        err = np.linalg.norm(analytic - numeric) / np.linalg.norm(numeric)
        assert err < 1e-5, f"{what}: relative error {err:.2e} against central differences"

    # the leaves: opacity (logits) through the whole forward
    close(g["opacity"], central(lambda op: loss_of(rasterize(dict(params, opacity=op))), params["opacity"], 1e-6),
          "d L / d opacity")
    # the compositing's inputs, the lists held fixed
    def with_(key, value):
        return dict(ref, **{key: value})
    close(g["z"], central(lambda z: loss_of(with_("xyz_c", np.concatenate([ref["xyz_c"][:, :2], z[:, None]], 1))),
                          np.array(ref["xyz_c"][:, 2]), 1e-6), "d L / d z")
    close(g["conic"], central(lambda k: loss_of(with_("conic", k)), np.array(ref["conic"]), 1e-7), "d L / d conic")
    close(np.asarray(g["uv"]) / np.array([0.5 * W, 0.5 * H]),
          central(lambda uv: loss_of(with_("uv", uv)), np.array(ref["uv"]), 1e-6), "d L / d uv")

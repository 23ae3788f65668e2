"""CPU checks of depth mode's options (gsplat_context_set_depth_mode) and the two depth regularisers: the C ABI declares
and binds the new entry points; A Q - D^2 of the float64 oracle maps IS the pair sum sum_{j<i} w_i w_j (s_i - s_j)^2 walked
directly over the oracle's own lists; the reference the GPU tests compare against (tests/depth_moment_reference.py) holds
up against central finite differences of mean(A Q - D^2) in float64; and so do the numpy versions of the two losses."""
import os
import re

import numpy as np
import pytest

import depth_moment_reference as dmr
from conftest import ROOT, pkg

F64 = np.float64
NEW = ("gsplat_context_set_depth_mode", "gsplat_context_depth_moment_map", "gsplat_backward_render_depth2",
       "gsplat_backward_pass_depth2", "gsplat_distortion_loss", "gsplat_depth_prior_loss")


def test_header_declares_and_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"#define GSPLAT_ABI_VERSION 9\b", text), "new entry points only: no ABI bump"
    lib_mod = pkg("_lib")
    assert lib_mod.ABI_VERSION == 9
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in lib_mod.SIGNATURES, name
    # the supersets: grad_depth2 sits right after grad_alpha
    for old, new, at in (("gsplat_backward_render_depth", "gsplat_backward_render_depth2", 4),
                         ("gsplat_backward_pass_depth", "gsplat_backward_pass_depth2", 6)):
        a, b = lib_mod.SIGNATURES[old][1], lib_mod.SIGNATURES[new][1]
        assert len(b) == len(a) + 1 and b[:at] == a[:at] and b[at + 1:] == a[at:], new
    assert "distortion" in pkg("dataset").EXTENSION_KEYS


@pytest.fixture(scope="module")
def tiny64(scene, orc):
    """`tiny`, view 2, rasterized by the float64 oracle over background 0 (shared; nothing below changes it)."""
    N, W, H, L, _ = scene.WORKLOADS["tiny"]
    params = {k: np.asarray(v, F64) for k, v in scene.make_gaussians(N, W, H, L).items()}
    cam = scene.make_camera(W, H, 2)
    c = scene.CONFIG
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, L, F64)
    return dict(params=params, cam=cam, W=W, H=H, L=L, ref=ref)


def _pair_sum_walk(ref, s, W, H):
    """sum_{j<i} w_i w_j (s_i - s_j)^2 per pixel, and sum w s^2, walking the oracle's tile lists front to back in float64
    with the oracle's compositing rules (alpha = min(0.99, sigmoid(o) exp(min(0, power))), dropped at or below 1/255; the
    splat that takes T below 1e-4 is the pixel's last).  Returns (pairs [H,W], AQ [H,W])."""
    uv, conic = np.asarray(ref["uv"], F64), np.asarray(ref["conic"], F64)
    opa = 1.0 / (1.0 + np.exp(-np.asarray(ref["opacity"], F64)))
    srt, ranges = np.asarray(ref["sorted"]), np.asarray(ref["ranges"])
    ntx = (W + 15) // 16
    pairs, AQ = np.zeros((H, W)), np.zeros((H, W))
    for tile in range(len(ranges) - 1):
        tx, ty = tile % ntx, tile // ntx
        ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
        T = np.ones(xs.shape)
        done = np.zeros(xs.shape, bool)
        ws, ss = [], []
        for k in range(ranges[tile], ranges[tile + 1]):
            g = srt[k]
            dx, dy = uv[g, 0] - xs, uv[g, 1] - ys
            power = np.minimum(0.0, -0.5 * (conic[g, 0] * dx * dx + 2.0 * conic[g, 1] * dx * dy + conic[g, 2] * dy * dy))
            alpha = np.minimum(0.99, opa[g] * np.exp(power))
            alpha = np.where((alpha > 0.00392156862) & ~done, alpha, 0.0)
            w = alpha * T
            T = np.where(done, T, T * (1.0 - alpha))
            done |= T < 0.0001
            ws.append(w)
            ss.append(s[g])
        if not ws:
            continue
        w, sv = np.stack(ws), np.asarray(ss)
        acc = np.zeros(xs.shape)
        for i in range(1, len(sv)):
            acc += w[i] * (w[:i] * ((sv[i] - sv[:i]) ** 2)[:, None, None]).sum(0)
        pairs[ys, xs] = acc
        AQ[ys, xs] = w.sum(0) * (w * (sv * sv)[:, None, None]).sum(0)
    return pairs, AQ


@pytest.mark.parametrize("inverse", [False, True])
def test_moments_give_the_pair_sum(orc, tiny64, inverse):
    k = tiny64
    ref, W, H = k["ref"], k["W"], k["H"]
    D, A, Q = dmr.maps(orc, ref, W, H, inverse, F64)
    assert np.allclose(A, 1.0 - ref["T"], rtol=0, atol=1e-14)
    pairs, AQ = _pair_sum_walk(ref, dmr.s_values(ref, inverse, F64), W, H)
    np.testing.assert_allclose(A * Q, AQ, rtol=1e-12, atol=0)  # the walk composites what the oracle composites
    assert (pairs > 0).mean() > 0.3, "the scene must put several splats on a pixel"
    err = np.abs((A * Q - D * D) - pairs)
    assert (err <= 1e-9 * (A * Q)).all(), float((err / np.maximum(A * Q, 1e-300)).max())


def _fd(f, x, h):
    x = np.array(x, F64)
    g = np.zeros_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


@pytest.mark.parametrize("inverse", [False, True])
def test_reference_gradients_match_finite_differences(scene, orc, tiny64, inverse):
    """L = mean(A Q - D^2).  As in tests/test_depth_cpu.py, what is new is checked where the reference chain is exact: d/d
    opacity at the leaves (through the whole float64 forward), and d/dz, d/d conic, d/d uv at the compositing's inputs
    with the lists held fixed.  Bars: those of test_oracle_known_answers.py::test_render_backward_unclamped_matches_fd
    (h = 1e-7 inside one piece of the 1/255 floor; rtol 1e-4 with atol 1e-5 for colour -- here z -- and opacity, 1e-4 for
    conic and uv)."""
    k = tiny64
    params, cam, W, H, L, ref = k["params"], k["cam"], k["W"], k["H"], k["L"], k["ref"]
    c = scene.CONFIG

    def loss_of(r):
        D, A, Q = dmr.maps(orc, r, W, H, inverse, F64)
        return float((A * Q - D * D).mean())

    D, A, Q = dmr.maps(orc, ref, W, H, inverse, F64)
    _, gA, gD, gQ = dmr.distortion_loss(1.0 - A, D, Q, 1.0)
    g = dmr.backward_pass(orc, ref, cam, np.zeros((H, W, 3)), gD, gA, gQ, 0.0, L, inverse, F64)
    h = 1e-7

    def with_(key, value):
        return dict(ref, **{key: value})

    def rasterize(op):
        return orc.rasterize(dict(params, opacity=op), cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, L, F64)

    mask = np.asarray(ref["mask"], bool)
    fd_op = _fd(lambda op: loss_of(rasterize(op)), params["opacity"], h)
    assert np.abs(fd_op[~mask]).max(initial=0.0) == 0.0
    np.testing.assert_allclose(g["opacity"], fd_op[mask], rtol=1e-4, atol=1e-5)
    fd_z = _fd(lambda z: loss_of(with_("xyz_c", np.concatenate([ref["xyz_c"][:, :2], z[:, None]], 1))), ref["xyz_c"][:, 2], h)
    assert np.linalg.norm(fd_z) > 0
    np.testing.assert_allclose(g["z"], fd_z, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(g["conic"], _fd(lambda x: loss_of(with_("conic", x)), ref["conic"], h), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(np.asarray(g["uv"]) / [0.5 * W, 0.5 * H], _fd(lambda x: loss_of(with_("uv", x)), ref["uv"], h),
                               rtol=1e-4, atol=1e-4)


def test_numpy_losses_match_finite_differences():
    rng = np.random.default_rng(3)
    H, W = 5, 7
    T, D, Q = rng.uniform(0, 1, (H, W)), rng.uniform(0, 8, (H, W)), rng.uniform(0, 60, (H, W))
    T[0] = 1.0  # rows nothing covers
    loss, gA, gD, gQ = dmr.distortion_loss(T, D, Q, 0.37)
    assert np.isclose(loss, 0.37 * ((1 - T) * Q - D * D).mean(), rtol=1e-14)
    h = 1e-6
    np.testing.assert_allclose(gA, -_fd(lambda x: dmr.distortion_loss(x, D, Q, 0.37)[0], T, h), rtol=1e-7, atol=1e-9)  # A = 1 - T
    np.testing.assert_allclose(gD, _fd(lambda x: dmr.distortion_loss(T, x, Q, 0.37)[0], D, h), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gQ, _fd(lambda x: dmr.distortion_loss(T, D, x, 0.37)[0], Q, h), rtol=1e-7, atol=1e-9)
    depth, target = rng.uniform(0.1, 1, (H, W)), rng.uniform(0.1, 1, (H, W))
    target[1, :3] = 0.0
    target[2, 2] = -1.0          # no data
    depth[3, 3] = target[3, 3]   # sign(0) = 0
    loss, gd = dmr.depth_prior_loss(depth, target, 0.8)
    valid = target > 0
    assert np.isclose(loss, 0.8 * np.abs(depth - target)[valid].sum() / (H * W), rtol=1e-14)
    assert (gd[~valid] == 0).all() and gd[3, 3] == 0.0
    fd = _fd(lambda x: dmr.depth_prior_loss(x, target, 0.8)[0], depth, 1e-7)
    away = valid & (np.abs(depth - target) > 1e-6)
    np.testing.assert_allclose(gd[away], fd[away], rtol=1e-6, atol=1e-9)

"""gsplat_distortion_loss and gsplat_depth_prior_loss against their numpy float64 versions
(tests/depth_moment_reference.py) at 17x9, 33x31 and 256x144: on rendered maps (`tiny` 64x48 and `small` 256x144 in mode
(1,1)) and on synthetic maps with T = 1 rows and target <= 0 holes.  The kernels evaluate every pixel in double from the
float maps and round once, so a gradient is held to 1e-6 relative plus an absolute floor of 1e-12, the loss (a double sum)
to 1e-6 relative; accumulate=True is the sum of two calls."""
import numpy as np
import pytest

import depth_moment_reference as dmr
from conftest import pkg

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _synthetic(H, W, seed):
    rng = np.random.default_rng(seed)
    T = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    T[::4] = 1.0  # rows nothing covers: A = 0
    s = rng.uniform(0.08, 0.5, (H, W))
    A = 1.0 - T.astype(np.float64)
    D = (A * s).astype(np.float32)
    Q = (A * s * s * rng.uniform(1.0, 1.3, (H, W))).astype(np.float32)
    target = rng.uniform(0.05, 0.6, (H, W)).astype(np.float32)
    target[rng.uniform(size=(H, W)) < 0.3] = 0.0   # no data
    target[1, 1::3] = -1.0
    target[2, 2] = D[2, 2]                         # sign(0) = 0
    return T, D, Q, target


def _rendered(torch, scene, name):
    raster = pkg("raster")
    N, W, H, L = scene.WORKLOADS[name][:4]
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True, inverse=True, moment=True)
    fwd = ctx.rasterize_image(raster.device_params(scene.make_gaussians(N, W, H, L)),
                              raster.device_camera(scene.make_camera(W, H, 2)), scene.CONFIG, 0.0, L)
    T, D, Q = (_np(fwd[k]).copy() for k in ("T", "depth", "depth2"))
    rng = np.random.default_rng(9)
    target = (D * rng.uniform(0.8, 1.2, D.shape)).astype(np.float32)
    target[D == 0] = 0.0
    target[rng.uniform(size=D.shape) < 0.2] = 0.0
    return T, D, Q, target


@pytest.fixture(scope="module")
def cases(gpu, scene):
    out = {f"synthetic{W}x{H}": _synthetic(H, W, H) for W, H in ((17, 9), (33, 31), (256, 144))}
    out["tiny"], out["small"] = _rendered(gpu, scene, "tiny"), _rendered(gpu, scene, "small")
    return out


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert (err <= 1e-6 * np.abs(ref) + 1e-12).all(), f"{what}: {float(err.max()):.3e}"


NAMES = ("synthetic17x9", "synthetic33x31", "synthetic256x144", "tiny", "small")


@pytest.mark.parametrize("name", NAMES)
def test_distortion_loss(gpu, cases, name):
    torch, ops = gpu, pkg("ops")
    T, D, Q, _ = cases[name]
    fwd = dict(T=torch.as_tensor(T).cuda(), depth=torch.as_tensor(D).cuda(), depth2=torch.as_tensor(Q).cuda())
    weight = 37.5
    loss_ref, gA, gD, gQ = dmr.distortion_loss(T, D, Q, weight)
    maps = [torch.full_like(fwd["T"], float("nan")) for _ in range(3)]
    loss = ops.distortion_loss(fwd, weight, *maps, blocking=True)
    assert abs(loss - loss_ref) <= 1e-6 * abs(loss_ref), (loss, loss_ref)
    for got, ref, what in zip(maps, (gA, gD, gQ), ("grad_alpha", "grad_depth", "grad_depth2")):
        _close(_np(got), ref, what)
    # accumulate: the sum of two calls (one float addition on top: the first call's floats + the second's)
    first = [m.clone() for m in maps]
    assert ops.distortion_loss(fwd, 2.0 * weight, *maps, accumulate=True) is None
    for m, f, ref, what in zip(maps, first, dmr.distortion_loss(T, D, Q, 2.0 * weight)[1:], ("grad_alpha", "grad_depth", "grad_depth2")):
        want = _np(f) + ref.astype(np.float32)
        assert np.array_equal(_np(m), want), what
    # any map may be left out
    only = torch.full_like(fwd["T"], float("nan"))
    ops.distortion_loss(fwd, weight, None, only, None)
    assert torch.equal(only, first[1])


@pytest.mark.parametrize("name", NAMES)
def test_depth_prior_loss(gpu, cases, name):
    torch, ops = gpu, pkg("ops")
    _, D, _, target = cases[name]
    d, t = torch.as_tensor(D).cuda(), torch.as_tensor(target).cuda()
    weight = 0.75  # (a float32 value, like 3 x it: the accumulate check below is exact)
    loss_ref, g_ref = dmr.depth_prior_loss(D, target, weight)
    assert (target <= 0).any() and (target > 0).any()
    g = torch.full_like(d, float("nan"))
    loss = ops.depth_prior_loss(d, t, weight, g, blocking=True)
    assert abs(loss - loss_ref) <= 1e-6 * abs(loss_ref), (loss, loss_ref)
    _close(_np(g), g_ref, "grad_depth")
    assert bool((g[t <= 0] == 0).all())
    first = g.clone()
    ops.depth_prior_loss(d, t, 3.0 * weight, g, accumulate=True)
    assert np.array_equal(_np(g), _np(first) + dmr.depth_prior_loss(D, target, 3.0 * weight)[1].astype(np.float32))
    # the target equal to the depth: no gradient anywhere
    ops.depth_prior_loss(d, d.clone(), weight, g)
    assert bool((g == 0).all())


def test_bad_arguments_raise(gpu):
    torch, ops = gpu, pkg("ops")
    m = torch.zeros(9, 17, device="cuda")
    with pytest.raises(ValueError):
        ops.distortion_loss(dict(T=m, depth=m), 1.0, m, m, m)  # no second moment
    with pytest.raises(ValueError):
        ops.distortion_loss(dict(T=m, depth=m, depth2=torch.zeros(9, 16, device="cuda")), 1.0, m, m, m)
    with pytest.raises(ValueError):
        ops.depth_prior_loss(m, m.double(), 1.0, m)

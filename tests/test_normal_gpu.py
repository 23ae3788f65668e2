"""gsplat_depth_to_normal, gsplat_depth_to_normal_backward, gsplat_normal_prior_loss and gsplat_normal_smoothness_loss
against their numpy float64 versions (tests/normal_reference.py).

Sizes: 1x1 and 2x2 (no normal anywhere), 3x3 (one), 5x4, 17x9, 33x31, 67x35 (2 x 3 tiles of 64 x 16 with a remainder in
both directions: the halo comes from the neighbouring tiles) and the rendered `tiny` (64x48); both `inverse` values;
accumulate on and off; either gradient output absent.  The synthetic maps mix validity without a borderline decision: T
is uniform in [0, 0.45] with 8 % of the pixels at 0.9, so A is >= 0.55 or 0.1 against alpha_min = 0.5.

The kernels evaluate every pixel in double from the float maps and round once, so every element is held to
1e-6 x absolute + 1e-12 (absolute: the sum of the absolute values of the element's terms; 1 for a normal), a loss value to
1e-6 relative; pixels without a normal and pixels no normal reads are exactly 0; accumulate=True is, bit for bit, the first
call's floats plus the second call's; two runs of every kernel give the same bits."""
import numpy as np
import pytest

import normal_reference as nr
from conftest import pkg

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (2, 2), (3, 3), (5, 4), (17, 9), (33, 31), (67, 35))  # (W, H)
NAMES = tuple(f"synthetic{W}x{H}" for W, H in SIZES) + ("tiny",)
ALPHA_MIN = 0.5


def _np(t):
    return t.detach().cpu().numpy()


def _synthetic(H, W, seed):
    rng = np.random.default_rng(seed)
    T = rng.uniform(0.0, 0.45, (H, W)).astype(np.float32)
    if H * W > 9:
        T[rng.uniform(size=(H, W)) < 0.08] = 0.9  # holes: A = 0.1
    s = rng.uniform(0.08, 0.5, (H, W))
    depth = ((1.0 - T.astype(np.float64)) * s).astype(np.float32)
    # intrinsics of a 60-degree camera of that size, off-centre: float32 values
    intr = tuple(float(np.float32(v)) for v in (0.87 * W, 0.91 * W, 0.5 * W - 0.25, 0.5 * H + 0.5))
    return depth, T, intr


def _rendered(scene, inverse):
    raster, ops = pkg("raster"), pkg("ops")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True, inverse=bool(inverse))
    cam = scene.make_camera(W, H, 2)
    fwd = ctx.rasterize_image(raster.device_params(scene.make_gaussians(N, W, H, L)), raster.device_camera(cam),
                              scene.CONFIG, 0.0, L)
    return _np(fwd["depth"]).copy(), _np(fwd["T"]).copy(), ops.pixel_intrinsics(cam)


def _case(depth, T, intr, inverse, seed):
    """The inputs of every test of one (map, inverse) and their float64 answers, computed once."""
    H, W = T.shape
    rng = np.random.default_rng(seed)
    c = dict(depth=depth, T=T, intr=intr, inverse=inverse, H=H, W=W)
    c["normal"] = nr.depth_to_normal(depth, T, intr, inverse, ALPHA_MIN)
    c["valid"] = nr.has_normal(c["normal"])
    c["G"] = rng.normal(size=(H, W, 3)).astype(np.float32)
    c["backward"] = nr.depth_to_normal_backward(depth, T, intr, inverse, c["G"], ALPHA_MIN)
    read = np.zeros((H, W), bool)
    v = c["valid"]
    read[:, 1:] |= v[:, :-1]; read[:, :-1] |= v[:, 1:]; read[1:] |= v[:-1]; read[:-1] |= v[1:]
    c["read"] = read
    prior = (rng.normal(size=(H, W, 3)) * rng.uniform(0.5, 2.0, (H, W, 1))).astype(np.float32)
    prior[rng.uniform(size=(H, W)) < 0.25] = 0.0  # no data
    c["prior"] = prior
    c["image"] = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    return c


@pytest.fixture(scope="module")
def cases(gpu, scene):
    out = {}
    for k, (W, H) in enumerate(SIZES):
        depth, T, intr = _synthetic(H, W, 100 + k)
        for inverse in (0, 1):
            out[(f"synthetic{W}x{H}", inverse)] = _case(depth, T, intr, inverse, 7 * k + inverse)
    for inverse in (0, 1):
        out[("tiny", inverse)] = _case(*_rendered(scene, inverse), inverse, 99 + inverse)
    return out


def _close(got, ref, absolute, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    bar = 1e-6 * np.asarray(absolute, np.float64) + 1e-12
    worst = float((err / bar).max()) if err.size else 0.0
    print(f"{what}: max error {float(err.max()) if err.size else 0.0:.3e}, {worst:.3e} of the bar")
    assert (err <= bar).all(), f"{what}: {float(err.max()):.3e}, {worst:.3e} of the bar"


def _fwd(torch, c):
    return dict(depth=torch.as_tensor(c["depth"]).cuda(), T=torch.as_tensor(c["T"]).cuda())


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("name", NAMES)
def test_populations(cases, name, inverse):
    """What the cases are made of: no normal below 3x3, one at 3x3, both populations from 17x9 on."""
    c = cases[(name, inverse)]
    H, W, valid = c["H"], c["W"], c["valid"]
    print(f"{name} inverse={inverse}: {int(valid.sum())} of {H * W} pixels have a normal")
    if min(H, W) < 3:
        assert not valid.any()
    elif (H, W) == (3, 3):
        assert valid.sum() == 1 and valid[1, 1]
    elif H * W > 20:
        assert valid.any() and not valid[1:-1, 1:-1].all()
        if name != "tiny":
            assert valid.sum() * 4 >= (H - 2) * (W - 2)
        assert not c["read"].all() or name == "tiny"


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("name", NAMES)
def test_depth_to_normal(gpu, cases, name, inverse):
    torch, ops = gpu, pkg("ops")
    c = cases[(name, inverse)]
    fwd = _fwd(torch, c)
    out = torch.full((c["H"], c["W"], 3), float("nan"), device="cuda")
    got = ops.depth_to_normal(fwd, c["intr"], inverse, alpha_min=ALPHA_MIN, out=out)
    assert got is out
    n = _np(out)
    _close(n, c["normal"], 1.0, "normal")
    assert (n[~c["valid"]] == 0).all() and nr.has_normal(n)[c["valid"]].all()
    length = np.linalg.norm(n[c["valid"]].astype(np.float64), axis=-1)
    assert (np.abs(length - 1.0) <= 1e-6).all()
    again = ops.depth_to_normal(fwd, c["intr"], inverse, alpha_min=ALPHA_MIN)  # a new map
    assert again is not out and torch.equal(again, out)


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("name", NAMES)
def test_depth_to_normal_backward(gpu, cases, name, inverse):
    torch, ops = gpu, pkg("ops")
    c = cases[(name, inverse)]
    fwd, G = _fwd(torch, c), torch.as_tensor(c["G"]).cuda()
    H, W = c["H"], c["W"]
    g_depth, g_alpha, a_depth, a_alpha = c["backward"]
    maps = [torch.full((H, W), float("nan"), device="cuda") for _ in range(2)]
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G, maps[0], maps[1], alpha_min=ALPHA_MIN)
    _close(_np(maps[0]), g_depth, a_depth, "grad_depth")
    _close(_np(maps[1]), g_alpha, a_alpha, "grad_alpha")
    for m in maps:  # a pixel no valid normal reads
        assert (_np(m)[~c["read"]] == 0).all()
    if c["valid"].any():
        assert float(maps[0].abs().sum()) > 0 and float(maps[1].abs().sum()) > 0
    # the same bits again
    second = [torch.full((H, W), float("nan"), device="cuda") for _ in range(2)]
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G, second[0], second[1], alpha_min=ALPHA_MIN)
    assert torch.equal(second[0], maps[0]) and torch.equal(second[1], maps[1])
    # either output may be left out
    only = torch.full((H, W), float("nan"), device="cuda")
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G, only, None, alpha_min=ALPHA_MIN)
    assert torch.equal(only, maps[0])
    only = torch.full((H, W), float("nan"), device="cuda")
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G, None, only, alpha_min=ALPHA_MIN)
    assert torch.equal(only, maps[1])
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G, None, None, alpha_min=ALPHA_MIN)
    # accumulate: the first call's floats plus the second call's (of another dL/dn), one float addition each
    G2 = (-2.5 * G + 0.125).contiguous()
    other = [torch.empty(H, W, device="cuda") for _ in range(2)]
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G2, other[0], other[1], alpha_min=ALPHA_MIN)
    acc = [m.clone() for m in maps]
    ops.depth_to_normal_backward(fwd, c["intr"], inverse, G2, acc[0], acc[1], alpha_min=ALPHA_MIN, accumulate=True)
    for a, m, o, what in zip(acc, maps, other, ("grad_depth", "grad_alpha")):
        assert np.array_equal(_np(a), _np(m) + _np(o)), what
    ref2 = nr.depth_to_normal_backward(c["depth"], c["T"], c["intr"], inverse, _np(G2), ALPHA_MIN)
    _close(_np(other[0]), ref2[0], ref2[2], "grad_depth (second dL/dn)")


@pytest.mark.parametrize("inverse", (0, 1))
@pytest.mark.parametrize("name", NAMES)
def test_losses(gpu, cases, name, inverse):
    torch, ops = gpu, pkg("ops")
    c = cases[(name, inverse)]
    H, W = c["H"], c["W"]
    normal = ops.depth_to_normal(_fwd(torch, c), c["intr"], inverse, alpha_min=ALPHA_MIN)
    n = _np(normal)  # the references read the float map the kernels read
    prior, image = torch.as_tensor(c["prior"]).cuda(), torch.as_tensor(c["image"]).cuda()
    w1, w2 = 0.75, 1.5  # (float32 values)
    runs = (("prior", lambda g, w, **k: ops.normal_prior_loss(normal, prior, w, g, **k),
             lambda w: nr.normal_prior_loss(n, c["prior"], w)),
            ("smoothness", lambda g, w, **k: ops.normal_smoothness_loss(normal, image, w, g, edge_scale=2.0, **k),
             lambda w: nr.normal_smoothness_loss(n, c["image"], w, 2.0)),
            ("smoothness without an image", lambda g, w, **k: ops.normal_smoothness_loss(normal, None, w, g, **k),
             lambda w: nr.normal_smoothness_loss(n, None, w)))
    for what, run, ref in runs:
        loss_ref, g_ref, absolute = ref(w1)
        g = torch.full((H, W, 3), float("nan"), device="cuda")
        loss = run(g, w1, blocking=True)
        print(f"{what}: loss {loss!r}, reference {loss_ref!r}")
        assert abs(loss - loss_ref) <= 1e-6 * abs(loss_ref), (what, loss, loss_ref)
        _close(_np(g), g_ref, absolute, "grad_normal, " + what)
        assert (_np(g)[~c["valid"]] == 0).all(), what
        if what == "prior":
            assert (_np(g)[(c["prior"] == 0).all(-1)] == 0).all()
        # the same bits again, value included; no value asked for: None, the same gradient
        g2 = torch.full((H, W, 3), float("nan"), device="cuda")
        assert run(g2, w1, blocking=True) == loss and torch.equal(g2, g)
        g2.fill_(float("nan"))
        assert run(g2, w1) is None and torch.equal(g2, g)
        assert run(None, w1, blocking=True) == loss  # the value alone
        # accumulate
        other = torch.empty(H, W, 3, device="cuda")
        run(other, w2)
        acc = g.clone()
        run(acc, w2, accumulate=True)
        assert np.array_equal(_np(acc), _np(g) + _np(other)), what
        _close(_np(other), ref(w2)[1], ref(w2)[2], "grad_normal at the second weight, " + what)


def test_fronto_parallel_plane_is_exact(gpu):
    torch, ops = gpu, pkg("ops")
    H, W = 19, 70
    intr = (30.0, 28.0, 15.5, 9.25)
    for inverse, value in ((0, 2.0), (1, 0.5)):
        fwd = dict(depth=torch.full((H, W), value, device="cuda"), T=torch.zeros(H, W, device="cuda"))
        n = _np(ops.depth_to_normal(fwd, intr, inverse))
        assert np.array_equal(n[1:-1, 1:-1], np.broadcast_to(np.float32([0.0, 0.0, -1.0]), (H - 2, W - 2, 3)))
        assert (n[0] == 0).all() and (n[-1] == 0).all() and (n[:, 0] == 0).all() and (n[:, -1] == 0).all()


def test_bad_arguments_raise_before_any_launch(gpu):
    torch, ops, lib_mod = gpu, pkg("ops"), pkg("_lib")
    H, W = 9, 17
    intr = (15.0, 15.0, 8.0, 4.0)
    m = torch.rand(H, W, device="cuda") * 0.4
    fwd = dict(depth=m + 0.1, T=m)
    out = torch.full((H, W, 3), 7.0, device="cuda")
    g = torch.full((H, W), 7.0, device="cuda")
    G = torch.ones(H, W, 3, device="cuda")
    wide = torch.ones(H, 2 * W, 3, device="cuda")
    bad = (
        lambda: ops.depth_to_normal(dict(T=m), intr, 0, out=out),                                    # no depth map
        lambda: ops.depth_to_normal(dict(depth=m[:, :-1].contiguous(), T=m), intr, 0, out=out),      # shape
        lambda: ops.depth_to_normal(dict(depth=m.double(), T=m), intr, 0, out=out),                  # dtype
        lambda: ops.depth_to_normal(dict(depth=m.t().contiguous().t(), T=m), intr, 0, out=out),      # not contiguous
        lambda: ops.depth_to_normal(fwd, intr, 0, out=torch.ones(H, W, 4, device="cuda")),
        lambda: ops.depth_to_normal(fwd, intr, 0, alpha_min=0.0, out=out),
        lambda: ops.depth_to_normal(fwd, intr, 0, alpha_min=1.5, out=out),
        lambda: ops.depth_to_normal(fwd, (0.0,) + intr[1:], 0, out=out),                             # fx = 0
        lambda: ops.depth_to_normal(fwd, (intr[0], 0.0) + intr[2:], 0, out=out),                     # fy = 0
        lambda: ops.depth_to_normal(fwd, intr[:2] + (float("nan"), 4.0), 0, out=out),
        lambda: ops.depth_to_normal_backward(fwd, intr, 0, G, g, g, alpha_min=0.0),
        lambda: ops.depth_to_normal_backward(fwd, (0.0,) + intr[1:], 0, G, g, g),
        lambda: ops.depth_to_normal_backward(fwd, intr, 0, G[:, :, :2].contiguous(), g, g),
        lambda: ops.depth_to_normal_backward(fwd, intr, 0, wide[:, ::2], g, g),                      # not contiguous
        lambda: ops.depth_to_normal_backward(fwd, intr, 0, G, g.double(), g),
        lambda: ops.depth_to_normal_backward(fwd, intr, 0, None, g, g),
        lambda: ops.normal_prior_loss(G, G[:-1].contiguous(), 1.0, out),
        lambda: ops.normal_prior_loss(G, G.double(), 1.0, out),
        lambda: ops.normal_prior_loss(G, None, 1.0, out),
        lambda: ops.normal_prior_loss(wide[:, ::2], G, 1.0, out),
        lambda: ops.normal_smoothness_loss(G, G[:, :-1].contiguous(), 1.0, out),
        lambda: ops.normal_smoothness_loss(G, None, 1.0, g),                                         # [H,W] for [H,W,3]
        lambda: ops.normal_smoothness_loss(G, None, 1.0, out, edge_scale=float("inf")),
    )
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert bool((out == 7.0).all()) and bool((g == 7.0).all()), k
    # the library's own checks, behind the Python ones: the project's argument error code, nothing launched
    lib = lib_mod.load()
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    invalid, null = -3, -1  # GSPLAT_ERR_INVALID_ARG, GSPLAT_ERR_NULL_POINTER
    codes = [lib.gsplat_depth_to_normal(p(fwd["depth"]), p(m), H, W, 15.0, 15.0, 8.0, 4.0, 0, 0.0, p(out), st),
             lib.gsplat_depth_to_normal(p(fwd["depth"]), p(m), H, W, 0.0, 15.0, 8.0, 4.0, 0, 0.5, p(out), st),
             lib.gsplat_depth_to_normal(p(fwd["depth"]), p(m), H, W, 15.0, 15.0, float("inf"), 4.0, 0, 0.5, p(out), st),
             lib.gsplat_depth_to_normal(p(fwd["depth"]), p(m), 0, W, 15.0, 15.0, 8.0, 4.0, 0, 0.5, p(out), st),
             lib.gsplat_depth_to_normal_backward(p(fwd["depth"]), p(m), H, W, 15.0, 0.0, 8.0, 4.0, 0, 0.5, p(G), 0, p(g), p(g), st),
             lib.gsplat_depth_to_normal_backward(p(fwd["depth"]), p(m), H, -1, 15.0, 15.0, 8.0, 4.0, 0, 0.5, p(G), 0, p(g), p(g), st),
             lib.gsplat_normal_prior_loss(p(G), p(G), 0, W, 1.0, 0, p(out), None, st),
             lib.gsplat_normal_smoothness_loss(p(G), None, H, 0, 1.0, 1.0, 0, p(out), None, st)]
    torch.cuda.synchronize()
    assert codes == [invalid] * len(codes), codes
    assert "invalid argument" in lib.gsplat_last_error().decode()
    assert lib.gsplat_depth_to_normal(None, p(m), H, W, 15.0, 15.0, 8.0, 4.0, 0, 0.5, p(out), st) == null
    assert lib.gsplat_depth_to_normal_backward(p(fwd["depth"]), p(m), H, W, 15.0, 15.0, 8.0, 4.0, 0, 0.5, None, 0, p(g), p(g), st) == null
    assert bool((out == 7.0).all()) and bool((g == 7.0).all())

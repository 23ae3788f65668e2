"""GPU tests of the median depth (gsplat_context_median_depth): the index against the band of the numpy reference
evaluated in float64 on the float32 oracle forward (tests/median_depth_reference.py), the value bit for bit against the z
the forward stored, the agreement with the forward's own transmittance, monotony in the threshold, reproducibility after
every kind of forward, occlusion, long lists, the refusals and the Trainer's call."""
import ctypes

import numpy as np
import pytest

import median_depth_reference as mdr
from conftest import max_pixels_above_tol, max_stop_index_mismatches, pkg

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _oracle(orc, scene, params, cam, L):
    c = scene.CONFIG
    return orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, L, threads=8)


def _occlusion_scene(scene):
    """64 x 64: six large opaque gaussians (logit 20), nearest first, in front of 100 small ones; the walls' centres lie
    left of the image, so that their alpha stays below the 0.99 cap on every pixel (tests/test_contribution_gpu.py)."""
    W = H = 64
    N, walls = 106, 6
    p = scene.make_gaussians(N, W, H, 0)
    cam = scene.make_camera(W, H, 0)
    p["xyz"][walls:, 2] += 4.0
    for k in range(walls):
        z = 1.0 + 0.1 * k
        p["xyz"][k] = ((-80.0 - W / 2) * z / cam["fx"], 0.0, z)
        p["scale"][k] = np.log(8.0)
        p["quaternion"][k] = (1.0, 0.0, 0.0, 0.0)
        p["opacity"][k] = 20.0
    return N, W, H, 0, p, cam


def _long_list_scene(scene):
    """32 x 32: 2200 tiny, mostly faint gaussians stacked over the first tile's middle: a list of ~2400 entries
    (tests/test_contribution_gpu.py)."""
    W = H = 32
    N, L = 2600, 0
    p = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, 0)
    rng = np.random.default_rng(11)
    lo, hi = 200, 2400
    k = hi - lo
    z = rng.uniform(3.0, 9.0, k)
    u, v = 9.0 + rng.uniform(-5, 5, k), 9.0 + rng.uniform(-5, 5, k)
    p["xyz"][lo:hi, 0] = (u - W / 2) * z / cam["fx"]
    p["xyz"][lo:hi, 1] = (v - H / 2) * z / cam["fy"]
    p["xyz"][lo:hi, 2] = z
    p["scale"][lo:hi] = np.log(rng.uniform(0.004, 0.012, (k, 3)))
    p["opacity"][lo:hi] = rng.choice([-5.0, -4.0, -3.0, -1.0, 3.0], size=k, p=[0.45, 0.3, 0.15, 0.08, 0.02])
    return N, W, H, L, p, cam


_REF = {}  # scene name -> parameters, camera, the oracle forward and the bands per threshold, made once and left alone


def _shared(scene, orc, name):
    if name not in _REF:
        if name == "partial":  # 70 x 45: partial tiles in both directions
            N, W, H, L = 300, 70, 45, 1
            params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
        elif name == "occlusion":
            N, W, H, L, params, cam = _occlusion_scene(scene)
        elif name == "long":
            N, W, H, L, params, cam = _long_list_scene(scene)
        else:
            N, W, H, L = scene.WORKLOADS[name][:4]
            params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
        _REF[name] = dict(N=N, W=W, H=H, L=L, params=params, cam=cam, ref=_oracle(orc, scene, params, cam, L), band={})
    return _REF[name]


def _band(case, threshold):
    if threshold not in case["band"]:
        case["band"][threshold] = mdr.median_band(case["ref"], case["W"], case["H"], threshold)
    return case["band"][threshold]


def _on_device(case):
    raster = pkg("raster")
    return raster, raster.device_params(case["params"]), raster.device_camera(case["cam"])


def _median(torch, ctx, H, W, threshold, with_index=True):
    index = torch.full((H, W), -7, dtype=torch.int32, device="cuda") if with_index else None
    depth = ctx.median_depth(threshold, index=index)
    torch.cuda.synchronize()
    return depth, index


def _check_band(case, index, threshold, what):
    """Assertion 1: lo <= index <= hi, -1 as +infinity, but for the borderline decisions conftest allows the forward."""
    P = case["W"] * case["H"]
    lo, hi = _band(case, threshold)
    out = mdr.outside_band(_np(index), lo, hi)
    allowed = max_stop_index_mismatches(P) + max_pixels_above_tol(P)
    print(f"{what}, threshold {threshold}: {int(out.sum())} of {P} pixels outside the band (allowed {allowed}); "
          f"{int((_np(index) >= 0).sum())} have a surface")
    assert int(out.sum()) <= allowed, what


def _check_value(fwd, depth, index, W, H, what):
    """Assertion 2: depth is, bit for bit, the z the forward stored for the list entry `index`; 0 iff index is -1."""
    d, i = _np(depth), _np(index).astype(np.int64)
    assert np.array_equal(d == 0, i < 0), what
    ranges, sorted_ids = _np(fwd["ranges"]).astype(np.int64), _np(fwd["sorted"]).astype(np.int64)
    start = ranges[mdr.tile_of_pixels(W, H)]
    length = np.diff(ranges)[mdr.tile_of_pixels(W, H)]
    assert (i < np.minimum(length, _np(fwd["n"]).reshape(H, W))).all(), what
    z = _np(fwd["xyz_c"]).reshape(-1, 3)[:, 2].copy()  # compacted order, as sorted names the gaussians
    has = i >= 0
    want = z[sorted_ids[(start + np.maximum(i, 0))[has]]]
    assert np.array_equal(d[has].view(np.uint32), want.view(np.uint32)), what
    assert (d[has] > 0).all()


@pytest.mark.parametrize("name", ["tiny", "small", "partial", "occlusion"])
def test_index_in_the_band_value_exact(gpu, scene, orc, name):
    torch, case = gpu, _shared(scene, orc, name)
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    for it in range(2):  # the second forward walks the compacted slots
        fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
        for threshold in (0.5, 0.9):
            depth, index = _median(torch, ctx, H, W, threshold)
            _check_band(case, index, threshold, f"{name}, forward {it}")
            _check_value(fwd, depth, index, W, H, f"{name}, forward {it}, threshold {threshold}")
    if name == "occlusion":  # assertion 7: every pixel's median lies within the six wall layers
        depth, index = _median(torch, ctx, H, W, 0.5)
        assert bool((index >= 0).all()) and bool((index < 6).all())
        wall_z = np.sort(_np(fwd["xyz_c"])[:, 2])[:6]  # the six walls are the nearest gaussians
        assert np.isin(_np(depth), wall_z).all()


@pytest.mark.parametrize("name", ["tiny", "small", "partial"])
def test_surface_exactly_where_the_forward_s_transmittance_says_and_monotone(gpu, scene, orc, name):
    """Assertions 3 and 4: these lists are walked whole, so the replay's T is the forward's bit for bit."""
    torch, case = gpu, _shared(scene, orc, name)
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    T = fwd["T"].reshape(H, W)
    idx = {}
    for threshold in (0.5, 0.1, 0.9):
        _, idx[threshold] = _median(torch, ctx, H, W, threshold)
        thr32 = torch.tensor(threshold, dtype=torch.float32, device="cuda")  # the library's float
        assert torch.equal(idx[threshold] >= 0, T <= thr32), threshold
    all3 = (idx[0.9] >= 0) & (idx[0.5] >= 0) & (idx[0.1] >= 0)
    assert bool(all3.any())
    assert bool((idx[0.9][all3] <= idx[0.5][all3]).all()) and bool((idx[0.5][all3] <= idx[0.1][all3]).all())
    assert bool((idx[0.9] < idx[0.1])[all3].any())


def test_same_bits_in_every_run_route_and_kind_of_forward(gpu, scene, orc):
    """Assertions 5 and 6."""
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    c = scene.CONFIG
    plain = raster.RasterContext(N, W, H)
    fwd = plain.rasterize_image(dp, dc, c, 0.0, L)
    depth, index = _median(torch, plain, H, W, 0.5)
    again = _median(torch, plain, H, W, 0.5)
    assert torch.equal(again[0], depth) and torch.equal(again[1], index)
    alone, none = _median(torch, plain, H, W, 0.5, with_index=False)
    assert none is None and torch.equal(alone, depth)
    out = torch.full((H, W), -3.0, device="cuda")
    assert plain.median_depth(0.5, out=out) is out and torch.equal(out, depth)
    grads = plain.alloc_gradients(fwd["num_culled"], L)
    plain.backward_pass(dp, dc, torch.as_tensor(scene.make_grad_image(W, H)).cuda(), 0.0, L, grads)
    after = _median(torch, plain, H, W, 0.5)
    assert torch.equal(after[0], depth) and torch.equal(after[1], index)
    for route in (1, 2):
        other = raster.RasterContext(N, W, H)
        other.set_binning_route(route)
        other.rasterize_image(dp, dc, c, 0.0, L)
        got = _median(torch, other, H, W, 0.5)
        assert torch.equal(got[0], depth) and torch.equal(got[1], index), route
    for kind in ("lean", "render_only", "depth", "inverse"):
        ctx = raster.RasterContext(N, W, H)
        if kind == "inverse":
            ctx.set_depth(True, inverse=True)  # the output is z all the same
        else:
            {"lean": ctx.set_lean_forward, "render_only": ctx.set_render_only, "depth": ctx.set_depth}[kind](True)
        ctx.rasterize_image(dp, dc, c, 0.0, L)
        got = _median(torch, ctx, H, W, 0.5)
        assert torch.equal(got[0], depth) and torch.equal(got[1], index), kind


def test_long_lists_are_walked_whole(gpu, scene, orc):
    """Assertion 8: assertions 1 and 2 on a list the forward segments (its T is another product order: no assertion 3)."""
    torch, case = gpu, _shared(scene, orc, "long")
    raster, dp, dc = _on_device(case)
    N, W, H, L, ref = case["N"], case["W"], case["H"], case["L"], case["ref"]
    assert int(np.diff(ref["ranges"]).max()) > 1488 and int(np.asarray(ref["n"]).max()) > 1488
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    ctx.set_segment_options(gate=0.0)
    for it in range(5):  # (the forward's own split follows the figures of the forward two back)
        fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    assert ctx.counters()["segmented_forwards"] > 0, ctx.counters()
    for threshold in (0.5, 0.9, 0.02):  # (0.02: answers far down the list, and pixels that walk all of it for none)
        depth, index = _median(torch, ctx, H, W, threshold)
        _check_band(case, index, threshold, "long list")
        _check_value(fwd, depth, index, W, H, f"long list, threshold {threshold}")
        print(f"long list, threshold {threshold}: largest index {int(index.max())}, none on {int((index < 0).sum())} pixels")


def test_refusals_launch_nothing(gpu, scene):
    """Assertion 9."""
    torch, lib, raster = gpu, pkg("_lib"), pkg("raster")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_gaussians(N, W, H, L))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    depth = torch.full((H, W), 7.0, device="cuda")
    index = torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    host = np.zeros((H, W), np.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pd, pi = ctypes.c_void_p(depth.data_ptr()), ctypes.c_void_p(index.data_ptr())

    def refused(ctx, n=N, threshold=0.5, d=pd, i=pi):
        h = ctx._h if ctx is not None else None
        rc = lib.load().gsplat_context_median_depth(h, n, threshold, d, i, st)
        assert rc == -3, rc  # GSPLAT_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert bool((depth == 7).all()) and bool((index == 7).all())

    refused(None)                                    # null context
    ctx = raster.RasterContext(N, W, H)
    refused(ctx)                                     # no forward yet
    with pytest.raises(lib.GsplatError):
        ctx.median_depth(0.5)
    ctx.rasterize_image(dp, dc, c, 0.0, L)
    refused(ctx, n=N - 1)                            # not the recorded forward's N
    for bad in (0.0, 1.0, -0.25, float("nan"), float("inf")):
        refused(ctx, threshold=bad)
    refused(ctx, d=None)                             # null depth
    refused(ctx, d=ctypes.c_void_p(host.ctypes.data))            # depth on the host
    refused(ctx, i=ctypes.c_void_p(host.ctypes.data))            # index on the host
    assert not host.any()
    for kw in (dict(out=torch.zeros(H, W)), dict(out=torch.zeros(H, W + 1, device="cuda")),
               dict(index=torch.zeros(H, W, device="cuda")), dict(out=torch.zeros(W, H, device="cuda").t())):
        with pytest.raises(ValueError):
            ctx.median_depth(0.5, **kw)
    got = ctx.median_depth(0.5, out=depth, index=index)  # and the same arrays are written by a good call
    torch.cuda.synchronize()
    fresh_index = torch.empty_like(index)
    fresh = ctx.median_depth(0.5, index=fresh_index)
    assert got is depth and torch.equal(depth, fresh) and torch.equal(index, fresh_index)
    assert not bool((depth == 7).any()) and bool((index < 0).any()) and bool((index > 7).any())


def test_trainer_render_median_depth(gpu, scene):
    """Assertion 10: the Trainer's map is the context's, and the context's flags are as before."""
    torch, raster, trainer_mod = gpu, pkg("raster"), pkg("trainer")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    params = raster.device_params(scene.make_gaussians(N, W, H, 0))
    cam = raster.device_camera(scene.make_camera(W, H, 0))
    blank = torch.zeros(H, W, 3, device="cuda")
    for cfg in (None, dict(antialiased=True)):
        t = trainer_mod.Trainer({k: v.clone() for k, v in params.items()}, [(cam, blank)], cfg, scene_extent=5.0, seed=1)
        ctx = t._context_for(t.num_gaussians)
        before = (ctx._depth, ctx._depth_inverse, ctx._depth_moment)
        got = t.render_median_depth(cam, 0.5)
        assert (ctx._depth, ctx._depth_inverse, ctx._depth_moment) == before
        fwd = ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)  # a training forward: render-only is off again
        want, T = ctx.median_depth(0.5), fwd["T"].reshape(H, W).clone()
        torch.cuda.synchronize()
        assert got.shape == (H, W) and torch.equal(got, want) and bool((got > 0).any()) and bool((got == 0).any())
        assert torch.equal(t.render_median_depth(cam, 0.9) > 0, T <= torch.tensor(0.9, dtype=torch.float32, device="cuda"))

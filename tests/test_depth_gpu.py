"""GPU parity of the depth / opacity maps (gsplat_context_set_depth, gsplat_backward_render_depth): the depth map against
the oracle's render_image on the colour (z, 1, 0), alpha = 1 - T exactly, the plain outputs untouched by depth mode, and
every leaf gradient against the oracle's chain with dL/d depth and dL/d alpha composed in (tests/depth_reference.py)."""
import numpy as np
import pytest

import depth_reference
from conftest import assert_grad_close, perf_check, pkg

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _maps(torch, W, H, seed=3):
    rng = np.random.default_rng(seed)
    # random, non-zero everywhere: the per-part gate of the reference and the kernel's combined gate see the same pairs
    gd = (rng.uniform(0.2, 1.0, (H, W)) * rng.choice([-1.0, 1.0], (H, W)) / (W * H)).astype(np.float32)
    ga = (rng.uniform(0.2, 1.0, (H, W)) * rng.choice([-1.0, 1.0], (H, W)) / (W * H)).astype(np.float32)
    return gd, ga, torch.as_tensor(gd).cuda(), torch.as_tensor(ga).cuda()


def _check_depth(fwd, ref, dref, image_ref):
    """depth within 1e-5 relative; a pixel beyond it must be one the image check flags too (an alpha threshold flip)."""
    got = _np(fwd["depth"]).astype(np.float64)
    err = np.abs(got - dref)
    bad = err > 1e-5 * np.maximum(np.abs(dref), 1e-3)
    img_bad = np.abs(_np(fwd["image"]).astype(np.float64) - image_ref).sum(-1) > 1e-5
    n_bad = np.asarray(_np(fwd["n"]) != ref["n"])
    assert not (bad & ~(img_bad | n_bad)).any(), f"{int(bad.sum())} depth pixels off, image / stop index agree there"
    assert bad.mean() < 1e-4, f"{int(bad.sum())} depth pixels off"


def _check_grads(grads, g):
    for k, rk in (("xyz", "xyz"), ("rgb", "band0"), ("sh", "sh"), ("opacity", "opacity"), ("scale", "scale"),
                  ("quaternion", "quaternion"), ("conic", "conic"), ("uv", "uv"), ("J", "J"), ("sigma", "sigma"),
                  ("xyz_c", "xyz_c"), ("precompute_rgb", "rgb_pre")):
        if g.get(rk) is not None and grads.get(k) is not None:
            assert_grad_close(_np(grads[k]), g[rk], "grad_" + k)


def _case(torch, scene, N, W, H, L, view=2):
    raster = pkg("raster")
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, view)
    return raster, params, cam, raster.device_params(params), raster.device_camera(cam)


CASES = [("tiny", None), ("small", None), ("l0", (3000, 200, 120, 0)), ("l1", (3000, 200, 120, 1)),
         ("l2", (3000, 200, 120, 2)), ("odd1", (1, 17, 9, 0)), ("odd2", (3, 33, 31, 1)), ("odd3", (37, 100, 7, 2)),
         ("odd4", (255, 16, 16, 3)), ("odd5", (257, 130, 66, 3))]


@pytest.mark.parametrize("name,shape", CASES)
def test_depth_and_gradients_match_oracle(gpu, scene, orc, name, shape):
    torch = gpu
    N, W, H, L = shape if shape else scene.WORKLOADS[name][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True)
    try:
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    except pkg("_lib").GsplatError as e:
        assert e.code == -5
        return
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    dref, aref = depth_reference.depth_alpha(orc, ref, W, H, threads=8)
    _check_depth(fwd, ref, dref.astype(np.float64), np.asarray(ref["image"], np.float64))
    assert torch.equal(fwd["alpha"], 1.0 - fwd["T"])
    np.testing.assert_allclose(_np(fwd["alpha"]), aref, rtol=0, atol=2e-5)
    gi = scene.make_grad_image(W, H)
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    for which in ("depth", "alpha", "both"):
        GD = gd if which != "alpha" else None
        GA = ga if which != "depth" else None
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        ctx.backward_pass(dp, dc, torch.as_tensor(gi).cuda(), c["bg"], L, grads,
                          grad_depth=gd_d if GD is not None else None, grad_alpha=ga_d if GA is not None else None)
        torch.cuda.synchronize()
        g = depth_reference.backward_pass(orc, ref, cam, gi, GD, GA, c["bg"], L, threads=8)
        _check_grads(grads, g)


def test_depth_mode_keeps_the_plain_outputs(gpu, scene):
    """Image, T, n and lists of a depth-mode forward are the plain forward's bits, in training, lean and render-only
    contexts, which give one depth map; a depth-mode forward followed by the plain backward, and zero depth / alpha
    gradients through the depth entry points, give the plain backward's gradients (within the float atomics' order)."""
    torch = gpu
    N, W, H, L = scene.WORKLOADS["small"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    keys = ("image", "T", "n", "sorted", "ranges")
    plain = raster.RasterContext(N, W, H)
    fp = plain.rasterize_image(dp, dc, c, c["bg"], L)
    assert "depth" not in fp
    base = {k: fp[k].clone() for k in keys}
    gp = plain.alloc_gradients(fp["num_culled"], L)
    plain.backward_pass(dp, dc, gi, c["bg"], L, gp)
    depth_maps = []
    for mode in ("train", "lean", "render_only"):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_depth(True)
        if mode == "lean":
            ctx.set_lean_forward(True)
        if mode == "render_only":
            ctx.set_render_only(True)
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        for k in keys:
            assert torch.equal(f[k], base[k]), (mode, k)
        depth_maps.append(f["depth"].clone())
        if mode == "train":
            g_plain = ctx.alloc_gradients(f["num_culled"], L)
            ctx.backward_pass(dp, dc, gi, c["bg"], L, g_plain)  # depth forward + plain backward
            torch.cuda.synchronize()
            for k in g_plain:  # (the compositing backward's float atomics add in launch order: not bitwise)
                assert_grad_close(_np(g_plain[k]), _np(gp[k]), k, rel=1e-5)
            z = torch.zeros(H, W, device="cuda")
            g0 = ctx.alloc_gradients(f["num_culled"], L)
            ctx.backward_pass(dp, dc, gi, c["bg"], L, g0, grad_depth=z, grad_alpha=z)
            torch.cuda.synchronize()
            for k in g0:
                assert_grad_close(_np(g0[k]), _np(gp[k]), k, rel=1e-5)
    assert torch.equal(depth_maps[0], depth_maps[1]) and torch.equal(depth_maps[0], depth_maps[2])


def test_depth_gradients_after_a_plain_forward_raise(gpu, scene):
    torch = gpu
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    _, _, gd_d, ga_d = _maps(torch, W, H)
    grads = ctx.alloc_gradients(f["num_culled"], L)
    for t in grads.values():
        t.fill_(7.0)
    before = {k: v.clone() for k, v in dp.items()}
    for kw in (dict(grad_depth=gd_d), dict(grad_alpha=ga_d)):
        with pytest.raises(pkg("_lib").GsplatError):
            ctx.backward_pass(dp, dc, gi, c["bg"], L, grads, **kw)
        with pytest.raises(pkg("_lib").GsplatError):
            ctx.backward_render(gi, c["bg"], **kw)
    torch.cuda.synchronize()
    for t in grads.values():
        assert bool((t == 7.0).all())
    for k in dp:
        assert torch.equal(dp[k], before[k]), k
    with pytest.raises(pkg("_lib").GsplatError):
        pkg("_lib").check(ctx._lib.gsplat_context_depth_map(ctx._h, __import__("ctypes").byref(__import__("ctypes").c_void_p())))


def test_every_per_gaussian_entry_point_takes_the_depth_term(gpu, scene, orc):
    """After gsplat_backward_render_depth the per-gaussian calls all read row slot 9: index ranges, the split exchange's
    common columns and the Adam-inside form in the Trainer's default mode against the unfused optimizer step."""
    torch, opt_mod = gpu, pkg("optimizer")
    N, W, H, L = 5000, 256, 144, 3
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L, view=1)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    M = fwd["num_culled"]
    ctx.backward_render(gi, c["bg"], grad_depth=gd_d, grad_alpha=ga_d)
    whole = ctx.backward_gaussians(dp, dc, L, ctx.alloc_gradients(M, L, intermediates=("uv", "xyz_c")))
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    g = depth_reference.backward_pass(orc, ref, cam, scene.make_grad_image(W, H), gd, ga, c["bg"], L, threads=8)
    _check_grads(whole, g)
    parts = ctx.alloc_gradients(M, L)
    for lo, hi in ((0, N // 3), (N // 3, 2 * N // 3), (2 * N // 3, N)):
        ctx.backward_gaussians_range(dp, dc, L, parts, lo, hi)
    torch.cuda.synchronize()
    for k in ("xyz", "opacity", "scale", "quaternion"):
        assert torch.equal(parts[k], whole[k]), k
    common = torch.zeros(N, 12, device="cuda")
    ctx.backward_gaussians_split(dp, dc, L, common)
    torch.cuda.synchronize()
    c2g = fwd["compact_to_global"].long()
    assert torch.equal(common[c2g, 0:3], whole["xyz"]) and torch.equal(common[c2g, 3], whole["opacity"])
    # the Trainer's default choreography (backward_pass_adam, mode 2) against backward + the unfused optimizer step
    dp_b = {k: v.clone() for k, v in dp.items()}
    oa, ob = opt_mod.AdamOptimizer(dp, L, scene_extent=2.5), opt_mod.AdamOptimizer(dp_b, L, scene_extent=2.5)
    g_a = ctx.alloc_gradients(M, L, intermediates=("uv",), factored_sh=True)
    ctx.backward_gaussians(dp, dc, L, g_a)
    oa.step(1, fwd, g_a, campos=cam["campos"])
    ctx.backward_gaussians_adam(dp_b, dc, L, ob.fused_state(1, mode=2))
    torch.cuda.synchronize()
    for k in oa.names:
        assert torch.equal(dp[k], dp_b[k]), k
        assert torch.equal(oa.exp_avg[k], ob.exp_avg[k]) and torch.equal(oa.exp_avg_sq[k], ob.exp_avg_sq[k]), k
    assert torch.equal(oa.uv_grad_accum, ob.uv_grad_accum)


@pytest.mark.parametrize("mode", [0, 1])
def test_adam_forms_take_the_depth_term(gpu, scene, orc, mode):
    """The other two Adam-inside forms behind gsplat_backward_render_depth (struct modes 0 and 1: preprocess_bwd_kernel's
    kAdam 2 and 1 with kDepthRow; mode 2 is in the test above), on the 200-gaussian 64x48 `tiny` scene (four waves of
    compacted slots, the last one partial).  The gradient arrays the call stores meet the float32 oracle's chain with
    dL/d depth and dL/d alpha composed in at conftest's bars, and parameters, moments and statistics are those of the
    plain depth backward + the unfused optimizer step, bit for bit."""
    torch, opt_mod = gpu, pkg("optimizer")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L, view=1)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True)
    gi = scene.make_grad_image(W, H)
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    M = fwd["num_culled"]
    assert M > 128  # more than two waves
    ctx.backward_render(torch.as_tensor(gi).cuda(), c["bg"], grad_depth=gd_d, grad_alpha=ga_d)
    dp_b = {k: v.clone() for k, v in dp.items()}
    oa, ob = opt_mod.AdamOptimizer(dp, L, scene_extent=2.5), opt_mod.AdamOptimizer(dp_b, L, scene_extent=2.5)
    g_a = ctx.alloc_gradients(M, L, intermediates=True, factored_sh=True)
    g_b = ctx.alloc_gradients(M, L, intermediates=True, factored_sh=True)
    for t in g_b.values():
        if t is not None:
            t.fill_(float("nan"))
    ctx.backward_gaussians(dp, dc, L, g_a)
    oa.step(1, fwd, g_a, campos=cam["campos"])
    ctx.backward_gaussians_adam(dp_b, dc, L, ob.fused_state(1, mode=mode), g_b)
    if mode == 1:  # the SH and the position group behind the kernel
        ob.step_after_partial_backward(1, fwd, g_b, cam["campos"])
    torch.cuda.synchronize()
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    g = depth_reference.backward_pass(orc, ref, cam, gi, gd, ga, c["bg"], L, threads=8)
    _check_grads({k: v for k, v in g_b.items() if v is not None}, g)
    no_depth = depth_reference.backward_pass(orc, ref, cam, gi, None, None, c["bg"], L, threads=8)
    assert np.abs(np.asarray(g["xyz"]) - np.asarray(no_depth["xyz"])).max() > 0  # the depth term is part of what is checked
    for k in oa.names:
        assert torch.equal(dp[k], dp_b[k]), k
        assert torch.equal(oa.exp_avg[k], ob.exp_avg[k]) and torch.equal(oa.exp_avg_sq[k], ob.exp_avg_sq[k]), k
    assert torch.equal(oa.uv_grad_accum, ob.uv_grad_accum) and torch.equal(oa.grad_accum_dur, ob.grad_accum_dur)


def _long_list_scene(scene):
    N, W, H, L = 24000, 160, 96, 1
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H)
    rng = np.random.default_rng(11)
    for lo, hi, (cu, cv), spread in ((2000, 4200, (24.0, 24.0), 5.0), (4200, 9200, (88.0, 40.0), 7.0),
                                     (9200, 16200, (136.0, 72.0), 4.0), (16200, 18200, (40.0, 72.0), 3.0)):
        k = hi - lo
        z = rng.uniform(3.0, 9.0, k)
        u, v = cu + rng.uniform(-spread, spread, k), cv + rng.uniform(-spread, spread, k)
        params["xyz"][lo:hi, 0] = (u - W / 2) * z / cam["fx"]
        params["xyz"][lo:hi, 1] = (v - H / 2) * z / cam["fy"]
        params["xyz"][lo:hi, 2] = z
        params["scale"][lo:hi] = np.log(rng.uniform(0.004, 0.012, (k, 3)))
        params["opacity"][lo:hi] = rng.choice([-5.0, -4.0, -3.0, -1.0, 3.0], size=k, p=[0.45, 0.3, 0.15, 0.08, 0.02])
    return N, W, H, L, params, cam


def test_long_lists_in_segments(gpu, scene, orc):
    """The scene of test_fused_gpu.py::test_long_lists_split_into_segments_for_the_backward: both segment paths are
    taken, depth and gradients are the oracle's on every iteration, and the segmented forward's depth map carries the
    same bits in every run and under every segment option."""
    torch, raster = gpu, pkg("raster")
    N, W, H, L, params, cam = _long_list_scene(scene)
    c = scene.CONFIG
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    ctx.set_depth(True)
    gi = scene.make_grad_image(W, H)
    gi_d = torch.as_tensor(gi).cuda()
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    dref, _ = depth_reference.depth_alpha(orc, ref, W, H, threads=8)
    g = depth_reference.backward_pass(orc, ref, cam, gi, gd, ga, c["bg"], L, threads=8)
    seg_depth = None
    for it in range(5):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        _check_depth(fwd, ref, dref.astype(np.float64), np.asarray(ref["image"], np.float64))
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        ctx.backward_pass(dp, dc, gi_d, c["bg"], L, grads, grad_depth=gd_d, grad_alpha=ga_d)
        torch.cuda.synchronize()
        _check_grads(grads, g)
        if it == 3:
            seg_depth = fwd["depth"].clone()
        elif it == 4:
            assert torch.equal(fwd["depth"], seg_depth)
    cnt = ctx.counters()
    assert cnt["segmented_backwards"] > 0 and cnt["segmented_forwards"] > 0, cnt
    for opts in (dict(thin_layer_blocks=0), dict(thin_layer_blocks=1 << 20), dict(poll_budget=1, thin_layer_blocks=1 << 20)):
        other = raster.RasterContext(N, W, H)
        other.set_binning_route(1)
        other.set_depth(True)
        other.set_segment_options(**opts)
        for it in range(4):
            out = other.rasterize_image(dp, dc, c, c["bg"], L)
        assert other.counters()["segmented_forwards"] == 1, opts
        assert torch.equal(out["depth"], seg_depth), opts


def test_full_size_depth_and_cost(gpu, scene, orc, config3_case):
    torch, raster = gpu, pkg("raster")
    k = config3_case
    N, W, H, L = k["N"], k["W"], k["H"], k["L"]
    c = scene.CONFIG
    dp, dc = raster.device_params(k["params"]), raster.device_camera(k["cam"])
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    ref = k["ref"]
    dref, _ = depth_reference.depth_alpha(orc, ref, W, H, threads=16)
    _check_depth(fwd, ref, dref.astype(np.float64), np.asarray(ref["image"], np.float64))
    # cost: a depth-mode forward + backward against a plain one, alternating, in this process
    gi = torch.as_tensor(k["gi"]).cuda()
    _, _, gd_d, ga_d = _maps(torch, W, H)
    plain = raster.RasterContext(N, W, H)
    gp = plain.alloc_gradients(N, L)
    gdp = ctx.alloc_gradients(N, L)

    def step(cx, depth):
        f = cx.rasterize_image(dp, dc, c, c["bg"], L)
        grads = gdp if depth else gp
        sub = {kk: (v[:f["num_culled"]] if v is not None else None) for kk, v in grads.items()}
        if depth:
            cx.backward_pass(dp, dc, gi, c["bg"], L, sub, grad_depth=gd_d, grad_alpha=ga_d)
        else:
            cx.backward_pass(dp, dc, gi, c["bg"], L, sub)

    times = {True: [], False: []}
    for rep in range(24):
        for depth in (False, True):
            cx = ctx if depth else plain
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(cx, depth)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 4:
                times[depth].append(e0.elapsed_time(e1))
    ratio = float(np.median(times[True]) / np.median(times[False]))
    perf_check(ratio <= 1.3, f"depth-mode step {ratio:.3f}x the plain step (bar 1.3x)")

"""GPU parity of depth mode's options (gsplat_context_set_depth_mode, gsplat_backward_render_depth2): the inverse-depth
and second-moment maps against the oracle's render_image on the colour (s, 1, s^2), the plain outputs untouched, every leaf
and intermediate gradient against the oracle's chain with dL/dD, dL/dA and dL/dQ composed in
(tests/depth_moment_reference.py), the long-list segment paths, every per-gaussian entry point, and the refusals."""
import ctypes

import numpy as np
import pytest

import depth_moment_reference as dmr
from conftest import assert_grad_close, perf_check, pkg
from test_depth_gpu import CASES, _case, _check_depth, _check_grads, _long_list_scene, _maps, _np

pytestmark = pytest.mark.gpu

MODES = [(1, 0), (0, 1), (1, 1)]


def _three_maps(torch, W, H):
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    gq, _, gq_d, _ = _maps(torch, W, H, seed=5)
    return (gd, ga, gq), (gd_d, ga_d, gq_d)


def _check_map(fwd, key, ref, mref):
    _check_depth({"depth": fwd[key], "image": fwd["image"], "n": fwd["n"]}, ref, np.asarray(mref, np.float64),
                 np.asarray(ref["image"], np.float64))


def _check_depth_term(orc, grads, g, ref, cam, W, H):
    """dL/dz on its own.  Inside dL/d xyz_c the depth term is a few 1e-4 of the norm (the uv term carries W / 2 and fx / z),
    so the 1e-3 bars of _check_grads cannot see it.  It is recovered here: the z column of the kernel's dL/d xyz_c minus
    what the kernel's own dL/d uv and dL/dJ give through the projection and Jacobian backwards (the oracle's operators in
    float64), against the reference's dL/dz.  Bar: the project's 1e-3 relative L2 on dL/dz, plus the rounding of the
    float32 chain the term was added to, 16 eps32 of its terms' magnitudes (about ten operations); that allowance must
    stay below 1e-2 of |dL/dz|, or the check would say nothing."""
    f64 = np.float64
    fx, fy = f64(cam["fx"]), f64(cam["fy"])
    tan_x, tan_y = np.tan(2.0 * np.arctan(W / (2.0 * fx)) * 0.5), np.tan(2.0 * np.arctan(H / (2.0 * fy)) * 0.5)
    a = np.asarray(orc.compute_projection_jacobian_backward(ref["xyz_c"], fx, fy, tan_x, tan_y, _np(grads["J"]), None, f64)).reshape(-1, 3)[:, 2]
    b = np.asarray(orc.project_to_screen_backward(ref["xyz_c"], cam["proj"], _np(grads["uv"]), W, H, None, f64)).reshape(-1, 3)[:, 2]
    got = _np(grads["xyz_c"]).astype(f64)[:, 2] - a - b
    want = np.asarray(g["z"], f64)
    norm = np.linalg.norm(want)
    if norm == 0:
        assert np.linalg.norm(got) <= 16 * np.finfo(np.float32).eps * np.linalg.norm(np.abs(a) + np.abs(b))
        return
    rounding = 16 * np.finfo(np.float32).eps * np.linalg.norm(np.abs(a) + np.abs(b) + np.abs(want))
    assert rounding < 1e-2 * norm, (rounding, norm)
    err = np.linalg.norm(got - want)
    assert err <= 1e-3 * norm + rounding, f"dL/dz: relative L2 error {err / norm:.3e} (rounding allowance {rounding / norm:.1e})"


@pytest.fixture(scope="module")
def oracle_forward(scene, orc):
    """The float32 oracle's forward per case, computed once and shared by the modes (never changed)."""
    cache = {}

    def get(name, shape):
        if name not in cache:
            N, W, H, L = shape if shape else scene.WORKLOADS[name][:4]
            params, cam, c = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 2), scene.CONFIG
            cache[name] = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
        return cache[name]
    return get


@pytest.mark.parametrize("inverse,moment", MODES)
@pytest.mark.parametrize("name,shape", CASES)
def test_maps_and_gradients_match_oracle(gpu, scene, orc, oracle_forward, name, shape, inverse, moment):
    torch = gpu
    N, W, H, L = shape if shape else scene.WORKLOADS[name][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True, inverse=bool(inverse), moment=bool(moment))
    try:
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    except pkg("_lib").GsplatError as e:
        assert e.code == -5
        return
    ref = oracle_forward(name, shape)
    dref, aref, qref = dmr.maps(orc, ref, W, H, bool(inverse), threads=8)
    _check_map(fwd, "depth", ref, dref)
    assert ("depth2" in fwd) == bool(moment)
    if moment:
        _check_map(fwd, "depth2", ref, qref)
    np.testing.assert_allclose(_np(fwd["alpha"]), aref, rtol=0, atol=2e-5)
    gi = scene.make_grad_image(W, H)
    (gd, ga, gq), (gd_d, ga_d, gq_d) = _three_maps(torch, W, H)
    subsets = ("D", "Q", "ADQ") if moment else ("D", "AD")
    for which in subsets:
        use = dict(D="D" in which, A="A" in which, Q="Q" in which)
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        ctx.backward_pass(dp, dc, torch.as_tensor(gi).cuda(), c["bg"], L, grads, grad_depth=gd_d if use["D"] else None,
                          grad_alpha=ga_d if use["A"] else None, grad_depth2=gq_d if use["Q"] else None)
        torch.cuda.synchronize()
        g = dmr.backward_pass(orc, ref, cam, gi, gd if use["D"] else None, ga if use["A"] else None,
                              gq if use["Q"] else None, c["bg"], L, bool(inverse), threads=8)
        _check_grads(grads, g)
        _check_depth_term(orc, grads, g, ref, cam, W, H)


def test_nothing_else_moves(gpu, scene):
    """Image, T, n and the lists of a (1,1) forward are the plain forward's bits in training, lean and render-only
    contexts; set_depth(True) gives the bits of set_depth_mode(0, 0); zero maps through the new entry points give the plain
    backward's gradients (within the float atomics' order)."""
    torch = gpu
    N, W, H, L = scene.WORKLOADS["small"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    keys = ("image", "T", "n", "sorted", "ranges")
    plain = raster.RasterContext(N, W, H)
    fp = plain.rasterize_image(dp, dc, c, c["bg"], L)
    assert "depth" not in fp and "depth2" not in fp
    base = {k: fp[k].clone() for k in keys}
    gp = plain.alloc_gradients(fp["num_culled"], L)
    plain.backward_pass(dp, dc, gi, c["bg"], L, gp)
    maps = []
    for mode in ("train", "lean", "render_only"):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_depth(True, inverse=True, moment=True)
        if mode == "lean":
            ctx.set_lean_forward(True)
        if mode == "render_only":
            ctx.set_render_only(True)
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        for k in keys:
            assert torch.equal(f[k], base[k]), (mode, k)
        maps.append((f["depth"].clone(), f["depth2"].clone()))
        if mode == "train":
            z = torch.zeros(H, W, device="cuda")
            for kw in (dict(grad_depth2=z), dict(grad_depth=z, grad_alpha=z, grad_depth2=z)):
                g0 = ctx.alloc_gradients(f["num_culled"], L)
                ctx.backward_pass(dp, dc, gi, c["bg"], L, g0, **kw)
                torch.cuda.synchronize()
                for k in g0:
                    assert_grad_close(_np(g0[k]), _np(gp[k]), k, rel=1e-5)
    for d, q in maps[1:]:
        assert torch.equal(d, maps[0][0]) and torch.equal(q, maps[0][1])
    # set_depth(True) is set_depth_mode(0, 0)
    a, b = raster.RasterContext(N, W, H), raster.RasterContext(N, W, H)
    a.set_depth(True)
    pkg("_lib").check(b._lib.gsplat_context_set_depth_mode(b._h, 0, 0))
    b._depth = True
    fa, fb = a.rasterize_image(dp, dc, c, c["bg"], L), b.rasterize_image(dp, dc, c, c["bg"], L)
    assert "depth2" not in fa
    assert torch.equal(fa["depth"], fb["depth"])
    for k in keys:
        assert torch.equal(fa[k], fb[k]) and torch.equal(fa[k], base[k]), k
    # ... and set_depth(False) clears the options
    b.set_depth(True, inverse=True, moment=True)
    b.set_depth(False)
    b.set_depth(True)
    assert torch.equal(b.rasterize_image(dp, dc, c, c["bg"], L)["depth"], fa["depth"])


def test_long_lists_in_segments(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    N, W, H, L, params, cam = _long_list_scene(scene)
    c = scene.CONFIG
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    ctx.set_depth(True, inverse=True, moment=True)
    gi = scene.make_grad_image(W, H)
    gi_d = torch.as_tensor(gi).cuda()
    (gd, ga, gq), (gd_d, ga_d, gq_d) = _three_maps(torch, W, H)
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    dref, _, qref = dmr.maps(orc, ref, W, H, True, threads=8)
    g = dmr.backward_pass(orc, ref, cam, gi, gd, ga, gq, c["bg"], L, True, threads=8)
    seg = None
    for it in range(5):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        _check_map(fwd, "depth", ref, dref)
        _check_map(fwd, "depth2", ref, qref)
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        ctx.backward_pass(dp, dc, gi_d, c["bg"], L, grads, grad_depth=gd_d, grad_alpha=ga_d, grad_depth2=gq_d)
        torch.cuda.synchronize()
        _check_grads(grads, g)
        _check_depth_term(orc, grads, g, ref, cam, W, H)
        if it == 3:
            seg = (fwd["depth"].clone(), fwd["depth2"].clone())
        elif it == 4:
            assert torch.equal(fwd["depth"], seg[0]) and torch.equal(fwd["depth2"], seg[1])
    cnt = ctx.counters()
    assert cnt["segmented_backwards"] > 0 and cnt["segmented_forwards"] > 0, cnt
    for opts in (dict(thin_layer_blocks=0), dict(thin_layer_blocks=1 << 20), dict(poll_budget=1, thin_layer_blocks=1 << 20)):
        other = raster.RasterContext(N, W, H)
        other.set_binning_route(1)
        other.set_depth(True, inverse=True, moment=True)
        other.set_segment_options(**opts)
        for it in range(4):
            out = other.rasterize_image(dp, dc, c, c["bg"], L)
        assert other.counters()["segmented_forwards"] == 1, opts
        assert torch.equal(out["depth2"], seg[1]) and torch.equal(out["depth"], seg[0]), opts


def test_every_per_gaussian_entry_point_takes_the_moment_term(gpu, scene, orc):
    """Mode (1,1) at 5000x256x144, SH 3: ranges and the split rows are the whole call's bits, the Adam-inside struct modes
    0, 1 and 2 those of backward + the unfused step, and the xyz gradient is not the one without the Q map."""
    torch, opt_mod = gpu, pkg("optimizer")
    N, W, H, L = 5000, 256, 144, 3
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L, view=1)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True, inverse=True, moment=True)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    (gd, ga, gq), (gd_d, ga_d, gq_d) = _three_maps(torch, W, H)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    M = fwd["num_culled"]
    ctx.backward_render(gi, c["bg"], grad_depth=gd_d, grad_alpha=ga_d)
    without_q = ctx.backward_gaussians(dp, dc, L, ctx.alloc_gradients(M, L))["xyz"].clone()
    ctx.backward_render(gi, c["bg"], grad_depth=gd_d, grad_alpha=ga_d, grad_depth2=gq_d)
    whole = ctx.backward_gaussians(dp, dc, L, ctx.alloc_gradients(M, L, intermediates=("uv", "J", "xyz_c")))
    torch.cuda.synchronize()
    assert not torch.equal(whole["xyz"], without_q)
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    g = dmr.backward_pass(orc, ref, cam, scene.make_grad_image(W, H), gd, ga, gq, c["bg"], L, True, threads=8)
    _check_grads(whole, g)
    _check_depth_term(orc, whole, g, ref, cam, W, H)
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
    for mode in (0, 1, 2):
        dp_a, dp_b = {k: v.clone() for k, v in dp.items()}, {k: v.clone() for k, v in dp.items()}
        oa, ob = opt_mod.AdamOptimizer(dp_a, L, scene_extent=2.5), opt_mod.AdamOptimizer(dp_b, L, scene_extent=2.5)
        g_a = ctx.alloc_gradients(M, L, intermediates=("uv",), factored_sh=True)
        ctx.backward_gaussians(dp, dc, L, g_a)  # (dp itself is never stepped: every form differentiates the same parameters)
        oa.step(1, fwd, g_a, campos=cam["campos"])
        if mode == 1:
            g_b = ctx.alloc_gradients(M, L, intermediates=("uv",), factored_sh=True)
            ctx.backward_gaussians_adam(dp_b, dc, L, ob.fused_state(1, mode=1), g_b)
            ob.step_after_partial_backward(1, fwd, g_b, cam["campos"])
        else:
            ctx.backward_gaussians_adam(dp_b, dc, L, ob.fused_state(1, mode=mode))
        torch.cuda.synchronize()
        for k in oa.names:
            assert torch.equal(dp_a[k], dp_b[k]), (mode, k)
            assert torch.equal(oa.exp_avg[k], ob.exp_avg[k]) and torch.equal(oa.exp_avg_sq[k], ob.exp_avg_sq[k]), (mode, k)
        assert torch.equal(oa.uv_grad_accum, ob.uv_grad_accum) and torch.equal(oa.grad_accum_dur, ob.grad_accum_dur), mode


def test_refusals_leave_everything_untouched(gpu, scene):
    torch = gpu
    err = pkg("_lib").GsplatError
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    _, (gd_d, ga_d, gq_d) = _three_maps(torch, W, H)
    before = {k: v.clone() for k, v in dp.items()}

    def refused(ctx, f, kws):
        grads = ctx.alloc_gradients(f["num_culled"], L)
        for t in grads.values():
            t.fill_(7.0)
        for kw in kws:
            with pytest.raises(err) as e:
                ctx.backward_pass(dp, dc, gi, c["bg"], L, grads, **kw)
            assert e.value.code == -3, e.value  # GSPLAT_ERR_INVALID_ARG
            with pytest.raises(err):
                ctx.backward_render(gi, c["bg"], **kw)
        torch.cuda.synchronize()
        for t in grads.values():
            assert bool((t == 7.0).all())
        for k in dp:
            assert torch.equal(dp[k], before[k]), k

    # grad_depth2 / the moment map after forwards without the moment: plain, depth, inverse depth
    for setup in (None, dict(), dict(inverse=True)):
        ctx = raster.RasterContext(N, W, H)
        if setup is not None:
            ctx.set_depth(True, **setup)
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        refused(ctx, f, (dict(grad_depth2=gq_d), dict(grad_depth=gd_d, grad_alpha=ga_d, grad_depth2=gq_d)))
        with pytest.raises(err):
            pkg("_lib").check(ctx._lib.gsplat_context_depth_moment_map(ctx._h, ctypes.byref(ctypes.c_void_p())))
    # the moment option has no absgrad form
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True, inverse=True, moment=True)
    ctx.set_absgrad(True)
    f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    refused(ctx, f, (dict(grad_depth2=gq_d), dict(grad_depth=gd_d), dict(grad_depth=gd_d, grad_alpha=ga_d, grad_depth2=gq_d)))
    # ... while inverse depth alone has one: the gradients are those of the mode off
    inv = raster.RasterContext(N, W, H)
    inv.set_depth(True, inverse=True)
    f = inv.rasterize_image(dp, dc, c, c["bg"], L)
    g_off = inv.backward_pass(dp, dc, gi, c["bg"], L, inv.alloc_gradients(f["num_culled"], L), grad_depth=gd_d, grad_alpha=ga_d)
    inv.set_absgrad(True)
    g_on = inv.backward_pass(dp, dc, gi, c["bg"], L, inv.alloc_gradients(f["num_culled"], L), grad_depth=gd_d, grad_alpha=ga_d)
    torch.cuda.synchronize()
    for k in g_off:
        assert_grad_close(_np(g_on[k]), _np(g_off[k]), k, rel=1e-5)


def test_full_size_cost(gpu, scene):
    """The bar of test_depth_gpu.py::test_full_size_depth_and_cost -- a depth-mode step within 1.3x the plain step at
    config 3 -- applied to mode (1,1) with all three gradient maps, the two alternating in this process."""
    torch, raster = gpu, pkg("raster")
    N, W, H, L = scene.WORKLOADS["config3"][:4]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_workload_gaussians("config3"))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    _, (gd_d, ga_d, gq_d) = _three_maps(torch, W, H)
    plain, ctx = raster.RasterContext(N, W, H), raster.RasterContext(N, W, H)
    ctx.set_depth(True, inverse=True, moment=True)
    grads = {False: plain.alloc_gradients(N, L), True: ctx.alloc_gradients(N, L)}

    def step(moment):
        cx = ctx if moment else plain
        f = cx.rasterize_image(dp, dc, c, c["bg"], L)
        sub = {kk: (v[:f["num_culled"]] if v is not None else None) for kk, v in grads[moment].items()}
        kw = dict(grad_depth=gd_d, grad_alpha=ga_d, grad_depth2=gq_d) if moment else {}
        cx.backward_pass(dp, dc, gi, c["bg"], L, sub, **kw)
        return f

    times = {True: [], False: []}
    for rep in range(24):
        for moment in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f = step(moment)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 4:
                times[moment].append(e0.elapsed_time(e1))
    assert float(f["depth2"].max()) > 0 and bool(torch.isfinite(f["depth2"]).all())
    ratio = float(np.median(times[True]) / np.median(times[False]))
    print(f"mode (1,1) step {ratio:.3f}x the plain step at config 3")
    perf_check(ratio <= 1.3, f"(1,1)-mode step {ratio:.3f}x the plain step (bar 1.3x)")

"""GPU checks of the camera gradient (gsplat_backward_gaussians_camera, gsplat_backward_pass_camera): the fifteen values
against the float32 oracle's chain composed in float64 (tests/pose_reference.py) and against the same sums formed on the
host from the kernel's own intermediates, the bits of the per-gaussian arrays and of repeated runs, edge and full-size
scenes, and refusals."""
import ctypes

import numpy as np
import pytest

import edge_scenes as es
import pose_reference
from conftest import perf_check, pkg

pytestmark = pytest.mark.gpu
C = dict(near_thresh=0.3, mh_dist=3.0, cull_mask_padding=100, bg=0.5)


def _np(t):
    return t.detach().cpu().numpy()


def _flat(gv, gc):
    return np.concatenate([_np(gv).reshape(12), _np(gc).reshape(3)]).astype(np.float64)


def _within(got, want, mass, bar, what):
    assert np.isfinite(got).all(), f"{what}: non-finite camera gradient {got}"
    bad = np.abs(got - want) > bar * mass
    assert not bad.any(), (f"{what}: components {np.nonzero(bad)[0].tolist()} beyond {bar} of their mass: got {got[bad]}, "
                           f"want {want[bad]}, mass {mass[bad]}")


def _maps(torch, W, H, seed=3):
    rng = np.random.default_rng(seed)
    gd = (rng.uniform(-1.0, 1.0, (H, W)) / (W * H)).astype(np.float32)
    ga = (rng.uniform(-1.0, 1.0, (H, W)) / (W * H)).astype(np.float32)
    return gd, ga, torch.as_tensor(gd).cuda(), torch.as_tensor(ga).cuda()


def _setup(torch, scene, N, W, H, L, view=2, depth=False):
    raster = pkg("raster")
    params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, view)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(depth)
    return raster, params, cam, raster.device_params(params), raster.device_camera(cam), ctx


CASES = [("tiny", None), ("l0", (3000, 200, 120, 0)), ("l1", (3000, 200, 120, 1)), ("l2", (3000, 200, 120, 2)),
         ("small", None)]


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("name,shape", CASES)
def test_camera_gradient_matches_oracle(gpu, scene, orc, name, shape, depth):
    torch = gpu
    N, W, H, L = shape if shape else scene.WORKLOADS[name][:4]
    raster, params, cam, dp, dc, ctx = _setup(torch, scene, N, W, H, L, depth=depth)
    ctx.rasterize_image(dp, dc, C, C["bg"], L)
    gi = scene.make_grad_image(W, H)
    gd = ga = None
    kw = {}
    if depth:
        gd, ga, gd_d, ga_d = _maps(torch, W, H)
        kw = dict(grad_depth=gd_d, grad_alpha=ga_d)
    _, gv, gc = ctx.backward_pass_camera(dp, dc, torch.as_tensor(gi).cuda(), C["bg"], L, **kw)
    torch.cuda.synchronize()
    assert gv.shape == (3, 4) and gc.shape == (3,)
    ref = orc.rasterize(params, cam, C["near_thresh"], C["mh_dist"], C["cull_mask_padding"], C["bg"], L, threads=8)
    want, mass = pose_reference.camera_gradient(orc, ref, cam, gi, gd, ga, C["bg"], L, threads=8)
    _within(_flat(gv, gc), want, mass, 1e-3, f"{name} depth={depth}")


@pytest.mark.parametrize("depth", [False, True])
def test_reduction_matches_the_kernels_own_intermediates(gpu, scene, orc, depth):
    """The fifteen sums formed on the host in float64 from what the same kernel stored: grad_xyz_c (c), grad_J (dM =
    grad_J (R^T)^-1), the forward's J, and grad_precompute_rgb through gs::sh_bwd's arithmetic (the oracle's) for s."""
    torch = gpu
    N, W, H, L = 5000, 256, 144, 3
    raster, params, cam, dp, dc, ctx = _setup(torch, scene, N, W, H, L, view=1, depth=depth)
    fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
    M = fwd["num_culled"]
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    kw = {}
    if depth:
        _, _, gd_d, ga_d = _maps(torch, W, H)
        kw = dict(grad_depth=gd_d, grad_alpha=ga_d)
    grads = ctx.alloc_gradients(M, L, intermediates=("xyz_c", "J", "precompute_rgb"))
    _, gv, gc = ctx.backward_pass_camera(dp, dc, gi, C["bg"], L, grads=grads, **kw)
    torch.cuda.synchronize()
    c2g = _np(fwd["compact_to_global"]).astype(np.int64)
    xyz, band0, sh = params["xyz"][c2g], params["rgb"][c2g], params["sh"][c2g]
    _, _, s = orc.precompute_spherical_harmonics_backward(xyz, band0, sh, cam["campos"], _np(grads["precompute_rgb"]), L)
    t = pose_reference.terms(xyz, _np(fwd["J"]), _np(grads["xyz_c"]),
                             pose_reference.dM_from_J_grad(_np(grads["J"]), cam["view"]), s)
    _within(_flat(gv, gc), t.sum(0), np.abs(t).sum(0), 1e-5, f"depth={depth}")


@pytest.mark.parametrize("depth", [False, True])
def test_bits_of_arrays_and_repeats(gpu, scene, depth):
    """On one compositing backward: the per-gaussian arrays of the camera form are gsplat_backward_gaussians' bits, three
    camera backwards give the same camera bits, and out = NULL gives them too."""
    torch = gpu
    N, W, H, L = 5000, 256, 144, 3
    raster, params, cam, dp, dc, ctx = _setup(torch, scene, N, W, H, L, view=2, depth=depth)
    fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
    M = fwd["num_culled"]
    kw = {}
    if depth:
        _, _, gd_d, ga_d = _maps(torch, W, H)
        kw = dict(grad_depth=gd_d, grad_alpha=ga_d)
    ctx.backward_render(torch.as_tensor(scene.make_grad_image(W, H)).cuda(), C["bg"], **kw)
    plain = ctx.alloc_gradients(M, L, intermediates=True)
    ctx.backward_gaussians(dp, dc, L, plain)
    first = None
    for rep in range(3):
        grads = ctx.alloc_gradients(M, L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        _, gv, gc = ctx.backward_gaussians_camera(dp, dc, L, grads)
        torch.cuda.synchronize()
        for k in plain:
            assert torch.equal(grads[k], plain[k]), f"grad_{k} differs from gsplat_backward_gaussians"
        got = torch.cat([gv.reshape(-1), gc]).clone()
        if first is None:
            first = got
        assert torch.equal(got, first), f"repeat {rep}: camera gradient bits differ"
    _, gv, gc = ctx.backward_gaussians_camera(dp, dc, L, None)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([gv.reshape(-1), gc]), first), "out = NULL changes the camera gradient"
    assert bool(torch.isfinite(first).all()) and bool((first != 0).any())


def test_edge_scene_camera_gradient(gpu, scene, orc):
    """Clamp-band, near-plane, NaN-radius, needle and saturated populations (tests/edge_scenes.py), culled rows between."""
    torch, raster = gpu, pkg("raster")
    params, cam, pops = es.make_edge_scene("small")
    N, W, H, L = es.SIZES["small"]
    ctx = raster.RasterContext(N, W, H)
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
    assert fwd["num_culled"] < N
    gi = scene.make_grad_image(W, H)
    _, gv, gc = ctx.backward_pass_camera(dp, dc, torch.as_tensor(gi).cuda(), C["bg"], L)
    torch.cuda.synchronize()
    ref = orc.rasterize(params, cam, C["near_thresh"], C["mh_dist"], C["cull_mask_padding"], C["bg"], L, threads=16)
    g = orc.backward_pass(ref, cam, gi, C["bg"], L, threads=16, tan_fov=es.backward_tan_fov(cam))
    t = pose_reference.from_chain(orc, ref, cam, g, L)
    _within(_flat(gv, gc), t.sum(0), np.abs(t).sum(0), 1e-3, "edge scene")


def test_full_size_camera_gradient_and_cost(gpu, scene, orc, config3_case):
    torch, raster = gpu, pkg("raster")
    k = config3_case
    N, W, H, L = k["N"], k["W"], k["H"], k["L"]
    dp, dc = raster.device_params(k["params"]), raster.device_camera(k["cam"])
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
    gi = torch.as_tensor(k["gi"]).cuda()
    grads = ctx.alloc_gradients(fwd["num_culled"], L)
    _, gv, gc = ctx.backward_pass_camera(dp, dc, gi, C["bg"], L, grads=grads)
    torch.cuda.synchronize()
    t = pose_reference.from_chain(orc, k["ref"], k["cam"], k["bref"], L)
    _within(_flat(gv, gc), t.sum(0), np.abs(t).sum(0), 1e-3, "config3")
    # cost: the per-gaussian backward with and without the camera sums, alternating on one set of compositing rows
    ctx.backward_render(gi, C["bg"])
    times = {False: [], True: []}
    for rep in range(24):
        for cam_grad in (False, True):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if cam_grad:
                ctx.backward_gaussians_camera(dp, dc, L, grads)
            else:
                ctx.backward_gaussians(dp, dc, L, grads)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 4:
                times[cam_grad].append(e0.elapsed_time(e1))
    ratio = float(np.median(times[True]) / np.median(times[False]))
    # (measured 1.29-1.33x, most of it the one-workgroup sum of the rows: DESIGN.md section 4)
    perf_check(ratio <= 1.45, f"camera backward {ratio:.3f}x the plain per-gaussian backward (bar 1.45x)")


def test_bad_calls_are_refused_before_anything_runs(gpu, scene):
    torch = gpu
    _lib = pkg("_lib")
    N, W, H, L = 500, 64, 48, 1
    raster, params, cam, dp, dc, ctx = _setup(torch, scene, N, W, H, L, view=0)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    # refused before anything ran: no forward, then a forward without backward_render
    with pytest.raises(_lib.GsplatError):
        ctx.backward_gaussians_camera(dp, dc, L)
    ctx.rasterize_image(dp, dc, C, C["bg"], L)
    with pytest.raises(_lib.GsplatError):
        ctx.backward_gaussians_camera(dp, dc, L)
    ctx.backward_render(gi, C["bg"])
    g, c = ctx._structs(dp, dc, L)
    gv = torch.full((12,), 7.0, device="cuda")
    gc = torch.full((3,), 7.0, device="cuda")
    host = torch.zeros(12)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = ctx._lib.gsplat_backward_gaussians_camera
    for view_ptr, camp_ptr in ((None, gc.data_ptr()), (gv.data_ptr(), None), (host.data_ptr(), gc.data_ptr())):
        with pytest.raises(_lib.GsplatError):
            _lib.check(fn(ctx._h, ctypes.byref(g), ctypes.byref(c), L, None, view_ptr, camp_ptr, st))
    with pytest.raises(_lib.GsplatError):  # l_max other than the forward's
        _lib.check(fn(ctx._h, ctypes.byref(g), ctypes.byref(c), L + 1, None, gv.data_ptr(), gc.data_ptr(), st))
    with pytest.raises(_lib.GsplatError):
        ctx.backward_pass_camera(dp, dc, gi, C["bg"], L + 1)
    torch.cuda.synchronize()
    assert bool((gv == 7.0).all()) and bool((gc == 7.0).all()), "a refused call wrote its outputs"
    # every gaussian behind the camera: the forward itself is refused, and with it the camera backward after it
    behind = dict(dp, xyz=dp["xyz"] * torch.tensor([1.0, 1.0, -1.0], device="cuda"))
    with pytest.raises(_lib.GsplatError):
        ctx.rasterize_image(behind, dc, C, C["bg"], L)
    with pytest.raises(_lib.GsplatError):
        _lib.check(fn(ctx._h, ctypes.byref(ctx._structs(behind, dc, L)[0]), ctypes.byref(c), L, None, gv.data_ptr(),
                      gc.data_ptr(), st))
    torch.cuda.synchronize()
    assert bool((gv == 7.0).all()) and bool((gc == 7.0).all())

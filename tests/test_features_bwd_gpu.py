"""GPU tests of the feature map's gradient with respect to the geometry (gsplat_context_features_backward).

Each test runs the GPU forward, builds the float64 terms (tests/feature_bwd_reference.py) from THAT forward's record (uv,
conic, lists, stop indices and final transmittances as the GPU produced them; opacity and the leaves from the input
parameters through compact_to_global), runs backward_render with a zero image gradient, features_backward and
backward_gaussians with intermediates into NaN-filled arrays, and holds grads["opacity" | "conic" | "uv"] to
tests/grad_bound.py's bar,

    every element:  |got - value64| <= 4 K_obs u unit + borderline,

with K_obs the reference's own float32 figure for the scene (tests/test_features_bwd_cpu.py: K_OBS_FEATURES); the leaves
xyz, scale, quaternion meet conftest.assert_grad_close.  Features and gradient maps are the first C columns of one seeded
35-channel array per scene (tests/feature_bwd_cases.py).  Every figure is printed before it is asserted (pytest -s)."""
import ctypes

import numpy as np
import pytest

import antialias_reference as aar
import feature_bwd_cases as fc
import feature_bwd_reference as fbr
import feature_reference as fr
import filter3d_reference as f3
import grad_bound
import render_bwd_reference as rbr
from conftest import assert_grad_close, pkg
from test_contribution_gpu import _occlusion_scene, _training_setup
from test_features_bwd_cpu import K_OBS_FEATURES
from test_grad_bound_cpu import K_OBS

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 16, 17, 35)  # one chunk of 4, the edge of a 16-chunk, one past it, two chunks and a remainder
GROUPS = ("opacity", "conic", "uv")
LEAVES = ("xyz", "scale", "quaternion")
_TERMS = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _on_device(case, params=None):
    raster = pkg("raster")
    return raster, raster.device_params(params or case["params"]), raster.device_camera(case["cam"])


def _record(fwd, opacity):
    rec = fc.record_of({k: _np(fwd[k]).copy() for k in ("uv", "conic", "sorted", "ranges", "n", "T")}, opacity)
    return rec, _np(fwd["compact_to_global"]).astype(np.int64)


def _feature_backward(torch, ctx, case, dp, dc, fwd, feats, gmap, grad_image=None, **depth):
    """backward_render (a zero image gradient unless one is given) -> features_backward (unless feats is None) ->
    backward_gaussians with intermediates, into NaN-filled arrays; returns them as numpy."""
    H, W, L = case["H"], case["W"], case["L"]
    grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
    for t in grads.values():
        t.fill_(float("nan"))
    gi = torch.zeros(H, W, 3, device="cuda") if grad_image is None else grad_image
    ctx.backward_render(gi, 0.0, **depth)
    if feats is not None:
        ctx.features_backward(feats, gmap)
    ctx.backward_gaussians(dp, dc, L, grads)
    torch.cuda.synchronize()
    return {k: _np(v).copy() for k, v in grads.items() if v is not None}


def _hold(t, got, table, what, groups=GROUPS):
    """The compositing arrays of `got` against the terms `t`: prints every worst ratio, then fails if any broke its bar."""
    failures, line = [], []
    position = grad_bound.deepest_position(t["sorted"], t["ranges"], len(t["rows"]))
    for name in groups:
        v, u, b = t[name]
        K = grad_bound.GPU_MARGIN * table[name]
        try:
            worst = grad_bound.assert_within_bound(got[name], v, u, b, K, f"{what}: grad {name}", t["on_list"], t["rows"], position)
        except AssertionError as e:
            failures.append(str(e))
            worst = grad_bound.observed_K(got[name], v, u, b)
        line.append(f"{name} {worst:.3g}/{K:.3g}")
    print(f"[feature grad bound {what}] worst ratio / bound (u*unit): " + ", ".join(line))
    assert not failures, "\n".join(failures)


def _terms(key, case, rec, rows, C, params=None):
    """The float64 terms of a record at C channels, computed once per key (the GPU forward gives the same bits again)."""
    if key not in _TERMS:
        t = fbr.bound_terms(rec, fc.visible_leaves(case, rows, params), case["cam"], case["feats"][rows][:, :C],
                            case["gmap"][..., :C], case["L"], case["cfg"]["mh_dist"])
        t.update(rows=rows, sorted=rec["sorted"], ranges=rec["ranges"])
        _TERMS[key] = t
    return _TERMS[key]


def _cols(torch, a, C):
    return _dev(torch, a[..., :C])


def _run(torch, ctx, case, dp, dc, C, what, table, leaves=True):
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    rec, rows = _record(fwd, case["params"]["opacity"][_np(fwd["compact_to_global"]).astype(np.int64)])
    got = _feature_backward(torch, ctx, case, dp, dc, fwd, _cols(torch, case["feats"], C), _cols(torch, case["gmap"], C))
    t = _terms((case["name"], C, rec["T"].tobytes(), rec["n"].tobytes()), case, rec, rows, C)
    _hold(t, got, table, f"{what}, C = {C}")
    assert (np.abs(got["precompute_rgb"]) == 0).all(), "a zero image gradient and no colour column written"
    if leaves:
        assert_grad_close(got["opacity"].reshape(-1), t["leaf_opacity"][0].reshape(-1), f"{what}, C = {C}: leaf opacity")
        for k in LEAVES:
            assert_grad_close(got[k], t["leaf_" + k][0].reshape(got[k].shape), f"{what}, C = {C}: leaf {k}")
    return t, got


# ------------------------------------------------------------------------------------------------ a feature loss alone
@pytest.mark.parametrize("name", ["tiny", "partial"])
def test_feature_loss_alone(gpu, name):
    torch, case = gpu, fc.make(name)
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    for it in range(2):  # the second forward walks the compacted slots
        for C in (CHANNELS if it == 0 else (17,)):
            _run(torch, ctx, case, dp, dc, C, f"{name}, forward {it}", K_OBS_FEATURES[name])


@pytest.mark.parametrize("C", [4, 16])
def test_an_unaligned_gradient_map_takes_the_scalar_path(gpu, C):
    """C a multiple of 4, but grad_map starts one float past a 16-byte boundary: the kernel reads it float by float.  The
    gradients agree with the aligned call's under the bar that call meets against the reference (float atomics)."""
    torch, case = gpu, fc.make("partial")
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    t, aligned = _run(torch, ctx, case, dp, dc, C, "partial, aligned map", K_OBS_FEATURES["partial"])
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    gmap = _cols(torch, case["gmap"], C)
    offset = torch.empty(gmap.numel() + 1, device="cuda")[1:].view(gmap.shape).copy_(gmap)
    assert offset.data_ptr() % 16 == 4 and offset.is_contiguous()
    got = _feature_backward(torch, ctx, case, dp, dc, fwd, _cols(torch, case["feats"], C), offset)
    against = dict(t, **{k: (aligned[k].astype(np.float64).reshape(np.shape(t[k][0])),) + tuple(t[k][1:]) for k in GROUPS})
    _hold(against, got, K_OBS_FEATURES["partial"], f"partial, C = {C}: offset map against the aligned call")
    for k in LEAVES:
        assert_grad_close(got[k], aligned[k], f"partial, C = {C}: offset map against the aligned call, leaf {k}")


def test_feature_loss_alone_on_small(gpu):
    """5000 gaussians at 256 x 144, lists of up to 150 entries, more than one round of workgroups per chunk: C = 16."""
    torch, case = gpu, fc.make("small")
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    _run(torch, ctx, case, dp, dc, 16, "small", K_OBS_FEATURES["small"])


def test_long_lists_are_walked_whole(gpu):
    """32 x 32, a list of ~2400 entries (beyond a batch, beyond the segment threshold), binning route 1 and gate 0, at
    forwards 0 and 4 (the forward's own split follows the figures of the forward two back): the same bound."""
    torch, case = gpu, fc.make("long")
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_binning_route(1)
    ctx.set_segment_options(gate=0.0)
    for it in range(5):
        if it in (0, 4):
            t, _ = _run(torch, ctx, case, dp, dc, 4, f"long list, forward {it}", K_OBS_FEATURES["long"], leaves=False)
            assert int(np.diff(t["ranges"]).max()) > 1488
        else:
            ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    assert ctx.counters()["segmented_forwards"] > 0, ctx.counters()


# ---------------------------------------------------------------------------- the library's own backward, additivity
def _image_case(torch, scene):
    """tiny with the forward's colours as features and the image gradient as the gradient map, background 0."""
    case = fc.make("tiny")
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    rec, rows = _record(fwd, case["params"]["opacity"][_np(fwd["compact_to_global"]).astype(np.int64)])
    gi = scene.make_grad_image(case["W"], case["H"])
    rgb = torch.zeros(case["N"], 3, device="cuda")
    rgb[fwd["compact_to_global"].long()] = fwd["rgb"]
    sums = rbr.compositing_sums(dict(rec, rgb=_np(fwd["rgb"])), gi, case["W"], case["H"], 0.0, with_split=True)
    return case, ctx, dp, dc, fwd, rec, rgb, gi, sums


def test_the_librarys_own_backward_is_a_special_case(gpu, scene):
    """Features = the forward's colours in global order, gradient map = the image gradient, background 0: the six columns
    from features_backward alone and from backward_render alone are two float32 evaluations of the same sums, each within
    its own bound (4 K_obs of tiny at view 0, tests/test_grad_bound_cpu.py; 4 K_OBS_FEATURES) of the float64 value."""
    torch = gpu
    case, ctx, dp, dc, fwd, rec, rgb, gi, (_, absolute, border, split) = _image_case(torch, scene)
    a = _feature_backward(torch, ctx, case, dp, dc, fwd, rgb, _dev(torch, gi))
    b = _feature_backward(torch, ctx, case, dp, dc, fwd, None, None, grad_image=_dev(torch, gi))
    unit = absolute + split
    for name, sl in rbr.SLICES.items():
        if name not in GROUPS:
            continue
        K = grad_bound.GPU_MARGIN * (K_OBS["tiny_v0"][name] + K_OBS_FEATURES["tiny"][name])
        M = len(unit)
        d = np.abs(a[name].reshape(M, -1).astype(np.float64) - b[name].reshape(M, -1))
        lim = K * grad_bound.U * unit[:, sl] + 2 * border[:, sl]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.nanmax(np.where(d > 0, d / lim, 0)))
        print(f"[special case] {name}: worst difference / the sum of both bounds {worst:.3f}")
        assert (d <= lim).all() and (a[name] != 0).any()
    for k in LEAVES:  # (the colour columns of the image backward reach xyz through the SH bands: not compared)
        if k != "xyz":
            assert_grad_close(a[k], b[k], f"special case: leaf {k}")


def test_image_gradient_and_feature_term_add(gpu, scene):
    """backward_render(gi) + features_backward(f, G) gives the sum of the two separate runs: each of the three runs is
    within its own bounds of the float64 value, so the difference is within twice the sum of both."""
    torch = gpu
    case, ctx, dp, dc, fwd, rec, _, gi, (_, absolute, border, split) = _image_case(torch, scene)
    C = 17
    feats, gmap = _cols(torch, case["feats"], C), _cols(torch, case["gmap"], C)
    rows = _np(fwd["compact_to_global"]).astype(np.int64)
    t = _terms((case["name"], C, rec["T"].tobytes(), rec["n"].tobytes()), case, rec, rows, C)
    both = _feature_backward(torch, ctx, case, dp, dc, fwd, feats, gmap, grad_image=_dev(torch, gi))
    image = _feature_backward(torch, ctx, case, dp, dc, fwd, None, None, grad_image=_dev(torch, gi))
    feat = _feature_backward(torch, ctx, case, dp, dc, fwd, feats, gmap)
    unit_i = absolute + split
    M = len(unit_i)
    for name, sl in rbr.SLICES.items():
        if name not in GROUPS:
            continue
        lim = 2 * (grad_bound.GPU_MARGIN * grad_bound.U * (K_OBS["tiny_v0"][name] * unit_i[:, sl] + K_OBS_FEATURES["tiny"][name] * t[name][1])
                   + border[:, sl] + t[name][2])
        d = np.abs(both[name].reshape(M, -1).astype(np.float64) - (image[name].reshape(M, -1).astype(np.float64) + feat[name].reshape(M, -1)))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = float(np.nanmax(np.where(d > 0, d / lim, 0)))
        print(f"[additivity] {name}: worst difference / bound {worst:.3f}")
        assert (d <= lim).all()
        assert not np.array_equal(both[name], image[name]) and not np.array_equal(both[name], feat[name])
    for k in LEAVES + ("opacity",):
        assert_grad_close(both[k], image[k].astype(np.float64) + feat[k], f"additivity: leaf {k}")
    # calling it twice adds twice
    grads = ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True)
    ctx.backward_render(torch.zeros(case["H"], case["W"], 3, device="cuda"), 0.0)
    ctx.features_backward(feats, gmap)
    ctx.features_backward(feats, gmap)
    ctx.backward_gaussians(dp, dc, case["L"], grads)
    for k in GROUPS:
        assert_grad_close(_np(grads[k]), 2.0 * feat[k].astype(np.float64), f"two calls: {k}")
    # backward_pass(feature_grads=...) is the same sequence
    grads2 = ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True)
    ctx.backward_pass(dp, dc, _dev(torch, gi), 0.0, case["L"], grads2, feature_grads=(feats, gmap))
    for k in GROUPS + LEAVES:
        assert_grad_close(_np(grads2[k]), both[k], f"backward_pass(feature_grads): {k}")


def test_a_zero_gradient_map_changes_nothing(gpu, scene):
    """The per-gaussian call's outputs before and after features_backward of a zero map, on the same rows: bit for bit."""
    torch, case = gpu, fc.make("partial")
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    gi = _dev(torch, scene.make_grad_image(case["W"], case["H"]))
    ctx.backward_render(gi, 0.0)
    before = ctx.backward_gaussians(dp, dc, case["L"], ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True))
    for C in (3, 17):
        ctx.features_backward(_cols(torch, case["feats"], C), torch.zeros(case["H"], case["W"], C, device="cuda"))
    after = ctx.backward_gaussians(dp, dc, case["L"], ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert bool((before["uv"] != 0).any())


def test_occluded_gaussians_get_nothing(gpu, scene):
    torch, raster = gpu, pkg("raster")
    N, W, H, walls, params, cam = _occlusion_scene(scene)
    case = dict(name="occlusion", N=N, W=W, H=H, L=0, params=params, cam=cam, cfg=dict(scene.CONFIG))
    ctx = raster.RasterContext(N, W, H)
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, 0)
    stop = int(fwd["n"].max())
    assert 2 <= stop < walls and fwd["num_culled"] == N
    C = 17
    feats, gmap = _dev(torch, fr.seeded_rows(N, C, 21)), _dev(torch, fr.seeded_rows(H * W, C, 22).reshape(H, W, C))
    got = _feature_backward(torch, ctx, case, dp, dc, fwd, feats, gmap)
    c2g = _np(fwd["compact_to_global"])
    hidden = c2g >= stop  # (the walls are the first gaussians, nearest first)
    assert hidden.sum() >= 100
    for k in GROUPS:  # (the walls themselves: sigmoid(20) is 1 in float32, no gradient either)
        assert (got[k].reshape(N, -1)[hidden] == 0).all(), k
    # ... while the same gaussians with the walls made faint do get a gradient
    faint = dict(params, opacity=params["opacity"].copy())
    faint["opacity"][:walls] = -3.0
    dpf = raster.device_params(faint)
    fwd = ctx.rasterize_image(dpf, dc, scene.CONFIG, 0.0, 0)
    got = _feature_backward(torch, ctx, case, dpf, dc, fwd, feats, gmap)
    assert (got["uv"].reshape(fwd["num_culled"], -1)[_np(fwd["compact_to_global"]) >= stop] != 0).any()


# ------------------------------------------------------------------------------------------------------------ modes
def test_antialiased_forward(gpu, orc):
    """The record carries the effective logit logit(sigmoid(logit) rho) the forward composited; the leaves follow through
    the compensation's chain (tests/antialias_reference.py: backward with the feature term's gradients as its base)."""
    torch, case = gpu, fc.make("small")
    raster, dp, dc = _on_device(case)
    C = 16
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_antialiased(True)
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    rows = _np(fwd["compact_to_global"]).astype(np.int64)
    p = case["params"]
    aa = dict(J=_np(fwd["J"]), sigma=_np(fwd["sigma"]), xyz_c=_np(fwd["xyz_c"]), xyz=p["xyz"][rows], scale=p["scale"][rows],
              quaternion=p["quaternion"][rows], logit=p["opacity"][rows].astype(np.float32))
    aa["rho"] = aar.compensation(aa["J"], aa["sigma"], case["cam"]["view"])
    rec, _ = _record(fwd, aar.effective_logit(aa["logit"], aa["rho"]))
    got = _feature_backward(torch, ctx, case, dp, dc, fwd, _cols(torch, case["feats"], C), _cols(torch, case["gmap"], C))
    t = _terms(("small aa", C), case, rec, rows, C)
    _hold(t, got, K_OBS_FEATURES["small"], "antialiased", groups=("conic", "uv"))
    M = len(rows)
    base = dict(opacity=t["opacity"][0], J=np.zeros((M, 6)), sigma=np.zeros((M, 6)), xyz_c=np.zeros((M, 3)),
                **{k: t["leaf_" + k][0] for k in LEAVES})
    want = aar.backward(orc, aa, case["cam"], None, 0.0, case["L"], base=lambda _: base, sigma_dtype=np.float32)
    for k in LEAVES + ("opacity",):
        assert_grad_close(got[k].reshape(M, -1), np.asarray(want[k]).reshape(M, -1), f"antialiased: leaf {k}")
    assert (np.abs(aa["rho"] - 1) > 1e-2).any(), "rho changes nothing here"


def test_filtered_forward(gpu):
    """3D filter with a random f: the terms of the filtered scale and opacity, then the filter's chain rule
    (tests/filter3d_reference.py: apply_backward) to the leaves."""
    torch, case = gpu, fc.make("small")
    N, C = case["N"], 16
    p = case["params"]
    f = np.exp(np.random.default_rng(5).uniform(-1.0, 1.0, N) + p["scale"].mean(1)).astype(np.float32)
    scale_eff, op_eff, _, _ = f3.apply(p["scale"], p["opacity"], f)
    filtered = dict(p, scale=scale_eff.astype(np.float32), opacity=op_eff.astype(np.float32))
    raster, dp, dc = _on_device(case)
    ctx = raster.RasterContext(N, case["W"], case["H"])
    ctx.set_filter3d(_dev(torch, f))
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    rows = _np(fwd["compact_to_global"]).astype(np.int64)
    rec, _ = _record(fwd, filtered["opacity"][rows])
    got = _feature_backward(torch, ctx, case, dp, dc, fwd, _cols(torch, case["feats"], C), _cols(torch, case["gmap"], C))
    t = _terms(("small filter3d", C), case, rec, rows, C, params=filtered)
    _hold(t, got, K_OBS_FEATURES["small"], "filter3d", groups=("conic", "uv"))
    g_scale, g_opacity = f3.apply_backward(p["scale"][rows], p["opacity"][rows], f[rows], t["leaf_scale"][0],
                                           t["leaf_opacity"][0].reshape(-1))
    assert_grad_close(got["scale"], np.asarray(g_scale).reshape(got["scale"].shape), "filter3d: leaf scale")
    assert_grad_close(got["opacity"].reshape(-1), np.asarray(g_opacity).reshape(-1), "filter3d: leaf opacity")
    for k in ("xyz", "quaternion"):
        assert_grad_close(got[k], t["leaf_" + k][0].reshape(got[k].shape), f"filter3d: leaf {k}")


def test_depth_mode_keeps_its_column(gpu, scene):
    """A depth-mode backward with grad_depth, then the feature term: dL/dz (row column 9) is not touched, so the
    camera-space position gradient is the sum of the depth run's and the feature run's."""
    import grad_bound_cases as gc
    torch, case = gpu, fc.make("tiny")
    raster, dp, dc = _on_device(case)
    C = 17
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_depth(True)
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, case["L"])
    gd, _ = gc.depth_maps(case["W"], case["H"])
    feats, gmap = _cols(torch, case["feats"], C), _cols(torch, case["gmap"], C)
    depth = dict(grad_depth=_dev(torch, gd))
    both = _feature_backward(torch, ctx, case, dp, dc, fwd, feats, gmap, **depth)
    only_depth = _feature_backward(torch, ctx, case, dp, dc, fwd, None, None, **depth)
    only_feat = _feature_backward(torch, ctx, case, dp, dc, fwd, feats, gmap)
    assert (only_depth["xyz_c"][:, 2] != 0).any() and (only_feat["uv"] != 0).any()
    for k in ("xyz_c", "xyz") + GROUPS:
        assert_grad_close(both[k], only_depth[k].astype(np.float64) + only_feat[k], f"depth mode: {k}")
    # (xyz_c's third column is dL/dz plus the uv / conic chain's share: additive only if column 9 was left alone)


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(gpu, scene):
    torch, lib, raster = gpu, pkg("_lib"), pkg("raster")
    case = fc.make("tiny")
    N, W, H, L, C = case["N"], case["W"], case["H"], case["L"], 3
    _, dp, dc = _on_device(case)
    feats, gmap = torch.full((N, C), 7.0, device="cuda"), torch.full((H, W, C), 7.0, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    gi = _dev(torch, scene.make_grad_image(W, H))

    def refused(ctx, n=N, ch=C, features=ptr(feats), grad_map=ptr(gmap), handle=True):
        h = ctx._h if handle else None
        assert ctx._lib.gsplat_context_features_backward(h, n, ch, features, grad_map, st) == -3  # GSPLAT_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert bool((feats == 7).all()) and bool((gmap == 7).all())

    ctx = raster.RasterContext(N, W, H)
    refused(ctx)                                     # no forward yet
    with pytest.raises(lib.GsplatError):
        ctx.features_backward(feats, gmap)
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, L)
    refused(ctx)                                     # no compositing backward since the forward
    ctx.backward_render(gi, 0.0)
    want = ctx.backward_gaussians(dp, dc, L, ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True))
    refused(ctx, handle=False)
    refused(ctx, n=N - 1)
    refused(ctx, ch=0)
    refused(ctx, ch=513)
    refused(ctx, features=None)
    refused(ctx, grad_map=None)
    host = np.full((H, W, C), 7.0, np.float32)       # not a device pointer
    refused(ctx, grad_map=ctypes.c_void_p(host.ctypes.data))
    refused(ctx, features=ctypes.c_void_p(host.ctypes.data))
    for bad in (feats.double(), feats[:, 0], torch.zeros(N, 2 * C, device="cuda")[:, ::2], feats.cpu(),
                torch.zeros(N, 0, device="cuda"), torch.zeros(N, 513, device="cuda")):
        with pytest.raises(ValueError):
            ctx.features_backward(bad, gmap)
    for bad in (gmap.double(), gmap[..., 0], torch.zeros(H, W + 1, C, device="cuda"), torch.zeros(H, W, C + 1, device="cuda"),
                gmap.cpu()):
        with pytest.raises(ValueError):
            ctx.features_backward(feats, bad)
    with pytest.raises(lib.GsplatError):
        ctx.features_backward(feats[: N - 1].contiguous(), gmap)
    # the rows are as the compositing backward left them
    after = ctx.backward_gaussians(dp, dc, L, ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True))
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(v, after[k]), k
    # a new forward: the rows belong to the forward before it
    ctx.rasterize_image(dp, dc, case["cfg"], 0.0, L)
    refused(ctx)
    ctx.backward_render(gi, 0.0)
    ctx.features_backward(feats, gmap)               # ... and now it is accepted
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], 0.0, L)
    ctx.backward_render(gi, 0.0)
    owned = [fwd[k].data_ptr() for k in ("mask", "uv_all", "xyz_c_all", "sigma", "conic", "J", "rgb", "radius", "sorted",
                                         "ranges", "image", "T", "n")]
    lib.check(ctx._lib.gsplat_context_detach_forward_outputs(ctx._h))
    refused(ctx)                                     # the forward's arrays are the caller's now
    for p in owned:
        lib.check(ctx._lib.gsplat_pool_free(ctypes.c_void_p(p)))


# ---------------------------------------------------------------------------------------------------------- Trainer
def test_trainer_feature_gradients(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    t.train(2, loss_every=0)
    n, ctx, cam = t.num_gaussians, t.ctx, views[1][0]
    H, W, C = int(cam["height"]), int(cam["width"]), 5
    feats = _dev(torch, fr.seeded_rows(n, C, 31))
    target = _dev(torch, fr.seeded_rows(H * W, C, 32).reshape(H, W, C))
    seen = {}

    def grad_fn(fmap):
        seen["fmap"] = fmap.clone()
        return (fmap - target) / (H * W)

    it, before = t.iter, {k: p.clone() for k, p in t.params.items()}
    o = t.opt
    state = lambda: list(o.exp_avg.values()) + list(o.exp_avg_sq.values()) + [o.uv_grad_accum, o.grad_accum_dur]
    kept = [x.clone() for x in state()]
    out = t.feature_gradients(cam, feats, grad_fn)
    torch.cuda.synchronize()
    assert t.iter == it and all(torch.equal(p, before[k]) for k, p in t.params.items())
    assert all(torch.equal(x, y) for x, y in zip(state(), kept))
    assert out["xyz"].shape == (n, 3) and out["opacity"].shape == (n,) and out["scale"].shape == (n, 3)
    assert out["quaternion"].shape == (n, 4) and out["features"].shape == (n, C)
    # the RasterContext sequence on the same state
    p = dict(t.params)
    fwd = ctx.rasterize_image(p, cam, t.cfg, 0.0, t.l_max)
    assert torch.equal(ctx.render_features(feats), seen["fmap"])
    gmap = (seen["fmap"] - target) / (H * W)
    grads = ctx.alloc_gradients(fwd["num_culled"], t.l_max)
    ctx.backward_render(torch.zeros(H, W, 3, device="cuda"), 0.0)
    ctx.features_backward(feats, gmap)
    ctx.backward_gaussians(p, cam, t.l_max, grads)
    c2g = fwd["compact_to_global"].long()
    culled = torch.ones(n, dtype=torch.bool, device="cuda")
    culled[c2g] = False
    for k in ("xyz", "opacity", "scale", "quaternion"):
        # (two runs of the same float atomics in another order)
        assert_grad_close(_np(out[k][c2g]), _np(grads[k]).reshape(_np(out[k][c2g]).shape), f"feature_gradients: {k}")
        assert bool((out[k][culled] == 0).all()) and bool((out[k] != 0).any()), k
    assert_grad_close(_np(out["features"]), _np(ctx.lift_features(gmap, torch.zeros(n, C, device="cuda"))),
                      "feature_gradients: features")
    with pytest.raises(ValueError):
        t.feature_gradients(cam, feats[:-1], grad_fn)
    t.train(4, loss_every=0)  # the loop still trains
    torch.cuda.synchronize()
    assert t.iter == it + 4 and all(bool(torch.isfinite(q).all()) for q in t.params.values())

"""GPU tests of the feature maps (gsplat_context_render_features, gsplat_context_lift_features): parity of both sides
with the numpy reference evaluated in float64 on the float32 oracle forward (tests/feature_reference.py), the library's
own forward and weight_sum as special cases, the adjoint identity on the device, reproducibility, accumulation, every
kind of forward, occlusion, long lists, the refusals, and the Trainer's render_features / lift_maps.

Features and maps are columns of ONE seeded 35-channel array per scene (uniform in [0,1], every second channel's sign
flipped): the C-channel case is its first C columns, so the reference is computed once per scene, at C = 35."""
import ctypes

import numpy as np
import pytest

import antialias_reference as aar
import feature_reference as fr
import filter3d_reference as f3
from conftest import (FLIP_MAX, PIXEL_L1_TOL, assert_grad_close, max_pixels_above_tol, max_stop_index_mismatches, pkg)
from test_contribution_gpu import _long_list_scene, _occlusion_scene, _training_setup

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 16, 17, 35)  # one chunk of 4, the edge of a 16-chunk, one past it, two chunks and a remainder
CMAX = max(CHANNELS)


def _np(t):
    return t.detach().cpu().numpy()


def _oracle(orc, scene, params, cam, L, bg=0.0):
    c = scene.CONFIG
    return orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], bg, L, threads=8)


def _reference(ref, W, H, N, channels=CMAX, condition=False):
    """Seeded features [N,C] (global order) and map [H,W,C], and the reference of both sides on the oracle forward
    `ref`, in global order."""
    c2g = np.nonzero(np.asarray(ref["mask"]))[0]
    feats = fr.seeded_rows(N, channels, 21)
    fmap = fr.seeded_rows(H * W, channels, 22).reshape(H, W, channels)
    r = fr.feature_maps(ref, W, H, features=feats[c2g], fmap=fmap, condition=condition)
    culled = np.ones(N, bool)
    culled[c2g] = False
    return dict(feats=feats, fmap=fmap, c2g=c2g, culled=culled, out=r["out"], lifted=fr.to_global(r["lifted"], c2g, N),
                out_abs=r["out_abs"], pixels=fr.to_global(r["pixels"], c2g, N, fill=0))


_REF = {}


def _shared(scene, orc, name):
    if name not in _REF:
        if name == "partial":  # 70 x 45: partial tiles in both directions
            N, W, H, L = 300, 70, 45, 1
        else:
            N, W, H, L = scene.WORKLOADS[name][:4]
        params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
        ref = _oracle(orc, scene, params, cam, L)
        _REF[name] = dict(N=N, W=W, H=H, L=L, params=params, cam=cam, ref=ref,
                          **_reference(ref, W, H, N, condition=(name == "tiny")))
    return _REF[name]


def _on_device(case):
    raster = pkg("raster")
    return raster, raster.device_params(case["params"]), raster.device_camera(case["cam"])


def _cols(torch, a, C):
    """The first C columns of a numpy [.., CMAX] array as a contiguous device tensor."""
    return torch.as_tensor(np.ascontiguousarray(a[..., :C])).cuda()


def _check_map(got, want, what):
    """Per channel, the project's pixel bar: within PIXEL_L1_TOL on all but the pixels a borderline 1/255 or stop
    decision may move, and those below FLIP_MAX."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    P = got.shape[0] * got.shape[1]
    allowed = max_pixels_above_tol(P) + max_stop_index_mismatches(P)
    err = np.abs(got - want)
    above = (err > PIXEL_L1_TOL).reshape(P, -1).sum(0)
    print(f"{what}: largest error {err.max():.2e}, pixels above {PIXEL_L1_TOL} per channel at most {int(above.max())} (allowed {allowed})")
    assert (above <= allowed).all(), f"{what}: {above.tolist()} pixels above {PIXEL_L1_TOL}"
    assert err.max() < FLIP_MAX, f"{what}: largest error {err.max():.3e}"


def _check_lifted(got, want, culled, what, fill=7.0):
    """got: lifted INTO an array filled with `fill`.  Culled rows keep the fill; the others meet the bar of weight_sum."""
    got = np.asarray(got, np.float64)
    assert (got[culled] == fill).all(), f"{what}: a culled row was written"
    for c in range(got.shape[1]):
        assert_grad_close(got[~culled, c] - fill, want[~culled, c], f"{what}: lifted, channel {c}")


def _both_sides(torch, ctx, case, C, what):
    N = case["N"]
    out = ctx.render_features(_cols(torch, case["feats"], C))
    lifted = ctx.lift_features(_cols(torch, case["fmap"], C), torch.full((N, C), 7.0, device="cuda"))
    torch.cuda.synchronize()
    _check_map(_np(out), case["out"][..., :C], f"{what}, C = {C}")
    _check_lifted(_np(lifted), case["lifted"][:, :C], case["culled"], f"{what}, C = {C}")
    return out


@pytest.mark.parametrize("name", ["tiny", "partial", "small"])
def test_both_sides_match_the_reference(gpu, scene, orc, name):
    torch, case = gpu, _shared(scene, orc, name)
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    for it in range(2):  # the second forward walks the compacted slots
        ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
        for C in (CHANNELS if it == 0 else (17,)):
            _both_sides(torch, ctx, case, C, f"{name}, forward {it}")
    if name == "small":
        assert int(np.diff(case["ref"]["ranges"]).max()) == 150


@pytest.mark.parametrize("C", [4, 16])
def test_unaligned_maps_take_the_scalar_path(gpu, scene, orc, C):
    """C a multiple of 4, but the [H,W,C] array starts one float past a 16-byte boundary: float-by-float accesses.  The
    rendered map is order-fixed, so it equals the aligned call bit for bit; the lifted sums (float atomics) agree with
    the aligned call's under the bar those meet against the reference."""
    torch, case = gpu, _shared(scene, orc, "partial")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    aligned = _both_sides(torch, ctx, case, C, "partial, aligned")

    def offset_like(t):
        v = torch.full((t.numel() + 1,), 7.0, device="cuda")[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    into = offset_like(aligned)
    assert ctx.render_features(_cols(torch, case["feats"], C), out=into) is into and torch.equal(into, aligned)
    fmap = _cols(torch, case["fmap"], C)
    want = ctx.lift_features(fmap, torch.zeros(N, C, device="cuda"))
    got = ctx.lift_features(offset_like(fmap).copy_(fmap), torch.zeros(N, C, device="cuda"))
    torch.cuda.synchronize()
    _check_lifted(_np(got), _np(want).astype(np.float64), case["culled"], f"partial, C = {C}: offset map against the aligned call", fill=0.0)


def test_long_lists_are_walked_whole(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    N, W, H, L, params, cam = _long_list_scene(scene)
    ref = _oracle(orc, scene, params, cam, L)
    # on the oracle first: a list beyond a 248-entry batch and beyond the forward's segment threshold, pixels that walk it
    # to the end and pixels that stop early
    assert int(np.diff(ref["ranges"]).max()) > 1488 > 248 and int(np.asarray(ref["n"]).max()) > 1488
    assert int((np.asarray(ref["n"])[:16, :16] < ref["ranges"][1]).sum()) > 0
    case = dict(N=N, **_reference(ref, W, H, N, channels=17))
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    ctx.set_segment_options(gate=0.0)
    for it in range(5):  # (the forward's own split follows the figures of the forward two back)
        ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
        if it in (0, 4):
            _both_sides(torch, ctx, case, 17, f"long list, forward {it}")
    assert ctx.counters()["segmented_forwards"] > 0, ctx.counters()


def test_the_forwards_own_image_and_weight_sum_are_special_cases(gpu, scene, orc):
    """No oracle: render_features of the forward's colours is the forward's image at background 0 -- the same fma chain
    in the same order; the bound allows the rounding of n additions of a sum within (1 - T) max|rgb| --, and
    lift_features of a map of ones is weight_sum: the same non-negative terms added in another order, each order within
    pixels * 2^-24 of the exact sum."""
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    assert int(np.diff(_np(fwd["ranges"])).max()) <= 1488
    rgb = torch.zeros(N, 3, device="cuda")
    rgb[fwd["compact_to_global"].long()] = fwd["rgb"]
    got = _np(ctx.render_features(rgb)).astype(np.float64)
    n, T = _np(fwd["n"]).astype(np.float64), _np(fwd["T"]).astype(np.float64)
    bound = n * 2.0 ** -23 * (1.0 - T) * float(fwd["rgb"].abs().max())
    err = np.abs(got - _np(fwd["image"]).astype(np.float64))
    worst = float((err / np.maximum(bound, 1e-300)[:, :, None])[bound > 0].max())
    print(f"small: render_features(rgb) against the forward's image: largest error {err.max():.2e}, worst error / bound {worst:.3f}")
    assert (err <= bound[:, :, None]).all() and (got != 0).any()
    stats = dict(weight_sum=torch.zeros(N, device="cuda"), pixels=torch.zeros(N, dtype=torch.int32, device="cuda"))
    ctx.accumulate_contributions(**stats)
    lifted = ctx.lift_features(torch.ones(H, W, 1, device="cuda"), torch.zeros(N, 1, device="cuda"))
    ws, px = _np(stats["weight_sum"]).astype(np.float64), _np(stats["pixels"]).astype(np.float64)
    d = np.abs(_np(lifted)[:, 0].astype(np.float64) - ws)
    lim = 2.0 * px * 2.0 ** -24 * ws
    print(f"small: lift_features(ones) against weight_sum: worst error / bound {float((d / np.maximum(lim, 1e-300))[lim > 0].max()):.3f}")
    assert (d <= lim).all() and (ws > 0).any()


def test_adjoint_identity_on_the_device(gpu, scene, orc):
    """<F f, g> = <f, Ft g>: both sides weigh with the same float32 w, bit for bit, so what separates them is the
    rounding of the sums -- at most n(p) additions per pixel on the left, pixels[j] per gaussian on the right, each within
    2^-24 of a partial sum that the condition sum bounds."""
    torch, case = gpu, _shared(scene, orc, "tiny")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    px = torch.zeros(N, dtype=torch.int32, device="cuda")
    ctx.accumulate_contributions(pixels=px)
    n_max, px_max = int(fwd["n"].max()), int(px.max())
    for C in CHANNELS:
        f, g = case["feats"][:, :C].astype(np.float64), case["fmap"][..., :C].astype(np.float64)
        out = _np(ctx.render_features(_cols(torch, case["feats"], C))).astype(np.float64)
        lifted = _np(ctx.lift_features(_cols(torch, case["fmap"], C), torch.zeros(N, C, device="cuda"))).astype(np.float64)
        lhs, rhs = (out * g).sum(), (f * lifted).sum()
        scale = (case["out_abs"][..., :C] * np.abs(g)).sum()
        lim = (n_max + px_max) * 2.0 ** -23 * scale
        print(f"tiny, C = {C}: <F f, g> = {lhs:.9e}, <f, Ft g> = {rhs:.9e}, difference / bound {abs(lhs - rhs) / lim:.3f}")
        assert scale > 0 and abs(lhs - rhs) <= lim


def test_the_map_carries_the_same_bits_in_every_run_route_width_and_kind_of_forward(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.rasterize_image(dp, dc, c, 0.0, L)
    wide = ctx.render_features(_cols(torch, case["feats"], CMAX))
    for _ in range(2):
        assert torch.equal(ctx.render_features(_cols(torch, case["feats"], CMAX)), wide)
    for C in CHANNELS[:-1]:  # every channel at every width: channel 2 of C = 35 is channel 2 of C = 3
        assert torch.equal(ctx.render_features(_cols(torch, case["feats"], C)), wide[..., :C]), C
    into = torch.full((H, W, 17), 7.0, device="cuda")
    assert ctx.render_features(_cols(torch, case["feats"], 17), out=into) is into and torch.equal(into, wide[..., :17])
    for route in (1, 2):
        other = raster.RasterContext(N, W, H)
        other.set_binning_route(route)
        other.rasterize_image(dp, dc, c, 0.0, L)
        assert torch.equal(other.render_features(_cols(torch, case["feats"], CMAX)), wide), route
    for kind in ("render_only", "lean", "depth"):
        other = raster.RasterContext(N, W, H)
        {"lean": other.set_lean_forward, "render_only": other.set_render_only, "depth": other.set_depth}[kind](True)
        other.rasterize_image(dp, dc, c, 0.0, L)
        assert torch.equal(other.render_features(_cols(torch, case["feats"], CMAX)), wide), kind
        lifted = other.lift_features(_cols(torch, case["fmap"], 17), torch.full((N, 17), 7.0, device="cuda"))
        _check_lifted(_np(lifted), case["lifted"][:, :17], case["culled"], kind)


def test_accumulation_over_calls_and_views_and_a_backward_behind(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    C = 17
    fmap = _cols(torch, case["fmap"], C)
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    once = ctx.lift_features(fmap, torch.zeros(N, C, device="cuda"))
    twice = ctx.lift_features(fmap, once.clone())
    assert_grad_close(_np(twice), 2.0 * _np(once).astype(np.float64), "two calls", rel=1e-6)
    # a backward behind both calls is the backward of a context that never made them, and both still work behind it
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    grads = ctx.backward_pass(dp, dc, gi, 0.0, L, ctx.alloc_gradients(fwd["num_culled"], L))
    plain = raster.RasterContext(N, W, H)
    pf = plain.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    want = plain.backward_pass(dp, dc, gi, 0.0, L, plain.alloc_gradients(pf["num_culled"], L))
    for k in ("xyz", "opacity", "scale", "quaternion", "rgb"):
        assert_grad_close(_np(grads[k]), _np(want[k]), f"backward behind the feature calls: {k}")
    assert_grad_close(_np(ctx.lift_features(fmap, torch.zeros(N, C, device="cuda"))), _np(once), "behind the backward", rel=1e-6)
    _check_map(_np(ctx.render_features(_cols(torch, case["feats"], C))), case["out"][..., :C], "behind the backward")
    # views 0 and 1 into one array
    ctx.rasterize_image(dp, raster.device_camera(scene.make_camera(W, H, 1)), scene.CONFIG, 0.0, L)
    one = ctx.lift_features(fmap, torch.zeros(N, C, device="cuda"))
    both = ctx.lift_features(fmap, once.clone())
    torch.cuda.synchronize()
    assert not torch.equal(one, once)
    assert_grad_close(_np(both), _np(once).astype(np.float64) + _np(one), "two views", rel=1e-6)


def test_antialiased_and_filtered_forwards_weigh_the_effective_opacity(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    c, C = scene.CONFIG, 17
    # anti-aliased: the oracle forward with logit(sigmoid(logit) * rho) composited
    _, aa = aar.forward(orc, case["params"], case["cam"], c, 0.0, L, threads=8)
    want = dict(N=N, **_reference(aa, W, H, N, channels=C))
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)
    ctx.rasterize_image(dp, dc, c, 0.0, L)
    _both_sides(torch, ctx, want, C, "antialiased")
    assert np.abs(want["out"] - case["out"][..., :C]).max() > 100 * PIXEL_L1_TOL, "rho changes nothing here"
    # 3D filter with a random f: the oracle forward of the filtered scale and opacity
    f = np.exp(np.random.default_rng(5).uniform(-1.0, 1.0, N) + case["params"]["scale"].mean(1)).astype(np.float32)
    scale_eff, op_eff, _, _ = f3.apply(case["params"]["scale"], case["params"]["opacity"], f)
    filtered = dict(case["params"], scale=scale_eff.astype(np.float32), opacity=op_eff.astype(np.float32))
    want3 = dict(N=N, **_reference(_oracle(orc, scene, filtered, case["cam"], L), W, H, N, channels=C))
    ctx = raster.RasterContext(N, W, H)
    ctx.set_filter3d(torch.as_tensor(f).cuda())
    ctx.rasterize_image(dp, dc, c, 0.0, L)
    _both_sides(torch, ctx, want3, C, "filter3d")
    assert np.abs(want3["out"] - case["out"][..., :C]).max() > 100 * PIXEL_L1_TOL, "the filter changes nothing here"


def test_occluded_gaussians_lift_nothing_and_colour_nothing(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    N, W, H, walls, params, cam = _occlusion_scene(scene)
    ref = _oracle(orc, scene, params, cam, 0)
    n = np.asarray(ref["n"])
    assert ref["num_culled"] == N and len(np.unique(ref["sorted"])) == N
    assert n.min() >= 2 and n.max() < walls, (n.min(), n.max())
    stop, C = int(n.max()), 17
    case = dict(N=N, **_reference(ref, W, H, N, channels=C))
    assert (case["pixels"][:stop] > 0).all() and (case["pixels"][stop:] == 0).all()
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(raster.device_params(params), raster.device_camera(cam), scene.CONFIG, 0.0, 0)
    assert int(fwd["n"].max()) == stop
    out = _both_sides(torch, ctx, case, C, "occlusion")
    lifted = ctx.lift_features(_cols(torch, case["fmap"], C), torch.zeros(N, C, device="cuda"))
    assert bool((lifted[stop:] == 0).all()) and bool((lifted[:stop] != 0).all())
    hidden = _cols(torch, case["feats"], C)
    hidden[stop:] = 1e6 * (1.0 + hidden[stop:])  # whatever sits behind the stop ...
    assert torch.equal(ctx.render_features(hidden), out)  # ... changes no bit of the map


def test_refusals_launch_nothing(gpu, scene):
    torch, lib, raster = gpu, pkg("_lib"), pkg("raster")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    c, C = scene.CONFIG, 3
    dp = raster.device_params(scene.make_gaussians(N, W, H, L))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    feats, fmap = torch.full((N, C), 7.0, device="cuda"), torch.full((H, W, C), 7.0, device="cuda")
    out, lifted = torch.full((H, W, C), 7.0, device="cuda"), torch.full((N, C), 7.0, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def refused(ctx, n=N, ch=C, null=None, code=-3):
        """Both entry points, raw: the status, and every array as it was."""
        a = dict(features=ptr(feats), out=ptr(out), map=ptr(fmap), lifted=ptr(lifted))
        if null:
            a[null] = None
        if null in (None, "features", "out"):
            assert ctx._lib.gsplat_context_render_features(ctx._h, n, ch, a["features"], a["out"], st) == code
        if null in (None, "map", "lifted"):
            assert ctx._lib.gsplat_context_lift_features(ctx._h, n, ch, a["map"], a["lifted"], st) == code
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in (feats, fmap, out, lifted))

    ctx = raster.RasterContext(N, W, H)
    refused(ctx)                                     # no forward yet
    with pytest.raises(lib.GsplatError):
        ctx.render_features(feats)
    with pytest.raises(lib.GsplatError):
        ctx.lift_features(fmap, lifted)
    fwd = ctx.rasterize_image(dp, dc, c, 0.0, L)
    refused(ctx, n=N - 1)                            # not the recorded forward's N
    refused(ctx, ch=0)
    refused(ctx, ch=513)
    for name in ("features", "out", "map", "lifted"):
        refused(ctx, null=name, code=-1)             # GSPLAT_ERR_NULL_POINTER
    with pytest.raises(lib.GsplatError):
        ctx.render_features(feats[: N - 1].contiguous())
    with pytest.raises(lib.GsplatError):
        ctx.lift_features(fmap, lifted[: N - 1].contiguous())
    # wrong dtype, shape, stride or device never reach the library
    for bad in (feats.double(), feats[:, 0], feats.reshape(N, C, 1), torch.zeros(N, 2 * C, device="cuda")[:, ::2],
                feats.cpu(), _np(feats), torch.zeros(N, 0, device="cuda"), torch.zeros(N, 513, device="cuda")):
        with pytest.raises(ValueError):
            ctx.render_features(bad)
    for bad in (out.double(), out[..., 0], torch.zeros(H, W + 1, C, device="cuda"), torch.zeros(H, W, C + 1, device="cuda"),
                torch.zeros(H, W, 2 * C, device="cuda")[..., ::2], out.cpu()):
        with pytest.raises(ValueError):
            ctx.render_features(feats, out=bad)
        with pytest.raises(ValueError):
            ctx.lift_features(bad, lifted)
    for bad in (lifted.double(), lifted[:, 0], torch.zeros(N, C + 1, device="cuda"), lifted.cpu(),
                torch.zeros(N, 2 * C, device="cuda")[:, ::2]):
        with pytest.raises(ValueError):
            ctx.lift_features(fmap, bad)
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in (feats, fmap, out, lifted))
    check = lib.check
    owned = [fwd[k].data_ptr() for k in ("mask", "uv_all", "xyz_c_all", "sigma", "conic", "J", "rgb", "radius", "sorted",
                                         "ranges", "image", "T", "n")]
    check(ctx._lib.gsplat_context_detach_forward_outputs(ctx._h))
    refused(ctx)                                     # the forward's arrays are the caller's now
    for p in owned:                                  # ... who returns them to the pool
        check(ctx._lib.gsplat_pool_free(ctypes.c_void_p(p)))
    behind = dp["xyz"].clone()
    behind[:, 2] = -behind[:, 2].abs() - 1.0
    fresh = raster.RasterContext(N, W, H)
    fresh.rasterize_image(dp, dc, c, 0.0, L)
    with pytest.raises(lib.GsplatError) as e:
        fresh.rasterize_image(dict(dp, xyz=behind), dc, c, 0.0, L)
    assert e.value.code == -5
    refused(fresh)                                   # the last forward saw nothing
    with pytest.raises(lib.GsplatError):
        fresh.render_features(feats)


# ---------------------------------------------------------------- Trainer
def test_trainer_render_features_and_lift_maps(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    t.train(2, loss_every=0)
    n, ctx = t.num_gaussians, t.ctx
    H, W = int(views[0][0]["height"]), int(views[0][0]["width"])
    # render_features: the context-level map of a render-only forward, and the context's modes as they were
    modes = (ctx._depth, ctx._depth_inverse, ctx._depth_moment, ctx._filter3d)
    feats = torch.as_tensor(fr.seeded_rows(n, 5, 31)).cuda()
    got = t.render_features(views[1][0], feats)
    assert got.shape == (H, W, 5) and (ctx._depth, ctx._depth_inverse, ctx._depth_moment, ctx._filter3d) == modes
    ctx.rasterize_image(dict(t.params), views[1][0], t.cfg, 0.0, t.l_max)  # (the loop's lean forward: the same bits)
    assert torch.equal(ctx.render_features(feats), got)
    with pytest.raises(ValueError):
        t.render_features(views[1][0], feats[:-1])
    # lift_maps: every view says the constant v (powers of two: w * v is exact), every composited gaussian hears v
    v = torch.tensor([0.5, -2.0, 4.0], device="cuda")
    maps = [(cam, v.expand(H, W, 3).contiguous()) for cam, _ in views]
    lifted = t.lift_maps(maps)
    px = _np(t.contribution_scores([(cam,) for cam, _ in views])["pixels"]).astype(np.float64)
    got, want = _np(lifted).astype(np.float64), _np(v).astype(np.float64)
    assert lifted.shape == (n, 3) and (px > 0).any() and (px[-50:] == 0).all()
    assert (got[px == 0] == 0).all()
    rel = np.abs(got[px > 0] / want - 1.0)
    print(f"lift_maps: worst relative error / (2 pixels 2^-24) = {float((rel / (2 * px[px > 0, None] * 2.0 ** -24)).max()):.3f}")
    assert (rel <= 2 * px[px > 0, None] * 2.0 ** -24).all()
    raw = t.lift_maps(maps, normalize=False)
    weight = _np(t.contribution_scores([(cam,) for cam, _ in views])["weight_sum"]).astype(np.float64)
    assert_grad_close(_np(raw), weight[:, None] * want[None, :], "lift_maps without normalisation")
    # the loop still trains
    before = {k: p.clone() for k, p in t.params.items()}
    it = t.iter
    t.train(6, loss_every=0)
    torch.cuda.synchronize()
    assert t.iter == it + 6 and all(bool(torch.isfinite(p).all()) for p in t.params.values())
    assert not torch.equal(t.params["xyz"], before["xyz"])

"""GPU: the forward and backward on tile grids around their limits (tests/tile_grid_cases.py has the table): the counting
sort up to kBinMaxTiles = 16 384 tiles (`per` = 1 .. 16 tiles per thread in bin_scatter_kernel's scan, 64 KB of dynamic
LDS at the limit, the second slot of tile_order_kernel, the ninth trip of the segment tables), the radix route beyond it
(key widths up to 17 bits, runs of empty tiles, no tile order, no split lists, no compact lists), and one context that
renders views on both sides of the limit.  Everything is compared with the CPU oracle at conftest's bars; lists and ranges
bit for bit."""
import numpy as np
import pytest

import absgrad_reference
import antialias_reference as aar
import depth_reference
import tile_grid_cases as tg
from conftest import assert_grad_close, assert_image_close, assert_stop_indices_close, pkg
from test_contribution_gpu import _check_parity as _check_contributions
from test_contribution_gpu import _reference_global
from test_depth_gpu import _check_depth, _maps
from test_fused_gpu import _check_backward, _check_forward, _np

pytestmark = pytest.mark.gpu

FWD_KEYS = ("image", "T", "n", "sorted", "ranges")
INTERMEDIATES = (("conic", "conic"), ("uv", "uv"), ("J", "J"), ("sigma", "sigma"), ("xyz_c", "xyz_c"),
                 ("precompute_rgb", "rgb_pre"))
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    """The oracle arrays of the shared cases (a few hundred MB) go when this module's tests are done."""
    yield
    _cases.clear()


def _case(scene, orc, name, kind="plain", keep=False):
    """Scene, camera, gradient image and the oracle's forward and backward of a case (kept for the cases several tests
    share; the oracle needs about a second at these sizes)."""
    key = (name, kind)
    if key in _cases:
        return _cases[key]
    if name == "small":
        W, H = tg.SMALL_VIEW
        L, N = 1, 20000
        params, cam = tg.build_scene(scene, W, H, L, N, kind)
    else:
        _, _, W, H, L, N, _ = tg.GRIDS[name]
        params, cam = tg.grid_scene(scene, name, kind)
    ref = tg.oracle_forward(orc, scene, params, cam, L)
    if name != "small":
        tg.check_preconditions(name, kind, ref)
    gi = tg.grad_image(scene, W, H)
    bref = orc.backward_pass(ref, cam, gi, scene.CONFIG["bg"], L, threads=16)
    case = dict(name=name, kind=kind, N=N, W=W, H=H, L=L, T=((W + 15) // 16) * ((H + 15) // 16), params=params, cam=cam,
                gi=gi, ref=ref, bref=bref)
    if keep:
        _cases[key] = case
    return case


def _device(torch, case):
    raster = pkg("raster")
    return raster.device_params(case["params"]), raster.device_camera(case["cam"]), torch.as_tensor(case["gi"]).cuda()


def _backward(ctx, scene, case, dp, dc, gi_d, fwd, **extra):
    grads = ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True)
    for g in grads.values():
        g.fill_(float("nan"))  # every gradient array must be overwritten
    ctx.backward_pass(dp, dc, gi_d, scene.CONFIG["bg"], case["L"], grads, **extra)
    return grads


def _check_all_gradients(grads, bref, what=""):
    _check_backward(grads, bref)
    for k, rk in INTERMEDIATES:
        assert_grad_close(_np(grads[k]), bref[rk], f"grad_{k}{what}")


def _bits(fwd):
    return {k: _np(fwd[k]).copy() for k in FWD_KEYS}


def _routes(T):
    """Up to the limit: the counting sort and the radix sorts, forced.  Beyond it: automatic, and the counting sort asked
    for, which must be harmless."""
    return (1, 2) if T <= tg.BIN_MAX_TILES else (0, 1)


# ------------------------------------------------------------------ 1. forward and backward against the oracle, every grid
@pytest.mark.parametrize("name", list(tg.GRIDS))
def test_forward_and_backward_match_the_oracle(gpu, scene, orc, name):
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, name, keep=name in ("t16384", "t16512"))
    dp, dc, gi_d = _device(torch, case)
    c = scene.CONFIG
    got = {}
    for route in _routes(case["T"]):
        ctx = raster.RasterContext(case["N"], case["W"], case["H"])
        ctx.set_binning_route(route)
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], case["L"])
        _check_forward(fwd, case["ref"])  # lists and ranges exact; image, T, stop indices at conftest's bars
        grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd)
        got[route] = _bits(fwd)
        _check_all_gradients(grads, case["bref"], f" (route {route})")
        cnt = ctx.counters()
        print(f"{name} route {route}: T={case['T']} S={fwd['num_splats']} counters {cnt}")
        if case["T"] > tg.BIN_MAX_TILES:
            assert cnt["compact_list_backwards"] == cnt["ordered_backwards"] == cnt["segmented_backwards"] == 0
        del fwd, grads
        ctx.close()
    a, b = (got[r] for r in _routes(case["T"]))
    for k in FWD_KEYS:
        assert np.array_equal(a[k], b[k]), f"{name}: {k} differs between the binning routes {_routes(case['T'])}"


@pytest.mark.parametrize("name", tg.EMPTY_TAIL_GRIDS)
def test_empty_tiles_at_the_end_of_the_grid(gpu, scene, orc, name):
    """The last tile rows empty (every other case fills the last tile): the ranges behind the last list must all be
    S, on both routes, also when the context's previous forward left larger values there."""
    torch, raster = gpu, pkg("raster")
    full = _case(scene, orc, name, keep=True)
    _, _, W, H, L, N, _ = tg.GRIDS[name]
    params, cam = tg.empty_tail_scene(scene, name)
    ref = tg.oracle_forward(orc, scene, params, cam, L)
    tg.check_empty_tail(name, ref, full["ref"])
    c = scene.CONFIG
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    dp_full, dc_full, _ = _device(torch, full)
    got = {}
    for route in _routes(full["T"]):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_binning_route(route)
        ctx.rasterize_image(dp_full, dc_full, c, c["bg"], L)
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        _check_forward(fwd, ref)
        got[route] = _bits(fwd)
        del fwd
        ctx.close()
    a, b = (got[r] for r in _routes(full["T"]))
    for k in FWD_KEYS:
        assert np.array_equal(a[k], b[k]), f"{name}: {k} differs between the binning routes"


# ------------------------------------------------------------------ 2. the path taken is the one documented
@pytest.mark.parametrize("name", ["t16384", "t16385", "t16512", "t65792"])
def test_compact_lists_up_to_the_limit_only(gpu, scene, orc, name):
    """Short lists, counting route asked for: up to 16 384 tiles the backwards walk the compact lists (out[10] of
    gsplat_context_get_counters), beyond they never do -- the radix route does not know the longest list."""
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, name, keep=name in ("t16384", "t16512"))
    dp, dc, gi_d = _device(torch, case)
    c = scene.CONFIG
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_binning_route(1)
    seen = []
    for it in range(2):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], case["L"])
        grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd)
        _check_all_gradients(grads, case["bref"], f" (forward {it})")
        seen.append(ctx.counters())
    print(f"{name}: {seen}")
    walked = [s["compact_list_backwards"] for s in seen]
    if case["T"] <= tg.BIN_MAX_TILES:
        assert walked[1] > walked[0] and walked[1] == 2, seen
        assert seen[1]["useful_entries"] > 0
    else:
        assert walked == [0, 0] and seen[1]["useful_entries"] == 0, seen
        assert seen[1]["ordered_backwards"] == 0 and seen[1]["segmented_backwards"] == 0
    assert seen[1]["forwards"] == 2 and seen[1]["tail_redone"] == 0


@pytest.mark.parametrize("name", tg.ORDER_GRIDS)
def test_tile_order_up_to_the_limit_only(gpu, scene, orc, name):
    """The skewed scene (longest list far above three times the average): the backward takes its tiles heaviest first
    from the second forward on (out[4]) where tile_order_kernel reaches, 16 384 tiles, and never beyond.  At 8 281 tiles
    the heavy tile sits in the twelve live threads of the kernel's second slot."""
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, name, "skewed")
    dp, dc, gi_d = _device(torch, case)
    c = scene.CONFIG
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_binning_route(1)
    seen = []
    for it in range(3):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], case["L"])
        if it == 0:
            _check_forward(fwd, case["ref"])
        grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd)
        _check_all_gradients(grads, case["bref"], f" (forward {it})")
        seen.append(ctx.counters())
    print(f"{name} skewed: {seen}")
    ordered = [s["ordered_backwards"] for s in seen]
    assert ordered == ([0, 1, 2] if case["T"] <= tg.BIN_MAX_TILES else [0, 0, 0]), seen


@pytest.mark.parametrize("name", tg.SEGMENT_GRIDS)
def test_segments_up_to_the_limit_only(gpu, scene, orc, name):
    """The long-list scene (one list of 2 000 entries near the end of the grid): up to 16 384 tiles the backward walks it
    in segments from the second forward on (out[5]) and, with the gate open, the forward splits it from the fourth on
    (out[6]; the figures of the forward two back decide).  At 16 385 tiles neither ever happens.  At 8 281 tiles the list
    is one of the 89 tiles of the segment tables' ninth, partial trip."""
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, name, "long")
    dp, dc, gi_d = _device(torch, case)
    c = scene.CONFIG
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_binning_route(1)
    ctx.set_segment_options(gate=0.0)
    limit = case["T"] <= tg.BIN_MAX_TILES
    seen = []
    for it in range(5):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], case["L"])
        _check_forward(fwd, case["ref"])
        grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd)
        cnt = ctx.counters()
        seen.append(cnt)
        assert cnt["segmented_backwards"] == (it if limit else 0), seen
        assert cnt["segmented_forwards"] == (max(0, it - 2) if limit else 0), seen
        _check_all_gradients(grads, case["bref"], f" (forward {it})")
    print(f"{name} long: {seen}")
    if limit:
        assert seen[-1]["longest_chain"] == int(_np(fwd["n"]).max()) > tg.SEG_SPLIT_MIN
    assert seen[-1]["compact_list_backwards"] == 0  # (the first forward's list is beyond kSegSplitMin)


# ------------------------------------------------------------------ 3. modes beyond the limit (2064 x 2048, 16 512 tiles)
def test_depth_mode_beyond_the_limit(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, "t16512", keep=True)
    dp, dc, gi_d = _device(torch, case)
    c, W, H, L, ref = scene.CONFIG, case["W"], case["H"], case["L"], case["ref"]
    ctx = raster.RasterContext(case["N"], W, H)
    ctx.set_depth(True)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    _check_forward(fwd, ref)
    # test_depth_gpu.py's bar, 1e-5 relative, against the reference evaluated in float64: over these 4.2 M pixels the
    # float32 evaluation is itself that far from the float64 one in four pixels (and the library is not)
    dref, aref = depth_reference.depth_alpha(orc, ref, W, H, dtype=np.float64, threads=16)
    _check_depth(fwd, ref, dref, np.asarray(ref["image"], np.float64))
    assert torch.equal(fwd["alpha"], 1.0 - fwd["T"])
    # alpha within test_depth_gpu.py's 2e-5 of the reference; as for the depth, a pixel beyond it must be one whose image
    # or stop index differs too (a threshold decision: one such pixel in these 4.2 M)
    off = np.abs(_np(fwd["alpha"]).astype(np.float64) - aref) > 2e-5
    flagged = (np.abs(_np(fwd["image"]).astype(np.float64) - ref["image"]).sum(-1) > 1e-5) | (_np(fwd["n"]) != ref["n"])
    assert not (off & ~flagged).any() and off.mean() < 1e-4, f"{int(off.sum())} alpha pixels off"
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd, grad_depth=gd_d, grad_alpha=ga_d)
    g = depth_reference.backward_pass(orc, ref, case["cam"], case["gi"], gd, ga, c["bg"], L, threads=16)
    _check_all_gradients(grads, g, " (depth mode)")


def test_absgrad_sums_beyond_the_limit(gpu, scene, orc):
    """(tile_grid_cases.absgrad_scene: 6 000 gaussians, for the float64 reference's sake.)"""
    torch, raster = gpu, pkg("raster")
    _, _, W, H, L, _, _ = tg.GRIDS["t16512"]
    N, c = tg.ABSGRAD_GAUSSIANS, scene.CONFIG
    params, cam = tg.absgrad_scene(scene)
    ref = tg.oracle_forward(orc, scene, params, cam, L)
    tg.check_absgrad_scene(ref)
    gi = _case(scene, orc, "t16512", keep=True)["gi"]
    bref = orc.backward_pass(ref, cam, gi, c["bg"], L, threads=16)
    case = dict(N=N, W=W, H=H, L=L, params=params, cam=cam, gi=gi)
    dp, dc, gi_d = _device(torch, case)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_absgrad(True)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd)
    got = _np(ctx.absgrad_uv())
    signed, absolute = absgrad_reference.absgrad_sums(ref, gi, W, H, c["bg"], dtype=np.float64)
    assert_grad_close(got, absolute, "abs_uv")
    assert_grad_close(_np(grads["uv"]), signed, "grad_uv")
    _check_all_gradients(grads, bref, " (absgrad mode)")


def test_contributions_beyond_the_limit(gpu, scene, orc):
    """accumulate_contributions after a plain and after a render-only forward: both meet the reference, and weight_max and
    pixels (bit-reproducible) are the same in both."""
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, "t16512", keep=True)
    dp, dc, _ = _device(torch, case)
    c, N, W, H, L = scene.CONFIG, case["N"], case["W"], case["H"], case["L"]
    want, c2g = _reference_global(case["ref"], W, H, N)
    culled = np.ones(N, bool)
    culled[c2g] = False
    got = {}
    for mode in ("plain", "render_only"):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_render_only(mode == "render_only")
        ctx.rasterize_image(dp, dc, c, c["bg"], L)
        a = dict(weight_sum=torch.zeros(N, device="cuda"), weight_max=torch.zeros(N, device="cuda"),
                 pixels=torch.zeros(N, dtype=torch.int32, device="cuda"))
        ctx.accumulate_contributions(**a)
        _check_contributions(a, want, culled, W * H, f"16 512 tiles, {mode} forward")
        got[mode] = a
    assert torch.equal(got["plain"]["weight_max"], got["render_only"]["weight_max"])
    assert torch.equal(got["plain"]["pixels"], got["render_only"]["pixels"])


def test_lean_and_antialiased_beyond_the_limit(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    case = _case(scene, orc, "t16512", keep=True)
    dp, dc, gi_d = _device(torch, case)
    c, N, W, H, L = scene.CONFIG, case["N"], case["W"], case["H"], case["L"]
    full = raster.RasterContext(N, W, H)
    base = full.rasterize_image(dp, dc, c, c["bg"], L)
    keep = {k: _np(base[k]).copy() for k in FWD_KEYS + ("radius",)}
    lean = raster.RasterContext(N, W, H)
    lean.set_lean_forward(True)
    out = lean.rasterize_image(dp, dc, c, c["bg"], L)
    for k, v in keep.items():
        assert np.array_equal(_np(out[k]), v), f"{k}: the lean forward differs"
    assert out["sigma"] is None and out["uv_all"] is None
    _check_all_gradients(_backward(lean, scene, case, dp, dc, gi_d, out), case["bref"], " (lean)")
    # anti-aliased mode, once
    plain, ref = aar.forward(orc, case["params"], case["cam"], c, c["bg"], L, threads=16)
    g = aar.backward(orc, ref, case["cam"], case["gi"], c["bg"], L, threads=16)
    full.set_antialiased(True)
    fwd = full.rasterize_image(dp, dc, c, c["bg"], L)
    _check_forward(fwd, ref)
    grads = _backward(full, scene, case, dp, dc, gi_d, fwd)
    for k, rk in (("xyz", "xyz"), ("rgb", "band0"), ("sh", "sh"), ("opacity", "opacity"), ("scale", "scale"),
                  ("quaternion", "quaternion")) + INTERMEDIATES:
        want = np.asarray(g[rk])
        assert_grad_close(_np(grads[k]).reshape(want.shape), want, f"grad_{k} (anti-aliased)")
    assert np.abs(_np(fwd["image"]).astype(np.float64) - plain["image"]).sum(-1).max() > 0.05  # the mode does something


# ------------------------------------------------------------------ 4. one context, views on both sides of the limit
def test_one_context_renders_views_on_both_sides_of_the_limit(gpu, scene, orc):
    """What Trainer does with a dataset of mixed image sizes: one context for the largest view, every view through it.
    dense_route, last_longest, compact_ready, order_ready and seg_ready travel from one regime into the other; each
    forward must give the bits of a fresh context's forward of that view, each backward the oracle's gradients."""
    torch, raster = gpu, pkg("raster")
    c = scene.CONFIG
    views = {"small": _case(scene, orc, "small"), "t16512": _case(scene, orc, "t16512", keep=True),
             "t16384": _case(scene, orc, "t16384", keep=True), "small_long": _case(scene, orc, "small", "long")}
    assert np.diff(views["small_long"]["ref"]["ranges"]).max() > tg.SEG_SPLIT_MIN
    dev, fresh = {}, {}
    for key, case in views.items():
        dev[key] = _device(torch, case)
        ctx = raster.RasterContext(case["N"], case["W"], case["H"])
        fwd = ctx.rasterize_image(dev[key][0], dev[key][1], c, c["bg"], case["L"])
        _check_forward(fwd, case["ref"])
        fresh[key] = _bits(fwd)
        del fwd
        ctx.close()
    big = views["t16512"]
    ctx = raster.RasterContext(big["N"], big["W"], big["H"])
    sequence = ("small", "t16512", "t16384", "small", "t16512", "small_long", "t16384")
    for step, key in enumerate(sequence):
        case, (dp, dc, gi_d) = views[key], dev[key]
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], case["L"])
        grads = _backward(ctx, scene, case, dp, dc, gi_d, fwd)
        got = _bits(fwd)
        for k in FWD_KEYS:
            if key == "small_long" and k == "image":
                assert_image_close(got[k], fresh[key][k], f"step {step} ({key}): image")
            else:
                assert np.array_equal(got[k], fresh[key][k]), f"step {step} ({key}): {k} differs from a fresh context's"
        _check_all_gradients(grads, case["bref"], f" (step {step}, {key})")
    cnt = ctx.counters()
    print(f"mixed sequence: {cnt}")
    assert cnt["forwards"] == len(sequence)


# ------------------------------------------------------------------ 5. stand-alone operators on big grids
@pytest.mark.parametrize("ntx,nty,empty_tail", tg.BAND_GRIDS)
def test_binning_operator_on_big_and_tiny_grids(gpu, orc, ntx, nty, empty_tail):
    """ops.get_sorted_gaussian_list, the two-call protocol: count, ranges and lists exact, nothing written behind them."""
    torch, ops = gpu, pkg("ops")
    uv, xyz, radius = tg.band_scene(ntx, nty, empty_tail)
    M = len(uv)
    want_sorted, want_ranges, cap = orc.get_sorted_gaussian_list(uv, xyz, radius, ntx, nty)
    tg.check_band_scene(ntx, nty, empty_tail, want_ranges)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    d_uv, d_xyz, d_r = dev(uv), dev(xyz), dev(radius)
    count = ops.get_sorted_gaussian_list(d_uv, d_xyz, d_r, ntx, nty, M, 0, None, None)
    assert count == cap
    GUARD = 64
    srt = torch.full((count + GUARD,), -7, dtype=torch.int32, device="cuda")
    ranges = torch.full((ntx * nty + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    ops.get_sorted_gaussian_list(d_uv, d_xyz, d_r, ntx, nty, M, count, srt, ranges)
    r, s = ranges.cpu().numpy(), srt.cpu().numpy()
    S = len(want_sorted)
    assert np.array_equal(r[:ntx * nty + 1], want_ranges)
    assert np.array_equal(s[:S], want_sorted)
    assert (r[ntx * nty + 1:] == -7).all() and (s[count:] == -7).all(), "written behind the outputs"


def test_render_operators_beyond_the_limit(gpu, scene, orc):
    """ops.render_image and ops.render_image_backward at 2064 x 2048 from the oracle's forward arrays."""
    torch, ops = gpu, pkg("ops")
    case = _case(scene, orc, "t16512", keep=True)
    f, b, W, H, bg = case["ref"], case["bref"], case["W"], case["H"], scene.CONFIG["bg"]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    uv, op, conic, rgb = dev(f["uv"]), dev(f["opacity"]), dev(f["conic"]), dev(f["rgb"])
    srt, rng = dev(f["sorted"]), dev(f["ranges"])
    n = torch.zeros(H, W, dtype=torch.int32, device="cuda")
    T = torch.zeros(H, W, device="cuda")
    img = torch.zeros(H, W, 3, device="cuda")
    ops.render_image(uv, op, conic, rgb, bg, srt, rng, W, H, n, T, img)
    assert_image_close(_np(img), f["image"], "image")
    assert_image_close(_np(T), f["T"], "final transmittance")
    assert_stop_indices_close(_np(n), f["n"])
    M = f["num_culled"]
    g_rgb, g_op = torch.zeros(M, 3, device="cuda"), torch.zeros(M, device="cuda")
    g_uv, g_conic = torch.zeros(M, 2, device="cuda"), torch.zeros(M, 3, device="cuda")
    ops.render_image_backward(uv, op, conic, rgb, bg, srt, rng, dev(f["n"]), dev(f["T"]), dev(case["gi"]), W, H, g_rgb,
                              g_op, g_uv, g_conic)
    assert_grad_close(_np(g_rgb), b["rgb_pre"], "grad_rgb")
    assert_grad_close(_np(g_op), b["opacity"], "grad_opacity")
    assert_grad_close(_np(g_uv), b["uv"], "grad_uv")
    assert_grad_close(_np(g_conic), b["conic"], "grad_conic")

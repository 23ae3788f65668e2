"""Compact lists for the compositing backward (gs_render.h: CompactLists; RasterContext.set_compact_lists): the forward
writes, per tile, the list entries whose ellipse alpha >= 1/255 can reach a 4x4 block of the tile, and the backward walks
only those.  Forward outputs must stay the same bits, gradients the oracle's and -- up to the order of the float atomics --
those of the full lists, in every mode of the backward; the counters say which lists a backward walked."""
import numpy as np
import pytest

from conftest import assert_grad_close, pkg
from test_fused_gpu import _check_backward, _check_forward, _np

pytestmark = pytest.mark.gpu

FWD_BATCH, SEG_SPLIT_MIN = 248, 1488  # gs_render.h: GS_FWD_BATCH, kSegSplitMin
LEAVES = ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")
INTERMEDIATES = ("conic", "uv", "J", "sigma", "xyz_c", "precompute_rgb")

# name: (gaussians, width, height, SH degree, opacity logits)
SCENES = {
    "main": (6000, 128, 96, 3, (-5.0, 3.0)),
    "saturating": (12000, 128, 96, 3, (-5.0, 6.0)),
    "small": (1500, 64, 48, 3, (-5.0, 3.0)),
}
_cases, _runs = {}, {}


def _provably_inert(ref, W):
    """Per instance of the oracle's lists, in float64: True when the box around the ellipse alpha >= 1/255 (gs_render.h:
    footprint), grown by half a pixel, misses the instance's tile, or the opacity can never reach 1/255.  Sufficient for
    an empty block mask, not necessary (the kernel tests the ellipse against 4x4 blocks): a lower bound on the entries the
    compact lists drop.  Returns (tile of each instance, flags)."""
    ranges, ids = np.asarray(ref["ranges"]), np.asarray(ref["sorted"])
    ntx = (W + 15) // 16
    tile = np.repeat(np.arange(len(ranges) - 1), np.diff(ranges))
    x0, y0 = (tile % ntx) * 16.0, (tile // ntx) * 16.0
    uv, con = np.asarray(ref["uv"], np.float64)[ids], np.asarray(ref["conic"], np.float64)[ids]
    opa = 1.0 / (1.0 + np.exp(-np.asarray(ref["opacity"], np.float64)[ids]))
    a, b, c = con[:, 0], con[:, 1], con[:, 2]
    det = a * c - b * b
    tau2 = 2.0 * np.maximum(0.0, np.log(255.0 * opa)) + 1e-3
    hx = np.sqrt(tau2 * c / det) * 1.0005 + 0.01 + 0.5
    hy = np.sqrt(tau2 * a / det) * 1.0005 + 0.01 + 0.5
    miss = (uv[:, 0] + hx < x0) | (uv[:, 0] - hx > x0 + 15) | (uv[:, 1] + hy < y0) | (uv[:, 1] - hy > y0 + 15)
    return tile, miss | (opa * 255.0 < 0.998)


def _oracle(scene, orc, params, cam, W, H, L):
    c = scene.CONFIG
    gi = scene.make_grad_image(W, H)
    ref = orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], c["bg"], L, threads=8)
    bref = orc.backward_pass(ref, cam, gi, c["bg"], L, threads=8)
    return dict(params=params, cam=cam, W=W, H=H, L=L, gi=gi, ref=ref, bref=bref, N=len(params["xyz"]))


def _case(scene, orc, name):
    """The scene and the oracle's forward and backward of it, computed once per session."""
    if name not in _cases:
        N, W, H, L, opacity = SCENES[name]
        _cases[name] = _oracle(scene, orc, scene.make_gaussians(N, W, H, L, opacity_range=opacity),
                               scene.make_camera(W, H, 0), W, H, L)
    return _cases[name]


def _step(torch, scene, case, compact, depth=False, absgrad=False, antialiased=False, route=None, backwards=1,
          check_forward=False):
    """One forward and `backwards` backwards in a fresh context; everything is copied to the host and the context closed
    (what this returns may be kept for other tests: nothing of it holds device memory).  check_forward: the forward against
    the case's oracle, while its views exist."""
    raster = pkg("raster")
    c = scene.CONFIG
    ctx = raster.RasterContext(case["N"], case["W"], case["H"])
    ctx.set_compact_lists(compact)
    if route is not None:
        ctx.set_binning_route(route)
    ctx.set_depth(depth)
    ctx.set_absgrad(absgrad)
    ctx.set_antialiased(antialiased)
    dp, dc = raster.device_params(case["params"]), raster.device_camera(case["cam"])
    bytes_before = ctx.workspace_bytes
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], case["L"])
    if check_forward:
        _check_forward(fwd, case["ref"])
    gi = torch.as_tensor(case["gi"]).cuda()
    extra = {}
    if depth:  # depth and alpha gradients of their own, not multiples of the image's
        extra = dict(grad_depth=(0.3 * gi[..., 0] - 0.1 * gi[..., 2]).contiguous(), grad_alpha=(0.5 * gi[..., 1]).contiguous())
    all_grads = []
    for _ in range(backwards):
        grads = ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True)
        for g in grads.values():
            g.fill_(float("nan"))
        ctx.backward_pass(dp, dc, gi, c["bg"], case["L"], grads, **extra)
        torch.cuda.synchronize()
        got = {k: _np(v).copy() for k, v in grads.items()}
        if absgrad:
            got["absgrad_uv"] = _np(ctx.absgrad_uv()).copy()
        all_grads.append(got)
    out = dict(grads=all_grads[-1], all_grads=all_grads, counters=ctx.counters(), num_splats=int(fwd["num_splats"]),
               grew=ctx.workspace_bytes > bytes_before,
               outputs={k: _np(fwd[k]).copy() for k in ("image", "T", "n", "ranges", "sorted")})
    if depth:
        out["outputs"]["depth"] = _np(fwd["depth"]).copy()
    del fwd, grads, g
    ctx.close()
    return out


def _plain_run(torch, scene, orc, name, compact):
    if (name, compact) not in _runs:
        _runs[(name, compact)] = _step(torch, scene, _case(scene, orc, name), compact, check_forward=True)
    return _runs[(name, compact)]


def _assert_walked_compact(run, ref, W, backwards=1):
    """From the counters: the backward ran on compact lists, and those hold under 80 % of the instances (the scenes of this
    file have 27 to 58 % inert ones) and none of the entries whose footprint provably misses their tile."""
    cnt, S = run["counters"], run["num_splats"]
    assert cnt["compact_list_backwards"] == backwards, cnt
    assert S == len(ref["sorted"])
    _, inert = _provably_inert(ref, W)
    print(f"useful entries {cnt['useful_entries']} of {S} instances ({cnt['useful_entries'] / S:.3f}); "
          f"{int(inert.sum())} provably inert")
    assert 0 < cnt["useful_entries"] < 0.8 * S, cnt
    assert cnt["useful_entries"] <= S - int(inert.sum()), cnt


def _assert_same_gradients(got, want, what):
    assert set(got) == set(want)
    for k in got:  # the same sums with the zero terms left out, in another order of the atomics
        assert_grad_close(got[k], want[k], f"{what}: grad_{k}", rel=1e-4)


@pytest.mark.parametrize("name", ["main", "saturating", "small"])
def test_compact_backward_matches_oracle(gpu, scene, orc, name):
    """main: 48 tiles, every list two or more forward batches, nearly every tile three or more backward batches of useful
    entries, 30.8 % of 19 883 instances inert, pixels that stop early in 47 tiles.  saturating: in 47 of 48 tiles every
    pixel stops before the end of its list (the forward's workgroups leave early and rank only what they walked), longest
    list 936.  small: 12 tiles, 27 % inert."""
    case = _case(scene, orc, name)
    ref, W = case["ref"], case["W"]
    lens, stops = np.diff(ref["ranges"]), np.asarray(ref["n"])
    assert lens.max() <= SEG_SPLIT_MIN, "the list must stay whole"
    if name == "main":
        assert len(lens) == 48 and lens.min() > FWD_BATCH and len(ref["sorted"]) == 19883 and lens.max() == 479
    elif name == "saturating":
        assert len(lens) == 48 and lens.max() == 936
        early = 0
        for t in range(48):  # tiles in which every pixel stops in front of the end of the list
            ty, tx = divmod(t, 8)
            early += int((stops[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] < lens[t]).all())
        assert early >= 40, early
    else:
        assert len(lens) == 12
    run = _plain_run(gpu, scene, orc, name, True)  # (checks the forward against the oracle)
    _assert_walked_compact(run, ref, W)
    _check_backward({k: gpu.as_tensor(v) for k, v in run["grads"].items()}, case["bref"])


@pytest.mark.parametrize("name", ["main", "saturating"])
def test_switch_changes_nothing(gpu, scene, orc, name):
    on, off = _plain_run(gpu, scene, orc, name, True), _plain_run(gpu, scene, orc, name, False)
    assert on["counters"]["compact_list_backwards"] == 1
    assert off["counters"]["compact_list_backwards"] == 0 and off["counters"]["useful_entries"] == 0, off["counters"]
    for k in ("image", "T", "n", "ranges", "sorted"):
        assert (on["outputs"][k] == off["outputs"][k]).all(), k
    _assert_same_gradients(on["grads"], off["grads"], "compact vs full lists")


@pytest.mark.parametrize("mode", ["depth", "absgrad", "antialiased"])
def test_modes_walk_compact_lists(gpu, scene, orc, mode):
    case = _case(scene, orc, "main")
    on = _step(gpu, scene, case, True, **{mode: True})
    off = _step(gpu, scene, case, False, **{mode: True})
    assert on["counters"]["compact_list_backwards"] == 1 and off["counters"]["compact_list_backwards"] == 0
    for k in on["outputs"]:
        assert (on["outputs"][k] == off["outputs"][k]).all(), k
    assert any(np.abs(v).max() > 0 for v in on["grads"].values())
    _assert_same_gradients(on["grads"], off["grads"], mode + ": compact vs full lists")


def _scene_with_untouched_tiles(scene):
    """96x64, 24 tiles.  Gaussians 0..31 sit in the middle of tile 10, gaussians 32..63 four pixels LEFT of the image;
    all have sigmas of 2 to 4 px (anisotropic: the rotation has a gradient) and opacity logit -5.5, just above 1/255: the mh_dist boxes span the neighbouring tiles, the
    ellipse alpha >= 1/255 is under a pixel wide.  The tiles of column 0 list only gaussians that cannot touch them."""
    N, W, H, L = 64, 96, 64, 1
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, 0)
    rng = np.random.default_rng(5)
    first = np.arange(N) < 32
    z = rng.uniform(4.0, 8.0, N)
    u = np.where(first, 72.0 + rng.uniform(-2, 2, N), -4.0 + rng.uniform(-0.5, 0.5, N))
    v = np.where(first, 24.0 + rng.uniform(-2, 2, N), 40.0 + rng.uniform(-2, 2, N))
    params["xyz"] = np.stack([(u - W / 2) * z / cam["fx"], (v - H / 2) * z / cam["fx"], z], 1).astype(np.float32)
    params["scale"][:] = np.log((3.0 * z / cam["fx"])[:, None] * np.array([1.0, 0.7, 1.3])).astype(np.float32)
    params["opacity"][:] = -5.5
    return params, cam, W, H, L


def test_tile_without_a_useful_entry(gpu, scene, orc):
    if "untouched" not in _cases:
        _cases["untouched"] = _oracle(scene, orc, *_scene_with_untouched_tiles(scene))
    case = _cases["untouched"]
    ref, W = case["ref"], case["W"]
    assert int(ref["mask"].sum()) == case["N"]  # (compacted order = global order)
    lens = np.diff(ref["ranges"])
    tile, inert = _provably_inert(ref, W)
    possibly_useful = np.bincount(tile[~inert], minlength=len(lens))
    bare = np.nonzero((lens > 0) & (possibly_useful == 0))[0]
    assert len(bare) >= 3 and {6, 12, 18} <= set(bare.tolist()), bare  # non-empty lists, nothing in them can touch the tile
    never = np.ones(case["N"], bool)
    never[np.asarray(ref["sorted"])[~inert]] = False
    assert never[32:].all() and not never[:32].any()  # the gaussians left of the image touch no tile at all
    run = _step(gpu, scene, case, True, check_forward=True)
    _assert_walked_compact(run, ref, W)
    _check_backward({k: gpu.as_tensor(v) for k, v in run["grads"].items()}, case["bref"])
    for k in LEAVES + INTERMEDIATES:  # every instance of these gaussians is inert: not one atomic, exact zeros
        assert (run["grads"][k][32:] == 0).all(), k
        assert np.abs(run["grads"][k][:32]).max() > 0, k


def test_second_backward_of_the_same_forward(gpu, scene, orc):
    case = _case(scene, orc, "small")
    run = _step(gpu, scene, case, True, backwards=2)
    assert run["counters"]["compact_list_backwards"] == 2
    _assert_same_gradients(run["all_grads"][1], run["all_grads"][0], "second backward vs first")
    _check_backward({k: gpu.as_tensor(v) for k, v in run["all_grads"][1].items()}, case["bref"])


def test_compact_lists_after_the_instance_buffers_grew(gpu, scene, orc):
    """The shape of test_instance_buffers_grow: many more than four instances per gaussian, so the forward finds its
    instance buffers too small after its speculative part has run, grows them -- the compact arrays with them -- and
    redoes placement, sorts and compositing."""
    if "grow" not in _cases:
        N, W, H, L = 300, 256, 144, 1
        params = scene.make_gaussians(N, W, H, L)
        params["scale"] += 2.5
        params["opacity"][:] = -3.0
        _cases["grow"] = _oracle(scene, orc, params, scene.make_camera(W, H), W, H, L)
    case = _cases["grow"]
    assert len(case["ref"]["sorted"]) > 6 * case["N"]
    run = _step(gpu, scene, case, True, route=1, check_forward=True)
    assert run["grew"] and run["counters"]["instance_growths"] == 1 and run["counters"]["tail_redone"] == 1, run["counters"]
    cnt, S = run["counters"], run["num_splats"]
    assert cnt["compact_list_backwards"] == 1 and 0 < cnt["useful_entries"] <= S, cnt
    _check_backward({k: gpu.as_tensor(v) for k, v in run["grads"].items()}, case["bref"])


def test_long_lists_keep_the_full_lists(gpu, scene):
    """The scene of test_long_lists_split_into_segments_for_the_backward (lists of 2 100 .. 7 000 entries): its first
    backward walks whole lists, the later ones segments -- none of them compact lists.  Parity is that test's business."""
    torch, raster = gpu, pkg("raster")
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
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    for it in range(3):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        assert int(np.diff(_np(fwd["ranges"])).max()) > SEG_SPLIT_MIN
        ctx.backward_pass(dp, dc, gi, c["bg"], L, ctx.alloc_gradients(fwd["num_culled"], L))
        cnt = ctx.counters()
        assert cnt["compact_list_backwards"] == 0 and cnt["segmented_backwards"] == it, cnt
        del fwd
    ctx.close()

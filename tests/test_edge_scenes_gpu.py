"""GPU parity on the edge scenes (tests/edge_scenes.py): clamped, near-plane, NaN-radius, needle, unnormalised and
saturated splats, culled rows interleaved.  Every comparison is made per population as well as over the whole array, so
a few dozen wrong edge rows cannot hide among thousands of ordinary ones.  The fused path is compared against the
float32 oracle (in the saturated population float32 and float64 disagree on which rows get a gradient)."""
import numpy as np
import pytest

import depth_reference
import edge_scenes as es
import parity_tools
from conftest import FLIP_MAX, MEAN_L1_TOL, assert_grad_close, assert_image_close, assert_stop_indices_close, pkg
from test_fused_gpu import _check_backward, _check_forward

pytestmark = pytest.mark.gpu
C = dict(near_thresh=0.3, mh_dist=3.0, cull_mask_padding=100, bg=0.5)
LEAVES = (("xyz", "xyz"), ("rgb", "band0"), ("sh", "sh"), ("opacity", "opacity"), ("scale", "scale"),
          ("quaternion", "quaternion"))


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


_CASES = {}


def _edge_case(scene, orc, size):
    if size in _CASES:
        return _CASES[size]
    params, cam, pops = es.make_edge_scene(size)
    N, W, H, L = es.SIZES[size]
    ref = orc.rasterize(params, cam, C["near_thresh"], C["mh_dist"], C["cull_mask_padding"], C["bg"], L, threads=16)
    gi = scene.make_grad_image(W, H)
    bref = orc.backward_pass(ref, cam, gi, C["bg"], L, threads=16, tan_fov=es.backward_tan_fov(cam))
    cp = es.compact_populations(pops, ref["mask"])
    on_list = np.zeros(ref["num_culled"], bool)
    on_list[ref["sorted"]] = True
    _CASES[size] = dict(size=size, N=N, W=W, H=H, L=L, params=params, cam=cam, pops=pops, cp=cp, ref=ref, gi=gi,
                        bref=bref, on_list=on_list)
    return _CASES[size]


@pytest.fixture(scope="module", params=["small", "large"])
def edge(request, scene, orc):
    return _edge_case(scene, orc, request.param)


# Where float32 itself cannot meet the element bar: the scale gradient of a needle's thin axis is mostly rounding (the
# float32 oracle against the float64 one: 8.3e-3 of the needle scale elements beyond 1e-3, relative L2 2.8e-4).  There
# the population is held to the relative L2 bar alone.
L2_ONLY = {("needle", "grad_scale")}
# Two populations of the larger scene are beyond float32 at the element level altogether (the float32 oracle against the
# float64 one): the near splats (faint, over ~1000-entry lists, sums with heavy cancellation: 1.8e-3 of the xyz elements
# beyond 1e-3, relative L2 1.1e-3) and the needles (scale 8.9e-3 beyond, relative L2 1.5e-3; quaternion 1.2e-3 beyond).
# Their rows are held to a relative L2 bar of LOOSE_L2: the HIP path and the float32 oracle each carry that rounding, so
# they may differ by up to about twice the largest figure (3e-3); a wrong branch or a dropped term is an O(1) error.
LOOSE = {("large", "near"), ("large", "needle")}
LOOSE_L2 = 5e-3


def _rel_l2(got, want, what, bar):
    a, b = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(a).all(), f"{what}: non-finite values"
    err = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    assert err < bar, f"{what}: relative L2 error {err:.3e} (bar {bar})"


def _per_population(got, want, cp, what, rel=1e-3, size=None):  # size: the scene's, for LOOSE
    assert_grad_close(got, want, what)
    for k, r in cp.items():
        if not len(r):
            continue
        if (size, k) in LOOSE:
            _rel_l2(got[r], want[r], f"{what} [{k}]", max(rel, LOOSE_L2))
        elif (k, what.split(" ")[0]) in L2_ONLY:
            _rel_l2(got[r], want[r], f"{what} [{k}]", rel)
        else:
            assert_grad_close(got[r], want[r], f"{what} [{k}]", rel=rel)


def _check_edge_forward(fwd, ref, size):
    """test_fused_gpu._check_forward on the small scene.  The large one has more pixels on a borderline alpha / T than the
    absolute caps of conftest allow (6 of 230 400 above 1e-4): there every differing pixel, stop index and instance must
    be explained in float64 as a borderline decision (parity_tools.explain); every other bar of _check_forward stays."""
    if size == "small":
        _check_forward(fwd, ref)
        return
    assert fwd["num_culled"] == int(ref["mask"].sum()) and fwd["num_pairs"] == int(ref["num_pairs"])
    assert (_np(fwd["mask"]).astype(bool) == ref["mask"]).all()
    np.testing.assert_allclose(_np(fwd["conic"]), ref["conic"], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(_np(fwd["rgb"]), ref["rgb"], rtol=1e-5, atol=2e-6)
    assert fwd["num_splats"] == len(ref["sorted"])
    assert (_np(fwd["ranges"]) == ref["ranges"]).all() and (_np(fwd["sorted"]) == ref["sorted"]).all()
    H, W = ref["n"].shape
    f = {k: _np(fwd[k]) for k in ("image", "T", "n", "sorted", "ranges", "radius")}
    rep = parity_tools.forward_parity_report(f, ref, W, H)
    worst = parity_tools.explain(rep, f, ref, W, H)
    print(f"[edge {size}] {int(round(rep['frac_above'] * W * H))} pixels > 1e-4, max {rep['max_l1']:.2e}, "
          f"n mismatches {rep['n_mismatch']}, worst alpha/T margin {worst['alpha_rel']:.2e}")
    _explained_image_bars(rep, f, ref)


def _explained_image_bars(rep, f, ref):
    """conftest.assert_image_close without its absolute pixel count (each such pixel is explained by the caller)."""
    assert rep["mean_l1"] < MEAN_L1_TOL and rep["max_l1"] < FLIP_MAX, (rep["mean_l1"], rep["max_l1"])
    t_err = np.abs(f["T"].astype(np.float64) - ref["T"])
    assert t_err.mean() < MEAN_L1_TOL and t_err.max() < FLIP_MAX
    assert_stop_indices_close(f["n"], ref["n"])


def test_edge_operators_match_oracle_per_population(gpu, orc, edge):
    """The stand-alone per-gaussian operators share the oracle's arithmetic order: H1 within 1e-5 per population, the
    conic and Sigma backwards within 1e-4, the NaN pattern of the radii exactly, the lists bit for bit; compositing with
    the north-star bars (on the large scene every pixel beyond them explained as borderline)."""
    torch, ops = gpu, pkg("ops")
    f, b, cam, cp = edge["ref"], edge["bref"], edge["cam"], edge["cp"]
    W, H, M = edge["W"], edge["H"], edge["ref"]["num_culled"]
    view = _dev(torch, cam["view"])
    sigma = torch.empty(M, 6, device="cuda")
    ops.compute_sigma(_dev(torch, f["quaternion"]), _dev(torch, f["scale"]), M, sigma)
    s_got = _np(sigma)
    for k, r in cp.items():  # (an off-diagonal entry is a difference of products: 2e-5 of its row's largest entry)
        err = np.abs(s_got[r] - f["sigma"][r])
        assert (err <= 2e-5 * np.abs(f["sigma"][r]).max(1, keepdims=True)).all(), f"sigma [{k}]: {err.max():.3e}"
    J, conic, radius = torch.empty(M, 6, device="cuda"), torch.empty(M, 3, device="cuda"), torch.empty(M, 4, device="cuda")
    ops.compute_conic(_dev(torch, f["xyz_c"]), view, _dev(torch, f["sigma"]), cam["fx"], cam["fy"], f["tan_fovx"],
                      f["tan_fovy"], 3.0, M, J, conic, radius)
    r_got = _np(radius)
    assert (np.isnan(r_got) == np.isnan(f["radius"])).all(), "NaN radii differ"
    assert np.isnan(r_got[cp["tiny"], 1]).all()
    for k, r in cp.items():
        if not len(r):
            continue
        np.testing.assert_allclose(_np(J)[r], f["J"][r], rtol=1e-6, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(_np(conic)[r], f["conic"][r], rtol=1e-5, atol=1e-7, err_msg=k)
        ok = (r_got[r, :2] == f["radius"][r, :2]) | np.isnan(f["radius"][r, :2])
        assert ok.mean() > 0.99, f"{k}: ceil'ed radii"
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    uv, xyz_c, rad = _dev(torch, f["uv"]), _dev(torch, f["xyz_c"]), _dev(torch, f["radius"])
    count = ops.get_sorted_gaussian_list(uv, xyz_c, rad, ntx, nty, M, 0, None, None)
    assert count == f["num_pairs"]
    srt = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    ranges = torch.full((ntx * nty + 1,), -1, dtype=torch.int32, device="cuda")
    ops.get_sorted_gaussian_list(uv, xyz_c, rad, ntx, nty, M, count, srt, ranges)
    assert (_np(ranges) == f["ranges"]).all() and (_np(srt)[:len(f["sorted"])] == f["sorted"]).all()
    # the per-gaussian backward chain, with the backward's tan(fov) given to both
    tfx, tfy = es.backward_tan_fov(cam)
    gJ, gS = torch.zeros(M, 6, device="cuda"), torch.zeros(M, 6, device="cuda")
    ops.compute_conic_backward(_dev(torch, f["J"]), _dev(torch, f["sigma"]), view, _dev(torch, f["conic"]),
                               _dev(torch, b["conic"]), M, gJ, gS)
    _per_population(_np(gJ), b["J"], cp, "grad_J", rel=1e-4)
    _per_population(_np(gS), b["sigma"], cp, "grad_sigma", rel=1e-4)
    want = orc.compute_projection_jacobian_backward(f["xyz_c"], cam["fx"], cam["fy"], tfx, tfy, b["J"])
    got = torch.zeros(M, 3, device="cuda")
    ops.compute_projection_jacobian_backward(xyz_c, cam["fx"], cam["fy"], float(tfx), float(tfy), _dev(torch, b["J"]), M, got)
    _per_population(_np(got), want, cp, "H1", rel=1e-5)
    gq, gs = torch.empty(M, 4, device="cuda"), torch.empty(M, 3, device="cuda")
    ops.compute_sigma_backward(_dev(torch, f["quaternion"]), _dev(torch, f["scale"]), _dev(torch, b["sigma"]), M, gq, gs)
    _per_population(_np(gq), b["quaternion"], cp, "grad_quaternion", rel=1e-4)
    _per_population(_np(gs), b["scale"], cp, "grad_scale", rel=1e-4)
    # compositing
    args = [_dev(torch, f[k]) for k in ("uv", "opacity", "conic", "rgb")]
    n, T, img = torch.zeros(H, W, dtype=torch.int32, device="cuda"), torch.zeros(H, W, device="cuda"), torch.zeros(H, W, 3, device="cuda")
    ops.render_image(*args, 0.5, _dev(torch, f["sorted"]), _dev(torch, f["ranges"]), W, H, n, T, img)
    if edge["size"] == "small":
        assert_image_close(_np(img), f["image"])
        assert_image_close(_np(T), f["T"], "final transmittance")
        assert_stop_indices_close(_np(n), f["n"])
    else:  # more borderline pixels than the absolute caps allow: each must be explained (see _check_edge_forward)
        got = dict(image=_np(img), T=_np(T), n=_np(n), sorted=f["sorted"], ranges=f["ranges"], radius=f["radius"])
        rep = parity_tools.forward_parity_report(got, f, W, H)
        parity_tools.explain(rep, got, f, W, H)
        _explained_image_bars(rep, got, f)
    g = [torch.zeros(M, 3, device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(M, 2, device="cuda"),
         torch.zeros(M, 3, device="cuda")]
    ops.render_image_backward(*args, 0.5, _dev(torch, f["sorted"]), _dev(torch, f["ranges"]), _dev(torch, f["n"]),
                              _dev(torch, f["T"]), _dev(torch, edge["gi"]), W, H, *g)
    for t, k in zip(g, ("rgb_pre", "opacity", "uv", "conic")):
        _per_population(_np(t), b[k], cp, "render backward " + k, size=edge["size"])


def test_edge_fused_matches_oracle(gpu, edge):
    """rasterize_image + backward_pass: the forward with the tight bookkeeping, every gradient per population, the rows
    that are visible but on no tile list exactly 0, arrays filled with NaN beforehand."""
    torch, raster = gpu, pkg("raster")
    ref, bref, cp, L = edge["ref"], edge["bref"], edge["cp"], edge["L"]
    ctx = raster.RasterContext(edge["N"], edge["W"], edge["H"])
    dp, dc = raster.device_params(edge["params"]), raster.device_camera(edge["cam"])
    gi = _dev(torch, edge["gi"])
    for it in range(3):  # the large scene's third forward is split into segments, its backwards from the second on
        fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
        _check_edge_forward(fwd, ref, edge["size"])
        assert (np.isnan(_np(fwd["radius"])) == np.isnan(ref["radius"])).all()
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        ctx.backward_pass(dp, dc, gi, C["bg"], L, grads)
        torch.cuda.synchronize()
        _check_backward(grads, bref)
        for k, rk in LEAVES + (("conic", "conic"), ("uv", "uv"), ("J", "J"), ("sigma", "sigma"), ("xyz_c", "xyz_c"),
                               ("precompute_rgb", "rgb_pre")):
            if grads.get(k) is None or bref.get(rk) is None:
                continue
            got = _np(grads[k]).reshape(len(bref[rk]), -1)
            _per_population(got, np.asarray(bref[rk]).reshape(len(got), -1), cp, f"grad_{k} (forward {it})",
                            size=edge["size"])
            off = ~edge["on_list"]
            assert (got[off] == 0).all(), f"grad_{k}: a visible row on no tile list got a gradient"
    if edge["size"] == "large":
        assert ctx.counters()["segmented_backwards"] >= 1 and ctx.counters()["segmented_forwards"] >= 1
    ctx.close()


def test_edge_lists_and_outputs_bit_identical_across_modes(gpu, edge):
    """Binning routes 0, 1, 2; preprocess split modes 0, 1, 2; lean and render-only contexts: the same bits."""
    torch, raster = gpu, pkg("raster")
    L = edge["L"]
    dp, dc = raster.device_params(edge["params"]), raster.device_camera(edge["cam"])
    keys = ("mask", "radius", "sorted", "ranges", "image", "T", "n")
    base = None
    variants = [("route", r) for r in (0, 1, 2)] + [("split", s) for s in (1, 2)] + [("lean", True), ("render_only", True)]
    for what, v in variants:
        ctx = raster.RasterContext(edge["N"], edge["W"], edge["H"])
        getattr(ctx, {"route": "set_binning_route", "split": "set_preprocess_split", "lean": "set_lean_forward",
                      "render_only": "set_render_only"}[what])(v)
        for _ in range(2):  # the second forward walks the compacted slots
            f = ctx.rasterize_image(dp, dc, C, C["bg"], L)
            got = {k: _np(f[k]).copy() for k in (keys if what != "render_only" else keys[2:])}
            if base is None:
                base = got
                _check_edge_forward(f, edge["ref"], edge["size"])
            for k in got:
                assert np.array_equal(got[k], base[k], equal_nan=True), f"{what}={v}: {k} differs"
        ctx.close()


def test_edge_backward_split_and_ranges_equal_the_whole(gpu, edge):
    """gsplat_backward_gaussians_range over ranges that start and end at every population boundary, and
    gsplat_backward_gaussians_split (the twelve columns of a view-sharded step at global indices), against the whole
    gsplat_backward_gaussians on the same compositing rows: bit for bit."""
    torch, raster = gpu, pkg("raster")
    N, L = edge["N"], edge["L"]
    ctx = raster.RasterContext(N, edge["W"], edge["H"])
    dp, dc = raster.device_params(edge["params"]), raster.device_camera(edge["cam"])
    gi = _dev(torch, edge["gi"])
    fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
    M = fwd["num_culled"]
    ctx.backward_render(gi, C["bg"])
    whole = ctx.alloc_gradients(N, L, intermediates=True)
    parts = ctx.alloc_gradients(N, L, intermediates=True)
    for t in list(whole.values()) + list(parts.values()):
        t.fill_(float("nan"))
    ctx.backward_gaussians(dp, dc, L, whole)
    bounds = sorted({0, N} | {int(r[0]) for r in edge["pops"].values() if len(r)} | {int(r[-1]) + 1 for r in edge["pops"].values() if len(r)})
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ctx.backward_gaussians_range(dp, dc, L, parts, lo, hi)
    torch.cuda.synchronize()
    for k in whole:
        assert torch.equal(whole[k][:M], parts[k][:M]), f"grad_{k}: ranges differ from the whole backward"
    _check_backward({k: whole[k][:M] for k in whole}, edge["bref"])
    # common[i] = {xyz 3, opacity, scale 3, quaternion 4, visible} at the global index i (gs_preprocess_bwd.hip: BwdOut)
    common = torch.full((N, 12), float("nan"), device="cuda")
    ctx.backward_gaussians_split(dp, dc, L, common)
    torch.cuda.synchronize()
    c2g = fwd["compact_to_global"].long()
    for k, (a, b) in (("xyz", (0, 3)), ("opacity", (3, 4)), ("scale", (4, 7)), ("quaternion", (7, 11))):
        assert torch.equal(common[c2g, a:b].reshape(whole[k][:M].shape), whole[k][:M]), f"split {k} differs"
    assert (common[c2g, 11] == 1).all()
    ctx.close()


def test_edge_depth_mode_matches_depth_reference(gpu, scene, orc):
    """Depth and alpha maps and every gradient with dL/d depth composed in, near-plane splats included."""
    torch, raster = gpu, pkg("raster")
    edge = _edge_case(scene, orc, "small")
    from test_depth_gpu import _check_depth, _check_grads, _maps
    N, W, H, L = edge["N"], edge["W"], edge["H"], edge["L"]
    ref, cam = edge["ref"], edge["cam"]
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True)
    dp, dc = raster.device_params(edge["params"]), raster.device_camera(cam)
    fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
    dref, aref = depth_reference.depth_alpha(orc, ref, W, H, threads=8)
    _check_depth(fwd, ref, dref.astype(np.float64), np.asarray(ref["image"], np.float64))
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
    for t in grads.values():
        t.fill_(float("nan"))
    ctx.backward_pass(dp, dc, _dev(torch, edge["gi"]), C["bg"], L, grads, grad_depth=gd_d, grad_alpha=ga_d)
    torch.cuda.synchronize()
    g = depth_reference.backward_pass(orc, ref, cam, edge["gi"], gd, ga, C["bg"], L, threads=8)
    _check_grads(grads, g)
    near = edge["cp"]["near"]
    assert_grad_close(_np(grads["xyz"])[near], g["xyz"][near], "grad_xyz [near]")
    ctx.close()

"""GPU tests of anti-aliased mode (gsplat_context_set_antialiased): image, transmittance, stop indices and every gradient
against the numpy reference on top of the float32 oracle (tests/antialias_reference.py); the two stand-alone operators;
lean against full contexts; the mode switched off again; depth and absgrad combinations; the edge populations; the
refusals; the split exchange; the Trainer."""
import numpy as np
import pytest

import absgrad_reference
import antialias_reference as aa
import depth_reference
from conftest import assert_grad_close, pkg
from test_fused_gpu import _check_forward

pytestmark = pytest.mark.gpu

LEAVES = (("xyz", "xyz"), ("rgb", "band0"), ("sh", "sh"), ("opacity", "opacity"), ("scale", "scale"),
          ("quaternion", "quaternion"))
INTERMEDIATES = (("conic", "conic"), ("uv", "uv"), ("J", "J"), ("sigma", "sigma"), ("xyz_c", "xyz_c"),
                 ("precompute_rgb", "rgb_pre"))


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _check_grads(grads, g, what=""):
    for k, rk in LEAVES + INTERMEDIATES:
        if grads.get(k) is not None and g.get(rk) is not None:
            want = np.asarray(g[rk])
            assert_grad_close(_np(grads[k]).reshape(want.shape), want, f"grad_{k}{what}")


def _population_close(got, want, pops, what):
    """All rows of the given populations together at conftest's bars (relative L2 and the element bar), then every
    population by itself at a relative L2 of 1e-3, so that a few dozen wrong edge rows cannot hide among thousands of
    ordinary ones.  The element bar is not
    repeated per population: conftest lets 5e-4 of the elements miss it, which in a population of 120 rows x 3 is no
    element at all, while the gradient here is a float32 sum of two terms of opposite sign (the conic's and the
    compensation's share) that may land 1e-3 off on a single small entry (measured: 1 of 360 scale and 2 of 720 J
    entries of one population).  A wrong branch or a dropped term moves whole rows, and with them the relative L2."""
    rows = np.sort(np.concatenate([np.asarray(r, np.int64) for r in pops.values() if len(r)]))
    assert_grad_close(got[rows], want[rows], what)
    for name, r in pops.items():
        if not len(r):
            continue
        a, b = np.asarray(got[r], np.float64), np.asarray(want[r], np.float64)
        assert np.isfinite(a).all(), f"{what} [{name}]: non-finite values"
        err = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
        assert err < 1e-3, f"{what} [{name}]: relative L2 error {err:.3e}"


SCENES = {"tiny": None, "small": None, "mid_l0": (3000, 200, 120, 0)}
_REFS = {}


def _scene_case(scene, orc, name, splat_scale, bg):
    """Parameters, camera and the reference's forward and backward, computed once per (scene, splat_scale, bg)."""
    key = (name, splat_scale, bg)
    if key not in _REFS:
        N, W, H, L = SCENES[name] if SCENES[name] else scene.WORKLOADS[name][:4]
        params = scene.make_gaussians(N, W, H, L, splat_scale=splat_scale)
        cam = scene.make_camera(W, H, 2)
        gi = scene.make_grad_image(W, H)
        plain, ref = aa.forward(orc, params, cam, scene.CONFIG, bg, L, threads=8)
        g = aa.backward(orc, ref, cam, gi, bg, L, threads=8)
        _REFS[key] = dict(N=N, W=W, H=H, L=L, params=params, cam=cam, gi=gi, plain=plain, ref=ref, g=g)
    return _REFS[key]


PARITY = [(n, s, b) for n in SCENES for s in (1.0, 0.25) for b in (0.0, 0.5)]


@pytest.mark.parametrize("name,splat_scale,bg", PARITY, ids=[f"{n}-s{s}-bg{b}" for n, s, b in PARITY])
def test_image_and_gradients_match_the_reference(gpu, scene, orc, name, splat_scale, bg):
    torch, raster = gpu, pkg("raster")
    case = _scene_case(scene, orc, name, splat_scale, bg)
    N, W, H, L, ref = case["N"], case["W"], case["H"], case["L"], case["ref"]
    dp, dc = raster.device_params(case["params"]), raster.device_camera(case["cam"])
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)
    for it in range(2):  # the second forward walks the compacted slots where the view culls enough
        fwd = ctx.rasterize_image(dp, dc, c, bg, L)
        _check_forward(fwd, ref)  # image, T, stop indices at the conftest bars; the lists explain every pixel beyond them
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        ctx.backward_pass(dp, dc, _dev(torch, case["gi"]), bg, L, grads)
        torch.cuda.synchronize()
        _check_grads(grads, case["g"], f" (forward {it})")
    # the mode does something here: the plain image is another image
    diff = np.abs(_np(fwd["image"]).astype(np.float64) - case["plain"]["image"]).sum(-1).max()
    print(f"{name} splat_scale {splat_scale} bg {bg}: plain and anti-aliased images differ by up to {diff:.3f} per pixel; "
          f"median rho {np.median(ref['rho']):.3f}, min {ref['rho'].min():.3f}")
    assert diff > 0.05
    ctx.close()


@pytest.mark.parametrize("name", ["tiny", "small"])  # M = 200 (one partial block) and 5000 (nineteen blocks and a partial one)
def test_stand_alone_operators(gpu, scene, orc, name):
    torch, ops = gpu, pkg("ops")
    case = _scene_case(scene, orc, name, 0.25, 0.5)
    f, cam = case["plain"], case["cam"]
    M = f["num_culled"]
    assert M % 256 != 0
    view = _dev(torch, cam["view"])
    xyz_c, sigma = _dev(torch, f["xyz_c"]), _dev(torch, f["sigma"])
    out = {}
    for which in ("plain", "aa"):
        J, conic, radius = torch.empty(M, 6, device="cuda"), torch.empty(M, 3, device="cuda"), torch.empty(M, 4, device="cuda")
        rho = torch.full((M + 1,), 7.0, device="cuda")
        args = (xyz_c, view, sigma, cam["fx"], cam["fy"], f["tan_fovx"], f["tan_fovy"], 3.0, M, J, conic, radius)
        if which == "aa":
            ops.compute_conic_antialiased(*args, rho)
        else:
            ops.compute_conic(*args)
        out[which] = (J, conic, radius, rho)
    torch.cuda.synchronize()
    for a, b in zip(out["plain"][:3], out["aa"][:3]):  # conic, radii, J untouched
        assert torch.equal(a, b)
    got = _np(out["aa"][3])
    assert got[M] == 7.0, "wrote past the last gaussian"
    want = aa.compensation(f["J"], f["sigma"], cam["view"])
    bound = aa.compensation_bound(f["J"], f["sigma"], cam["view"])
    err = np.abs(got[:M].astype(np.float64) - want)
    print(f"{name}: compensation off by at most {np.max(err / want):.2e} relative; the float32 bound allows "
          f"{np.max(bound / want):.2e}")
    assert (err <= bound).all()
    assert ((got[:M] >= 0) & (got[:M] <= 1)).all()
    # backward: random conic and compensation gradients
    rng = np.random.default_rng(5)
    gc = rng.normal(size=(M, 3)).astype(np.float32)
    gr = rng.normal(size=M).astype(np.float32)
    gJ0, gS0 = rng.normal(size=(M, 6)).astype(np.float32), rng.normal(size=(M, 6)).astype(np.float32)  # "+=" semantics
    gJ, gS = _dev(torch, gJ0), _dev(torch, gS0)
    ops.compute_conic_antialiased_backward(_dev(torch, f["J"]), sigma, view, _dev(torch, f["conic"]), _dev(torch, gc),
                                           _dev(torch, gr), M, gJ, gS)
    torch.cuda.synchronize()
    rJ, rS = orc.compute_conic_backward(f["J"], f["sigma"], cam["view"], f["conic"], gc, None, None, np.float64)
    dJ, dS = aa.compensation_backward(f["J"], f["sigma"], cam["view"], gr)
    assert_grad_close(_np(gJ) - gJ0, rJ + dJ, "J_grad")
    assert_grad_close(_np(gS) - gS0, rS + dS, "sigma_grad")
    # the compensation term alone (zero conic gradient), so that it cannot hide behind the conic's
    gJ, gS = torch.zeros(M, 6, device="cuda"), torch.zeros(M, 6, device="cuda")
    ops.compute_conic_antialiased_backward(_dev(torch, f["J"]), sigma, view, _dev(torch, f["conic"]),
                                           torch.zeros(M, 3, device="cuda"), _dev(torch, gr), M, gJ, gS)
    assert_grad_close(_np(gJ), dJ, "J_grad, compensation term")
    assert_grad_close(_np(gS), dS, "sigma_grad, compensation term")


def test_lean_and_full_contexts_give_the_same_bits(gpu, scene):
    """Image, T and stop indices bit for bit, and every gradient bit for bit on image gradients with ONE non-zero pixel:
    the compositing backward adds a gaussian's tiles into its row with float atomics, in arrival order, so two launches
    agree bitwise only where every row receives a single non-zero addend.  The per-gaussian backward -- the part the
    mode changes, which recomputes rho in both kinds of context -- is deterministic."""
    torch, raster = gpu, pkg("raster")
    N, W, H, L = scene.WORKLOADS["small"][:4]
    params = scene.make_gaussians(N, W, H, L, splat_scale=0.25)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 2))
    c = scene.CONFIG
    gi = torch.zeros(H, W, 3, device="cuda")
    out = {}
    for lean in (False, True):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_antialiased(True)
        ctx.set_lean_forward(lean)
        res = []
        for py, px in ((H // 2, W // 2), (5, 7), (H - 3, W - 2)):
            gi.zero_()
            gi[py, px] = torch.tensor([0.7, -0.4, 0.2], device="cuda")
            f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
            g = ctx.alloc_gradients(f["num_culled"], L)
            ctx.backward_pass(dp, dc, gi, c["bg"], L, g)
            torch.cuda.synchronize()
            res.append(({k: f[k].clone() for k in ("image", "T", "n")}, {k: v.clone() for k, v in g.items()}))
        out[lean] = res
        ctx.close()
    moved = 0
    for (fa, ga), (fb, gb) in zip(out[False], out[True]):
        for k in fa:
            assert torch.equal(fa[k], fb[k]), k
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k
        moved += int((ga["scale"] != 0).any(1).sum())
    assert moved > 0


def test_mode_off_is_the_parent_bit_for_bit(gpu, scene):
    """A context that never heard of the mode against one that had it set, used and cleared: image, T, n, lists and --
    on one pixel's gradient, where no row receives two addends -- every gradient."""
    torch, raster = gpu, pkg("raster")
    N, W, H, L = scene.WORKLOADS["small"][:4]
    params = scene.make_gaussians(N, W, H, L)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 2))
    c = scene.CONFIG
    gi = torch.zeros(H, W, 3, device="cuda")
    gi[H // 2, W // 2] = torch.tensor([0.7, -0.4, 0.2], device="cuda")
    out = []
    for touched in (False, True):
        ctx = raster.RasterContext(N, W, H)
        if touched:
            ctx.set_antialiased(True)
            f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
            ctx.backward_pass(dp, dc, gi, c["bg"], L, ctx.alloc_gradients(f["num_culled"], L))
            ctx.set_antialiased(False)
        for _ in range(2):
            f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
            g = ctx.alloc_gradients(f["num_culled"], L, intermediates=True)
            ctx.backward_pass(dp, dc, gi, c["bg"], L, g)
            torch.cuda.synchronize()
        out.append(({k: f[k].clone() for k in ("image", "T", "n", "sorted", "ranges", "radius", "conic")},
                    {k: v.clone() for k, v in g.items()}))
        ctx.close()
    for k, v in out[0][0].items():
        assert torch.equal(v, out[1][0][k]), k
    for k, v in out[0][1].items():
        assert torch.equal(v, out[1][1][k]), k
    assert bool((out[0][1]["opacity"] != 0).any())


def test_depth_and_absgrad_combination(gpu, scene, orc):
    """set_depth + grad_depth / grad_alpha + set_absgrad in anti-aliased mode: the kDepthRow and kAbsRow forms of the
    per-gaussian backward, against the depth and absgrad references on the substituted logits."""
    from test_depth_gpu import _maps
    torch, raster = gpu, pkg("raster")
    case = _scene_case(scene, orc, "mid_l0", 0.25, 0.5)
    N, W, H, L, ref, cam, gi = case["N"], case["W"], case["H"], case["L"], case["ref"], case["cam"], case["gi"]
    c, bg = scene.CONFIG, 0.5
    dp, dc = raster.device_params(case["params"]), raster.device_camera(cam)
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)
    ctx.set_depth(True)
    ctx.set_absgrad(True)
    fwd = ctx.rasterize_image(dp, dc, c, bg, L)
    dref, aref = depth_reference.depth_alpha(orc, ref, W, H, threads=8)
    np.testing.assert_allclose(_np(fwd["alpha"]), aref, rtol=0, atol=2e-5)
    np.testing.assert_allclose(_np(fwd["depth"]), dref, rtol=1e-4, atol=2e-4)
    z = np.asarray(ref["xyz_c"])[:, 2]
    for with_maps in (True, False):  # kDepthRow + kAbsRow, then kAbsRow alone
        GD, GA = (gd, ga) if with_maps else (None, None)
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        ctx.backward_pass(dp, dc, _dev(torch, gi), bg, L, grads, grad_depth=gd_d if with_maps else None,
                          grad_alpha=ga_d if with_maps else None)
        torch.cuda.synchronize()
        base = (lambda r: depth_reference.backward_pass(orc, r, cam, gi, GD, GA, bg, L, threads=8)) if with_maps else None
        g = aa.backward(orc, ref, cam, gi, bg, L, threads=8, base=base)
        _check_grads(grads, g, " (depth + absgrad)" if with_maps else " (absgrad)")
        kw = dict(grad_depth=GD, grad_alpha=GA, z=z) if with_maps else {}
        signed, absolute = absgrad_reference.absgrad_sums(ref, gi, W, H, bg, dtype=np.float64, **kw)
        assert_grad_close(_np(ctx.absgrad_uv()), absolute, "abs_uv")
        assert_grad_close(_np(grads["uv"]), signed, "grad_uv")
    # the kDepthRow form alone
    ctx.set_absgrad(False)
    fwd = ctx.rasterize_image(dp, dc, c, bg, L)
    grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
    ctx.backward_pass(dp, dc, _dev(torch, gi), bg, L, grads, grad_depth=gd_d, grad_alpha=ga_d)
    torch.cuda.synchronize()
    _check_grads(grads, aa.backward(orc, ref, cam, gi, bg, L, threads=8,
                                    base=lambda r: depth_reference.backward_pass(orc, r, cam, gi, gd, ga, bg, L, threads=8)),
                 " (depth)")
    ctx.close()


def test_edge_populations(gpu, scene, orc):
    """Clamped, near-plane, NaN-radius, needle, unnormalised and saturated splats in anti-aliased mode: the image at the
    conftest bars, the NaN pattern of the radii passed through, every gradient per population with no non-finite value
    (assert_grad_close checks it; the reference has none), visible rows on no list exactly 0, and the saturated
    population (sigma == 1 in float32, rho < 1) with the gradient the reference gives it."""
    import edge_scenes as es
    from test_edge_scenes_gpu import C, _edge_case
    torch, raster = gpu, pkg("raster")
    edge = _edge_case(scene, orc, "small")
    N, W, H, L, cam, gi, cp = edge["N"], edge["W"], edge["H"], edge["L"], edge["cam"], edge["gi"], edge["cp"]
    plain = edge["ref"]
    rho = aa.compensation(plain["J"], plain["sigma"], cam["view"])
    ref = dict(plain, logit=np.asarray(plain["opacity"], np.float32), rho=rho)
    ref["opacity"] = aa.effective_logit(ref["logit"], rho)
    ref["n"], ref["T"], ref["image"] = orc.render_image(plain["uv"], ref["opacity"], plain["conic"], plain["rgb"], C["bg"],
                                                       plain["sorted"], plain["ranges"], W, H, np.float32, 8)
    g = aa.backward(orc, ref, cam, gi, C["bg"], L, threads=8, tan_fov=es.backward_tan_fov(cam), sigma_dtype=np.float32)
    for k, v in g.items():
        if v is not None:
            assert np.isfinite(v).all(), f"the reference's grad_{k} has a non-finite value"
    # Where float32 cannot hold rho: det0 = a c - b^2 of a needle or a flat splat cancels, so rho evaluated with every
    # product rounded to float32 is off by up to 2e-2 of itself (needle) and 6e-4 (flat) against the float64 evaluation of
    # the same float32 J and Sigma -- the number format's doing, whatever the order of the sums.  o, dL/d rho = k / rho and
    # d rho/d cov ~ 1 / rho scale with it, so such a population is held to a relative L2 bar of 1e-3 plus TWICE that
    # difference (the kernel and this float32 evaluation each carry it), computed here from the inputs alone; a wrong
    # branch or a dropped term is an O(1) error.  Their rows stay out of the element bar altogether: the definition's chain
    # evaluated in numpy with every operation rounded to float32 already puts 44 of the 25 962 grad_sigma entries outside
    # it, every one of them a needle's (the kernel: 28).  Every other population, and all their rows together:
    # _population_close.
    rho32 = aa.compensation(plain["J"], plain["sigma"], cam["view"], np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        rho_err = np.where(rho > 0, np.abs(rho32 - rho) / rho, 0.0)
    loose = {k: 1e-3 + 2 * float(rho_err[r].max()) for k, r in cp.items() if len(r) and rho_err[r].max() > 1e-4}
    print("populations beyond float32's rho, their relative L2 bars:", {k: f"{v:.1e}" for k, v in loose.items()})
    assert set(loose) <= {"needle", "flat"}
    tight = {k: r for k, r in cp.items() if k not in loose}
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)
    dp, dc = raster.device_params(edge["params"]), raster.device_camera(cam)
    for it in range(2):
        fwd = ctx.rasterize_image(dp, dc, C, C["bg"], L)
        _check_forward(fwd, ref)
        assert (np.isnan(_np(fwd["radius"])) == np.isnan(plain["radius"])).all()
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=True)
        for t in grads.values():
            t.fill_(float("nan"))
        ctx.backward_pass(dp, dc, _dev(torch, gi), C["bg"], L, grads)
        torch.cuda.synchronize()
        for k, rk in LEAVES + INTERMEDIATES:
            if grads.get(k) is None or g.get(rk) is None:
                continue
            want = np.asarray(g[rk]).reshape(fwd["num_culled"], -1)
            got = _np(grads[k]).reshape(want.shape)
            pops = tight
            if k == "opacity":
                # dL/d logit = k (1 - sigma) with sigma held in float32: two correct float32 sigmoids may differ by an ulp
                # (2^-24 next to 1), i.e. by eps32 |k| in this product, which in the saturated population (1 - sigma down
                # to 2e-9) is more than 1e-3 of the value.  Those rows: the element bar plus that rounding on both sides;
                # where float32 rounds sigma to 1 the reference is an exact 0 and so must the kernel's value be.
                pops = {p: r for p, r in tight.items() if p != "saturated"}
                sat, eps = cp["saturated"], float(np.finfo(np.float32).eps)
                a, b = got[sat, 0].astype(np.float64), want[sat, 0]
                assert np.isfinite(a).all()
                tol = 1e-3 * np.abs(b) + 1e-3 * np.abs(b).mean() + 2 * eps * np.abs(g["k"][sat])
                assert (np.abs(a - b) <= tol).all(), f"grad_opacity (forward {it}) [saturated]"
                one = aa.sigmoid(ref["logit"][sat]).astype(np.float32) == 1
                assert one.any() and (a[one] == 0).all() and (b[one] == 0).all(), "the sigma == 1 guard"
            _population_close(got, want, pops, f"grad_{k} (forward {it})")
            for pop, bar in loose.items():
                a, b = got[cp[pop]].astype(np.float64), want[cp[pop]]
                assert np.isfinite(a).all(), f"grad_{k} [{pop}]: non-finite values"
                err = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
                assert err < bar, f"grad_{k} (forward {it}) [{pop}]: relative L2 error {err:.3e} (bar {bar:.1e})"
            assert (got[~edge["on_list"]] == 0).all(), f"grad_{k}: a visible row on no tile list got a gradient"
    sat = cp["saturated"]
    assert len(sat) and (aa.sigmoid(ref["logit"][sat]).astype(np.float32) == 1).any()
    ctx.close()


def test_refusals_leave_the_context_usable(gpu, scene):
    torch, raster, lib, opt_mod = gpu, pkg("raster"), pkg("_lib"), pkg("optimizer")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    params = scene.make_gaussians(N, W, H, L, splat_scale=0.25)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 2))
    c = scene.CONFIG
    gi = _dev(torch, scene.make_grad_image(W, H))
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)

    def good():
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        g = ctx.alloc_gradients(f["num_culled"], L)
        ctx.backward_pass(dp, dc, gi, c["bg"], L, g)
        torch.cuda.synchronize()
        return f["image"].clone(), {k: v.clone() for k, v in g.items()}

    image, grads = good()

    def refused(call):
        with pytest.raises(lib.GsplatError) as e:
            call()
        assert e.value.code == -3  # GSPLAT_ERR_INVALID_ARG
        again, g2 = good()
        assert torch.equal(again, image)
        for k in grads:  # (two compositing backwards: the rows carry the order of their float atomics)
            assert_grad_close(_np(g2[k]), _np(grads[k]), k, rel=1e-5)

    for mode in (0, 1, 2):  # the three Adam-inside forms; parameters and moments must come back untouched
        p = {k: v.clone() for k, v in dp.items()}
        opt = opt_mod.AdamOptimizer(p, L, scene_extent=2.5)
        before = {k: v.clone() for k, v in p.items()}
        M = ctx._last[1]
        g2 = dict(xyz=torch.empty(M, 3, device="cuda"), precompute_rgb=torch.empty(M, 3, device="cuda")) if mode == 1 else None
        refused(lambda: ctx.backward_gaussians_adam(p, dc, L, opt.fused_state(1, mode=mode), g2))
        for k in before:
            assert torch.equal(before[k], p[k]), (mode, k)
        assert int(opt.grad_accum_dur.sum()) == 0
    refused(lambda: ctx.backward_gaussians_camera(dp, dc, L))
    refused(lambda: ctx.backward_pass_camera(dp, dc, gi, c["bg"], L))
    for split in (1, 2):
        ctx.set_preprocess_split(split)
        with pytest.raises(lib.GsplatError) as e:
            ctx.rasterize_image(dp, dc, c, c["bg"], L)
        assert e.value.code == -3
        ctx.set_preprocess_split(0)
        again, _ = good()
        assert torch.equal(again, image)
    # with the mode off again all of them serve
    ctx.set_antialiased(False)
    ctx.rasterize_image(dp, dc, c, c["bg"], L)
    ctx.backward_pass_camera(dp, dc, gi, c["bg"], L)
    ctx.close()


def test_split_exchange_equals_backward_and_pack(gpu, scene):
    """backward_gaussians_split (whole and in ranges) in anti-aliased mode against backward_gaussians + pack, on the same
    compositing rows: bit for bit, as tests/test_dist_gpu.py checks for the plain form."""
    torch, raster = gpu, pkg("raster")
    N, W, H, L = 3000, 200, 120, 2
    params = scene.cull_half(scene.make_gaussians(N, W, H, L, splat_scale=0.25), fraction=0.3)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 2))
    c = scene.CONFIG
    gi = _dev(torch, scene.make_grad_image(W, H))
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)
    ctx.set_lean_forward(True)
    for _ in range(2):  # the second forward walks the compacted slots
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    assert ctx.counters()["compact_walks"] >= 1
    ctx.backward_render(gi, c["bg"])
    nan = float("nan")
    com_w, uv_w = torch.zeros(N, 12, device="cuda"), torch.zeros(N, device="cuda")
    ctx.backward_gaussians_split(dp, dc, L, com_w, uv_w)
    com_r, uv_r = torch.zeros(N, 12, device="cuda"), torch.zeros(N, device="cuda")
    for lo, hi in ((0, 700), (700, 701), (701, 2200), (2200, N)):
        ctx.backward_gaussians_split(dp, dc, L, com_r, uv_r, lo, hi)
    g = ctx.alloc_gradients(N, L, intermediates=("uv", "precompute_rgb"))
    ctx.backward_gaussians(dp, dc, L, g)
    com_p, rgb_p, uv_p = torch.full((N, 12), nan, device="cuda"), torch.full((N + 1, 3), nan, device="cuda"), torch.full((N,), nan, device="cuda")
    raster.pack_gradients_split(ctx, g, N, com_p, rgb_p)
    raster.pack_uv_grad_norm(ctx, g, N, uv_p)
    parts = ctx.alloc_gradients(N, L, intermediates=("uv", "precompute_rgb"))
    for lo, hi in ((0, 1500), (1500, N)):
        ctx.backward_gaussians_range(dp, dc, L, parts, lo, hi)
    torch.cuda.synchronize()
    assert torch.equal(com_r, com_w) and torch.equal(uv_r, uv_w), "the ranges do not add up to the whole backward"
    assert torch.equal(com_w, com_p) and torch.equal(uv_w, uv_p), "direct global-order rows differ from the packed compacted ones"
    M = fwd["num_culled"]
    for k in g:
        assert torch.equal(g[k][:M], parts[k][:M]), k
    assert bool((com_w[:, 3] != 0).any())
    ctx.close()


def test_trainer_takes_the_unfused_path_and_learns(gpu, scene, monkeypatch):
    from test_absgrad_gpu import _training_setup
    torch, trainer_mod, raster, ops = gpu, pkg("trainer"), pkg("raster"), pkg("ops")
    init, views, cfg = _training_setup(torch, scene)
    monkeypatch.setenv("GSPLAT_FUSED_ADAM", "1")
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, antialiased=True), scene_extent=5.0, seed=3)
    assert t.fused_adam == 0
    calls = dict(adam=0, plain=0)
    real_adam, real_plain = t.ctx.backward_gaussians_adam, t.ctx.backward_pass

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    t.ctx.backward_gaussians_adam = count("adam", real_adam)
    t.ctx.backward_pass = count("plain", real_plain)
    hist = t.train(30, loss_every=1)
    assert calls == dict(adam=0, plain=30)
    losses = [h[1] for h in hist]
    print(f"anti-aliased training: loss {np.mean(losses[:5]):.4f} -> {np.mean(losses[-5:]):.4f}")
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    # evaluate renders in the mode the run trains in
    psnr = t.evaluate(views)
    want = {}
    for mode in (True, False):
        ctx = raster.RasterContext(t.num_gaussians, t.ctx.max_width, t.ctx.max_height)
        ctx.set_antialiased(mode)
        ctx.set_render_only(True)
        total = 0.0
        for cam, gt in views:
            f = ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)
            total += ops.compute_psnr(f["image"], gt, int(cam["height"]), int(cam["width"]))
        want[mode] = total / len(views)
        ctx.close()
    assert psnr == want[True] and psnr != want[False], (psnr, want)

"""GPU tests of the 3D smoothing filter: the three operators against the float64 references (tests/filter3d_reference.py),
the context mode (gsplat_context_set_filter3d) against its parts bit for bit and against the float64 oracle end to end,
the split / range / camera backwards, the refusals, switching off, and the Trainer.

Bitwise comparisons of gradients between TWO compositing backwards use image gradients with one non-zero pixel: the
compositing backward adds a gaussian's tiles into its row with float atomics in arrival order, so two launches agree
bit for bit only where every row receives a single addend (tests/test_antialias_gpu.py::
test_lean_and_full_contexts_give_the_same_bits).  Comparisons on ONE set of compositing rows are bitwise on a dense image
gradient."""
import numpy as np
import pytest

import filter3d_reference as f3
from conftest import assert_grad_close, pkg

pytestmark = pytest.mark.gpu

LEAVES = ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")
N, W, H, L = 3000, 200, 120, 2
PIXELS = ((H // 2, W // 2), (5, 7), (H - 3, W - 2))

# relative L2 error of gsplat_filter3d_apply_backward against the float64 reference, per population: four times what was
# measured on MI355X ("3D smoothing filter"), and never looser than the project's gradient bar
MEASURED_BWD = {"f<<s": 7.3e-8, "f~s": 7.9e-8, "f>>s": 5.5e-8, "logit>8": 2.2e-7}  # the larger of grad_scale's and grad_opacity's
BWD_BARS = {k: min(4 * v, 1e-3) for k, v in MEASURED_BWD.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-300))


_CASE = {}


def _case(torch, scene):
    """One scene for the context tests: 3000 gaussians at 200x120, SH degree 2, a third behind the camera, and the filter
    three cameras give it (computed once)."""
    if not _CASE:
        raster, ops = pkg("raster"), pkg("ops")
        params = scene.cull_half(scene.make_gaussians(N, W, H, L, splat_scale=0.5), fraction=0.3)
        cams = [scene.make_camera(W, H, k) for k in (1, 2, 3)]
        dp = raster.device_params(params)
        filt = ops.compute_filter3d(dp["xyz"], *ops.camera_arrays(cams), near=f3.NEAR)
        se, oe = ops.filter3d_apply(dp["scale"], dp["opacity"], filt)
        torch.cuda.synchronize()
        _CASE.update(params=params, cam=scene.make_camera(W, H, 2), dp=dp, filt=filt, sub=dict(dp, scale=se, opacity=oe),
                     gi=_dev(torch, scene.make_grad_image(W, H)))
        s = np.exp(params["scale"].astype(np.float64))
        ratio = _np(filt).astype(np.float64)[:, None] / s
        print(f"context scene: filter3d / exp(scale) between {ratio.min():.2f} and {ratio.max():.2f}, median {np.median(ratio):.2f}")
        assert 0.05 < np.median(ratio) < 20  # the filter matters here and does not swamp the gaussians
    return _CASE


def _pixel_gi(torch, py, px):
    gi = torch.zeros(H, W, 3, device="cuda")
    gi[py, px] = torch.tensor([0.7, -0.4, 0.2], device="cuda")
    return gi


# ------------------------------------------------------------------------------------------------ 1: compute_filter3d
def test_compute_filter3d_matches_the_reference(gpu, scene):
    torch, ops = gpu, pkg("ops")
    xyz, cams, pops = f3.make_scene(scene)
    want, sampled, _ = f3.compute_filter3d(xyz, cams, f3.NEAR)
    frag = f3.fragile(xyz, cams, f3.NEAR)
    assert frag.mean() <= 0.01
    n = len(xyz)
    assert n % 256 != 0 and n > 256
    dx, arrays = _dev(torch, xyz), ops.camera_arrays(cams)
    runs = []
    for _ in range(2):
        out = torch.full((n + 1,), 7.0, device="cuda")
        ops.compute_filter3d(dx, *arrays, near=f3.NEAR, out=out)
        torch.cuda.synchronize()
        runs.append(_np(out))
    assert runs[0][n] == 7.0, "wrote past the last gaussian"
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), "two runs differ"
    got = runs[0][:n]
    ok = ~frag
    rel = np.abs(got[ok & sampled].astype(np.float64) - want[ok & sampled]) / want[ok & sampled]
    print(f"filter3d on sampled rows: off by at most {rel.max():.2e} relative")
    assert rel.max() <= 1e-5
    # the GPU's maximum is attained on a sampled row, and every unsampled row carries exactly it
    top = got.max()
    assert top == got[sampled & ok].max() and abs(float(top) - want.max()) <= 1e-5 * want.max()
    assert (got[ok & ~sampled].view(np.uint32) == np.float32(top).view(np.uint32)).all()
    assert (~sampled & ok).sum() >= 400 and (got[ok & sampled] < top).sum() > 2000
    # more cameras than one staged chunk holds, the only camera that sees the `one` population last: the same bits
    many = (cams[:4] * 18)[:69] + [cams[4]]
    more = ops.compute_filter3d(dx, *ops.camera_arrays(many), near=f3.NEAR)
    assert np.array_equal(_np(more).view(np.uint32), got.view(np.uint32))
    # one camera
    w1, s1, _ = f3.compute_filter3d(xyz, cams[:1], f3.NEAR)
    g1 = _np(ops.compute_filter3d(dx, *ops.camera_arrays(cams[:1]), near=f3.NEAR))
    ok1 = ~f3.fragile(xyz, cams[:1], f3.NEAR)
    np.testing.assert_allclose(g1[ok1 & s1], w1[ok1 & s1], rtol=1e-5)
    assert (g1[ok1 & ~s1] == g1.max()).all() and s1.any() and not s1.all()
    # nothing sampled: zeros
    behind = _dev(torch, xyz[pops["behind"]])
    g0 = ops.compute_filter3d(behind, *arrays, near=f3.NEAR, out=torch.full((len(pops["behind"]),), 7.0, device="cuda"))
    assert bool((g0 == 0).all())


# ------------------------------------------------------------------------------------------------ 2: filter3d_apply
def test_filter3d_apply_matches_the_reference(gpu):
    torch, ops = gpu, pkg("ops")
    scale, opacity, f, pops = f3.transform_rows()
    n = len(f)
    assert n % 256 != 0
    want_s, want_o, o_ref, _ = f3.apply(scale, opacity, f)
    se, oe = torch.full((n + 1, 3), 7.0, device="cuda"), torch.full((n + 1,), 7.0, device="cuda")
    ops.filter3d_apply(_dev(torch, scale), _dev(torch, opacity), _dev(torch, f), se, oe)
    torch.cuda.synchronize()
    se, oe = _np(se), _np(oe)
    assert (se[n] == 7.0).all() and oe[n] == 7.0, "wrote past the last gaussian"
    se, oe = se[:n], oe[:n]
    assert np.isfinite(se).all() and np.isfinite(oe).all()
    err_s = np.abs(se.astype(np.float64) - want_s) / np.maximum(1.0, np.abs(want_s))
    o_got = 1.0 / (1.0 + np.exp(-oe.astype(np.float64)))
    err_o = np.abs(o_got - o_ref) / o_ref
    for name, rows in pops.items():
        print(f"{name}: scale_eff off by {err_s[rows].max():.2e}, sigmoid(opacity_eff) by {err_o[rows].max():.2e} relative")
    assert err_s.max() <= 1e-5 and err_o.max() <= 1e-5
    zero = pops["f=0"]
    assert np.array_equal(se[zero].view(np.uint32), scale[zero].view(np.uint32))
    assert np.array_equal(oe[zero].view(np.uint32), opacity[zero].view(np.uint32))
    # logits up to 20 with f > 0, across f << s .. f >> s: finite, and o <= sigma
    m = 1000
    rng = np.random.default_rng(8)
    sc = rng.uniform(-6, 1, (m, 3)).astype(np.float32)
    ff = np.exp(sc.mean(1) + rng.uniform(-12, 8, m)).astype(np.float32)
    op = np.linspace(12.0, 20.0, m).astype(np.float32)
    se2, oe2 = ops.filter3d_apply(_dev(torch, sc), _dev(torch, op), _dev(torch, ff))
    assert bool(torch.isfinite(se2).all()) and bool(torch.isfinite(oe2).all())
    assert bool((oe2 <= _dev(torch, op) * (1 + 1e-6)).all()) and bool((se2 >= _dev(torch, sc)).all())  # (logit rounded: an ulp)


# ------------------------------------------------------------------------------------------------ 3: the chain rule
def test_filter3d_apply_backward_matches_the_reference(gpu):
    torch, ops = gpu, pkg("ops")
    scale, opacity, f, pops = f3.transform_rows()
    n = len(f)
    rng = np.random.default_rng(4)
    rows = rng.permutation(n)[:1900].astype(np.int32)  # gradient row j belongs to gaussian rows[j]
    M = len(rows)
    g_s = rng.normal(size=(M, 3)).astype(np.float32)
    g_o = rng.normal(size=M).astype(np.float32)
    want_s, want_o = f3.apply_backward(scale[rows], opacity[rows], f[rows], g_s, g_o)
    ds, do, df, dr = _dev(torch, scale), _dev(torch, opacity), _dev(torch, f), _dev(torch, rows, np.int32)
    # compacted layout: [M,3] and [M]
    a_s, a_o = torch.full((M + 1, 3), 7.0, device="cuda"), torch.full((M + 1,), 7.0, device="cuda")
    a_s[:M], a_o[:M] = _dev(torch, g_s), _dev(torch, g_o)
    ops.filter3d_apply_backward(ds, do, df, a_s[:M], a_o[:M], dr)
    # strided layout: columns 4..6 and 3 of twelve-float rows, in a buffer with more rows than are listed
    rows12 = rng.normal(size=(n, 12)).astype(np.float32)
    rows12[:M, 4:7], rows12[:M, 3] = g_s, g_o
    b = _dev(torch, rows12)
    ops.filter3d_apply_backward(ds, do, df, b[:M, 4:7], b[:M, 3], dr)
    torch.cuda.synchronize()
    assert bool((a_s[M] == 7.0).all()) and float(a_o[M]) == 7.0
    a_s, a_o, b = _np(a_s)[:M], _np(a_o)[:M], _np(b)
    assert np.array_equal(b[:M, 4:7].view(np.uint32), a_s.view(np.uint32)) and np.array_equal(b[:M, 3].view(np.uint32), a_o.view(np.uint32))
    keep = np.ones(12, bool)
    keep[3:7] = False
    assert np.array_equal(b[:, keep].view(np.uint32), rows12[:, keep].view(np.uint32)), "another column was touched"
    assert np.array_equal(b[M:].view(np.uint32), rows12[M:].view(np.uint32)), "an unlisted row was touched"
    where = {int(g): j for j, g in enumerate(rows)}
    for name in ("f<<s", "f~s", "f>>s", "logit>8"):
        js = np.array([where[int(g)] for g in pops[name] if int(g) in where])
        assert len(js) > 100
        e_s, e_o = _rel_l2(a_s[js], want_s[js]), _rel_l2(a_o[js], want_o[js])
        print(f"{name}: grad_scale relative L2 error {e_s:.2e}, grad_opacity {e_o:.2e} (bar {BWD_BARS[name]:.1e})")
        assert np.isfinite(a_s[js]).all() and np.isfinite(a_o[js]).all()
        assert e_s <= BWD_BARS[name] and e_o <= BWD_BARS[name], name
        assert_grad_close(a_s[js], want_s[js], f"grad_scale [{name}]")
        assert_grad_close(a_o[js], want_o[js], f"grad_opacity [{name}]")
    js = np.array([where[int(g)] for g in pops["f=0"] if int(g) in where])
    assert len(js) and np.array_equal(a_s[js].view(np.uint32), g_s[js].view(np.uint32)) and np.array_equal(a_o[js], g_o[js])
    # rows == None: gradient row j is gaussian j
    c_s, c_o = _dev(torch, g_s[:700]), _dev(torch, g_o[:700])
    ops.filter3d_apply_backward(ds[:700], do[:700], df[:700], c_s, c_o)
    w_s, w_o = f3.apply_backward(scale[:700], opacity[:700], f[:700], g_s[:700], g_o[:700])
    assert_grad_close(_np(c_s), w_s, "grad_scale (rows = None)")
    assert_grad_close(_np(c_o), w_o, "grad_opacity (rows = None)")


# ------------------------------------------------------------------------------------------------ 4: the mode = its parts
@pytest.mark.parametrize("antialiased,depth", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "antialiased", "depth", "antialiased-depth"])
def test_mode_equals_its_parts_bit_for_bit(gpu, scene, antialiased, depth):
    torch, raster, ops = gpu, pkg("raster"), pkg("ops")
    case = _case(torch, scene)
    dp, sub, filt = case["dp"], case["sub"], case["filt"]
    dc, c = raster.device_camera(case["cam"]), scene.CONFIG
    on, off = raster.RasterContext(N, W, H), raster.RasterContext(N, W, H)
    for ctx in (on, off):
        ctx.set_antialiased(antialiased)
        ctx.set_depth(depth)
    before = on.workspace_bytes
    on.set_filter3d(filt)
    assert on.workspace_bytes == before == off.workspace_bytes  # the two arrays come with the first forward in the mode
    for it in range(2):  # the second forward walks the compacted slots
        fa, fb = on.rasterize_image(dp, dc, c, c["bg"], L), off.rasterize_image(sub, dc, c, c["bg"], L)
        torch.cuda.synchronize()
        for k in ("image", "T", "n", "sorted", "ranges", "radius", "compact_to_global") + (("depth",) if depth else ()):
            assert torch.equal(fa[k], fb[k]), (k, it)
    assert on.workspace_bytes >= off.workspace_bytes + 16 * N  # (both took what every first forward takes)
    M = fa["num_culled"]
    assert 0 < M < N
    c2g = fa["compact_to_global"]

    def both(gi, gd, ga):
        out = []
        for ctx, p in ((on, dp), (off, sub)):
            ctx.backward_render(gi, c["bg"], grad_depth=gd, grad_alpha=ga)
            g = ctx.alloc_gradients(M, L, intermediates=True)
            for t in g.values():
                t.fill_(float("nan"))
            ctx.backward_gaussians(p, dc, L, g)
            if ctx is off:
                ops.filter3d_apply_backward(dp["scale"], dp["opacity"], filt, g["scale"], g["opacity"], c2g)
            torch.cuda.synchronize()
            out.append(g)
        return out

    moved = 0
    for py, px in PIXELS:
        gd = ga = None
        if depth:
            gd, ga = torch.zeros(H, W, device="cuda"), torch.zeros(H, W, device="cuda")
            gd[py, px], ga[py, px] = 0.3, -0.6
        ga_, gb_ = both(_pixel_gi(torch, py, px), gd, ga)
        for k in ga_:
            assert torch.equal(ga_[k], gb_[k]), (k, py, px)
        moved += int((ga_["scale"] != 0).any(1).sum())
    assert moved > 0
    # a dense image gradient: two compositing backwards, so to rounding only -- but every visible row
    ga_, gb_ = both(case["gi"], None, None)
    for k in LEAVES:
        assert_grad_close(_np(ga_[k]), _np(gb_[k]), f"grad_{k}", rel=1e-5)
    # ... and the chain rule did something: the gradient with respect to scale_eff is another one
    raw = off.alloc_gradients(M, L)
    off.backward_gaussians(sub, dc, L, raw)
    assert _rel_l2(_np(raw["scale"]), _np(gb_["scale"])) > 1e-2
    on.close()
    off.close()


# ------------------------------------------------------------------------------------------------ 5: end to end
def test_gradients_match_the_float64_oracle(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    case = _case(torch, scene)
    params, cam, c, bg = case["params"], case["cam"], scene.CONFIG, 0.5
    filt = _np(case["filt"])
    se, oe, _, _ = f3.apply(params["scale"], params["opacity"], filt)
    eff = dict(params, scale=se.astype(np.float32), opacity=oe.astype(np.float32))
    gi = _np(case["gi"])
    ref = orc.rasterize(eff, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], bg, L, threads=8)
    g = orc.backward_pass(ref, cam, gi, bg, L, dtype=np.float64, threads=8)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_filter3d(case["filt"])
    dc = raster.device_camera(cam)
    fwd = ctx.rasterize_image(case["dp"], dc, c, bg, L)
    M = fwd["num_culled"]
    assert M == len(ref["xyz"])
    np.testing.assert_allclose(_np(fwd["image"]), ref["image"], rtol=0, atol=1e-4)
    grads = ctx.alloc_gradients(M, L)
    for t in grads.values():
        t.fill_(float("nan"))
    ctx.backward_pass(case["dp"], dc, case["gi"], bg, L, grads)
    torch.cuda.synchronize()
    rows = _np(fwd["compact_to_global"])
    want_s, want_o = f3.apply_backward(params["scale"][rows], params["opacity"][rows], filt[rows],
                                       np.asarray(g["scale"]).reshape(M, 3), np.asarray(g["opacity"]).reshape(M))
    assert_grad_close(_np(grads["scale"]), want_s, "grad_scale")
    assert_grad_close(_np(grads["opacity"]), want_o, "grad_opacity")
    assert _rel_l2(np.asarray(g["scale"]).reshape(M, 3), want_s) > 1e-2, "the chain rule changes nothing on this scene"
    for k, rk in (("xyz", "xyz"), ("rgb", "band0"), ("sh", "sh"), ("quaternion", "quaternion")):
        want = np.asarray(g[rk])
        assert_grad_close(_np(grads[k]).reshape(want.shape), want, f"grad_{k}")
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6: split and range
def test_split_and_range_equal_backward_and_pack(gpu, scene):
    torch, raster = gpu, pkg("raster")
    case = _case(torch, scene)
    dp, dc, c, gi = case["dp"], raster.device_camera(case["cam"]), scene.CONFIG, case["gi"]
    ctx = raster.RasterContext(N, W, H)
    ctx.set_filter3d(case["filt"])
    ctx.set_lean_forward(True)
    for _ in range(2):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    assert ctx.counters()["compact_walks"] >= 1
    ctx.backward_render(gi, c["bg"])
    nan = float("nan")
    com_w, uv_w = torch.zeros(N, 12, device="cuda"), torch.zeros(N, device="cuda")
    ctx.backward_gaussians_split(dp, dc, L, com_w, uv_w)
    com_r, uv_r = torch.zeros(N, 12, device="cuda"), torch.zeros(N, device="cuda")
    for lo, hi in ((0, 700), (700, 2200), (2200, N)):
        ctx.backward_gaussians_split(dp, dc, L, com_r, uv_r, lo, hi)
    g = ctx.alloc_gradients(N, L, intermediates=("uv", "precompute_rgb"))
    ctx.backward_gaussians(dp, dc, L, g)
    com_p, rgb_p, uv_p = torch.full((N, 12), nan, device="cuda"), torch.full((N + 1, 3), nan, device="cuda"), torch.full((N,), nan, device="cuda")
    raster.pack_gradients_split(ctx, g, N, com_p, rgb_p)
    raster.pack_uv_grad_norm(ctx, g, N, uv_p)
    parts = ctx.alloc_gradients(N, L, intermediates=("uv", "precompute_rgb"))
    for lo, hi in ((0, 1000), (1000, 1001), (1001, N)):
        ctx.backward_gaussians_range(dp, dc, L, parts, lo, hi)
    torch.cuda.synchronize()
    assert torch.equal(com_r, com_w) and torch.equal(uv_r, uv_w), "the ranges do not add up to the whole backward"
    assert torch.equal(com_w, com_p) and torch.equal(uv_w, uv_p), "direct global-order rows differ from the packed compacted ones"
    M = fwd["num_culled"]
    for k in g:
        assert torch.equal(g[k][:M], parts[k][:M]), k
    assert bool((com_w[:, 3] != 0).any()) and bool((com_w[:, 11] == 0).any())
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7: camera gradient
def test_camera_gradient_is_that_of_the_substituted_parameters(gpu, scene):
    torch, raster = gpu, pkg("raster")
    case = _case(torch, scene)
    dp, sub, dc, c = case["dp"], case["sub"], raster.device_camera(case["cam"]), scene.CONFIG
    on, off = raster.RasterContext(N, W, H), raster.RasterContext(N, W, H)
    on.set_filter3d(case["filt"])
    moved = dict.fromkeys((True, False), False)  # (a single pixel may lie under no gaussian: then both are zero)
    for gi, exact in [(_pixel_gi(torch, *p), True) for p in PIXELS] + [(case["gi"], False)]:
        res = []
        for ctx, p in ((on, dp), (off, sub)):
            ctx.rasterize_image(p, dc, c, c["bg"], L)
            _, gv, gc = ctx.backward_pass_camera(p, dc, gi, c["bg"], L)
            torch.cuda.synchronize()
            res.append((gv.clone(), gc.clone()))
        if exact:
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        else:  # (two compositing backwards of a dense image gradient: to rounding)
            assert_grad_close(_np(res[0][0]), _np(res[1][0]), "grad_view", rel=1e-5)
            assert_grad_close(_np(res[0][1]), _np(res[1][1]), "grad_campos", rel=1e-5)
        moved[exact] |= bool((res[0][0] != 0).any()) and bool((res[0][1] != 0).any())
    assert moved[True] and moved[False]
    # with gradient arrays too: the leaves of the camera form are those of the plain one
    fwd = on.rasterize_image(dp, dc, c, c["bg"], L)
    on.backward_render(case["gi"], c["bg"])
    a, b = on.alloc_gradients(fwd["num_culled"], L), on.alloc_gradients(fwd["num_culled"], L)
    on.backward_gaussians(dp, dc, L, a)
    on.backward_gaussians_camera(dp, dc, L, b)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    on.close()
    off.close()


# ------------------------------------------------------------------------------------------------ 8: refusals, off
def test_refusals_and_switching_off(gpu, scene):
    torch, raster, lib, opt_mod = gpu, pkg("raster"), pkg("_lib"), pkg("optimizer")
    case = _case(torch, scene)
    dp, dc, c = case["dp"], raster.device_camera(case["cam"]), scene.CONFIG
    gi = _pixel_gi(torch, *PIXELS[0])

    def run(ctx, p=dp):
        f = ctx.rasterize_image(p, dc, c, c["bg"], L)
        g = ctx.alloc_gradients(f["num_culled"], L, intermediates=True)
        ctx.backward_pass(p, dc, gi, c["bg"], L, g)
        torch.cuda.synchronize()
        return {k: f[k].clone() for k in ("image", "T", "n", "sorted", "ranges")}, {k: v.clone() for k, v in g.items()}

    def same(a, b):
        for part_a, part_b in zip(a, b):
            for k in part_a:
                assert torch.equal(part_a[k], part_b[k]), k

    parent = raster.RasterContext(N, W, H)  # a context that never heard of the mode
    want_off = run(parent)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_filter3d(case["filt"])
    want_on = run(ctx)
    assert not torch.equal(want_on[0]["image"], want_off[0]["image"])
    for mode in (0, 1, 2):  # the three Adam-inside forms: -3, nothing touched, the context still serves
        p = {k: v.clone() for k, v in dp.items()}
        opt = opt_mod.AdamOptimizer(p, L, scene_extent=2.5)
        before = {k: v.clone() for k, v in p.items()}
        moments = {k: (opt.exp_avg[k].clone(), opt.exp_avg_sq[k].clone()) for k in opt.names}
        ctx.rasterize_image(p, dc, c, c["bg"], L)
        ctx.backward_render(gi, c["bg"])
        M = ctx._last[1]
        g2 = dict(xyz=torch.empty(M, 3, device="cuda"), precompute_rgb=torch.empty(M, 3, device="cuda")) if mode == 1 else None
        with pytest.raises(lib.GsplatError) as e:
            ctx.backward_gaussians_adam(p, dc, L, opt.fused_state(1, mode=mode), g2)
        assert e.value.code == -3
        torch.cuda.synchronize()
        for k in before:
            assert torch.equal(before[k], p[k]), (mode, k)
        for k, (m, v) in moments.items():
            assert torch.equal(opt.exp_avg[k], m) and torch.equal(opt.exp_avg_sq[k], v), (mode, k)
        assert int(opt.grad_accum_dur.sum()) == 0 and float(opt.uv_grad_accum.abs().sum()) == 0
        same(run(ctx), want_on)
    # a filter of zeros is the mode off, bit for bit; so is None
    ctx.set_filter3d(torch.zeros(N, device="cuda"))
    same(run(ctx), want_off)
    ctx.set_filter3d(None)
    same(run(ctx), want_off)
    p = {k: v.clone() for k, v in dp.items()}
    ctx.rasterize_image(p, dc, c, c["bg"], L)
    ctx.backward_pass_adam(p, dc, gi, c["bg"], L, opt_mod.AdamOptimizer(p, L, scene_extent=2.5).fused_state(1))  # serves again
    with pytest.raises(ValueError):
        ctx.set_filter3d(torch.zeros(N, 2, device="cuda"))
    ctx.set_filter3d(torch.zeros(N - 1, device="cuda"))
    with pytest.raises(ValueError):
        ctx.rasterize_image(dp, dc, c, c["bg"], L)
    ctx.close()
    parent.close()


# ------------------------------------------------------------------------------------------------ 9: the Trainer
def test_trainer_trains_in_the_mode(gpu, scene, monkeypatch, tmp_path):
    from test_absgrad_gpu import _training_setup
    torch, trainer_mod, ops, ds = gpu, pkg("trainer"), pkg("ops"), pkg("dataset")
    init, views, cfg = _training_setup(torch, scene)
    cfg = dict(cfg, filter3d=True, filter3d_interval=10, uv_grad_threshold=1e-6)
    monkeypatch.setenv("GSPLAT_FUSED_ADAM", "1")
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    assert t.fused_adam == 0 and t.filter3d is not None and t.ctx._filter3d is t.filter3d
    first = t.filter3d
    t.train(15, loss_every=1)
    assert t.filter3d is not first, "the filter was not recomputed at iteration 10"
    n0 = t.num_gaussians
    t.adaptive_density_step()
    t.sort_gaussians()
    t.reset_grad_accum()
    assert t.num_gaussians != n0
    assert t.filter3d.shape == (t.num_gaussians,)
    want = ops.compute_filter3d(t.params["xyz"], *ops.camera_arrays([c for c, _ in views]), near=0.2)
    assert torch.equal(t.filter3d, want)
    hist = t.train(15, loss_every=1)  # (the run's whole history)
    assert len(hist) == 30 and t.iter == 30
    losses = [h[1] for h in hist]
    print(f"training with the 3D filter: loss {np.mean(losses[:5]):.4f} -> {np.mean(losses[-5:]):.4f}, "
          f"{n0} -> {t.num_gaussians} gaussians")
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5])
    assert t.ctx._filter3d is t.filter3d and t.ctx._filter3d.numel() == t.num_gaussians
    se, oe = ops.filter3d_apply(t.params["scale"], t.params["opacity"], t.filter3d)
    # exp(scale_eff) >= filter3d row by row; scale_eff = max(scale, log f) + ..., held in float32: logf's and the sum's
    # roundings are 2^-24 relative of values below 16, i.e. at most 2e-6 of exp(.)
    assert bool((torch.exp(se.double()) >= t.filter3d.double()[:, None] * (1 - 4e-6)).all())
    assert bool((se >= t.params["scale"]).all()) and bool((oe <= t.params["opacity"] + 1e-5).all())
    ds.build()
    n, width = t.num_gaussians, 17 + 3 * ((t.l_max + 1) ** 2 - 1)
    for raw, (s_want, o_want) in ((False, (se, oe)), (True, (t.params["scale"], t.params["opacity"]))):
        path = tmp_path / ("raw.ply" if raw else "fused.ply")
        t.save_to_ply(path, raw=raw) if raw else t.save_to_ply(path)
        rows = np.frombuffer(path.read_bytes().split(b"end_header\n", 1)[1], np.float32).reshape(n, width)
        assert np.array_equal(rows[:, -7:-4], _np(s_want)) and np.array_equal(rows[:, -8], _np(o_want)), raw
    # evaluate renders in the mode
    psnr = t.evaluate(views)
    raster = pkg("raster")
    want = {}
    for mode in (True, False):
        ctx = raster.RasterContext(n, t.ctx.max_width, t.ctx.max_height)
        ctx.set_filter3d(t.filter3d if mode else None)
        ctx.set_render_only(True)
        want[mode] = np.mean([ops.compute_psnr(ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)["image"], gt,
                                               int(cam["height"]), int(cam["width"])) for cam, gt in views])
        ctx.close()
    assert psnr == pytest.approx(want[True], rel=1e-12) and psnr != pytest.approx(want[False], rel=1e-6), (psnr, want)


def test_two_rank_training_keeps_the_replicas_identical(gpu, scene):
    from test_absgrad_gpu import _training_setup
    torch, trainer_mod, gdist = gpu, pkg("trainer"), pkg("dist")
    init, views, cfg = _training_setup(torch, scene)
    cfg = dict(cfg, filter3d=True, filter3d_interval=4, antialiased=True)

    def body(comm):
        t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3, comm=comm)
        t.train(6, loss_every=0)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in t.params.items()}
        out["filter3d"] = t.filter3d.cpu().numpy()
        out["uv_grad_accum"] = t.opt.uv_grad_accum.cpu().numpy()
        comm.barrier()
        return out

    r = gdist.ThreadGroup(2).run(body)
    for k in r[0]:
        assert np.array_equal(r[0][k], r[1][k]), k
    assert np.isfinite(r[0]["xyz"]).all() and (r[0]["filter3d"] > 0).all()
    moved = np.abs(r[0]["scale"] - _np(init["scale"])).max()
    assert moved > 0


# ------------------------------------------------------------------------------------------------ 10: what it is for
def test_zoom_in_keeps_every_gaussian_above_the_filter(gpu, scene):
    """The splat_scale = 0.1 scene of README's anti-aliasing bullet, the filter of one camera at 256x144, rendered at four
    times that resolution (same pose, focal x 4), anti-aliased, with and without the mode: with it no gaussian's
    projected minor radius falls below that of an isotropic gaussian of size filter3d at the same place (rendered by the
    same context)."""
    torch, raster, ops = gpu, pkg("raster"), pkg("ops")
    n, w, h = 5000, 256, 144
    params = scene.make_gaussians(n, w, h, 0, splat_scale=0.1)
    cam = scene.make_camera(w, h, 0)
    big = scene.make_camera(4 * w, 4 * h, 0)  # the same field of view at four times the resolution: focal x 4
    assert big["fx"] == pytest.approx(4 * cam["fx"], rel=1e-6)
    dp = raster.device_params(params)
    filt = ops.compute_filter3d(dp["xyz"], *ops.camera_arrays([cam]), near=f3.NEAR)
    c = scene.CONFIG
    ctx = raster.RasterContext(n, 4 * w, 4 * h)
    ctx.set_antialiased(True)
    dc = raster.device_camera(big)
    iso = dict(dp, scale=torch.log(filt)[:, None].expand(n, 3).contiguous())  # isotropic gaussians of size filter3d
    out = {}
    for name, p, mode in (("off", dp, False), ("on", dp, True), ("floor", iso, False)):
        ctx.set_filter3d(filt if mode else None)
        f = ctx.rasterize_image(p, dc, c, 0.0, 0)
        out[name] = (float(f["image"].mean()), f["radius"][:, 1].clone(), f["compact_to_global"].clone())
    for name in ("on", "floor"):
        assert torch.equal(out[name][2], out["off"][2])  # culling follows the positions: the same rows
    # Sigma + f^2 I >= f^2 I, the projection and the radius formula (its clamp and ceilf included) are monotone in the
    # covariance: no minor radius below the floor's
    r_off, r_on, floor = out["off"][1], out["on"][1], out["floor"][1]
    print(f"4x zoom, anti-aliased: mean brightness {out['off'][0]:.4f} without the 3D filter, {out['on'][0]:.4f} with it; "
          f"minor radius below the filter's: {int((r_off < floor).sum())} of {len(floor)} gaussians without, "
          f"{int((r_on < floor).sum())} with; median minor radius {float(r_off.median()):.0f} / {float(r_on.median()):.0f} px")
    assert bool((r_on >= floor).all())
    assert int((r_off < floor).sum()) > len(floor) // 10, "without the mode many gaussians are below the floor"
    ctx.close()

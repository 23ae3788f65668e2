"""GPU tests of absgrad mode (gsplat_context_set_absgrad): the absolute sums of the pixels' shares of grad_uv against the
numpy reference evaluated in float64 on the float32 oracle forward (tests/absgrad_reference.py), the outputs the mode must
not touch, its invariants, long lists, depth mode, the edge populations, the densification statistic of every
per-gaussian entry point, the refusals, and the Trainer / view-sharded step."""
import ctypes

import numpy as np
import pytest

import absgrad_reference
from conftest import assert_grad_close, pkg

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _case(torch, scene, N, W, H, L, view=2):
    raster = pkg("raster")
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, view)
    return raster, params, cam, raster.device_params(params), raster.device_camera(cam)


def _oracle(orc, scene, params, cam, bg, L):
    c = scene.CONFIG
    return orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], bg, L, threads=8)


def _reference(ref, gi, W, H, bg, **kw):
    return absgrad_reference.absgrad_sums(ref, gi, W, H, bg, dtype=np.float64, **kw)


def _norm32(abs_uv):
    """absnorm as the kernels form it: float32 products, sum and square root, each rounded once."""
    u, v = abs_uv[:, 0].astype(np.float32), abs_uv[:, 1].astype(np.float32)
    return np.sqrt(u * u + v * v)


# abs_u >= |grad_u| holds term by term in exact arithmetic; both sides are float32 sums of the same ~1e2..1e3 products
# (6e-8 each, in different orders), so the slack is 1e-5 of the row's absolute sum plus 1e-5 of the mean row.
def _assert_dominates(abs_uv, grad_uv):
    slack = 1e-5 * abs_uv + 1e-5 * abs_uv.mean()
    assert (abs_uv >= np.abs(grad_uv) - slack).all()


PARITY = [("small", None, 0.0), ("small", None, 0.5), ("mid_l0", (3000, 200, 120, 0), 0.5), ("mid_l3", (3000, 200, 120, 3), 0.0)]


@pytest.mark.parametrize("name,shape,bg", PARITY, ids=[f"{p[0]}-bg{p[2]}" for p in PARITY])
def test_absolute_sums_match_the_reference(gpu, scene, orc, name, shape, bg):
    torch = gpu
    N, W, H, L = shape if shape else scene.WORKLOADS[name][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = scene.make_grad_image(W, H)
    ref = _oracle(orc, scene, params, cam, bg, L)
    signed, absolute = _reference(ref, gi, W, H, bg)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_absgrad(True)
    for it in range(2):  # the second forward walks the compacted slots
        fwd = ctx.rasterize_image(dp, dc, c, bg, L)
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=("uv",))
        ctx.backward_pass(dp, dc, torch.as_tensor(gi).cuda(), bg, L, grads)
        got = _np(ctx.absgrad_uv())
        err = np.linalg.norm(got - absolute) / np.linalg.norm(absolute)
        print(f"{name} bg {bg} forward {it}: abs_uv relative L2 {err:.2e}, grad_uv "
              f"{np.linalg.norm(_np(grads['uv']) - signed) / np.linalg.norm(signed):.2e}")
        assert_grad_close(got, absolute, "abs_uv")
        assert_grad_close(_np(grads["uv"]), signed, "grad_uv")
        _assert_dominates(got, _np(grads["uv"]))
        on_list = np.zeros(fwd["num_culled"], bool)
        on_list[_np(fwd["sorted"])] = True
        assert (got[~on_list] == 0).all()
    assert ctx.counters()["compact_walks"] >= 0


def test_mode_leaves_image_and_gradients_alone(gpu, scene):
    torch = gpu
    N, W, H, L = scene.WORKLOADS["small"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    out = {}
    for mode in (False, True):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_absgrad(mode)
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        g = ctx.alloc_gradients(f["num_culled"], L, intermediates=True)
        ctx.backward_pass(dp, dc, gi, c["bg"], L, g)
        torch.cuda.synchronize()
        out[mode] = ({k: f[k].clone() for k in ("image", "T", "n", "sorted", "ranges")}, g)
    for k, v in out[False][0].items():
        assert torch.equal(v, out[True][0][k]), k
    for k, v in out[False][1].items():  # (the compositing backward's float atomics add in launch order: not bitwise)
        assert_grad_close(_np(out[True][1][k]), _np(v), k, rel=1e-5)


def test_invariants_zero_gradient_and_gate(gpu, scene):
    torch = gpu
    N, W, H, L = scene.WORKLOADS["small"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    ctx.set_absgrad(True)
    f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    ctx.backward_render(torch.zeros(H, W, 3, device="cuda"), c["bg"])
    assert bool((ctx.absgrad_uv() == 0).all())
    # saturate every fourth visible gaussian: sigma(20) is 1 in float32 and the gate drops all its sums
    c2g = _np(f["compact_to_global"])
    params["opacity"][c2g[::4]] = 20.0
    dp = raster.device_params(params)
    f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    assert np.array_equal(_np(f["compact_to_global"]), c2g)
    ctx.backward_render(torch.as_tensor(scene.make_grad_image(W, H)).cuda(), c["bg"])
    got = _np(ctx.absgrad_uv())
    assert (got[::4] == 0).all() and (got > 0).any()


def test_long_lists_in_segments(gpu, scene, orc):
    from test_depth_gpu import _long_list_scene, _maps
    torch, raster = gpu, pkg("raster")
    N, W, H, L, params, cam = _long_list_scene(scene)
    c = scene.CONFIG
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    ctx.set_depth(True)
    ctx.set_absgrad(True)
    gi = scene.make_grad_image(W, H)
    gi_d = torch.as_tensor(gi).cuda()
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    ref = _oracle(orc, scene, params, cam, c["bg"], L)
    _, plain = _reference(ref, gi, W, H, c["bg"])
    _, deep = _reference(ref, gi, W, H, c["bg"], grad_depth=gd, grad_alpha=ga, z=np.asarray(ref["xyz_c"])[:, 2])
    for it in range(4):
        ctx.rasterize_image(dp, dc, c, c["bg"], L)
        ctx.backward_render(gi_d, c["bg"])
        assert_grad_close(_np(ctx.absgrad_uv()), plain, f"abs_uv, forward {it}")
        ctx.backward_render(gi_d, c["bg"], grad_depth=gd_d, grad_alpha=ga_d)  # a second backward of the same forward
        assert_grad_close(_np(ctx.absgrad_uv()), deep, f"abs_uv with depth gradients, forward {it}")
    assert ctx.counters()["segmented_backwards"] > 0, ctx.counters()


def test_depth_gradients_enter_the_shares(gpu, scene, orc):
    from test_depth_gpu import _maps
    torch = gpu
    N, W, H, L = 3000, 200, 120, 1
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = scene.make_grad_image(W, H)
    gd, ga, gd_d, ga_d = _maps(torch, W, H)
    ref = _oracle(orc, scene, params, cam, c["bg"], L)
    z = np.asarray(ref["xyz_c"])[:, 2]
    ctx = raster.RasterContext(N, W, H)
    ctx.set_depth(True)
    ctx.set_absgrad(True)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    _, plain = _reference(ref, gi, W, H, c["bg"])
    for which in ("depth", "alpha", "both"):
        GD, GA = (gd if which != "alpha" else None), (ga if which != "depth" else None)
        grads = ctx.alloc_gradients(fwd["num_culled"], L, intermediates=("uv",))
        ctx.backward_pass(dp, dc, torch.as_tensor(gi).cuda(), c["bg"], L, grads,
                          grad_depth=gd_d if GD is not None else None, grad_alpha=ga_d if GA is not None else None)
        signed, absolute = _reference(ref, gi, W, H, c["bg"], grad_depth=GD, grad_alpha=GA, z=z)
        got = _np(ctx.absgrad_uv())
        assert_grad_close(got, absolute, f"abs_uv ({which})")
        assert_grad_close(_np(grads["uv"]), signed, f"grad_uv ({which})")
        assert np.linalg.norm(absolute - plain) > 1e-2 * np.linalg.norm(plain), "the maps' gradients change nothing here"


def test_edge_populations(gpu, scene, orc):
    import edge_scenes as es
    from test_edge_scenes_gpu import _edge_case, _per_population
    torch, raster = gpu, pkg("raster")
    edge = _edge_case(scene, orc, "small")
    C = scene.CONFIG
    N, W, H, L = edge["N"], edge["W"], edge["H"], edge["L"]
    ctx = raster.RasterContext(N, W, H)
    ctx.set_absgrad(True)
    dp, dc = raster.device_params(edge["params"]), raster.device_camera(edge["cam"])
    ctx.rasterize_image(dp, dc, C, C["bg"], L)
    ctx.backward_render(torch.as_tensor(np.ascontiguousarray(edge["gi"])).cuda(), C["bg"])
    _, absolute = _reference(edge["ref"], edge["gi"], W, H, C["bg"])
    _per_population(_np(ctx.absgrad_uv()), absolute, edge["cp"], "abs_uv", size="small")
    assert es.SIZES["small"][0] == N


def test_statistic_of_every_entry_point(gpu, scene):
    """uv_norm / uv_grad_accum == sqrtf(u^2 + v^2) of absgrad_uv(), bit for bit, wherever the library writes it."""
    torch, opt_mod = gpu, pkg("optimizer")
    N, W, H, L = 5000, 256, 144, 3
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L, view=1)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx = raster.RasterContext(N, W, H)
    durs = {}
    for mode in (False, True):
        ctx.set_absgrad(mode)
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        M = fwd["num_culled"]
        c2g = _np(fwd["compact_to_global"])
        rgb, common = torch.zeros(N, 3, device="cuda"), torch.full((N, 12), 7.0, device="cuda")
        uv_norm = torch.full((N,), 7.0, device="cuda")
        ctx.backward_render(gi, c["bg"], rgb, common, uv_norm)
        want = np.zeros(N, np.float32)
        if mode:
            want[c2g] = _norm32(_np(ctx.absgrad_uv()))
            assert (want > 0).any()
            # plain form + pack (hosts that keep the unfused path)
            grads = ctx.backward_gaussians(dp, dc, L, ctx.alloc_gradients(M, L, intermediates=("uv",)))
            packed = raster.pack_absgrad_norm(ctx, N, torch.full((N,), 7.0, device="cuda"))
            assert np.array_equal(_np(packed), want)
            signed = np.zeros(N, np.float32)
            signed[c2g] = _norm32(_np(grads["uv"]))
            assert (want >= signed * (1 - 1e-5)).all() and np.median(want[c2g] / np.maximum(signed[c2g], 1e-30)) > 1.5
            # split form, whole and in three ranges
            ctx.backward_gaussians_split(dp, dc, L, common, uv_norm)
            assert np.array_equal(_np(uv_norm), want)
            uv2 = uv_norm.clone()
            uv2[torch.as_tensor(c2g).cuda().long()] = 7.0
            for lo, hi in ((0, N // 3), (N // 3, 2 * N // 3), (2 * N // 3, N)):
                ctx.backward_gaussians_split(dp, dc, L, common, uv2, lo, hi)
            assert np.array_equal(_np(uv2), want)
        # the three Adam forms (struct modes 0, 1, 2), each on its own copy of the parameters, all on the same rows
        for adam_mode in (0, 1, 2):
            p = {k: v.clone() for k, v in dp.items()}
            opt = opt_mod.AdamOptimizer(p, L, scene_extent=2.5)
            g2 = dict(xyz=torch.empty(M, 3, device="cuda"), precompute_rgb=torch.empty(M, 3, device="cuda")) if adam_mode == 1 else None
            ctx.backward_gaussians_adam(p, dc, L, opt.fused_state(1, mode=adam_mode), g2)
            torch.cuda.synchronize()
            if mode:
                assert np.array_equal(_np(opt.uv_grad_accum), want), adam_mode
                assert np.array_equal(_np(opt.grad_accum_dur), durs[adam_mode]), adam_mode
            else:
                durs[adam_mode] = _np(opt.grad_accum_dur)
                assert durs[adam_mode].sum() == M


def test_refusals_launch_nothing(gpu, scene):
    torch, lib = gpu, pkg("_lib")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    raster, params, cam, dp, dc = _case(torch, scene, N, W, H, L)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx = raster.RasterContext(N, W, H)
    f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    M = f["num_culled"]
    abs_uv, norm = torch.full((M, 2), 7.0, device="cuda"), torch.full((N,), 7.0, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused():
        for call in (lambda: ctx._lib.gsplat_context_absgrad_uv(ctx._h, ctypes.c_void_p(abs_uv.data_ptr()), st),
                     lambda: ctx._lib.gsplat_pack_absgrad_norm(ctx._h, N, ctypes.c_void_p(norm.data_ptr()), st)):
            assert call() == -3  # GSPLAT_ERR_INVALID_ARG
        with pytest.raises(lib.GsplatError):
            ctx.absgrad_uv()
        with pytest.raises(lib.GsplatError):
            raster.pack_absgrad_norm(ctx, N, norm)
        torch.cuda.synchronize()
        assert bool((abs_uv == 7.0).all()) and bool((norm == 7.0).all())

    refused()                      # no backward since the forward
    ctx.backward_render(gi, c["bg"])
    refused()                      # that backward did not run in absgrad mode
    ctx.set_absgrad(True)
    refused()                      # the mode takes effect at the next compositing backward only
    ctx.backward_render(gi, c["bg"])
    assert ctx.absgrad_uv().shape == (M, 2)
    ctx.rasterize_image(dp, dc, c, c["bg"], L)
    refused()                      # the rows' window ends at the next forward
    ro = raster.RasterContext(N, W, H)
    ro.set_render_only(True)
    ro.set_absgrad(True)
    ro.rasterize_image(dp, dc, c, c["bg"], L)
    for call in (lambda: ro._lib.gsplat_context_absgrad_uv(ro._h, ctypes.c_void_p(abs_uv.data_ptr()), st),
                 lambda: ro._lib.gsplat_pack_absgrad_norm(ro._h, N, ctypes.c_void_p(norm.data_ptr()), st)):
        assert call() == -3
    torch.cuda.synchronize()
    assert bool((abs_uv == 7.0).all()) and bool((norm == 7.0).all())
    # lean and depth forwards serve the mode as well
    for setup in ("lean", "depth"):
        cx = raster.RasterContext(N, W, H)
        cx.set_absgrad(True)
        cx.set_lean_forward(True) if setup == "lean" else cx.set_depth(True)
        cx.rasterize_image(dp, dc, c, c["bg"], L)
        cx.backward_render(gi, c["bg"])
        # (two compositing backwards: the rows carry the order of their float atomics)
        assert_grad_close(_np(cx.absgrad_uv()), _np(ctx_abs(ctx, dp, dc, c, L, gi)), setup, rel=1e-5)


def ctx_abs(ctx, dp, dc, c, L, gi):
    ctx.rasterize_image(dp, dc, c, c["bg"], L)
    ctx.backward_render(gi, c["bg"])
    return ctx.absgrad_uv()


def _training_setup(torch, scene, n_views=4):
    raster, ops = pkg("raster"), pkg("ops")
    N, W, H = 3000, 160, 96
    truth = scene.make_gaussians(N, W, H, 0)
    truth["opacity"][:] = np.clip(truth["opacity"], 0.5, 3.0)
    ctx = raster.RasterContext(N, W, H)
    dpt = raster.device_params(truth)
    views = []
    for v in range(n_views):
        cam = raster.device_camera(scene.make_camera(W, H, v))
        views.append((cam, ctx.rasterize_image(dpt, cam, scene.CONFIG, 0.0, 0)["image"].clone()))
    idx = np.random.default_rng(2).choice(N, N // 3, replace=False)
    pts = torch.from_numpy(truth["xyz"][idx].astype(np.float64)).cuda()
    col = torch.from_numpy(np.clip((truth["rgb"][idx] * 0.28209479 + 0.5) * 255, 0, 255).astype(np.uint8)).cuda()
    init = ops.initialize_gaussians(pts, col)
    torch.cuda.synchronize()
    # no density control inside the run: the statistics of all its iterations are there at the end
    cfg = dict(num_iters=36, add_sh_band_interval=12, max_sh_band=2, adaptive_control_start=10 ** 9,
               reset_opacity_start=10 ** 9, uv_grad_threshold=2e-5, max_gaussians=20000, use_background=False)
    return init, views, cfg


def test_trainer_statistic_under_every_fused_adam_mode(gpu, scene, monkeypatch):
    """36 iterations with absgrad=True; every iteration is taken under each GSPLAT_FUSED_ADAM in {0, 1, 2, 3} from the same
    state and must leave identical uv_grad_accum / grad_accum_dur.

    The four paths of an iteration share ONE compositing backward: path 1 runs the whole step, paths 0, 2 and 3 are taken
    from the restored state with the forward and the compositing backward replaced by what path 1 left in the context
    (the rows are valid until the next forward).  Four trainings run apart cannot be compared bit for bit, with or without
    the mode: the compositing backward adds a gaussian's tiles into its row with float atomics, in arrival order, so two
    runs of the SAME path already differ (printed below; measured 1e-5 relative after 36 iterations)."""
    torch, trainer_mod, ops = gpu, pkg("trainer"), pkg("ops")
    init, views, cfg = _training_setup(torch, scene)
    monkeypatch.setenv("GSPLAT_FUSED_ADAM", "1")
    runs = {}
    for absgrad in (True, False):  # two plain trainings: the mode against |grad_uv|, and (below) run against run
        t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, absgrad=absgrad), scene_extent=5.0, seed=3)
        t.train(36, loss_every=0)
        runs[(absgrad, 1)] = t
    acc = {k: t.opt.uv_grad_accum for k, t in runs.items()}

    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, absgrad=True, add_sh_band_interval=10 ** 9),
                            scene_extent=5.0, seed=3)
    t.add_sh_band()  # SH degree 1: the colour kernels of paths 2 and 3 have rows to read
    ctx = t.ctx

    def snap():
        o = t.opt
        return ({k: v.clone() for k, v in t.params.items()}, {g: o.exp_avg[g].clone() for g in o.names},
                {g: o.exp_avg_sq[g].clone() for g in o.names}, o.uv_grad_accum.clone(), o.grad_accum_dur.clone(), t.iter)

    def restore(s):
        o = t.opt
        for k, v in s[0].items():
            t.params[k].copy_(v)
        for g in o.names:
            o.exp_avg[g].copy_(s[1][g])
            o.exp_avg_sq[g].copy_(s[2][g])
        o.uv_grad_accum.copy_(s[3])
        o.grad_accum_dur.copy_(s[4])
        t.iter = s[5]

    real_fwd = ctx.rasterize_image
    for it in range(36):
        cam, gt = views[t.draw_views()[0]]
        before, kept = snap(), {}

        def recording_forward(*a, **k):
            kept["fwd"] = real_fwd(*a, **k)
            return kept["fwd"]

        t.fused_adam = 1
        ctx.rasterize_image = recording_forward
        t.train_step(cam, gt, want_loss=False)
        after = snap()
        assert int(after[4].sum()) > int(before[4].sum())
        ctx.rasterize_image = lambda *a, **k: kept["fwd"]
        ctx.backward_render = lambda *a, **k: None
        ctx.backward_pass = lambda p, cm, gi, bg, L, grads: ctx.backward_gaussians(p, cm, L, grads)
        for fused in (0, 2, 3):
            restore(before)
            t.fused_adam = fused
            t.train_step(cam, gt, want_loss=False)
            torch.cuda.synchronize()
            assert torch.equal(t.opt.uv_grad_accum, after[3]), f"iteration {it}, GSPLAT_FUSED_ADAM={fused}"
            assert torch.equal(t.opt.grad_accum_dur, after[4]), f"iteration {it}, GSPLAT_FUSED_ADAM={fused}"
        del ctx.rasterize_image, ctx.backward_render, ctx.backward_pass
        restore(after)
    assert float(t.opt.uv_grad_accum.sum()) > 0
    again = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, absgrad=True), scene_extent=5.0, seed=3)
    again.train(36, loss_every=0)
    d = (again.opt.uv_grad_accum - acc[(True, 1)]).abs().max() / acc[(True, 1)].abs().max()
    print(f"two trainings run apart, same path: uv_grad_accum differs by {float(d):.1e} of its largest entry")
    on = runs[(True, 1)]
    ratio = float((acc[(True, 1)].sum() / acc[(False, 1)].sum()).item())
    print(f"generated scene, 36 iterations: sum absnorm / sum |grad_uv| = {ratio:.2f}")
    assert ratio > 1.0
    # the same state and threshold, the two statistics of ONE backward of the trained state: the mode's masks are supersets
    raster, c = pkg("raster"), on.cfg
    cam, gt = views[0]
    H, W = int(cam["height"]), int(cam["width"])
    p = dict(on.params)
    fwd = on.ctx.rasterize_image(p, cam, c, 0.0, on.l_max)
    gi = torch.empty(H, W, 3, device="cuda")
    ops.fused_loss(fwd["image"], gt, H, W, float(c["ssim_frac"]), gi, blocking=False)
    grads = on.ctx.alloc_gradients(fwd["num_culled"], on.l_max, intermediates=("uv",))
    on.ctx.backward_pass(p, cam, gi, 0.0, on.l_max, grads)
    n = on.num_gaussians
    stat_on = raster.pack_absgrad_norm(on.ctx, n, torch.empty(n, device="cuda"))
    stat_off = raster.pack_uv_grad_norm(on.ctx, grads, n, torch.empty(n, device="cuda"))
    dur = (stat_on > 0).to(torch.int32)
    step_ratio = float((stat_on.sum() / stat_off.sum()).item())
    print(f"trained state, one view: sum absnorm / sum |grad_uv| = {step_ratio:.2f}")
    thr = float(torch.quantile(stat_off[stat_off > 0], 0.9).item())  # a threshold the signed statistic passes for a tenth
    masks = {}
    for name, a in (("on", stat_on), ("off", stat_off)):
        masks[name] = ops.density_masks(on.params["opacity"], on.params["scale"], a, dur,
                                        trainer_mod._logit(float(c["delete_opacity_threshold"])), on.scene_extent * 0.1,
                                        thr, on.scene_extent * 0.01)
    for k, what in ((1, "clone"), (2, "split")):
        m_on, m_off = masks["on"][k].bool(), masks["off"][k].bool()
        assert bool((m_on | ~m_off).all()), what
    assert int(masks["on"][1].sum() + masks["on"][2].sum()) > int(masks["off"][1].sum() + masks["off"][2].sum())


def test_sharded_step_sums_absnorm_over_ranks(gpu, scene):
    torch, raster, gdist = gpu, pkg("raster"), pkg("dist")
    N, W, H, L = 3000, 160, 96, 1
    params = scene.make_gaussians(N, W, H, L)
    c = scene.CONFIG
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    cams = [raster.device_camera(scene.make_camera(W, H, v)) for v in range(2)]
    base = raster.device_params(params)
    singles = []
    for cam in cams:  # each view on its own: absnorm in global order
        ctx = raster.RasterContext(N, W, H)
        ctx.set_absgrad(True)
        ctx.rasterize_image(base, cam, c, c["bg"], L)
        ctx.backward_render(gi, c["bg"])
        singles.append(raster.pack_absgrad_norm(ctx, N, torch.empty(N, device="cuda")).clone())

    def body(comm):
        dp = {k: v.clone() for k, v in base.items()}
        out = {}
        for exchange in ("split", "full"):
            step = gdist.ViewShardedStep(dp, L, W, H, c, c["bg"], exchange=exchange, with_uv_norm=True, comm=comm, absgrad=True)
            step.step(cams[comm.rank], grad_image=gi)
            torch.cuda.synchronize()
            out[exchange] = step.uv_norm_sum.cpu().numpy().copy()
            comm.barrier()
        return out

    r = gdist.ThreadGroup(2).run(body)
    want = _np(singles[0] + singles[1])
    for exchange in ("split", "full"):
        for rank in range(2):
            # (each rank's own compositing backward: the rows carry the float atomics' order, so not bitwise)
            assert_grad_close(r[rank][exchange], want, f"{exchange} rank {rank}", rel=1e-5)
        assert np.array_equal(r[0][exchange], r[1][exchange]), exchange

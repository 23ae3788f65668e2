"""The Trainer's depth regularisers (config keys distortion, depth_prior) on the generated 3000-gaussian, 160x96 scene of
tests/test_absgrad_gpu.py: one train_step against the same step composed by hand, the depth prior's third view element,
the keys off, and the distortion of the trained state with and without the key."""
import numpy as np
import pytest

from conftest import assert_grad_close, pkg
from test_absgrad_gpu import _training_setup

pytestmark = pytest.mark.gpu

ITERS = 36  # the iteration count of that scene's training test (test_trainer_statistic_under_every_fused_adam_mode)


def _np(t):
    return t.detach().cpu().numpy()


def _clone(init):
    return {k: v.clone() for k, v in init.items()}


def test_one_step_is_the_hand_composed_step(gpu, scene, monkeypatch):
    torch, trainer_mod, ops, opt_mod = gpu, pkg("trainer"), pkg("ops"), pkg("optimizer")
    monkeypatch.setenv("GSPLAT_FUSED_ADAM", "0")
    init, views, cfg = _training_setup(torch, scene)
    cfg = dict(cfg, distortion=True, distortion_start=0)
    t = trainer_mod.Trainer(_clone(init), views, cfg, scene_extent=5.0, seed=3)
    assert t.fused_adam == 0 and t.ctx._depth and t.ctx._depth_moment and t.ctx._depth_inverse
    cam, gt = views[0]
    H, W = int(cam["height"]), int(cam["width"])
    # by hand, on a context and an optimizer of its own
    c = t.cfg
    p = {k: v.clone() for k, v in t.params.items()}
    l_max = t.l_max
    po = dict(p)
    if l_max == 0:
        po.pop("sh")
    opt = opt_mod.AdamOptimizer(po, l_max, lr_config=c, scene_extent=5.0)
    ctx = pkg("raster").RasterContext(t.num_gaussians, W, H)
    ctx.set_lean_forward(True)
    ctx.set_depth(True, inverse=True, moment=True)
    bg = 0.0  # use_background=False
    fwd = ctx.rasterize_image(p, cam, c, bg, l_max)
    gi = torch.empty(H, W, 3, device="cuda")
    ops.fused_loss(fwd["image"], gt, H, W, float(c["ssim_frac"]), gi, blocking=False)
    maps = [torch.empty(H, W, device="cuda") for _ in range(3)]
    ops.distortion_loss(fwd, float(c["distortion_weight"]), *maps)
    grads = ctx.alloc_gradients(fwd["num_culled"], l_max, intermediates=("uv",), factored_sh=True)
    ctx.backward_pass(p, cam, gi, bg, l_max, grads, grad_alpha=maps[0], grad_depth=maps[1], grad_depth2=maps[2])
    opt.step(0, fwd, grads, campos=cam["campos"])
    # ... and the Trainer's
    t.train_step(cam, gt, want_loss=False)
    torch.cuda.synchronize()
    assert t.last_regularisers == {"distortion": float(c["distortion_weight"])}
    assert float(maps[2].abs().sum()) > 0
    for k in t.opt.names:  # (float atomics add in arrival order: not bitwise)
        assert_grad_close(_np(t.params[k]), _np(p[k]), k, rel=1e-5)
        assert_grad_close(_np(t.opt.exp_avg[k]), _np(opt.exp_avg[k]), "exp_avg " + k, rel=1e-5)
        assert_grad_close(_np(t.opt.exp_avg_sq[k]), _np(opt.exp_avg_sq[k]), "exp_avg_sq " + k, rel=1e-5)
    # the step is not the plain one
    plain = trainer_mod.Trainer(_clone(init), views, dict(cfg, distortion=False), scene_extent=5.0, seed=3)
    plain.train_step(cam, gt, want_loss=False)
    torch.cuda.synchronize()
    assert not torch.allclose(plain.opt.exp_avg["xyz"], t.opt.exp_avg["xyz"], rtol=1e-3, atol=0)


def test_depth_prior_takes_the_third_view_element(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    cfg = dict(cfg, depth_prior=True)
    probe = trainer_mod.Trainer(_clone(init), views, cfg, scene_extent=5.0, seed=3)
    assert probe.ctx._depth and probe.ctx._depth_inverse and not probe.ctx._depth_moment
    cam, gt = views[0]
    own = probe.ctx.rasterize_image(dict(probe.params), cam, probe.cfg, 0.0, probe.l_max)
    assert "depth2" not in own
    own_depth = own["depth"].clone()
    assert float(own_depth.max()) > 0
    H, W = own_depth.shape
    # the target equal to the render's own inverse depth: the term's gradient map is zero
    probe.train_step(cam, gt, want_loss=False, depth_target=own_depth)
    torch.cuda.synchronize()
    assert probe.last_regularisers == {"depth_prior": probe.depth_prior_weight(0)}
    assert bool((probe._depth_maps[(H, W)][1] == 0).all())
    # a target that is off: a gradient where there is data, none in the holes; a view without one skips the term
    target = own_depth * 1.5
    target[: H // 2] = 0.0
    t = trainer_mod.Trainer(_clone(init), [(cam, gt, target), views[1]], cfg, scene_extent=5.0, seed=3)
    before = t.params["xyz"].clone()
    t.train(2, loss_every=0)  # iteration 0: view 0 (with the target), iteration 1: view 1 (without)
    torch.cuda.synchronize()
    g = t._depth_maps[(H, W)][1]
    assert bool((g[: H // 2] == 0).all()) and float(g[H // 2:].abs().sum()) > 0
    assert t.last_regularisers == {}
    assert not torch.equal(before, t.params["xyz"])
    w0, w1 = float(t.cfg["depth_prior_weight_init"]), float(t.cfg["depth_prior_weight_final"])
    assert t.depth_prior_weight(0) == w0 and abs(t.depth_prior_weight(t.cfg["num_iters"]) - w1) < 1e-12
    assert t.evaluate() > 0  # (three-element views are views everywhere)


def test_keys_off_and_combinations(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    t = trainer_mod.Trainer(_clone(init), views, cfg, scene_extent=5.0, seed=3)
    assert t.ctx._depth is False
    seen = {}
    real = t.ctx.rasterize_image

    def recording(*a, **k):
        seen["fwd"] = real(*a, **k)
        return seen["fwd"]

    t.ctx.rasterize_image = recording
    t.train_step(*views[0], want_loss=False)
    assert "depth" not in seen["fwd"] and "depth2" not in seen["fwd"]
    assert t._depth_maps == {} and t.last_regularisers == {}
    with pytest.raises(ValueError):
        trainer_mod.Trainer(_clone(init), views, dict(cfg, distortion=True, absgrad=True), scene_extent=5.0, seed=3)

    class TwoRanks:
        world, rank = 2, 0

    for key in ("distortion", "depth_prior"):
        with pytest.raises(ValueError):
            trainer_mod.Trainer(_clone(init), views, dict(cfg, **{key: True}), scene_extent=5.0, seed=3, comm=TwoRanks())
    # before distortion_start the step carries no term
    late = trainer_mod.Trainer(_clone(init), views, dict(cfg, distortion=True, distortion_start=5), scene_extent=5.0, seed=3)
    late.train_step(*views[0], want_loss=False)
    assert late.last_regularisers == {} and late._depth_maps == {}


def _mean_distortion(t, views):
    """mean over the views and pixels of A Q - D^2 (s = 1/z), in double from the maps of a (1,1) forward."""
    raster = pkg("raster")
    cam0 = views[0][0]
    ctx = raster.RasterContext(t.num_gaussians, int(cam0["width"]), int(cam0["height"]))
    ctx.set_render_only(True)
    ctx.set_depth(True, inverse=True, moment=True)
    total = 0.0
    for cam, _ in views:
        f = ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)
        A, D, Q = (1.0 - f["T"].double()), f["depth"].double(), f["depth2"].double()
        total += float((A * Q - D * D).mean())
    return total / len(views)


def test_distortion_goes_down(gpu, scene):
    """The same seed with and without the key, at the recorded default weight (README, "Depth regularisers"): the mean
    distortion over the training views after the scene's 36 iterations is strictly lower with it."""
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    out = {}
    for on in (False, True):
        t = trainer_mod.Trainer(_clone(init), views, dict(cfg, distortion=on, distortion_start=0), scene_extent=5.0, seed=3)
        assert t.cfg["distortion_weight"] == trainer_mod.DISTORTION_WEIGHT
        t.train(ITERS, loss_every=0)
        out[on] = (_mean_distortion(t, views), t.evaluate())
    print(f"mean A Q - D^2 after {ITERS} iterations: {out[False][0]:.6e} without, {out[True][0]:.6e} with the key; "
          f"PSNR {out[False][1]:.2f} / {out[True][1]:.2f}")
    assert out[True][0] < out[False][0]

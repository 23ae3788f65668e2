"""The Trainer's normal terms (config keys normal_prior, normal_smooth) on the generated 3000-gaussian, 160x96 scene of
tests/test_absgrad_gpu.py: the keys off, each key against the run without it from the same seed, all four depth terms in
one step against the separate terms' maps, the refusal on more than one rank, and render_normals."""
import math

import numpy as np
import pytest

from conftest import assert_grad_close, pkg
from test_absgrad_gpu import _training_setup

pytestmark = pytest.mark.gpu

ITERS = 36  # the iteration count of that scene's training test


def _np(t):
    return t.detach().cpu().numpy()


def _clone(init):
    return {k: v.clone() for k, v in init.items()}


class _Recorder:
    """The loaded library with every entry point that is fetched from it written down, in order."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._real, name)


def _rotation(degrees):
    """A fixed rotation about the axis (1, 2, 0) / sqrt 5."""
    a = math.radians(degrees)
    k = np.array([1.0, 2.0, 0.0]) / math.sqrt(5.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def _mean_smoothness(t, views):
    """Mean over the views of the smoothness loss at weight 1 of the trained state's normal map (edge-aware on the view's
    ground truth, config key normal_edge_scale)."""
    ops = pkg("ops")
    return sum(ops.normal_smoothness_loss(t.render_normals(v[0]), v[1], 1.0, None, edge_scale=float(t.cfg["normal_edge_scale"]),
                                          blocking=True) for v in views) / len(views)


def _mean_prior(t, views):
    ops = pkg("ops")
    return sum(ops.normal_prior_loss(t.render_normals(v[0]), v[3], 1.0, None, blocking=True) for v in views) / len(views)


@pytest.fixture(scope="module")
def setup(gpu, scene):
    """The scene, the run that was never given the keys, and every view's prior: the initial state's normal map turned by
    10 degrees."""
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    R = torch.as_tensor(_rotation(10.0).astype(np.float32)).cuda()
    first = trainer_mod.Trainer(_clone(init), views, cfg, scene_extent=5.0, seed=3)
    prior_views = []
    for cam, gt in views:
        n = first.render_normals(cam)
        assert tuple(n.shape) == (int(cam["height"]), int(cam["width"]), 3)
        prior_views.append((cam, gt, None, (n @ R.T).contiguous()))
    plain = trainer_mod.Trainer(_clone(init), views, cfg, scene_extent=5.0, seed=3)
    plain.train(ITERS, loss_every=0)
    torch.cuda.synchronize()
    return dict(init=init, views=views, cfg=cfg, prior_views=prior_views, plain=plain)


def test_keys_off_is_the_run_without_them(gpu, setup, monkeypatch):
    """Given as False the keys change nothing: over 36 iterations the same entry points in the same order as a Trainer
    that never heard of them, none of them a normal or depth-mode one, nothing allocated, the first iteration's image and
    transmittance bit for bit, and the first step's parameters and moments as close as one step has them.

    Bit for bit the parameters cannot be asked for: the compositing backward adds a gaussian's tiles into its row with
    float atomics, in arrival order, so two runs of the SAME Trainer already differ
    (tests/test_absgrad_gpu.py::test_trainer_statistic_under_every_fused_adam_mode), and Adam's normalised step carries a
    difference in a small gradient's last bits into the parameter.  One step is held to what
    tests/test_trainer_distortion_gpu.py holds a step and its hand-composed twin to for the same reason (assert_grad_close
    at 1e-5).  After 36 iterations the distance is printed, not asserted: measured between this run and a never-given
    one, and between two never-given ones, xyz 4.27e-6 and 4.27e-6 (norm 2.6e2), scale 2.34e-4 and 2.36e-4 (norm 42),
    opacity 1.99e-4 and 2.01e-4 (norm 50) in one process, xyz 4.1e-6 and 1.2e-6, scale 2.3e-4 and 4.0e-5 in another:
    the same kind of number, and no bound to take from either."""
    torch, trainer_mod, lib_mod = gpu, pkg("trainer"), pkg("_lib")
    real = lib_mod.load()
    off = dict(normal_prior=False, normal_smooth=False)
    out = []
    for cfg in (setup["cfg"], dict(setup["cfg"], **off)):
        rec = _Recorder(real)
        monkeypatch.setattr(lib_mod, "_lib", rec)
        t = trainer_mod.Trainer(_clone(setup["init"]), setup["prior_views"], cfg, scene_extent=5.0, seed=3)
        first, forward = [], t.ctx.rasterize_image

        def recording(*a, _first=first, _forward=forward, **k):
            fwd = _forward(*a, **k)
            if not _first:
                _first.append((fwd["image"].clone(), fwd["T"].clone()))
            return fwd

        t.ctx.rasterize_image = recording
        t.train(1, loss_every=0)
        step1 = {}
        for k in t.opt.names:
            step1[k], step1["exp_avg " + k] = _np(t.params[k]), _np(t.opt.exp_avg[k])
            step1["exp_avg_sq " + k] = _np(t.opt.exp_avg_sq[k])
        t.train(ITERS - 1, loss_every=0)
        torch.cuda.synchronize()
        monkeypatch.setattr(lib_mod, "_lib", real)
        assert t.ctx._depth is False and t._normal_maps == {} and t._depth_maps == {} and t.last_regularisers == {}
        out.append((t, rec.calls, first[0], step1))
    (a, calls_a, first_a, step_a), (b, calls_b, first_b, step_b) = out
    assert calls_a == calls_b and len(calls_a) > 3 * ITERS
    assert not [c for c in calls_a if "normal" in c or "set_depth" in c or c.endswith("_depth") or c.endswith("_depth2")]
    assert a.cfg == b.cfg
    assert torch.equal(first_a[0], first_b[0]) and torch.equal(first_a[1], first_b[1])
    for what in step_a:
        assert_grad_close(step_b[what], step_a[what], what + " after one step", rel=1e-5)
    plain = setup["plain"]  # a second run that was never given the keys
    dist = lambda x, y: float((x.double() - y.double()).norm())
    for k in a.opt.names:
        print(f"{k} after {ITERS} iterations: |off - never| = {dist(a.params[k], b.params[k]):.3e}, |never - never| = "
              f"{dist(a.params[k], plain.params[k]):.3e}, |value| = {float(a.params[k].double().norm()):.3e}")


def test_smoothness_goes_down(gpu, setup):
    """The same seed with and without normal_smooth, at its default weight from iteration 0: the mean smoothness loss over
    the training views after the scene's 36 iterations is strictly lower with it."""
    torch, trainer_mod = gpu, pkg("trainer")
    views, plain = setup["views"], setup["plain"]
    t = trainer_mod.Trainer(_clone(setup["init"]), views, dict(setup["cfg"], normal_smooth=True, normal_start=0),
                            scene_extent=5.0, seed=3)
    assert t.cfg["normal_smooth_weight"] == trainer_mod.NORMAL_SMOOTH_WEIGHT and t.cfg["normal_edge_scale"] == 1.0
    assert t.ctx._depth and t.ctx._depth_inverse and not t.ctx._depth_moment
    t.train(ITERS, loss_every=0)
    assert t.last_regularisers == {"normal_smooth": trainer_mod.NORMAL_SMOOTH_WEIGHT}
    without, with_ = _mean_smoothness(plain, views), _mean_smoothness(t, views)
    print(f"mean smoothness loss after {ITERS} iterations: {without:.6e} without, {with_:.6e} with the key; "
          f"PSNR {plain.evaluate():.2f} / {t.evaluate():.2f}")
    assert without > 0 and with_ < without


def test_prior_loss_goes_down(gpu, setup):
    """normal_prior with every view's prior (the fourth view element): the mean prior loss over the training views is
    lower than after the run without the key; a view without a prior skips the term."""
    torch, trainer_mod = gpu, pkg("trainer")
    pv, plain = setup["prior_views"], setup["plain"]
    assert all(float(v[3].abs().sum()) > 0 for v in pv)
    t = trainer_mod.Trainer(_clone(setup["init"]), pv, dict(setup["cfg"], normal_prior=True, normal_start=0),
                            scene_extent=5.0, seed=3)
    assert t.cfg["normal_prior_weight"] == trainer_mod.NORMAL_PRIOR_WEIGHT
    t.train(ITERS, loss_every=0)
    assert t.last_regularisers == {"normal_prior": trainer_mod.NORMAL_PRIOR_WEIGHT}
    without, with_ = _mean_prior(plain, pv), _mean_prior(t, pv)
    print(f"mean normal-prior loss after {ITERS} iterations: {without:.6e} without, {with_:.6e} with the key; "
          f"PSNR {plain.evaluate():.2f} / {t.evaluate():.2f}")
    assert without > 0 and with_ < without
    # a view without the fourth element: no term, no launch; before normal_start: neither
    t.train_step(*setup["views"][0], want_loss=False)
    assert t.last_regularisers == {}
    late = trainer_mod.Trainer(_clone(setup["init"]), pv, dict(setup["cfg"], normal_prior=True, normal_smooth=True, normal_start=5),
                               scene_extent=5.0, seed=3)
    late.train_step(pv[0][0], pv[0][1], want_loss=False, normal_target=pv[0][3])
    assert late.last_regularisers == {} and late._normal_maps == {} and late._depth_maps == {}


def test_four_terms_add_up(gpu, setup, monkeypatch):
    """distortion, depth_prior, normal_prior and normal_smooth in one step: the maps the backward was given are the
    separate terms' maps added in float, in the order the step evaluates them."""
    torch, trainer_mod, ops = gpu, pkg("trainer"), pkg("ops")
    monkeypatch.setenv("GSPLAT_FUSED_ADAM", "0")
    cam, gt, _, n_prior = setup["prior_views"][0]
    cfg = dict(setup["cfg"], distortion=True, distortion_start=0, depth_prior=True, normal_prior=True, normal_smooth=True,
               normal_start=0)
    t = trainer_mod.Trainer(_clone(setup["init"]), setup["views"], cfg, scene_extent=5.0, seed=3)
    assert t.ctx._depth and t.ctx._depth_moment and t.ctx._depth_inverse
    seen = {}
    real = t.ctx.rasterize_image

    def recording(*a, **k):
        seen["fwd"] = real(*a, **k)
        return seen["fwd"]

    t.ctx.rasterize_image = recording
    H, W = int(cam["height"]), int(cam["width"])
    probe = t.ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)
    d_target = (probe["depth"] * 1.5).contiguous()
    d_target[: H // 2] = 0.0
    t.train_step(cam, gt, want_loss=False, depth_target=d_target, normal_target=n_prior)
    torch.cuda.synchronize()
    c = t.cfg
    assert t.last_regularisers == {"distortion": float(c["distortion_weight"]), "depth_prior": t.depth_prior_weight(0),
                                   "normal_prior": float(c["normal_prior_weight"]), "normal_smooth": float(c["normal_smooth_weight"])}
    assert list(t.last_regularisers) == ["distortion", "depth_prior", "normal_prior", "normal_smooth"]
    g_alpha, g_depth, g_depth2 = t._depth_maps[(H, W)]
    fwd = seen["fwd"]  # the step's forward: its maps stay until the next one
    z = lambda: torch.empty(H, W, device="cuda")
    dist = [z(), z(), z()]
    ops.distortion_loss(fwd, float(c["distortion_weight"]), *dist)
    prior = z()
    ops.depth_prior_loss(fwd["depth"], d_target, t.depth_prior_weight(0), prior)
    normal = ops.depth_to_normal(fwd, cam, True, alpha_min=float(c["normal_alpha_min"]))
    g_n, g_s = torch.empty(H, W, 3, device="cuda"), torch.empty(H, W, 3, device="cuda")
    ops.normal_prior_loss(normal, n_prior, float(c["normal_prior_weight"]), g_n)
    ops.normal_smoothness_loss(normal, gt, float(c["normal_smooth_weight"]), g_s, edge_scale=float(c["normal_edge_scale"]))
    assert torch.equal(t._normal_maps[(H, W)][0], normal) and torch.equal(t._normal_maps[(H, W)][1], g_n + g_s)
    nd, na = z(), z()
    ops.depth_to_normal_backward(fwd, cam, True, g_n + g_s, nd, na, alpha_min=float(c["normal_alpha_min"]))
    assert float(nd.abs().sum()) > 0 and float(na.abs().sum()) > 0
    assert torch.equal(g_depth, (dist[1] + prior) + nd)
    assert torch.equal(g_alpha, dist[0] + na)
    assert torch.equal(g_depth2, dist[2])
    # the depth prior alone before the normals: the opacity map's gradient is the normal term's own
    t2 = trainer_mod.Trainer(_clone(setup["init"]), setup["views"], dict(cfg, distortion=False), scene_extent=5.0, seed=3)
    t2.train_step(cam, gt, want_loss=False, depth_target=d_target, normal_target=n_prior)
    torch.cuda.synchronize()
    assert torch.equal(t2._depth_maps[(H, W)][0], na) and torch.equal(t2._depth_maps[(H, W)][1], prior + nd)
    # the normals alone: overwritten, not added to
    t3 = trainer_mod.Trainer(_clone(setup["init"]), setup["views"], dict(cfg, distortion=False, depth_prior=False),
                             scene_extent=5.0, seed=3)
    for m in (t3._depth_maps.setdefault((H, W), tuple(torch.full((H, W), float("nan"), device="cuda") for _ in range(3)))):
        assert bool(m.isnan().all())
    t3.train_step(cam, gt, want_loss=False, normal_target=n_prior)
    torch.cuda.synchronize()
    assert torch.equal(t3._depth_maps[(H, W)][0], na) and torch.equal(t3._depth_maps[(H, W)][1], nd)


def test_keys_are_refused_on_more_than_one_rank(gpu, setup):
    trainer_mod = pkg("trainer")

    class TwoRanks:
        world, rank = 2, 0

    for key in ("normal_prior", "normal_smooth"):
        with pytest.raises(ValueError):
            trainer_mod.Trainer(_clone(setup["init"]), setup["views"], dict(setup["cfg"], **{key: True}), scene_extent=5.0,
                                seed=3, comm=TwoRanks())


def test_render_normals(gpu, setup):
    torch = gpu
    plain = setup["plain"]
    cam = setup["views"][1][0]
    n = plain.render_normals(cam)
    assert plain.ctx._depth is False  # (depth mode was on for that forward only)
    assert tuple(n.shape) == (int(cam["height"]), int(cam["width"]), 3) and n.dtype == torch.float32
    has = (n != 0).any(-1)
    length = n.double().norm(dim=-1)
    print(f"render_normals: {int(has.sum())} of {has.numel()} pixels have a normal")
    assert int(has.sum()) > has.numel() // 10 and not bool(has.all())
    assert bool(((length[has] - 1.0).abs() <= 1e-6).all()) and bool((length[~has] == 0).all())
    assert float(n[has][:, 2].mean()) < 0  # facing the camera
    assert torch.equal(plain.render_normals(cam), n)
    # the training path is as it was: the next step of a run without depth terms renders no depth
    assert plain.evaluate() > 0

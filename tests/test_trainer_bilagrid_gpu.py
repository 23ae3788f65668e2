"""The Trainer's per-view bilateral grids (config key bilagrid) on the generated 1000-gaussian, 160x96, four-view scene of
tests/test_absgrad_gpu.py (3000 truth gaussians, a third of them as the initial points).

One step against its pieces: the forward, the slice, the fused loss, the slice's backward and the TV loss carry the same
bits in every run, so the dL/d image the backward is handed is compared bit for bit with the hand-composed one, and the
view's grid and its two moments are held to the single-step Adam tolerance of tests/test_optimizer_gpu.py against the Adam
reference on the hand-composed gradient."""
import numpy as np
import pytest

import feature_loss_reference as flr
from conftest import pkg
from test_absgrad_gpu import _training_setup

pytestmark = pytest.mark.gpu

ITERS = 120
GAINS = ((0.7, 1.0, 1.3), (1.3, 0.7, 1.0), (1.0, 1.3, 0.7), (1.3, 1.0, 0.7))  # per view and channel


def _np(t):
    return t.detach().cpu().numpy()


def _clone(init):
    return {k: v.clone() for k, v in init.items()}


@pytest.fixture(scope="module")
def setup(gpu, scene):
    return _training_setup(gpu, scene)  # built once: (init, views, cfg)


def _trainer(setup, views=None, **keys):
    init, plain, cfg = setup
    return pkg("trainer").Trainer(_clone(init), plain if views is None else views, dict(cfg, **keys), scene_extent=5.0, seed=3)


def _record_backward(monkeypatch, raster, seen):
    """Keep a copy of the dL/d image every backward of a RasterContext is handed."""
    for name in ("backward_pass", "backward_pass_adam"):
        real = getattr(raster.RasterContext, name)

        def keeping(self, p, cam, grad_image, *rest, _real=real, **kw):
            seen.append(grad_image.clone())
            return _real(self, p, cam, grad_image, *rest, **kw)

        monkeypatch.setattr(raster.RasterContext, name, keeping)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 4)], ids=lambda v: "x".join(map(str, v)))
def test_one_step_is_what_its_pieces_say(gpu, scene, setup, monkeypatch, shape):
    torch, ops, raster, opt_mod = gpu, pkg("ops"), pkg("raster"), pkg("optimizer")
    init, views, cfg = setup
    N = init["xyz"].shape[0]
    view, tv_weight, lr, steps_before = 2, 3.0, 0.004, 5
    t = _trainer(setup, bilagrid=True, bilagrid_shape=shape, bilagrid_tv_weight=tv_weight, bilagrid_lr=lr)
    Wg, Hg, L = shape
    assert tuple(t.bilagrids.shape) == (4, 12, L, Hg, Wg)
    assert _np(t.bilagrids).tobytes() == _np(ops.identity_bilagrid(Wg, Hg, L, views=4)).tobytes()
    # a state a run reaches: grids off the identity, moments and a step count of the view's own
    rng = np.random.default_rng(11)
    noise = lambda scale: torch.from_numpy((scale * rng.standard_normal(tuple(t.bilagrids.shape))).astype(np.float32)).cuda()
    t.bilagrids += noise(0.05)
    m, sq, counts, _ = t._bilagrid_state
    m.copy_(noise(1e-4))
    sq.copy_(noise(1e-4) ** 2)
    counts[view] = steps_before
    grid0, m0, sq0 = t.bilagrids.clone(), m.clone(), sq.clone()
    cam, gt = views[view]
    H, W = int(cam["height"]), int(cam["width"])
    # the pieces, on a context of their own, from the initial state
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image({k: v.clone() for k, v in t.params.items()}, cam, t.cfg, 0.0, t.l_max)
    corrected = ops.bilagrid_slice(grid0[view], fwd["image"])
    grad_corrected, grad_render = torch.empty(H, W, 3, device="cuda"), torch.empty(H, W, 3, device="cuda")
    loss = ops.fused_loss(corrected, gt, H, W, float(t.cfg["ssim_frac"]), grad_corrected, blocking=True)
    grad_grid = torch.empty_like(grid0[view])
    ops.bilagrid_slice_backward(grid0[view], fwd["image"], grad_corrected, grad_render, grad_grid)
    ops.bilagrid_tv_loss(grid0[view], tv_weight, grad_grid, accumulate=True)
    torch.cuda.synchronize()
    b1c, b2c = opt_mod.AdamOptimizer.bias_corrections(steps_before)
    want = flr.adam_step(_np(grid0[view]), _np(grad_grid), _np(m0[view]), _np(sq0[view]), lr, opt_mod.B1, opt_mod.B2,
                         opt_mod.EPS, b1c, b2c)
    # ... and the Trainer's step
    seen = []
    _record_backward(monkeypatch, raster, seen)
    with pytest.raises(ValueError):
        t.train_step(cam, gt, want_loss=False)  # the key is on: which view's grid?
    assert t.iter == 0
    got_loss = t.train_step(cam, gt, want_loss=True, view_index=view)
    torch.cuda.synchronize()
    assert t.iter == 1 and t.last_regularisers == {"bilagrid_tv": tv_weight} and counts[view] == steps_before + 1
    assert np.float32(got_loss).tobytes() == np.float32(loss).tobytes()
    assert len(seen) == 1 and _np(seen[0]).tobytes() == _np(grad_render).tobytes()
    assert _np(seen[0]).tobytes() != _np(grad_corrected).tobytes()
    others = [v for v in range(4) if v != view]
    for now, before in ((t.bilagrids, grid0), (m, m0), (sq, sq0)):
        assert _np(now[others]).tobytes() == _np(before[others]).tobytes()  # the other views' grids: untouched
    moved = np.abs(_np(t.bilagrids[view]) - _np(grid0[view]))
    print(f"[{shape}] one step: loss {got_loss:.6f}, largest move of the grid {moved.max():.3e}; against the hand-composed "
          f"step: worst |difference| {np.abs(_np(t.bilagrids[view]) - want[0]).max():.3e}")
    assert moved.max() > 0
    np.testing.assert_allclose(_np(t.bilagrids[view]), want[0], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(_np(m[view]), want[1], rtol=2e-6, atol=1e-12)
    np.testing.assert_allclose(_np(sq[view]), want[2], rtol=2e-6, atol=1e-20)
    # the gaussians moved too: they see the gradient behind the grid
    assert not torch.equal(t.params["rgb"], init["rgb"])


def test_key_off_and_before_the_start_nothing_new_runs(gpu, scene, setup, monkeypatch):
    torch, ops, raster = gpu, pkg("ops"), pkg("raster")
    _, views, _ = setup
    calls = []
    for name in ("bilagrid_slice", "bilagrid_slice_backward", "bilagrid_tv_loss", "adam_step", "fused_loss"):
        real = getattr(ops, name)

        def counting(*a, _real=real, _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)

        monkeypatch.setattr(ops, name, counting)
    seen = []
    _record_backward(monkeypatch, raster, seen)
    cam, gt = views[0]
    off = _trainer(setup)
    assert off.bilagrids is None and off._bilagrid_state is None
    off.train_step(cam, gt, want_loss=False)
    off.train_step(cam, gt, want_loss=False, view_index=0)  # (accepted and ignored)
    torch.cuda.synchronize()
    assert calls == ["fused_loss", "fused_loss"] and off._grad_render == {} and len(off._grad_image) == 1
    assert off.last_regularisers == {} and off.bilagrids is None
    assert len(seen) == 2
    with pytest.raises(ValueError):
        off.render_corrected(0)
    # the key on, but not yet started: the same calls, and the grids stay the identity
    del calls[:]
    late = _trainer(setup, bilagrid=True, bilagrid_shape=(2, 2, 2), bilagrid_start=1)
    late.train_step(cam, gt, want_loss=False, view_index=0)
    torch.cuda.synchronize()
    assert calls == ["fused_loss"] and late._grad_render == {} and late.last_regularisers == {}
    assert _np(late.bilagrids).tobytes() == _np(ops.identity_bilagrid(2, 2, 2, views=4)).tobytes()
    late.train_step(cam, gt, want_loss=False, view_index=0)
    torch.cuda.synchronize()
    assert calls[1:] == ["bilagrid_slice", "fused_loss", "bilagrid_slice_backward", "bilagrid_tv_loss", "adam_step"]
    assert late.last_regularisers == {"bilagrid_tv": 10.0} and late._bilagrid_state[2] == [1, 0, 0, 0]
    assert list(late._grad_render) == [(96, 160)] and not torch.equal(late.bilagrids[0], ops.identity_bilagrid(2, 2, 2))


def test_refusals(gpu, scene, setup):
    class TwoRanks:
        world, rank = 2, 0

    init, views, cfg = setup
    make = lambda config, **kw: pkg("trainer").Trainer(_clone(init), views, dict(cfg, **config), scene_extent=5.0, seed=3, **kw)
    with pytest.raises(ValueError):
        make(dict(bilagrid=True), comm=TwoRanks())
    for shape in ((16, 16), (0, 16, 8), (16, 65, 8), (16, 16, 17), (16.0, 16, 8), "16x16x8", None):
        with pytest.raises(ValueError):
            make(dict(bilagrid=True, bilagrid_shape=shape))
    make(dict(bilagrid_shape=None))  # (the key is off: nothing reads the shape)
    t = make(dict(bilagrid=True, bilagrid_shape=(2, 2, 2)))
    cam, gt = views[0]
    for bad in (None, -1, 4):
        with pytest.raises(ValueError):
            t.train_step(cam, gt, want_loss=False, view_index=bad)
        with pytest.raises(ValueError):
            t.render_corrected(bad)
    assert t.iter == 0


def test_it_learns_and_the_corrected_render(gpu, scene, setup):
    """Every view's photograph is the scene's own render times per-channel gains 0.3 away from 1, in mixed directions.
    With the key the training loss ends below the run without it, and every off-1 gain has pulled the mean of its diagonal
    coefficient off 1 in its own direction."""
    torch, ops = gpu, pkg("ops")
    _, views, cfg = setup
    gains = torch.tensor(GAINS, device="cuda")
    gained = [(cam, (gt * gains[v]).contiguous()) for v, (cam, gt) in enumerate(views)]

    def final_loss(t, corrected):
        total = 0.0
        for v, (cam, gt) in enumerate(gained):
            H, W = int(cam["height"]), int(cam["width"])
            image = t.render_corrected(v) if corrected else _raw_render(t, cam)
            total += ops.fused_loss(image, gt, H, W, float(t.cfg["ssim_frac"]), torch.empty(H, W, 3, device="cuda"), blocking=True)
        return total / len(gained)

    with_key = _trainer(setup, views=gained, bilagrid=True)
    without = _trainer(setup, views=gained)
    assert tuple(with_key.cfg["bilagrid_shape"]) == (16, 16, 8) and with_key.cfg["bilagrid_lr"] == 0.002
    with_key.train(ITERS, loss_every=0)
    without.train(ITERS, loss_every=0)
    torch.cuda.synchronize()
    loss_on, loss_off = final_loss(with_key, True), final_loss(without, False)
    psnr_on, psnr_off = with_key.evaluate(views), without.evaluate(views)
    print(f"after {ITERS} iterations on gained photographs: training loss {loss_on:.6f} with the key, {loss_off:.6f} without; "
          f"raw-render PSNR against the un-gained images {psnr_on:.3f} dB with, {psnr_off:.3f} dB without; "
          f"steps per view {with_key._bilagrid_state[2]}")
    assert sum(with_key._bilagrid_state[2]) == ITERS
    assert loss_on < loss_off
    diag = _np(with_key.bilagrids)[:, [0, 5, 10]].reshape(4, 3, -1).mean(-1)  # [view, channel]
    print("mean diagonal coefficients per view and channel:\n", diag)
    for v in range(4):
        for c in range(3):
            if GAINS[v][c] != 1.0:
                assert (diag[v, c] - 1.0) * (GAINS[v][c] - 1.0) > 0, (v, c, diag[v, c])
    # render_corrected: bilagrid_slice of the render-only forward, bit for bit
    for v, (cam, _) in enumerate(gained):
        want = ops.bilagrid_slice(with_key.bilagrids[v], _raw_render(with_key, cam))
        assert torch.equal(with_key.render_corrected(v), want)
        assert not torch.equal(want, _raw_render(with_key, cam))


def _raw_render(t, cam):
    ctx = t._context_for(t.num_gaussians)
    ctx.set_render_only(True)
    try:
        return ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)["image"].clone()
    finally:
        ctx.set_render_only(False)

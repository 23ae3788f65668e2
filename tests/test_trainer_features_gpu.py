"""The Trainer's feature field (config key features) on the generated 3000-gaussian, 160x96, four-view scene of
tests/test_absgrad_gpu.py.  Labels: every truth gaussian gets one of four labels from the signs of two of its coordinates,
the one-hot [N,4] is rendered with render_features on the truth state per view, and a pixel's label is the argmax where
the opacity 1 - T is at least 0.5, -1 (ignored) elsewhere.

One step against its pieces: the compositing backward and lift_features add with float atomics in arrival order, so two
runs of the same step differ in the last bits of a lifted gradient (tests/test_trainer_distortion_gpu.py says the same of
its rows).  The column itself is held to the Adam reference's single-step tolerance (tests/test_optimizer_gpu.py) against
the step composed by hand; the two moments, which are proportional to the gradient and so carry a cancelling gradient's
last bits at full size, are held to that tolerance against the Adam reference on the very gradient the step consumed,
and that gradient to the bar tests/test_features_gpu.py holds two lifts of one map to."""
import math

import numpy as np
import pytest

import feature_loss_reference as flr
from conftest import assert_grad_close, pkg
from test_absgrad_gpu import _training_setup

pytestmark = pytest.mark.gpu

ITERS = 36  # the iteration count of that scene's training tests
C = 4


def _np(t):
    return t.detach().cpu().numpy()


def _clone(init):
    return {k: v.clone() for k, v in init.items()}


def build_setup(torch, scene):
    """(init, views with the label map as fifth element, plain views, cfg, labels as numpy)."""
    raster = pkg("raster")
    init, views, cfg = _training_setup(torch, scene)
    N, W, H = 3000, 160, 96
    truth = scene.make_gaussians(N, W, H, 0)  # _training_setup's truth state
    truth["opacity"][:] = np.clip(truth["opacity"], 0.5, 3.0)
    centred = truth["xyz"] - np.median(truth["xyz"], 0)
    label_of = (centred[:, 0] > 0).astype(np.int64) + 2 * (centred[:, 1] > 0).astype(np.int64)
    onehot = torch.from_numpy(np.eye(C, dtype=np.float32)[label_of]).cuda()
    ctx = raster.RasterContext(N, W, H)
    ctx.set_render_only(True)
    dpt = raster.device_params(truth)
    labelled = []
    for cam, gt in views:
        fwd = ctx.rasterize_image(dpt, cam, scene.CONFIG, 0.0, 0)
        fmap = ctx.render_features(onehot)
        lab = torch.where(1.0 - fwd["T"] >= 0.5, fmap.argmax(-1), torch.full_like(fmap.argmax(-1), -1)).to(torch.int32)
        labelled.append((cam, gt, None, None, lab.contiguous()))
    torch.cuda.synchronize()
    labels = [_np(v[4]) for v in labelled]
    assert len(np.unique(np.concatenate([l[l >= 0] for l in labels]))) == C and all((l >= 0).mean() > 0.05 for l in labels)
    return init, labelled, views, cfg, labels


@pytest.fixture(scope="module")
def setup(gpu, scene):
    return build_setup(gpu, scene)  # built once


def _trainer(setup, views=None, features=None, init=None, **keys):
    labelled, cfg = setup[1], setup[3]
    init = setup[0] if init is None else init
    return pkg("trainer").Trainer(_clone(init), labelled if views is None else views, dict(cfg, features=C, **keys),
                                  scene_extent=5.0, seed=3, features=features)


def _target(torch, kind, labels, seed=0):
    """A view's feature target for `kind` from its label map: the labels, or a one-hot-ish float map with a validity map."""
    if kind == "ce":
        return labels
    lab = _np(labels)
    rng = np.random.default_rng(seed)
    target = (np.eye(C, dtype=np.float32)[np.clip(lab, 0, C - 1)] + 0.1 * rng.standard_normal(lab.shape + (C,))).astype(np.float32)
    return torch.from_numpy(target).cuda(), torch.from_numpy((lab >= 0).astype(np.uint8)).cuda()


@pytest.mark.parametrize("kind", ["ce", "l1", "cosine"])
def test_one_step_is_what_its_pieces_say(gpu, scene, setup, monkeypatch, kind):
    torch, ops, raster, opt_mod = gpu, pkg("ops"), pkg("raster"), pkg("optimizer")
    init, labelled, _, cfg, _ = setup
    N = init["xyz"].shape[0]
    init = _clone(init)
    init["xyz"][::7, 2] *= -1.0  # the view sees the whole scene: a seventh of the rows goes behind it (identity pose, +z)
    # ce starts from the default, zeros; the other two from a random column (the cosine of a zero row has no gradient)
    feats0 = None if kind == "ce" else torch.from_numpy(np.random.default_rng(1).standard_normal((N, C)).astype(np.float32)).cuda()
    t = _trainer(setup, features=None if feats0 is None else feats0.clone(), init=init, feature_loss=kind, feature_weight=0.5)
    if feats0 is None:
        feats0 = torch.zeros(N, C, device="cuda")
    assert torch.equal(t.features, feats0) and t.features.shape == (N, C)
    cam, gt, _, _, labels = labelled[0]
    H, W = int(cam["height"]), int(cam["width"])
    target = _target(torch, kind, labels)
    # the pieces, on a context of their own, from the initial state
    ctx = raster.RasterContext(N, W, H)
    p = {k: v.clone() for k, v in t.params.items()}
    fwd = ctx.rasterize_image(p, cam, t.cfg, 0.0, t.l_max)  # (use_background=False: background 0)
    fmap = ctx.render_features(feats0)
    if kind == "ce":
        ref = flr.ce_loss(_np(fmap), _np(target), 0.5)
    else:
        ref = flr.LOSSES[kind](_np(fmap), _np(target[0]), _np(target[1]), 0.5)
    grad_map = torch.from_numpy(ref[1].astype(np.float32)).cuda()
    lifted = _np(ctx.lift_features(grad_map, torch.zeros(N, C, device="cuda")))
    seen = np.sort(_np(fwd["compact_to_global"]).astype(np.int64))
    assert 0 < len(seen) < N and np.abs(lifted).max() > 0
    b1c, b2c = opt_mod.AdamOptimizer.bias_corrections(0)
    adam = lambda g: flr.adam_step(_np(feats0)[seen], g[seen], np.zeros((len(seen), C)), np.zeros((len(seen), C)),
                                   t.cfg["feature_lr"], opt_mod.B1, opt_mod.B2, opt_mod.EPS, b1c, b2c)
    want = adam(lifted)
    # ... and the Trainer's step, with the gradient it consumed kept
    consumed, real = {}, ops.feature_adam_step

    def keeping(c2g, m, f, ea, eas, grad, *rest):
        consumed["grad"], consumed["rows"] = grad.clone(), (c2g[:m].clone(), m)
        return real(c2g, m, f, ea, eas, grad, *rest)

    monkeypatch.setattr(ops, "feature_adam_step", keeping)
    t.train_step(cam, gt, want_loss=False, feature_target=target)
    torch.cuda.synchronize()
    assert t.last_regularisers == {"feature": 0.5} and t.iter == 1
    assert np.array_equal(np.sort(_np(consumed["rows"][0]).astype(np.int64)), seen)
    got, got_m, got_v = _np(t.features), _np(t._feat[1]), _np(t._feat[2])
    hidden = np.ones(N, bool)
    hidden[seen] = False
    assert got[hidden].tobytes() == _np(feats0)[hidden].tobytes() and not got_m[hidden].any() and not got_v[hidden].any()
    moved = np.abs(got[seen] - _np(feats0)[seen])
    print(f"[{kind}] one step: {len(seen)} of {N} rows seen, largest move {moved.max():.3e}; column against the hand-composed "
          f"step: worst |difference| {np.abs(got[seen] - want[0]).max():.3e}")
    assert moved.max() > 0
    np.testing.assert_allclose(got[seen], want[0], rtol=2e-6, atol=1e-7)
    g = _np(consumed["grad"])[:N]
    assert_grad_close(g, lifted, "the consumed gradient against lift_features of the reference's map", rel=1e-6)
    assert not g[hidden].any()
    mine = adam(g)
    np.testing.assert_allclose(got[seen], mine[0], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(got_m[seen], mine[1], rtol=2e-6, atol=1e-12)
    np.testing.assert_allclose(got_v[seen], mine[2], rtol=2e-6, atol=1e-20)
    assert not bool(t._feat_grad.any())  # consumed rows are zero again, the others never were anything else


def test_it_learns(gpu, scene, setup):
    """Zero features give a uniform softmax: the initial mean cross-entropy over the views is ln 4 x the labelled share of
    the pixels.  After the scene's 36 iterations at the default feature_lr the loss is below that and the accuracy above
    what the constant predictor of the most frequent label reaches on the label maps."""
    torch = gpu
    _, _, _, _, labels = setup
    start = float(np.mean([math.log(C) * (l >= 0).mean() for l in labels]))
    counts = np.sum([np.bincount(l[l >= 0], minlength=C) for l in labels], 0)
    constant = counts.max() / counts.sum()
    t = _trainer(setup)
    assert t.cfg["feature_lr"] == 0.0025 and t.cfg["feature_loss"] == "ce"
    first = t.evaluate_features()
    assert first["views"] == 4 and abs(first["loss"] - start) <= 1e-6 * start
    t.train(ITERS, loss_every=0)
    torch.cuda.synchronize()
    after = t.evaluate_features()
    print(f"mean cross-entropy over the views: {start:.6f} at zero features (ln 4 x the labelled share), {after['loss']:.6f} "
          f"after {ITERS} iterations; accuracy {after['accuracy']:.4f} against {constant:.4f} for the most frequent label")
    assert after["loss"] < start and after["accuracy"] > constant
    assert t.evaluate() > 0 and not bool(t._feat_grad.any())


def test_geometry_off_leaves_the_image_training_alone(gpu, scene, setup):
    torch, trainer_mod = gpu, pkg("trainer")
    init, labelled, views, cfg, _ = setup
    N = init["xyz"].shape[0]
    feats = torch.from_numpy(np.random.default_rng(2).standard_normal((N, C)).astype(np.float32)).cuda()
    plain = trainer_mod.Trainer(_clone(init), views, cfg, scene_extent=5.0, seed=3)
    off = _trainer(setup, features=feats.clone())
    on = _trainer(setup, features=feats.clone(), feature_geometry=True)
    cam, gt, _, _, labels = labelled[0]
    plain.train_step(cam, gt, want_loss=False)
    off.train_step(cam, gt, want_loss=False, feature_target=labels)
    on.train_step(cam, gt, want_loss=False, feature_target=labels)
    torch.cuda.synchronize()
    assert plain.last_regularisers == {} and off.last_regularisers == on.last_regularisers == {"feature": 1.0}
    for k in ("xyz", "opacity", "scale", "quaternion", "rgb"):  # (float atomics add in arrival order: not bitwise)
        assert_grad_close(_np(off.params[k]), _np(plain.params[k]), k, rel=1e-5)
        assert_grad_close(_np(off.opt.exp_avg[k]), _np(plain.opt.exp_avg[k]), "exp_avg " + k, rel=1e-5)
    assert not torch.equal(off.features, feats)
    for k in ("xyz", "opacity"):
        assert not torch.allclose(on.opt.exp_avg[k], plain.opt.exp_avg[k], rtol=1e-3, atol=0)
    assert_grad_close(_np(on.opt.exp_avg["rgb"]), _np(plain.opt.exp_avg["rgb"]), "exp_avg rgb", rel=1e-5)  # no colour term


def _with_ids(setup, **keys):
    """A trainer whose feature rows carry the gaussian's id in channel 0 (exact in float32 at these counts), non-zero
    feature moments, and the xyz rows remembered by id."""
    import torch
    init = setup[0]
    N = init["xyz"].shape[0]
    feats = torch.from_numpy(np.random.default_rng(3).standard_normal((N, C)).astype(np.float32)).cuda()
    feats[:, 0] = torch.arange(N, dtype=torch.float32, device="cuda")
    t = _trainer(setup, features=feats, **keys)
    t._feat[1].copy_(feats * 0.25 + 1.0)
    t._feat[2].copy_(feats * feats + 1.0)
    return t, _np(feats).copy(), _np(t.params["xyz"]).copy()


def _ids(t):
    ids = _np(t.features)[:, 0]
    assert (ids == np.round(ids)).all()
    return ids.astype(np.int64)


def _assert_rows_follow(t, feats0, xyz0, moments=True):
    """Every row's channel 0 names the gaussian whose xyz the row holds, and the rest of its feature row (and moments)."""
    ids = _ids(t)
    assert _np(t.params["xyz"]).tobytes() == xyz0[ids].tobytes()
    assert _np(t.features).tobytes() == feats0[ids].tobytes()
    if moments:
        assert _np(t._feat[1]).tobytes() == (feats0 * np.float32(0.25) + np.float32(1.0))[ids].tobytes()
        assert _np(t._feat[2]).tobytes() == (feats0 * feats0 + np.float32(1.0))[ids].tobytes()
    return ids


def test_the_column_follows_sort_prune_and_the_sh_band(gpu, scene, setup):
    torch = gpu
    t, feats0, xyz0 = _with_ids(setup)
    N = t.num_gaussians
    t.sort_gaussians()
    ids = _assert_rows_follow(t, feats0, xyz0)
    assert sorted(ids) == list(range(N)) and (ids != np.arange(N)).any()
    scores = t.contribution_scores()
    removed = t.prune_by_contribution(threshold=float(scores["weight_max"].median()), scores=scores)  # about half
    ids = _assert_rows_follow(t, feats0, xyz0)
    assert 0 < removed < N and len(ids) == N - removed == len(set(ids))
    before, l_max = t.features, t.l_max
    t.add_sh_band()
    assert t.l_max == l_max + 1 and t.features is before
    _assert_rows_follow(t, feats0, xyz0)
    t.train_step(*setup[1][0][:2], want_loss=False, feature_target=setup[1][0][4])  # the step runs on the edited table
    torch.cuda.synchronize()
    assert not bool(t._feat_grad.any()) and t._feat_grad.shape[0] >= t.num_gaussians


def test_the_column_follows_a_density_step(gpu, scene, setup):
    torch, ops, trainer_mod = gpu, pkg("ops"), pkg("trainer")
    t, feats0, xyz0 = _with_ids(setup, uv_grad_threshold=0.0)
    for v in setup[1]:  # four steps: densification statistics, and real feature moments on the rows the views saw
        t.train_step(v[0], v[1], want_loss=False, feature_target=v[4])
    N = t.num_gaussians
    feats1, m1, v1 = (_np(x).copy() for x in t._feat)
    t.features[:, 0] = torch.arange(N, dtype=torch.float32, device="cuda")
    feats1[:, 0] = np.arange(N)  # (the four steps moved channel 0 like any other: the ids are written again)
    xyz1 = _np(t.params["xyz"]).copy()
    t.params["opacity"][:40] = -10.0  # below delete_opacity_threshold: pruned
    # clones and splits both: the clone / split boundary at the median size
    sizes = torch.exp(t.params["scale"]).max(1).values
    t.scene_extent = float(sizes.median()) / 0.01
    c = t.cfg
    prune, clone, split, keep, counts = ops.density_masks(
        t.params["opacity"], t.params["scale"], t.opt.uv_grad_accum, t.opt.grad_accum_dur,
        trainer_mod._logit(float(c["delete_opacity_threshold"])), t.scene_extent * 0.1, 0.0, t.scene_extent * 0.01)
    prune, clone, split = (_np(m).astype(bool) for m in (prune, clone, split))
    out = t.adaptive_density_step()
    torch.cuda.synchronize()
    assert out == dict(pruned=int(prune.sum()), cloned=int(clone.sum()), split=int(split.sum()), skipped=False)
    assert out["pruned"] >= 40 and out["cloned"] > 10 and out["split"] > 10
    keep_n = N - out["pruned"] - out["split"]
    ids = _ids(t)
    assert len(ids) == t.num_gaussians == keep_n + out["cloned"] + 2 * out["split"]
    times = np.bincount(ids, minlength=N)
    assert (times[clone] == 2).all() and (times[split] == 2).all() and (times[prune] == 0).all()
    assert (times[~(clone | split | prune)] == 1).all()
    new = np.arange(len(ids)) >= keep_n
    assert split[ids[new][out["cloned"]:]].all() and clone[ids[new][:out["cloned"]]].all()  # the parents of a split are gone
    assert not split[ids[~new]].any()
    assert _np(t.features).tobytes() == feats1[ids].tobytes()  # a copy carries its source's whole row
    assert _np(t.params["xyz"])[~new].tobytes() == xyz1[ids[~new]].tobytes()  # a kept row is still its gaussian's
    m, v = _np(t._feat[1]), _np(t._feat[2])
    assert not m[new].any() and not v[new].any()
    assert m[~new].tobytes() == m1[ids[~new]].tobytes() and v[~new].tobytes() == v1[ids[~new]].tobytes() and m[~new].any()


def test_the_column_follows_mcmc_relocation_and_growth(gpu, scene, setup):
    torch = gpu
    t, feats0, xyz0 = _with_ids(setup, mcmc=True)
    N = t.num_gaussians
    t.params["opacity"][5:45] = -10.0  # dead: below mcmc_min_opacity
    dead = np.zeros(N, bool)
    dead[5:45] = True
    moved = t.mcmc_relocate(seed=11)
    torch.cuda.synchronize()
    assert moved == 40
    ids = _assert_rows_follow(t, feats0, xyz0, moments=False)  # a moved row is its source's, position and features alike
    assert not dead[ids].any() and (ids[~dead] == np.arange(N)[~dead]).all()
    sources = np.unique(ids[dead])
    restarted = dead.copy()
    restarted[sources] = True
    m, v = _np(t._feat[1]), _np(t._feat[2])
    assert not m[restarted].any() and not v[restarted].any()
    assert m[~restarted].tobytes() == (feats0 * np.float32(0.25) + np.float32(1.0))[~restarted].tobytes()
    # growth, on a table of its own (after a relocation a source and its copies share a position)
    t, feats0, xyz0 = _with_ids(setup, mcmc=True)
    t._feat[1].fill_(1.0)
    t._feat[2].fill_(1.0)
    xyz1, feats1 = xyz0, feats0
    added = t.mcmc_grow(seed=12)
    torch.cuda.synchronize()
    assert added == int(1.05 * N) - N and t.num_gaussians == N + added
    got_f, got_xyz = _np(t.features), _np(t.params["xyz"])
    assert got_f[:N].tobytes() == feats1.tobytes()
    # a new row is a copy of one old row: its features and its position name the same one
    src = np.array([int(np.flatnonzero((xyz1 == got_xyz[N + k]).all(1))[0]) for k in range(added)])
    assert got_f[N:].tobytes() == feats1[src].tobytes()
    m = _np(t._feat[1])
    restarted = np.zeros(N + added, bool)
    restarted[N:] = True
    restarted[src] = True
    assert not m[restarted].any() and (m[~restarted] == 1.0).all() and _np(t._feat[2])[~restarted].all()
    t.train_step(*setup[1][0][:2], want_loss=False, feature_target=setup[1][0][4])
    torch.cuda.synchronize()
    assert not bool(t._feat_grad.any())


def test_views_without_a_target_skip_the_term(gpu, scene, setup, monkeypatch):
    torch, ops, raster = gpu, pkg("ops"), pkg("raster")
    init, labelled, views, cfg, _ = setup
    N = init["xyz"].shape[0]
    feats = torch.from_numpy(np.random.default_rng(4).standard_normal((N, C)).astype(np.float32)).cuda()

    def refuse(*a, **k):
        raise AssertionError("a feature launch in a step without a target")

    late = _trainer(setup, features=feats.clone(), feature_start=5)  # (before feature_start: the same)
    t = _trainer(setup, views=views, features=feats.clone())
    for name in ("feature_ce_loss", "feature_l1_loss", "feature_cosine_loss", "feature_adam_step"):
        monkeypatch.setattr(ops, name, refuse)
    for name in ("render_features", "lift_features", "features_backward"):
        monkeypatch.setattr(raster.RasterContext, name, refuse)
    t.train(2, loss_every=0)
    t.train_step(labelled[0][0], labelled[0][1], want_loss=False, feature_target=None)
    late.train_step(labelled[0][0], labelled[0][1], want_loss=False, feature_target=labelled[0][4])
    torch.cuda.synchronize()
    for tr in (t, late):
        assert torch.equal(tr.features, feats) and not bool(tr._feat[1].any()) and not bool(tr._feat[2].any())
        assert tr._feat_grad is None and tr._feat_maps == {} and tr.last_regularisers == {}
    assert t.evaluate_features() is None


def test_refusals_and_the_key_off(gpu, scene, setup):
    torch, trainer_mod = gpu, pkg("trainer")
    init, labelled, views, cfg, _ = setup
    N = init["xyz"].shape[0]

    class TwoRanks:
        world, rank = 2, 0

    make = lambda config, **kw: trainer_mod.Trainer(_clone(init), labelled, dict(cfg, **config), scene_extent=5.0, seed=3, **kw)
    with pytest.raises(ValueError):
        make(dict(features=C), comm=TwoRanks())
    for bad in (torch.zeros(N - 1, C, device="cuda"), torch.zeros(N, C + 1, device="cuda"),
                torch.zeros(N, C, dtype=torch.float64, device="cuda"), torch.zeros(N, C)):
        with pytest.raises(ValueError):
            make(dict(features=C), features=bad)
    with pytest.raises(ValueError):
        make(dict(features=C, feature_loss="l2"))
    with pytest.raises(ValueError):
        make(dict(features=513))
    with pytest.raises(ValueError):
        make(dict(), features=torch.zeros(N, C, device="cuda"))  # a column without the key
    cam, gt, _, _, labels = labelled[0]
    H, W = labels.shape
    t = make(dict(features=C))
    for target in (labels.float(), labels.long(), labels[:-1], labels.cpu(), torch.zeros(H, W, C, device="cuda")):
        with pytest.raises(ValueError):
            t.train_step(cam, gt, want_loss=False, feature_target=target)
    t1 = make(dict(features=C, feature_loss="l1"))
    good = torch.zeros(H, W, C, device="cuda")
    for target in (labels, good[..., :3], good.double(), (good, labels), (good, torch.ones(H, W + 1, dtype=torch.uint8, device="cuda")),
                   (good,)):
        with pytest.raises(ValueError):
            t1.train_step(cam, gt, want_loss=False, feature_target=target)
    assert t.iter == 0 and t1.iter == 0 and not bool(t.features.any())
    # the key off: no column, nothing allocated, and a feature target given anyway is not looked at
    off = make(dict())
    off.train_step(cam, gt, want_loss=False, feature_target=labels)
    assert off.features is None and off._feat is None and off._feat_grad is None and off._feat_maps == {}
    assert off._rows().features is None and off.last_regularisers == {}
    with pytest.raises(ValueError):
        off.evaluate_features()

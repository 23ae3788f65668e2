"""The six row edits of the Trainer, each run once on one small Trainer and each made to do something: what every one of
them leaves in ALL per-gaussian columns (parameters, both moments of every group, the two statistics), what it leaves
bound to what (the optimizer to the parameter tensors, the view-sharded step, the 3D filter) -- and then the run goes on.
The statistics' policy per edit is the table in CHANGELOG.md: kept by add_sh_band and mcmc_relocate, moved by
sort_gaussians and prune_by_contribution, zero at the new length after adaptive_density_step and mcmc_grow."""
import math

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

N, W, H = 300, 64, 48
# read as float32: a denormal, a signalling NaN, a quiet NaN with a payload, another NaN; and ordinary counts
SPECIAL_COUNTS = np.array([1, 0x7F800001, 0x7FC00001, 0xFFFFFFFF, 3, 12, 0, 7], np.uint32).view(np.int32)
M_TAG, V_TAG = 0.25, 0.5


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _columns(t):
    """name -> tensor, every per-gaussian column of the run."""
    cols = {"params." + g: v for g, v in t.params.items()}
    cols.update({"exp_avg." + g: t.opt.exp_avg[g] for g in t.opt.names})
    cols.update({"exp_avg_sq." + g: t.opt.exp_avg_sq[g] for g in t.opt.names})
    cols["uv_grad_accum"], cols["grad_accum_dur"] = t.opt.uv_grad_accum, t.opt.grad_accum_dur
    return cols


def _tag(torch, t):
    """Row i: exp_avg i + 0.25 and exp_avg_sq i + 0.5 in every element, uv_grad_accum i / 2 + 0.125, grad_accum_dur
    cycling through SPECIAL_COUNTS.  Returns a copy of every column."""
    n = t.num_gaussians
    ids = torch.arange(n, dtype=torch.float32, device="cuda")
    for g in t.opt.names:
        shape = (n,) + (1,) * (t.opt.exp_avg[g].dim() - 1)
        t.opt.exp_avg[g].copy_((ids + M_TAG).reshape(shape).expand_as(t.opt.exp_avg[g]))
        t.opt.exp_avg_sq[g].copy_((ids + V_TAG).reshape(shape).expand_as(t.opt.exp_avg_sq[g]))
    t.opt.uv_grad_accum.copy_(ids * 0.5 + 0.125)
    t.opt.grad_accum_dur.copy_(torch.from_numpy(np.resize(SPECIAL_COUNTS, n)))
    return {k: v.clone() for k, v in _columns(t).items()}


def _moment_ids(torch, t):
    """The row id each row's moments carry (-1: all of them zero); every moment column has to agree, element by element."""
    n = t.num_gaussians
    first = t.opt.exp_avg["xyz"][:, 0]
    ids = torch.where(first == 0, torch.full_like(first, -1.0), first - M_TAG)
    for g in t.opt.names:
        for m, tag in ((t.opt.exp_avg[g], M_TAG), (t.opt.exp_avg_sq[g], V_TAG)):
            want = torch.where(ids < 0, torch.zeros_like(ids), ids + tag).reshape((n,) + (1,) * (m.dim() - 1)).expand_as(m)
            assert torch.equal(m, want), g
    return ids.long()


def _assert_columns_are_rows_of(torch, t, before, index, what):
    after = _columns(t)
    assert after.keys() == before.keys()
    for k in before:
        assert after[k].dtype == before[k].dtype and _bits(after[k]) == _bits(before[k][index]), (what, k)


def _assert_statistics(torch, t, want_accum, want_dur, what):
    assert _bits(t.opt.uv_grad_accum) == _bits(want_accum) and t.opt.uv_grad_accum.dtype == torch.float32, what
    assert _bits(t.opt.grad_accum_dur) == _bits(want_dur) and t.opt.grad_accum_dur.dtype == torch.int32, what


def _assert_installed(torch, t, what, sharded=None):
    """What holds after every edit, whatever it did to the rows."""
    n = t.num_gaussians
    nsh = (t.l_max + 1) ** 2 - 1
    shapes = dict(xyz=(n, 3), rgb=(n, 3), sh=(n, nsh, 3), opacity=(n,), scale=(n, 3), quaternion=(n, 4))
    assert list(t.params) == list(shapes) and t.opt.names == list(shapes) and t.opt.l_max == t.l_max, what
    for g, shape in shapes.items():
        for c in (t.params[g], t.opt.exp_avg[g], t.opt.exp_avg_sq[g]):
            assert tuple(c.shape) == shape and c.dtype == torch.float32 and c.is_contiguous(), (what, g)
        assert t.opt.params[g].data_ptr() == t.params[g].data_ptr(), (what, g)
    assert t.opt.uv_grad_accum.shape == (n,) and t.opt.uv_grad_accum.dtype == torch.float32, what
    assert t.opt.grad_accum_dur.shape == (n,) and t.opt.grad_accum_dur.dtype == torch.int32, what
    assert t._sharded is sharded, what
    assert t.filter3d.shape == (n,) and t.filter3d.dtype == torch.float32, what


def test_every_row_edit_moves_every_column(gpu, scene, monkeypatch):
    torch, raster, ops, trainer_mod = gpu, pkg("raster"), pkg("ops"), pkg("trainer")
    truth = scene.make_gaussians(N, W, H, 0)
    truth["opacity"][:] = np.clip(truth["opacity"], 0.5, 3.0)
    ctx = raster.RasterContext(N, W, H)
    views = []
    for v in range(2):
        cam = raster.device_camera(scene.make_camera(W, H, v))
        views.append((cam, ctx.rasterize_image(raster.device_params(truth), cam, scene.CONFIG, 0.0, 0)["image"].clone()))
    init = scene.make_gaussians(N, W, H, 0, seed=7)
    # the density thresholds, from the rows themselves: a fifth is transparent enough to prune, and the boundary between
    # cloning and splitting (0.01 x the scene extent) is the median of the largest extents
    extent = np.exp(init["scale"].astype(np.float64)).max(1)
    scene_extent = float(np.median(extent)) / 0.01
    delete_below = float(1.0 / (1.0 + np.exp(-np.quantile(init["opacity"].astype(np.float64), 0.2))))
    dp = raster.device_params(init)
    dp.pop("sh", None)
    cfg = dict(filter3d=True, use_background=False, delete_opacity_threshold=delete_below, max_gaussians=2000)
    t = trainer_mod.Trainer(dp, views, cfg, scene_extent=scene_extent, seed=3)
    t.add_sh_band()
    assert t.l_max == 1 and t.num_gaussians == N
    _assert_installed(torch, t, "a fresh Trainer at SH degree 1")
    stale = object()  # stands for a view-sharded step bound to the tensors of before

    # ---- add_sh_band, degree 1 -> 2: the same rows; `sh` and its moments re-laid out, everything else kept
    before, t._sharded = _tag(torch, t), stale
    t.add_sh_band()
    _assert_installed(torch, t, "add_sh_band")
    assert t.l_max == 2
    for name, old in (("params.sh", before["params.sh"]), ("exp_avg.sh", before["exp_avg.sh"]),
                      ("exp_avg_sq.sh", before["exp_avg_sq.sh"])):
        new = _columns(t)[name]
        assert _bits(new[:, :3]) == _bits(old) and not bool(new[:, 3:].any()), name
    ids = torch.arange(N, device="cuda", dtype=torch.float32)
    assert torch.equal(t.opt.exp_avg["sh"][:, :3], (ids + M_TAG).reshape(N, 1, 1).expand(N, 3, 3))
    after = _columns(t)
    for k in before:
        if not k.endswith(".sh"):
            assert _bits(after[k]) == _bits(before[k]), ("add_sh_band", k)
    _assert_statistics(torch, t, before["uv_grad_accum"], before["grad_accum_dur"], "add_sh_band keeps the statistics")

    # ---- sort_gaussians: every column gathered by one order
    before, t._sharded = _tag(torch, t), stale
    t.sort_gaussians()
    _assert_installed(torch, t, "sort_gaussians")
    order = _moment_ids(torch, t)
    assert sorted(order.tolist()) == list(range(N)) and order.tolist() != list(range(N))
    _assert_columns_are_rows_of(torch, t, before, order, "sort_gaussians")

    # ---- adaptive_density_step: [kept | clones | split pairs]; moments follow the kept rows, statistics zero
    _tag(torch, t)
    t.opt.uv_grad_accum.copy_((torch.arange(N, device="cuda") % 3 != 0).float())  # two rows in three have a gradient
    t.opt.grad_accum_dur.fill_(1)
    prune, clone, split, keep, counts = ops.density_masks(
        t.params["opacity"], t.params["scale"], t.opt.uv_grad_accum, t.opt.grad_accum_dur,
        trainer_mod._logit(delete_below), scene_extent * 0.1, float(t.cfg["uv_grad_threshold"]), scene_extent * 0.01)
    before, t._sharded, t.iter = {k: v.clone() for k, v in _columns(t).items()}, stale, 5
    result = t.adaptive_density_step()
    assert result == dict(pruned=counts[0], cloned=counts[1], split=counts[2], skipped=False) and min(counts) > 0, result
    kept = keep.bool().nonzero().reshape(-1)
    n = len(kept) + counts[1] + 2 * counts[2]
    assert t.num_gaussians == n
    _assert_installed(torch, t, "adaptive_density_step")
    assert _moment_ids(torch, t).tolist() == kept.tolist() + [-1] * (n - len(kept))
    for g in t.params:
        assert _bits(t.params[g][:len(kept)]) == _bits(before["params." + g][kept]), g
        clones = before["params." + g][clone.bool()]
        assert _bits(t.params[g][len(kept):len(kept) + counts[1]]) == _bits(clones), g
    zeros = torch.zeros(n, device="cuda")
    _assert_statistics(torch, t, zeros, zeros.int(), "adaptive_density_step zeroes the statistics")

    # ---- mcmc_relocate: in place; 20 dead rows become copies, moments restart on them and their sources
    t.params["opacity"].fill_(1.0)
    dead = torch.arange(20, device="cuda") * 7 + 3
    t.params["opacity"][dead] = -8.0
    before, t._sharded = _tag(torch, t), stale
    tensors = {k: (v, v.data_ptr()) for k, v in _columns(t).items()}
    drawn, real = {}, ops.sample_by_weight

    def recording(weights, K, seed, counts=None):
        drawn["samples"], _ = out = real(weights, K, seed, counts)
        return out

    monkeypatch.setattr(ops, "sample_by_weight", recording)
    t.filter3d  # (computed: the edit has to drop it)
    assert t._filter3d is not None
    assert t.mcmc_relocate() == 20
    assert t._filter3d is None
    _assert_installed(torch, t, "mcmc_relocate", sharded=stale)
    for k, v in _columns(t).items():
        assert v is tensors[k][0] and v.data_ptr() == tensors[k][1], ("mcmc_relocate replaced", k)
    src = drawn["samples"].long()
    assert len(src) == 20 and not bool(torch.isin(src, dead).any())
    want = torch.arange(n, device="cuda")
    want[torch.cat([src, dead])] = -1
    assert torch.equal(_moment_ids(torch, t), want)
    for g in t.params:
        assert _bits(t.params[g][dead]) == _bits(t.params[g][src]), g
    _assert_statistics(torch, t, before["uv_grad_accum"], before["grad_accum_dur"], "mcmc_relocate keeps the statistics")

    # ---- mcmc_grow: [old | copies of the drawn]; moments zero on the drawn and the new, statistics zero
    before, t._sharded = _tag(torch, t), stale
    k = trainer_mod.mcmc_growth(n, 1.05, 2000)
    assert t.mcmc_grow() == k == int(1.05 * n) - n > 0
    _assert_installed(torch, t, "mcmc_grow")
    assert t.num_gaussians == n + k and t.ctx_capacity >= n + k
    src = drawn["samples"].long()
    assert len(src) == k
    want = torch.cat([torch.arange(n, device="cuda"), torch.full((k,), -1, device="cuda")])
    want[src] = -1
    assert torch.equal(_moment_ids(torch, t), want) and int((want >= 0).sum()) >= n - k
    for g in t.params:
        assert _bits(t.params[g][n:]) == _bits(t.params[g][src]), g
        if g not in ("opacity", "scale"):  # (those two are corrected on the drawn rows)
            assert _bits(t.params[g][:n]) == _bits(before["params." + g]), g
    n += k
    zeros = torch.zeros(n, device="cuda")
    _assert_statistics(torch, t, zeros, zeros.int(), "mcmc_grow zeroes the statistics")
    monkeypatch.undo()

    # ---- prune_by_contribution with given scores: every column compacted by one mask
    before, t._sharded = _tag(torch, t), stale
    gone = torch.arange(n, device="cuda") % 7 == 2
    scores = dict(weight_sum=None, weight_max=torch.where(gone, 0.1, 0.9), pixels=torch.ones(n, dtype=torch.int32, device="cuda"))
    assert t.prune_by_contribution(0.5, scores=scores) == int(gone.sum()) > 0
    _assert_installed(torch, t, "prune_by_contribution")
    assert t.num_gaussians == n - int(gone.sum())
    _assert_columns_are_rows_of(torch, t, before, ~gone, "prune_by_contribution")

    # ---- and the run goes on
    loss = t.train_step(*views[0])
    assert loss is not None and math.isfinite(loss)
    assert t.ctx._filter3d is t.filter3d and t.ctx._filter3d.numel() == t.num_gaussians

"""Training a feature field, without a GPU: the float64 reference of the three feature losses
(tests/feature_loss_reference.py) against central differences and at its edge cases, the new entry points exported, bound
and refusing bad arguments before they touch a device, and the row table's feature column through every kind of row edit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import feature_loss_reference as flr
from conftest import ROOT, pkg

ENTRY_POINTS = {"gsplat_feature_ce_loss": 10, "gsplat_feature_l1_loss": 11, "gsplat_feature_cosine_loss": 11,
                "gsplat_feature_adam_step": 14}
INVALID_ARG = -3


def _case(seed, H=3, W=5, C=6):
    rng = np.random.default_rng(seed)
    fmap = rng.uniform(-3, 3, (H, W, C))
    target = rng.uniform(-3, 3, (H, W, C))
    labels = rng.integers(0, C, (H, W)).astype(np.int32)
    labels[0, 0], labels[1, 2], labels[2, 4] = -1, C, -7  # ignored, out of range, ignored
    valid = (rng.random((H, W)) > 0.3).astype(np.uint8)
    return fmap, target, labels, valid


@pytest.mark.parametrize("kind", ["ce", "l1", "cosine"])
def test_reference_against_central_differences(kind):
    """Steps of 1e-6 in float64: every gradient element within 1e-7 of its condition sum plus the O(h^2) term (the losses'
    third derivatives are O(scale) here); L1's elements are kept 1e-3 away from its kink."""
    fmap, target, labels, valid = _case(1)
    if kind == "l1":
        near = np.abs(fmap - target) < 1e-3
        fmap = np.where(near, target + 0.5, fmap)
    weight, h = 0.7, 1e-6

    def loss(x):
        return flr.ce_loss(x, labels, weight)[0] if kind == "ce" else flr.LOSSES[kind](x, target, valid, weight)[0]

    _, grad, grad_abs, loss_abs = flr.ce_loss(fmap, labels, weight) if kind == "ce" else flr.LOSSES[kind](fmap, target, valid, weight)
    assert (grad_abs >= np.abs(grad) * (1 - 1e-12)).all() and loss_abs >= abs(loss(fmap)) * (1 - 1e-12)
    scale = np.float32(weight) / (fmap.shape[0] * fmap.shape[1])
    worst = 0.0
    for idx in np.ndindex(fmap.shape):
        up, dn = fmap.copy(), fmap.copy()
        up[idx] += h
        dn[idx] -= h
        fd = (loss(up) - loss(dn)) / (2 * h)
        # eps / h of the loss's own magnitude, and h^2 x the third derivative
        bar = 1e-7 * max(grad_abs[idx], scale) + 4e-16 * loss_abs / h + 10 * scale * h * h
        worst = max(worst, abs(fd - grad[idx]) / bar)
        assert abs(fd - grad[idx]) <= bar, (kind, idx, fd, grad[idx])
    print(f"{kind}: worst finite-difference error {worst:.3f} of its bar")
    assert np.abs(grad).max() > 0


def test_ce_reference_at_large_logits_and_all_ignored():
    rng = np.random.default_rng(2)
    x = rng.uniform(-80, 80, (4, 7, 9))
    labels = rng.integers(0, 9, (4, 7)).astype(np.int32)
    loss, grad, grad_abs, loss_abs = flr.ce_loss(x, labels, 1.0)
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(loss_abs)
    assert np.abs(grad.sum(-1)).max() <= 1e-15  # softmax - onehot sums to 0 over the channels
    # the definition, evaluated without the maximum trick where that does not overflow float64 (|x| <= 80: e^80 ~ 5e34)
    direct = (np.log(np.exp(x).sum(-1)) - np.take_along_axis(x, labels[..., None].astype(np.int64), -1)[..., 0]).sum() / 28
    assert abs(loss - direct) <= 1e-13 * loss_abs
    # a spike of +80 against -80 everywhere else: the loss of that pixel is 0 for the spike's label and 160 for any other
    spike = np.full((1, 1, 5), -80.0)
    spike[0, 0, 3] = 80.0
    assert abs(flr.ce_loss(spike, np.array([[3]], np.int32), 1.0)[0]) <= 1e-60
    assert abs(flr.ce_loss(spike, np.array([[1]], np.int32), 1.0)[0] - 160.0) <= 1e-12
    ignored = np.full((4, 7), -1, np.int32)
    ignored[1, 1] = 9  # out of range counts as ignored too
    loss, grad, grad_abs, loss_abs = flr.ce_loss(x, ignored, 1.0)
    assert loss == 0.0 and loss_abs == 0.0 and (grad == 0).all() and (grad_abs == 0).all()


def test_l1_and_cosine_reference_edge_cases():
    fmap, target, _, valid = _case(3)
    same = flr.l1_loss(fmap, fmap, None, 2.0)
    assert same[0] == 0.0 and (same[1] == 0).all()  # sign(0) = 0
    loss, grad, _, _ = flr.l1_loss(fmap, target, valid, 2.0)
    assert (grad[valid == 0] == 0).all() and np.abs(grad[valid != 0]).min() > 0
    assert abs(loss - 2.0 * np.abs(fmap - target)[valid != 0].sum() / fmap.size) <= 1e-15
    f2, t2 = fmap.copy(), target.copy()
    f2[0, 1], t2[1, 3] = 0.0, 0.0  # a zero map row and a zero target row
    loss, grad, grad_abs, _ = flr.cosine_loss(f2, t2, None, 1.0)
    assert (grad[0, 1] == 0).all() and (grad[1, 3] == 0).all() and (grad_abs[0, 1] == 0).all()
    assert np.abs((grad * f2).sum(-1)).max() <= 1e-15  # the gradient is orthogonal to f: the loss ignores |f|
    aligned = flr.cosine_loss(fmap, 3.0 * fmap, None, 1.0)
    assert abs(aligned[0]) <= 1e-15 and np.abs(aligned[1]).max() <= 1e-15


def test_adam_reference_in_both_precisions():
    rng = np.random.default_rng(4)
    # (float32 values; gradient and first moment of one sign, so that no element is a difference of its two terms)
    p, g, m, v = (a.astype(np.float32) for a in (rng.standard_normal(50), rng.random(50) * 1e-3, rng.random(50) * 1e-4,
                                                 rng.random(50) * 1e-8))
    g[7] = np.nan
    args = (0.0025, 0.9, 0.999, 1e-8, 1 - 0.9 ** 4, 1 - 0.999 ** 4)
    a32, a64 = flr.adam_step(p, g, m, v, *args), flr.adam_step(p, g, m, v, *args, dtype=np.float64)
    assert all(a.dtype == np.float32 for a in a32) and all(a.dtype == np.float64 for a in a64)
    for x32, x64 in zip(a32, a64):
        np.testing.assert_allclose(x32, x64, rtol=2e-6, atol=1e-12)
    assert a32[1][7] == np.float32(0.9) * np.float32(m[7]) and np.isfinite(a32[0]).all()


def test_entry_points_are_declared_and_bound():
    lib_mod, ops, trainer_mod = pkg("_lib"), pkg("ops"), pkg("trainer")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    lib = lib_mod.load()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(lib_mod.SIGNATURES[name][1]) == nargs and callable(getattr(lib, name))
    assert lib_mod.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    for fn in ("feature_ce_loss", "feature_l1_loss", "feature_cosine_loss", "feature_adam_step"):
        assert callable(getattr(ops, fn))
    assert callable(trainer_mod.Trainer.evaluate_features) and isinstance(trainer_mod.Trainer.features, property)
    cfg = trainer_mod.DEFAULT_CONFIG
    assert (cfg["features"], cfg["feature_loss"], cfg["feature_weight"], cfg["feature_start"], cfg["feature_lr"],
            cfg["feature_geometry"]) == (0, "ce", 1.0, 0, 0.0025, False)
    makefile = open(os.path.join(ROOT, "3dgs_amd", "csrc", "Makefile")).read()
    assert "gs_featloss.hip" in makefile


def test_refusals_need_no_device():
    """Sizes, the channel count and null pointers are refused with GSPLAT_ERR_INVALID_ARG before any pointer is looked at
    (the non-null pointers here are host addresses that must never be dereferenced or asked about)."""
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    buf = (ctypes.c_float * 4)()
    x = ctypes.cast(buf, ctypes.c_void_p)
    ce = lambda *a: lib.gsplat_feature_ce_loss(*a)
    assert ce(None, x, 1, 1, 1, 1.0, 0, x, None, None) == INVALID_ARG      # map
    assert ce(x, None, 1, 1, 1, 1.0, 0, x, None, None) == INVALID_ARG      # labels
    assert ce(x, x, 1, 1, 1, 1.0, 0, None, None, None) == INVALID_ARG      # grad_map and loss_out both null
    for C in (0, 513, -1):
        assert ce(x, x, 1, 1, C, 1.0, 0, x, None, None) == INVALID_ARG
    for rows, cols in ((0, 1), (1, 0), (-3, 2)):
        assert ce(x, x, rows, cols, 1, 1.0, 0, x, None, None) == INVALID_ARG
    for fn in (lib.gsplat_feature_l1_loss, lib.gsplat_feature_cosine_loss):
        assert fn(None, x, None, 1, 1, 1, 1.0, 0, x, None, None) == INVALID_ARG   # map
        assert fn(x, None, None, 1, 1, 1, 1.0, 0, x, None, None) == INVALID_ARG   # target
        assert fn(x, x, None, 1, 1, 1, 1.0, 0, None, None, None) == INVALID_ARG   # both outputs null
        assert fn(x, x, None, 1, 1, 0, 1.0, 0, x, None, None) == INVALID_ARG
        assert fn(x, x, None, 1, 1, 513, 1.0, 0, x, None, None) == INVALID_ARG
        assert fn(x, x, None, 0, 1, 1, 1.0, 0, x, None, None) == INVALID_ARG
    adam = lambda n, C, *ptrs: lib.gsplat_feature_adam_step(ptrs[0], n, C, ptrs[1], ptrs[2], ptrs[3], ptrs[4], 1e-3, 0.9,
                                                            0.999, 1e-8, 0.1, 0.001, None)
    assert adam(1, 0, x, x, x, x, x) == INVALID_ARG and adam(1, 513, x, x, x, x, x) == INVALID_ARG
    assert adam(-1, 4, x, x, x, x, x) == INVALID_ARG
    for k in range(5):
        ptrs = [x] * 5
        ptrs[k] = None
        assert adam(1, 4, *ptrs) == INVALID_ARG
    assert adam(0, 4, None, None, None, None, None) == 0  # nothing visible: nothing to launch, nothing to check
    with pytest.raises(lib_mod.GsplatError):
        lib_mod.check(ce(None, x, 1, 1, 1, 1.0, 0, x, None, None))
    assert b"gsplat_feature_ce_loss" in lib.gsplat_last_error()


# ---------------------------------------------------------------- the row table's feature column
N, C = 11, 5


def _table(with_features, degree=1):
    rows = pkg("rows")
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    params = dict(xyz=r(N, 3), rgb=r(N, 3), sh=r(N, (degree + 1) ** 2 - 1, 3), opacity=r(N), scale=r(N, 3), quaternion=r(N, 4))
    names = [k for k in rows.GROUPS if k != "sh" or degree > 0]
    feats = (r(N, C), r(N, C), r(N, C)) if with_features else None
    return rows.RowTable(params, {k: r(*params[k].shape) for k in names}, {k: r(*params[k].shape) for k in names},
                         r(N), torch.arange(N, dtype=torch.int32), feats)


def _columns(t):
    cols = {"param." + k: v for k, v in t.params.items()}
    cols.update({"m." + k: v for k, v in t.exp_avg.items()})
    cols.update({"v." + k: v for k, v in t.exp_avg_sq.items()})
    cols.update(uv=t.uv_grad_accum, dur=t.grad_accum_dur)
    if t.features is not None:
        cols.update({"feat.%d" % i: v for i, v in enumerate(t.features)})
    return cols


def test_map_hands_the_feature_column_over_by_name():
    rows = pkg("rows")
    t = _table(True)
    t.check()
    seen = []
    t.map(lambda kind, name, c: seen.append((kind, name)) or c)
    assert seen[-3:] == [(rows.PARAM, "features"), (rows.MOMENT, "features"), (rows.MOMENT, "features")]
    assert (rows.PARAM, "features") not in seen[:-3] and rows.GROUPS == ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")


def test_row_edits_carry_the_feature_column_row_for_row():
    t = _table(True)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(6))
    keep = torch.tensor([1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1], dtype=torch.bool)
    src = torch.tensor([3, 3, 9])
    edits = {"permutation": (lambda kind, name, c: c[perm], perm),
             "keep mask": (lambda kind, name, c: c[keep], keep.nonzero().reshape(-1)),
             "concatenation": (lambda kind, name, c: torch.cat([c, c[src]], 0), torch.cat([torch.arange(N), src]))}
    for what, (fn, index) in edits.items():
        out = t.map(fn)
        out.check()
        assert out.features is not None and out.num_rows == len(index), what
        before, after = _columns(t), _columns(out)
        assert list(before) == list(after)
        for k in before:
            assert torch.equal(after[k], before[k][index]), (what, k)  # every column took the same rows, bit for bit
        assert after["feat.0"].shape == (len(index), C)


def test_fresh_and_the_five_argument_constructor_are_unchanged():
    rows = pkg("rows")
    t = _table(False)
    assert t.features is None
    t.check()
    seen = []
    out = t.map(lambda kind, name, c: seen.append((kind, name)) or c.clone())
    assert out.features is None and all(name != "features" for _, name in seen)
    assert len(seen) == 6 + 6 + 6 + 2
    for k, v in _columns(t).items():
        assert torch.equal(_columns(out)[k], v)
    fresh = rows.RowTable.fresh(t.params)
    assert fresh.features is None
    fresh.check()
    feats = torch.randn(N, C)
    withf = rows.RowTable.fresh(t.params, feats)
    withf.check()
    assert withf.features[0] is feats and all((m == 0).all() and m.shape == (N, C) for m in withf.features[1:])


@pytest.mark.parametrize("which", [0, 1, 2])
def test_check_rejects_a_bad_feature_column(which):
    def broken(fn):
        t = _table(True)
        f = list(t.features)
        f[which] = fn(f[which])
        t.features = tuple(f)
        return t

    _table(True).check()
    for fn in (lambda c: c[:N - 1].clone(),                    # a row short
               lambda c: c.double(),                             # wrong dtype
               lambda c: torch.randn(C, N).t()):                 # [N,C] but not contiguous
        with pytest.raises(ValueError):
            broken(fn).check()
    if which == 0:
        with pytest.raises(ValueError):
            broken(lambda c: c.reshape(-1)).check()              # not [N,C]
    else:
        with pytest.raises(ValueError):
            broken(lambda c: c[:, :C - 1].clone()).check()       # moments shaped unlike the column

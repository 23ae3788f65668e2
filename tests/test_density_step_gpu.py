"""Classic adaptive density control on the GPU, row by row: gsplat_density_masks against the reference's functors (exact:
on the thresholds themselves and on random rows that keep a stated distance from them), clone / split at the block
edges, what Trainer.adaptive_density_step leaves behind (layout, moments, accumulators, flags, capacity), the Morton
re-order of everything that travels with a gaussian, and the cadence of Trainer.maintenance.  The model of all of it is
tests/density_reference.py; nothing here is toleranced except the split children's xyz / scale, which take the bound of
tests/test_density_gpu.py (a float32 draw through device logf / cosf against the host's)."""
import math

import numpy as np
import pytest

import density_reference as ref
from conftest import pkg

pytestmark = pytest.mark.gpu

SPLIT_TOL = dict(rtol=2e-5, atol=2e-6)  # tests/test_density_gpu.py::test_clone_and_split_match_oracle
F = np.float32
OP_T, G_T = F(math.log(0.02) - math.log(0.98)), F(2e-4)
W = H = 32
SEED, ITER = 3, 37  # the split seed of the step is SEED * 1000003 + ITER: not the trivial one


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_mask_invariants(prune, clone, split, keep):
    assert not (prune & clone).any() and not (prune & split).any() and not (clone & split).any()
    assert np.array_equal(keep, ~(prune | split))


# ---------------------------------------------------------------------------------------------------- masks
def _device_masks(torch, opacity, scale, accum, dur, thr):
    ops = pkg("ops")
    got = ops.density_masks(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (opacity, scale, accum, dur)],
                            *[float(t) for t in thr])
    return [_np(g).astype(bool) for g in got[:4]], got[4]


def test_masks_on_the_thresholds(gpu):
    """Every row's largest log-scale is exactly 0.0f, so its largest extent is exactly 1 (expf(0) is 1 in any
    implementation) and each call puts one comparison on equality; the functors' side of it is written out, and every
    mask of every call equals the model.  No flips."""
    torch = gpu
    nan, inf = float("nan"), float("inf")
    hot, cold = (1.0, 1), (0.0, 1)  # (accum, dur): average 1 and 0
    rows = [  # opacity, log-extents, (accum, dur)
        (0.0, (0, -1, -2), hot),                                # 0 a gradient
        (0.0, (-1, 0, -2), cold),                               # 1 none
        (OP_T, (0, -1, -1), hot),                               # 2 opacity on its threshold: not pruned
        (np.nextafter(OP_T, F(-inf)), (0, -1, -1), hot),        # 3 one step below: pruned
        (0.0, (-2, -1, 0), (G_T * F(8), 8)),                    # 4 average == threshold (power-of-two division): not densified
        (0.0, (-2, -1, 0), (np.nextafter(G_T * F(8), F(inf)), 8)),  # 5 one step above
        (0.0, (nan, 0, -1), hot),                               # 6 NaN extent: ignored by fmaxf
        (0.0, (inf, 0, 0), hot),                                # 7 infinite extent
        (0.0, (-inf, 0, -1), hot),                              # 8 zero extent next to 1
        (0.0, (0, -1, -2), (100.0, 0)),                         # 9 never seen: average 0
        (nan, (0, 0, 0), hot),                                  # 10 NaN opacity: not pruned by opacity
        (0.0, (nan, nan, nan), hot),                            # 11 nothing to compare
    ]
    opacity = F([r[0] for r in rows])
    scale = F([r[1] for r in rows])
    accum, dur = F([r[2][0] for r in rows]), np.int32([r[2][1] for r in rows])
    assert (G_T * F(8)) / F(8) == G_T and np.nextafter(G_T * F(8), F(inf)) / F(8) > G_T
    below_one, ratio = np.nextafter(F(1), F(0)), F(1) / F(1.6)
    P, C, S = 0, 1, 2
    calls = [  # (max_scale, clone_scale_threshold), [(row, mask, the value the functors give)]
        ((F(2), F(1)), [(0, C, 1), (2, C, 1), (3, P, 1), (4, C, 0), (5, C, 1), (6, C, 1), (7, P, 1), (8, C, 1), (9, C, 0),
                        (10, C, 1), (10, P, 0), (11, C, 0), (11, P, 0)]),          # extent == clone threshold: clone ..
        ((F(2), below_one), [(0, S, 1), (5, S, 1), (4, S, 0)]),                   # .. one step down: split
        ((F(1), F(0.5)), [(0, P, 0), (0, S, 1), (1, P, 0)]),    # extent == max_scale: not pruned, gradient or not
        ((below_one, F(0.5)), [(0, S, 1), (1, P, 1)]),          # one step down: pruned unless about to densify
        ((ratio, F(0.5)), [(0, P, 0), (0, S, 1), (1, P, 1), (4, P, 1), (9, P, 1), (10, S, 1)]),  # extent / 1.6 == max_scale
        ((np.nextafter(ratio, F(0)), F(0.5)), [(0, P, 1), (5, P, 1)]),                           # one step down: not exempt
    ]
    for (max_scale, c_t), sides in calls:
        thr = (OP_T, max_scale, G_T, c_t)
        want = ref.masks(opacity, scale, accum, dur, *thr)
        got, counts = _device_masks(torch, opacity, scale, accum, dur, thr)
        for name, g, w in zip(("prune", "clone", "split", "keep"), got, want[:4]):
            assert np.array_equal(g, w), (name, float(max_scale), float(c_t), g.astype(int), w.astype(int))
        assert counts == [int(m.sum()) for m in got[:3]]
        _assert_mask_invariants(*got)
        for row, mask, value in sides:
            assert bool(got[mask][row]) == bool(value), (row, mask, value, float(max_scale), float(c_t))
    # the first call once more, spelled out: on equality clone and not split, NaN opacity survives, NaN extents do nothing
    got, _ = _device_masks(torch, opacity, scale, accum, dur, (OP_T, F(2), G_T, F(1)))
    assert got[1].astype(int).tolist() == [1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0] and not got[2].any()
    assert got[0].astype(int).tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0]


def _random_rows(n, seed, thr):
    """The distribution of tests/test_trainer_gpu.py::test_density_masks_match_the_reference_functors; a row closer than
    ref.MARGIN (relative) to any threshold is drawn again until none is (a last-bit expf difference is 1e-7)."""
    rng = np.random.default_rng(seed)

    def draw(k):
        return (rng.normal(-2, 2, k).astype(F), rng.normal(-3, 1.5, (k, 3)).astype(F), (rng.random(k) * 0.01).astype(F),
                rng.integers(0, 12, k).astype(np.int32))

    cols = list(draw(n))
    redrawn = 0
    while True:
        close = ref.masks(*cols, *thr)[4] < ref.MARGIN
        if not close.any():
            return cols, redrawn
        redrawn += int(close.sum())
        for c, new in zip(cols, draw(int(close.sum()))):
            c[close] = new


RANDOM_THR = (OP_T, F(0.4), G_T, F(0.04))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_masks_on_random_rows_are_exact(gpu, n):
    """Through the C ABI, into outputs with 64 guard bytes behind them: all four masks equal the model bit for bit, the
    counts are the masks' own sums, nothing is written past row N (partial last wave, partial last block), and a second
    call into the same counts gives the same counts (the launcher zeroes them)."""
    torch, lib = gpu, pkg("_lib").load()
    (opacity, scale, accum, dur), redrawn = _random_rows(n, 100 + n, RANDOM_THR)
    want = ref.masks(opacity, scale, accum, dur, *RANDOM_THR)
    assert (want[4] >= ref.MARGIN).all() and redrawn <= max(2, n // 100)  # every row has the margin; few were redrawn
    if n >= 255:
        assert all(m.any() for m in want[:4])
    d = [torch.from_numpy(a).cuda() for a in (opacity, scale, accum, dur)]
    out = [torch.full((n + 64,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(4)]
    counts = torch.full((12 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    results = []
    for _ in range(2):
        assert lib.gsplat_density_masks(n, *[t.data_ptr() for t in d], *[float(t) for t in RANDOM_THR],
                                        *[t.data_ptr() for t in out], counts.data_ptr(), None) == 0
        torch.cuda.synchronize()
        results.append(([_np(t) for t in out], _np(counts)))
    (masks, cnt), (masks2, cnt2) = results
    for name, g, w in zip(("prune", "clone", "split", "keep"), masks, want[:4]):
        assert (g[n:] == 0xAB).all(), name + ": guard bytes"
        assert set(np.unique(g[:n]).tolist()) <= {0, 1}, name
        assert np.array_equal(g[:n].astype(bool), w), (name, np.nonzero(g[:n].astype(bool) != w)[0][:10])
    assert (cnt[12:] == 0xAB).all(), "counts: guard bytes"
    assert cnt[:12].view(np.int32).tolist() == [int(m[:n].sum()) for m in masks[:3]] == [int(w.sum()) for w in want[:3]]
    _assert_mask_invariants(*[m[:n].astype(bool) for m in masks])
    assert all(_same_bits(a, b) for a, b in zip(masks, masks2)) and _same_bits(cnt, cnt2)


# ---------------------------------------------------------------------------------------------------- clone / split
ATTRS = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")


def _cloud(n, nsh, seed):
    rng = np.random.default_rng(seed)
    return dict(xyz=rng.normal(size=(n, 3)).astype(F) * 3, rgb=rng.normal(size=(n, 3)).astype(F),
                opacity=rng.normal(size=n).astype(F), scale=(rng.normal(size=(n, 3)) - 2).astype(F),
                quaternion=rng.normal(size=(n, 4)).astype(F), sh=rng.normal(size=(n, nsh * 3)).astype(F))


@pytest.mark.parametrize("nsh", [0, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_clone_and_split_at_the_block_edges(gpu, orc, n, nsh):
    """No row, every row, and only the last row selected, at sizes around one 256-thread block: copies bit for bit, the
    split draw within the project's bound, and three NaN-filled rows behind the destination that nothing may touch."""
    torch, ops = gpu, pkg("ops")
    g = _cloud(n, nsh, seed=n + nsh)
    src = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    last = np.zeros(n, np.uint8)
    last[-1] = 1
    for mask in (np.zeros(n, np.uint8), np.ones(n, np.uint8), last):
        wid = (np.cumsum(mask) - mask).astype(np.int32)
        d_mask, d_wid = torch.from_numpy(mask).cuda(), torch.from_numpy(wid).cuda()
        for split in (False, True):
            rows = int(mask.sum()) * (2 if split else 1)
            dst = {k: torch.full((rows + 3,) + tuple(v.shape[1:]), float("nan"), device="cuda") for k, v in src.items()}
            fill = {k: _np(v).copy() for k, v in dst.items()}
            if split:
                ops.split_gaussians(n, 1.6, nsh, d_mask, d_wid, src, dst, seed=42)
            else:
                ops.clone_gaussians(n, nsh, d_mask, d_wid, src, dst)
            torch.cuda.synchronize()
            want = orc.clone_split(g, mask, nsh, split=split, scale_factor=1.6, seed=42)
            for k in ATTRS:
                got = _np(dst[k])
                assert _same_bits(got[rows:], fill[k][rows:]), (k, "rows behind the last written one")
                new = got[:rows].reshape(want[k].shape)
                if split and k in ("xyz", "scale"):
                    np.testing.assert_allclose(new, want[k], err_msg=k, **SPLIT_TOL)
                else:
                    assert _same_bits(new, want[k]), k


# ---------------------------------------------------------------------------------------------------- the step
CLASSES = ("keep", "low", "big", "exempt", "clone", "split", "unseen")


def _rows_of_classes(classes, seed):
    """(opacity, scale, accum, dur) with row i of class classes[i], at the thresholds of scene_extent 1 (largest extent
    0.1, clone / split boundary 0.01, average gradient 2e-4, opacity logit(0.02)), every quantity well off them."""
    rng = np.random.default_rng(seed)
    n = len(classes)
    opacity, scale = np.empty(n, F), np.empty((n, 3), F)
    accum, dur = np.empty(n, F), np.empty(n, np.int32)
    extent = dict(keep=(0.012, 0.09), low=(0.002, 0.09), exempt=(0.105, 0.155), clone=(0.002, 0.0095),
                  split=(0.0105, 0.095), unseen=(0.002, 0.09))
    for i, c in enumerate(classes):
        hot = c in ("exempt", "clone", "split") or (c in ("low", "big") and i % 2 == 0)
        lo, hi = extent[c] if c != "big" else ((0.17, 0.5) if hot else (0.12, 0.5))
        e = rng.uniform(lo, hi) * np.append(1.0, rng.uniform(0.3, 0.95, 2))
        scale[i] = np.log(np.roll(e, i % 3))
        opacity[i] = rng.uniform(-8.0, -4.5) if c == "low" else rng.uniform(-2.0, 3.0)
        dur[i] = 0 if c == "unseen" else (1, 2, 4, 8, 3, 5)[i % 6]
        accum[i] = 5.0 if c == "unseen" else (rng.uniform(3e-4, 5e-3) if hot else rng.uniform(0.0, 1.5e-4)) * dur[i]
    return opacity, scale, accum, dur


@pytest.fixture(scope="module")
def views(gpu, scene):
    """One 32x32 view, built as _synthetic_views of tests/test_trainer_gpu.py builds its views."""
    raster = pkg("raster")
    truth = scene.make_gaussians(200, W, H, 0)
    truth["opacity"][:] = np.clip(truth["opacity"], 0.5, 3.0)
    cam = raster.device_camera(scene.make_camera(W, H, 0))
    image = raster.RasterContext(200, W, H).rasterize_image(raster.device_params(truth), cam, scene.CONFIG, 0.0, 0)["image"]
    return [(cam, image.clone())]


def _trainer(torch, scene, views, classes, l_max, config=None, seed=11):
    """A Trainer whose rows are of the given classes, every moment tagged with its row (exp_avg: row + 0.25, exp_avg_sq:
    row + 0.5), the accumulators loaded, t.iter set; and the same state as numpy arrays."""
    raster, trainer_mod = pkg("raster"), pkg("trainer")
    n = len(classes)
    p = scene.make_gaussians(n, W, H, l_max, seed=seed)
    p["opacity"], p["scale"], accum, dur = _rows_of_classes(classes, seed)
    p = {k: np.ascontiguousarray(v, F) for k, v in p.items()}
    dp = raster.device_params(p)
    if l_max == 0:
        dp.pop("sh")
    t = trainer_mod.Trainer(dp, views, dict(use_background=False, **(config or {})), scene_extent=1.0, seed=SEED)
    assert t.l_max == l_max and t.num_gaussians == n
    t.opt.uv_grad_accum.copy_(torch.from_numpy(accum))
    t.opt.grad_accum_dur.copy_(torch.from_numpy(dur))
    _tag_moments(torch, t)
    t.iter = ITER
    return t, dict(params=p, accum=accum, dur=dur)


def _tag_moments(torch, t):
    rows = torch.arange(t.num_gaussians, dtype=torch.float32, device="cuda")
    for g in t.opt.names:
        shape = (-1,) + (1,) * (t.opt.exp_avg[g].dim() - 1)
        t.opt.exp_avg[g].copy_((rows + 0.25).reshape(shape).expand_as(t.opt.exp_avg[g]))
        t.opt.exp_avg_sq[g].copy_((rows + 0.5).reshape(shape).expand_as(t.opt.exp_avg_sq[g]))


def _snapshot(t):
    s = {"param/" + g: _np(v).copy() for g, v in t.params.items()}
    s.update({"m/" + g: _np(t.opt.exp_avg[g]).copy() for g in t.opt.names})
    s.update({"v/" + g: _np(t.opt.exp_avg_sq[g]).copy() for g in t.opt.names})
    s["uv_grad_accum"], s["grad_accum_dur"] = _np(t.opt.uv_grad_accum).copy(), _np(t.opt.grad_accum_dur).copy()
    return s


def _assert_unchanged(t, before):
    after = _snapshot(t)
    assert after.keys() == before.keys()
    for k in before:
        assert _same_bits(after[k], before[k]), k


def _expected(orc, t, host, flags=(1, 1, 1), max_gaussians=None):
    """density_reference.step of the Trainer's state as loaded (None: skipped or nothing to do) and the model's masks."""
    p, n = host["params"], t.num_gaussians
    nsh = (t.l_max + 1) ** 2 - 1 if t.l_max > 0 else 0
    thr = (F(pkg("trainer")._logit(0.02)), F(0.1), G_T, F(0.01))
    assert thr[0] == OP_T
    mk = ref.masks(p["opacity"], p["scale"], host["accum"], host["dur"], *thr)
    assert (mk[4] >= ref.MARGIN).all(), "a row of the constructed state sits on a threshold"
    split = ref.apply_flags(mk, flags)[2]
    children = None
    if split.any():
        children = orc.clone_split(dict(p, sh=p["sh"].reshape(n, -1)), split.astype(np.uint8), nsh, split=True,
                                   scale_factor=1.6, seed=SEED * 1000003 + ITER)
    tag = np.arange(n, dtype=F)
    m = {g: np.broadcast_to((tag + F(0.25)).reshape((n,) + (1,) * (p[g].ndim - 1)), p[g].shape) for g in t.opt.names}
    v = {g: a + F(0.25) for g, a in m.items()}
    cap = t.cfg["max_gaussians"] if max_gaussians is None else max_gaussians
    return ref.step(p, m, v, mk, [int(a.sum()) for a in mk[:3]], flags, cap, nsh, children), mk


def _assert_step(torch, t, want, result):
    """Everything the step leaves behind against the model: bitwise, except the split children's xyz / scale."""
    n, nsh = want["n"], (t.l_max + 1) ** 2 - 1 if t.l_max > 0 else 0
    assert result == want["result"]
    assert t.num_gaussians == n
    children = n - 2 * want["result"]["split"]
    shapes = dict(xyz=(n, 3), rgb=(n, 3), sh=(n, nsh, 3), opacity=(n,), scale=(n, 3), quaternion=(n, 4))
    for g in ref.GROUPS:
        got = t.params[g]
        assert tuple(got.shape) == shapes[g] and got.is_contiguous() and got.dtype == torch.float32, g
        got, w = _np(got), want["params"][g]
        assert _same_bits(got[:children], w[:children]), g + ": kept rows and clones"
        if g in ("xyz", "scale"):
            np.testing.assert_allclose(got[children:], w[children:], err_msg=g + ": split children", **SPLIT_TOL)
        else:
            assert _same_bits(got[children:], w[children:]), g + ": split children"
    assert list(t.opt.names) == [g for g in ref.GROUPS if g in want["m"]]
    for g in t.opt.names:
        for name, got, w in (("exp_avg", t.opt.exp_avg[g], want["m"][g]), ("exp_avg_sq", t.opt.exp_avg_sq[g], want["v"][g])):
            assert tuple(got.shape) == shapes[g] and got.is_contiguous(), (g, name)
            assert _same_bits(_np(got), w), (g, name)
    assert _same_bits(_np(t.opt.uv_grad_accum), want["uv_grad_accum"])
    assert _same_bits(_np(t.opt.grad_accum_dur), want["grad_accum_dur"])


INTERLEAVED = [CLASSES[i % 7] for i in range(777)]


@pytest.mark.parametrize("l_max", [0, 1, 3])
def test_step_layout_moments_and_accumulators(gpu, scene, orc, views, l_max):
    torch = gpu
    t, host = _trainer(torch, scene, views, INTERLEAVED, l_max)
    want, mk = _expected(orc, t, host)
    assert [int(a.sum()) for a in mk[:3]] == [222, 111, 222]  # low + big | clone | exempt + split
    result = t.adaptive_density_step()
    torch.cuda.synchronize()
    assert want["n"] == 777 - 222 - 222 + 111 + 444
    _assert_step(torch, t, want, result)


@pytest.mark.parametrize("flags", [(d, c, s) for d in (1, 0) for c in (1, 0) for s in (1, 0)])
def test_step_under_the_config_flags(gpu, scene, orc, views, flags):
    """use_delete / use_clone / use_split, each off: the pruned rows stay and are neither cloned nor split, the would-be
    clones stay once, the would-be splits stay as kept rows; all off, the step has nothing to do."""
    torch = gpu
    cfg = dict(use_delete=bool(flags[0]), use_clone=bool(flags[1]), use_split=bool(flags[2]))
    t, host = _trainer(torch, scene, views, INTERLEAVED, 1, cfg)
    want, _ = _expected(orc, t, host, flags)
    before = _snapshot(t)
    result = t.adaptive_density_step()
    torch.cuda.synchronize()
    if flags == (0, 0, 0):
        assert want is None and result == dict(pruned=0, cloned=0, split=0, skipped=False)
        _assert_unchanged(t, before)
        return
    assert want["n"] == 777 - (222 if flags[0] else 0) + (111 if flags[1] else 0) + (222 if flags[2] else 0)
    _assert_step(torch, t, want, result)


def test_step_capacity_and_nothing_to_do(gpu, scene, orc, views):
    torch = gpu
    # exactly the room the step needs: it proceeds
    t, host = _trainer(torch, scene, views, INTERLEAVED, 1, dict(max_gaussians=888))
    want, _ = _expected(orc, t, host)
    assert want["n"] == 888
    _assert_step(torch, t, want, t.adaptive_density_step())
    # one row short: skipped, and not a bit of the state changes
    t, host = _trainer(torch, scene, views, INTERLEAVED, 1, dict(max_gaussians=887))
    assert _expected(orc, t, host)[0] is None
    before = _snapshot(t)
    assert t.adaptive_density_step() == dict(pruned=0, cloned=0, split=0, skipped=True)
    torch.cuda.synchronize()
    _assert_unchanged(t, before)
    # nothing to prune or add: all zeros, not skipped, unchanged
    t, host = _trainer(torch, scene, views, ["keep", "unseen", "keep"] * 100, 1)
    assert _expected(orc, t, host)[0] is None
    before = _snapshot(t)
    assert t.adaptive_density_step() == dict(pruned=0, cloned=0, split=0, skipped=False)
    torch.cuda.synchronize()
    _assert_unchanged(t, before)


def test_step_down_to_one_gaussian_then_trains(gpu, scene, orc, views):
    torch = gpu
    classes = ["low" if i % 2 else "big" for i in range(300)]
    classes[123] = "keep"
    t, host = _trainer(torch, scene, views, classes, 1)
    want, _ = _expected(orc, t, host)
    assert want["n"] == 1 and want["result"] == dict(pruned=299, cloned=0, split=0, skipped=False)
    _assert_step(torch, t, want, t.adaptive_density_step())
    t.params["xyz"].copy_(torch.tensor([[0.0, 0.0, 4.0]]))  # in front of the camera, whatever row 123 drew
    t.params["scale"].fill_(math.log(0.3))
    loss = t.train_step(*views[0])
    assert loss is not None and math.isfinite(loss)


def test_context_after_growth(gpu, scene, orc, views):
    """A step that grows past the workspace the Trainer was built with: the next iteration trains, and evaluate() gives
    the bits a Trainer freshly built on the grown parameters gives (no stale workspace state)."""
    torch, trainer_mod = gpu, pkg("trainer")
    t, host = _trainer(torch, scene, views, ["clone", "split", "keep", "exempt"] * 150, 1)
    assert t.ctx_capacity == 600
    want, _ = _expected(orc, t, host)
    _assert_step(torch, t, want, t.adaptive_density_step())
    assert t.num_gaussians == 600 + 150 + 300 > t.ctx_capacity
    loss = t.train_step(*views[0])
    assert loss is not None and math.isfinite(loss)
    assert t.ctx_capacity >= t.num_gaussians
    psnr = t.evaluate()
    fresh = trainer_mod.Trainer({k: v.clone() for k, v in t.params.items()}, views, dict(use_background=False),
                                scene_extent=1.0, seed=SEED)
    assert fresh.ctx_capacity == t.num_gaussians and fresh.l_max == t.l_max
    assert math.isfinite(psnr) and psnr == fresh.evaluate()
    assert psnr == t.evaluate()


# ---------------------------------------------------------------------------------------------------- Morton re-order
SPECIAL_COUNTS = np.array([1, 0x7F800001, 0x7FC00001, 0xFFFFFFFF, 3, 12, 0, 7], np.uint32).view(np.int32)  # (0xFFFFFFFF: -1)
# read as float32: a denormal, a signalling NaN, a quiet NaN with a payload, another NaN; and ordinary counts


def _assert_sorted_by(torch, t, before, order):
    after = _snapshot(t)
    assert after.keys() == before.keys()
    for k in before:
        assert _same_bits(after[k], before[k][order]), k


def _load_accumulators(torch, t):
    n = t.num_gaussians
    t.opt.uv_grad_accum.copy_(torch.arange(n, dtype=torch.float32, device="cuda") * 0.5 + 0.125)
    t.opt.grad_accum_dur.copy_(torch.from_numpy(np.resize(SPECIAL_COUNTS, n)))


def test_sort_after_a_step_moves_everything_by_the_stable_morton_order(gpu, scene, orc, views):
    torch = gpu
    t, host = _trainer(torch, scene, views, INTERLEAVED, 1)
    t.adaptive_density_step()
    _tag_moments(torch, t)  # (the new rows' moments are zero: tag all rows again, so that every row is told apart)
    _load_accumulators(torch, t)
    before = _snapshot(t)
    xyz = before["param/xyz"]
    order = ref.morton_order(xyz)
    codes = orc.compute_morton_codes(xyz, xyz.max(0), xyz.min(0))
    assert len(np.unique(codes)) <= len(codes) - 111, "every clone shares its source's code"
    assert not np.array_equal(order, np.arange(len(order)))
    assert "param/sh" in before and before["param/sh"].shape[1:] == (3, 3) and "m/sh" in before
    t.sort_gaussians()
    torch.cuda.synchronize()
    _assert_sorted_by(torch, t, before, order)
    assert t.params["sh"].shape == before["param/sh"].shape and t.params["opacity"].dim() == 1
    assert t.opt.grad_accum_dur.dtype == torch.int32


@pytest.mark.parametrize("case", ["one", "plane", "point", "point32", "clones24"])
def test_sort_on_degenerate_boxes_and_small_clouds(gpu, scene, orc, views, case):
    """A box with no extent along an axis makes that axis' scale factor infinite and its quantised coordinate 0 * inf:
    the reference's conversion gives 0.  One gaussian; all z equal; all points identical (the order is the identity), at
    300 rows and at 32, where a key sort that is not asked to be stable may run as a bitonic network, which is not;
    and 12 gaussians followed by their 12 clones, each of which has to land directly behind its source."""
    torch = gpu
    n = dict(one=1, plane=300, point=300, point32=32, clones24=24)[case]
    t, host = _trainer(torch, scene, views, ["keep"] * n, 0)
    if case == "plane":
        t.params["xyz"][:, 2] = 4.0
    elif case in ("point", "point32"):
        t.params["xyz"].copy_(torch.tensor([[0.25, -0.5, 4.0]]).expand(n, 3))
    elif case == "clones24":
        t.params["xyz"][12:] = t.params["xyz"][:12]
    _load_accumulators(torch, t)
    before = _snapshot(t)
    order = ref.morton_order(before["param/xyz"])
    if case == "plane":
        assert not np.array_equal(order, np.arange(n))
    elif case == "clones24":
        where = np.argsort(order)
        assert (where[12:] == where[:12] + 1).all() and not np.array_equal(order, np.arange(n))
    else:
        assert order.tolist() == list(range(n))
    t.sort_gaussians()
    torch.cuda.synchronize()
    _assert_sorted_by(torch, t, before, order)


# ---------------------------------------------------------------------------------------------------- cadence
DENSITY, RESET = ["adaptive_density_step", "sort_gaussians", "reset_grad_accum"], ["reset_opacity", "reset_grad_accum"]
CADENCE = dict(adaptive_control_start=500, adaptive_control_interval=100, adaptive_control_end=2000,
               reset_opacity_start=600, reset_opacity_interval=300, reset_opacity_end=1800)
CADENCE_TABLE = [  # iteration, density control, opacity reset  (cuda/trainer.cu:1392-1404: > start, % interval == 0, < end)
    (0, False, False), (100, False, False), (499, False, False),
    (500, False, False),    # equal to adaptive_control_start: not yet
    (501, False, False), (550, False, False),
    (600, True, False),     # the next multiple fires; equal to reset_opacity_start: no reset yet
    (601, False, False), (700, True, False),
    (900, True, True),      # the first multiple of 300 past 600: both
    (1500, True, True), (1799, False, False),
    (1800, True, False),    # equal to reset_opacity_end: no reset
    (1900, True, False),
    (2000, False, False),   # equal to adaptive_control_end: nothing
    (2100, False, False), (2400, False, False),
]


def test_maintenance_cadence(gpu, scene, views, monkeypatch):
    torch, trainer_mod = gpu, pkg("trainer")
    t, _ = _trainer(torch, scene, views, ["keep"] * 10, 0, CADENCE)
    calls = []
    for name in set(DENSITY + RESET):
        monkeypatch.setattr(trainer_mod.Trainer, name, lambda self, _name=name: calls.append(_name))
    c = CADENCE
    for it, density, reset in CADENCE_TABLE:
        assert density == (it > c["adaptive_control_start"] and it % c["adaptive_control_interval"] == 0
                           and it < c["adaptive_control_end"]), it
        assert reset == (it > c["reset_opacity_start"] and it % c["reset_opacity_interval"] == 0
                         and it < c["reset_opacity_end"]), it
        del calls[:]
        t.iter = it + 1  # maintenance() follows the train_step of iteration `it`, which has advanced the counter
        t.maintenance()
        assert calls == (DENSITY if density else []) + (RESET if reset else []), (it, calls)
    assert t.mcmc_steps == [] and t.contribution_prunes == []

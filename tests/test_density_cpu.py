"""Oracle pins for the f4 operators: compute_morton_codes (tests/cuda_forward_test.cpp:918-1020) and clone / split
(tests/adaptive_density_test.cpp:187-297)."""
import numpy as np

MAXC = (1 << 21) - 1


def _ref_spread(n):  # the expectation the reference's own test builds (cuda_forward_test.cpp:964-972)
    n &= MAXC
    n = (n | (n << 32)) & 0x1F000000FFFF
    n = (n | (n << 16)) & 0x1F0000FF0000FF
    n = (n | (n << 8)) & 0x100F807C0F807C0F
    n = (n | (n << 4)) & 0x1084210842108421
    n = (n | (n << 2)) & 0x1249249249249249
    return n


def test_morton_codes_reference_case(orc):
    lo, hi = np.float32([-10, -5, 0]), np.float32([10, 5, 20])
    pts = np.float32([[-10, -5, 0], [10, 5, 20], [0, 0, 10], [5, 2, 5], [-5, -2, 15]])
    want = []
    for p in pts:
        norm = np.clip((p - lo) / (hi - lo), np.float32(0), np.float32(1)).astype(np.float32)
        q = [int(np.float32(v) * np.float32(MAXC)) for v in norm]
        want.append((_ref_spread(q[2]) << 2) | (_ref_spread(q[1]) << 1) | _ref_spread(q[0]))
    got = orc.compute_morton_codes(pts, hi, lo)
    assert [int(c) for c in got] == want
    assert got[0] == 0


def test_clone_and_split_reference_cases(orc):
    g = dict(xyz=np.float32([[1, 2, 3], [4, 5, 6]]), rgb=np.float32([[.1, .2, .3], [.4, .5, .6]]),
             opacity=np.float32([0.8, 0.7]), scale=np.log(np.float32([[2, 2, 2], [.1, .1, .1]])),
             quaternion=np.float32([[1, 0, 0, 0], [1, 0, 0, 0]]), sh=np.zeros((2, 0), np.float32))
    c = orc.clone_split(g, [1, 0], 0)
    assert c["xyz"].tolist() == [[1, 2, 3]] and c["opacity"].tolist() == [np.float32(0.8)]
    s = orc.clone_split(g, [1, 0], 0, split=True, scale_factor=1.6, seed=3)
    np.testing.assert_allclose(s["scale"], np.log(np.float32(2.0) / np.float32(1.6)), atol=1e-6)
    assert s["opacity"].tolist() == [np.float32(0.8)] * 2 and s["xyz"].shape == (2, 3)
    assert not np.allclose(s["xyz"][0], s["xyz"][1])  # two different draws
    assert (orc.clone_split(g, [1, 0], 0, split=True, scale_factor=1.6, seed=3)["xyz"] == s["xyz"]).all()  # reproducible


def test_split_positions_follow_the_gaussian(orc):
    """Many splits of one anisotropic, rotated gaussian: sample mean -> xyz, covariance -> R diag(exp(s))^2 R^T."""
    n = 20000
    q = np.float32([0.9, 0.1, -0.3, 0.2])
    g = dict(xyz=np.tile(np.float32([1, -2, 0.5]), (n, 1)), rgb=np.zeros((n, 3), np.float32), opacity=np.zeros(n, np.float32),
             scale=np.tile(np.log(np.float32([0.5, 0.1, 0.02])), (n, 1)), quaternion=np.tile(q, (n, 1)),
             sh=np.arange(n * 9, dtype=np.float32).reshape(n, 9))
    s = orc.clone_split(g, np.ones(n, np.uint8), 3, split=True, scale_factor=1.6, seed=11)
    assert s["xyz"].shape == (2 * n, 3) and (s["sh"][0::2] == g["sh"]).all() and (s["sh"][1::2] == g["sh"]).all()
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    cov = R @ np.diag([0.25, 0.01, 0.0004]) @ R.T
    d = s["xyz"].astype(np.float64) - [1, -2, 0.5]
    assert np.abs(d.mean(0)).max() < 0.01
    np.testing.assert_allclose(d.T @ d / len(d), cov, atol=0.004)


# ------------------------------------------------------------------ the model of classic density control itself
# (tests/density_reference.py: what tests/test_density_step_gpu.py holds the kernels and the Trainer to)
def _table():
    """Ten rows, one per class, at the thresholds of scene_extent 1: opacity logit(0.02) = -3.89, largest extent 0.1
    (0.16 for a row about to be densified), average gradient 2e-4, clone / split boundary 0.01."""
    import math
    nan, inf = float("nan"), float("inf")
    ln = math.log
    rows = [  # opacity, the three extents' logs,           accum, dur
        (0.0, (ln(.05), ln(.04), ln(.03)), 0.0, 4),       # 0 kept: no gradient, moderate size
        (-5.0, (ln(.005), ln(.004), ln(.003)), 0.01, 2),  # 1 low opacity: goes, whatever its gradient
        (0.0, (ln(.5), ln(.04), ln(.03)), 0.0, 4),        # 2 oversized, no gradient: goes
        (0.0, (ln(.15), ln(.04), ln(.03)), 0.004, 4),     # 3 oversized, but 0.15 / 1.6 <= 0.1 and it will split: stays
        (0.0, (ln(.005), ln(.004), ln(.003)), 0.004, 4),  # 4 clone: gradient, small
        (0.0, (ln(.05), ln(.04), ln(.03)), 0.004, 4),     # 5 split: gradient, large
        (0.0, (ln(.005), ln(.004), ln(.003)), 100.0, 0),  # 6 never seen: the average is 0 whatever was accumulated
        (0.0, (nan, ln(.005), ln(.003)), 0.004, 4),       # 7 a NaN extent is ignored by fmaxf: 0.005, clone
        (0.0, (inf, ln(.04), ln(.03)), 0.004, 4),         # 8 +inf: infinite extent, goes even with a gradient
        (0.0, (-inf, ln(.05), ln(.02)), 0.004, 4),        # 9 -inf: that extent is 0, the largest is 0.05, split
    ]
    opacity = np.float32([r[0] for r in rows])
    scale = np.float32([r[1] for r in rows])
    accum, dur = np.float32([r[2] for r in rows]), np.int32([r[3] for r in rows])
    thresholds = (np.float32(ln(0.02) - ln(0.98)), np.float32(0.1), np.float32(2e-4), np.float32(0.01))
    return opacity, scale, accum, dur, thresholds


TABLE_PRUNE = [0, 1, 1, 0, 0, 0, 0, 0, 1, 0]
TABLE_CLONE = [0, 0, 0, 0, 1, 0, 0, 1, 0, 0]
TABLE_SPLIT = [0, 0, 0, 1, 0, 1, 0, 0, 0, 1]
TABLE_KEEP = [1, 0, 0, 0, 1, 0, 1, 1, 0, 0]


def _assert_mask_invariants(prune, clone, split, keep):
    assert not (prune & clone).any() and not (prune & split).any() and not (clone & split).any()
    assert np.array_equal(keep, ~(prune | split))


def test_model_masks_on_the_hand_worked_table():
    import density_reference as ref
    opacity, scale, accum, dur, thr = _table()
    prune, clone, split, keep, margin = ref.masks(opacity, scale, accum, dur, *thr)
    assert prune.astype(int).tolist() == TABLE_PRUNE
    assert clone.astype(int).tolist() == TABLE_CLONE
    assert split.astype(int).tolist() == TABLE_SPLIT
    assert keep.astype(int).tolist() == TABLE_KEEP
    _assert_mask_invariants(prune, clone, split, keep)
    assert (margin > 0.05).all()  # hand-worked: no row is anywhere near a threshold (row 3: 0.15 / 1.6 = 0.094)
    # on the thresholds themselves the functors' own sides: > and <= as written
    one = np.zeros((1, 3), np.float32)
    for c_t, want in ((1.0, (0, 1, 0)), (np.nextafter(np.float32(1), np.float32(0)), (0, 0, 1))):
        p, c, s, k, m = ref.masks([0.0], one, [1.0], [1], -1.0, 2.0, 0.5, c_t)
        assert (int(p[0]), int(c[0]), int(s[0])) == want and (m[0] == 0) == (c_t == 1.0)


def test_model_mask_invariants_on_random_rows():
    import density_reference as ref
    rng = np.random.default_rng(0)
    n = 5000
    scale = rng.normal(-3, 1.5, (n, 3)).astype(np.float32)
    scale[rng.random((n, 3)) < 0.01] = np.nan
    scale[rng.random((n, 3)) < 0.01] = np.inf
    scale[rng.random((n, 3)) < 0.01] = -np.inf
    opacity = rng.normal(-2, 2, n).astype(np.float32)
    opacity[::97] = np.nan
    prune, clone, split, keep, margin = ref.masks(opacity, scale, (rng.random(n) * 0.01).astype(np.float32),
                                                  rng.integers(0, 12, n), -3.89, 0.4, 2e-4, 0.04)
    _assert_mask_invariants(prune, clone, split, keep)
    assert prune.any() and clone.any() and split.any() and keep.any() and not np.isnan(margin).any()
    assert not prune[np.isnan(scale).all(1) & ~(opacity < -3.89)].any()  # nothing to compare: neither pruned ..
    assert not (clone | split)[np.isnan(scale).all(1)].any()             # .. nor densified


# (use_delete, use_clone, use_split) -> rows that stay in front, in order
TABLE_KEPT = {(1, 1, 1): [0, 4, 6, 7], (1, 1, 0): [0, 3, 4, 5, 6, 7, 9], (1, 0, 1): [0, 4, 6, 7],
              (1, 0, 0): [0, 3, 4, 5, 6, 7, 9], (0, 1, 1): [0, 1, 2, 4, 6, 7, 8], (0, 1, 0): list(range(10)),
              (0, 0, 1): [0, 1, 2, 4, 6, 7, 8], (0, 0, 0): list(range(10))}
TABLE_NEW_N = {(1, 1, 1): 12, (1, 1, 0): 9, (1, 0, 1): 10, (1, 0, 0): 7, (0, 1, 1): 15, (0, 1, 0): 12, (0, 0, 1): 13}


def test_model_step_layout_for_the_eight_flag_combinations(orc):
    import density_reference as ref
    opacity, scale, accum, dur, thr = _table()
    n, nsh = 10, 3
    rng = np.random.default_rng(1)
    tag = np.arange(n, dtype=np.float32)
    params = dict(xyz=rng.normal(size=(n, 3)).astype(np.float32), rgb=np.stack([tag, tag + 100, tag + 200], 1),
                  sh=rng.normal(size=(n, nsh, 3)).astype(np.float32), opacity=opacity, scale=scale,
                  quaternion=rng.normal(size=(n, 4)).astype(np.float32))
    m = {g: np.broadcast_to((tag + 0.25).reshape((n,) + (1,) * (v.ndim - 1)), v.shape).copy() for g, v in params.items()}
    v = {g: a + 0.25 for g, a in m.items()}
    mk = ref.masks(opacity, scale, accum, dur, *thr)
    counts = (3, 2, 3)
    for flags, kept in TABLE_KEPT.items():
        split_mask = ref.apply_flags(mk, flags)[2]
        children = orc.clone_split(dict(params, sh=params["sh"].reshape(n, -1)), split_mask.astype(np.uint8), nsh,
                                   split=True, scale_factor=1.6, seed=5) if split_mask.any() else None
        out = ref.step(params, m, v, mk, counts, flags, 15, nsh, children)
        if flags == (0, 0, 0):
            assert out is None  # nothing pruned, nothing added
            continue
        clones = [4, 7] if flags[1] else []
        pairs = [3, 3, 5, 5, 9, 9] if flags[2] else []
        assert out["n"] == TABLE_NEW_N[flags] == len(kept) + len(clones) + len(pairs)
        assert out["params"]["rgb"][:, 0].tolist() == kept + clones + pairs, flags
        assert out["result"] == dict(pruned=3 if flags[0] else 0, cloned=len(clones), split=len(pairs) // 2, skipped=False)
        k = len(kept)
        for g in ref.GROUPS:
            p = out["params"][g]
            assert p.shape[0] == out["n"] and p.dtype == np.float32
            assert np.array_equal(p[:k].view(np.uint32), params[g][kept].view(np.uint32)), g       # NaN and inf rows too
            assert np.array_equal(p[k:k + len(clones)].view(np.uint32), params[g][clones].view(np.uint32)), g
            assert (out["m"][g][:k].reshape(k, -1)[:, 0] == tag[kept] + 0.25).all()
            assert (out["v"][g][:k].reshape(k, -1)[:, 0] == tag[kept] + 0.5).all()
            assert not out["m"][g][k:].any() and not out["v"][g][k:].any() and out["m"][g].shape == p.shape
        assert out["params"]["sh"].shape == (out["n"], nsh, 3) and out["params"]["opacity"].ndim == 1
        if pairs:  # the children shrink by 1.6 and are two different draws
            s = out["params"]["scale"][k + len(clones):]
            np.testing.assert_allclose(s[:2, 1:], np.log(np.exp(scale[3, 1:]) / np.float32(1.6))[None].repeat(2, 0), rtol=1e-5)
            x = out["params"]["xyz"][k + len(clones):]
            assert not np.array_equal(x[0], x[1]) and np.isneginf(s[4:, 0]).all()
        assert not out["uv_grad_accum"].any() and not out["grad_accum_dur"].any()
        assert out["uv_grad_accum"].shape == out["grad_accum_dur"].shape == (out["n"],)
        assert out["grad_accum_dur"].dtype == np.int32
    # the capacity check: one row short of the room the step needs, nothing happens
    split_mask = ref.apply_flags(mk, (1, 1, 1))[2]
    children = orc.clone_split(dict(params, sh=params["sh"].reshape(n, -1)), split_mask.astype(np.uint8), nsh, split=True,
                               scale_factor=1.6, seed=5)
    assert ref.step(params, m, v, mk, counts, (1, 1, 1), 12, nsh, children)["n"] == 12
    assert ref.step(params, m, v, mk, counts, (1, 1, 1), 11, nsh, children) is None
    # no SH group: the array keeps its zero width, the optimizer has no such group
    no_sh = dict(params, sh=np.zeros((n, 0, 3), np.float32))
    m0, v0 = ({g: a for g, a in d.items() if g != "sh"} for d in (m, v))
    children = orc.clone_split(dict(no_sh, sh=np.zeros((n, 0), np.float32)), split_mask.astype(np.uint8), 0, split=True,
                               scale_factor=1.6, seed=5)
    out = ref.step(no_sh, m0, v0, mk, counts, (1, 1, 1), 100, 0, children)
    assert out["params"]["sh"].shape == (12, 0, 3) and "sh" not in out["m"] and "sh" not in out["v"]


def test_model_morton_order_is_stable_on_ties(orc):
    import density_reference as ref
    rng = np.random.default_rng(2)
    xyz = rng.normal(size=(50, 3)).astype(np.float32)
    xyz = np.concatenate([xyz, xyz[10:20]], 0)  # ten clones behind their sources
    order = ref.morton_order(xyz)
    assert sorted(order.tolist()) == list(range(60))
    pos = np.argsort(order)
    assert (pos[50:] == pos[10:20] + 1).all()  # every clone directly behind its source
    codes = orc.compute_morton_codes(xyz, xyz.max(0), xyz.min(0))
    assert (codes[order][1:] >= codes[order][:-1]).all()
    # degenerate boxes: one row; all rows the same point (identity); a plane
    assert ref.morton_order(xyz[:1]).tolist() == [0]
    assert ref.morton_order(np.tile(xyz[:1], (7, 1))).tolist() == list(range(7))
    flat = xyz.copy()
    flat[:, 2] = 0.5
    assert sorted(ref.morton_order(flat).tolist()) == list(range(60))

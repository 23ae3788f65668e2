"""Plain numpy model of classic adaptive density control: the masks of gsplat_density_masks (the reference's functors,
cuda/trainer.cu:416-512, restated literally in float32), the row layout Trainer.adaptive_density_step leaves behind
(cuda/trainer.cu:645-769) and the order Trainer.sort_gaussians puts the rows in (cuda/trainer.cu:853-922).

Nothing here is recomputed from the code under test: the masks come from the functors, the split children are handed in
(the oracle's clone_split with the step's seed) and the Morton codes are the oracle's."""
import numpy as np

GROUPS = ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")
MARGIN = 1e-5  # input-construction rule of the GPU tests: no compared quantity closer than this (relative) to its threshold
_F = np.float32


def _rel(q, t):
    """|q - t| / |t| in float64; a quantity that is NaN or infinite is on one side of any threshold in every
    implementation: its distance is infinite."""
    q, t = np.asarray(q, np.float64), float(t)
    with np.errstate(invalid="ignore"):
        d = np.abs(q - t) / max(abs(t), np.finfo(np.float64).tiny)
    return np.where(np.isfinite(q), d, np.inf)


def masks(opacity, scale, accum, dur, op_t, max_s, g_t, c_t):
    """(prune, clone, split, keep, margin): four bool arrays [N] and, per row, the smallest relative distance in float64
    from any compared quantity to its threshold (the largest extent against max_s, against 1.6 * max_s through the
    division, against c_t; the average gradient against g_t; the opacity against op_t).

    ComputeAvgGrad, ComputeScaleMax, IdentifyPrune, IdentifyClone, IdentifySplit and CombineMasks in float32; exp in
    float64, rounded; the maximum with np.fmax, which like fmaxf ignores a NaN operand."""
    opacity, accum = np.asarray(opacity, _F).reshape(-1), np.asarray(accum, _F).reshape(-1)
    scale, dur = np.asarray(scale, _F).reshape(-1, 3), np.asarray(dur, np.int32).reshape(-1)
    op_t, max_scale, g_t, c_t = _F(op_t), _F(max_s), _F(g_t), _F(c_t)
    with np.errstate(all="ignore"):
        avg = np.where(dur == 0, _F(0), accum / np.where(dur == 0, 1, dur).astype(_F)).astype(_F)
        e64 = np.exp(scale.astype(np.float64))
        e = e64.astype(_F)
        smax = np.fmax(e[:, 0], np.fmax(e[:, 1], e[:, 2]))
        smax64 = np.fmax(e64[:, 0], np.fmax(e64[:, 1], e64[:, 2]))
        exempt = (avg > g_t) & ((smax / _F(1.6)).astype(_F) <= max_scale)
        prune = np.where(opacity < op_t, True, np.where(exempt, False, smax > max_scale))
        clone = ~prune & (avg > g_t) & (smax <= c_t)
        split = ~prune & (avg > g_t) & (smax > c_t)
        keep = ~(prune | split)
        avg64 = np.where(dur == 0, 0.0, accum.astype(np.float64) / np.where(dur == 0, 1, dur))
        margin = np.minimum.reduce([_rel(smax64, max_scale), _rel(smax64 / 1.6, max_scale), _rel(smax64, c_t),
                                    _rel(avg64, g_t), _rel(opacity, op_t)])
    return prune, clone, split, keep, margin


def apply_flags(m, flags):
    """(prune, clone, split, keep) as the step uses them under flags = (use_delete, use_clone, use_split): without
    use_delete the pruned rows stay (and are neither cloned nor split: the functors already excluded them), without
    use_clone the would-be clones simply stay, without use_split the would-be splits stay as kept rows."""
    prune, clone, split = (np.asarray(a).astype(bool) for a in m[:3])
    use_delete, use_clone, use_split = flags
    if not use_delete:
        prune = np.zeros_like(prune)
    if not use_clone:
        clone = np.zeros_like(clone)
    if not use_split:
        split = np.zeros_like(split)
    return prune, clone, split, ~(prune | split)


def _rows(a, n):
    return np.asarray(a).reshape(n, -1)


def step(params, moments_m, moments_v, masks, counts, flags, max_gaussians, nsh, split_children):
    """The state after Trainer.adaptive_density_step, or None when the step is skipped (it would exceed max_gaussians)
    or has nothing to do.

    params: dict xyz rgb sh opacity scale quaternion of arrays with N rows; moments_m / moments_v: dicts of the optimizer
    groups' exp_avg / exp_avg_sq (no "sh" entry when nsh == 0); masks: what masks() returned; counts: (pruned, cloned,
    split) of those masks; split_children: dict of the 2 * count(split) new rows of apply_flags' split mask, child 0 and
    child 1 of every source in source order (oracle.clone_split(..., split=True)), or None when there is none.

    Returns dict(n, params, m, v, uv_grad_accum, grad_accum_dur, result): rows are [kept in original order | clones in
    source order | split pairs in source order]; moments follow the kept rows and are zero on new rows; the
    accumulators are zero at the new length; result is the dict the step returns."""
    n = int(np.asarray(params["xyz"]).shape[0])
    assert tuple(int(c) for c in counts) == tuple(int(np.asarray(a).sum()) for a in masks[:3]), "counts are the masks' sums"
    prune, clone, split, keep = apply_flags(masks, flags)
    n_prune, n_clone, n_split = int(prune.sum()), int(clone.sum()), int(split.sum())
    n_add = n_clone + 2 * n_split
    new_n = n - n_prune - n_split + n_add
    if new_n > max_gaussians or (n_add == 0 and n_prune == 0):
        return None
    width = dict(xyz=3, rgb=3, sh=3 * nsh, opacity=1, scale=3, quaternion=4)
    shape = dict(xyz=(new_n, 3), rgb=(new_n, 3), sh=(new_n, nsh, 3), opacity=(new_n,), scale=(new_n, 3),
                 quaternion=(new_n, 4))
    src_of_children = np.repeat(np.nonzero(split)[0], 2)
    out_p, out_m, out_v = {}, {}, {}
    for g in GROUPS:
        rows = _rows(params[g], n).astype(_F) if width[g] else np.zeros((n, 0), _F)
        assert rows.shape[1] == width[g], g
        if n_split:
            children = _rows(split_children[g], 2 * n_split).astype(_F) if width[g] else np.zeros((2 * n_split, 0), _F)
            if g not in ("xyz", "scale"):  # everything but the draw and the shrunk extent is a copy of the source
                assert np.array_equal(children.view(np.uint32), rows[src_of_children].view(np.uint32)), g
        else:
            children = np.zeros((0, width[g]), _F)
        out_p[g] = np.concatenate([rows[keep], rows[clone], children], 0).reshape(shape[g])
        if g in moments_m:
            zeros = np.zeros((n_add, width[g]), _F)
            out_m[g] = np.concatenate([_rows(moments_m[g], n)[keep], zeros], 0).astype(_F).reshape(shape[g])
            out_v[g] = np.concatenate([_rows(moments_v[g], n)[keep], zeros], 0).astype(_F).reshape(shape[g])
    return dict(n=new_n, params=out_p, m=out_m, v=out_v, uv_grad_accum=np.zeros(new_n, _F),
                grad_accum_dur=np.zeros(new_n, np.int32),
                result=dict(pruned=n_prune, cloned=n_clone, split=n_split, skipped=False))


def morton_order(xyz):
    """The permutation of Trainer.sort_gaussians: a stable sort of the oracle's Morton codes over the cloud's own box, so
    rows that share a code (a clone and its source) keep their order."""
    from oracle import oracle as orc
    xyz = np.asarray(xyz, _F).reshape(-1, 3)
    codes = orc.compute_morton_codes(xyz, xyz.max(0), xyz.min(0))
    return np.argsort(codes, kind="stable")

"""GPU tests of the view-sharded exchange's device side against tests/exchange_reference.py (float64, numpy + the CPU
oracle): gs_exchange.hip's pack and unpack kernels, and optimizer_sh_views_kernel / optimizer_sh_factored_kernel of
gs_loss.hip, at one gaussian, at +-1 around a wave (64) and a workgroup (256), at every SH degree and at 1, 2, 3 and 8
ranks.  The bound of the rebuilt SH columns is exchange_reference.K (measured by tests/test_exchange_cpu.py, which also
checks that these inputs are not vacuous); everything that only moves floats is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import exchange_reference as xr
from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7FC12345  # a quiet NaN with a payload of its own: "untouched" is checked on the bits
B1, B2, EPS = 0.9, 0.999, 1e-8


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _sentinel(*shape):
    return _dev(np.full(shape, SENTINEL_BITS, np.uint32).view(np.float32))


def _untouched(a):
    return (_bits(a) == SENTINEL_BITS).all()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


_REFS = {}


def _case(N, L, W):
    """synthetic_case + its float64 rebuild (without the rank whose camera sits on the pinned gaussian) and the
    per-element bound: computed once per shape and shared by the tests below, never modified."""
    key = (N, L, W)
    if key not in _REFS:
        c = xr.synthetic_case(N, L, W)
        c["ref"] = xr.sh_rebuild(c["xyz"], c["campos"], c["rgb"], L, skip=[c["pinned"]])
        c["bound"] = xr.rebuild_bound(c["xyz"], c["campos"], c["rgb"], L)
        rgb_all = np.zeros((W, N + 1, 3), np.float32)
        rgb_all[:, :N], rgb_all[:, N] = c["rgb"], c["campos"]
        c["rgb_all"] = rgb_all
        c["factored"] = np.concatenate([c["common"]] + [c["rgb"][r] for r in range(W)], 1)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = c
    return _REFS[key]


def _check_sh(got, c, what):
    err = np.abs(got.astype(np.float64) - c["ref"])
    worst = float((err / np.maximum(c["bound"], 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst error {worst:.3f} bounds")
    assert np.isfinite(got).all(), what
    assert (err <= c["bound"]).all(), (what, worst)  # per element, none may miss (an all-zero row: bound 0, exact 0)


# ------------------------------------------------------------------------------------ (a) unpack against float64
@pytest.mark.parametrize("world", xr.GRID_WORLD)
@pytest.mark.parametrize("L", xr.GRID_L)
@pytest.mark.parametrize("N", xr.GRID_N)
def test_unpack_matches_the_float64_rebuild(gpu, N, L, world):
    raster = pkg("raster")
    c = _case(N, L, world)
    n3, wo = 3 * xr.n_coeffs(L), xr.packed_width(L)
    sh_cols, com_cols = xr.sh_columns(L), xr.common_columns(L)
    xyz, common, rgb_all = _dev(c["xyz"]), _dev(c["common"]), _dev(c["rgb_all"])
    stride = 3 * (N + 1)
    out = {}
    full = _sentinel(N + 1, wo)
    raster.unpack_gradients_factored(xyz, _dev(c["campos"]), _dev(c["factored"]), L, N, world, full)
    out["factored"] = _np(full)
    for form, (com_in, rgb_in) in dict(both=(common, rgb_all), sh=(None, rgb_all), common=(common, None)).items():
        full = _sentinel(N + 1, wo)
        raster.unpack_gradients_split(xyz if rgb_in is not None else None, com_in, rgb_in, stride, L, N, world, full)
        out[form] = _np(full)
    for form, got in out.items():
        assert _untouched(got[N]), (form, "row N written")
        if form != "common":
            _check_sh(got[:N][:, sh_cols], c, f"{form} N={N} L={L} W={world}")
        else:
            assert _untouched(got[:N][:, sh_cols]), "the common-only form wrote an SH column"
        if form != "sh":
            assert _same_bits(got[:N][:, com_cols], c["common"]), (form, "common columns are copies")
        else:
            assert _untouched(got[:N][:, com_cols]), "the SH-only form wrote a common column"
    assert sh_cols.size == n3 and sh_cols.size + com_cols.size == wo
    assert _same_bits(out["factored"], out["both"]), "factored and split unpack differ"
    assert _same_bits(out["sh"][:N][:, sh_cols], out["both"][:N][:, sh_cols])
    rank, row = c["pinned"]  # that rank's camera sits on this gaussian and its g_rgb there is zero: the rank is skipped,
    assert (c["campos"][rank] == c["xyz"][row]).all() and not c["rgb"][rank, row].any()  # (c["ref"] was built without it)


def test_unpack_with_padded_rank_blocks(gpu):
    """rank_stride larger than 3 (N + 1): the floats between the blocks are NaN sentinels and must not be read."""
    import torch
    raster = pkg("raster")
    N, L, W = 65, 3, 3
    c = _case(N, L, W)
    wo, stride = xr.packed_width(L), 3 * (N + 1) + 5
    padded = np.full((W, stride), SENTINEL_BITS, np.uint32).view(np.float32)
    padded[:, :3 * (N + 1)] = c["rgb_all"].reshape(W, -1)
    xyz, common = _dev(c["xyz"]), _dev(c["common"])
    tight, wide = _sentinel(N + 1, wo), _sentinel(N + 1, wo)
    raster.unpack_gradients_split(xyz, common, _dev(c["rgb_all"]), 3 * (N + 1), L, N, W, tight)
    raster.unpack_gradients_split(xyz, common, _dev(padded), stride, L, N, W, wide)
    torch.cuda.synchronize()
    _check_sh(_np(wide)[:N][:, xr.sh_columns(L)], c, "padded stride")
    assert _same_bits(_np(wide), _np(tight))


# ------------------------------------------------------------------------- (b) pack on a real context's mask and rank
def _packing_scene(scene, N, W, H, L):
    params = scene.make_gaussians(N, W, H, L)
    params["xyz"][1::3, 2] *= -1  # every third gaussian behind the camera (gaussian 0 stays: N = 1 has one in view)
    params["xyz"][60:69, 2] = -np.abs(params["xyz"][60:69, 2])  # and a culled run across the wave bound at 64
    return params


def _known_gradients(torch, ctx, M, L, seed):
    grads = ctx.alloc_gradients(M, L, intermediates=("uv", "precompute_rgb"))
    rng = np.random.default_rng(seed)
    host = {}
    for k, t in grads.items():
        host[k] = rng.standard_normal(tuple(t.shape)).astype(np.float32)
        t.copy_(torch.from_numpy(host[k]))
    return grads, host


@pytest.mark.parametrize("L", [0, 2, 3])
@pytest.mark.parametrize("N", [1, 65, 257, 600])
def test_pack_moves_exactly_the_reference_rows(gpu, scene, N, L):
    """Every pack kernel against exchange_reference on the mask and compact_to_global of a real forward -- the kernels
    index through rank[], the reference through compact_to_global -- after the context's first forward and again after
    its second, which walks the compacted slots and leaves rank[] of culled rows slice-local.  No backward runs: the
    gradient arrays hold known random values."""
    torch, raster = gpu, pkg("raster")
    W, H = 96, 64
    params = _packing_scene(scene, N, W, H, L)
    c = scene.CONFIG
    ctx = raster.RasterContext(N, W, H)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 1))
    wo = xr.packed_width(L)
    for visit in (0, 1):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        M = int(fwd["num_culled"])
        mask, c2g = _np(fwd["mask"]).astype(bool), _np(fwd["compact_to_global"]).copy()
        assert int(mask.sum()) == M and (N == 1 or 0 < M < 0.8 * N)
        if N > 1:
            assert not mask[1] and not mask[60:69].any() and ctx.counters()["compact_walks"] == visit
        grads, host = _known_gradients(torch, ctx, M, L, seed=100 * N + 10 * L + visit)
        # global rows
        packed = _sentinel(N + 1, wo)
        ctx.pack_gradients_global(grads, L, N, packed)
        got = _np(packed)
        assert _same_bits(got[:N], xr.global_rows(mask, c2g, host, L)) and _untouched(got[N]), (visit, "global")
        # factored rows: a rank fills its own slot, the other ranks' slots are exactly zero
        for world in (1, 3):
            for rank in range(world):
                f = _sentinel(N + 1, 12 + 3 * world)
                raster.pack_gradients_factored(ctx, grads, N, rank, world, f)
                got, want = _np(f), xr.factored_rows(mask, c2g, host, rank, world)
                assert _same_bits(got[:N], want) and _untouched(got[N]), (visit, "factored", rank, world)
                others = [k for k in range(12, 12 + 3 * world) if (k - 12) // 3 != rank]
                assert (_bits(got[:N][:, others]) == 0).all()
        # split rows, with and without the g_rgb block
        want_common, want_rgb = xr.split_rows(mask, c2g, host)
        common, rgb = _sentinel(N + 1, 12), _sentinel(N + 1, 3)
        raster.pack_gradients_split(ctx, grads, N, common, rgb)
        assert _same_bits(_np(common)[:N], want_common) and _same_bits(_np(rgb)[:N], want_rgb), (visit, "split")
        assert _untouched(_np(common)[N]) and _untouched(_np(rgb)[N])
        common = _sentinel(N + 1, 12)
        raster.pack_gradients_split(ctx, grads, N, common, None)
        assert _same_bits(_np(common)[:N], want_common) and _untouched(_np(common)[N]), (visit, "split, no rgb")
        # ranges: empty, one row at either end, bounds at the wave edge +-1, bounds on culled indices
        culled = np.flatnonzero(~mask)
        ranges = [(0, 0), (0, 1), (N - 1, N), (N, N), (63, 64), (63, 65), (64, 65), (65, N), (1, 63)]
        if len(culled) >= 2:
            ranges += [(int(culled[0]), int(culled[-1])), (int(culled[1]), int(culled[-1]) + 1)]
            if N > 65:
                ranges += [(61, int(culled[-1])), (64, 67)]  # inside the culled run, across the wave bound
        for first, end in ranges:
            if not 0 <= first <= end <= N:
                continue
            for with_rgb in (True, False):
                common, rgb = _sentinel(N + 1, 12), _sentinel(N + 1, 3)
                raster.pack_gradients_split_range(ctx, grads, N, first, end, common, rgb if with_rgb else None)
                gc, gr = _np(common), _np(rgb)
                inside = np.zeros(N + 1, bool)
                inside[first:end] = True
                assert _same_bits(gc[first:end], want_common[first:end]), (visit, first, end)
                assert _untouched(gc[~inside]), (visit, first, end, "a row outside the range was written")
                if with_rgb:
                    assert _same_bits(gr[first:end], want_rgb[first:end]) and _untouched(gr[~inside]), (visit, first, end)
                else:
                    assert _untouched(gr)
        # |grad_uv|: within one ulp of the float64 value rounded to float32, exactly 0 where culled
        norm = _sentinel(N + 1)
        raster.pack_uv_grad_norm(ctx, grads, N, norm)
        got = _np(norm)
        want = xr.uv_norm(mask, c2g, host["uv"]).astype(np.float32)
        assert _untouched(got[N:]) and (_bits(got[:N][~mask]) == 0).all()
        assert (np.abs(got[:N].astype(np.float64) - want) <= np.spacing(want)).all(), (visit, "uv norm")


@pytest.mark.parametrize("exchange", ["split", "factored", "full"])
@pytest.mark.parametrize("N", [1, 65])
def test_a_view_that_culls_everything_packs_zeros(gpu, scene, N, exchange):
    """M = 0: the forward reports "nothing in view" (-5) and records nothing, so there is no rank[] to pack through; the
    exchange step (dist.ViewShardedStep) takes that report and must deliver all-zero rows, uv norms and g_rgb without
    raising -- over buffers that held another view's values."""
    torch, raster, gdist = gpu, pkg("raster"), pkg("dist")
    W, H, L = 96, 64, 2
    params = scene.make_gaussians(N, W, H, L)
    c = scene.CONFIG
    cam = raster.device_camera(scene.make_camera(W, H, 1))
    dp = raster.device_params(params)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    step = gdist.ViewShardedStep(dp, L, W, H, c, c["bg"], exchange=exchange, with_uv_norm=True, exchange_at_world_one=True)
    assert step.step(cam, gi) is not None
    assert bool((step.packed != 0).any())
    dp["xyz"][:, 2] = -dp["xyz"][:, 2].abs()  # everything behind the camera
    assert step.step(cam, gi) is None
    torch.cuda.synchronize()
    assert (_bits(_np(step.packed)) == 0).all() and (_bits(_np(step.uv_norm_sum)) == 0).all()
    if exchange == "split":
        assert (_bits(_np(step.common)) == 0).all() and (_bits(_np(step.rgb_all[0, :N])) == 0).all()
        assert torch.equal(step.rgb_all[0, N], cam["campos_dev"])
    # and the pack entry points themselves refuse a context whose last forward recorded nothing
    grads = step.ctx.alloc_gradients(1, L, intermediates=("uv", "precompute_rgb"))
    with pytest.raises(pkg("_lib").GsplatError) as refused:
        step.ctx.pack_gradients_global(grads, L, N, torch.zeros(N, xr.packed_width(L), device="cuda"))
    assert refused.value.code == -3


# ------------------------------------------------------------- (c) the colour groups' optimizer kernels at the edges
def _seen_column(N, world, rng):
    """common[:, 11] with, where the waves are there: wave 0 unseen as a whole, wave 1 seen in lane 0 only, wave 2 in lane
    63 only, a mixed wave holding one NaN and one -1 (neither is `> 0`), and the last wave -- ragged unless 64 divides N --
    seen in its last row.  Two waves (N = 65): wave 0 seen in lane 63 only, holding the NaN and the -1."""
    s = rng.integers(0, world + 1, N).astype(np.float32)
    nw = (N + 63) // 64
    special = []
    if nw >= 4:
        s[0:192] = 0
        s[64], s[191] = 1, world
        mixed = 3
    elif nw == 2:
        s[0:64] = 0
        s[63] = 1
        mixed = 0
    else:
        mixed = 0
    if N >= 3:
        special = [64 * mixed + 1, 64 * mixed + 2]
        s[special[0]], s[special[1]] = np.nan, -1.0
        if nw == 1:
            s[3 if N > 3 else 0] = world  # (a seen row beside them)
    s[N - 1] = world
    return s, special


def _plant(arrays, rows):
    """bits that must survive in rows no view saw (as test_masked_optimizer_steps_equal_adam_step_bit_for_bit plants them)"""
    vals = np.float32([np.nan, np.inf, -np.inf, 1e-40, -0.0, 0.0])
    for a in arrays:
        flat = a.reshape(a.shape[0], -1)
        for j, r in enumerate(rows):
            if flat.shape[1]:
                flat[r] = np.resize(np.roll(vals, j), flat.shape[1])


def _opt_cases():
    out = []
    for i, N in enumerate(xr.GRID_N):
        for L in xr.GRID_L:
            out.append((N, L, xr.GRID_WORLD[(i + L) % 4]))
            if N == 257 and out[-1][2] != 8:
                out.append((N, L, 8))
    return out


@pytest.mark.parametrize("N,L,world", _opt_cases())
def test_split_step_at_wave_and_block_edges(gpu, orc, N, L, world):
    """AdamOptimizer.step_split (optimizer_sh_views_kernel + the packed kernel on common) against
    unpack_gradients_split + step_packed, two consecutive steps: parameters and both moments of every group bit-identical,
    rows no view saw untouched bit for bit; and the seen rows' first step anchored to the oracle's adam_step on the float32
    gradient that the unpack produced (which test_unpack_matches_the_float64_rebuild pins to float64)."""
    torch, raster, opt_mod = gpu, pkg("raster"), pkg("optimizer")
    c = _case(N, L, world)
    rng = np.random.default_rng([7, N, L, world])
    common = c["common"].copy()
    common[:, 11], special = _seen_column(N, world, rng)
    seen = common[:, 11] > 0
    unseen = np.flatnonzero(~seen)
    assert seen[N - 1] and (N < 3 or (len(unseen) >= 2 and not seen[special].any()))
    if N >= 255:
        assert not seen[:64].any() and list(np.flatnonzero(seen[64:192])) == [0, 127]
    nr = xr.n_coeffs(L) - 1
    shapes = dict(xyz=(N, 3), rgb=(N, 3), sh=(N, nr, 3), opacity=(N,), scale=(N, 3), quaternion=(N, 4))
    start = {}
    for g, s in shapes.items():
        p = c["xyz"].copy() if g == "xyz" else rng.standard_normal(s).astype(np.float32)
        m = (rng.standard_normal(s) * 1e-4).astype(np.float32)
        v = (rng.random(s) * 1e-8).astype(np.float32)
        if g != "xyz":  # (xyz feeds the directions of every row, seen or not: its unseen rows stay ordinary numbers)
            _plant((p, m, v), list(special) + list(unseen[:2]))
        start[g] = (p, m, v)
    twins = []
    for _ in range(2):
        params = {g: _dev(start[g][0]) for g in shapes}
        opt = opt_mod.AdamOptimizer(params, L, scene_extent=2.5)
        for g in opt.names:
            opt.exp_avg[g].copy_(_dev(start[g][1]))
            opt.exp_avg_sq[g].copy_(_dev(start[g][2]))
        twins.append((params, opt))
    (pa, oa), (pb, ob) = twins
    d_common, d_rgb_all = _dev(common), _dev(c["rgb_all"])
    wo = xr.packed_width(L)
    first_grad = None
    for it in (3, 4):
        packed = _sentinel(N, wo)
        raster.unpack_gradients_split(pb["xyz"], d_common, d_rgb_all, 3 * (N + 1), L, N, world, packed)
        if first_grad is None:
            first_grad = _np(packed)
        oa.step_split(it, d_common, d_rgb_all)
        ob.step_packed(it, packed)
        torch.cuda.synchronize()
        for g in oa.names:
            got = [_np(pa[g]), _np(oa.exp_avg[g]), _np(oa.exp_avg_sq[g])]
            twin = [_np(pb[g]), _np(ob.exp_avg[g]), _np(ob.exp_avg_sq[g])]
            for what, a, b, s0 in zip("pmv", got, twin, start[g]):
                assert _same_bits(a, b), (it, g, what)
                assert _same_bits(a[~seen], s0[~seen]), (it, g, what, "a row no view saw was written")
                if it == 3 and seen.any() and a[seen].size:
                    assert not _same_bits(a[seen], s0[seen]), (g, what, "seen rows did not move")
        if it == 3:  # the colour groups' seen rows against the oracle's adam_step
            b1c, b2c = opt_mod.AdamOptimizer.bias_corrections(it)
            lrs = oa.learning_rates(it)
            for g, lo, hi in (("rgb", 3, 6), ("sh", 6, 6 + 3 * nr)):
                if g not in oa.names:
                    continue
                p0, m0, v0 = (x.reshape(N, -1)[seen] for x in start[g])
                grad = first_grad[seen][:, lo:hi]
                p, m, v = orc.adam_step(p0, grad, m0, v0, np.float32(lrs[g]), np.float32(B1), np.float32(B2),
                                        np.float32(EPS), np.float32(b1c), np.float32(b2c))
                np.testing.assert_allclose(_np(oa.exp_avg[g]).reshape(N, -1)[seen], m.reshape(grad.shape), rtol=2e-6, atol=1e-12)
                np.testing.assert_allclose(_np(oa.exp_avg_sq[g]).reshape(N, -1)[seen], v.reshape(grad.shape), rtol=2e-6, atol=1e-20)
                np.testing.assert_allclose(_np(pa[g]).reshape(N, -1)[seen], p.reshape(grad.shape), rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 63, 65, 257])
def test_factored_sh_step_at_wave_and_block_edges(gpu, orc, M, L):
    """gsplat_optimizer_step_sh_factored on M rows of N = M + 7 through a permuted compact_to_global, against
    gsplat_optimizer_step reading the stored g (x) Y rows -- which are the rebuild of one view on the compacted positions
    (gsplat_unpack_gradients_split, world 1), checked here against float64 with the bound of the unpack tests.  Two steps:
    the SH group and both moments bit-identical, the seven rows outside the view untouched bit for bit, the first step
    within the optimizer tests' tolerances of the oracle's adam_step."""
    torch, raster, opt_mod, lib_mod = gpu, pkg("raster"), pkg("optimizer"), pkg("_lib")
    lib, check = lib_mod.load(), lib_mod.check
    N, nr = M + 7, xr.n_coeffs(L) - 1
    rng = np.random.default_rng([11, M, L])
    c2g = rng.permutation(N)[:M].astype(np.int32)
    outside = np.setdiff1d(np.arange(N), c2g)
    xyz = (2.0 * rng.standard_normal((N, 3))).astype(np.float32)
    campos = (3.0 * rng.standard_normal(3)).astype(np.float32)
    g_rgb = (rng.standard_normal((M, 3)) * 10.0 ** rng.uniform(-4, 0, (M, 1))).astype(np.float32)
    g_rgb[np.arange(M) % 5 == 2] = 0.0
    # the stored gradient rows: one view's rebuild on the compacted positions
    rgb_all = np.concatenate([g_rgb, campos[None]])[None]
    full = _sentinel(M, xr.packed_width(L))
    raster.unpack_gradients_split(_dev(xyz[c2g]), None, _dev(rgb_all), 3 * (M + 1), L, M, 1, full)
    stored = np.ascontiguousarray(_np(full)[:, 6:6 + 3 * nr])
    ref = xr.sh_rebuild(xyz[c2g], campos[None], g_rgb[None], L)[:, 3:]
    bound = xr.rebuild_bound(xyz[c2g], campos[None], g_rgb[None], L)[:, 3:]
    assert (np.abs(stored.astype(np.float64) - ref) <= bound).all()
    start = [rng.standard_normal((N, nr, 3)).astype(np.float32), (rng.standard_normal((N, nr, 3)) * 1e-4).astype(np.float32),
             (rng.random((N, nr, 3)) * 1e-8).astype(np.float32)]
    _plant(start, outside[:3])
    a, b = [_dev(x) for x in start], [_dev(x) for x in start]
    d_c2g, d_xyz, d_g, d_stored = _dev(c2g), _dev(xyz), _dev(g_rgb), _dev(stored)
    lr = 1.25e-4
    grp = (lib_mod.AdamGroup * 1)()
    grp[0].param, grp[0].exp_avg, grp[0].exp_avg_sq, grp[0].grad = (t.data_ptr() for t in (*b, d_stored))
    grp[0].stride, grp[0].packed_column, grp[0].lr = 3 * nr, 0, lr
    for it in (3, 4):
        b1c, b2c = opt_mod.AdamOptimizer.bias_corrections(it)
        check(lib.gsplat_optimizer_step_sh_factored(_p(d_c2g), M, L, _p(a[0]), _p(a[1]), _p(a[2]), lr, B1, B2, EPS, b1c, b2c,
                                                    _p(d_xyz), float(campos[0]), float(campos[1]), float(campos[2]), _p(d_g),
                                                    _stream()))
        check(lib.gsplat_optimizer_step(_p(d_c2g), M, grp, 1, B1, B2, EPS, b1c, b2c, None, None, None, _stream()))
        torch.cuda.synchronize()
        for what, x, y, s0 in zip("pmv", a, b, start):
            assert _same_bits(_np(x), _np(y)), (it, what)
            assert _same_bits(_np(x)[outside], s0[outside]), (it, what, "a row outside the view was written")
        if it == 3:
            want = orc.adam_step(start[0][c2g], stored, start[1][c2g], start[2][c2g], np.float32(lr), np.float32(B1),
                                 np.float32(B2), np.float32(EPS), np.float32(b1c), np.float32(b2c))
            for x, w, atol in zip(a, want, (1e-7, 1e-12, 1e-20)):
                np.testing.assert_allclose(_np(x)[c2g].reshape(M, -1), w.reshape(M, -1), rtol=2e-6, atol=atol)
            assert not _same_bits(_np(a[0])[c2g], start[0][c2g])


# -------------------------------------------------------------------------------- (d) refusals: status codes, no launch
def test_exchange_argument_refusals(gpu, scene):
    torch, raster, lib_mod = gpu, pkg("raster"), pkg("_lib")
    lib = lib_mod.load()
    N, L, W, H = 65, 3, 96, 64
    wo = xr.packed_width(L)
    xyz, common = torch.zeros(N, 3, device="cuda"), torch.zeros(N, 12, device="cuda")
    rgb_all, full = torch.zeros(2, N + 1, 3, device="cuda"), _sentinel(N, wo)
    fact, campos = torch.zeros(N, 18, device="cuda"), torch.zeros(2, 3, device="cuda")
    split = lambda stride, l, world: lib.gsplat_unpack_gradients_split(_p(xyz), _p(common), _p(rgb_all), stride, l, N, world,
                                                                       _p(full), None)
    factored = lambda l, world: lib.gsplat_unpack_gradients_factored(_p(xyz), _p(campos), _p(fact), l, N, world, _p(full), None)
    assert split(3 * N + 2, L, 2) == -3   # rank_stride short of [N,3] g_rgb + campos[3]
    assert split(3 * N + 3, L, 0) == -3 and factored(L, 0) == -3   # world_size 0
    assert split(3 * N + 3, 4, 2) == -3 and factored(4, 2) == -3   # l_max 4
    assert split(3 * N + 3, -1, 2) == -3 and factored(-1, 2) == -3
    assert lib.gsplat_unpack_gradients_split(_p(xyz), None, None, 3 * N + 3, L, N, 2, _p(full), None) == -3  # nothing to unpack
    torch.cuda.synchronize()
    assert _untouched(_np(full)), "a refused unpack wrote"
    # the pack entry points: a context with no recorded forward, then bad ranges / ranks on one that has one
    ctx = raster.RasterContext(N, W, H)
    grads = ctx.alloc_gradients(N, L, intermediates=("uv", "precompute_rgb"))
    gs = raster.RasterContext._grad_struct(grads)
    out12, out3, outw, outf = _sentinel(N, 12), _sentinel(N, 3), _sentinel(N, wo), _sentinel(N, 18)
    calls = dict(
        glob=lambda: lib.gsplat_pack_gradients_global(ctx._h, ctypes.byref(gs), L, N, _p(outw), None),
        fact=lambda: lib.gsplat_pack_gradients_factored(ctx._h, ctypes.byref(gs), N, 0, 2, _p(outf), None),
        split=lambda: lib.gsplat_pack_gradients_split(ctx._h, ctypes.byref(gs), N, _p(out12), _p(out3), None),
        rng=lambda: lib.gsplat_pack_gradients_split_range(ctx._h, ctypes.byref(gs), N, 0, N, _p(out12), _p(out3), None),
        uv=lambda: lib.gsplat_pack_uv_grad_norm(ctx._h, ctypes.byref(gs), N, _p(out3), None))
    for name, call in calls.items():
        assert call() == -3, (name, "packed through a context without a forward")
    params = scene.make_gaussians(N, W, H, L)
    c = scene.CONFIG
    ctx.rasterize_image(raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 1)), c, c["bg"], L)
    rng_call = lambda first, end: lib.gsplat_pack_gradients_split_range(ctx._h, ctypes.byref(gs), N, first, end, _p(out12),
                                                                        _p(out3), None)
    assert rng_call(5, 4) == -3 and rng_call(0, N + 1) == -3 and rng_call(-1, 3) == -3   # first > end, end > N
    assert lib.gsplat_pack_gradients_split_range(ctx._h, ctypes.byref(gs), N + 1, 0, N, _p(out12), _p(out3), None) == -3
    assert lib.gsplat_pack_gradients_global(ctx._h, ctypes.byref(gs), L - 1, N, _p(outw), None) == -3   # another l_max
    for rank, world in ((0, 0), (2, 2), (-1, 2)):
        assert lib.gsplat_pack_gradients_factored(ctx._h, ctypes.byref(gs), N, rank, world, _p(outf), None) == -3
    bare = raster.RasterContext._grad_struct({k: v for k, v in grads.items() if k != "precompute_rgb"})
    assert lib.gsplat_pack_gradients_factored(ctx._h, ctypes.byref(bare), N, 0, 2, _p(outf), None) == -1   # no g_rgb array
    assert lib.gsplat_pack_gradients_split(ctx._h, ctypes.byref(bare), N, _p(out12), _p(out3), None) == -1
    torch.cuda.synchronize()
    for t in (out12, out3, outw, outf):
        assert _untouched(_np(t)), "a refused pack wrote"

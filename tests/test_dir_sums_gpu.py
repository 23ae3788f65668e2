"""The SH direction sums (gs_math.h: sh_dir_sums; RasterContext.set_dir_sums): the fused per-gaussian forward leaves the
nine sums over each SH row that the backward needs, and the plain per-gaussian backward -- and the one with the small
groups' Adam step inside, the trainer's default -- reads those instead of the rows, band 0 and the camera-space position
(SH degree 1 and up: degree 0 has no row to save and writes no sums).  The sums are the backward's own -- the same
arithmetic on the same inputs -- so every forward output and every gradient must be the SAME BITS with the switch on and off, NaN and inf coefficients included; a
backward may read only the sums of the forward it differentiates; the counters say which path a backward took.

The compositing backward's float atomics are order-dependent, so the two per-gaussian backwards that are compared always
run on the rows of ONE gsplat_backward_render call."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

W, H = 64, 48
LEAVES = ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")
FORWARD_OUTPUTS = ("image", "T", "n", "sorted", "ranges", "radius", "uv", "xyz_c", "compact_to_global", "mask")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _scene(scene, N, L, culled, seed_shift=0):
    """culled: about 40 % of the gaussians behind the camera, interleaved (scattered rows in every wave); else all of them in
    view (each wave's rows one linear span).  One coefficient NaN and one inf, in gaussians the camera sees."""
    params = scene.make_gaussians(N, W, H, L, seed=scene.SEED + seed_shift)
    if culled:
        params = scene.cull_half(params, fraction=0.4)
    seen = np.flatnonzero(params["xyz"][:, 2] > 1.0)
    a, b = int(seen[len(seen) // 3]), int(seen[(2 * len(seen)) // 3])
    if L > 0:
        params["sh"][a, 0, 1] = np.nan
        params["sh"][b, -1, 2] = np.inf
    else:  # degree 0: band 0 is the only coefficient there is
        params["rgb"][a, 1] = np.nan
        params["rgb"][b, 2] = np.inf
    return params


def _backward_both(torch, ctx, dp, dc, L, M):
    """backward_gaussians twice on the rows that are there: switch on, switch off.  Returns the two gradient dicts (host) and
    how the counters moved."""
    before = ctx.counters()
    out = []
    for on in (True, False):
        ctx.set_dir_sums(on)
        grads = ctx.alloc_gradients(M, L)
        for g in grads.values():
            g.fill_(float("nan"))
        ctx.backward_gaussians(dp, dc, L, grads)
        torch.cuda.synchronize()
        out.append({k: _np(v).copy() for k, v in grads.items()})
    ctx.set_dir_sums(True)
    after = ctx.counters()
    moved = {k: after[k] - before[k] for k in ("dir_sums_backwards", "dir_sums_fallbacks")}
    return out[0], out[1], moved


def _assert_same_bits(got, want, what):
    for k in LEAVES:
        assert got[k].shape == want[k].shape, (what, k)
        diff = int((_bits(got[k]) != _bits(want[k])).sum())
        assert diff == 0, f"{what}: grad_{k} differs in {diff} of {got[k].size} words"


CASES = [(N, L, True, False) for N in (257, 1000) for L in (0, 1, 2, 3)] + [(1000, 3, False, False), (257, 1, False, False),
                                                                            (1000, 3, True, True), (1000, 2, False, True)]


@pytest.mark.parametrize("N,L,culled,full", CASES,
                         ids=[f"N{n}-L{l}-{'culled' if c else 'all'}-{'full' if f else 'lean'}" for n, l, c, f in CASES])
def test_switch_changes_no_bit(gpu, scene, N, L, culled, full):
    """Two forwards with the switch on (the second walks the compacted slots when the first culled a fifth or more), one
    with it off: the same forward outputs; after each forward with the switch on, the backward on the sums and the
    backward on the rows give the same six leaf arrays, word for word."""
    torch, raster = gpu, pkg("raster")
    c = scene.CONFIG
    params = _scene(scene, N, L, culled)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_lean_forward(not full)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    outputs = []
    for it, on in enumerate((True, True, False)):
        ctx.set_dir_sums(on)
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        torch.cuda.synchronize()
        M = fwd["num_culled"]
        outputs.append({k: _np(fwd[k]).copy() for k in FORWARD_OUTPUTS})
        if it == 0:
            if culled:
                assert 0.5 * N < M < 0.7 * N and M % 64 != 0, M  # scattered rows, a partial last wave
            else:
                assert M == N and M % 64 != 0, M
        ctx.backward_render(gi, c["bg"])
        g_on, g_off, moved = _backward_both(torch, ctx, dp, dc, L, M)
        if on and L == 0:  # degree 0 has no row to save: no forward writes sums there
            assert moved == dict(dir_sums_backwards=0, dir_sums_fallbacks=2), moved
            _assert_same_bits(g_on, g_off, f"forward {it}")
        elif on:
            assert moved == dict(dir_sums_backwards=1, dir_sums_fallbacks=1), moved
            _assert_same_bits(g_on, g_off, f"forward {it}")
            assert np.isnan(g_on["xyz"]).any(), "the NaN coefficient must reach the position gradient"
        else:  # a forward that wrote no sums: both backwards read the rows
            assert moved == dict(dir_sums_backwards=0, dir_sums_fallbacks=2), moved
            _assert_same_bits(g_on, g_off, f"forward {it}")
    if culled:
        assert ctx.counters()["compact_walks"] >= 1
    for k in FORWARD_OUTPUTS:
        for other in outputs[1:]:
            a, b = outputs[0][k], other[k]
            same = (_bits(a) == _bits(b)) if a.dtype == np.float32 else (a == b)
            assert same.all(), k
    ctx.close()


def _fresh(raster, scene, N, L, seed_shift=0):
    params = _scene(scene, N, L, True, seed_shift)
    return params, raster.device_params(params)


def test_forwards_that_write_no_sums_fall_back(gpu, scene):
    """The two-kernel forwards, the anti-aliased forward and a forward with the switch off leave no sums: a backward behind
    them reads the rows -- also when the forward BEFORE wrote sums, which are stale by then."""
    torch, raster = gpu, pkg("raster")
    N, L, c = 1000, 3, scene.CONFIG
    params, dp = _fresh(raster, scene, N, L)
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx = raster.RasterContext(N, W, H)
    for name, setup, undo in (("split 1", lambda: ctx.set_preprocess_split(1), lambda: ctx.set_preprocess_split(0)),
                              ("split 2", lambda: ctx.set_preprocess_split(2), lambda: ctx.set_preprocess_split(0)),
                              ("antialiased", lambda: ctx.set_antialiased(True), lambda: ctx.set_antialiased(False)),
                              ("switch off", lambda: ctx.set_dir_sums(False), lambda: ctx.set_dir_sums(True))):
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)  # writes sums
        setup()
        fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)  # writes none: the buffer still holds the forward before's
        undo()  # (the switches are read by forwards; the backward follows the recorded forward)
        ctx.backward_render(gi, c["bg"])
        g_on, g_off, moved = _backward_both(torch, ctx, dp, dc, L, fwd["num_culled"])
        assert moved == dict(dir_sums_backwards=0, dir_sums_fallbacks=2), (name, moved)
        _assert_same_bits(g_on, g_off, name)
    ctx.close()


def test_backward_reads_the_last_forwards_sums(gpu, scene):
    """Forward A, then forward B on other parameters, then a backward of B: B's sums, the bits of the rows path on B.  A
    backward that is handed OTHER arrays than its forward was reads the rows, as does one at another camera centre."""
    torch, raster = gpu, pkg("raster")
    N, L, c = 1000, 3, scene.CONFIG
    _, dpa = _fresh(raster, scene, N, L)
    _, dpb = _fresh(raster, scene, N, L, seed_shift=1)
    cam = scene.make_camera(W, H, 0)
    dc = raster.device_camera(cam)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx = raster.RasterContext(N, W, H)
    ctx.rasterize_image(dpa, dc, c, c["bg"], L)
    fwd = ctx.rasterize_image(dpb, dc, c, c["bg"], L)
    ctx.backward_render(gi, c["bg"])
    g_on, g_off, moved = _backward_both(torch, ctx, dpb, dc, L, fwd["num_culled"])
    assert moved == dict(dir_sums_backwards=1, dir_sums_fallbacks=1), moved
    _assert_same_bits(g_on, g_off, "forward B")
    # the same values in other arrays: not the arrays the sums were formed from
    dpc = {k: v.clone() for k, v in dpb.items()}
    g_on2, g_off2, moved = _backward_both(torch, ctx, dpc, dc, L, fwd["num_culled"])
    assert moved == dict(dir_sums_backwards=0, dir_sums_fallbacks=2), moved
    _assert_same_bits(g_on2, g_off, "cloned arrays")
    # another camera centre (the view direction of the backward would not be the forward's)
    cam2 = dict(cam)
    cam2["campos"] = np.asarray(cam["campos"], np.float32) + np.float32(0.25)
    dc2 = raster.device_camera(cam2)
    dc2["view"], dc2["proj"] = dc["view"], dc["proj"]
    g_on3, g_off3, moved = _backward_both(torch, ctx, dpb, dc2, L, fwd["num_culled"])
    assert moved == dict(dir_sums_backwards=0, dir_sums_fallbacks=2), moved
    _assert_same_bits(g_on3, g_off3, "other camera centre")
    ctx.close()


def test_another_degree_is_refused_either_way(gpu, scene):
    """A backward at another l_max than its forward's never reaches a kernel, with the switch on or off (the entry points
    compare it with the recorded forward); the context goes on as before."""
    torch, raster, lib = gpu, pkg("raster"), pkg("_lib")
    N, c = 257, scene.CONFIG
    params, dp = _fresh(raster, scene, N, 3)
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], 3)
    ctx.backward_render(gi, c["bg"])
    low = dict(dp)
    low["sh"] = dp["sh"][:, :8, :].contiguous()
    before = ctx.counters()
    for on in (True, False):
        ctx.set_dir_sums(on)
        with pytest.raises(lib.GsplatError):
            ctx.backward_gaussians(low, dc, 2, ctx.alloc_gradients(fwd["num_culled"], 2))
    after = ctx.counters()
    assert (after["dir_sums_backwards"], after["dir_sums_fallbacks"]) == (before["dir_sums_backwards"], before["dir_sums_fallbacks"])
    g_on, g_off, moved = _backward_both(torch, ctx, dp, dc, 3, fwd["num_culled"])
    assert moved == dict(dir_sums_backwards=1, dir_sums_fallbacks=1), moved
    _assert_same_bits(g_on, g_off, "after the refusals")
    ctx.close()


def test_render_only_context_allocates_no_sums(gpu, scene):
    torch, raster = gpu, pkg("raster")
    N, L, c = 1000, 3, scene.CONFIG
    params, dp = _fresh(raster, scene, N, L)
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    sizes = {}
    for name, render_only, on in (("render-only", True, True), ("training", False, True), ("training, off", False, False)):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_render_only(render_only)
        ctx.set_dir_sums(on)
        before = ctx.workspace_bytes
        ctx.rasterize_image(dp, dc, c, c["bg"], L)
        torch.cuda.synchronize()
        sizes[name] = ctx.workspace_bytes - before
        ctx.close()
    assert sizes["training"] >= sizes["training, off"] + 36 * N, sizes
    assert sizes["render-only"] <= sizes["training, off"], sizes


@pytest.mark.parametrize("L,culled", [(3, True), (1, True), (3, False), (0, True)], ids=["L3-culled", "L1-culled", "L3-all", "L0-culled"])
def test_backward_with_the_small_groups_adam_inside(gpu, scene, L, culled):
    """The trainer's default iteration: gsplat_backward_gaussians_adam, mode 1.  On the sums and on the rows -- the same
    compositing rows, the same parameters and moments restored in place in between -- parameters, moments, statistics and
    the arrays handed to the optimizer kernels are the same bits.  An Adam backward steps parameters the sums were formed
    from: whatever it read, the sums are nobody's afterwards."""
    torch, raster, opt_mod = gpu, pkg("raster"), pkg("optimizer")
    N, c = 1000, scene.CONFIG
    params = _scene(scene, N, L, culled)
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    opt = opt_mod.AdamOptimizer(dp, L, scene_extent=2.5)
    rng = np.random.default_rng(7)
    for g in opt.names:
        opt.exp_avg[g].copy_(torch.from_numpy((rng.standard_normal(tuple(opt.exp_avg[g].shape)) * 1e-4).astype(np.float32)))
        opt.exp_avg_sq[g].copy_(torch.from_numpy((rng.random(tuple(opt.exp_avg_sq[g].shape)) * 1e-8).astype(np.float32)))
    ctx = raster.RasterContext(N, W, H)
    ctx.set_lean_forward(True)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    M = fwd["num_culled"]
    ctx.backward_render(gi, c["bg"])
    state = dict(dp)
    state.update({"m_" + g: opt.exp_avg[g] for g in opt.names})
    state.update({"v_" + g: opt.exp_avg_sq[g] for g in opt.names})
    state.update(uv_accum=opt.uv_grad_accum, dur=opt.grad_accum_dur)
    start = {k: v.clone() for k, v in state.items()}
    runs = []
    for want in ("sums", "rows"):
        for k, v in state.items():
            v.copy_(start[k])
        g_part = ctx.alloc_gradients(M, L, intermediates=("uv",), factored_sh=True)
        for t in g_part.values():
            if t is not None:
                t.fill_(float("nan"))
        before = ctx.counters()
        ctx.backward_gaussians_adam(dp, dc, L, opt.fused_state(20, mode=1), g_part)
        torch.cuda.synchronize()
        after = ctx.counters()
        moved = (after["dir_sums_backwards"] - before["dir_sums_backwards"], after["dir_sums_fallbacks"] - before["dir_sums_fallbacks"])
        assert moved == ((1, 0) if want == "sums" and L > 0 else (0, 1)), (want, moved)
        out = {k: _np(v).copy() for k, v in state.items()}
        out.update({"g_" + k: _np(v).copy() for k, v in g_part.items() if v is not None})
        runs.append(out)
    a, b = runs
    assert set(a) == set(b)
    changed = 0
    for k in a:
        x, y = a[k].view(np.int32) if a[k].dtype == np.float32 else a[k], b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]
        assert (x == y).all(), k
        if k in start:
            changed += int((_np(start[k]) != a[k]).sum() if a[k].dtype != np.float32 else (_bits(_np(start[k])) != _bits(a[k])).sum())
    assert changed > 0, "the step must have moved something"
    ctx.close()


def test_a_forward_queued_twice_drops_its_sums(gpu, scene):
    """Splats of dozens of tiles: the instances outgrow the room the first forward of a context queued its tail into, and the
    tail is queued again.  Such a forward's backward reads the rows; the next forward's reads the sums again."""
    torch, raster = gpu, pkg("raster")
    N, L, c = 1000, 3, scene.CONFIG
    params = _scene(scene, N, L, False)
    params["scale"] += 2.5
    params["opacity"][:] = -3.0
    dp, dc = raster.device_params(params), raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    assert ctx.counters()["tail_redone"] == 1, ctx.counters()
    ctx.backward_render(gi, c["bg"])
    g_on, g_off, moved = _backward_both(torch, ctx, dp, dc, L, fwd["num_culled"])
    assert moved == dict(dir_sums_backwards=0, dir_sums_fallbacks=2), moved
    _assert_same_bits(g_on, g_off, "queued twice")
    fwd = ctx.rasterize_image(dp, dc, c, c["bg"], L)
    assert ctx.counters()["tail_redone"] == 1
    ctx.backward_render(gi, c["bg"])
    g_on, g_off, moved = _backward_both(torch, ctx, dp, dc, L, fwd["num_culled"])
    assert moved == dict(dir_sums_backwards=1, dir_sums_fallbacks=1), moved
    _assert_same_bits(g_on, g_off, "the forward after")
    ctx.close()

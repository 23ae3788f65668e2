"""GPU tests of the per-gaussian blend-weight statistics (gsplat_context_accumulate_contributions): parity with the numpy
reference evaluated in float64 on the float32 oracle forward (tests/contribution_reference.py), the pixel-sum identity,
accumulation, reproducibility, every kind of forward, occlusion, long lists, the refusals, and the Trainer's scores,
pruning and schedule."""
import ctypes

import numpy as np
import pytest

import antialias_reference as aar
import contribution_reference as cr
import filter3d_reference as f3
from conftest import assert_grad_close, max_pixels_above_tol, max_stop_index_mismatches, pkg

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _oracle(orc, scene, params, cam, L, bg=0.0):
    c = scene.CONFIG
    return orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], bg, L, threads=8)


def _arrays(torch, N):
    return dict(weight_sum=torch.zeros(N, device="cuda"), weight_max=torch.zeros(N, device="cuda"),
                pixels=torch.zeros(N, dtype=torch.int32, device="cuda"))


def _stats(torch, ctx, N):
    a = _arrays(torch, N)
    ctx.accumulate_contributions(**a)
    torch.cuda.synchronize()
    return a


def _reference_global(ref, W, H, N):
    c2g = np.nonzero(np.asarray(ref["mask"]))[0]
    return cr.to_global(cr.contribution_stats(ref, W, H), c2g, N), c2g


def _check_parity(got, want, culled, P, what):
    """got: the three device tensors; want: the reference in global order.  The sums and maxima meet the bar of the
    compositing backward's per-gaussian sums (the same reduction); the pixel counts may differ by the borderline stop and
    1/255 decisions conftest allows the forward, in how many gaussians and in total."""
    s, m, px = _np(got["weight_sum"]), _np(got["weight_max"]), _np(got["pixels"]).astype(np.int64)
    assert (s[culled] == 0).all() and (m[culled] == 0).all() and (px[culled] == 0).all(), f"{what}: a culled row was written"
    diff = np.abs(px - want[2])
    print(f"{what}: weight_sum relative L2 {np.linalg.norm(s - want[0]) / np.linalg.norm(want[0]):.2e}, weight_max "
          f"{np.linalg.norm(m - want[1]) / np.linalg.norm(want[1]):.2e}, pixels differ on {int((diff > 0).sum())} gaussians "
          f"by {int(diff.sum())} in total")
    assert_grad_close(s, want[0], f"{what}: weight_sum")
    assert_grad_close(m, want[1], f"{what}: weight_max")
    allowed = max_stop_index_mismatches(P) + max_pixels_above_tol(P)
    assert int((diff > 0).sum()) <= allowed and int(diff.sum()) <= allowed, f"{what}: pixels"
    assert np.array_equal(px == 0, m == 0)


_REF = {}  # (scene name) -> what the parity tests share: parameters, camera, the oracle forward and the reference, made once


def _shared(scene, orc, name):
    if name not in _REF:
        if name == "partial":  # 70 x 45: partial tiles in both directions
            N, W, H, L = 300, 70, 45, 1
        else:
            N, W, H, L = scene.WORKLOADS[name][:4]
        params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
        ref = _oracle(orc, scene, params, cam, L)
        want, c2g = _reference_global(ref, W, H, N)
        culled = np.ones(N, bool)
        culled[c2g] = False
        _REF[name] = dict(N=N, W=W, H=H, L=L, params=params, cam=cam, ref=ref, want=want, culled=culled)
    return _REF[name]


def _on_device(case):
    raster = pkg("raster")
    return raster, raster.device_params(case["params"]), raster.device_camera(case["cam"])


@pytest.mark.parametrize("name", ["tiny", "small", "partial"])
def test_statistics_match_the_reference(gpu, scene, orc, name):
    torch, case = gpu, _shared(scene, orc, name)
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    for it in range(2):  # the second forward walks the compacted slots
        ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
        _check_parity(_stats(torch, ctx, N), case["want"], case["culled"], W * H, f"{name}, forward {it}")


def test_weight_sums_add_up_to_the_covered_image(gpu, scene, orc):
    """sum_j weight_sum[j] = sum_p (1 - T(p)).  Both sides blend the same weights; the kernel's T follows the forward's
    bit for bit, so what separates them is the rounding of a pixel's chain of at most L additions 1 - T = sum w against
    its product form, each step half an ulp of a number below 1: relative error at most L * 2^-22 (a worst-case linear
    bound, L the scene's longest tile list), plus nothing for the float64 sums on the host."""
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    got = _stats(torch, ctx, N)
    longest = int(np.diff(_np(fwd["ranges"])).max())
    covered = (1.0 - _np(fwd["T"]).astype(np.float64)).sum()
    rel = abs(_np(got["weight_sum"]).astype(np.float64).sum() - covered) / covered
    print(f"small: longest list {longest}, |sum weight_sum - sum (1 - T)| / sum (1 - T) = {rel:.2e} (bound {longest * 2.0 ** -22:.2e})")
    assert longest == 150
    assert rel <= longest * 2.0 ** -22


def test_accumulation_over_calls_views_and_pointers(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    once = _stats(torch, ctx, N)
    twice = {k: v.clone() for k, v in once.items()}
    ctx.accumulate_contributions(**twice)  # two calls on one forward
    assert torch.equal(twice["pixels"], 2 * once["pixels"])
    assert torch.equal(twice["weight_max"], once["weight_max"])
    assert_grad_close(_np(twice["weight_sum"]), 2.0 * _np(once["weight_sum"]).astype(np.float64), "two calls", rel=1e-6)
    # each pointer alone
    for k in ("weight_sum", "weight_max", "pixels"):
        alone = _arrays(torch, N)[k]
        ctx.accumulate_contributions(**{k: alone})
        if k == "weight_sum":
            assert_grad_close(_np(alone), _np(once[k]), "weight_sum alone", rel=1e-6)
        else:
            assert torch.equal(alone, once[k]), k
    # views 0 and 1 into the same arrays
    cam1 = raster.device_camera(scene.make_camera(W, H, 1))
    both = {k: v.clone() for k, v in once.items()}
    ctx.rasterize_image(dp, cam1, scene.CONFIG, 0.0, L)
    one = _stats(torch, ctx, N)
    ctx.accumulate_contributions(**both)
    torch.cuda.synchronize()
    assert not torch.equal(one["pixels"], once["pixels"])
    assert torch.equal(both["pixels"], once["pixels"] + one["pixels"])
    assert torch.equal(both["weight_max"], torch.maximum(once["weight_max"], one["weight_max"]))
    assert_grad_close(_np(both["weight_sum"]), _np(once["weight_sum"]).astype(np.float64) + _np(one["weight_sum"]),
                      "two views", rel=1e-6)


def test_pixels_and_weight_max_carry_the_same_bits_in_every_run_and_route(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    ctx = raster.RasterContext(N, W, H)
    ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
    first = _stats(torch, ctx, N)
    for _ in range(2):
        again = _stats(torch, ctx, N)
        assert torch.equal(again["pixels"], first["pixels"]) and torch.equal(again["weight_max"], first["weight_max"])
    for route in (1, 2):
        other = raster.RasterContext(N, W, H)
        other.set_binning_route(route)
        other.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
        got = _stats(torch, other, N)
        assert torch.equal(got["pixels"], first["pixels"]) and torch.equal(got["weight_max"], first["weight_max"]), route


def test_every_kind_of_forward_serves_it(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    c = scene.CONFIG
    plain = raster.RasterContext(N, W, H)
    fwd = plain.rasterize_image(dp, dc, c, 0.0, L)
    want = _stats(torch, plain, N)
    _check_parity(want, case["want"], case["culled"], W * H, "plain")
    # after the backward of that forward (it only reads the records)
    grads = plain.alloc_gradients(fwd["num_culled"], L)
    plain.backward_pass(dp, dc, torch.as_tensor(scene.make_grad_image(W, H)).cuda(), 0.0, L, grads)
    got = _stats(torch, plain, N)
    assert torch.equal(got["pixels"], want["pixels"]) and torch.equal(got["weight_max"], want["weight_max"])
    for kind in ("lean", "render_only", "depth"):
        ctx = raster.RasterContext(N, W, H)
        {"lean": ctx.set_lean_forward, "render_only": ctx.set_render_only, "depth": ctx.set_depth}[kind](True)
        ctx.rasterize_image(dp, dc, c, 0.0, L)
        got = _stats(torch, ctx, N)
        assert torch.equal(got["pixels"], want["pixels"]) and torch.equal(got["weight_max"], want["weight_max"]), kind
        assert_grad_close(_np(got["weight_sum"]), _np(want["weight_sum"]), kind, rel=1e-6)


def test_antialiased_and_filtered_forwards_weigh_the_effective_opacity(gpu, scene, orc):
    torch, case = gpu, _shared(scene, orc, "small")
    raster, dp, dc = _on_device(case)
    N, W, H, L = case["N"], case["W"], case["H"], case["L"]
    c = scene.CONFIG
    # anti-aliased: the oracle forward with logit(sigmoid(logit) * rho) composited
    _, aa = aar.forward(orc, case["params"], case["cam"], c, 0.0, L, threads=8)
    want, c2g = _reference_global(aa, W, H, N)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_antialiased(True)
    ctx.rasterize_image(dp, dc, c, 0.0, L)
    _check_parity(_stats(torch, ctx, N), want, case["culled"], W * H, "antialiased")
    assert np.linalg.norm(want[0] - case["want"][0]) > 5e-3 * np.linalg.norm(case["want"][0]), "rho changes nothing here"
    # 3D filter with a random f: the oracle forward of the filtered scale and opacity
    f = np.exp(np.random.default_rng(5).uniform(-1.0, 1.0, N) + case["params"]["scale"].mean(1)).astype(np.float32)
    scale_eff, op_eff, _, _ = f3.apply(case["params"]["scale"], case["params"]["opacity"], f)
    filtered = dict(case["params"], scale=scale_eff.astype(np.float32), opacity=op_eff.astype(np.float32))
    ref = _oracle(orc, scene, filtered, case["cam"], L)
    want3, c2g3 = _reference_global(ref, W, H, N)
    culled3 = np.ones(N, bool)
    culled3[c2g3] = False
    ctx = raster.RasterContext(N, W, H)
    ctx.set_filter3d(torch.as_tensor(f).cuda())
    ctx.rasterize_image(dp, dc, c, 0.0, L)
    _check_parity(_stats(torch, ctx, N), want3, culled3, W * H, "filter3d")
    assert np.linalg.norm(want3[0] - case["want"][0]) > 1e-2 * np.linalg.norm(case["want"][0]), "the filter changes nothing here"


def _occlusion_scene(scene):
    """64 x 64: six large opaque gaussians (logit 20), nearest first, in front of 100 small ones.  The walls' centres lie
    left of the image, so that their alpha stays below the 0.99 cap on every pixel (a capped wall leaves T = 0.01, then
    0.01^2 against the 1e-4 stop test: a borderline decision on every pixel at once)."""
    W = H = 64
    N, walls = 106, 6
    p = scene.make_gaussians(N, W, H, 0)
    cam = scene.make_camera(W, H, 0)
    p["xyz"][walls:, 2] += 4.0
    for k in range(walls):
        z = 1.0 + 0.1 * k
        p["xyz"][k] = ((-80.0 - W / 2) * z / cam["fx"], 0.0, z)
        p["scale"][k] = np.log(8.0)
        p["quaternion"][k] = (1.0, 0.0, 0.0, 0.0)
        p["opacity"][k] = 20.0
    return N, W, H, walls, p, cam


def test_occluded_gaussians_get_nothing(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    N, W, H, walls, params, cam = _occlusion_scene(scene)
    ref = _oracle(orc, scene, params, cam, 0)
    # on the oracle first: every visible gaussian is on a list, every pixel stops inside the wall layers
    n = np.asarray(ref["n"])
    assert ref["num_culled"] == N and len(np.unique(ref["sorted"])) == N
    assert n.min() >= 2 and n.max() < walls, (n.min(), n.max())
    stop = int(n.max())
    want, c2g = _reference_global(ref, W, H, N)
    assert (want[2][:stop] > 0).all() and (want[2][stop:] == 0).all()
    ctx = raster.RasterContext(N, W, H)
    fwd = ctx.rasterize_image(raster.device_params(params), raster.device_camera(cam), scene.CONFIG, 0.0, 0)
    assert int(fwd["n"].max()) == stop
    got = _stats(torch, ctx, N)
    for k in ("weight_sum", "weight_max", "pixels"):
        assert bool((got[k][stop:] == 0).all()), k  # the wall layers behind the stop and the hidden hundred
    _check_parity(got, want, np.zeros(N, bool), W * H, "occlusion")


def _long_list_scene(scene):
    """32 x 32: 2200 tiny, mostly faint gaussians stacked over the first tile's middle: a list of ~2400 entries whose
    outer pixels never stop (n = the list's length) while the middle saturates early."""
    W = H = 32
    N, L = 2600, 0
    p = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, 0)
    rng = np.random.default_rng(11)
    lo, hi = 200, 2400
    k = hi - lo
    z = rng.uniform(3.0, 9.0, k)
    u, v = 9.0 + rng.uniform(-5, 5, k), 9.0 + rng.uniform(-5, 5, k)
    p["xyz"][lo:hi, 0] = (u - W / 2) * z / cam["fx"]
    p["xyz"][lo:hi, 1] = (v - H / 2) * z / cam["fy"]
    p["xyz"][lo:hi, 2] = z
    p["scale"][lo:hi] = np.log(rng.uniform(0.004, 0.012, (k, 3)))
    p["opacity"][lo:hi] = rng.choice([-5.0, -4.0, -3.0, -1.0, 3.0], size=k, p=[0.45, 0.3, 0.15, 0.08, 0.02])
    return N, W, H, L, p, cam


def test_long_lists_are_walked_whole(gpu, scene, orc):
    torch, raster = gpu, pkg("raster")
    N, W, H, L, params, cam = _long_list_scene(scene)
    ref = _oracle(orc, scene, params, cam, L)
    # on the oracle first: a list beyond the forward's segment threshold, and pixels that walk beyond it
    assert int(np.diff(ref["ranges"]).max()) > 1488 and int(np.asarray(ref["n"]).max()) > 1488
    assert int((np.asarray(ref["n"])[:16, :16] < ref["ranges"][1]).sum()) > 0  # ... and pixels that stop early
    want, c2g = _reference_global(ref, W, H, N)
    culled = np.ones(N, bool)
    culled[c2g] = False
    dp, dc = raster.device_params(params), raster.device_camera(cam)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_binning_route(1)
    ctx.set_segment_options(gate=0.0)
    for it in range(5):  # (the forward's own split follows the figures of the forward two back)
        ctx.rasterize_image(dp, dc, scene.CONFIG, 0.0, L)
        if it in (0, 4):
            _check_parity(_stats(torch, ctx, N), want, culled, W * H, f"long list, forward {it}")
    assert ctx.counters()["segmented_forwards"] > 0, ctx.counters()


def test_refusals_launch_nothing(gpu, scene):
    torch, lib, raster = gpu, pkg("_lib"), pkg("raster")
    N, W, H, L = scene.WORKLOADS["tiny"][:4]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_gaussians(N, W, H, L))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    a = dict(weight_sum=torch.full((N,), 7.0, device="cuda"), weight_max=torch.full((N,), 7.0, device="cuda"),
             pixels=torch.full((N,), 7, dtype=torch.int32, device="cuda"))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in a.items()}

    def refused(ctx, n=N, ptrs=None):
        ptrs = p if ptrs is None else ptrs
        rc = ctx._lib.gsplat_context_accumulate_contributions(ctx._h, n, ptrs["weight_sum"], ptrs["weight_max"],
                                                              ptrs["pixels"], st)
        assert rc == -3, rc  # GSPLAT_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert all(bool((v == 7).all()) for v in a.values())

    ctx = raster.RasterContext(N, W, H)
    refused(ctx)                                     # no forward yet
    with pytest.raises(lib.GsplatError):
        ctx.accumulate_contributions(**a)
    fwd = ctx.rasterize_image(dp, dc, c, 0.0, L)
    refused(ctx, n=N - 1)                            # not the recorded forward's N
    refused(ctx, ptrs=dict(weight_sum=None, weight_max=None, pixels=None))  # nothing asked for
    with pytest.raises(lib.GsplatError):
        ctx.accumulate_contributions()
    with pytest.raises(lib.GsplatError):
        ctx.accumulate_contributions(weight_sum=a["weight_sum"][: N - 1].contiguous())
    check = pkg("_lib").check
    owned = [fwd[k].data_ptr() for k in ("mask", "uv_all", "xyz_c_all", "sigma", "conic", "J", "rgb", "radius", "sorted",
                                         "ranges", "image", "T", "n")]
    check(ctx._lib.gsplat_context_detach_forward_outputs(ctx._h))
    refused(ctx)                                     # the forward's arrays are the caller's now
    for ptr in owned:                                # ... who returns them to the pool
        check(ctx._lib.gsplat_pool_free(ctypes.c_void_p(ptr)))
    behind = dp["xyz"].clone()
    behind[:, 2] = -behind[:, 2].abs() - 1.0
    fresh = raster.RasterContext(N, W, H)
    fresh.rasterize_image(dp, dc, c, 0.0, L)
    with pytest.raises(lib.GsplatError) as e:
        fresh.rasterize_image(dict(dp, xyz=behind), dc, c, 0.0, L)
    assert e.value.code == -5
    refused(fresh)                                   # the last forward saw nothing
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in a.values())
    # wrong dtype or shape never reach the library
    ok = raster.RasterContext(N, W, H)
    ok.rasterize_image(dp, dc, c, 0.0, L)
    for bad in (dict(weight_sum=torch.zeros(N, dtype=torch.float64, device="cuda")),
                dict(pixels=torch.zeros(N, device="cuda")), dict(weight_max=torch.zeros(N, dtype=torch.int32, device="cuda")),
                dict(weight_sum=torch.zeros(N, 1, device="cuda")), dict(weight_max=torch.zeros(2 * N, device="cuda")[::2]),
                dict(pixels=torch.zeros(N, dtype=torch.int32)), dict(weight_sum=np.zeros(N, np.float32)),
                dict(weight_sum=torch.zeros(N, device="cuda"), pixels=torch.zeros(N + 1, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            ok.accumulate_contributions(**bad)


# ---------------------------------------------------------------- Trainer
def _training_setup(torch, scene, n_views=4, faint=50):
    """The 3000-gaussian 160 x 96 generated training scene of tests/test_absgrad_gpu.py, built the same way, with `faint`
    gaussians of logit -8 appended: their sigmoid, 3.4e-4, is below 1/255, so nothing ever composites them."""
    raster, ops = pkg("raster"), pkg("ops")
    N, W, H = 3000, 160, 96
    truth = scene.make_gaussians(N, W, H, 0)
    truth["opacity"][:] = np.clip(truth["opacity"], 0.5, 3.0)
    ctx = raster.RasterContext(N, W, H)
    dpt = raster.device_params(truth)
    views = []
    for v in range(n_views):
        cam = raster.device_camera(scene.make_camera(W, H, v))
        views.append((cam, ctx.rasterize_image(dpt, cam, scene.CONFIG, 0.0, 0)["image"].clone()))
    idx = np.random.default_rng(2).choice(N, N // 3, replace=False)
    pts = torch.from_numpy(truth["xyz"][idx].astype(np.float64)).cuda()
    col = torch.from_numpy(np.clip((truth["rgb"][idx] * 0.28209479 + 0.5) * 255, 0, 255).astype(np.uint8)).cuda()
    init = ops.initialize_gaussians(pts, col)
    torch.cuda.synchronize()
    if faint:
        init = {k: torch.cat([v, v[:faint].clone()], 0).contiguous() for k, v in init.items() if v is not None}
        init["opacity"][-faint:] = -8.0
    cfg = dict(num_iters=36, add_sh_band_interval=12, max_sh_band=2, adaptive_control_start=10 ** 9,
               reset_opacity_start=10 ** 9, uv_grad_threshold=2e-5, max_gaussians=20000, use_background=False)
    return init, views, cfg


def _renders(t):
    out = []
    t.ctx.set_render_only(True)
    for cam, _ in t.views:
        out.append(t.ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)["image"].clone())
    t.ctx.set_render_only(False)
    return out


def test_trainer_scores_and_prune_of_the_never_composited(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    t.train(13, loss_every=0)  # (an SH band is added at iteration 12: the colour rows are compacted as well)
    assert t.l_max == 1 and "sh" in t.opt.names
    n = t.num_gaussians
    scores = t.contribution_scores()
    assert scores["pixels"].dtype == torch.int32 and all(v.shape == (n,) for v in scores.values())
    assert bool((scores["pixels"][-50:] == 0).all()) and bool((scores["weight_max"][-50:] == 0).all())
    again = t.contribution_scores(t.views)
    assert torch.equal(again["pixels"], scores["pixels"]) and torch.equal(again["weight_max"], scores["weight_max"])
    gone = scores["pixels"] == 0
    assert 50 <= int(gone.sum()) < n
    # mark the rows: moments and statistics of the survivors must follow them
    t.opt.uv_grad_accum.copy_(torch.arange(n, device="cuda", dtype=torch.float32))
    t.opt.grad_accum_dur.copy_(torch.arange(n, device="cuda", dtype=torch.int32))
    for g in t.opt.names:
        rows = torch.arange(n, device="cuda", dtype=torch.float32).reshape((n,) + (1,) * (t.opt.exp_avg[g].dim() - 1))
        t.opt.exp_avg[g].copy_(rows.expand_as(t.opt.exp_avg[g]) + 0.25)
        t.opt.exp_avg_sq[g].copy_(rows.expand_as(t.opt.exp_avg_sq[g]) + 0.5)
    before = {k: v.clone() for k, v in t.params.items()}
    images = _renders(t)
    removed = t.prune_by_contribution(0.0)
    assert removed == int(gone.sum()) and t.num_gaussians == n - removed
    keep = ~gone
    ids = torch.arange(n, device="cuda")[keep]
    for k, v in before.items():
        assert torch.equal(t.params[k], v[keep]), k
    assert torch.equal(t.opt.uv_grad_accum, ids.float()) and torch.equal(t.opt.grad_accum_dur, ids.int())
    for g in t.opt.names:
        assert t.opt.exp_avg[g].shape == t.params[g].shape
        assert torch.equal(t.opt.exp_avg[g].reshape(len(ids), -1)[:, 0], ids.float() + 0.25), g
        assert torch.equal(t.opt.exp_avg_sq[g].reshape(len(ids), -1)[:, -1], ids.float() + 0.5), g
    # no list exceeds 1488 entries, so every pixel's summation order is fixed, and a removed entry only ever contributed
    # fma(c, 0, acc): the render of every training view keeps its bits
    for k, (a, b) in enumerate(zip(images, _renders(t))):
        assert torch.equal(a, b), f"view {k}: max difference {float((a - b).abs().max()):.2e}"
    assert t.prune_by_contribution(0.0) == 0  # nothing left to remove
    t.train(2, loss_every=0)                  # the loop goes on with the compacted state
    assert all(bool(torch.isfinite(v).all()) for v in t.params.values())


def test_trainer_prune_at_the_default_threshold(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = _training_setup(torch, scene)
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    t.train(20, loss_every=0)
    n = t.num_gaussians
    scores = t.contribution_scores()
    want = int(((scores["weight_max"] < 0.01) | (scores["pixels"] == 0)).sum())
    psnr0 = t.evaluate()
    removed = t.prune_by_contribution()
    psnr1 = t.evaluate()
    print(f"default threshold: removed {removed} of {n} gaussians, evaluate() {psnr0:.3f} dB -> {psnr1:.3f} dB")
    assert removed == want and 50 <= removed < n and t.num_gaussians == n - removed
    given = dict(weight_sum=None, weight_max=torch.zeros(t.num_gaussians, device="cuda"),
                 pixels=torch.ones(t.num_gaussians, dtype=torch.int32, device="cuda"))
    assert t.prune_by_contribution(scores=given) == 0 and t.num_gaussians == n - removed  # never everything


def test_trainer_schedule(gpu, scene, monkeypatch):
    """With adaptive_control_end=20 and prune_contribution_interval=10, 31 iterations prune at iterations 20 and 30.  With
    the key off nothing in the loop changes: none of the new code runs (its three entry points are replaced by functions
    that raise), the gaussian count stays, and maintenance() at the pruning iterations leaves every tensor where it is.

    The parameters of that run cannot be held against a second run's, bit for bit or at any bar derived from the
    number format: the compositing backward adds a gaussian's tiles into its gradient row with float atomics, in arrival
    order, so two trainings run apart differ whatever their configuration (tests/test_absgrad_gpu.py measures it on this
    scene), and Adam's normalised step turns a last-bit difference of a small gradient into up to a learning rate per
    iteration.  Measured on an MI355X after 31 iterations, largest absolute difference per group, in two sessions: two runs
    WITHOUT the new keys 5e-7 (xyz) to 8e-5 (opacity) and 2e-7 (sh) to 2e-5 (scale); key off against no keys 3e-7 (sh) to
    1.3e-4 (quaternion) and 4e-6 (xyz) to 5.7e-4 (opacity).  Both pairs are printed; what is asserted is what is exact."""
    torch, trainer_mod, raster = gpu, pkg("trainer"), pkg("raster")
    init, views, cfg = _training_setup(torch, scene)
    sched = dict(cfg, adaptive_control_end=20, prune_contribution_interval=10)

    def run(config):
        t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, config, scene_extent=5.0, seed=3)
        t.train(31, loss_every=0)
        torch.cuda.synchronize()
        return t

    on = run(dict(sched, prune_contribution=True))
    assert [it for it, _ in on.contribution_prunes] == [20, 30], on.contribution_prunes
    assert on.contribution_prunes[0][1] >= 50 and on.num_gaussians == len(init["xyz"]) - sum(r for _, r in on.contribution_prunes)
    bare, bare2 = run(dict(cfg, adaptive_control_end=20)), run(dict(cfg, adaptive_control_end=20))

    def never(*a, **k):
        raise AssertionError("the contribution code ran with prune_contribution off")

    monkeypatch.setattr(trainer_mod.Trainer, "contribution_scores", never)
    monkeypatch.setattr(trainer_mod.Trainer, "prune_by_contribution", never)
    monkeypatch.setattr(raster.RasterContext, "accumulate_contributions", never)
    off = run(dict(sched, prune_contribution=False))
    assert off.contribution_prunes == [] and bare.contribution_prunes == []
    assert off.num_gaussians == bare.num_gaussians == len(init["xyz"])
    held = {k: v for k, v in off.params.items()}
    for it in (21, 31):  # maintenance() at the iterations that prune when the key is on: nothing moves
        off.iter = it
        off.maintenance()
        assert all(off.params[k] is v for k, v in held.items())
    for k in off.params:
        if off.params[k].numel():
            d = float((off.params[k] - bare.params[k]).abs().max()), float((bare2.params[k] - bare.params[k]).abs().max())
            print(f"{k}: key off against no new keys differ by at most {d[0]:.2e}, two runs without the keys by {d[1]:.2e}")


def test_two_ranks_prune_to_identical_replicas(gpu, scene):
    torch, trainer_mod, gdist = gpu, pkg("trainer"), pkg("dist")
    init, views, cfg = _training_setup(torch, scene)

    def body(comm):
        mine = {k: v.clone() for k, v in init.items()}
        t = trainer_mod.Trainer(mine, views, cfg, scene_extent=5.0, seed=3, exchange="split", comm=comm)
        t.train(6, loss_every=0)
        removed = t.prune_by_contribution()
        t.train(2, loss_every=0)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy().copy() for k, v in t.params.items()}
        out["removed"] = np.array([removed, t.num_gaussians])
        comm.barrier()
        return out

    r = gdist.ThreadGroup(2).run(body)
    assert r[0]["removed"][0] >= 50
    for k in r[0]:
        assert np.array_equal(r[0][k], r[1][k]), k

"""GPU tests of the MCMC densification (config key mcmc): the four kernels of gs_density.hip against the float64 reference
(tests/mcmc_reference.py), the Trainer mode, and what a relocation does to the rendered image."""
import math

import numpy as np
import pytest

import mcmc_reference as ref
from conftest import MEAN_L1_TOL, PIXEL_L1_TOL, pkg

pytestmark = pytest.mark.gpu

MIN_OPACITY = 0.005


def _np(t):
    return t.detach().cpu().numpy()


def _logit(p):
    return math.log(p) - math.log1p(-p)


# ---------------------------------------------------------------------------------------------------- sampling
def test_sampling_matches_the_reference_bit_for_bit(gpu):
    torch, ops = gpu, pkg("ops")
    rng = np.random.default_rng(5)
    N, K, seed = 1000, 4096, 2 ** 40 + 12345
    # multiples of 2^-20: every partial sum is exact in float64, so the device's scan and numpy's running sum agree
    w = (rng.integers(1, 2 ** 20, N) / 2.0 ** 20).astype(np.float32)
    zero = rng.random(N) < 0.3
    zero[[0, N - 1]] = True
    w[zero] = 0.0
    want_s, want_c = ref.sample_by_weight(w, K, seed)
    wd = torch.as_tensor(w).cuda()
    samples, counts = ops.sample_by_weight(wd, K, seed)
    assert samples.dtype == torch.int32 and counts.dtype == torch.int32
    assert np.array_equal(_np(samples), want_s)
    assert np.array_equal(_np(counts), want_c) and np.array_equal(want_c, np.bincount(want_s, minlength=N))
    assert not zero[_np(samples)].any()
    again, counts2 = ops.sample_by_weight(wd, K, seed, counts=counts)  # the same seed, into the uncleared counts
    assert counts2 is counts
    assert torch.equal(again, samples) and np.array_equal(_np(counts), 2 * want_c)
    other, _ = ops.sample_by_weight(wd, K, seed + 1)
    assert not torch.equal(other, samples)


def test_sampling_one_row_and_nothing_to_draw(gpu):
    torch, ops = gpu, pkg("ops")
    samples, counts = ops.sample_by_weight(torch.full((1,), 0.25, device="cuda"), 5, 9)
    assert _np(samples).tolist() == [0] * 5 and _np(counts).tolist() == [5]
    samples, counts = ops.sample_by_weight(torch.ones(7, device="cuda"), 0, 9)
    assert samples.numel() == 0 and _np(counts).tolist() == [0] * 7
    # a total that is not positive is refused on the device: nothing is written
    lib, st = pkg("_lib").load(), None
    cdf = torch.zeros(4, dtype=torch.float64, device="cuda")
    s, c = torch.full((8,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -7, dtype=torch.int32, device="cuda")
    assert lib.gsplat_sample_by_weight(cdf.data_ptr(), 4, 8, 1, s.data_ptr(), c.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((s == -7).all()) and bool((c == -7).all())
    with pytest.raises(ValueError):
        ops.sample_by_weight(torch.zeros(4, device="cuda"), 8, 1)


# ---------------------------------------------------------------------------------------------------- relocation
GRID_LOGITS = [_logit(0.005), _logit(0.02), 0.0, _logit(0.9), _logit(0.99), 13.8, 20.0]
GRID_COUNTS = [0, 1, 2, 9, 50, 51, 200]
GRID_SCALES = (-3.0, 0.5, 2.0)


def test_relocation_grid(gpu):
    """Every (logit, count) pair of the grid, each row with three different log-scales, against the float64 reference to
    1e-5 absolute: the kernel's arithmetic is double, so what is left is the final rounding to float32 (magnitudes below
    16: an ulp is 1e-6) and the device's double exp / log.

    A written row has n = count + 1 >= 2 copies, and then o' = 1 - (1 - o)^(1/n) reaches the upper clamp 1 - 2^-23 only
    when o is 1 in double (logit 20 gives o' = 1 - 4.5e-5 at n = 2); the lower clamp is inside the grid (o = 0.005,
    n = 51).  One row outside the grid, logit 40 with count 1, lands on the upper clamp."""
    torch, ops = gpu, pkg("ops")
    logits = np.array([l for l in GRID_LOGITS for _ in GRID_COUNTS] + [40.0], np.float32)
    counts = np.array([c for _ in GRID_LOGITS for c in GRID_COUNTS] + [1], np.int32)
    scales = np.tile(np.array(GRID_SCALES, np.float32), (len(logits), 1))
    want_l, want_s = ref.relocate(logits, scales, counts, np.float32(MIN_OPACITY))
    op, sc = torch.as_tensor(logits).cuda(), torch.as_tensor(scales).cuda()
    ops.mcmc_relocate(op, sc, torch.as_tensor(counts).cuda(), MIN_OPACITY)
    got_l, got_s = _np(op), _np(sc)
    still = counts == 0
    assert np.array_equal(got_l[still].view(np.uint32), logits[still].view(np.uint32))
    assert np.array_equal(got_s[still].view(np.uint32), scales[still].view(np.uint32))
    err_l, err_s = np.abs(got_l - want_l)[~still].max(), np.abs(got_s - want_s)[~still].max()
    print(f"relocation grid: largest error logit {err_l:.2e}, log-scale {err_s:.2e}")
    assert np.abs(want_l[~still]).max() < 16 and np.abs(want_s).max() < 16
    assert err_l <= 1e-5 and err_s <= 1e-5
    row = lambda l, c: GRID_LOGITS.index(l) * len(GRID_COUNTS) + GRID_COUNTS.index(c)
    lo = np.float32(_logit(float(np.float32(MIN_OPACITY))))
    assert abs(got_l[row(GRID_LOGITS[0], 50)] - lo) <= 1e-5 and abs(want_l[row(GRID_LOGITS[0], 50)] - lo) <= 1e-5
    hi = _logit(ref.FLT_ONE_MINUS_EPS)
    assert abs(got_l[-1] - hi) <= 1e-5 and abs(want_l[-1] - hi) <= 1e-5
    for l in GRID_LOGITS:  # the cap: 50 (n = 51), 51 and 200 draws give the same bits
        a, b, c = row(l, 50), row(l, 51), row(l, 200)
        assert got_l[a] == got_l[b] == got_l[c] and np.array_equal(got_s[a], got_s[b]) and np.array_equal(got_s[b], got_s[c])
    assert (got_s[~still] < scales[~still]).all()  # every copy is smaller than its source


# ---------------------------------------------------------------------------------------------------- position noise
def _noise_case():
    rng = np.random.default_rng(17)
    N = 4096 + 37
    quat = rng.normal(size=(N, 4)).astype(np.float32) * rng.uniform(0.2, 5.0, (N, 1)).astype(np.float32)
    scale = rng.uniform(-4.0, 0.0, (N, 3)).astype(np.float32)
    # o from 0.001 to 0.9: 3000 rows spread over 0.001 .. 0.7 in the logit, 500 at 0.9 (the gate is closed: expf
    # overflows), the rest in between (see test_noise_matches_the_reference)
    logit = np.concatenate([np.linspace(_logit(0.001), _logit(0.7), 3000), np.full(500, _logit(0.9)),
                            np.linspace(_logit(0.7), _logit(0.9), N - 3500 + 2)[1:-1]]).astype(np.float32)
    band = np.arange(N) >= 3500
    perm = rng.permutation(N)
    return N, quat, scale, logit[perm], band[perm]


def test_noise_matches_the_reference(gpu):
    """|delta - delta_ref| <= 1e-4 * 5.77 * g * scaler * sum_b |Sigma_ab| per component, 5.77 being the largest normal the
    generator emits: 1e-4 of the largest displacement the row could have had.  The positions start at zero, so that the
    stored result IS the displacement (added to a position of magnitude 1 it would be rounded to that position's ulp,
    6e-8, which says nothing about the kernel).

    Rows with 0.7 < o < 0.9 displace by less than 1e-36 and towards o = 0.89 by less than float32's smallest normal number,
    1.2e-38, where results are multiples of 2^-149 and no float32 arithmetic has four digits.  The bound above is
    asserted as it stands on the rows with o <= 0.7 and on those at 0.9, where the gate is exactly 0; the rows in
    between are held to the same bound plus eight steps of 2^-149 (three products, two sums, the scaling)."""
    torch, ops = gpu, pkg("ops")
    N, quat, scale, logit, band = _noise_case()
    scaler, seed = 0.01, 777
    want, g, row_abs = ref.noise(logit, scale, quat, scaler, seed)
    o = 1.0 / (1.0 + np.exp(-logit.astype(np.float64)))
    assert o.min() < 0.00101 and o.max() > 0.899
    # no row sits on expf's overflow threshold (float32 knows 100 (o - 0.005) to 2e-5 there)
    assert (np.abs(100.0 * (o - 0.005) - ref.LOG_FLT_MAX) > 1e-3).all()
    d = {k: torch.as_tensor(v).cuda() for k, v in dict(opacity=logit, scale=scale, quaternion=quat).items()}

    def run(xyz0, scaler, seed):
        xyz = torch.as_tensor(xyz0).cuda()
        ops.mcmc_add_noise(xyz, d["opacity"], d["scale"], d["quaternion"], scaler, seed)
        return _np(xyz)

    zeros = np.zeros((N, 3), np.float32)
    got = run(zeros, scaler, seed)
    bound = 1e-4 * ref.NORMAL_MAX * g[:, None] * scaler * row_abs
    err = np.abs(got.astype(np.float64) - want)
    main = ~band
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    print(f"noise: largest error / bound on the {int(main.sum())} asserted rows {ratio[main].max():.3f}, "
          f"on the {int(band.sum())} rows in the band {ratio[band].max():.3f}; largest displacement {np.abs(got).max():.2e}")
    assert np.isfinite(got).all() and np.abs(got).max() > 1e-6
    assert (err[main] <= bound[main]).all()
    assert (got[g == 0] == 0).all() and (g[main] == 0).sum() == 500
    assert (err[band] <= bound[band] + 8 * 2.0 ** -149).all()
    closed = logit > 0  # the gate closes: nothing that could be seen
    assert (np.abs(got[closed]) < 1e-8 * scaler * row_abs[closed]).all()
    # the same seed: the same bits; another seed: other bits
    assert np.array_equal(run(zeros, scaler, seed).view(np.uint32), got.view(np.uint32))
    moved = np.abs(got).max(1) > 0
    assert (run(zeros, scaler, seed + 1)[moved] != got[moved]).any(1).mean() > 0.99
    # += : on positions that are not zero the result is the float32 sum of the position and the same displacement; a row
    # whose gate is exactly 0 is not written (its -0.0 stays -0.0)
    xyz0 = np.random.default_rng(3).normal(size=(N, 3)).astype(np.float32)
    xyz0[::7] = -0.0
    summed = np.where((g == 0)[:, None], xyz0, xyz0 + got)
    assert np.array_equal(run(xyz0, scaler, seed).view(np.uint32), summed.view(np.uint32))
    assert np.array_equal(run(xyz0, 0.0, seed).view(np.uint32), xyz0.view(np.uint32))  # scaler 0: not a bit changes


# ---------------------------------------------------------------------------------------------------- regulariser
def test_regulariser_adds_to_the_visible_rows(gpu):
    torch, ops = gpu, pkg("ops")
    rng = np.random.default_rng(23)
    N, M, room = 1000, 300, 340
    c2g = np.sort(rng.choice(N, M, replace=False)).astype(np.int32)
    logit = rng.uniform(-6.0, 6.0, N).astype(np.float32)
    scale = rng.uniform(-4.0, 1.0, (N, 3)).astype(np.float32)
    g_o, g_s = rng.normal(size=room).astype(np.float32), rng.normal(size=(room, 3)).astype(np.float32)
    w_o, w_s = 2.0, 0.5
    add_o, add_s = ref.regularize(c2g, logit, scale, np.float32(w_o), np.float32(w_s))
    want_o, want_s = g_o[:M].astype(np.float64) + add_o, g_s[:M].astype(np.float64) + add_s
    t_o, t_s = torch.as_tensor(g_o).cuda(), torch.as_tensor(g_s).cuda()
    ops.mcmc_regularize(torch.as_tensor(c2g).cuda(), torch.as_tensor(logit).cuda(), torch.as_tensor(scale).cuda(), w_o, w_s,
                        t_o, t_s, M=M)
    got_o, got_s = _np(t_o), _np(t_s)
    for got, want, what in ((got_o[:M], want_o, "opacity"), (got_s[:M], want_s, "scale")):
        err = np.abs(got - want)
        tol = 1e-6 * np.abs(want) + 1e-6 * np.abs(want).mean()
        print(f"regulariser, {what}: largest error / tolerance {(err / tol).max():.3f}")
        assert (err <= tol).all(), what
    assert np.abs(add_o).mean() > 0.05 and np.abs(add_s).mean() > 0.05  # the additions are no rounding matter
    assert np.array_equal(got_o[M:].view(np.uint32), g_o[M:].view(np.uint32))
    assert np.array_equal(got_s[M:].view(np.uint32), g_s[M:].view(np.uint32))


# ---------------------------------------------------------------------------------------------------- Trainer
def _training_setup(torch, scene, n_views=4):
    """The generated training scene of tests/test_absgrad_gpu.py: 3000 gaussians rendered into four 160x96 views, a third
    of their centres as the initial point cloud."""
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
    cfg = dict(mcmc=True, adaptive_control_start=4, adaptive_control_interval=5, adaptive_control_end=40, max_gaussians=1300,
               add_sh_band_interval=12, max_sh_band=2, use_background=False)
    return init, views, cfg


@pytest.fixture(scope="module")
def training(gpu, scene):
    return _training_setup(gpu, scene)


def _moments(t):
    return [m[g] for m in (t.opt.exp_avg, t.opt.exp_avg_sq) for g in t.opt.names]


def test_trainer_grows_to_the_cap(gpu, scene, training, monkeypatch):
    torch, trainer_mod = gpu, pkg("trainer")
    init, views, cfg = training
    assert init["xyz"].shape[0] == 1000

    def never(*a, **k):
        raise AssertionError("clone / split / prune or the opacity reset ran with mcmc on")

    monkeypatch.setattr(trainer_mod.Trainer, "reset_opacity", never)
    monkeypatch.setattr(trainer_mod.Trainer, "adaptive_density_step", never)
    grow = trainer_mod.Trainer.mcmc_grow
    grown = []

    def checked_grow(self, seed=None):  # straight after the growth (the Morton re-order follows): the new rows' moments
        before = self.num_gaussians
        added = grow(self, seed)
        assert self.num_gaussians == before + added
        for m in _moments(self):
            assert m.shape[0] == before + added and not bool(m[before:].any())
        grown.append(added)
        return added

    monkeypatch.setattr(trainer_mod.Trainer, "mcmc_grow", checked_grow)
    monkeypatch.setenv("GSPLAT_FUSED_ADAM", "1")  # the mode overrides it
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    assert t.fused_adam == 0
    history = t.train(45, loss_every=1)
    torch.cuda.synchronize()
    # the schedule: refinement after iterations 5, 10, .. 35, each adding what the pure function says
    n, want_steps, count_after = 1000, [], {}
    for it in range(5, 40, 5):
        add = trainer_mod.mcmc_growth(n, 1.05, 1300)
        want_steps.append((it, add))
        n += add
        count_after[it] = n
    assert [s[0] for s in t.mcmc_steps] == [s[0] for s in want_steps]
    assert [s[2] for s in t.mcmc_steps] == [s[1] for s in want_steps] == grown
    assert [n for n in count_after.values()] == [1050, 1102, 1157, 1214, 1274, 1300, 1300]
    assert len(history) == 45
    for iteration, _, count in history:  # (history carries iteration index + 1 and the count after its maintenance)
        done = [v for it, v in count_after.items() if it <= iteration - 1]
        assert count == (done[-1] if done else 1000) and count <= 1300
    assert t.num_gaussians == 1300 and t.l_max == 2
    for name, p in t.params.items():
        assert p.shape[0] == 1300 and bool(torch.isfinite(p).all()), name
    for m in _moments(t):
        assert m.shape[0] == 1300 and bool(torch.isfinite(m).all())
    assert t.opt.uv_grad_accum.shape[0] == 1300 and t.opt.grad_accum_dur.shape[0] == 1300
    first, last = history[0][1], history[-1][1]
    print(f"mcmc training, 45 iterations: loss {first:.4f} -> {last:.4f}, relocated per step {[s[1] for s in t.mcmc_steps]}")
    assert last < first


def test_trainer_relocates_the_dead(gpu, scene, training, monkeypatch):
    """Trainer.mcmc_relocate on a state with 150 dead rows and every moment at 1: the dead rows become copies of the rows
    that were drawn, carrying the corrected opacity and scale; moments restart on the drawn and the moved rows only."""
    torch, trainer_mod, ops = gpu, pkg("trainer"), pkg("ops")
    init, views, cfg = training
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3)
    t.add_sh_band()
    n = t.num_gaussians
    rng = np.random.default_rng(4)
    dead_idx = np.sort(rng.choice(n, 150, replace=False))
    t.params["opacity"].copy_(torch.as_tensor(rng.uniform(-3.0, 3.0, n).astype(np.float32)))
    t.params["opacity"][torch.as_tensor(dead_idx).cuda()] = -8.0
    t.params["sh"].copy_(torch.as_tensor(rng.normal(size=tuple(t.params["sh"].shape)).astype(np.float32)))
    for m in _moments(t):
        m.fill_(1.0)
    before = {k: _np(v).copy() for k, v in t.params.items()}
    drawn = {}
    real = ops.sample_by_weight

    def recording(weights, K, seed, counts=None):
        drawn["weights"], drawn["seed"] = _np(weights).copy(), seed
        drawn["samples"], drawn["counts"] = real(weights, K, seed, counts)
        return drawn["samples"], drawn["counts"]

    monkeypatch.setattr(ops, "sample_by_weight", recording)
    t.iter = 11
    assert t.mcmc_relocate() == 150
    torch.cuda.synchronize()
    assert drawn["seed"] == 3 * 1000003 + 10
    assert (drawn["weights"][dead_idx] == 0).all() and (np.delete(drawn["weights"], dead_idx) > 0).all()
    src, counts = _np(drawn["samples"]), _np(drawn["counts"])
    want_s, want_c = ref.sample_by_weight(drawn["weights"], 150, drawn["seed"])
    # (float32 weights in [2^-5, 1) are multiples of 2^-29 and their sum stays below 2^10: every partial sum is exact in
    # float64, in the device's scan as in numpy's running sum)
    assert np.array_equal(src, want_s) and np.array_equal(counts, want_c) and not np.isin(src, dead_idx).any()
    want_l, want_sc = ref.relocate(before["opacity"], before["scale"], counts, np.float32(MIN_OPACITY))
    after = {k: _np(v) for k, v in t.params.items()}
    live = np.setdiff1d(np.arange(n), dead_idx)
    assert np.abs(after["opacity"][live] - want_l[live]).max() <= 1e-5
    assert np.abs(after["scale"][live] - want_sc[live]).max() <= 1e-5
    untouched = np.setdiff1d(live, src)
    for k in after:
        assert np.array_equal(after[k][untouched], before[k][untouched]), k
        assert np.array_equal(after[k][dead_idx], after[k][src]), k           # copies of the updated sources
        if k not in ("opacity", "scale"):
            assert np.array_equal(after[k][src], before[k][src]), k
    reset = np.union1d(src, dead_idx)
    for m in _moments(t):
        m = _np(m).reshape(n, -1)
        assert (m[reset] == 0).all() and (np.delete(m, reset, 0) == 1).all()
    # none dead, or all: nothing to do
    t.params["opacity"].fill_(1.0)
    assert t.mcmc_relocate() == 0
    t.params["opacity"].fill_(-9.0)
    assert t.mcmc_relocate() == 0


def test_mode_off_runs_none_of_it(gpu, scene, training, monkeypatch):
    torch, trainer_mod, ops = gpu, pkg("trainer"), pkg("ops")
    init, views, cfg = training

    def never(*a, **k):
        raise AssertionError("MCMC code ran with mcmc off")

    for name in ("sample_by_weight", "mcmc_relocate", "mcmc_add_noise", "mcmc_regularize"):
        monkeypatch.setattr(ops, name, never)
    t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, mcmc=False), scene_extent=5.0, seed=3)
    t.train(12, loss_every=0)
    torch.cuda.synchronize()
    assert t.mcmc_steps == [] and t.iter == 12


def test_mode_refuses_more_than_one_rank(gpu, scene, training):
    trainer_mod = pkg("trainer")
    init, views, cfg = training

    class TwoRanks:
        world, rank = 2, 0

    with pytest.raises(ValueError):
        trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, cfg, scene_extent=5.0, seed=3, comm=TwoRanks())
    trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, mcmc=False), scene_extent=5.0, seed=3,
                        comm=TwoRanks())  # (the stand-in itself is accepted)


# ---------------------------------------------------------------------------------------------------- the image
def test_relocation_keeps_the_central_ray(gpu, scene, orc):
    """One gaussian of opacity 0.9 facing the camera (5 px wide, centred on pixel (32, 32) of 64x64, colour 0.78), against
    its three coincident copies after ops.mcmc_relocate with count 2 (n = 3: o' = 0.5358, scale x 0.8278).  The relocation
    keeps the integral along the central ray, not the image: the copies are smaller and more transparent further out.

    The float64 composite of the two scenes (the CPU oracle in float64) differs by 1.8e-9 (L1 over the three channels) at the centre
    pixel (0.70388532 both), by up to 4.3e-2 at other pixels, and the image's mean falls by 6.42 % (0.027194 -> 0.025449).  So the
    reference itself does not keep the mean within 5 %: that is printed, not asserted.  Asserted: the centre pixel
    agrees to the reference's own difference plus the project's float32 bar for one pixel (PIXEL_L1_TOL) for each of the
    two renders -- well inside 1e-3 -- and the change of the mean per-pixel L1 equals the reference's to MEAN_L1_TOL per
    render.  On the MI355X: centre pixel bit-identical, largest pixel difference 4.28e-2, mean -6.42 %, as the reference."""
    torch, raster, ops = gpu, pkg("raster"), pkg("ops")
    W = H = 64
    cam, c = scene.make_camera(W, H, 0), scene.CONFIG
    z = 4.0
    s = 5.0 * z / cam["fx"]
    one = dict(xyz=np.array([[0.0, 0.0, z]], np.float32), rgb=np.ones((1, 3), np.float32), sh=np.zeros((1, 0, 3), np.float32),
               opacity=np.array([_logit(0.9)], np.float32), scale=np.full((1, 3), math.log(s), np.float32),
               quaternion=np.array([[1.0, 0.0, 0.0, 0.0]], np.float32))
    three = {k: np.repeat(v, 3, 0) for k, v in one.items()}
    counts = np.full(3, 2, np.int32)
    ref_l, ref_s = ref.relocate(three["opacity"], three["scale"], counts, np.float32(MIN_OPACITY))
    three_ref = dict(three, opacity=ref_l.astype(np.float32), scale=ref_s.astype(np.float32))

    def oracle64(p):
        r = orc.rasterize(p, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, 0, dtype=np.float64)
        assert np.allclose(r["uv"], 32.0)
        return np.asarray(r["image"], np.float64)

    a64, b64 = oracle64(one), oracle64(three_ref)
    ref_centre = np.abs(b64[32, 32] - a64[32, 32]).sum()
    ref_mean = (b64 - a64).sum(-1).mean()
    print(f"float64 reference: centre {a64[32, 32, 0]:.8f} -> {b64[32, 32, 0]:.8f} (L1 {ref_centre:.2e}), largest pixel "
          f"difference {np.abs(b64 - a64).max():.2e}, mean {a64.mean():.6f} -> {b64.mean():.6f} ({b64.mean() / a64.mean() - 1:+.2%})")
    assert ref_centre < 1e-6 and a64[32, 32, 0] > 0.7

    dc = raster.device_camera(cam)
    d3 = raster.device_params(three)
    ops.mcmc_relocate(d3["opacity"], d3["scale"], torch.as_tensor(counts).cuda(), MIN_OPACITY)
    assert np.abs(_np(d3["opacity"]) - ref_l).max() <= 1e-5 and np.abs(_np(d3["scale"]) - ref_s).max() <= 1e-5
    a = _np(raster.RasterContext(1, W, H).rasterize_image(raster.device_params(one), dc, c, 0.0, 0)["image"]).astype(np.float64)
    b = _np(raster.RasterContext(3, W, H).rasterize_image(d3, dc, c, 0.0, 0)["image"]).astype(np.float64)
    centre, mean = np.abs(b[32, 32] - a[32, 32]).sum(), (b - a).sum(-1).mean()
    np.set_printoptions(precision=4, suppress=True, linewidth=200)
    print(f"device: centre {a[32, 32, 0]:.8f} -> {b[32, 32, 0]:.8f} (L1 {centre:.2e}), largest pixel difference "
          f"{np.abs(b - a).max():.2e}, mean {a.mean():.6f} -> {b.mean():.6f} ({b.mean() / a.mean() - 1:+.2%})")
    print("difference along the centre row, pixels 24..40:", (b - a)[32, 24:41, 0])
    assert centre <= ref_centre + 2 * PIXEL_L1_TOL <= 1e-3
    assert abs(mean - ref_mean) <= 2 * MEAN_L1_TOL

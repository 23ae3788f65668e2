"""The float64 oracle as a reference for gsplat_fused_loss on the inputs of tests/loss_cases.py, and the float32
oracle's own error on them -- the yardstick of tests/test_loss_cases_gpu.py.  Nothing here needs a GPU.

Run with -s to see the table of figures (float32 oracle against float64, lambda = 0.2): on uniform noise the largest
gradient error is a few 1e-7 of the largest entry; on flat, ramp and near-white images it is 1e-5 .. 1e-4."""
import numpy as np
import pytest

import loss_cases

SIZES = [(48, 96), (37, 53)]


def _fd_pixels(pred, gt, rng, count=4):
    """A handful of (y, x, c) at least 10 px from every edge (the forward clamps, the adjoint zero-pads: only there is
    the analytic gradient the derivative of the loss) where pred is far enough from gt for a 1e-6 step not to cross
    the kink of |pred - gt|."""
    H, W, _ = pred.shape
    ok = np.abs(pred.astype(np.float64) - gt.astype(np.float64)) > 1e-5
    ok[:10], ok[H - 10:], ok[:, :10], ok[:, W - 10:] = False, False, False, False
    idx = np.argwhere(ok)
    if len(idx) == 0:
        return []
    return [tuple(int(i) for i in idx[k]) for k in rng.choice(len(idx), size=min(count, len(idx)), replace=False)]


@pytest.mark.parametrize("shape", SIZES)
@pytest.mark.parametrize("name", loss_cases.FAMILY_NAMES)
def test_f64_oracle_gradient_matches_finite_differences(orc, name, shape):
    """Step, tolerance and interior rule of test_fused_loss_gradient_matches_finite_differences_f64, on every family.
    Families with pred == gt everywhere (black) have no differentiable pixel and contribute nothing."""
    H, W = shape
    pred, gt = (a.astype(np.float64) for a in loss_cases.family(name, H, W))
    pixels = _fd_pixels(pred, gt, np.random.default_rng(H * W))
    if name != "black":
        assert pixels, "no interior pixel with pred != gt"
    _, grad = orc.fused_loss(pred, gt, 0.2, dtype=np.float64)
    eps = 1e-6
    for (y, x, c) in pixels:
        p, m = pred.copy(), pred.copy()
        p[y, x, c] += eps
        m[y, x, c] -= eps
        fd = (orc.fused_loss(p, gt, 0.2, dtype=np.float64)[0] - orc.fused_loss(m, gt, 0.2, dtype=np.float64)[0]) / (2 * eps)
        assert abs(fd - grad[y, x, c]) < 1e-9 + 1e-5 * abs(fd), (name, y, x, c, fd, grad[y, x, c])


@pytest.mark.parametrize("shape", SIZES)
def test_f32_oracle_error_per_family(orc, shape):
    """The yardstick, computed (never hard-coded): float32 oracle against float64 oracle on the same float32 inputs.
    Asserted: every figure is finite, and noise is the best-conditioned family with a non-constant gradient."""
    H, W = shape
    figs = {}
    print(f"\n  {H}x{W} lambda 0.2: float32 oracle vs float64   max|dgrad|/max|grad|   rel L2      |dloss|      loss")
    for name, (pred, gt) in loss_cases.families(H, W).items():
        loss64, grad64, f = loss_cases.oracle_pair(orc, pred, gt, 0.2)
        figs[name] = f
        print(f"  {name:16s} {f['share']:.3e}   {f['l2']:.3e}   {f['loss']:.3e}   {loss64:.6f}")
        assert all(np.isfinite(v) for v in f.values()), (name, f)
        assert np.isfinite(grad64).all() and np.isfinite(loss64), name
    # Noise is the best-conditioned input: every family with low local variance is at least ten times worse.  Four
    # families sit at noise's own level and are compared with a factor of 4 instead: `unclamped` IS noise (of nine
    # times the variance), the bottom half of `half_identical` is, `dark` has mu^2 << C1 so that the L1 term makes up
    # the gradient, and `black` has one constant gradient value.
    at_noise_level = ("unclamped", "half_identical", "dark", "black")
    noise = figs["noise"]
    for n, f in figs.items():
        if n == "noise":
            continue
        if n in at_noise_level:
            assert f["share"] <= 4.0 * noise["share"] and f["l2"] <= 4.0 * noise["l2"], (n, f, noise)
        else:  # (the blob's L2 is carried by its few bright pixels: five times, where the largest entry says ten)
            assert f["share"] >= 10.0 * noise["share"] and f["l2"] >= 5.0 * noise["l2"], (n, f, noise)


@pytest.mark.parametrize("shape", SIZES + [(13, 27), (1, 1)])
def test_plain_loss_is_the_oracles_formula(orc, shape):
    """loss_cases.plain_loss, the second float32 evaluation behind the yardstick of the loss value, computes in float64
    what the float64 oracle computes, on every family: to 2e-7, since the two may differ in how C1 and C2 are rounded (one
    float32 ulp, 6e-8 of a constant to which the per-pixel term has a sensitivity below 1)."""
    H, W = shape
    for name, (pred, gt) in loss_cases.families(H, W).items():
        for lam in (0.2, 1.0):
            loss64 = orc.fused_loss(pred, gt, lam, dtype=np.float64)[0]
            assert abs(loss_cases.plain_loss(pred, gt, lam, np.float64) - loss64) <= 2e-7, (name, lam)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_l1_gradient_at_equal_pixels_is_minus_one(orc, dtype):
    """A reference quirk: at pred == gt the L1 part is -(1 - lambda) / (3 H W), not 0 (cuda/loss.cu:418,
    `p1 > p2 ? 1 : -1`).  On two black images at lambda = 0 the whole gradient is exactly that constant."""
    H, W = 37, 53
    pred, gt = loss_cases.family("black", H, W)
    loss, grad = orc.fused_loss(pred, gt, 0.0, dtype=dtype)
    assert loss == 0.0
    want = dtype(-1.0) * (dtype(1.0) / dtype(np.float32(H * W * 3)))
    assert grad.dtype == dtype and (grad == want).all()


def test_families_are_deterministic_and_as_described():
    a, b = loss_cases.families(48, 96), loss_cases.families(48, 96)
    assert list(a) == list(loss_cases.FAMILY_NAMES)
    for name in a:
        for k in range(2):
            assert a[name][k].dtype == np.float32 and a[name][k].shape == (48, 96, 3) and a[name][k].flags.c_contiguous
            assert np.array_equal(a[name][k], b[name][k]), name
    pred, gt = a["half_identical"]
    assert np.array_equal(pred[:24], gt[:24]) and not np.array_equal(pred[24:], gt[24:])
    pred, gt = a["bg_band"]
    assert (pred[:12] == loss_cases.BG).all() and (gt[:, :24] == loss_cases.BG).all() and pred[24, 48, 0] != loss_cases.BG
    pred, gt = a["unclamped"]
    assert pred.min() < -0.9 and pred.max() > 1.9
    assert (a["near_white"][1] == 1.0).all() and a["near_white"][0].max() <= 1.0
    for (H, W) in ((48, 96), (96, 160), (17, 33), (33, 65)):  # the step lies on a tile seam whenever the image has one
        xs, ys = loss_cases.seam_positions(H, W)
        assert (xs + 1) % 32 == 0 and (ys + 1) % 16 == 0 and 0 <= xs < W - 1 and 0 <= ys < H - 1, (H, W, xs, ys)
        gt = loss_cases.family("seam_edge", H, W)[1]
        assert gt[0, xs, 0] != gt[0, xs + 1, 0] and gt[ys, 0, 0] != gt[ys + 1, 0, 0]


def test_adam_table_covers_the_classes(orc):
    """The f32 oracle on the edge table: the rows reach every class the GPU test pins (finite, NaN, +inf, -inf in p;
    inf in v), so `class must match` is not vacuous."""
    p, g, m, v = loss_cases.adam_table()
    assert np.isnan(g).sum() == 8 and np.isinf(g).sum() == 16 and (np.abs(g[g != 0]) < 1.2e-38).any()
    seen = set()
    for h in loss_cases.adam_hypers():
        with np.errstate(all="ignore"):
            po, mo, vo = orc.adam_step(p, g, m, v, *h)
        seen |= {"nan"} if np.isnan(po).any() else set()
        seen |= {"finite"} if np.isfinite(po).any() else set()
        seen |= {"vinf"} if np.isinf(vo).any() else set()
        seen |= {"minf"} if np.isinf(mo).any() else set()
    assert {"nan", "finite", "vinf", "minf"} <= seen, seen

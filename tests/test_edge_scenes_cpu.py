"""The edge scenes (tests/edge_scenes.py) hit the regimes they are named for, and the oracle -- the GPU tests' checker --
is right there: its float64 per-gaussian backward chain against float64 central differences of its own forward, stage
by stage and population by population.  Runs without a GPU."""
import numpy as np
import pytest

import edge_scenes as es

C = dict(near_thresh=0.3, mh_dist=3.0, cull_mask_padding=100, bg=0.5)
ALPHA_MIN = 1.0 / 255.0


def _forward(orc, size, dtype=np.float32):
    params, cam, pops = es.make_edge_scene(size)
    L = es.SIZES[size][3]
    ref = orc.rasterize(params, cam, C["near_thresh"], C["mh_dist"], C["cull_mask_padding"], C["bg"], L, dtype, threads=8)
    return params, cam, pops, ref


@pytest.mark.parametrize("size", ["small", "large"])
def test_edge_scene_populations_hit_their_regimes(orc, size):
    params, cam, pops, ref = _forward(orc, size)
    N = len(params["xyz"])
    W, H = cam["width"], cam["height"]
    mask = ref["mask"]
    M = int(mask.sum())
    cp = es.compact_populations(pops, mask)
    rows = np.sort(np.concatenate(list(pops.values())))
    assert (rows == np.arange(N)).all(), "the populations partition the rows"
    # culled rows interleave with visible ones
    culled = pops["culled"]
    assert not mask[culled].any() and M < N
    assert (np.diff(culled) > 1).all() and mask[culled + 1].mean() > 0.9
    for k in set(pops) - {"culled", "near_edge"}:
        assert mask[pops[k]].all(), f"{k}: every row is visible"
    f = np.float32
    xc, uv, rad = ref["xyz_c"], ref["uv"], ref["radius"]
    tfx, tfy = es.forward_tan_fov(cam)
    bfx, bfy = es.backward_tan_fov(cam)
    ratio_x, ratio_y = xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2]  # the forward's x / z in float (gs::jacobian)
    zi = f(1.0) / (xc[:, 2] + f(1e-6))
    bratio_x, bratio_y = xc[:, 0] * zi, xc[:, 1] * zi            # the backward's (gs::jacobian_bwd)
    cx, cy = np.abs(ratio_x) > f(1.3) * tfx, np.abs(ratio_y) > f(1.3) * tfy
    on_list = np.zeros(M, bool)
    on_list[ref["sorted"]] = True
    # clamp band: the intended axis clamps, the other does not; some rows reach a tile, some do not
    for k, wx, wy in (("clamp_x", True, False), ("clamp_y", False, True), ("clamp_corner", True, True)):
        r = cp[k]
        assert (cx[r] == wx).all() and (cy[r] == wy).all(), k
        assert (uv[r, 0] >= -C["cull_mask_padding"]).all() and (uv[r, 0] <= W + C["cull_mask_padding"]).all()
        assert 0.1 < on_list[r].mean() < 0.9, f"{k}: {on_list[r].sum()} of {len(r)} rows on a tile list"
        for axis, want, lim in ((0, wx, W), (1, wy, H)):
            if want:  # both sides
                assert (uv[r, axis] < 0).sum() > len(r) // 5 and (uv[r, axis] > lim).sum() > len(r) // 5, (k, axis)
    # clamp boundary: rows on either side of the forward's and of the backward's limit, on both axes and signs
    r = cp["clamp_boundary"]
    for rat, brat, t, b in ((ratio_x, bratio_x, tfx, bfx), (ratio_y, bratio_y, tfy, bfy)):
        for sgn in (1, -1):
            for v, lim in ((sgn * rat[r], f(1.3) * t), (sgn * brat[r], f(1.3) * b)):
                near = np.abs(v - lim) <= 8 * np.spacing(lim)
                assert (near & (v < lim)).sum() >= 3 and (near & (v > lim)).sum() >= 3
    assert on_list[r].mean() > 0.5
    # NaN minor radius: every tiny row, and those rows are on tile lists
    nan_r = np.isnan(rad[:, 1])
    assert nan_r[cp["tiny"]].all() and on_list[cp["tiny"]].all()
    assert nan_r.sum() >= len(cp["tiny"]) and not np.isnan(rad[:, 0]).any()
    # near plane: z in [0.3, 0.45], over many tiles; z == near_thresh kept, the float below culled
    r = cp["near"]
    assert (xc[r, 2] >= f(0.3)).all() and (xc[r, 2] <= 0.45).all()
    assert np.median(rad[r, 0]) > (30 if size == "small" else 120)
    e = pops["near_edge"]
    z_e = params["xyz"][e, 2]
    assert (mask[e] == (z_e >= f(0.3))).all() and mask[e].sum() == 4 and (~mask[e]).sum() == 4
    assert (z_e[~mask[e]] == np.nextafter(f(0.3), f(0))).all()
    # needle / flat: 100 - 1000 : 1 in 3D; a fifth of the needles stay beyond 8 : 1 on screen
    for k in ("needle", "flat"):
        sc = np.exp(params["scale"][pops[k]].astype(np.float64))
        assert (sc.max(1) / sc.min(1) > 90).all(), k
    r = cp["needle"]
    assert (rad[r, 0] / np.maximum(np.nan_to_num(rad[r, 1], nan=1.0), 1.0) > 8).mean() > 0.15
    for k, lo, hi in (("quat_small", 1e-4, 1e-2), ("quat_large", 1e2, 1e4)):
        n = np.linalg.norm(params["quaternion"][pops[k]], axis=1)
        assert (n > lo).all() and (n < hi).all(), k
    # opacity: the alpha clamp (0.99) is hit, sigmoid rounds to 1 in float; the gate population peaks at 1/255
    sig = f(1) / (f(1) + np.exp(-ref["opacity"].astype(f)))
    r = cp["saturated"]
    assert (sig[r] > 0.99).all() and (sig[r] == f(1)).sum() >= len(r) // 5 and on_list[r].mean() > 0.9
    g = sig[cp["gate"]].astype(np.float64)
    assert (np.abs(g / ALPHA_MIN - 1) < 0.06).all() and (g < ALPHA_MIN).any() and (g > ALPHA_MIN).any()
    assert (sig[cp["vanishing"]] < 1e-5).all() and on_list[cp["vanishing"]].mean() > 0.8
    # visible rows on no tile list (their gradient must come back exactly 0)
    assert (~on_list).sum() >= (100 if size == "small" else 300)
    lens = np.diff(ref["ranges"])
    if size == "large":  # lists long enough for the segmented forward / backward
        assert (lens > 1488).sum() >= 50 and (np.asarray(ref["n"]) > 2 * 496).sum() > 1000


def _central(f, x, h):
    """d f / d x[:, k] for every column k (rows independent), central differences with per-element steps h."""
    out = np.empty(x.shape)
    for k in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, k] += h[:, k]
        xm[:, k] -= h[:, k]
        out[:, k] = (f(xp) - f(xm)) / (xp[:, k] - xm[:, k])
    return out


def _close(got, want, pops, what, rtol):
    """Per population: relative L2 below rtol, and every row within 10 rtol of its own size plus the population's rms row
    (no row hides in a sum)."""
    for k, r in pops.items():
        if not len(r):
            continue
        tol = rtol(r) if callable(rtol) else rtol
        a, b = got[r], want[r]
        nb = np.linalg.norm(b)
        if nb == 0:
            assert np.abs(a).max() == 0, f"{what} [{k}]"
            continue
        assert np.linalg.norm(a - b) <= tol * nb, f"{what} [{k}]: relative error {np.linalg.norm(a - b) / nb:.2e}"
        row = np.linalg.norm(a - b, axis=1) <= 10 * tol * (np.linalg.norm(b, axis=1) + nb / np.sqrt(len(r)))
        assert row.all(), f"{what} [{k}]: rows {np.nonzero(~row)[0][:5]} off"


def test_oracle_backward_chain_matches_finite_differences_per_population(orc):
    """conic -> (J, Sigma) -> (xyz_c, q, s) and uv -> xyz_c, in float64, each stage against central differences of the
    oracle's own forward for that stage, with random upstream gradients.  In the clamp band this pins dJ02/dx = 0 and the
    fx cx / z^2 term of dJ02/dz; the boundary rows are left out (within an ulp of the kink no step fits), and every other
    row is further from the kink than the step."""
    f64 = np.float64
    params, cam, pops, ref = _forward(orc, "small", f64)
    cp = es.compact_populations(pops, ref["mask"])
    cp.pop("clamp_boundary")
    M = ref["num_culled"]
    W, H = cam["width"], cam["height"]
    fx, fy = float(cam["fx"]), float(cam["fy"])
    tfx, tfy = W / (2.0 * fx), H / (2.0 * fy)  # one tan(fov) for forward and backward: the derivative of what is run
    rng = np.random.default_rng(17)
    view, proj = np.asarray(cam["view"], f64), np.asarray(cam["proj"], f64)
    xyz_c, J, sigma, q, s = (np.array(ref[k], f64) for k in ("xyz_c", "J", "sigma", "quaternion", "scale"))
    g_conic = rng.standard_normal((M, 3))
    g_uv = rng.standard_normal((M, 2))
    # (1) conic(J, Sigma)
    conic = orc.conic_from_J(sigma, view, J, 3.0, f64)[0]
    gJ, gS = orc.compute_conic_backward(J, sigma, view, conic, g_conic, dtype=f64)
    # the conic's gradient is per matrix element (its stored off-diagonal stands for two), Sigma's per stored entry
    wc = np.array([1.0, 2.0, 1.0])
    loss_J = lambda Jx: (orc.conic_from_J(sigma, view, Jx, 3.0, f64)[0] * g_conic * wc).sum(1)
    loss_S = lambda Sx: (orc.conic_from_J(Sx, view, J, 3.0, f64)[0] * g_conic * wc).sum(1)
    jmax, smax = np.abs(J).max(1, keepdims=True), np.abs(sigma).max(1, keepdims=True)
    # steps of 1e-4 of the largest entry (Sigma: plus what adds 1e-4 of the 0.3 px^2 floor of the 2D covariance): the
    # truncation error of a needle's strongly curved conic and the rounding of a tiny splat's both stay below 1e-6
    hJ = np.repeat(1e-4 * jmax, 6, 1)
    hS = 1e-4 * 0.3 / jmax ** 2
    _close(gJ, _central(loss_J, J, hJ), cp, "dconic/dJ", 1e-5)
    _close(gS, _central(loss_S, sigma, np.repeat(hS, 6, 1)), cp, "dconic/dSigma", 1e-5)
    # (2) Sigma(q, s): relative steps
    gq, gs = orc.compute_sigma_backward(q, s, gS, f64)
    loss_q = lambda qx: (orc.compute_sigma(qx, s, f64) * gS).sum(1)
    loss_s = lambda sx: (orc.compute_sigma(q, sx, f64) * gS).sum(1)
    # the forward normalises by 1 / (|q| + 1e-6), the backward differentiates q / |q| (as the reference does): a relative
    # difference of 1e-6 / |q|, 1e-3 for the quaternions of norm 1e-3
    qn = np.linalg.norm(q, axis=1)
    _close(gq, _central(loss_q, q, 1e-7 * np.repeat(qn[:, None], 4, 1)), cp, "dSigma/dq",
           lambda r: max(1e-4, 5e-6 / qn[r].min()))
    _close(gs, _central(loss_s, s, np.full(s.shape, 1e-6)), cp, "dSigma/ds", 1e-4)
    # (3) J(xyz_c) with the clamp; (4) uv(xyz_c).  H1 and Q1 use 1 / (z + 1e-6) and 1 / w where their forwards divide by
    # z and w + 1e-6: a relative difference of a few 1e-6 / z (z >= 0.3), hence 1e-4
    h = 1e-7 * np.repeat(np.abs(xyz_c[:, [2]]), 3, 1)
    lim_x, lim_y = 1.3 * tfx, 1.3 * tfy
    kink = np.minimum(np.abs(np.abs(xyz_c[:, 0] / xyz_c[:, 2]) - lim_x), np.abs(np.abs(xyz_c[:, 1] / xyz_c[:, 2]) - lim_y))
    kink = kink[np.concatenate(list(cp.values()))]
    assert kink.min() > 100 * 1e-7 * (1.0 + max(lim_x, lim_y)), f"a row sits {kink.min():.2e} from the clamp"
    g_xyz = orc.compute_projection_jacobian_backward(xyz_c, fx, fy, tfx, tfy, gJ, dtype=f64)
    loss_x = lambda xc: (orc.projection_jacobian(xc, fx, fy, tfx, tfy, f64) * gJ).sum(1)
    fd = _central(loss_x, xyz_c, h)
    _close(g_xyz, fd, cp, "dJ/dxyz_c", 1e-4)
    band = np.concatenate([cp["clamp_x"], cp["clamp_corner"]])
    assert (g_xyz[band, 0] == 0).all() and (np.abs(fd[band, 0]) <= 1e-9 * np.abs(fd[band, 2])).all(), "dJ02/dx = 0 when x clamps"
    u = lambda xc: orc.project_to_screen(xc, proj, W, H, f64)
    g_uvx = orc.project_to_screen_backward(xyz_c, proj, g_uv, W, H, dtype=f64)
    _close(g_uvx, _central(lambda xc: (u(xc) * g_uv).sum(1), xyz_c, h), cp, "duv/dxyz_c", 1e-4)

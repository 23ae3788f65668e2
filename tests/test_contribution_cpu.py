"""CPU tests of the blend-weight statistics: the numpy reference (tests/contribution_reference.py) against identities of
the oracle's forward and against known answers, the declared entry point and config keys, and the pruning policy."""
import os
import re

import numpy as np
import pytest

import contribution_reference as cr
from conftest import ROOT, pkg


def _oracle(orc, scene, name, view=0):
    N, W, H, L = scene.WORKLOADS[name][:4]
    c = scene.CONFIG
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H, view)
    return W, H, orc.rasterize(params, cam, c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0, L, threads=4)


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_reference_identities_on_the_oracle_forward(orc, scene, name):
    W, H, ref = _oracle(orc, scene, name)
    s, m, px = cr.contribution_stats(ref, W, H)
    covered = (1.0 - np.asarray(ref["T"], np.float64)).sum()  # sum_j weight_sum[j] = sum_p (1 - T_final(p))
    rel = abs(s.sum() - covered) / covered
    print(f"{name}: |sum weight_sum - sum (1 - T)| / sum (1 - T) = {rel:.1e}; never composited {int((px == 0).sum())}, "
          f"weight_max < 0.01: {int((m < 0.01).sum())} of {len(px)}")
    assert rel < 1e-6
    assert np.array_equal(px == 0, s == 0) and np.array_equal(px == 0, m == 0)
    assert (m <= 0.99).all() and (m >= 0).all()
    assert (s <= px * m * (1 + 1e-12)).all()
    assert (px > 0).any() and (px == 0).any()


def _forward(orc, uv, logit, conic, sorted_ids, ranges, W, H):
    uv, conic = np.asarray(uv, np.float32).reshape(-1, 2), np.asarray(conic, np.float32).reshape(-1, 3)
    logit = np.asarray(logit, np.float32)
    rgb = np.ones((len(logit), 3), np.float32)
    sorted_ids, ranges = np.asarray(sorted_ids, np.int32), np.asarray(ranges, np.int32)
    n, T, _ = orc.render_image(uv, logit, conic, rgb, 0.0, sorted_ids, ranges, W, H)
    return dict(uv=uv, opacity=logit, conic=conic, sorted=sorted_ids, ranges=ranges, n=n, T=T)


def _alpha_map(u, v, k, logit, W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.minimum(0.99, 1.0 / (1.0 + np.exp(-logit)) * np.exp(-0.5 * k * ((x - u) ** 2 + (y - v) ** 2)))
    return np.where(a > np.float32(0.00392156862), a, 0.0)


def test_one_isotropic_gaussian_alone_weighs_its_alpha(orc):
    W = H = 32
    u, v, k, logit = 15.25, 17.5, 0.02, 1.0
    fwd = _forward(orc, [u, v], [logit], [k, 0.0, k], [0, 0, 0, 0], [0, 1, 2, 3, 4], W, H)
    s, m, px = cr.contribution_stats(fwd, W, H)
    a = _alpha_map(u, v, np.float64(np.float32(k)), logit, W, H)
    assert px[0] == (a > 0).sum() and 0 < px[0] < W * H
    np.testing.assert_allclose(s[0], a.sum(), rtol=1e-6)
    np.testing.assert_allclose(m[0], a.max(), rtol=1e-6)


def test_the_second_of_two_stacked_gaussians_weighs_alpha_times_one_minus_alpha(orc):
    W = H = 32
    u, v, k, logit = 16.0, 16.0, 0.03, 0.5
    fwd = _forward(orc, [u, v, u, v], [logit, logit], [k, 0.0, k] * 2, [0, 1] * 4, [0, 2, 4, 6, 8], W, H)
    s, m, px = cr.contribution_stats(fwd, W, H)
    a = _alpha_map(u, v, np.float64(np.float32(k)), logit, W, H)
    assert px[0] == px[1] == (a > 0).sum()
    np.testing.assert_allclose(s, [a.sum(), (a * (1 - a)).sum()], rtol=1e-6)
    np.testing.assert_allclose(m, [a.max(), (a * (1 - a)).max()], rtol=1e-6)


def test_global_order_leaves_culled_rows_at_zero():
    stats = (np.array([1.0, 2.0]), np.array([0.5, 0.25]), np.array([3, 4]))
    s, m, px = cr.to_global(stats, [4, 1], 6)
    assert s.tolist() == [0, 2, 0, 0, 1, 0] and m.tolist() == [0, 0.25, 0, 0, 0.5, 0] and px.tolist() == [0, 4, 0, 0, 3, 0]


def test_abi_declares_the_entry_point_and_the_config_keys_default_off(tmp_path):
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    name = "gsplat_context_accumulate_contributions"
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert len(lib.SIGNATURES[name][1]) == 6
    assert lib.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    cfg = pkg("trainer").DEFAULT_CONFIG
    assert cfg["prune_contribution"] is False
    assert cfg["prune_contribution_threshold"] == 0.01 and cfg["prune_contribution_interval"] == 1000
    ds = pkg("dataset")
    f = tmp_path / "c.yaml"
    f.write_text("num_iters: 5\nprune_contribution: true\nprune_contribution_interval: 500\n")
    assert ds.parseExtensions(f) == {"prune_contribution": True}  # (the numeric keys are dict-only)
    f.write_text("num_iters: 5\nprune_contribution: off\nabsgrad: true\n")
    assert ds.parseExtensions(f) == {"prune_contribution": False, "absgrad": True}
    f.write_text("num_iters: 5\n")
    assert ds.parseExtensions(f) == {}


def test_prune_policy():
    import torch
    mask = pkg("trainer").contribution_prune_mask
    w_max = torch.tensor([0.5, 0.005, 0.0, 0.02, 0.0099999, 0.01])
    pixels = torch.tensor([10, 3, 0, 1, 7, 2], dtype=torch.int32)
    assert mask(w_max, pixels, 0.01).tolist() == [False, True, True, False, True, False]  # strictly below the threshold
    assert mask(w_max, pixels, 0.0).tolist() == [False, False, True, False, False, False]  # only the never-composited
    assert mask(w_max, pixels, 0.6).tolist() == [False] * 6                                # never everything
    assert mask(torch.zeros(3), torch.zeros(3, dtype=torch.int32), 0.0).tolist() == [False] * 3
    assert mask(w_max[:0], pixels[:0], 0.01).tolist() == []

"""The float64 references of the 3D smoothing filter (tests/filter3d_reference.py) checked against themselves -- the chain
rule against central differences of the transform, the limits -- and the shared filter scene: its populations lie where
they were placed, and few enough sampling decisions sit on a boundary for the GPU comparison to skip them."""
import numpy as np

import filter3d_reference as f3


def test_chain_rule_matches_central_differences():
    """Central differences of the reference transform against the reference chain rule, 1e-6 relative, on rows with
    f = 0, f >> s, f << s, f ~ s and logits from -8 to 12."""
    scale, opacity, f, pops = f3.transform_rows()
    scale, opacity, f = scale.astype(np.float64), opacity.astype(np.float64), f.astype(np.float64)
    assert opacity.min() < -7.9 and opacity.max() > 11.9
    for name in ("f<<s", "f~s", "f>>s", "logit>8", "f=0"):
        assert len(pops[name]) > 10, name
    rng = np.random.default_rng(0)
    c_s, c_o = rng.normal(size=scale.shape), rng.normal(size=opacity.shape)

    def loss_rows(sc, op):  # every row is a function of its own parameters only
        se, oe, _, _ = f3.apply(sc, op, f)
        return (c_s * se).sum(1) + c_o * oe

    want_s, want_o = f3.apply_backward(scale, opacity, f, c_s, c_o)
    h = 1e-5
    fd_s = np.empty_like(scale)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd_s[:, k] = (loss_rows(scale + e, opacity) - loss_rows(scale - e, opacity)) / (2 * h)
    fd_o = (loss_rows(scale, opacity + h) - loss_rows(scale, opacity - h)) / (2 * h)
    for name, rows in pops.items():
        row_size = np.maximum(np.abs(want_s[rows]).max(1), np.abs(want_o[rows]))
        err_s = np.abs(fd_s[rows] - want_s[rows]) / row_size[:, None]
        err_o = np.abs(fd_o[rows] - want_o[rows]) / row_size
        print(f"{name}: central differences off by {err_s.max():.1e} (scale), {err_o.max():.1e} (opacity) of the row")
        assert err_s.max() < 1e-6 and err_o.max() < 1e-6, name
    # the two opacity factors by themselves, where a difference quotient resolves them (f ~ s)
    rows = pops["f~s"]
    se, oe, o, _ = f3.apply(scale[rows], opacity[rows], f[rows])
    d_oe = (f3.apply(scale[rows], opacity[rows] + h, f[rows])[1] - f3.apply(scale[rows], opacity[rows] - h, f[rows])[1]) / (2 * h)
    sig = 1.0 / (1.0 + np.exp(-opacity[rows]))
    np.testing.assert_allclose(d_oe, (1 - sig) / (1 - o), rtol=1e-6)
    zero = np.zeros_like(c_s[rows])
    gs, _ = f3.apply_backward(scale[rows], opacity[rows], f[rows], zero, np.ones(len(rows)))
    w = np.exp(2 * scale[rows]) / (np.exp(2 * scale[rows]) + f[rows, None] ** 2)
    np.testing.assert_allclose(gs, (1 - w) / (1 - o)[:, None], rtol=1e-9)


def test_limits():
    scale, opacity, f, pops = f3.transform_rows()
    zero = pops["f=0"]
    se, oe, o, rho = f3.apply(scale, opacity, f)
    assert (se[zero] == scale[zero]).all() and (oe[zero] == opacity[zero]).all() and (rho[zero] == 1).all()
    gs, go = f3.apply_backward(scale, opacity, f, np.ones_like(se), np.ones_like(oe))
    assert (gs[zero] == 1).all() and (go[zero] == 1).all()
    # Sigma_eff = Sigma + f^2 I and rho3 = sqrt(det Sigma / det Sigma_eff)
    live = f > 0
    s2 = np.exp(2.0 * scale[live].astype(np.float64))
    f2 = f[live].astype(np.float64)[:, None] ** 2
    np.testing.assert_allclose(np.exp(2 * se[live]), s2 + f2, rtol=1e-12)
    np.testing.assert_allclose(rho[live], np.sqrt(np.prod(s2 / (s2 + f2), 1)), rtol=1e-10, atol=1e-300)
    # f -> infinity: rho3 -> 0, monotonically
    last = np.ones(len(scale))
    for mult in (1e0, 1e2, 1e4, 1e6):
        rho = f3.apply(scale, opacity, np.exp(scale.max(1).astype(np.float64)) * mult)[3]
        assert (rho < last).all()
        last = rho
    assert last.max() < 1e-17
    # f -> 0: the identity in the limit
    se, oe, _, rho = f3.apply(scale, opacity, np.exp(scale.min(1).astype(np.float64)) * 1e-9)
    np.testing.assert_allclose(se, scale, rtol=0, atol=1e-15)
    np.testing.assert_allclose(oe, opacity.astype(np.float64), rtol=0, atol=1e-9)


def test_filter_scene(scene):
    xyz, cams, pops = f3.make_scene(scene)
    assert len(xyz) == 3000 and len(cams) == 5
    assert len({(c["width"], c["height"]) for c in cams}) == 5 and len({c["fx"] for c in cams}) == 5
    filt, sampled, per_cam = f3.compute_filter3d(xyz, cams, f3.NEAR)
    z = np.stack([f3.project(c, xyz)[0] for c in cams])
    assert (z[:, pops["behind"]] < 0).all() and not sampled[pops["behind"]].any()
    assert (z[:, pops["outside"]] > f3.NEAR).all() and not sampled[pops["outside"]].any()
    one = per_cam[:, pops["one"]]
    assert one[4].all() and not one[:4].any(), "seen by the wide camera and by no other"
    assert sampled[pops["base"]].mean() > 0.99
    seen_by = per_cam[:, pops["base"]].sum(0)
    assert (seen_by >= 2).mean() > 0.5 and (seen_by == 5).any()  # the minimum is taken over several cameras
    # unsampled rows carry the largest value of the sampled ones
    assert (filt[~sampled] == filt[sampled].max()).all() and (~sampled).sum() >= 400
    t = filt / np.sqrt(0.2)
    want = np.min(np.where(per_cam, z / np.array([c["fx"] for c in cams])[:, None], np.inf), 0)
    np.testing.assert_allclose(t[sampled], want[sampled], rtol=1e-15)
    share = f3.fragile(xyz, cams, f3.NEAR).mean()
    print(f"fragile sampling decisions: {share:.4%} of {len(xyz)} gaussians")
    assert share <= 0.01
    # no camera samples anything: all zeros
    filt0, s0, _ = f3.compute_filter3d(xyz[pops["behind"]], cams, f3.NEAR)
    assert not s0.any() and (filt0 == 0).all()


def test_abi_declares_the_entry_points_and_the_config_keys_default_off(tmp_path):
    import os
    import re

    from conftest import ROOT, pkg
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gsplat_compute_filter3d", "gsplat_filter3d_apply", "gsplat_filter3d_apply_backward",
                 "gsplat_context_set_filter3d"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
    assert len(lib.SIGNATURES["gsplat_compute_filter3d"][1]) == 10
    assert len(lib.SIGNATURES["gsplat_filter3d_apply"][1]) == 7
    assert len(lib.SIGNATURES["gsplat_filter3d_apply_backward"][1]) == 10
    assert lib.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1))
    trainer_src = open(os.path.join(ROOT, "3dgs_amd", "trainer.py")).read()
    assert re.search(r"\bfilter3d=False, filter3d_interval=100, filter3d_near=0\.2\b", trainer_src)
    ds = pkg("dataset")
    f = tmp_path / "c.yaml"
    f.write_text("num_iters: 5\nfilter3d: true\nantialiased: true\n")
    assert ds.parseExtensions(f) == {"filter3d": True, "antialiased": True}
    f.write_text("num_iters: 5\n")
    assert ds.parseExtensions(f) == {}

"""Trainer.save_compressed / compress.load_scene on the generated 1000-gaussian, 160x96, four-view scene of
tests/test_absgrad_gpu.py after its 36 iterations: the file decodes to what the numpy reference decoder says, bit for bit;
its SH indices are nearest for the decoded codebook; a Trainer built from it renders.  The PSNR of the decoded scene against
the uncompressed one is printed, not asserted (README)."""
import numpy as np
import pytest

import vq_reference as vqr
from conftest import pkg
from test_absgrad_gpu import _training_setup

pytestmark = pytest.mark.gpu

BAR, FLOOR = 1e-6, 2.0 ** -149
KEYS = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def setup(gpu, scene):
    return _training_setup(gpu, scene)  # built once: (init, views, cfg)


def _trained(setup, iters=36, **keys):
    init, views, cfg = setup
    t = pkg("trainer").Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, **keys), scene_extent=5.0, seed=3)
    t.train(iters, loss_every=0)
    return t


def _renders(torch, params, l_max, views, cfg):
    raster = pkg("raster")
    n = params["xyz"].shape[0]
    ctx = raster.RasterContext(n, int(views[0][0]["width"]), int(views[0][0]["height"]))
    out = [ctx.rasterize_image({k: params[k] for k in KEYS}, cam, cfg, 0.0, l_max)["image"].clone() for cam, _ in views]
    torch.cuda.synchronize()
    return [_np(i).astype(np.float64) for i in out]


def _psnr(a, b):
    return float(np.mean([10.0 * np.log10(1.0 / max(np.mean((x - y) ** 2), 1e-30)) for x, y in zip(a, b)]))


@pytest.mark.parametrize("l_max", [3, 0])
def test_saved_scene_loads_as_the_reference_decodes_it(gpu, setup, tmp_path, l_max):
    compress, raster, trainer_mod = pkg("compress"), pkg("raster"), pkg("trainer")
    _, views, _ = setup
    t = _trained(setup, max_sh_band=l_max, add_sh_band_interval=10)
    assert t.l_max == l_max
    n = t.num_gaussians
    path = tmp_path / "scene.npz"
    written = t.save_compressed(path, codebook_size=64, iterations=5, seed=2)
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    assert "objective" not in arrays and all(arrays[k].tobytes() == written[k].tobytes() for k in arrays)
    loaded, ref = compress.load_scene(path), vqr.decode(arrays)
    assert loaded["l_max"] == l_max
    for k in KEYS:
        assert loaded[k].dtype == np.float32 and loaded[k].shape == tuple(t.params[k].shape), k
        assert loaded[k].tobytes() == ref[k].tobytes(), k
    if l_max:
        # the stored indices are nearest, by the assign condition, for the codebook a loader sees
        rows = _np(t.params["sh"]).reshape(n, -1)
        book = vqr.dequantise(arrays["sh_codebook_q"], 8, arrays["sh_codebook_lo"], arrays["sh_codebook_hi"])
        assert book.shape == (64, 45) and arrays["sh_index"].dtype == np.uint16 and arrays["sh_index"].shape == (n,)
        got = arrays["sh_index"].astype(np.int64)
        ref_index, ref_dist = vqr.assign(rows, book)
        bar = BAR * np.maximum(vqr.cond(rows, book[got]), vqr.cond(rows, book[ref_index])) + FLOOR
        frac = (vqr.distance_to(rows, book[got]) - ref_dist) / bar
        print(f"[sh_index] worst {float(frac.max()):.4f} of the bar; k-means objective per assign:",
              " ".join(f"{o:.5g}" for o in written["objective"]))
        assert (frac <= 1.0).all() and len(written["objective"]) == 6
    else:
        assert "sh_index" not in arrays and "sh_codebook_q" not in arrays and len(written["objective"]) == 0
    # the same seed writes the same arrays
    again = t.save_compressed(tmp_path / "again.npz", codebook_size=64, iterations=5, seed=2)
    assert all(again[k].tobytes() == written[k].tobytes() for k in arrays)
    # a Trainer built from the file renders every training view
    params = raster.device_params({k: loaded[k] for k in KEYS})
    t2 = trainer_mod.Trainer(params, views, dict(t.cfg), scene_extent=5.0, seed=3)
    assert t2.l_max == l_max and t2.num_gaussians == n
    decoded = _renders(gpu, t2.params, l_max, views, t2.cfg)
    assert all(np.isfinite(i).all() for i in decoded)
    plain = _renders(gpu, t.params, l_max, views, t.cfg)
    truth = [_np(gt).astype(np.float64) for _, gt in views]
    size = path.stat().st_size
    print(f"[compressed scene, SH {l_max}, {n} gaussians, codebook 64] {size} bytes against {n * 4 * (17 + 3 * ((l_max + 1) ** 2 - 1))}"
          f" in the PLY; PSNR of the decoded scene's renders {_psnr(decoded, plain):.2f} dB against the uncompressed renders,"
          f" {_psnr(decoded, truth):.2f} dB against the ground truth (uncompressed: {_psnr(plain, truth):.2f} dB)")
    assert np.isfinite(t2.evaluate())


def test_filter3d_scene_holds_the_fused_scale_and_opacity(gpu, setup, tmp_path):
    ops = pkg("ops")
    t = _trained(setup, iters=5, filter3d=True, max_sh_band=0)
    fused_scale, fused_opacity = (_np(v).astype(np.float64) for v in
                                  ops.filter3d_apply(t.params["scale"], t.params["opacity"], t.filter3d))
    raw_scale, raw_opacity = _np(t.params["scale"]).astype(np.float64), _np(t.params["opacity"]).astype(np.float64)
    assert (fused_scale.min(0) != raw_scale.min(0)).any() and fused_opacity.min() != raw_opacity.min()
    fused = t.save_compressed(tmp_path / "fused.npz")
    raw = t.save_compressed(tmp_path / "raw.npz", raw=True)
    # the stored ranges are the column minima and maxima of what was quantised, exactly
    for arrays, scale, opacity in ((fused, fused_scale, fused_opacity), (raw, raw_scale, raw_opacity)):
        assert (arrays["scale_lo"] == scale.min(0)).all() and (arrays["scale_hi"] == scale.max(0)).all()
        assert arrays["opacity_lo"] == opacity.min() and arrays["opacity_hi"] == opacity.max()
    out = pkg("compress").load_scene(tmp_path / "fused.npz")
    step = (fused_scale.max(0) - fused_scale.min(0)) / 255.0
    assert (np.abs(out["scale"] - fused_scale) <= step / 2 * (1 + 1e-12) + np.abs(out["scale"]) * 2.0 ** -24).all()

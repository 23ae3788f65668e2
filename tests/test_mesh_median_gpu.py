"""Trainer.extract_mesh with median depth and the component filter, end to end: the sphere of tests/test_tsdf_gpu.py (2000
small opaque gaussians on the unit sphere, six cameras on the axes at distance 3, 64x48, resolution 32), rebuilt here, with
a floater of 40 opaque gaussians of the same width around (0, 0, 1.3).

The median mesh equals the reference pipeline (tests/tsdf_reference.py) run on the GPU's own median and T maps, at the
bars of test_extract_mesh_end_to_end: weights equal, tsdf within 1e-6 x (|old| + |val|) + 1e-12, faces equal, vertices
within 1e-6 x (|p_a| + |p_b|) + 1e-12.  The reference integrates depth = median with T' = 0 where the pixel passes the
opacity gate and 1 elsewhere and inverse = False, so that its d / A is d exactly.  The surface integration is a batch bit
for bit its views in sequence, the filtered mesh is mesh_filter_reference applied to the unfiltered one exactly, and the
call without any new keyword gives the bits of the call sequence it made before the keywords existed.

Printed, not asserted: | |v| - 1 | in voxels without the floater.  Measured on one MI355X: expected depth median 1.053,
maximum 3.335 (6 % of the vertices inside the sphere); median depth 1.029 and 3.525 (2 % inside) -- the splats are opaque
and overlap, so both depths sit on the front of the shell.  With the floater the meshes have 18 (expected) and 25 (median)
components, and keep_largest=1 takes 22 114 faces to 21 784 and 21 022 to 20 432."""
import numpy as np
import pytest

import mesh_filter_reference as mfr
import tsdf_reference as tr
from conftest import pkg

pytestmark = pytest.mark.gpu

BOX = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _setup(torch, scene, floater):
    raster = pkg("raster")
    rng = np.random.default_rng(11)
    n = 2000
    xyz = rng.normal(size=(n, 3))
    xyz = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(np.float32)
    rgb = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    if floater:
        blob = (np.array([0.0, 0.0, 1.3]) + 0.03 * np.random.default_rng(12).normal(size=(40, 3))).astype(np.float32)
        xyz = np.concatenate([xyz, blob])
        rgb = np.concatenate([rgb, np.full((40, 3), 0.5, np.float32)])
        n += 40
    params = dict(xyz=xyz, rgb=rgb, sh=np.zeros((n, 0, 3), np.float32), opacity=np.full(n, 4.0, np.float32),
                  scale=np.full((n, 3), np.log(0.06), np.float32),
                  quaternion=np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)))
    W, H = 64, 48
    views = []
    for eye in ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3)):
        cam = scene.make_camera(W, H, 0)
        m = tr.look_at(eye, (0, 0, 0), up=(0.0, 1.0, 0.0) if eye[1] == 0 else (0.0, 0.0, 1.0))
        cam["view"] = np.concatenate([m, np.array([0, 0, 0, 1], np.float32)])
        cam["campos"] = np.asarray(eye, np.float32)
        views.append((raster.device_camera(cam), torch.zeros(H, W, 3, device="cuda")))
    return raster.device_params(params), views


@pytest.fixture(scope="module")
def floater_case(gpu, scene):
    """The trainer of the sphere with the floater, its median, T and image maps per view, and the view matrices."""
    torch, ops, trainer_mod = gpu, pkg("ops"), pkg("trainer")
    dp, views = _setup(torch, scene, floater=True)
    t = trainer_mod.Trainer(dp, views, None, scene_extent=1.5, seed=3)
    ctx = t.ctx
    ctx.set_render_only(True)
    maps = []
    for cam, _ in views:
        fwd = ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)
        maps.append((_np(ctx.median_depth(0.5)).copy(), _np(fwd["T"]).copy(), _np(fwd["image"]).copy()))
    ctx.set_render_only(False)
    view = np.stack([_np(cam["view"]).reshape(-1)[:12] for cam, _ in views])
    intr = np.asarray([ops.pixel_intrinsics(cam) for cam, _ in views], np.float32)
    return dict(t=t, views=views, maps=maps, view=view, intr=intr, alpha_min=float(t.cfg["normal_alpha_min"]))


def _gated(T, alpha_min):
    """T' of the reference: 0 where the surface form's opacity gate 1 - T >= alpha_min passes, 1 elsewhere."""
    ok = (1.0 - T.astype(np.float64)) >= float(np.float32(alpha_min))
    return np.where(ok, 0.0, 1.0).astype(np.float32)


def _assert_mesh_close(got, ref_v, ref_f, ref_c, ends, color_ends):
    v, faces, colors = (_np(t) for t in got)
    assert v.dtype == np.float32 and faces.dtype == np.int32
    assert faces.shape == ref_f.shape and np.array_equal(faces, ref_f)
    assert v.shape == ref_v.shape
    assert (np.abs(v.astype(np.float64) - ref_v.astype(np.float64)) <= 1e-6 * np.abs(ends).sum(1) + 1e-12).all()
    assert colors.shape == ref_c.shape
    assert (np.abs(colors.astype(np.float64) - ref_c.astype(np.float64)) <= 1e-6 * np.abs(color_ends).sum(1) + 1e-12).all()


def test_median_mesh_equals_the_reference_pipeline(gpu, floater_case, tmp_path):
    torch, mesh = gpu, pkg("mesh")
    case, t = floater_case, floater_case["t"]
    ctx = t.ctx
    modes = (ctx._depth, ctx._depth_inverse, ctx._depth_moment)
    assert not modes[0]
    path = str(tmp_path / "median.ply")
    got = t.extract_mesh(path=path, resolution=32, bounds=BOX, depth="median")
    assert (ctx._depth, ctx._depth_inverse, ctx._depth_moment) == modes  # and depth mode was never needed
    assert got["filter"] is None
    vol = got["volume"]
    assert vol["dims"] == (33, 33, 33) and len(got["faces"]) > 500
    maps = case["maps"]
    zero = dict(tsdf=np.zeros((33, 33, 33), np.float32), weight=np.zeros((33, 33, 33), np.float32),
                color=np.zeros((33, 33, 33, 3), np.float32))
    ref = tr.integrate(zero, vol["origin"], vol["voxel"], vol["dims"], np.stack([m[0] for m in maps]),
                       np.stack([_gated(m[1], case["alpha_min"]) for m in maps]), np.stack([m[2] for m in maps]),
                       case["view"], case["intr"], False, case["alpha_min"], 4.0 * vol["voxel"])
    assert np.array_equal(_np(vol["weight"]), ref["weight"]) and ref["weight"].max() >= 1
    err = np.abs(_np(vol["tsdf"]).astype(np.float64) - ref["tsdf"].astype(np.float64))
    assert (err <= 1e-6 * ref["bound_tsdf"] + 1e-12).all()
    err = np.abs(_np(vol["color"]).astype(np.float64) - ref["color"].astype(np.float64))
    assert (err <= 1e-6 * ref["bound_color"] + 1e-12).all()
    ref_v, ref_f, ref_c, ends, color_ends = tr.extract(_np(vol["tsdf"]), _np(vol["weight"]), _np(vol["color"]),
                                                       vol["origin"], vol["voxel"])
    _assert_mesh_close((got["vertices"], got["faces"], got["colors"]), ref_v, ref_f, ref_c, ends, color_ends)
    if np.array_equal(_np(vol["tsdf"]) < 0, ref["tsdf"] < 0):
        assert np.array_equal(tr.extract(ref["tsdf"], ref["weight"], ref["color"], vol["origin"], vol["voxel"])[1], ref_f)
    v2, f2, _ = mesh.load_ply(path)
    assert np.array_equal(v2, _np(got["vertices"])) and np.array_equal(f2, _np(got["faces"]))
    # not the expected-depth mesh
    expected = t.extract_mesh(resolution=32, bounds=BOX)
    assert not torch.equal(expected["volume"]["tsdf"], vol["tsdf"])
    with pytest.raises(ValueError):
        t.extract_mesh(resolution=32, bounds=BOX, depth="mode")


def test_surface_integration_matches_the_reference_and_its_views_in_sequence(gpu, floater_case):
    torch, ops = gpu, pkg("ops")
    case = floater_case
    order = [0, 1, 2, 3, 4, 5, 0, 1, 2]  # K = 9: a full pass of 8 and a remainder
    depth = np.stack([case["maps"][v][0] for v in order])
    T = np.stack([case["maps"][v][1] for v in order])
    image = np.stack([case["maps"][v][2] for v in order])
    view, intr = case["view"][order], case["intr"][order]
    origin, voxel, dims = (-1.5, -1.5, -1.5), 3.0 / 32.0, (33, 33, 33)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()

    def run(lo, hi, vol=None, t_maps=T, **kw):
        vol = ops.tsdf_volume(origin, voxel, dims, color=True) if vol is None else vol
        return ops.tsdf_integrate(vol, dev(depth[lo:hi]), None if t_maps is None else dev(t_maps[lo:hi]), view[lo:hi],
                                  intr[lo:hi], image=dev(image[lo:hi]), alpha_min=case["alpha_min"], max_weight=5.0,
                                  surface=True, **kw)

    whole = run(0, 9)
    zero = dict(tsdf=np.zeros(dims[::-1], np.float32), weight=np.zeros(dims[::-1], np.float32),
                color=np.zeros(dims[::-1] + (3,), np.float32))
    ref = tr.integrate(zero, whole["origin"], whole["voxel"], dims, depth, _gated(T, case["alpha_min"]), image, view, intr,
                       False, case["alpha_min"], 4.0 * whole["voxel"], max_weight=5.0)
    assert np.array_equal(_np(whole["weight"]), ref["weight"]) and ref["weight"].max() == 5.0
    err = np.abs(_np(whole["tsdf"]).astype(np.float64) - ref["tsdf"].astype(np.float64))
    assert (err <= 1e-6 * ref["bound_tsdf"] + 1e-12).all()
    err = np.abs(_np(whole["color"]).astype(np.float64) - ref["color"].astype(np.float64))
    assert (err <= 1e-6 * ref["bound_color"] + 1e-12).all()
    single = run(0, 1)
    for v in range(1, 9):
        run(v, v + 1, vol=single)
    split = run(4, 9, vol=run(0, 4))
    for other in (run(0, 9), single, split):
        assert all(torch.equal(whole[k], other[k]) for k in ("tsdf", "weight", "color"))
    # T = None: no opacity gate -- what an all-zero T gives; an all-one T closes the gate everywhere
    ungated, zeros = run(0, 9, t_maps=None), run(0, 9, t_maps=np.zeros_like(T))
    assert all(torch.equal(ungated[k], zeros[k]) for k in ("tsdf", "weight", "color"))
    assert float(ungated["weight"].max()) == 5.0 and float(run(0, 9, t_maps=np.ones_like(T))["weight"].max()) == 0.0
    with pytest.raises(ValueError):
        run(0, 9, inverse=True)
    with pytest.raises(ValueError):
        ops.tsdf_integrate(ops.tsdf_volume(origin, voxel, dims, color=False), dev(depth), None, view, intr)


def test_keep_largest_leaves_the_sphere(gpu, floater_case):
    torch, ops = gpu, pkg("ops")
    t = floater_case["t"]
    for depth in ("median", "expected"):
        full = t.extract_mesh(resolution=32, bounds=BOX, depth=depth)
        kept = t.extract_mesh(resolution=32, bounds=BOX, depth=depth, keep_largest=1)
        assert 0 < len(kept["faces"]) < len(full["faces"]), depth
        label, count = mfr.components(_np(kept["faces"]), len(kept["vertices"]))
        assert (label == 0).all() and count[0] == len(kept["faces"]), depth  # exactly one component
        ref = mfr.mesh_filter(_np(full["vertices"]), _np(full["faces"]), _np(full["colors"]), keep_largest=1)
        assert np.array_equal(_np(kept["vertices"]).view(np.uint32), ref[0].view(np.uint32))
        assert np.array_equal(_np(kept["faces"]), ref[1])
        assert np.array_equal(_np(kept["colors"]).view(np.uint32), ref[2].view(np.uint32))
        assert kept["filter"] == ref[3] and ref[3]["kept"] == 1 and ref[3]["components"] >= 2
        print(f"{depth}: {ref[3]['components']} components, {len(full['faces'])} -> {len(kept['faces'])} faces")
        small = t.extract_mesh(resolution=32, bounds=BOX, depth=depth, min_component_faces=len(kept["faces"]))
        assert torch.equal(small["faces"], kept["faces"]) and torch.equal(small["vertices"], kept["vertices"])


def test_defaults_give_the_bits_of_the_call_sequence_before(gpu, floater_case):
    """extract_mesh() with no new keyword against the calls it made before the keywords existed: depth mode on the
    render-only context, the expected depth and T stacked four views at a time, tsdf_integrate, tsdf_extract."""
    torch, ops = gpu, pkg("ops")
    case, t = floater_case, floater_case["t"]
    got = t.extract_mesh(resolution=32, bounds=BOX)
    ctx = t.ctx
    inverse = bool(t.cfg["distortion_inverse"])
    vol = ops.tsdf_volume(BOX[0], 3.0 / 32.0, (33, 33, 33), color=True)
    ctx.set_render_only(True)
    ctx.set_depth(True, inverse=inverse)
    try:
        for lo in (0, 4):
            d, T, im = [], [], []
            for cam, _ in case["views"][lo:lo + 4]:
                fwd = ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)
                d.append(fwd["depth"].clone()); T.append(fwd["T"].clone()); im.append(fwd["image"].clone())
            ops.tsdf_integrate(vol, torch.stack(d), torch.stack(T), case["view"][lo:lo + 4], case["intr"][lo:lo + 4],
                               image=torch.stack(im), inverse=inverse, alpha_min=case["alpha_min"],
                               trunc=4.0 * vol["voxel"], near=0.0, max_depth=0.0)
    finally:
        ctx.set_depth(False)
        ctx.set_render_only(False)
    v, f, c = ops.tsdf_extract(vol, min_weight=1.0)
    assert all(torch.equal(vol[k], got["volume"][k]) for k in ("tsdf", "weight", "color"))
    assert torch.equal(v, got["vertices"]) and torch.equal(f, got["faces"]) and torch.equal(c, got["colors"])
    assert got["filter"] is None


def test_distance_from_the_sphere_printed(gpu, scene):
    torch, trainer_mod = gpu, pkg("trainer")
    dp, views = _setup(torch, scene, floater=False)
    t = trainer_mod.Trainer(dp, views, None, scene_extent=1.5, seed=3)
    for depth in ("expected", "median"):
        got = t.extract_mesh(resolution=32, bounds=BOX, depth=depth)
        off = np.abs(np.linalg.norm(_np(got["vertices"]).astype(np.float64), axis=1) - 1.0) / got["volume"]["voxel"]
        inside = float((np.linalg.norm(_np(got["vertices"]).astype(np.float64), axis=1) < 1.0).mean())
        print(f"sphere mesh, depth {depth}: {len(got['vertices'])} vertices, {len(got['faces'])} faces, "
              f"| |v| - 1 | median {np.median(off):.3f} max {off.max():.3f} voxels, {100 * inside:.0f} % inside the sphere")
        assert len(got["faces"]) > 500

"""gsplat_tsdf_integrate and the marching-tetrahedra extraction (gsplat_tsdf_mark / gsplat_tsdf_emit) against their numpy
float64 versions (tests/tsdf_reference.py), and Trainer.extract_mesh end to end.

Integration: every element of tsdf and color is held to 1e-6 x (|old| + |val|) + 1e-12 of its last update, weights are
equal exactly, no node is excluded -- tests/test_tsdf_cpu.py asserts that every decision of these cases sits at least 1e-9
from its boundary.  Grids 1x1x1, 3x5x7, 33x17x9 and 65x2x2 (either side of a wave of 64 along x), images 1x1, 5x3 and
40x24, K = 1, 2, 5, 9 (one pass holds 8 views: 9 is a full pass and a remainder), inverse, colour, max_depth and
max_weight on and off, a camera behind the volume and one whose frustum misses it.  A batch is bit for bit its views one
call at a time; refused arguments leave sentinel-filled arrays untouched.

Extraction: faces equal element for element, vertices and colours within 1e-6 x (|p_a| + |p_b|) + 1e-12, two runs the
same bits.

End to end: 2000 small opaque gaussians on the unit sphere, six cameras on the axes at distance 3, 64x48; the mesh equals
the reference pipeline run on the GPU's own depth and T maps.  Measured on one MI355X: | |v| - 1 | of the mesh's vertices
has median 1.05 and maximum 3.34 voxels at resolution 32 (printed, not asserted): the expected depth of 0.06-wide splats
lies in front of their centres."""
import ctypes

import numpy as np
import pytest

import tsdf_reference as tr
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = tr.integration_cases()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _volume(torch, ops, case, state):
    vol = ops.tsdf_volume(case["origin"], case["voxel"], case["dims"], color=state["color"] is not None)
    for k in ("tsdf", "weight", "color"):
        if state[k] is not None:
            vol[k].copy_(torch.as_tensor(state[k]))
    return vol


def _integrate(torch, ops, vol, case, lo=0, hi=None):
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a[lo:hi])).cuda()
    return ops.tsdf_integrate(vol, dev(case["depth"]), dev(case["T"]), case["view"][lo:hi], case["intrinsics"][lo:hi],
                              image=dev(case["image"]), inverse=case["inverse"], alpha_min=case["alpha_min"],
                              trunc=case["trunc"], near=case["near"], max_depth=case["max_depth"],
                              max_weight=case["max_weight"])


@pytest.fixture(scope="module")
def references():
    return {name: (tr.start_state(c), tr.run_reference(c, tr.start_state(c))) for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_integrate_matches_the_reference(gpu, references, name):
    torch, ops = gpu, pkg("ops")
    case = CASES[name]
    start, ref = references[name]
    vol = _integrate(torch, ops, _volume(torch, ops, case, start), case)
    assert np.array_equal(_np(vol["weight"]), ref["weight"])
    err = np.abs(_np(vol["tsdf"]).astype(np.float64) - ref["tsdf"].astype(np.float64))
    tol = 1e-6 * ref["bound_tsdf"] + 1e-12
    print(f"{name}: tsdf max err/tol {float((err / tol).max()):.3g}, updated {int((ref['bound_tsdf'] > 0).sum())}")
    assert (err <= tol).all(), float((err / tol).max())
    if case["image"] is not None:
        err = np.abs(_np(vol["color"]).astype(np.float64) - ref["color"].astype(np.float64))
        tol = 1e-6 * ref["bound_color"] + 1e-12
        assert (err <= tol).all(), float((err / tol).max())
    if name in ("behind", "miss"):
        assert all(np.array_equal(_np(vol[k]), start[k]) for k in ("tsdf", "weight", "color"))


@pytest.mark.parametrize("name", ["K9_color_limits", "K9_inverse_plain"])
def test_a_batch_is_bit_for_bit_its_views_in_sequence(gpu, name):
    torch, ops = gpu, pkg("ops")
    case = CASES[name]
    assert case["K"] == 9
    start = tr.start_state(case)
    keys = ("tsdf", "weight") + (("color",) if case["image"] is not None else ())
    whole = _integrate(torch, ops, _volume(torch, ops, case, start), case)
    again = _integrate(torch, ops, _volume(torch, ops, case, start), case)
    single = _volume(torch, ops, case, start)
    for v in range(9):
        _integrate(torch, ops, single, case, v, v + 1)
    split = _volume(torch, ops, case, start)
    _integrate(torch, ops, split, case, 0, 4)
    _integrate(torch, ops, split, case, 4, 9)
    for other in (again, single, split):
        assert all(torch.equal(whole[k], other[k]) for k in keys)
    assert not torch.equal(whole["tsdf"], torch.as_tensor(start["tsdf"]).cuda())


def test_bad_arguments_are_refused_before_any_launch(gpu):
    torch, ops, lib_mod = gpu, pkg("ops"), pkg("_lib")
    lib = lib_mod.load()
    nx, ny, nz, K, H, W = 5, 4, 3, 2, 6, 7
    full = lambda *s: torch.full(s, 7.0, device="cuda")
    tsdf, weight, color = full(nz, ny, nx), full(nz, ny, nx), full(nz, ny, nx, 3)
    depth, T, image = full(K, H, W), full(K, H, W) * 0 + 0.25, full(K, H, W, 3)
    origin = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    view = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (K, 1))
    intr = np.tile(np.array([5.0, 5.0, 3.0, 3.0], np.float32), (K, 1))
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    hp = lambda a: None if a is None else a.ctypes.data

    def call(**kw):
        a = dict(tsdf=tsdf, weight=weight, color=color, nx=nx, ny=ny, nz=nz, origin=origin, voxel=0.1, depth=depth, T=T,
                 image=image, view=view, intr=intr, K=K, H=H, W=W, inverse=0, alpha_min=0.5, trunc=0.4, near=0.0,
                 max_depth=0.0, max_weight=0.0)
        a.update(kw)
        return lib.gsplat_tsdf_integrate(p(a["tsdf"]), p(a["weight"]), p(a["color"]), a["nx"], a["ny"], a["nz"],
                                         a["origin"], a["voxel"], p(a["depth"]), p(a["T"]), p(a["image"]), hp(a["view"]),
                                         hp(a["intr"]), a["K"], a["H"], a["W"], a["inverse"], a["alpha_min"], a["trunc"],
                                         a["near"], a["max_depth"], a["max_weight"], st)

    def bad_intr(col, value):
        b = intr.copy()
        b[1, col] = value
        return b

    rows = dict(
        nx0=dict(nx=0), ny_negative=dict(ny=-1), nz0=dict(nz=0), H0=dict(H=0), W_negative=dict(W=-3), K_negative=dict(K=-1),
        voxel0=dict(voxel=0.0), voxel_negative=dict(voxel=-0.1), voxel_inf=dict(voxel=float("inf")),
        voxel_nan=dict(voxel=float("nan")), trunc0=dict(trunc=0.0), trunc_negative=dict(trunc=-1.0),
        trunc_nan=dict(trunc=float("nan")), trunc_inf=dict(trunc=float("inf")),
        alpha0=dict(alpha_min=0.0), alpha_above_1=dict(alpha_min=1.5), alpha_nan=dict(alpha_min=float("nan")),
        fx0=dict(intr=bad_intr(0, 0.0)), fy0=dict(intr=bad_intr(1, 0.0)), cx_nan=dict(intr=bad_intr(2, float("nan"))),
        cy_inf=dict(intr=bad_intr(3, float("inf"))), fx_inf=dict(intr=bad_intr(0, float("inf"))),
        no_tsdf=dict(tsdf=None), no_weight=dict(weight=None), no_origin=dict(origin=None), no_depth=dict(depth=None),
        no_T=dict(T=None), no_view=dict(view=None), no_intrinsics=dict(intr=None),
        image_without_color=dict(color=None), color_without_image=dict(image=None),
        too_many_nodes=dict(nx=2048, ny=2048, nz=512),
    )
    codes = {name: call(**kw) for name, kw in rows.items()}
    torch.cuda.synchronize()
    assert codes == {name: -3 for name in rows}, codes  # GSPLAT_ERR_INVALID_ARG
    assert "invalid argument" in lib.gsplat_last_error().decode()
    assert all(bool((t == 7.0).all()) for t in (tsdf, weight, color))
    assert call(K=0) == 0 and call(K=0, depth=None, T=None, image=None, color=None, view=None, intr=None) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (tsdf, weight, color))
    # the Python surface: shapes, dtypes and placement
    vol = dict(tsdf=tsdf, weight=weight, color=color, origin=(0.0, 0.0, 1.0), voxel=0.1, dims=(nx, ny, nz))
    bad = (
        lambda: ops.tsdf_integrate(vol, depth, T, view, intr),                                        # colour, no image
        lambda: ops.tsdf_integrate(dict(vol, color=None), depth, T, view, intr, image=image),        # image, no colour
        lambda: ops.tsdf_integrate(vol, depth[:, :-1].contiguous(), T, view, intr, image=image),
        lambda: ops.tsdf_integrate(vol, depth.double(), T, view, intr, image=image),
        lambda: ops.tsdf_integrate(vol, depth, T, view[:, :11], intr, image=image),
        lambda: ops.tsdf_integrate(vol, depth, T, view, intr[:1], image=image),
        lambda: ops.tsdf_integrate(dict(vol, dims=(nx, ny, nz + 1)), depth, T, view, intr, image=image),
        lambda: ops.tsdf_integrate(dict(vol, weight=weight.cpu()), depth, T, view, intr, image=image),
        lambda: ops.tsdf_extract(dict(vol, tsdf=tsdf[:, :, :-1])),
        lambda: ops.tsdf_volume((0, 0, 0), 0.0, (2, 2, 2)),
        lambda: ops.tsdf_volume((0, 0, 0), 0.1, (2, 0, 2)),
    )
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(lib_mod.GsplatError) as e:
        ops.tsdf_integrate(vol, depth, T, view, intr, image=image, alpha_min=0.0)
    assert e.value.code == -3
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (tsdf, weight, color))
    # extraction: the library's own checks
    n = nx * ny * nz
    u8 = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    i32 = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    i64 = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = full(4, 3)
    faces = torch.full((4, 3), 7, dtype=torch.int32, device="cuda")
    codes = [lib.gsplat_tsdf_mark(p(tsdf), p(weight), 0, ny, nz, 1.0, p(u8), p(i32), p(u8), p(i32), st),
             lib.gsplat_tsdf_mark(p(tsdf), None, nx, ny, nz, 1.0, p(u8), p(i32), p(u8), p(i32), st),
             lib.gsplat_tsdf_mark(p(tsdf), p(weight), nx, ny, nz, float("nan"), p(u8), p(i32), p(u8), p(i32), st),
             lib.gsplat_tsdf_mark(p(tsdf), p(weight), nx, ny, nz, 1.0, p(u8), None, p(u8), p(i32), st),
             lib.gsplat_tsdf_emit(p(tsdf), None, nx, ny, nz, origin, 0.0, p(u8), p(u8), p(i64), p(i64), 4, 4, p(out), None,
                                  p(faces), st),
             lib.gsplat_tsdf_emit(p(tsdf), None, nx, ny, nz, origin, 0.1, p(u8), p(u8), p(i64), p(i64), -1, 4, p(out), None,
                                  p(faces), st),
             lib.gsplat_tsdf_emit(p(tsdf), None, nx, ny, nz, origin, 0.1, p(u8), p(u8), p(i64), p(i64), 4, 4, None, None,
                                  p(faces), st),
             lib.gsplat_tsdf_emit(p(tsdf), None, nx, ny, nz, origin, 0.1, p(u8), p(u8), None, p(i64), 4, 4, p(out), None,
                                  p(faces), st)]
    torch.cuda.synchronize()
    assert codes == [-3] * len(codes), codes
    assert bool((u8 == 7).all()) and bool((i32 == 7).all()) and bool((out == 7.0).all()) and bool((faces == 7).all())


@pytest.fixture(scope="module")
def field_meshes():
    out = {}
    for name in tr.FIELDS:
        f = tr.field(name)
        out[name] = (f,) + tr.extract(f["tsdf"], f["weight"], f["color"], f["origin"], f["voxel"])
    return out


def _assert_mesh_close(got, ref_v, ref_f, ref_c, ends, color_ends):
    v, faces, colors = (_np(t) for t in got)
    assert v.dtype == np.float32 and faces.dtype == np.int32
    assert faces.shape == ref_f.shape and np.array_equal(faces, ref_f)
    assert v.shape == ref_v.shape
    tol = 1e-6 * np.abs(ends).sum(1) + 1e-12
    assert (np.abs(v.astype(np.float64) - ref_v.astype(np.float64)) <= tol).all()
    if ref_c is None:
        assert colors is None
    else:
        assert colors.shape == ref_c.shape
        tol = 1e-6 * np.abs(color_ends).sum(1) + 1e-12
        assert (np.abs(colors.astype(np.float64) - ref_c.astype(np.float64)) <= tol).all()


@pytest.mark.parametrize("name", tr.FIELDS)
@pytest.mark.parametrize("with_color", [True, False])
def test_extract_matches_the_reference(gpu, field_meshes, name, with_color):
    torch, ops = gpu, pkg("ops")
    f, ref_v, ref_f, ref_c, ends, color_ends = field_meshes[name]
    vol = ops.tsdf_volume(f["origin"], f["voxel"], f["dims"], color=with_color)
    vol["tsdf"].copy_(torch.as_tensor(f["tsdf"]))
    vol["weight"].copy_(torch.as_tensor(f["weight"]))
    if with_color:
        vol["color"].copy_(torch.as_tensor(f["color"]))
    got = ops.tsdf_extract(vol)
    _assert_mesh_close(got, ref_v, ref_f, ref_c if with_color else None, ends, color_ends)
    again = ops.tsdf_extract(vol)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, again))
    if name == "positive":
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    if name == "sphere":  # a higher bar for the weight: nothing is observed often enough
        assert ops.tsdf_extract(vol, min_weight=2.0)[1].shape == (0, 3)


def _sphere_setup(torch, scene):
    raster = pkg("raster")
    rng = np.random.default_rng(11)
    n = 2000
    xyz = rng.normal(size=(n, 3))
    xyz = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(np.float32)
    params = dict(xyz=xyz, rgb=rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32), sh=np.zeros((n, 0, 3), np.float32),
                  opacity=np.full(n, 4.0, np.float32), scale=np.full((n, 3), np.log(0.06), np.float32),
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


def test_extract_mesh_end_to_end(gpu, scene, tmp_path):
    torch, ops, trainer_mod, mesh = gpu, pkg("ops"), pkg("trainer"), pkg("mesh")
    dp, views = _sphere_setup(torch, scene)
    t = trainer_mod.Trainer(dp, views, None, scene_extent=1.5, seed=3)
    box = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    path = str(tmp_path / "sphere.ply")
    ctx = t.ctx
    modes = (ctx._depth, ctx._depth_inverse, ctx._depth_moment)
    got = t.extract_mesh(path=path, resolution=32, bounds=box)
    assert (ctx._depth, ctx._depth_inverse, ctx._depth_moment) == modes
    vol = got["volume"]
    assert vol["dims"] == (33, 33, 33) and abs(vol["voxel"] - 3.0 / 32.0) < 1e-7
    assert len(got["faces"]) > 500 and len(got["vertices"]) > 250
    # the reference pipeline on the GPU's own maps
    inverse = bool(t.cfg["distortion_inverse"])
    ctx.set_render_only(True)
    ctx.set_depth(True, inverse=inverse)
    maps = []
    for cam, _ in views:
        fwd = ctx.rasterize_image(dict(t.params), cam, t.cfg, 0.0, t.l_max)
        maps.append((_np(fwd["depth"]).copy(), _np(fwd["T"]).copy(), _np(fwd["image"]).copy()))
    ctx.set_depth(False)
    ctx.set_render_only(False)
    view = np.stack([_np(cam["view"]).reshape(-1)[:12] for cam, _ in views])
    intr = np.asarray([ops.pixel_intrinsics(cam) for cam, _ in views], np.float32)
    zero = dict(tsdf=np.zeros((33, 33, 33), np.float32), weight=np.zeros((33, 33, 33), np.float32),
                color=np.zeros((33, 33, 33, 3), np.float32))
    ref = tr.integrate(zero, vol["origin"], vol["voxel"], vol["dims"], np.stack([m[0] for m in maps]),
                       np.stack([m[1] for m in maps]), np.stack([m[2] for m in maps]), view, intr, inverse,
                       float(t.cfg["normal_alpha_min"]), 4.0 * vol["voxel"])
    assert np.array_equal(_np(vol["weight"]), ref["weight"])
    ref_v, ref_f, ref_c, ends, color_ends = tr.extract(_np(vol["tsdf"]), _np(vol["weight"]), _np(vol["color"]), vol["origin"], vol["voxel"])
    _assert_mesh_close((got["vertices"], got["faces"], got["colors"]), ref_v, ref_f, ref_c, ends, color_ends)
    # ... and from the reference's own volume: the same faces unless a node's sign sits within rounding of 0
    err = np.abs(_np(vol["tsdf"]).astype(np.float64) - ref["tsdf"].astype(np.float64))
    assert (err <= 1e-6 * ref["bound_tsdf"] + 1e-12).all()
    if np.array_equal(_np(vol["tsdf"]) < 0, ref["tsdf"] < 0):
        assert np.array_equal(tr.extract(ref["tsdf"], ref["weight"], ref["color"], vol["origin"], vol["voxel"])[1], ref_f)
    # the PLY, and a second call
    v2, f2, c2 = mesh.load_ply(path)
    assert np.array_equal(v2, _np(got["vertices"])) and np.array_equal(f2, _np(got["faces"]))
    assert np.array_equal(c2, np.floor(np.clip(_np(got["colors"]).astype(np.float64), 0, 1) * 255.0 + 0.5).astype(np.uint8))
    again = t.extract_mesh(resolution=32, bounds=box)
    assert all(torch.equal(got[k], again[k]) for k in ("vertices", "faces", "colors"))
    assert all(torch.equal(vol[k], again["volume"][k]) for k in ("tsdf", "weight", "color"))
    other = t.extract_mesh(resolution=32, bounds=box, batch=8, color=False)  # another batching: the same bits
    assert other["colors"] is None and torch.equal(other["vertices"], got["vertices"]) and torch.equal(other["faces"], got["faces"])
    rep = mesh.edge_report(_np(got["faces"]))
    off = np.abs(np.linalg.norm(_np(got["vertices"]).astype(np.float64), axis=1) - 1.0) / vol["voxel"]
    print(f"sphere mesh: {len(got['vertices'])} vertices, {len(got['faces'])} faces, edges {rep}, "
          f"| |v| - 1 | median {np.median(off):.3f} max {off.max():.3f} voxels")

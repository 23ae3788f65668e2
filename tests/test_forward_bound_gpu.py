"""Every output of the HIP forward, bounded by its own float64 condition sum (tests/forward_reference.py).

Each test runs one forward of a non-lean context (sigma, J, conic and rgb are stored) and holds

  stage A  xyz_c, uv, sigma, J, conic, rgb of the compacted rows against the float64 values derived from the scene's
           float32 parameters and camera; the keep mask, the ceil'ed radii, (sin, cos) and the tile lists against the
           float64 decisions (the lists: orc.get_sorted_gaussian_list on the GPU's own uv, xyz_c and radius);
  stage B  image, T, n (depth, depth2, alpha in depth mode) against the float64 compositing of the GPU's OWN uv, conic,
           rgb and lists,

every element to  |got - value64| <= 4 max(1, K_obs) u unit + borderline  (tests/grad_bound.py), K_obs the float32 oracle's
figure for the scene and array (tests/test_forward_bound_cpu.py: K_OBS).  Every worst ratio is printed before anything is
asserted (pytest -s); CHANGELOG.md keeps the figures the kernels reached."""
import hashlib

import numpy as np
import pytest

import edge_scenes
import forward_bound_cases as fc
import forward_reference as fr
import grad_bound
import grad_bound_cases as gc
from conftest import pkg
from test_forward_bound_cpu import K_OBS, K_OBS_EDGE

pytestmark = pytest.mark.gpu
MARGIN = grad_bound.GPU_MARGIN
RECORD = ("mask", "compact_to_global", "xyz_c", "uv", "sigma", "J", "conic", "rgb", "radius", "sorted", "ranges", "image", "T", "n")
_LONG_TERMS = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _forward(torch, case, ctx, extra=()):
    """One forward of `ctx` as numpy arrays, and the global rows of its compacted ones."""
    raster = pkg("raster")
    fwd = ctx.rasterize_image(raster.device_params(case["params"]), raster.device_camera(case["cam"]), case["cfg"],
                              case["bg"], case["L"])
    torch.cuda.synchronize()
    rec = {k: _np(fwd[k]).copy() for k in RECORD + tuple(extra)}
    rec["num_culled"] = int(fwd["num_culled"])
    return rec, rec["compact_to_global"].astype(np.int64)


def _hold_a(case, rec, rows, orc, what, table=None):
    """Stage A of one forward: prints the figures, returns the failures."""
    table = table or K_OBS[case["name"]]
    failures, line = fc.hold_stage_a(case, rec, rows, table, MARGIN, what)
    mf, free = fc.hold_mask(case, rec["mask"], table, MARGIN, what)
    lf, lfig = fr.list_failures(orc, rec, case["W"], case["H"])
    print(f"[forward bound {what}] stage A worst ratio / bound (u*unit): {line}; {free} rows within a bar of a cull bound; "
          f"{lfig['differ']} list instances differ from the oracle's on the same uv, xyz_c, radius")
    if rec["num_culled"] != int(rec["mask"].astype(bool).sum()) or len(rows) != rec["num_culled"]:
        failures.append(f"{what}: num_culled {rec['num_culled']} against {int(rec['mask'].astype(bool).sum())} kept rows")
    elif not (rows == np.nonzero(rec["mask"])[0]).all():
        failures.append(f"{what}: compact_to_global is not the kept rows in order")
    return failures + mf + [f"{what}: {m}" for m in lf]


def _hold_b(case, rec, t, what, table=None):
    failures, line = fc.hold_stage_b(t, rec, table or K_OBS[case["name"]], MARGIN, what)
    print(f"[forward bound {what}] stage B worst ratio / bound (u*unit): {line}")
    return failures


def _run_scene(torch, orc, name):
    case = gc.make(name)
    ctx = pkg("raster").RasterContext(len(case["params"]["xyz"]), case["W"], case["H"])
    rec, rows = _forward(torch, case, ctx)
    ctx.close()
    failures = _hold_a(case, rec, rows, orc, name) + _hold_b(case, rec, fc.stage_b_terms(case, rec, rows), name)
    assert not failures, "\n".join(failures)
    return case, rec, rows


@pytest.mark.parametrize("name", list(gc.BASIC))
def test_basic_sizes(gpu, orc, name):
    """tiny and small at views 0 and 2; SH 0, 1, 2 at 3000 gaussians, 200x120; 1 gaussian at 17x9, 37 at 100x7, 257 at
    130x66 (SH 3)."""
    _run_scene(gpu, orc, name)


def test_culled_rows_interleaved(gpu, orc):
    """small through scene.cull_half: scattered kept rows and a partial last wave; the culled rows' decisions too."""
    case, rec, rows = _run_scene(gpu, orc, "culled")
    assert 0 < len(rows) < len(case["params"]["xyz"]) and len(rows) % 64 != 0 and (np.diff(rows) > 1).any()


def test_long_lists_whole_and_segmented(gpu, orc):
    """The long-list scene (24 000 gaussians at 160x96, lists of 2 100 .. 7 000 entries), forwards 0 to 3 of one context:
    forward 3 walks the lists beyond 1 488 entries in segments (counters()), and its unit carries the combine's
    roundings; then two more contexts whose segments obtain their prefix transmittance in other ways."""
    case = gc.make("long")
    N, W, H = len(case["params"]["xyz"]), case["W"], case["H"]
    failures = []

    def four_forwards(ctx, what, only_last):
        for it in range(4):
            rec, rows = _forward(gpu, case, ctx)
            assert ctx.counters()["segmented_forwards"] == max(0, it - 2)
            if only_last and it < 3:
                continue
            segmented = it == 3
            # the float64 walk costs seconds on this scene: once per distinct record (forwards 0 to 2 give the same bits)
            key = (segmented, hashlib.sha1(b"".join(rec[k].tobytes() for k in sorted(RECORD))).hexdigest())
            if key not in _LONG_TERMS:
                _LONG_TERMS[key] = (_hold_a(case, rec, rows, orc, f"{what}, forward {it}"),
                                    fc.stage_b_terms(case, rec, rows, segmented=segmented))
            fa, t = _LONG_TERMS[key]
            failures.extend(fa + _hold_b(case, rec, t, f"{what}, forward {it}"))

    ctx = pkg("raster").RasterContext(N, W, H)
    ctx.set_binning_route(1)
    four_forwards(ctx, "long lists", False)
    ctx.close()
    for what, opts in (("one poll, all layers side by side", dict(poll_budget=1, thin_layer_blocks=1 << 20)),
                       ("every workgroup waits for the one in front", dict(thin_layer_blocks=0))):
        other = pkg("raster").RasterContext(N, W, H)
        other.set_binning_route(1)
        other.set_segment_options(**opts)
        four_forwards(other, "long lists, " + what, True)
        other.close()
    assert not failures, "\n".join(failures)


def test_edge_scene_per_population(gpu, orc):
    """edge_scenes size small: stage A of every population to its own K (every visible row is in one of them), the mask,
    the lists and stage B on the whole scene."""
    case = gc.make("edge_fwd")
    ctx = pkg("raster").RasterContext(len(case["params"]["xyz"]), case["W"], case["H"])
    rec, rows = _forward(gpu, case, ctx)
    ctx.close()
    failures = _hold_a(case, rec, rows, orc, "edge") + _hold_b(case, rec, fc.stage_b_terms(case, rec, rows), "edge")
    for k, r in gc.populations_of(case, rows).items():
        if not len(r) or k == "culled":
            continue
        fa, line = fc.hold_stage_a(case, rec, rows, K_OBS_EDGE[k], MARGIN, f"edge [{k}]", r)
        print(f"[forward bound edge [{k}]] {line}")
        failures += fa
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("variant", list(fc.DEPTH_VARIANTS))
def test_depth_mode(gpu, orc, variant):
    """Depth mode on small, view 2: plain, inverse, inverse with the second moment -- depth, depth2 and alpha = 1 - T
    next to the image."""
    inverse, moment = fc.DEPTH_VARIANTS[variant]
    case = gc.make("depth")
    ctx = pkg("raster").RasterContext(len(case["params"]["xyz"]), case["W"], case["H"])
    ctx.set_depth(True, inverse=inverse, moment=moment)
    rec, rows = _forward(gpu, case, ctx, ("depth", "alpha") + (("depth2",) if moment else ()))
    ctx.close()
    failures = _hold_a(case, rec, rows, orc, variant)
    failures += _hold_b(case, rec, fc.stage_b_terms(case, rec, rows, variant), variant, K_OBS[variant])
    assert not failures, "\n".join(failures)


def test_standalone_operators(gpu, orc):
    """ops.project_to_screen, compute_sigma, compute_conic, precompute_spherical_harmonics and render_image on the float32
    oracle's arrays of small, view 2: the same bars (the inputs carry the oracle's roundings, the unit counts them)."""
    torch, ops = gpu, pkg("ops")
    case = gc.make("small_v2")
    ref, rows = fc.oracle_forward(case, orc)
    cam, W, H, L, M, N = case["cam"], case["W"], case["H"], case["L"], len(rows), len(case["params"]["xyz"])
    out = lambda *shape, dtype=torch.float32: torch.full(shape, float("nan") if dtype == torch.float32 else -1, dtype=dtype, device="cuda")
    uv_all = out(N, 2)
    ops.project_to_screen(_dev(torch, ref["xyz_c_all"]), _dev(torch, cam["proj"]), N, W, H, uv_all)
    sigma = out(M, 6)
    ops.compute_sigma(_dev(torch, ref["quaternion"]), _dev(torch, ref["scale"]), M, sigma)
    J, conic, radius = out(M, 6), out(M, 3), out(M, 4)
    tan_x, tan_y = (float(x) for x in edge_scenes.forward_tan_fov(cam))
    ops.compute_conic(_dev(torch, ref["xyz_c"]), _dev(torch, cam["view"]), _dev(torch, ref["sigma"]), float(cam["fx"]),
                      float(cam["fy"]), tan_x, tan_y, case["cfg"]["mh_dist"], M, J, conic, radius)
    rgb = out(M, 3)
    ops.precompute_spherical_harmonics(_dev(torch, ref["xyz"]), _dev(torch, ref["sh"]), _dev(torch, ref["band0"]),
                                       cam["campos"], L, M, rgb)
    n, T, image = out(H, W, dtype=torch.int32), out(H, W), out(H, W, 3)
    ops.render_image(*(_dev(torch, ref[k]) for k in ("uv", "opacity", "conic", "rgb")), case["bg"],
                     _dev(torch, ref["sorted"]), _dev(torch, ref["ranges"]), W, H, n, T, image)
    torch.cuda.synchronize()
    got = dict(uv=_np(uv_all)[rows], sigma=_np(sigma), J=_np(J), conic=_np(conic), radius=_np(radius), rgb=_np(rgb))
    failures, line = fc.hold_stage_a(case, got, rows, K_OBS["small_v2"], MARGIN, "stand-alone operators")
    print(f"[forward bound stand-alone operators] {line}")
    pg = fc.per_gaussian(case)  # and project_to_screen on the culled rows too
    failures_uv = []
    try:
        grad_bound.assert_within_bound(_np(uv_all), pg["uv"][0], pg["uv"][1], np.zeros_like(pg["uv"][1]),
                                       MARGIN * fc.K_of(K_OBS["small_v2"], "uv"), "stand-alone project_to_screen, all rows")
    except AssertionError as e:
        failures_uv.append(str(e))
    if "fwd_terms_b" not in case:
        case["fwd_terms_b"] = fc.stage_b_terms(case, ref, rows)
    fb = _hold_b(case, dict(n=_np(n), T=_np(T), image=_np(image)), case["fwd_terms_b"], "stand-alone render_image")
    assert not failures + failures_uv + fb, "\n".join(failures + failures_uv + fb)

"""Every gaussian's gradient from the HIP backward, bounded by its own float64 condition sum.

Each test runs the GPU forward, builds the float64 terms (tests/render_bwd_reference.py) from THAT forward's record
(uv, conic, rgb, lists, stop indices and final transmittances as the GPU produced them; opacity and the leaves from the
input parameters through compact_to_global), runs backward_pass with intermediates=True into NaN-filled arrays, and holds
all six leaves and the four compositing arrays to tests/grad_bound.py's bar,

    every element:  |got - value64| <= 4 K_obs u unit + borderline,

with K_obs the float32 oracle's own figure for the scene and array (tests/test_grad_bound_cpu.py: K_OBS).  Every figure
is printed before it is asserted (pytest -s); CHANGELOG.md keeps the worst ratio the kernels reached."""
import hashlib

import numpy as np
import pytest

import grad_bound
import grad_bound_cases as gc
from conftest import pkg
from test_grad_bound_cpu import K_OBS, K_OBS_EDGE

pytestmark = pytest.mark.gpu
SEG_ENTRIES, SEG_SPLIT_MIN = 496, 1488  # gs_render.h: kSegEntries, kSegSplitMin
_LONG_TERMS = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _context(case, depth=False, route=None):
    ctx = pkg("raster").RasterContext(len(case["params"]["xyz"]), case["W"], case["H"])
    if route is not None:
        ctx.set_binning_route(route)
    if depth:
        ctx.set_depth(True)
    return ctx


def _forward_backward(torch, case, ctx):
    """One forward and one backward of `ctx`; returns (record as numpy, global rows, z, gradient arrays by ARRAYS name)."""
    raster = pkg("raster")
    dp, dc = raster.device_params(case["params"]), raster.device_camera(case["cam"])
    fwd = ctx.rasterize_image(dp, dc, case["cfg"], case["bg"], case["L"])
    record = {k: _np(fwd[k]).copy() for k in ("uv", "conic", "rgb", "sorted", "ranges", "n", "T", "image")}
    rows, z = _np(fwd["compact_to_global"]).astype(np.int64), _np(fwd["xyz_c"])[:, 2].copy()
    grads = ctx.alloc_gradients(fwd["num_culled"], case["L"], intermediates=True)
    for t in grads.values():
        t.fill_(float("nan"))
    kw = {} if case["gd"] is None else dict(grad_depth=_dev(torch, case["gd"]), grad_alpha=_dev(torch, case["ga"]))
    ctx.backward_pass(dp, dc, _dev(torch, case["gi"]), case["bg"], case["L"], grads, **kw)
    torch.cuda.synchronize()
    got = {name: _np(grads[key]).copy() for name, _, key in gc.ARRAYS if grads.get(key) is not None}
    return record, rows, z, got


def _hold(case, t, got, what, table=None):
    """All arrays of `got` against the terms `t`: prints every worst ratio, then fails if any array broke its bar."""
    table = table or K_OBS[case["name"]]
    failures, line = [], []
    for name, arr in got.items():
        v, u, b = t[name]
        K = grad_bound.GPU_MARGIN * table[name]
        try:
            worst = grad_bound.assert_within_bound(arr, v, u, b, K, f"{what}: grad {name}", t["on_list"], t["rows"],
                                                   t["position"], t.get("populations"))
        except AssertionError as e:
            failures.append(str(e))
            worst = grad_bound.observed_K(arr, v, u, b)
        line.append(f"{name} {worst:.3g}/{K:.3g}")
    print(f"[grad bound {what}] worst ratio / bound (u*unit): " + ", ".join(line))
    assert not failures, "\n".join(failures)


def _subset(t, got, rows):
    ts = {k: tuple(a[rows] for a in v) for k, v in t.items() if isinstance(v, tuple)}
    ts.update(on_list=t["on_list"][rows], rows=t["rows"][rows], position=t["position"][rows])
    return ts, {k: np.asarray(v).reshape(len(t["rows"]), -1)[rows] for k, v in got.items()}


def _run_scene(torch, name, pingpong=False):
    case = gc.make(name)
    ctx = _context(case, depth=case["gd"] is not None)
    record, rows, z, got = _forward_backward(torch, case, ctx)
    ctx.close()
    _hold(case, gc.terms(case, record, rows, z), got, name + (" (ping-pong)" if pingpong else ""))


@pytest.mark.parametrize("name", list(gc.BASIC))
def test_basic_sizes(gpu, name):
    """tiny and small at views 0 and 2; SH 0, 1, 2 at 3000 gaussians, 200x120; the odd sizes."""
    _run_scene(gpu, name)


def test_culled_rows_interleaved(gpu):
    """small through scene.cull_half: the chain kernel's scattered-row path and a partial last wave."""
    case = gc.make("culled")
    ctx = _context(case)
    record, rows, z, got = _forward_backward(gpu, case, ctx)
    ctx.close()
    assert 0 < len(rows) < len(case["params"]["xyz"]) and len(rows) % 64 != 0
    assert (np.diff(rows) > 1).any()
    _hold(case, gc.terms(case, record, rows, z), got, "culled")


def _depth_report(t, got, table):
    """The worst ratio per band of list depth (the deepest position a row sits at), over all arrays."""
    edges = (0, 496, 992, 1488, 2480, 1 << 30)
    pos = t["position"]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (pos >= lo) & (pos < hi)
        if not sel.any():
            continue
        worst = max(grad_bound.ratios(np.asarray(a).reshape(len(pos), -1)[sel], *(x[sel] for x in t[n])).max()
                    / (grad_bound.GPU_MARGIN * table[n]) for n, a in got.items() if a.size)
        # and what the bound is worth there, relative to the value itself (uv: the array the densification reads)
        v, u, b = (x[sel] for x in t["uv"])
        live = (u > 0) & (v != 0)
        bar = grad_bound.GPU_MARGIN * table["uv"] * grad_bound.U * u[live] + b[live]
        rel = np.median(bar / np.abs(v[live])) if live.any() else 0.0
        out.append(f"[{lo}, {hi if hi < 1 << 30 else 'end'}): {int(sel.sum())} rows, worst {worst:.3g} of the bound, median uv "
                   f"bound {rel:.1e} of |value|")
    return "; ".join(out)


def _long_lists(torch, pingpong):
    case = gc.make("long")
    ctx = _context(case, route=1)
    for it in range(4):  # whole lists; from forward 1 a segmented backward; forward 3 is segmented itself
        record, rows, z, got = _forward_backward(torch, case, ctx)
        assert ctx.counters()["segmented_backwards"] == it and ctx.counters()["segmented_forwards"] == max(0, it - 2)
        segmented = it >= 1  # the backward of forward 1 onwards walks the lists beyond SEG_SPLIT_MIN in segments
        # the reference costs 15 s on this scene: one per distinct record (forwards 0 to 2 give the same bits, and so does
        # the ping-pong test's context), whole-list and segmented
        key = (segmented, hashlib.sha1(b"".join(record[k].tobytes() for k in sorted(record))).hexdigest())
        if key not in _LONG_TERMS:
            ck = dict(image=record["image"], entries=SEG_ENTRIES, split_min=SEG_SPLIT_MIN) if segmented else None
            _LONG_TERMS[key] = gc.terms(case, record, rows, z, ck)
        t = _LONG_TERMS[key]
        what = f"long lists, forward {it}" + (" (ping-pong)" if pingpong else "")
        print(f"[grad bound {what}] by list depth: " + _depth_report(t, got, K_OBS["long"]))
        _hold(case, t, got, what)
    ctx.close()


def test_long_lists_whole_and_segmented(gpu):
    """The long-list scene (24 000 gaussians, lists of 2 100 .. 7 000 entries), forwards 0 to 3 of one context: whole
    lists, a segmented backward, a segmented forward -- rows behind 1500 faint entries, orders of magnitude below the
    array mean, each held to its own unit."""
    _long_lists(gpu, False)


def test_edge_scene_per_population(gpu):
    """edge_scenes size small: every population to its own K (every visible row is in one of them)."""
    case = gc.make("edge")
    ctx = _context(case)
    record, rows, z, got = _forward_backward(gpu, case, ctx)
    ctx.close()
    t = gc.terms(case, record, rows, z)
    pops = gc.populations_of(case, rows)
    t["populations"] = pops
    failures = []
    for k, r in pops.items():
        if not len(r) or k == "culled":
            continue
        ts, gs = _subset(t, got, r)
        try:
            _hold(case, ts, gs, f"edge [{k}]", K_OBS_EDGE[k])
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_depth_mode(gpu):
    """Plain depth mode with grad_depth and grad_alpha on small: the z row reaches grad_xyz."""
    _run_scene(gpu, "depth")


def test_standalone_render_image_backward(gpu, orc):
    """ops.render_image_backward on the oracle's forward of small: the four compositing arrays."""
    torch, ops = gpu, pkg("ops")
    case = gc.make("small_v2")
    oc = gc.oracle_case(case, orc)
    f, W, H, M = oc["ref"], case["W"], case["H"], len(oc["rows"])
    args = [_dev(torch, f[k]) for k in ("uv", "opacity", "conic", "rgb")]
    g = [torch.zeros(M, 3, device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(M, 2, device="cuda"),
         torch.zeros(M, 3, device="cuda")]
    ops.render_image_backward(*args, case["bg"], _dev(torch, f["sorted"]), _dev(torch, f["ranges"]), _dev(torch, f["n"]),
                              _dev(torch, f["T"]), _dev(torch, case["gi"]), W, H, *g)
    torch.cuda.synchronize()
    got = dict(zip(("precompute_rgb", "opacity", "uv", "conic"), (_np(x) for x in g)))
    _hold(case, oc["terms"], got, "stand-alone render_image_backward, small")


@pytest.mark.parametrize("name", ["small_v2", "long"])
def test_pingpong_backward(gpu, monkeypatch, name):
    """The ping-pong compositing backward (GSPLAT_BWD_PINGPONG=1 per launch, as tests/test_bwd_pingpong_gpu.py sets it)."""
    monkeypatch.setenv("GSPLAT_BWD_PINGPONG", "1")
    if name == "long":
        _long_lists(gpu, True)
    else:
        _run_scene(gpu, name, pingpong=True)

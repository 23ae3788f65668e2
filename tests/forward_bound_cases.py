"""What tests/test_forward_bound_cpu.py and tests/test_forward_bound_gpu.py share: the scenes are grad_bound_cases.make's,
the terms tests/forward_reference.py's, the bar tests/grad_bound.py's.  A forward (the float32 oracle's on the CPU, the HIP
kernels' on the GPU) is a dict of numpy arrays; stage A holds its per-gaussian arrays against the float64 values derived
from the scene's float32 parameters, stage B its per-pixel arrays against the float64 compositing of ITS OWN uv, conic,
rgb and lists."""
import numpy as np

import depth_moment_reference
import forward_reference as fr
import grad_bound
import grad_bound_cases as gc
from conftest import assert_image_close, assert_stop_indices_close

DEPTH_VARIANTS = {"depth": (False, False), "depth_inverse": (True, False), "depth_inverse_moment": (True, True)}
# grad_bound_cases.SCENES with the edge scene from the seed whose rows meet the input condition (grad_bound_cases.make)
SCENES = tuple("edge_fwd" if s == "edge" else s for s in gc.SCENES)
_PG = {}


def K_of(table, name):
    """The K an array is held to on the CPU: the measured figure, floored at 1 (no float32 evaluation promises less than
    the roundings the unit counts)."""
    return max(1.0, float(table[name]))


def per_gaussian(case):
    if case["name"] not in _PG:
        _PG[case["name"]] = fr.per_gaussian(case["params"], case["cam"], case["cfg"]["mh_dist"], case["L"])
    return _PG[case["name"]]


def oracle_forward(case, orc):
    """The float32 oracle's forward of a scene (once)."""
    if "oracle_fwd" not in case:
        cfg = case["cfg"]
        ref = orc.rasterize(case["params"], case["cam"], cfg["near_thresh"], cfg["mh_dist"], cfg["cull_mask_padding"],
                            case["bg"], case["L"], threads=8)
        case["oracle_fwd"] = (ref, np.nonzero(ref["mask"])[0])
    return case["oracle_fwd"]


def logits(case, rows):
    return np.asarray(case["params"]["opacity"], np.float32).reshape(-1)[rows]


def aux_colours(z, inverse, moment):
    """The auxiliary channels of depth mode from the record's float32 z, in float64, with their colours' own relative
    error in u: s = z is stored (0), s = 1 / z is a reciprocal (a library one: LIB), s^2 one product of that."""
    z = np.asarray(z, np.float32).astype(np.float64)
    s, rel = (1.0 / z, fr.LIB) if inverse else (z, 0.0)
    cols, rels = [s], [rel]
    if moment:
        cols.append(s * s)
        rels.append(2.0 * rel + 1.0)
    return np.stack(cols, 1), np.asarray(rels)


def stage_a_ratios(case, fwd, rows, sel=None):
    """name -> worst ratio (u * unit) of the per-gaussian arrays of `fwd` (compacted rows = global `rows`; sel: a subset
    of the compacted rows); theta: the stored (sin, cos) against theta64, in u (e_theta + 1 + LIB)."""
    pg = per_gaussian(case)
    sel = np.arange(len(rows)) if sel is None else np.asarray(sel)
    out = {}
    for name in fr.ROW_ARRAYS:
        if fwd.get(name) is None:
            continue
        v, u = pg[name]
        got = np.asarray(fwd[name], np.float64).reshape(len(rows), -1)[sel]
        out[name] = grad_bound.observed_K(got, v[rows][sel], u[rows][sel], np.zeros_like(u[rows][sel]))
    _, figs = fr.radius_failures(np.asarray(fwd["radius"]).reshape(-1, 4)[sel], pg, rows[sel], 1.0)
    out["theta"] = figs["theta_ratio"]
    return out


def hold_stage_a(case, fwd, rows, table, margin, what, sel=None):
    """Every per-gaussian array of `fwd` to its bar (K = margin x the table's figure, floored at 1), the radii and the
    (sin, cos) to the float64 decisions.  Returns (failures, report line)."""
    pg = per_gaussian(case)
    sel_ = np.arange(len(rows)) if sel is None else np.asarray(sel)
    failures, line = [], []
    for name in fr.ROW_ARRAYS:
        if fwd.get(name) is None:
            continue
        v, u = pg[name]
        K = margin * K_of(table, name)
        got = np.asarray(fwd[name], np.float64).reshape(len(rows), -1)[sel_]
        vv, uu = v[rows][sel_], u[rows][sel_]
        try:
            worst = grad_bound.assert_within_bound(got, vv, uu, np.zeros_like(uu), K, f"{what}: {name}", None, rows[sel_])
        except AssertionError as e:
            failures.append(str(e))
            worst = grad_bound.observed_K(got, vv, uu, np.zeros_like(uu))
        line.append(f"{name} {worst:.3g}/{K:.3g}")
    # rho and theta come off the same 2-D covariance as the conic: its K
    K = margin * K_of(table, "conic")
    msgs, figs = fr.radius_failures(np.asarray(fwd["radius"]).reshape(-1, 4)[sel_], pg, rows[sel_], K)
    failures += [f"{what}: {m}" for m in msgs]
    line.append(f"theta {figs['theta_ratio']:.3g}/{K:.3g}; radii: {figs['differs']} rows differ from ceil(rho64), "
                f"{figs['either']} borderline, {figs['nan']} NaN, {figs['loose_theta']} near-isotropic")
    return failures, ", ".join(line)


def hold_mask(case, mask, table, margin, what):
    """The keep mask (and with it num_culled) against the float64 decision; rows within their bar of a bound are free."""
    pg = per_gaussian(case)
    keep, free = fr.mask_terms(pg, case["cfg"], case["W"], case["H"], margin * K_of(table, "xyz_c"), margin * K_of(table, "uv"))
    bad = (np.asarray(mask).astype(bool) != keep) & ~free
    return ([f"{what}: the keep mask differs from the float64 decision on {int(bad.sum())} rows clear of every bound, "
             f"first {int(np.nonzero(bad)[0][0])}"] if bad.any() else []), int(free.sum())


def stage_b_terms(case, fwd, rows, variant=None, segmented=False):
    """The float64 compositing of the record `fwd` (uv conic rgb sorted ranges; xyz_c in depth mode)."""
    aux = rel = None
    if variant is not None:
        aux, rel = aux_colours(np.asarray(fwd["xyz_c"]).reshape(-1, 3)[:, 2], *DEPTH_VARIANTS[variant])
    t = fr.compositing(fwd, logits(case, rows), case["bg"], case["W"], case["H"], aux, rel, segmented)
    if variant is not None:
        v, u, b = t["aux"]
        t["depth"] = (v[..., 0], u[..., 0], b[..., 0])
        if DEPTH_VARIANTS[variant][1]:
            t["depth2"] = (v[..., 1], u[..., 1], b[..., 1])
    return t


def stage_b_arrays(t):
    return [k for k in ("image", "T", "depth", "depth2", "alpha") if k in t]


def stage_b_ratios(t, fwd):
    P = t["n64"].size
    return {k: grad_bound.observed_K(np.asarray(fwd[k], np.float64).reshape(P, -1), *(a.reshape(P, -1) for a in t[k]))
            for k in stage_b_arrays(t) if fwd.get(k) is not None}


def hold_stage_b(t, fwd, table, margin, what):
    """Every per-pixel array to its bar; n to the float64 stop index (either walk's where the stop is borderline).
    Returns (failures, report line)."""
    P = t["n64"].size
    failures, line = [], []
    for k in stage_b_arrays(t):
        if fwd.get(k) is None:
            continue
        K = margin * K_of(table, k)
        got, (v, u, b) = np.asarray(fwd[k], np.float64).reshape(P, -1), (a.reshape(P, -1) for a in t[k])
        try:
            worst = grad_bound.assert_within_bound(got, v, u, b, K, f"{what}: {k}")
        except AssertionError as e:
            failures.append(str(e))
            worst = grad_bound.observed_K(got, *(a.reshape(P, -1) for a in t[k]))
        line.append(f"{k} {worst:.3g}/{K:.3g}")
    n = np.asarray(fwd["n"])
    bad = (n != t["n64"]) & ~(t["stop_borderline"] & (n == t["n_alt"]))
    if bad.any():
        y, x = np.argwhere(bad)[0]
        failures.append(f"{what}: n[{y}, {x}] = {n[y, x]}, float64 {t['n64'][y, x]} (the other walk: {t['n_alt'][y, x]}); {int(bad.sum())} such pixels")
    line.append(f"n: {int((n != t['n64']).sum())} pixels on the other side of a borderline stop ({int(t['stop_borderline'].sum())} borderline)")
    return failures, ", ".join(line)


def old_bars_pass(got, ref):
    """tests/test_fused_gpu.py::_check_forward's tolerances (and conftest's) on the arrays both forwards have."""
    try:
        np.testing.assert_allclose(got["conic"], ref["conic"], rtol=2e-4, atol=1e-7)
        np.testing.assert_allclose(got["rgb"], ref["rgb"], rtol=1e-5, atol=2e-6)
        assert_image_close(got["image"], ref["image"], "image")
        assert_image_close(got["T"], ref["T"], "transmittance")
        assert_stop_indices_close(got["n"], ref["n"])
        return True
    except AssertionError:
        return False


def oracle_depth_maps(case, orc, ref, variant):
    inverse, moment = DEPTH_VARIANTS[variant]
    D, A, Q = depth_moment_reference.maps(orc, ref, case["W"], case["H"], inverse, threads=8)
    out = dict(depth=D, alpha=np.float32(1) - ref["T"])
    if moment:
        out["depth2"] = Q
    return out

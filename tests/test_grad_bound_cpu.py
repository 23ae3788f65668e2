"""The per-gaussian gradient bound without a GPU: the float64 reference (tests/render_bwd_reference.py) against a
hand-worked case and the float64 oracle, the chain's linearity, the K_obs tables the GPU tests take their bounds from, the
condition on the scenes, and four perturbations of the float32 oracle's own output that the bar must reject.

What conftest.assert_grad_close says to the four perturbations (printed by test_the_bar_rejects_perturbations, -s):
see PERTURBATIONS_ACCEPTED_BY_ASSERT_GRAD_CLOSE below."""
import numpy as np
import pytest

import absgrad_reference
import depth_reference
import edge_scenes
import grad_bound
import grad_bound_cases as gc
import render_bwd_reference as rbr
from conftest import assert_grad_close

U = grad_bound.U

# K_obs = max (|float32 oracle - value64| - borderline) / (u * unit), measured by test_k_obs_tables on every run and held
# to these figures (the measurement, rounded up to two digits).  The GPU bound is grad_bound.GPU_MARGIN times the entry.
# An entry is never below 1: the measurement falls under it wherever the oracle's roundings happen to cancel (one gaussian
# at 17x9: opacity 0.0019), and no float32 evaluation can promise less than the one rounding of its stored result, u |value|,
# which reaches u * unit on a row whose shares do not cancel.
# precompute_rgb / band0 / sh grow with the list depth: a share alpha T_i G carries T_i = T_final / prod (1 - alpha), one
# rounding per list entry behind it.
K_OBS = {
    "tiny_v0": {"precompute_rgb": 1.7, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.7, "leaf_sh": 1.0, "leaf_scale": 4.6, "leaf_quaternion": 2.3},
    "tiny_v2": {"precompute_rgb": 2.3, "opacity": 1.1, "conic": 1.7, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 2.3, "leaf_sh": 1.0, "leaf_scale": 2.3, "leaf_quaternion": 1.8},
    "small_v0": {"precompute_rgb": 3.7, "opacity": 1.7, "conic": 2.0, "uv": 2.3, "leaf_xyz": 2.3, "leaf_band0": 3.7, "leaf_sh": 1.1, "leaf_scale": 3.7, "leaf_quaternion": 8.8},
    "small_v2": {"precompute_rgb": 6.3, "opacity": 5.4, "conic": 4.6, "uv": 5.1, "leaf_xyz": 5.1, "leaf_band0": 6.4, "leaf_sh": 1.7, "leaf_scale": 15.0, "leaf_quaternion": 4.0},
    "sh0": {"precompute_rgb": 7.0, "opacity": 5.4, "conic": 5.2, "uv": 5.3, "leaf_xyz": 5.3, "leaf_band0": 7.1, "leaf_sh": 1.0, "leaf_scale": 3.4, "leaf_quaternion": 4.8},
    "sh1": {"precompute_rgb": 7.0, "opacity": 5.1, "conic": 5.0, "uv": 5.1, "leaf_xyz": 5.0, "leaf_band0": 7.1, "leaf_sh": 1.6, "leaf_scale": 3.3, "leaf_quaternion": 4.6},
    "sh2": {"precompute_rgb": 7.0, "opacity": 6.5, "conic": 6.4, "uv": 6.4, "leaf_xyz": 6.4, "leaf_band0": 7.1, "leaf_sh": 1.7, "leaf_scale": 3.9, "leaf_quaternion": 6.0},
    "odd_1": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "odd_37": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "odd_257": {"precompute_rgb": 2.0, "opacity": 1.2, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 2.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 2.7},
    "culled": {"precompute_rgb": 2.3, "opacity": 2.1, "conic": 1.3, "uv": 1.7, "leaf_xyz": 1.7, "leaf_band0": 2.3, "leaf_sh": 1.0, "leaf_scale": 13.0, "leaf_quaternion": 4.5},
    "long": {"precompute_rgb": 14.0, "opacity": 7.5, "conic": 8.0, "uv": 6.6, "leaf_xyz": 6.6, "leaf_band0": 14.0, "leaf_sh": 3.2, "leaf_scale": 85.0, "leaf_quaternion": 55.0},
    "edge": {"precompute_rgb": 190.0, "opacity": 45.0, "conic": 87.0, "uv": 83.0, "leaf_xyz": 150.0, "leaf_band0": 190.0, "leaf_sh": 49.0, "leaf_scale": 53.0, "leaf_quaternion": 68.0},
    "depth": {"precompute_rgb": 6.3, "opacity": 5.8, "conic": 5.1, "uv": 5.5, "leaf_xyz": 5.5, "leaf_band0": 6.4, "leaf_sh": 1.7, "leaf_scale": 7.2, "leaf_quaternion": 4.6, "z": 6.2},
}
# edge_scenes size small, per population (rows of that population only)
K_OBS_EDGE = {
    "clamp_x": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "clamp_y": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "clamp_corner": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "near": {"precompute_rgb": 110.0, "opacity": 34.0, "conic": 34.0, "uv": 36.0, "leaf_xyz": 36.0, "leaf_band0": 110.0, "leaf_sh": 28.0, "leaf_scale": 21.0, "leaf_quaternion": 13.0},
    "tiny": {"precompute_rgb": 4.2, "opacity": 2.6, "conic": 1.0, "uv": 2.0, "leaf_xyz": 2.0, "leaf_band0": 4.0, "leaf_sh": 1.1, "leaf_scale": 1.0, "leaf_quaternion": 2.6},
    "needle": {"precompute_rgb": 11.0, "opacity": 3.1, "conic": 7.1, "uv": 5.1, "leaf_xyz": 5.1, "leaf_band0": 11.0, "leaf_sh": 2.9, "leaf_scale": 25.0, "leaf_quaternion": 2.4},
    "flat": {"precompute_rgb": 3.2, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 3.1, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "quat_small": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "quat_large": {"precompute_rgb": 2.7, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 2.7, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.7},
    "saturated": {"precompute_rgb": 6.4, "opacity": 1.0, "conic": 1.0, "uv": 1.2, "leaf_xyz": 1.2, "leaf_band0": 6.4, "leaf_sh": 1.9, "leaf_scale": 1.2, "leaf_quaternion": 1.2},
    "gate": {"precompute_rgb": 4.7, "opacity": 2.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 4.8, "leaf_sh": 1.9, "leaf_scale": 1.0, "leaf_quaternion": 1.1},
    "vanishing": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "clamp_boundary": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 23.0, "uv": 1.0, "leaf_xyz": 150.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 15.0, "leaf_quaternion": 2.8},
    "near_edge": {"precompute_rgb": 1.0, "opacity": 1.0, "conic": 1.0, "uv": 1.0, "leaf_xyz": 1.0, "leaf_band0": 1.0, "leaf_sh": 1.0, "leaf_scale": 1.0, "leaf_quaternion": 1.0},
    "base": {"precompute_rgb": 190.0, "opacity": 45.0, "conic": 87.0, "uv": 83.0, "leaf_xyz": 83.0, "leaf_band0": 190.0, "leaf_sh": 49.0, "leaf_scale": 53.0, "leaf_quaternion": 68.0},
}
# (perturbation, array) pairs that conftest.assert_grad_close ACCEPTS although every touched element is wrong: filled in
# from the run of test_the_bar_rejects_perturbations, which asserts that the list is still what the suite's older check
# says.  (a) zeroes every element below 1e-3 of the array's mean, (b) scales one row behind list position 1000 by 1.01,
# (c) drops one pixel's share from one row, (d) flips one row's sign.
CHECKED_NAMES = ("precompute_rgb", "opacity", "conic", "uv", "leaf_xyz", "leaf_band0", "leaf_sh", "leaf_scale", "leaf_quaternion")
PERTURBATIONS_ACCEPTED_BY_ASSERT_GRAD_CLOSE = {
    "a": CHECKED_NAMES, "b": CHECKED_NAMES, "c": (), "d": (),
}
CHECKED = [n for n, _, _ in gc.ARRAYS]


def _f64_bar(unit):
    """Two float64 evaluations of the same sums in another order: 1e-6 u = 6e-14 of the condition sum."""
    return 1e-6 * U * unit


# ------------------------------------------------------------------------------------------ the hand-worked case
def test_hand_worked_case():
    """One tile, two gaussians (0 in front of 1), three pixels with a non-zero gradient.  At pixel C gaussian 1's alpha is
    0.1 % below 1/255: not composited, so in neither signed nor absolute, but in borderline as if it were.  Every share
    is written out with the plain formulas (pixel offsets, no row polynomial)."""
    W, H, bg = 8, 4, 0.25
    uv = np.array([[2.3, 1.6], [4.1, 2.2]])
    conic = np.array([[0.5, 0.1, 0.7], [0.3, -0.05, 0.4]])
    rgb = np.array([[0.9, 0.2, 0.4], [0.1, 0.8, 0.6]])
    pixels = {(2, 1): np.array([0.3, -0.2, 0.5]), (4, 2): np.array([-0.4, 0.1, 0.2]), (5, 0): np.array([0.2, 0.6, -0.3])}
    a_min = float(np.float32(0.00392156862))

    def gauss(k, px, py):
        dx, dy = uv[k, 0] - px, uv[k, 1] - py
        return dx, dy, np.exp(-0.5 * (conic[k, 0] * dx * dx + 2 * conic[k, 1] * dx * dy + conic[k, 2] * dy * dy))

    opa = np.array([0.6, 0.0])
    opa[1] = a_min * (1 - 1e-3) / gauss(1, 5, 0)[2]  # gaussian 1 at pixel C = (5, 0): 0.1 % below the threshold
    assert 0 < opa[1] < 1
    logit = np.log(opa / (1 - opa))
    n = np.full((H, W), 2, np.int32)
    T = np.ones((H, W))
    G = np.zeros((H, W, 3))
    want = {k: np.zeros((2, 9)) for k in ("signed", "absolute", "borderline")}
    for py in range(H):
        for px in range(W):
            alpha = [min(0.99, opa[k] * gauss(k, px, py)[2]) for k in (0, 1)]
            on = [a >= a_min for a in alpha]
            T[py, px] = np.prod([1 - a for a, o in zip(alpha, on) if o])
            if (px, py) not in pixels:
                continue
            g = G[py, px] = pixels[(px, py)]
            assert on[0], "gaussian 0 is composited at all three pixels"
            assert on[1] == ((px, py) != (5, 0))
            a0 = alpha[0]
            for k in (0, 1):
                dx, dy, gg = gauss(k, px, py)
                a_k = alpha[k]
                # in front of k / behind k; a pair valued "as if composited" changes nothing for the other gaussian
                T_front = 1.0 if k == 0 else 1 - a0
                behind = (alpha[1] * rgb[1] if on[1] else np.zeros(3)) if k == 0 else np.zeros(3)
                T_final_as_if = T[py, px] if on[k] else T[py, px] * (1 - a_k)
                ga = ((rgb[k] - behind) * g).sum() * T_front - T_final_as_if / (1 - a_k) * (bg * g).sum()
                gpow = gg * ga * opa[k]
                share = np.concatenate([a_k * T_front * g, [gpow * (1 - opa[k])],
                                        gpow * np.array([-0.5 * dx * dx, -dx * dy, -0.5 * dy * dy]),
                                        [gpow * (-conic[k, 0] * dx - conic[k, 1] * dy) * 0.5 * W,
                                         gpow * (-conic[k, 2] * dy - conic[k, 1] * dx) * 0.5 * H]])
                if on[k]:
                    want["signed"][k] += share
                    want["absolute"][k] += np.abs(share)
                if abs(opa[k] * gg - a_min) <= rbr.ALPHA_REL_TOL * a_min:
                    want["borderline"][k] += np.abs(share)
    rec = dict(uv=uv, opacity=logit, conic=conic, rgb=rgb, sorted=np.array([0, 1], np.int32),
               ranges=np.array([0, 2], np.int32), n=n, T=T)
    signed, absolute, borderline = rbr.compositing_sums(rec, G, W, H, bg)
    assert (want["borderline"][0] == 0).all() and (want["borderline"][1] > 0).all()
    for name, got in (("signed", signed), ("absolute", absolute), ("borderline", borderline)):
        np.testing.assert_allclose(got, want[name], rtol=1e-12, atol=0, err_msg=name)


# --------------------------------------------------------------------------- the reference against the float64 oracle
@pytest.mark.parametrize("name", ["tiny_v2", "small_v2", "culled", "depth"])
def test_signed_is_the_float64_oracle(orc, name):
    """signed equals the float64 oracle's render_image_backward on the same record within 1e-6 u absolute (measured for
    uv: 6e-8); absolute >= |signed|; the uv columns are absgrad_reference's; depth mode: tests/depth_reference.py's sum."""
    case = gc.make(name)
    oc = gc.oracle_case(case, orc)
    ref, W, H = oc["ref"], case["W"], case["H"]
    z = ref["xyz_c"][:, 2] if case["gd"] is not None else None
    signed, absolute, _ = rbr.compositing_sums(ref, case["gi"], W, H, case["bg"], case["gd"], case["ga"], z)
    if case["gd"] is None:
        w = orc.render_image_backward(ref["uv"], ref["opacity"], ref["conic"], ref["rgb"], case["bg"], ref["sorted"],
                                      ref["ranges"], ref["n"], ref["T"], case["gi"], W, H, np.float64, 8)
        want = np.concatenate([w[0], w[1][:, None], w[3], w[2]], 1)
    else:
        g = depth_reference.backward_pass(orc, ref, case["cam"], case["gi"], case["gd"], case["ga"], case["bg"], case["L"],
                                          np.float64, 8)
        want = np.concatenate([g["rgb_pre"], g["opacity"][:, None], g["conic"], g["uv"], g["z"][:, None]], 1)
    excess = np.abs(signed - want) - _f64_bar(absolute)
    worst = (np.abs(signed - want) / (U * np.maximum(absolute, 1e-300))).max()
    print(f"[{name}] signed against the float64 oracle: worst {worst:.2e} u*absolute")
    assert (excess <= 0).all(), f"{worst:.3e} u*absolute"
    assert (absolute >= np.abs(signed) - _f64_bar(absolute)).all()
    s_uv, a_uv = absgrad_reference.absgrad_sums(ref, case["gi"], W, H, case["bg"], case["gd"], case["ga"], z)
    uvs = rbr.SLICES["uv"]  # the same shares, summed in another order
    assert (np.abs(signed[:, uvs] - s_uv) <= _f64_bar(a_uv)).all() and (np.abs(absolute[:, uvs] - a_uv) <= _f64_bar(a_uv)).all()


@pytest.mark.parametrize("name", ["tiny_v2", "sh1", "edge"])
def test_chain_is_linear(orc, name):
    """A_i . signed_i equals the float64 oracle.backward_pass leaves on the same (float64) record.  The bar: both are
    float64 evaluations (eps = 1.9e-9 u) of a chain of about a hundred operations whose inner products cancel up to the
    screen covariance's condition number, ~1e3 in these scenes (edge_scenes: the needles): 1e-4 u of the unit."""
    case = gc.make(name)
    cfg = case["cfg"]
    ref = orc.rasterize(case["params"], case["cam"], cfg["near_thresh"], cfg["mh_dist"], cfg["cull_mask_padding"],
                        case["bg"], case["L"], dtype=np.float64, threads=8)
    b = orc.backward_pass(ref, case["cam"], case["gi"], case["bg"], case["L"], np.float64, 8,
                          tan_fov=edge_scenes.backward_tan_fov(case["cam"]))
    rows = np.nonzero(ref["mask"])[0]
    t = gc.terms(case, ref, rows)
    # sigma(logit) == 1 in float32: the reference adds nothing, as every float32 path does; the float64 oracle does add
    lg = np.asarray(case["params"]["opacity"], np.float32)[rows]
    opaque = (np.float32(1) / (np.float32(1) + np.exp(-lg))) == 1
    for name_, key, _ in gc.ARRAYS[4:]:
        v, u, _b = t[name_]
        want = np.asarray(b[key], np.float64).reshape(v.shape)
        assert np.isfinite(want).all() and np.isfinite(v).all(), name_ + ": a non-finite float64 value"
        assert (v[opaque] == 0).all()
        want[opaque] = 0.0
        r = grad_bound.ratios(want, v, u, np.zeros_like(u))
        i, j = np.unravel_index(int(np.argmax(r)), r.shape)
        print(f"[{name}] chain {name_}: worst {r.max():.2e} u*unit (row {i}: {v[i, j]:.6e} against {want[i, j]:.6e}, unit {u[i, j]:.2e})")
        assert (r <= 1e-4).all(), name_


# ----------------------------------------------------------------------------------------- the tables and the scenes
@pytest.mark.parametrize("name", gc.SCENES)
def test_k_obs_tables(orc, name):
    """The measurement behind K_OBS, run here: the float32 oracle against the float64 terms of its own record."""
    case = gc.make(name)
    oc = gc.oracle_case(case, orc)
    if oc is None:
        pytest.fail("nothing is visible in " + name)
    k = gc.compare(oc["terms"], gc.oracle_arrays(oc["bref"]))
    print(f"[K_obs {name}] " + ", ".join(f"{n} {v:.3g}" for n, v in k.items()))
    for n, v in k.items():
        assert v <= K_OBS[name][n], f"{name} {n}: K_obs {v:.4g} has grown beyond {K_OBS[name][n]}"
    if name == "edge":
        pops = gc.populations_of(case, oc["rows"])
        got = gc.oracle_arrays(oc["bref"])
        for p, r in pops.items():
            if not len(r) or p == "culled":
                continue
            ts = {n: tuple(a[r] for a in oc["terms"][n]) for n in got if n in oc["terms"]}
            kp = {n: grad_bound.observed_K(np.asarray(got[n]).reshape(len(oc["rows"]), -1)[r], *ts[n]) for n in ts}
            print(f"[K_obs edge {p}] " + ", ".join(f"{n} {v:.3g}" for n, v in kp.items()))
            for n, v in kp.items():
                assert v <= K_OBS_EDGE[p][n], f"edge [{p}] {n}: K_obs {v:.4g} has grown beyond {K_OBS_EDGE[p][n]}"


@pytest.mark.parametrize("name", gc.SCENES)
def test_input_condition(orc, name):
    """At most 0.5 % of a scene's live elements may have borderline > 1e-2 unit (they are held to a loose bar), for every
    array; from the reference alone."""
    case = gc.make(name)
    t = gc.oracle_case(case, orc)["terms"]
    shares = {n: grad_bound.loose_share(t[n][1], t[n][2]) for n in CHECKED + (["z"] if "z" in t else [])}
    print(f"[loose share {name}] " + ", ".join(f"{n} {100 * v:.3f}%" for n, v in shares.items()))
    for n, v in shares.items():
        assert v <= grad_bound.LOOSE_SHARE, f"{name} {n}: {100 * v:.3f} % of the live elements sit on a borderline pair"


def test_the_tail_is_really_there(orc):
    """The long-list scene: at least 100 rows behind list position 992 whose condition sum is below 1e-3 of the array's
    mean -- the rows assert_grad_close cannot see."""
    case = gc.make("long")
    t = gc.oracle_case(case, orc)["terms"]
    deep = t["position"] > 992
    for n in ("uv", "precompute_rgb", "conic", "opacity"):
        v, absolute = t[n][0], t["absolute"][:, rbr.SLICES[n]]
        faint = (absolute.max(1) < 1e-3 * np.abs(v).mean()) & (absolute.max(1) > 0) & deep
        print(f"[tail] {n}: {int(faint.sum())} live rows behind position 992 below 1e-3 of the mean; {int(deep.sum())} deep rows")
        assert faint.sum() >= 100, n


# ------------------------------------------------------------------------------------------------- the bar bites
def _accepted(got, ref):
    try:
        assert_grad_close(got, ref)
        return True
    except AssertionError:
        return False


def _pixel_share(case, oc, px, py):
    """The shares of one pixel for every row: the sums are linear in the gradient image, pixel by pixel."""
    one = {k: None if case[k] is None else np.zeros_like(case[k]) for k in ("gd", "ga")}
    gi = np.zeros_like(case["gi"])
    gi[py, px] = case["gi"][py, px]
    ref = oc["ref"]
    return rbr.compositing_sums(ref, gi, case["W"], case["H"], case["bg"], one["gd"], one["ga"], None)[0]


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_the_bar_rejects_perturbations(orc, kind):
    """Four perturbations of the float32 oracle's own output, per array: the bar (at the GPU's K = 4 K_obs) must reject
    each; what assert_grad_close says is printed and pinned in PERTURBATIONS_ACCEPTED_BY_ASSERT_GRAD_CLOSE."""
    scene = {"b": "long", "c": "tiny_v2"}.get(kind, "small_v2")
    case = gc.make(scene)
    oc = gc.oracle_case(case, orc)
    t, M = oc["terms"], len(oc["rows"])
    base = {n: np.array(a, np.float64).reshape(M, -1) for n, a in gc.oracle_arrays(oc["bref"]).items() if a is not None}
    A = t["A"]
    accepted = set()
    if kind == "c":
        # the strongest of the compact rows well inside the image, and the first pixel around its centre whose share
        # counts in all nine sums
        uvr, rad = oc["ref"]["uv"], oc["ref"]["radius"]
        inside = ((uvr[:, 0] > 8) & (uvr[:, 0] < case["W"] - 8) & (uvr[:, 1] > 8) & (uvr[:, 1] < case["H"] - 8)
                  & (rad[:, 0] <= 4))
        row = int(np.argmax(np.where(inside, np.abs(t["uv"][0]).sum(1), -1.0)))
        for ox, oy in ((1, 1), (-1, 1), (1, -1), (-1, -1), (0, 1), (1, 0), (0, 0), (2, 1), (1, 2)):
            share = np.zeros((M, 9))
            share[row] = _pixel_share(case, oc, int(np.floor(uvr[row, 0])) + ox, int(np.floor(uvr[row, 1])) + oy)[row]
            if (np.abs(share[row]) > 1e-3 * t["absolute"][row]).all():
                break
        assert (np.abs(share[row]) > 1e-3 * t["absolute"][row]).all(), "the share is above 1e-3 of absolute in all nine sums"
    for n in CHECKED:
        v, u, b = t[n]
        K = grad_bound.GPU_MARGIN * K_OBS[scene][n]
        got = base[n].copy()
        slack = K * U * u + b
        if kind == "a":
            small = (np.abs(got) < 1e-3 * np.abs(got).mean()) & (got != 0)
            assert small.sum() > 10, n
            got[small] = 0.0
        elif kind == "b":
            row = int(np.argmax(np.where(t["position"] > 1000, (0.01 * np.abs(v) - slack).max(1), -np.inf)))
            assert t["position"][row] > 1000
            got[row] *= 1.01
        elif kind == "d":
            row = int(np.argmax((2 * np.abs(v) - slack).max(1)))
            got[row] = -got[row]
        else:  # one pixel's share, above 1e-3 of the row's absolute, dropped from one row
            got = got - (rbr.apply(A, share)[n[5:]] if n.startswith("leaf_") else share[:, rbr.SLICES[n]])
        with pytest.raises(AssertionError):
            grad_bound.assert_within_bound(got, v, u, b, K, f"perturbation ({kind}) of {n}", t["on_list"])
        if _accepted(got, base[n]):
            accepted.add(n)
    print(f"[perturbation ({kind}) on {scene}] assert_grad_close accepts: {sorted(accepted) or 'none'}")
    assert accepted == set(PERTURBATIONS_ACCEPTED_BY_ASSERT_GRAD_CLOSE[kind]), sorted(accepted)


# The share of the elements on which a 1 % error is beyond the bar (0.01 |value| > 4 K_obs u unit + borderline), from the
# reference alone: all live elements of `small`, and the deep rows (list position > 992) of the long-list scene under
# the whole-list unit and under the segmented backward's.  The figures are the measurement rounded down; they say how
# much of the tail the bar covers, which test_the_bar_rejects_perturbations (one chosen row per array) cannot.  The
# segmented unit carries the checkpoint term (render_bwd_reference: e_ck): there the deep rows of opacity, conic, uv
# and what hangs on them are covered far less -- the cost of recovering the colour behind a boundary as (image - C_b) /
# T_b, which the kernels' own error shows too (4e3 u * the whole-list unit on the GPU).
COVERAGE_1_PERCENT = {
    "small_v2": {"precompute_rgb": 0.96, "opacity": 0.95, "conic": 0.92, "uv": 0.94, "leaf_xyz": 0.93, "leaf_band0": 0.96, "leaf_sh": 0.84, "leaf_scale": 0.80, "leaf_quaternion": 0.89},
    "long_whole": {"precompute_rgb": 0.97, "opacity": 0.98, "conic": 0.88, "uv": 0.98, "leaf_xyz": 0.97, "leaf_band0": 0.97, "leaf_sh": 0.84, "leaf_scale": 0.33, "leaf_quaternion": 0.45},
    "long_segmented": {"precompute_rgb": 0.97, "opacity": 0.42, "conic": 0.37, "uv": 0.44, "leaf_xyz": 0.43, "leaf_band0": 0.97, "leaf_sh": 0.84, "leaf_scale": 0.15, "leaf_quaternion": 0.19},
}


@pytest.mark.parametrize("which", ["small_v2", "long_whole", "long_segmented"])
def test_how_much_of_the_tail_the_bar_covers(orc, which):
    scene = "small_v2" if which == "small_v2" else "long"
    case = gc.make(scene)
    oc = gc.oracle_case(case, orc)
    t = oc["terms"]
    if which == "long_segmented":
        t = gc.terms(case, oc["ref"], oc["rows"], None, dict(image=oc["ref"]["image"], entries=496, split_min=1488))
    sel = t["position"] > 992 if scene == "long" else t["position"] >= 0
    shares, bounds = {}, {}
    for n in CHECKED:
        v, u, b = (a[sel] for a in t[n])
        live = u > 0
        bar = grad_bound.GPU_MARGIN * K_OBS[scene][n] * U * u + b
        shares[n] = float((0.01 * np.abs(v[live]) > bar[live]).mean()) if live.any() else 1.0
        with np.errstate(divide="ignore"):
            bounds[n] = float(np.median((bar[live] / np.abs(v[live]))[v[live] != 0])) if live.any() else 0.0
    print(f"[coverage {which}] a 1 % error is beyond the bar on: " + ", ".join(f"{n} {100 * x:.1f}%" for n, x in shares.items()))
    print(f"[coverage {which}] median bound / |value|: " + ", ".join(f"{n} {x:.1e}" for n, x in bounds.items()))
    for n, x in shares.items():
        assert x >= COVERAGE_1_PERCENT[which][n], f"{which} {n}: a 1 % error is visible on {100 * x:.1f} % of the elements only"

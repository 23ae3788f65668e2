"""The feature map's gradient with respect to the geometry, without a GPU: the C-channel reference
(tests/feature_bwd_reference.py) against the 3-channel float64 module summed over channel triplets and against central
finite differences of the feature map itself, the K_obs table the GPU tests take their bounds from, the condition on the
scenes, and the entry point's refusal of a null context."""
import ctypes
import os
import re

import numpy as np
import pytest

import feature_bwd_cases as fc
import feature_bwd_reference as fbr
import feature_reference as fr
import grad_bound
import render_bwd_reference as rbr
from conftest import ROOT, pkg

U = grad_bound.U

# K_obs = max (|float32 mode - float64| - borderline) / (u * unit) of tests/feature_bwd_reference.py, per scene (at the
# channel count of feature_bwd_cases.TABLE_CHANNELS) and column group, measured by test_k_obs_table on every run and held
# to these figures: the measurement rounded up to two digits, never below 1 (the rule of tests/test_grad_bound_cpu.py:
# no float32 evaluation can promise less than the one rounding of its stored result).  The GPU bound is
# grad_bound.GPU_MARGIN times the entry.  The long-list scene's rows sit behind up to 2400 entries: T_i = T_final / prod
# (1 - alpha) carries one rounding per entry behind it.
K_OBS_FEATURES = {
    "tiny": {"opacity": 1.0, "conic": 1.1, "uv": 1.0},
    "partial": {"opacity": 1.0, "conic": 1.8, "uv": 1.0},
    "small": {"opacity": 3.2, "conic": 1.8, "uv": 1.9},
    "long": {"opacity": 7.4, "conic": 5.3, "uv": 6.9},
}
_SUMS = {}


def _sums(orc, name):
    """The float64 sums of a scene at its table's channel count, on the oracle's forward (computed once)."""
    if name not in _SUMS:
        case = fc.make(name)
        ref, rows = fc.oracle_forward(case, orc)
        C = fc.TABLE_CHANNELS[name]
        rec = fc.record_of(ref, ref["opacity"])
        f, G = case["feats"][rows][:, :C], case["gmap"][..., :C]
        _SUMS[name] = (case, rec, f, G, fbr.feature_sums(rec, f, G, case["W"], case["H"]))
    return _SUMS[name]


def _triplets(rec, f, G, W, H):
    """The sum over channel triplets of the 3-channel module: (all nine columns of signed [M,9], its absolute)."""
    C = f.shape[1]
    pad = (-C) % 3
    f3, G3 = np.pad(f, ((0, 0), (0, pad))), np.pad(G, ((0, 0), (0, 0), (0, pad)))
    total, rgb = 0.0, []
    for k in range(0, C + pad, 3):
        s = rbr.compositing_sums(dict(rec, rgb=f3[:, k:k + 3]), G3[..., k:k + 3], W, H, 0.0)[0]
        total = total + s[:, 3:9]
        rgb.append(s[:, 0:3])
    return total, np.concatenate(rgb, 1)[:, :C]


def test_abi_declares_the_entry_point_and_stays_at_9():
    lib = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"\bint\s+gsplat_context_features_backward\s*\(", header)
    assert len(lib.SIGNATURES["gsplat_context_features_backward"][1]) == 6
    assert lib.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    assert callable(pkg("raster").RasterContext.features_backward) and callable(pkg("trainer").Trainer.feature_gradients)
    assert "FROZEN" not in header


def test_a_null_context_is_refused():
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    assert lib.gsplat_context_features_backward(None, 1, 1, None, None, None) == -3  # GSPLAT_ERR_INVALID_ARG
    with pytest.raises(lib_mod.GsplatError):
        lib_mod.check(lib.gsplat_context_features_backward(None, 1, 1, None, None, None))


@pytest.mark.parametrize("name", ["tiny", "partial"])
def test_the_sum_over_channel_triplets(orc, name):
    """At C = 35 the six columns equal the sum over channel triplets of compositing_sums (colours := the triplet, pixel
    gradient := the triplet, background 0) to 1e-12 of `absolute`: the expression is linear in (f, G) over channels.  The
    triplets' colour columns are feature_reference's `lifted` of the gradient map (the same weights; a few 1e-7 in relative
    L2 from the float32 T of the record that compositing_sums starts from, held to 1e-6)."""
    case, rec, f, G, (signed, absolute, _, _) = _sums(orc, name)
    W, H = case["W"], case["H"]
    assert f.shape[1] == fc.CMAX
    want, rgb = _triplets(rec, f, G, W, H)
    live = absolute > 0
    worst = float((np.abs(signed - want)[live] / absolute[live]).max())
    print(f"[{name}] six columns against the sum over triplets: worst {worst:.2e} of absolute")
    assert live.any() and (np.abs(signed - want) <= 1e-12 * absolute).all()
    assert (absolute >= np.abs(signed) * (1 - 1e-12)).all()
    lifted = fr.feature_maps(rec, W, H, fmap=G)
    # (relative L2 over the array, conftest.assert_grad_close's measure: a single element deep in a list carries one
    # float32 rounding of T per entry in front of it, 4e-6 of its own condition sum at 60 entries)
    rel = float(np.sqrt(((rgb - lifted["lifted"]) ** 2).sum() / (lifted["lifted"] ** 2).sum()))
    each = np.abs(rgb - lifted["lifted"]) / np.maximum(lifted["lifted_abs"], 1e-300)
    print(f"[{name}] the triplets' colour columns against feature_reference's lifted: relative L2 {rel:.2e}, worst element "
          f"{each[lifted['lifted_abs'] > 0].max():.2e} of its condition sum")
    assert rel <= 1e-6


def test_three_channels_are_the_three_channel_module(orc):
    """At C = 3 all four arrays are compositing_sums' (with_split) columns 3..8: the same definitions and gates."""
    case, rec, f, G, _ = _sums(orc, "tiny")
    W, H = case["W"], case["H"]
    got = fbr.feature_sums(rec, f[:, :3], G[..., :3], W, H)
    want = rbr.compositing_sums(dict(rec, rgb=f[:, :3]), G[..., :3], W, H, 0.0, with_split=True)
    for name, g, w in zip(("signed", "absolute", "borderline", "split"), got, want):
        scale = want[1][:, 3:9] + want[3][:, 3:9]
        assert (np.abs(g - w[:, 3:9]) <= 1e-12 * scale).all(), name
    assert (got[1] > 0).any() and (got[3] > 0).any()


def test_finite_differences(orc):
    """Central differences (steps of 1e-5, float64) of L = <feature_maps(out), G> on tiny over the opacity logit, uv and
    conic of the five rows with the largest `absolute` whose borderline is 0: within 1e-6 of absolute (the figure is
    printed; the bar leaves room for the O(h^2) and eps/h terms, a wrong formula is off by O(1)).  uv is in pixels here and
    in normalised device coordinates in the gradient: d pixel / d ndc = W / 2, H / 2."""
    case, rec, f, G, (signed, absolute, borderline, _) = _sums(orc, "tiny")
    W, H = case["W"], case["H"]
    G64 = G.astype(np.float64)

    def loss(r):
        return float((fr.feature_maps(r, W, H, features=f, condition=False)["out"] * G64).sum())

    order = np.argsort(-absolute.sum(1))
    picked = [int(j) for j in order if (borderline[j] == 0).all() and (absolute[j] > 0).all()][:5]
    assert len(picked) == 5
    # (key of the record, column of the key's array, column of `signed`, d parameter / d the gradient's own variable)
    params = (("opacity", None, 0, 1.0), ("conic", 0, 1, 1.0), ("conic", 1, 2, 1.0), ("conic", 2, 3, 1.0),
              ("uv", 0, 4, 0.5 * W), ("uv", 1, 5, 0.5 * H))
    worst = 0.0
    for j in picked:
        ca, _, cc = (float(x) for x in rec["conic"][j])
        for key, col, k, scale in params:
            # L itself jumps where a pair crosses the 1/255 threshold; borderline == 0 says that no pair of the row lies
            # within ALPHA_REL_TOL = 2e-3 of it, so a step must move no alpha by that much.  1e-5 on the logit or on a
            # pixel coordinate moves alpha by 1e-5 relative; on a conic entry it moves the exponent by 0.5e-5 dx^2, which
            # for the large gaussians these rows are (a ~ 1e-3, dx^2 ~ 1e3) is a percent: the conic's step is 1e-5 OF
            # the entry (of sqrt(a c) for b, which may vanish), the exponent then moves by at most 1e-5 of itself
            h = 1e-5 * {"opacity": 1.0, "uv": 1.0, "conic": (ca, np.sqrt(ca * cc), cc)[col or 0]}[key]
            vals = []
            for sgn in (1.0, -1.0):
                r = dict(rec)
                arr = np.array(rec[key], np.float64)
                if col is None:
                    arr[j] += sgn * h
                else:
                    arr[j, col] += sgn * h
                r[key] = arr
                vals.append(loss(r))
            fd = (vals[0] - vals[1]) / (2 * h) * scale
            err = abs(fd - signed[j, k]) / absolute[j, k]
            worst = max(worst, err)
            assert err <= 1e-6, f"row {j}, {fbr.COLUMNS[k]}: finite difference {fd:.9e}, signed {signed[j, k]:.9e}, {err:.2e} of absolute"
    print(f"[tiny] finite differences of the feature map, rows {picked}: worst {worst:.2e} of absolute")


@pytest.mark.parametrize("name", list(K_OBS_FEATURES))
def test_k_obs_table(orc, name):
    """The measurement behind K_OBS_FEATURES, run here: the reference's float32 mode against its float64 terms."""
    case, rec, f, G, (signed, absolute, borderline, split) = _sums(orc, name)
    s32 = fbr.feature_sums(rec, f, G, case["W"], case["H"], dtype=np.float32, with_split=False)[0]
    unit = absolute + split
    k = {n: grad_bound.observed_K(s32[:, sl], signed[:, sl], unit[:, sl], borderline[:, sl]) for n, sl in fbr.SLICES.items()}
    print(f"[K_obs features {name}, C = {f.shape[1]}] " + ", ".join(f"{n} {v:.3g}" for n, v in k.items()))
    assert (unit > 0).any()
    for n, v in k.items():
        assert v <= K_OBS_FEATURES[name][n], f"{name} {n}: K_obs {v:.4g} has grown beyond {K_OBS_FEATURES[name][n]}"
    if name == "long":
        assert int(np.diff(rec["ranges"]).max()) > 1488


@pytest.mark.parametrize("name", list(K_OBS_FEATURES))
def test_input_condition(orc, name):
    """At most 0.5 % of a scene's live elements may have borderline > 1e-2 unit (they are held to a loose bar)."""
    _, _, _, _, (_, absolute, borderline, split) = _sums(orc, name)
    unit = absolute + split
    shares = {n: grad_bound.loose_share(unit[:, sl], borderline[:, sl]) for n, sl in fbr.SLICES.items()}
    print(f"[loose share features {name}] " + ", ".join(f"{n} {100 * v:.3f}%" for n, v in shares.items()))
    for n, v in shares.items():
        assert v <= grad_bound.LOOSE_SHARE, f"{name} {n}: {100 * v:.3f} % of the live elements sit on a borderline pair"

"""The bar for a gradient array held against its float64 value (tests/render_bwd_reference.py):

    EVERY element:   |got - value64| <= K * u * unit + borderline,        u = 2^-24

unit is the element's own condition sum (|A_i| . sum_p |share_p|): what one rounding of every share is worth for THIS
gaussian, however faint it is next to the array's mean and however much its signed shares cancel.  borderline is what
the (pixel, gaussian) pairs whose alpha sits on the 1/255 threshold are worth: two correct float32 implementations may
decide them differently.  No fraction of the elements is exempt; an element whose unit and borderline are 0 (a row on
no tile list, a row behind every stop index, a fully opaque gaussian) must be exactly 0.

K is measured, not chosen: K_obs = max (|float32 oracle - value64| - borderline) / (u * unit) on the CPU, per scene and
array (tests/test_grad_bound_cpu.py keeps the tables); a GPU array is held to K = GPU_MARGIN * K_obs, the margin the
exchange tests use -- the HIP kernels and the oracle each carry that rounding and may differ in order.

The input condition: an element with borderline > LOOSE_RATIO * unit is held to a loose bar; at most LOOSE_SHARE of a
scene's live elements may be such.

The same bar holds the forward's arrays (tests/forward_reference.py, tests/test_forward_bound_*.py): there an element is an
entry of a per-gaussian array or a pixel's channel, unit its float32 running error from the float32 inputs, borderline
what the pixel's pairs on the 1/255 threshold and its stop decision are worth; rows = gaussians or pixels."""
import numpy as np

U = 2.0 ** -24
GPU_MARGIN = 4.0
LOOSE_RATIO, LOOSE_SHARE = 1e-2, 5e-3


def _2d(a, rows):
    return np.asarray(a, np.float64).reshape(rows, -1)


def ratios(got, value64, unit, borderline):
    """(|got - value64| - borderline)+ / (u * unit) per element; an element with unit 0 that is off by more than its
    borderline term gives inf."""
    rows = len(np.asarray(unit))
    got, value64, unit, borderline = (_2d(a, rows) for a in (got, value64, unit, borderline))
    excess = np.maximum(np.abs(got - value64) - borderline, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(excess == 0, 0.0, excess / (U * unit))
    return np.where(np.isnan(r), np.inf, r)


def observed_K(got, value64, unit, borderline):
    r = ratios(got, value64, unit, borderline)
    return float(r.max()) if r.size else 0.0


def loose_share(unit, borderline):
    """The share of the live elements (unit > 0) whose borderline term exceeds LOOSE_RATIO of their unit."""
    unit, borderline = np.asarray(unit, np.float64), np.asarray(borderline, np.float64)
    live = unit > 0
    return float((borderline[live] > LOOSE_RATIO * unit[live]).mean()) if live.any() else 0.0


def deepest_position(sorted_ids, ranges, M):
    """The largest list position at which each gaussian sits on any tile's list (-1: on no list)."""
    sorted_ids, ranges = np.asarray(sorted_ids), np.asarray(ranges)
    pos = np.arange(len(sorted_ids)) - np.repeat(ranges[:-1], np.diff(ranges))
    out = np.full(M, -1, np.int64)
    np.maximum.at(out, sorted_ids, pos)
    return out


def assert_within_bound(got, value64, unit, borderline, K, what, on_list=None, global_index=None, position=None,
                        populations=None):
    """Asserts the bar on every element and returns the worst ratio |got - value64| / (u * unit) reached (borderline
    excused).  on_list [rows]: rows off every list must be exactly 0.  global_index, position [rows] and populations
    (name -> rows) only serve the failure report."""
    rows = len(np.asarray(unit))
    got = _2d(got, rows)
    assert got.shape == _2d(value64, rows).shape, (what, got.shape, _2d(value64, rows).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    if on_list is not None:
        off = ~np.asarray(on_list, bool)
        assert (got[off] == 0).all(), f"{what}: a row on no tile list got a gradient"
    r = ratios(got, value64, unit, borderline)
    worst = float(r.max()) if r.size else 0.0
    if worst > K:
        row, col = np.unravel_index(int(np.argmax(r)), r.shape)
        where = f"row {row}"
        if global_index is not None:
            where += f" (global index {int(np.asarray(global_index)[row])})"
        if position is not None:
            where += f", deepest list position {int(np.asarray(position)[row])}"
        pop = [k for k, v in (populations or {}).items() if row in set(int(x) for x in v)]
        where += f", population {pop[0]}" if pop else ""
        n_bad = int((r > K).sum())
        raise AssertionError(
            f"{what}: worst |got - f64| = {worst:.3g} u*unit > K = {K:.3g} at {where}, column {col}: got "
            f"{got[row, col]:.9e}, f64 {_2d(value64, rows)[row, col]:.9e}, unit {_2d(unit, rows)[row, col]:.3e}, borderline "
            f"{_2d(borderline, rows)[row, col]:.3e}; {n_bad} of {r.size} elements beyond the bound")
    return worst

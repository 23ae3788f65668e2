"""Reference for the median (quantile) depth of a recorded forward (gsplat_context_median_depth), vectorised numpy.

contribution_reference.contribution_stats' walk -- all tiles together, one list position per numpy step, render_image's
expressions in float64 on the oracle's float32 arrays -- reduced per pixel instead of per gaussian.  With T(after i) the
transmittance behind the composited entry i (composited: i < n(p) and alpha > 1/255), it returns per pixel a BAND of list
positions the answer must lie in:

    lo[p] = the first composited entry with T(after) <= threshold (1 + eps)
    hi[p] = the first composited entry with T(after) <= threshold (1 - eps), -1 when there is none

eps = 1e-4: the project's per-pixel bar (conftest.PIXEL_L1_TOL) for a quantity of this chain -- T is a product of at most
a list's length factors below 1, each within a float32 rounding of the reference's, and 1 - T is what a pixel of the
image weighs.  lo[p] = -1 when no entry gets below the upper edge either.  -1 reads as "beyond every entry"; lo <= hi in
that order.  The band is a single position (lo == hi) except where T(after) of some entry sits within eps of the
threshold."""
import numpy as np

EPS = 1e-4


def median_band(fwd, W, H, threshold, eps=EPS, dtype=np.float64):
    """fwd: an oracle forward (uv, opacity, conic, sorted, ranges, n).  Returns (lo [H,W], hi [H,W]) int64."""
    R = np.dtype(dtype).type
    uv, conic = np.asarray(fwd["uv"], dtype), np.asarray(fwd["conic"], dtype)
    with np.errstate(over="ignore"):
        opa_all = R(1) / (R(1) + np.exp(-np.asarray(fwd["opacity"]).astype(dtype)))
    sorted_ids, ranges = np.asarray(fwd["sorted"]), np.asarray(fwd["ranges"])
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    nt = ntx * nty
    t = np.arange(nt)
    ly, lx = np.divmod(np.arange(256), 16)
    px = (t % ntx)[:, None] * 16 + lx[None, :]                  # [tiles, 256]
    py = (t // ntx)[:, None] * 16 + ly[None, :]
    by = (t // ntx)[:, None] * 16 + (ly // 8 * 8)[None, :]      # the lane's base row
    ii = np.broadcast_to((ly % 8).astype(dtype)[None, :], px.shape)
    valid = (px < W) & (py < H)
    pxc, pyc = np.minimum(px, W - 1), np.minimum(py, H - 1)
    npx = np.where(valid, np.asarray(fwd["n"]).reshape(H, W)[pyc, pxc], 0)
    top = npx.max(1) if nt else np.zeros(0, int)
    T = valid.astype(dtype)
    lo = np.full(px.shape, -1, np.int64)
    hi = np.full(px.shape, -1, np.int64)
    a_max, a_min = R(np.float32(0.99)), R(np.float32(0.00392156862))
    upper, lower = R(threshold) * (R(1) + R(eps)), R(threshold) * (R(1) - R(eps))
    pxf, byf = px.astype(dtype), by.astype(dtype)
    for idx in range(int(top.max()) if nt else 0):
        act = np.nonzero(top > idx)[0]
        g = sorted_ids[ranges[act] + idx]
        a, b, c = conic[g, 0][:, None], conic[g, 1][:, None], conic[g, 2][:, None]
        dx, dy = uv[g, 0][:, None] - pxf[act], uv[g, 1][:, None] - byf[act]
        i = ii[act]
        basic = R(-0.5) * (a * dx * dx + R(2) * b * dx * dy + c * dy * dy)
        linear, quad = c * dy + b * dx, R(-0.5) * c
        with np.errstate(all="ignore"):
            alpha = np.minimum(a_max, opa_all[g][:, None] * np.exp(np.minimum(R(0), basic + linear * i + quad * i * i)))
            on = valid[act] & (alpha > a_min) & (idx < npx[act])  # (NaN compares false: no splat)
        alpha = np.where(on, alpha, 0)
        T[act] = T[act] * (R(1) - alpha)
        lo[act] = np.where(on & (lo[act] < 0) & (T[act] <= upper), idx, lo[act])
        hi[act] = np.where(on & (hi[act] < 0) & (T[act] <= lower), idx, hi[act])
    out_lo, out_hi = np.full((H, W), -1, np.int64), np.full((H, W), -1, np.int64)
    out_lo[py[valid], px[valid]] = lo[valid]
    out_hi[py[valid], px[valid]] = hi[valid]
    return out_lo, out_hi


def outside_band(index, lo, hi):
    """The pixels whose index does not lie in [lo, hi], -1 counting as +infinity everywhere -> bool [H,W]."""
    big = np.iinfo(np.int64).max
    inf = lambda a: np.where(np.asarray(a, np.int64) < 0, big, np.asarray(a, np.int64))
    i = inf(index)
    return (i < inf(lo)) | (i > inf(hi))


def tile_of_pixels(W, H):
    """[H,W]: the index of the 16x16 tile that holds each pixel."""
    y, x = np.mgrid[0:H, 0:W]
    return (y // 16) * ((W + 15) // 16) + x // 16

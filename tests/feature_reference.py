"""Reference for the feature maps (gsplat_context_render_features, gsplat_context_lift_features), vectorised numpy.

The walk of tests/contribution_reference.py -- an oracle forward front to back, in float64 on the oracle's float32
arrays, render_image's expressions; entry i of a tile's list is composited at pixel p iff i < n(p) and alpha passes the
1/255 test, with blend weight w = alpha T(before) -- carrying the caller's channels instead of reducing the weight:

    render   out[p, c]    = sum_i w_ip f[g_i, c]           f [M,C] per gaussian, compacted order
    lift     lifted[g, c] = sum_p w_gp map[p, c]           map [H,W,C]

and, for the bounds of the tests, the two condition sums (the same sums over absolute values)

    out_abs[p, c] = sum_i w_ip |f[g_i, c]|,    lifted_abs[g, c] = sum_p w_gp |map[p, c]|

and pixels[g], the number of pixels that composite g.  `opacity` is the logit the forward composited: hand in the
EFFECTIVE one for the anti-aliased mode or the 3D filter."""
import numpy as np


def feature_maps(fwd, W, H, features=None, fmap=None, dtype=np.float64, condition=True):
    """fwd: an oracle forward (uv, opacity, conic, sorted, ranges, n); features [M,C] or None; fmap [H,W,C] or None.
    Returns dict(out [H,W,C], out_abs, lifted [M,C], lifted_abs, pixels [M] int64); the entries of a side that was not
    asked for are None, and so are the condition sums with condition=False."""
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
    M = uv.shape[0]
    pixels = np.zeros(M, np.int64)
    f = f_abs = acc = acc_abs = None
    if features is not None:
        f = np.asarray(features, dtype).reshape(M, -1)
        f_abs = np.abs(f)
        acc, acc_abs = np.zeros((nt, 256, f.shape[1]), dtype), np.zeros((nt, 256, f.shape[1]), dtype)
    m = m_abs = lifted = lifted_abs = None
    if fmap is not None:
        m = np.asarray(fmap, dtype).reshape(H, W, -1)[pyc, pxc] * valid[:, :, None]  # [tiles, 256, C]
        m_abs = np.abs(m)
        lifted, lifted_abs = np.zeros((M, m.shape[2]), dtype), np.zeros((M, m.shape[2]), dtype)
    T = valid.astype(dtype)
    a_max, a_min = R(np.float32(0.99)), R(np.float32(0.00392156862))
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
        w = alpha * T[act]
        T[act] = T[act] * (R(1) - alpha)
        np.add.at(pixels, g, on.sum(1))
        if f is not None:
            acc[act] += w[:, :, None] * f[g][:, None, :]
            if condition:
                acc_abs[act] += w[:, :, None] * f_abs[g][:, None, :]
        if m is not None:
            np.add.at(lifted, g, np.einsum("tp,tpc->tc", w, m[act]))
            if condition:
                np.add.at(lifted_abs, g, np.einsum("tp,tpc->tc", w, m_abs[act]))

    def image(tiles):
        if tiles is None:
            return None
        out = np.zeros((H, W, tiles.shape[2]), dtype)
        out[py[valid], px[valid]] = tiles[valid]
        return out

    return dict(out=image(acc), out_abs=image(acc_abs) if condition else None, lifted=lifted,
                lifted_abs=lifted_abs if condition else None, pixels=pixels)


def to_global(rows, compact_to_global, N, fill=0.0):
    """[M,C] in compacted order scattered to global gaussian order [N,C]; rows of culled gaussians are `fill`."""
    full = np.full((N,) + rows.shape[1:], fill, rows.dtype)
    full[np.asarray(compact_to_global)] = rows
    return full


def seeded_rows(n_rows, channels, seed):
    """What the tests feed both sides: uniform in [0,1], the sign flipped on every second channel."""
    v = np.random.default_rng(seed).uniform(0.0, 1.0, (n_rows, channels))
    v[:, 1::2] *= -1.0
    return v.astype(np.float32)

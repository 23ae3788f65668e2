"""Reference for the per-gaussian blend-weight statistics (gsplat_context_accumulate_contributions), vectorised numpy.

Visible gaussian j at position i of the list of the tile that holds pixel p is composited at p iff i < n(p) (the
forward's stop index) and its alpha at p passes the forward's 1/255 test; its blend weight there is
w_jp = alpha_jp T_p(before j).  This module walks an oracle forward front to back -- render_image's expressions: the row
polynomial basic + linear i + quad i^2 on the lane's base row, min(0, power), the 0.99 cap, alpha > 1/255, T <- T (1 -
alpha) -- in float64 on the oracle's float32 arrays and returns, per gaussian in compacted order,

    weight_sum[j] = sum_p w_jp,    weight_max[j] = max_p w_jp,    pixels[j] = the number of pixels that composite j.

All tiles advance together, one list position per numpy step (tests/absgrad_reference.py walks the same lists back to
front).  `opacity` is the logit the forward composited: hand in the EFFECTIVE one for the anti-aliased mode or the 3D
filter."""
import numpy as np


def contribution_stats(fwd, W, H, dtype=np.float64):
    """fwd: an oracle forward (uv, opacity, conic, sorted, ranges, n).  Returns (weight_sum [M], weight_max [M],
    pixels [M] int64)."""
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
    w_sum, w_max, pixels = np.zeros(M, dtype), np.zeros(M, dtype), np.zeros(M, np.int64)
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
        np.add.at(w_sum, g, w.sum(1))
        np.maximum.at(w_max, g, w.max(1))
        np.add.at(pixels, g, on.sum(1))
    return w_sum, w_max, pixels


def to_global(stats, compact_to_global, N):
    """The three compacted arrays scattered to global gaussian order [N]; rows of culled gaussians are 0."""
    out = []
    for s in stats:
        full = np.zeros(N, s.dtype)
        full[np.asarray(compact_to_global)] = s
        out.append(full)
    return tuple(out)


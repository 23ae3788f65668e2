"""Reference for the feature map's gradient with respect to the geometry (gsplat_context_features_backward), numpy.

out[p, c] = sum_i w_ip f[g_i, c] is the forward's image with colours f, pixel gradient G = dL/d out and background 0,
for any number of channels C: with d_i(p) = sum_c G[p, c] f[g_i, c],

    dL/d alpha_i(p) = T_i (d_i - s_i),      s_i = G . (the features composited behind entry i) at p,

and from it the shares of d/d opacity logit (1), d/d conic (3) and d/d uv (2) exactly as
tests/render_bwd_reference.py::compositing_sums forms them (the row polynomial on the lane's base row, the recurrence of
T, the 0.99 clamp differentiated as if absent, the 1/255 threshold, the gate per tile, nothing for sigma(logit) == 1 in
float32).  feature_sums returns, per visible gaussian and for these six columns (COLUMNS), compositing_sums' four arrays:

    signed      the gradient
    absolute    sum_p |share_p|, the shares of ALL channels together (the gate per pixel)
    borderline  sum |share_p| over the pairs whose float64 alpha lies within ALPHA_REL_TOL of 1/255
    split       what the cancellations inside a share add to its condition sum (render_bwd_reference's text): here ga's
                own terms are sum_c (|f_c| + |behind_c|) |G_c| T -- a sum over C channels of random sign, which is also
                what the channel chunks of the kernel cancel among themselves.

The walk is the kernel's (gs_replay.hip: features_bwd_kernel), not compositing_sums': channels in chunks of CHUNK = 16,
every chunk with its own scalar s (t = d_i - s, s <- s + alpha t) and its own sums, the chunks' sums added at the end.
In float64 that is the same number as compositing_sums' vector form to 1e-16 (tests/test_features_bwd_cpu.py holds it to
the sum over channel triplets of compositing_sums itself).  dtype=np.float32 models the kernel's summation: d_i chained
in float32 in channel order within a chunk (a product, then fused multiply-adds), the recurrence's fma, every share and
every sum in float32, the chunks added in float32.  (A chunk narrower than 16 is padded with zero channels, which add
exact zeros to the chain: the kernel's K = 4 and 8 are the same chain.)

bound_terms wraps render_bwd_reference.geometry64 / chain_matrix for the leaves: the columns ride as columns 3..8 of
the nine, with zeros in the colour columns."""
import numpy as np

import render_bwd_reference as rbr

COLUMNS = rbr.COLUMNS[3:9]
SLICES = dict(opacity=slice(0, 1), conic=slice(1, 4), uv=slice(4, 6))
CHUNK = 16


def _fma(a, b, c, dtype):
    """a * b + c with one rounding (float32: the product of two float32 is exact in float64, the sum rounds once more to
    53 bits before the 24: a double rounding on one sum in 2^29)."""
    if np.dtype(dtype) == np.float64:
        return a * b + c
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def feature_sums(fwd, features, grad_map, W, H, dtype=np.float64, with_split=True):
    """fwd: a forward record (uv, opacity, conic, sorted, ranges, n, T; `opacity` the logit the forward composited);
    features [M,C] in compacted order, grad_map [H,W,C].  Returns (signed, absolute, borderline, split), each [M, 6] in
    the order of COLUMNS; split is zeros with with_split=False."""
    R = np.dtype(dtype).type
    uv, conic = np.asarray(fwd["uv"], dtype).reshape(-1, 2), np.asarray(fwd["conic"], dtype).reshape(-1, 3)
    logit_in = np.asarray(fwd["opacity"]).reshape(-1)
    with np.errstate(over="ignore"):
        opa_gate = (1.0 / (1.0 + np.exp(-logit_in))).astype(logit_in.dtype) == 1  # sigma == 1 in the inputs' precision
        opa_all = R(1) / (R(1) + np.exp(-logit_in.astype(dtype)))
    M = uv.shape[0]
    f = np.asarray(features, dtype).reshape(M, -1)
    C = f.shape[1]
    nch = (C + CHUNK - 1) // CHUNK
    fpad = np.zeros((M, nch * CHUNK), dtype)
    fpad[:, :C] = f
    G = np.zeros((H, W, nch * CHUNK), dtype)
    G[..., :C] = np.asarray(grad_map, dtype).reshape(H, W, C)
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
    npx = np.minimum(npx, np.diff(ranges)[:nt, None])
    Tf = np.where(valid, np.asarray(fwd["T"], dtype).reshape(H, W)[pyc, pxc], 0)
    Gp = np.where(valid[..., None], G[pyc, pxc], 0)             # [tiles, 256, nch * CHUNK]
    Gc = Gp.reshape(nt, 256, nch, CHUNK)
    fc = fpad.reshape(M, nch, CHUNK)
    T = Tf.copy()
    s = np.zeros((nt, 256, nch), dtype)                         # per chunk: G . (the features behind)
    acc = np.zeros((nt, 256, nch * CHUNK), dtype) if with_split else None  # the features behind, per channel
    top = npx.max(1) if nt else np.zeros(0, int)
    signed_k = np.zeros((M, nch, 6), dtype)
    absolute, borderline, split = (np.zeros((M, 6), dtype) for _ in range(3))
    a_max, a_min = R(np.float32(0.99)), R(np.float32(0.00392156862))
    halfW, halfH = R(0.5) * R(W), R(0.5) * R(H)
    pxf, byf, pyf = px.astype(dtype), by.astype(dtype), py.astype(dtype)
    tcx = ((t % ntx) * 16 + 7.5).astype(dtype)[:, None]        # the tile's centre
    tcy = ((t // ntx) * 16 + 7.5).astype(dtype)[:, None]

    def shares(gpow, g_o, a, b, c, dx, dy, i):
        """compositing_sums' S[..., 3:9]; gpow and g_o may carry a trailing chunk axis."""
        if gpow.ndim == 3:
            a, b, c, dx, dy, i = (x[..., None] for x in (a, b, c, dx, dy, i))
        S = np.empty(gpow.shape + (6,), dtype)
        S[..., 0] = g_o
        S[..., 1] = gpow * (R(-0.5) * dx * dx)
        S[..., 2] = gpow * (-dx * dy) + (gpow * i) * dx
        S[..., 3] = gpow * (R(-0.5) * dy * dy) + (gpow * i) * dy - R(0.5) * (gpow * i * i)
        S[..., 4] = ((-a * dx - b * dy) * gpow + b * (gpow * i)) * halfW
        S[..., 5] = ((-c * dy - b * dx) * gpow + c * (gpow * i)) * halfH
        return S

    for idx in range(int(top.max()) - 1 if nt else -1, -1, -1):
        act = np.nonzero(top > idx)[0]
        g = sorted_ids[ranges[act] + idx]
        a, b, c = conic[g, 0][:, None], conic[g, 1][:, None], conic[g, 2][:, None]
        opa = opa_all[g][:, None]
        dx, dy = uv[g, 0][:, None] - pxf[act], uv[g, 1][:, None] - byf[act]
        i = ii[act]
        basic = R(-0.5) * (a * dx * dx + R(2) * b * dx * dy + c * dy * dy)
        linear, quad = c * dy + b * dx, R(-0.5) * c
        with np.errstate(all="ignore"):
            gg = np.exp(np.minimum(R(0), basic + linear * i + quad * i * i))
            raw = opa * gg
            reach = valid[act] & (idx < npx[act])
            vs = reach & (np.minimum(a_max, raw) >= a_min)
            near = reach & (np.abs(raw - a_min) <= R(rbr.ALPHA_REL_TOL) * a_min)
        cand = vs | near                                        # a pair just below 1/255 is valued as if composited
        alpha = np.where(cand, np.minimum(a_max, raw), 0)
        Tprev = T[act]
        below = near & ~vs                                      # as if composited: the T in front of it is Tprev itself
        Ti = np.where(below, Tprev, Tprev * (R(1) / (R(1) - alpha)))
        T[act] = np.where(vs, Ti, Tprev)
        # d_i per chunk: one chain in channel order
        fg, Ga = fc[g][:, None], Gc[act]                        # [act, 1, nch, CHUNK], [act, 256, nch, CHUNK]
        d = fg[..., 0] * Ga[..., 0]
        for ch in range(1, CHUNK):
            d = _fma(fg[..., ch], Ga[..., ch], d, dtype)
        s_act = s[act]
        tt = d - s_act                                          # [act, 256, nch]
        ga_k = tt * Ti[..., None]
        s[act] = np.where(vs[..., None], _fma(alpha[..., None], tt, s_act, dtype), s_act)
        ga = ga_k[..., 0]
        for k in range(1, nch):
            ga = ga + ga_k[..., k]
        candk = cand[..., None]
        gpow_k = np.where(candk, gg[..., None] * (ga_k * opa[..., None]), 0)
        g_o_k = np.where(candk, gg[..., None] * ga_k * opa[..., None] * (R(1) - opa[..., None]), 0)
        S_k = shares(gpow_k, g_o_k, a, b, c, dx, dy, i)         # [act, 256, nch, 6]
        open_tile_k = ((g_o_k != 0) & vs[..., None]).any(1) & ~opa_gate[g][:, None]  # [act, nch]
        np.add.at(signed_k, g, (S_k * vs[..., None, None]).sum(1) * open_tile_k[..., None])
        # the condition sums: the shares of all channels together
        gpow = np.where(cand, gg * (ga * opa), 0)
        g_o = np.where(cand, gg * ga * opa * (R(1) - opa), 0)
        S = shares(gpow, g_o, a, b, c, dx, dy, i)
        open_px = (g_o != 0) & ~opa_gate[g][:, None]
        A = np.abs(S) * open_px[..., None]
        np.add.at(absolute, g, (A * vs[..., None]).sum(1))
        np.add.at(borderline, g, (A * near[..., None]).sum(1))
        if with_split:
            cg = fpad[g][:, None, :]
            ga_abs = ((np.abs(cg) + np.abs(acc[act])) * np.abs(Gp[act])).sum(-1) * Ti
            a_vs = np.where(vs, alpha, 0)[..., None]
            acc[act] = a_vs * cg + (R(1) - a_vs) * acc[act]
            Q = np.where(cand, gg * opa, 0)
            ga_m = np.abs(ga)
            F = np.zeros_like(S)
            F[..., 0] = R(1) + opa                              # 1 - opa is a difference: off by u (1 + opa)
            # the oracle's form, on the lane's base row | the kernel's form, moments about the tile centre: the larger
            mx = np.abs(uv[g, 0][:, None] - tcx[act]) + np.abs(pxf[act] - tcx[act])
            my = np.abs(uv[g, 1][:, None] - tcy[act]) + np.abs(pyf[act] - tcy[act])
            ax, ay = np.abs(dx), np.abs(dy) + i
            F[..., 1] = np.maximum(R(0.5) * ax * ax, R(0.5) * mx * mx)
            F[..., 2] = np.maximum(ax * ay, mx * my)
            F[..., 3] = np.maximum(R(0.5) * ay * ay, R(0.5) * my * my)
            F[..., 4] = np.maximum(np.abs(a) * ax + np.abs(b) * ay, np.abs(a) * mx + np.abs(b) * my) * halfW
            F[..., 5] = np.maximum(np.abs(c) * ay + np.abs(b) * ax, np.abs(c) * my + np.abs(b) * mx) * halfH
            pw = (R(0.5) * (np.abs(a) * dx * dx + R(2) * np.abs(b * dx * dy) + np.abs(c) * dy * dy)
                  + (np.abs(c * dy) + np.abs(b * dx)) * i + R(0.5) * np.abs(c) * i * i)
            X = np.abs(S) * pw[..., None]                       # exp(power): off by u times the power's own terms
            with np.errstate(divide="ignore", invalid="ignore"):
                f_m = np.where(ga_m[..., None] > 0, np.abs(S) / (Q * ga_m)[..., None], 0)  # |f|
            X += (Q * (ga_abs - ga_m))[..., None] * f_m + (Q * ga_m)[..., None] * np.maximum(F - f_m, 0)
            X = np.nan_to_num(X)
            np.add.at(split, g, (np.maximum(X, 0) * (open_px & vs)[..., None]).sum(1))
    signed = signed_k[:, 0].copy()
    for k in range(1, nch):
        signed = signed + signed_k[:, k]
    return signed, absolute, borderline, split


def bound_terms(fwd, leaves, cam, features, grad_map, l_max, mh_dist):
    """What the bar needs (tests/grad_bound.py).  Returns dict name -> (value64, unit, borderline), each [M, d], for
    opacity, conic and uv and for the leaves leaf_xyz, leaf_opacity, leaf_scale, leaf_quaternion, plus "on_list" [M]
    and the plain "absolute"."""
    W, H = int(cam["width"]), int(cam["height"])
    signed, absolute, border, split = feature_sums(fwd, features, grad_map, W, H)
    unit = absolute + split
    out = {name: (signed[:, sl], unit[:, sl], border[:, sl]) for name, sl in SLICES.items()}
    nine = lambda x: np.concatenate([np.zeros((len(x), 3)), x], 1)
    A = rbr.chain_matrix(rbr.geometry64(leaves, cam, mh_dist, l_max), 9)
    v, u, b = rbr.apply(A, nine(signed)), rbr.apply(A, nine(unit), True), rbr.apply(A, nine(border), True)
    for leaf in ("xyz", "opacity", "scale", "quaternion"):
        out["leaf_" + leaf] = (v[leaf], u[leaf], b[leaf])
    on_list = np.zeros(len(signed), bool)
    on_list[np.asarray(fwd["sorted"])] = True
    out["on_list"], out["absolute"] = on_list, absolute
    return out

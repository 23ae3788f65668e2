"""Reference for absgrad mode (gsplat_context_set_absgrad), vectorised numpy.

render_image_backward adds, for a visible gaussian j and every pixel p that composites it, the pixel's share
(du_p, dv_p) to grad_uv[j] (0.5 W / 0.5 H factors included; nothing when the :170 gate is closed).  This module forms
those shares exactly as the oracle does -- the row polynomial basic + linear i + quad i^2 on the lane's base row, the
recurrences of T and of the colour behind, the gate -- and returns per gaussian both

    signed[j] = sum_p (du_p, dv_p)   (= the oracle's grad_uv)        absolute[j] = sum_p (|du_p|, |dv_p|).

The gate: the oracle drops a (gaussian, tile) pair when d/d logit = gg ga opa (1 - opa) is zero on every lane.  The
absolute sums are DEFINED as the sum over single-pixel calls (the gradient image non-zero at p only), so their gate is
per pixel: the share of p counts iff that pixel's d/d logit is non-zero.  sigma(opacity) for the gate is evaluated in
the dtype of the opacity array handed in: float32 inputs summed in float64 still drop a logit-20 gaussian, whose float32
sigmoid is exactly 1, as a float32 implementation does.

Depth mode: pass `z` (the gaussians' camera-space depth) and grad_depth / grad_alpha; the two channels (z, 1) over
background 0 join the colour channels, which is tests/depth_reference.py's sum of two render_image_backward calls per pixel.
All tiles advance together, one list position per numpy step."""
import numpy as np


def absgrad_sums(fwd, grad_image, W, H, bg, grad_depth=None, grad_alpha=None, z=None, dtype=np.float64):
    """fwd: an oracle forward (uv, opacity, conic, rgb, sorted, ranges, n, T).  Returns (signed [M,2], absolute [M,2])."""
    R = np.dtype(dtype).type
    uv, conic = np.asarray(fwd["uv"], dtype), np.asarray(fwd["conic"], dtype)
    logit_in = np.asarray(fwd["opacity"])
    opa_gate = (1.0 / (1.0 + np.exp(-logit_in))).astype(logit_in.dtype) == 1  # sigma == 1 in the inputs' precision
    opa_all = R(1) / (R(1) + np.exp(-logit_in.astype(dtype)))
    col = np.asarray(fwd["rgb"], dtype)
    G = np.asarray(grad_image, dtype).reshape(H, W, 3)
    bgc = np.full(3, bg, dtype)
    if grad_depth is not None or grad_alpha is not None:
        zc = np.asarray(z, dtype).reshape(-1, 1)
        col = np.concatenate([col, zc, np.ones_like(zc)], 1)
        gd = np.zeros((H, W), dtype) if grad_depth is None else np.asarray(grad_depth, dtype)
        ga_ = np.zeros((H, W), dtype) if grad_alpha is None else np.asarray(grad_alpha, dtype)
        G = np.concatenate([G, gd[..., None], ga_[..., None]], -1)
        bgc = np.concatenate([bgc, np.zeros(2, dtype)])
    C = col.shape[1]
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
    Tf = np.where(valid, np.asarray(fwd["T"], dtype).reshape(H, W)[pyc, pxc], 0)
    Gp = np.where(valid[..., None], G[pyc, pxc], 0)            # [tiles, 256, C]
    bgdot = (Gp * bgc).sum(-1)
    T = Tf.copy()
    acc = np.zeros(px.shape + (C,), dtype)
    top = npx.max(1)
    M = uv.shape[0]
    signed, absolute = np.zeros((M, 2), dtype), np.zeros((M, 2), dtype)
    a_max, a_min = R(np.float32(0.99)), R(np.float32(0.00392156862))
    halfW, halfH = R(0.5) * R(W), R(0.5) * R(H)
    pxf, byf = px.astype(dtype), by.astype(dtype)
    for idx in range(int(top.max()) - 1 if nt else -1, -1, -1):
        act = np.nonzero(top > idx)[0]
        g = sorted_ids[ranges[act] + idx]
        a, b, c = conic[g, 0][:, None], conic[g, 1][:, None], conic[g, 2][:, None]
        opa = opa_all[g][:, None]
        dx, dy = uv[g, 0][:, None] - pxf[act], uv[g, 1][:, None] - byf[act]
        i = ii[act]
        basic = R(-0.5) * (a * dx * dx + R(2) * b * dx * dy + c * dy * dy)
        linear, quad = c * dy + b * dx, R(-0.5) * c
        gg = np.exp(np.minimum(R(0), basic + linear * i + quad * i * i))
        alpha = np.minimum(a_max, opa * gg)
        vs = valid[act] & (alpha >= a_min) & (idx < npx[act])
        alpha = np.where(vs, alpha, 0)
        Ti = T[act] * (R(1) / (R(1) - alpha))
        T[act] = Ti
        cg = col[g][:, None, :]
        ga = ((cg - acc[act]) * Gp[act]).sum(-1) * Ti + (-Tf[act] / (R(1) - alpha)) * bgdot[act]
        acc[act] = alpha[..., None] * cg + (R(1) - alpha[..., None]) * acc[act]
        g_o = np.where(vs, gg * ga * opa * (R(1) - opa), 0)
        gpow = np.where(vs, gg * (ga * opa), 0)
        du = ((-a * dx - b * dy) * gpow + b * (gpow * i)) * halfW
        dv = ((-c * dy - b * dx) * gpow + c * (gpow * i)) * halfH
        open_px = (g_o != 0) & ~opa_gate[g][:, None]
        open_tile = (g_o != 0).any(1)
        np.add.at(signed, g, np.stack([(du * open_tile[:, None]).sum(1), (dv * open_tile[:, None]).sum(1)], 1))
        np.add.at(absolute, g, np.stack([(np.abs(du) * open_px).sum(1), (np.abs(dv) * open_px).sum(1)], 1))
    return signed, absolute

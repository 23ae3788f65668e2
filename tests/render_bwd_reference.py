"""The compositing backward in float64 with its condition sums, and the per-gaussian chain behind it as a matrix.

render_image_backward adds, for a visible gaussian j and every pixel p that composites it, the pixel's share to nine
sums: d/d precompute_rgb (3), d/d opacity logit (1), d/d conic (3), d/d uv (2) -- and in depth mode, where the two
channels (z, 1) over background 0 join the colour channels, a tenth: dL/dz.  compositing_sums forms those shares exactly
as the oracle does (tests/absgrad_reference.py is the pattern: the row polynomial basic + linear i + quad i^2 on the
lane's base row, the recurrences of T and of the colour behind, the 0.99 clamp, the 1/255 threshold, the gate per tile)
and returns per gaussian

    signed[j]     = sum_p share_p            the gradient
    absolute[j]   = sum_p |share_p|          its condition sum: a float32 evaluation of signed[j], whatever its order,
                                             is off by a small multiple of 2^-24 * absolute[j], however much the signed
                                             shares cancel (gate per pixel, as absgrad_reference defines it)
    borderline[j] = sum |share_p| over the (pixel, gaussian) pairs whose float64 alpha lies within ALPHA_REL_TOL of 1/255,
                    pairs just below the threshold included and valued as if they were composited: two correct float32
                    implementations may decide such a pair differently (parity_tools.explain's alpha_rel_tol).

The forward record (uv, opacity, conic, rgb: float32 values as produced, widened; sorted, ranges, n, T: as given) is not
re-derived: the stop indices and final transmittances are the forward's own.

chain_matrix evaluates the chain from these ten gradients to the six leaves (xyz, band0, sh, opacity, scale, quaternion)
with the oracle's float64 instantiations, once per unit incoming gradient over all rows at once: the chain is linear in
the incoming gradient for fixed parameters, so the calls give each gaussian's matrix A_i, and

    leaf64 = A_i . signed_i        unit = |A_i| . absolute_i        propagated borderline = |A_i| . borderline_i.

The unit of the bar (bound_terms) is absolute + split.  |share_p| alone does not bound what a correct float32 evaluation
loses, because a share is itself a sum of terms that cancel, in four places (the float32 oracle against this module: a
gaussian whose only pixel lies 0.0025 rows from its centre misses u*|share| by 2.4e5, a one-pixel gaussian behind 1400
list entries by 6.2e3):

  * every share of opacity, conic and uv carries the factor ga = sum_c (colour_c - behind_c) G_c T - T_final/(1-alpha)
    bg.G, a sum over channels of random sign: its float32 value is off by u times ga_abs = sum_c (|colour_c| +
    |behind_c|) |G_c| T + T_final/(1-alpha) |bg| sum_c |G_c|, not u |ga|;
  * the opacity share carries 1 - sigma(logit), a difference of two numbers of size 1: off by u (1 + sigma), which for a
    logit of 6 is 400 times u (1 - sigma);
  * every share carries exp(power), power = basic + linear i + quad i^2 on the lane's base row: terms of up to
    0.5 c 15^2 for a sum between -5.5 and 0, so exp(power) is off by u times pw = the sum of the terms' magnitudes,
    relatively: the share's condition number gains pw;
  * the conic and uv shares are formed on the lane's base row as g_basic f(dx, dy) + g_lin f'(dx, dy) + g_quad f'':
    d/dc is -0.5 gpow (dy - i)^2 evaluated as gpow (-0.5 dy^2 + dy i - 0.5 i^2), three terms of up to 0.5 * 15^2 for a
    result that vanishes on the gaussian's own row; likewise d/db = gpow (-dx dy + dx i), du = gpow (-a dx - b dy + b i),
    dv = gpow (-c dy - b dx + c i).  The HIP kernels form the same sums another way: per tile, the moments of gpow
    about the tile's centre (sum gpow, gpow ox, gpow oy, gpow ox^2, gpow ox oy, gpow oy^2 with o = pixel - centre,
    |o| <= 7.5, products and row sums in float32), shifted to the gaussian's centre at the end: sum gpow dx^2 =
    X^2 S_1 - 2 X S_x + S_xx with X = u - centre, whose terms are gpow (|X| + |ox|)^2 for a result gpow (X - ox)^2.
    Both are correct float32 evaluations; F takes, per share, the larger of the two forms' term sums.

The segmented backward (gs_render.h: TileSegments; `checkpoints` = dict(image, entries, split_min)): a list longer than
split_min is walked in segments of `entries`, and a pixel that stops behind a segment's far boundary B enters it with the
forward's checkpoint {T_b, C_b}: the colour behind B is recovered as (image - C_b) / T_b, a difference of two float32
numbers of the size of the image for a result of the size of T_b -- off by u e_ck, e_ck = sum_c |g_c| (|image_c| +
|C_b,c|), whatever T_b is.  The recurrence of the colour behind is linear and hands that error, times T_b / T_i (1 -
alpha), to every entry i of the segment: ga_i is off by u e_ck / (1 - alpha_i), which ga_abs takes in for those pairs.
Behind 1500 faint entries T_b is 1e-3 .. 1e-4, so this term is what bounds such rows in a segmented backward (measured
on the GPU without it: 4e3 u * unit for opacity, conic and uv, the whole-list backward of the same scene 7).

split[j] = sum_p |share_p| (pw + (ga_abs - |ga|) / |ga| + (F - |f|) / |f|) >= 0, f the share's last factor (1 - sigma, or
the row polynomial's value) and F the same with every term taken absolutely: what the four cancellations add to the
condition sum, to first order in u (the relative errors of a product's factors add).  `absolute` itself stays the plain
sum of |share_p|, which is what tests/absgrad_reference.py defines and the absgrad mode accumulates.

Sigma, J and the conic are recomputed in float64 from the float32 leaf parameters and the camera."""
import numpy as np

import edge_scenes

COLUMNS = ("rgb_r", "rgb_g", "rgb_b", "opacity", "conic_a", "conic_b", "conic_c", "uv_u", "uv_v", "z")
SLICES = dict(precompute_rgb=slice(0, 3), opacity=slice(3, 4), conic=slice(4, 7), uv=slice(7, 9), z=slice(9, 10))
ALPHA_REL_TOL = 2e-3  # parity_tools.explain: alpha_rel_tol
LEAVES = ("xyz", "band0", "sh", "opacity", "scale", "quaternion")
# d/d sh_k = Y_k(direction) d/d rgb.  Y_k is a polynomial of degree <= 3 in the unit direction whose monomials sum, taken
# absolutely, to at most 1.5 on the sphere (0.373 z (2 z^2 - 3 x^2 - 3 y^2) at the pole: 0.75; 0.457 x (4 z^2 - x^2 -
# y^2): at most 1.1; 1.445 z (x^2 - y^2) ...), while Y_k itself vanishes on its nodal lines: a float32 basis value is off
# by u * that sum, not by u |Y_k| (the float32 oracle: 4.6e3 u |Y_k| |d rgb| on `small`).  The sh unit takes the sum.
SH_TERMS = 1.5


def compositing_sums(fwd, grad_image, W, H, bg, grad_depth=None, grad_alpha=None, z=None, dtype=np.float64,
                     with_split=False, checkpoints=None):
    """fwd: a forward record (uv, opacity, conic, rgb, sorted, ranges, n, T).  Returns (signed, absolute, borderline),
    each [M, 9] in the order of COLUMNS, [M, 10] in depth mode (grad_depth or grad_alpha given, with z); with_split adds
    the fourth array `split` (see the module's text)."""
    R = np.dtype(dtype).type
    uv, conic = np.asarray(fwd["uv"], dtype).reshape(-1, 2), np.asarray(fwd["conic"], dtype).reshape(-1, 3)
    logit_in = np.asarray(fwd["opacity"]).reshape(-1)
    opa_gate = (1.0 / (1.0 + np.exp(-logit_in))).astype(logit_in.dtype) == 1  # sigma == 1 in the inputs' precision
    opa_all = R(1) / (R(1) + np.exp(-logit_in.astype(dtype)))
    col = np.asarray(fwd["rgb"], dtype).reshape(-1, 3)
    G = np.asarray(grad_image, dtype).reshape(H, W, 3)
    bgc = np.full(3, bg, dtype)
    depth = grad_depth is not None or grad_alpha is not None
    if depth:
        zc = np.asarray(z, dtype).reshape(-1, 1)
        col = np.concatenate([col, zc, np.ones_like(zc)], 1)
        gd = np.zeros((H, W), dtype) if grad_depth is None else np.asarray(grad_depth, dtype)
        ga_ = np.zeros((H, W), dtype) if grad_alpha is None else np.asarray(grad_alpha, dtype)
        G = np.concatenate([G, gd[..., None], ga_[..., None]], -1)
        bgc = np.concatenate([bgc, np.zeros(2, dtype)])
    K = 10 if depth else 9
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
    acc = np.zeros(px.shape + (col.shape[1],), dtype)
    top = npx.max(1) if nt else np.zeros(0, int)
    M = uv.shape[0]
    signed, absolute, borderline, split = (np.zeros((M, K), dtype) for _ in range(4))
    a_max, a_min = R(np.float32(0.99)), R(np.float32(0.00392156862))
    halfW, halfH = R(0.5) * R(W), R(0.5) * R(H)
    pxf, byf, pyf = px.astype(dtype), by.astype(dtype), py.astype(dtype)
    tcx = ((t % ntx) * 16 + 7.5).astype(dtype)[:, None]        # the tile's centre
    tcy = ((t // ntx) * 16 + 7.5).astype(dtype)[:, None]
    if checkpoints is not None:  # the segmented backward (see the module's text)
        assert with_split and not depth
        seg_n, seg_min = int(checkpoints["entries"]), int(checkpoints["split_min"])
        img = np.where(valid[..., None], np.asarray(checkpoints["image"], dtype).reshape(H, W, 3)[pyc, pxc], 0)
        is_split = np.diff(ranges)[:nt] > seg_min
        e_ck = np.zeros(px.shape, dtype)
    for idx in range(int(top.max()) - 1 if nt else -1, -1, -1):
        act = np.nonzero(top > idx)[0]
        if checkpoints is not None and (idx + 1) % seg_n == 0:
            # T, acc: the state in front of entry idx + 1, a boundary.  The pixels that stop behind it enter there with
            # s T_b = sum_c g_c (image_c - C_b,c), C_b = image - T_b acc - T_final bg: off by u times e_ck
            c_b = img - T[..., None] * acc - (Tf[..., None] * bgc)
            e_ck = np.where(is_split[:, None] & (npx > idx + 1), (np.abs(Gp) * (np.abs(img) + np.abs(c_b))).sum(-1), 0)
        g = sorted_ids[ranges[act] + idx]
        a, b, c = conic[g, 0][:, None], conic[g, 1][:, None], conic[g, 2][:, None]
        opa = opa_all[g][:, None]
        dx, dy = uv[g, 0][:, None] - pxf[act], uv[g, 1][:, None] - byf[act]
        i = ii[act]
        basic = R(-0.5) * (a * dx * dx + R(2) * b * dx * dy + c * dy * dy)
        linear, quad = c * dy + b * dx, R(-0.5) * c
        gg = np.exp(np.minimum(R(0), basic + linear * i + quad * i * i))
        raw = opa * gg
        reach = valid[act] & (idx < npx[act])
        vs = reach & (np.minimum(a_max, raw) >= a_min)
        near = reach & (np.abs(raw - a_min) <= R(ALPHA_REL_TOL) * a_min)
        cand = vs | near                                        # a pair just below 1/255 is valued as if composited
        alpha = np.where(cand, np.minimum(a_max, raw), 0)
        Tprev = T[act]
        below = near & ~vs                                      # as if composited: the T in front of it is Tprev itself
        Ti = np.where(below, Tprev, Tprev * (R(1) / (R(1) - alpha)))
        T[act] = np.where(vs, Ti, Tprev)
        Tbg = np.where(below, Tf[act], Tf[act] / (R(1) - alpha))
        cg = col[g][:, None, :]
        ga = ((cg - acc[act]) * Gp[act]).sum(-1) * Ti + (-Tbg) * bgdot[act]
        if with_split:  # ga's own terms, each taken absolutely
            ga_abs = (((np.abs(cg) + np.abs(acc[act])) * np.abs(Gp[act])).sum(-1) * Ti
                      + Tbg * (np.abs(Gp[act]) * np.abs(bgc)).sum(-1))
            if checkpoints is not None:
                ga_abs = ga_abs + e_ck[act] / (R(1) - alpha)
        a_vs = np.where(vs, alpha, 0)[..., None]
        acc[act] = a_vs * cg + (R(1) - a_vs) * acc[act]
        g_o = np.where(cand, gg * ga * opa * (R(1) - opa), 0)
        gpow = np.where(cand, gg * (ga * opa), 0)
        w = np.where(cand, alpha * Ti, 0)
        S = np.empty(gg.shape + (K,), dtype)                    # the shares, [tiles, 256, K]
        S[..., 0:3] = w[..., None] * Gp[act][..., 0:3]
        S[..., 3] = g_o
        S[..., 4] = gpow * (R(-0.5) * dx * dx)
        S[..., 5] = gpow * (-dx * dy) + (gpow * i) * dx
        S[..., 6] = gpow * (R(-0.5) * dy * dy) + (gpow * i) * dy - R(0.5) * (gpow * i * i)
        S[..., 7] = ((-a * dx - b * dy) * gpow + b * (gpow * i)) * halfW
        S[..., 8] = ((-c * dy - b * dx) * gpow + c * (gpow * i)) * halfH
        if depth:
            S[..., 9] = w * Gp[act][..., 3]
        open_px = (g_o != 0) & ~opa_gate[g][:, None]
        open_tile = ((g_o != 0) & vs).any(1) & ~opa_gate[g]     # sigma == 1 in float32: no float32 path adds anything
        np.add.at(signed, g, (S * vs[..., None]).sum(1) * open_tile[:, None])
        A = np.abs(S) * open_px[..., None]
        np.add.at(absolute, g, (A * vs[..., None]).sum(1))
        np.add.at(borderline, g, (A * near[..., None]).sum(1))
        if with_split:
            # to first order the relative errors of a share's factors ADD: |share| (pw + ga_abs / |ga| + F / |f|), with f
            # the share's own last factor and F the same with every term taken absolutely
            Q = np.where(cand, gg * opa, 0)
            ga_m = np.abs(ga)
            F = np.zeros_like(S)
            F[..., 3] = R(1) + opa                              # 1 - opa is a difference: off by u (1 + opa)
            # the oracle's form, on the lane's base row | the kernels' form, moments about the tile centre: the larger
            mx = np.abs(uv[g, 0][:, None] - tcx[act]) + np.abs(pxf[act] - tcx[act])
            my = np.abs(uv[g, 1][:, None] - tcy[act]) + np.abs(pyf[act] - tcy[act])
            ax, ay = np.abs(dx), np.abs(dy) + i
            F[..., 4] = np.maximum(R(0.5) * ax * ax, R(0.5) * mx * mx)
            F[..., 5] = np.maximum(ax * ay, mx * my)
            F[..., 6] = np.maximum(R(0.5) * ay * ay, R(0.5) * my * my)
            F[..., 7] = np.maximum(np.abs(a) * ax + np.abs(b) * ay, np.abs(a) * mx + np.abs(b) * my) * halfW
            F[..., 8] = np.maximum(np.abs(c) * ay + np.abs(b) * ax, np.abs(c) * my + np.abs(b) * mx) * halfH
            pw = (R(0.5) * (np.abs(a) * dx * dx + R(2) * np.abs(b * dx * dy) + np.abs(c) * dy * dy)
                  + (np.abs(c * dy) + np.abs(b * dx)) * i + R(0.5) * np.abs(c) * i * i)
            X = np.abs(S) * pw[..., None]                       # exp(power): off by u times the power's own terms
            Sm = np.abs(S[..., 3:9])
            with np.errstate(divide="ignore", invalid="ignore"):
                f_m = np.where(ga_m[..., None] > 0, Sm / (Q * ga_m)[..., None], 0)  # |f|
            X[..., 3:9] += (Q * (ga_abs - ga_m))[..., None] * f_m + (Q * ga_m)[..., None] * np.maximum(F[..., 3:9] - f_m, 0)
            X = np.nan_to_num(X)
            np.add.at(split, g, (np.maximum(X, 0) * (open_px & vs)[..., None]).sum(1))
    if with_split:
        return signed, absolute, borderline, split
    return signed, absolute, borderline


def geometry64(leaves, cam, mh_dist, l_max):
    """The float64 per-gaussian forward of the visible rows: leaves is a dict xyz band0 sh opacity scale quaternion of
    float32 rows in compacted order (sh may be None at degree 0)."""
    from oracle import oracle as orc
    f8 = np.float64
    W, H = int(cam["width"]), int(cam["height"])
    fx, fy = float(cam["fx"]), float(cam["fy"])
    g = dict(W=W, H=H, fx=fx, fy=fy, l_max=l_max, cam=cam)
    for k in ("xyz", "band0", "scale", "quaternion"):
        g[k] = np.asarray(leaves[k], f8).reshape(len(leaves["xyz"]), -1)
    g["sh"] = None if l_max == 0 or leaves.get("sh") is None else np.asarray(leaves["sh"], f8).reshape(len(g["xyz"]), -1)
    g["xyz_c"] = orc.compute_camera_space_points(g["xyz"], cam["view"], f8)
    g["sigma"] = orc.compute_sigma(g["quaternion"], g["scale"], f8)
    g["J"], g["conic"], _ = orc.compute_conic(g["xyz_c"], cam["view"], g["sigma"], fx, fy, W / (2.0 * fx), H / (2.0 * fy),
                                              mh_dist, f8)
    g["tan_fov"] = tuple(float(t) for t in edge_scenes.backward_tan_fov(cam))
    return g


def chain(geom, G):
    """The per-gaussian chain in float64: G [M, 9 or 10] (COLUMNS) -> dict of the six leaf gradients."""
    from oracle import oracle as orc
    f8 = np.float64
    cam, L = geom["cam"], geom["l_max"]
    G = np.asarray(G, f8)
    M = len(geom["xyz"])
    out = {}
    sh_g, out["band0"], xyz_g = orc.precompute_spherical_harmonics_backward(
        geom["xyz"], geom["band0"], geom["sh"], cam["campos"], G[:, 0:3], L, None, f8)
    out["sh"] = sh_g.reshape(M, sh_g.shape[1] * 3)
    out["opacity"] = G[:, 3:4].copy()
    Jg, Sg = orc.compute_conic_backward(geom["J"], geom["sigma"], cam["view"], geom["conic"], G[:, 4:7], None, None, f8)
    xc = orc.compute_projection_jacobian_backward(geom["xyz_c"], geom["fx"], geom["fy"], geom["tan_fov"][0],
                                                  geom["tan_fov"][1], Jg, None, f8)
    out["quaternion"], out["scale"] = orc.compute_sigma_backward(geom["quaternion"], geom["scale"], Sg, f8)
    xc = orc.project_to_screen_backward(geom["xyz_c"], cam["proj"], G[:, 7:9], geom["W"], geom["H"], xc, f8)
    if G.shape[1] > 9:
        xc = np.array(xc, f8).reshape(-1, 3)
        xc[:, 2] += G[:, 9]
    out["xyz"] = orc.compute_camera_space_points_backward(geom["xyz"], cam["view"], xc, xyz_g, f8)
    return out


def chain_matrix(geom, K):
    """A[k][leaf]: the leaf gradients [M, d] for a unit incoming gradient in column k on every row (K = 9 or 10 calls)."""
    M = len(geom["xyz"])
    A = []
    for k in range(K):
        E = np.zeros((M, K))
        E[:, k] = 1.0
        A.append(chain(geom, E))
    return A


def apply(A, S, absolute=False):
    """A_i . S_i (or |A_i| . S_i) for every row: dict leaf -> [M, d]."""
    out = {}
    for leaf in LEAVES:
        total = 0.0
        for k, Ak in enumerate(A):
            m = np.abs(Ak[leaf]) if absolute else Ak[leaf]
            with np.errstate(invalid="ignore"):
                total = total + m * S[:, k:k + 1]
        out[leaf] = total
    return out


def bound_terms(fwd, leaves, cam, grad_image, bg, l_max, mh_dist, grad_depth=None, grad_alpha=None, z=None,
                checkpoints=None):
    """Everything the bar needs, for the ten arrays it covers.  Returns dict name -> (value64, unit, borderline), each
    [M, d], for the four compositing arrays (precompute_rgb, opacity, conic, uv -- and z in depth mode) and the six
    leaves, plus "on_list" [M] (rows on some tile list) under that key."""
    W, H = int(cam["width"]), int(cam["height"])
    signed, absolute, border, split = compositing_sums(fwd, grad_image, W, H, bg, grad_depth, grad_alpha, z,
                                                       with_split=True, checkpoints=checkpoints)
    plain = absolute
    absolute = absolute + split  # the unit: the condition sum of the shares as the row polynomial forms them
    K = signed.shape[1]
    out = {}
    for name, sl in SLICES.items():
        if sl.start < K:
            out[name] = (signed[:, sl], absolute[:, sl], border[:, sl])
    geom = geometry64(leaves, cam, mh_dist, l_max)
    A = chain_matrix(geom, K)
    v, u, b = apply(A, signed), apply(A, absolute, True), apply(A, border, True)
    if u["sh"].shape[1]:  # the SH basis in float32 is off by u * SH_TERMS whatever its value: see SH_TERMS
        u["sh"] = u["sh"] + SH_TERMS * np.tile(absolute[:, 0:3], u["sh"].shape[1] // 3)
    for leaf in LEAVES:
        out["leaf_" + leaf] = (v[leaf], u[leaf], b[leaf])
    on_list = np.zeros(len(signed), bool)
    on_list[np.asarray(fwd["sorted"])] = True
    out["on_list"], out["A"], out["absolute"] = on_list, A, plain
    return out

"""Reference for anti-aliased mode (gsplat_context_set_antialiased), numpy on top of the unchanged CPU oracle.

The mode composites gaussian j with the effective opacity o = sigmoid(logit) * rho, rho = sqrt(max(0, det0 / det1)),
det0 = a c - b^2, det1 = (a + 0.3f)(c + 0.3f) - b^2, (a, b, c) the entries of M Sigma M^T (M = J W) before the 0.3 blur.

forward:   rho in float64, the logit of o substituted for the opacity, the oracle's render_image as it is;
backward:  the oracle's backward_pass on the substituted logits gives g_eff = dL/d logit(o) as its opacity gradient; the
           chain rule of the definition (include/gsplat_hip.h) in float64 turns it into dL/d logit and dL/d rho, and
           dL/d rho through rho(det0, det1), cov = M Sigma M^T (Sigma as the six-vector) and M = J W into increments of
           dL/dJ and dL/dSigma; the oracle's (linear) Jacobian, view-transform and Sigma backward operators in float64
           carry those to the leaves.

rho is evaluated from the oracle's float32 J and Sigma -- the inputs of its conic step -- not from the float32 conic it
stores: the conic is the inverse of the BLURRED covariance, and recovering a = a' - 0.3 from it loses every digit a
sub-pixel splat has (a' ~ 0.3 carries an absolute error of 3e-8, a is 1e-3 .. 1e-2 there), which is exactly the
population the mode exists for.  compensation_from_conic is that evaluation, kept to say how far it is off
(tests/test_antialias_cpu.py)."""
import numpy as np

BLUR = float(np.float32(0.3))  # the kernels' 0.3f


def _sym(sigma):
    s = np.asarray(sigma, np.float64).reshape(-1, 6)
    S = np.empty((len(s), 3, 3))
    S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = s[:, 0], s[:, 3], s[:, 5]
    S[:, 0, 1] = S[:, 1, 0] = s[:, 1]
    S[:, 0, 2] = S[:, 2, 0] = s[:, 2]
    S[:, 1, 2] = S[:, 2, 1] = s[:, 4]
    return S


def covariance(J, sigma, view, dtype=np.float64):
    """(M [n,2,3], Sigma [n,3,3], a, b, c) in float64: cov = M Sigma M^T before the blur.  dtype=float32: the same
    products rounded to float32 (not in the kernels' order): what the number format alone does to the result."""
    Jm = np.asarray(J, dtype).reshape(-1, 2, 3)
    W = np.asarray(view, dtype).reshape(4, 4)[:3, :3]
    S = _sym(sigma).astype(dtype)
    M = Jm @ W
    cov = M @ S @ M.transpose(0, 2, 1)
    return M, S, cov[:, 0, 0], 0.5 * (cov[:, 0, 1] + cov[:, 1, 0]), cov[:, 1, 1]


def rho_of(a, b, c):
    blur = a.dtype.type(BLUR)
    det0 = a * c - b * b
    det1 = (a + blur) * (c + blur) - b * b
    with np.errstate(all="ignore"):
        ratio = det0 / det1
    return np.sqrt(np.where(ratio > 0, ratio, ratio.dtype.type(0))), det0, det1  # fmaxf(0, .): NaN and negative -> 0


def compensation(J, sigma, view, dtype=np.float64):
    """rho [n] in float64 (or rounded to `dtype` throughout) from float32 J, Sigma and the view matrix."""
    _, _, a, b, c = covariance(J, sigma, view, dtype)
    return rho_of(a, b, c)[0]


def compensation_from_conic(conic):
    """rho from the stored conic = inverse(cov + 0.3 I): ill-conditioned for sub-pixel splats (module docstring)."""
    q = np.asarray(conic, np.float64).reshape(-1, 3)
    det = q[:, 0] * q[:, 2] - q[:, 1] ** 2
    a1, b, c1 = q[:, 2] / det, -q[:, 1] / det, q[:, 0] / det
    return rho_of(a1 - BLUR, b, c1 - BLUR)[0]


def compensation_bound(J, sigma, view):
    """What a float32 evaluation of rho by the definition's sums may differ from the float64 one by, per gaussian.

    a, b, c are sums of 27 products of three float32 factors formed in three stages (M = J W, V = Sigma M^T, m . v): every
    product and partial sum carries at most ~8 roundings, so each entry is off by at most 8 eps times the sum of the
    ABSOLUTE products, A = |M| |Sigma| |M|^T.  det0 = a c - b^2 then carries |c| da + |a| dc + 2 |b| db plus two roundings
    of its own products; det1 the same with a', c' (whose addition of 0.3f adds one rounding).  The bound is the largest
    move of sqrt(det0 / det1) over that box, plus 3 eps rho for the division, the square root and the clamp."""
    eps = float(np.finfo(np.float32).eps)
    M, S, a, b, c = covariance(J, sigma, view)
    A = np.abs(M) @ np.abs(S) @ np.abs(M).transpose(0, 2, 1)
    da, db, dc = 8 * eps * A[:, 0, 0], 8 * eps * A[:, 0, 1], 8 * eps * A[:, 1, 1]
    a1, c1 = a + BLUR, c + BLUR
    d0 = np.abs(c) * da + np.abs(a) * dc + 2 * np.abs(b) * db + 2 * eps * (np.abs(a * c) + b * b)
    d1 = np.abs(c1) * (da + eps * a1) + np.abs(a1) * (dc + eps * c1) + 2 * np.abs(b) * db + 2 * eps * (np.abs(a1 * c1) + b * b)
    rho, det0, det1 = rho_of(a, b, c)
    with np.errstate(all="ignore"):
        hi = np.sqrt(np.maximum(0.0, (det0 + d0) / np.maximum(det1 - d1, 1e-300)))
        lo = np.sqrt(np.maximum(0.0, (det0 - d0) / (det1 + d1)))
    return np.maximum(hi - rho, rho - lo) + 3 * eps * rho


def sigmoid(logit):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(logit, np.float64)))


def effective_logit(logit, rho):
    """logit(sigmoid(logit) * rho) as float32: -inf where o == 0, +inf where o == 1."""
    o = sigmoid(logit) * rho
    with np.errstate(divide="ignore"):
        return (np.log(o) - np.log1p(-o)).astype(np.float32)


def split_effective(g_eff, logit, rho, sigma_dtype=np.float64, with_k=False):
    """g_eff = dL/d logit(o) -> (dL/d logit, dL/d rho): k = g_eff / (1 - o), 0 where 1 - o == 0; k (1 - sigma); k / rho,
    0 where rho == 0.  sigma_dtype=float32: sigma rounded as the kernels hold it -- where it rounds to 1 (logits above
    ~17) the definition's 1 - sigma is an exact 0, the float32 oracle's sigma == 1 guard."""
    g_eff, rho = np.asarray(g_eff, np.float64), np.asarray(rho, np.float64)
    sig = sigmoid(logit).astype(sigma_dtype).astype(np.float64)
    om = 1.0 - sig * rho
    with np.errstate(all="ignore"):
        k = np.where(om == 0, 0.0, g_eff / om)
        out = k * (1.0 - sig), np.where(rho == 0, 0.0, k / rho)
    return out + (k,) if with_k else out


def compensation_backward(J, sigma, view, drho):
    """dL/d rho [n] -> (dL/dJ [n,6], dL/dSigma [n,6]) by the definition's chain, in float64.  Sigma's off-diagonal
    entries receive the sum of both symmetric positions (compute_conic_backward's convention)."""
    M, S, a, b, c = covariance(J, sigma, view)
    W = np.asarray(view, np.float64).reshape(4, 4)[:3, :3]
    rho, det0, det1 = rho_of(a, b, c)
    a1, c1 = a + BLUR, c + BLUR
    drho = np.asarray(drho, np.float64)
    with np.errstate(all="ignore"):
        r0 = 1.0 / (2.0 * rho * det1)   # d rho / d det0
        r1 = -rho / (2.0 * det1)        # d rho / d det1
        ga = drho * (r0 * c + r1 * c1)
        gb = drho * (-2.0 * b) * (r0 + r1)
        gc = drho * (r0 * a + r1 * a1)
    dead = ~(rho > 0)  # no gradient through the clamp
    ga, gb, gc = (np.where(dead, 0.0, g) for g in (ga, gb, gc))
    G = np.empty((len(a), 2, 2))
    G[:, 0, 0], G[:, 1, 1] = ga, gc
    G[:, 0, 1] = G[:, 1, 0] = 0.5 * gb
    dM = 2.0 * G @ M @ S
    dJ = dM @ W.T
    dSf = M.transpose(0, 2, 1) @ G @ M
    dS = np.stack([dSf[:, 0, 0], dSf[:, 0, 1] + dSf[:, 1, 0], dSf[:, 0, 2] + dSf[:, 2, 0], dSf[:, 1, 1],
                   dSf[:, 1, 2] + dSf[:, 2, 1], dSf[:, 2, 2]], 1)
    return dJ.reshape(-1, 6), dS


def forward(orc, params, cam, config, bg, l_max, threads=1):
    """(plain, aa): the oracle's float32 forward, and the same with the effective logits composited.  aa carries `logit`
    (the leaf) and `rho` next to the oracle's keys; its `opacity` is the substituted logit."""
    W, H = int(cam["width"]), int(cam["height"])
    plain = orc.rasterize(params, cam, config["near_thresh"], config["mh_dist"], config["cull_mask_padding"], bg, l_max,
                          threads=threads)
    aa = dict(plain)
    aa["logit"] = np.asarray(plain["opacity"], np.float32)
    aa["rho"] = compensation(plain["J"], plain["sigma"], cam["view"])
    aa["opacity"] = effective_logit(aa["logit"], aa["rho"])
    aa["n"], aa["T"], aa["image"] = orc.render_image(plain["uv"], aa["opacity"], plain["conic"], plain["rgb"], bg,
                                                    plain["sorted"], plain["ranges"], W, H, np.float32, threads)
    return plain, aa


def _backward_tan_fov(cam):
    rt = np.float32
    W, H, fx, fy = int(cam["width"]), int(cam["height"]), rt(cam["fx"]), rt(cam["fy"])
    return (float(np.tan(rt(2.0) * np.arctan(rt(W) / (rt(2.0) * fx)) * rt(0.5))),
            float(np.tan(rt(2.0) * np.arctan(rt(H) / (rt(2.0) * fy)) * rt(0.5))))


def backward(orc, aa, cam, grad_image, bg, l_max, threads=1, tan_fov=None, base=None, sigma_dtype=np.float64):
    """Gradients of the anti-aliased image in compacted order (float64), keys as oracle.backward_pass plus `rho` and `k`.
    base: a function aa -> gradients to use instead of oracle.backward_pass (depth mode: depth_reference.backward_pass);
    sigma_dtype: see split_effective."""
    if base is None:
        g = orc.backward_pass(aa, cam, grad_image, bg, l_max, threads=threads, tan_fov=tan_fov)
    else:
        g = base(aa)
    g = {k: (np.array(v, np.float64) if v is not None else None) for k, v in g.items()}
    d_logit, d_rho, g["k"] = split_effective(g["opacity"].reshape(-1), aa["logit"], aa["rho"], sigma_dtype, with_k=True)
    dJ, dS = compensation_backward(aa["J"], aa["sigma"], cam["view"], d_rho)
    g["opacity"], g["rho"] = d_logit, d_rho
    g["J"] = g["J"].reshape(-1, 6) + dJ
    g["sigma"] = g["sigma"].reshape(-1, 6) + dS
    tfx, tfy = tan_fov if tan_fov is not None else _backward_tan_fov(cam)
    xc = orc.compute_projection_jacobian_backward(aa["xyz_c"], cam["fx"], cam["fy"], tfx, tfy, dJ, None, np.float64)
    g["xyz_c"] = g["xyz_c"].reshape(-1, 3) + xc
    g["xyz"] = g["xyz"].reshape(-1, 3) + orc.compute_camera_space_points_backward(aa["xyz"], cam["view"], xc, None, np.float64)
    dq, ds = orc.compute_sigma_backward(aa["quaternion"], aa["scale"], dS, np.float64)
    g["quaternion"] = g["quaternion"].reshape(-1, 4) + dq
    g["scale"] = g["scale"].reshape(-1, 3) + ds
    return g

"""Numpy float64 reference of the normal map and its two losses (gsplat_depth_to_normal, gsplat_depth_to_normal_backward,
gsplat_normal_prior_loss, gsplat_normal_smoothness_loss; definitions: include/gsplat_hip.h) and of ops.pixel_intrinsics.

    A = 1 - T,  ok = A >= alpha_min and depth > 0 and both finite,  z = depth / A  (inverse: A / depth)
    P(x, y) = z ((x - cx) / fx, (y - cy) / fy, 1)            x, y: integer pixel coordinates
    tx = P(x+1, y) - P(x-1, y),  ty = P(x, y+1) - P(x, y-1),  c = ty x tx,  n = c / |c|
    valid: ok at the pixel and its four neighbours and |c| > 0; everything else, the border included, is (0, 0, 0)

Every scalar argument goes through float32 first, as the C ABI takes it; the maps are taken as they are given.  Every
gradient comes with `absolute`, the sum of the absolute values of the terms it is made of (carried through the
normalisation, the cross product and the dot product with the pixel's ray): the bar of the tests is a fraction of it."""
import numpy as np


def _f32(v):
    return float(np.float32(v))


def pixel_intrinsics(cam):
    """(fx, fy, cx, cy) in float64 from the camera dict's projection: project_to_screen(P(x, y)) = (x, y)."""
    proj = np.asarray(cam["proj"], np.float64).reshape(-1)
    W, H = float(cam["width"]), float(cam["height"])
    return proj[0] * W / 2.0, proj[5] * H / 2.0, (proj[2] + 1.0) * W / 2.0, (proj[6] + 1.0) * H / 2.0


def expected_depth(depth, T, inverse, alpha_min=0.5):
    """(z [H,W] with 0 where not ok, ok, depth, A) in float64."""
    d, A = np.asarray(depth, np.float64), 1.0 - np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        ok = (A >= _f32(alpha_min)) & (d > 0) & np.isfinite(A) & np.isfinite(d)
        z = np.where(ok, (A / d) if inverse else (d / A), 0.0)
    return z, ok, d, A


def rays(H, W, intrinsics):
    fx, fy, cx, cy = (_f32(v) for v in intrinsics)
    return (np.arange(W, dtype=np.float64) - cx) / fx, (np.arange(H, dtype=np.float64) - cy) / fy


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _cross_abs(a_abs, b_abs):
    """The sum of the absolute values of the two products of every component of a x b."""
    return np.stack([a_abs[..., 1] * b_abs[..., 2] + a_abs[..., 2] * b_abs[..., 1],
                     a_abs[..., 2] * b_abs[..., 0] + a_abs[..., 0] * b_abs[..., 2],
                     a_abs[..., 0] * b_abs[..., 1] + a_abs[..., 1] * b_abs[..., 0]], -1)


def tangents(depth, T, intrinsics, inverse, alpha_min=0.5):
    """dict(tx, ty, c [H,W,3], length [H,W], valid [H,W], z, ok, d, A, rx, ry): zeros outside `valid`."""
    z, ok, d, A = expected_depth(depth, T, inverse, alpha_min)
    H, W = z.shape
    rx, ry = rays(H, W, intrinsics)
    tx, ty, c = (np.zeros((H, W, 3)) for _ in range(3))
    length, valid = np.zeros((H, W)), np.zeros((H, W), bool)
    if H >= 3 and W >= 3:
        zl, zr, zu, zd = z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
        rxl, rxc, rxr = rx[None, :-2], rx[None, 1:-1], rx[None, 2:]
        ryu, ryc, ryd = ry[:-2, None], ry[1:-1, None], ry[2:, None]
        five = ok[1:-1, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:] & ok[:-2, 1:-1] & ok[2:, 1:-1]
        txi = np.stack([zr * rxr - zl * rxl, zr * ryc - zl * ryc, zr - zl], -1)
        tyi = np.stack([zd * rxc - zu * rxc, zd * ryd - zu * ryu, zd - zu], -1)
        ci = _cross(tyi, txi)
        li = np.sqrt((ci * ci).sum(-1))
        vi = five & (li > 0) & np.isfinite(li)
        tx[1:-1, 1:-1], ty[1:-1, 1:-1], c[1:-1, 1:-1] = (np.where(vi[..., None], a, 0.0) for a in (txi, tyi, ci))
        length[1:-1, 1:-1], valid[1:-1, 1:-1] = np.where(vi, li, 0.0), vi
    return dict(tx=tx, ty=ty, c=c, length=length, valid=valid, z=z, ok=ok, d=d, A=A, rx=rx, ry=ry)


def depth_to_normal(depth, T, intrinsics, inverse, alpha_min=0.5):
    """n [H,W,3] float64."""
    t = tangents(depth, T, intrinsics, inverse, alpha_min)
    with np.errstate(all="ignore"):
        return np.where(t["valid"][..., None], t["c"] / t["length"][..., None], 0.0)


def depth_to_normal_backward(depth, T, intrinsics, inverse, grad_normal, alpha_min=0.5):
    """(dL/d depth, dL/d(1 - T), absolute of the first, absolute of the second), [H,W] float64 each."""
    t = tangents(depth, T, intrinsics, inverse, alpha_min)
    G = np.asarray(grad_normal, np.float64)
    valid, L = t["valid"][..., None], t["length"][..., None]
    with np.errstate(all="ignore"):
        n = np.where(valid, t["c"] / L, 0.0)
        nG = (n * G).sum(-1, keepdims=True)
        gc = np.where(valid, (G - n * nG) / L, 0.0)                                        # dL/dc
        gc_abs = np.where(valid, (np.abs(G) + np.abs(n) * np.abs(n * G).sum(-1, keepdims=True)) / L, 0.0)
    d_tx, d_ty = _cross(gc, t["ty"]), _cross(t["tx"], gc)                                  # dL/dtx, dL/dty
    a_tx, a_ty = _cross_abs(gc_abs, np.abs(t["ty"])), _cross_abs(np.abs(t["tx"]), gc_abs)
    # a pixel is the right end of its left neighbour's tx, the left end of its right neighbour's, the lower end of its
    # upper neighbour's ty and the upper end of its lower neighbour's
    dP, aP = np.zeros_like(d_tx), np.zeros_like(d_tx)
    dP[:, 1:] += d_tx[:, :-1]; dP[:, :-1] -= d_tx[:, 1:]; dP[1:] += d_ty[:-1]; dP[:-1] -= d_ty[1:]
    aP[:, 1:] += a_tx[:, :-1]; aP[:, :-1] += a_tx[:, 1:]; aP[1:] += a_ty[:-1]; aP[:-1] += a_ty[1:]
    H, W = t["z"].shape
    r = np.stack([np.broadcast_to(t["rx"][None, :], (H, W)), np.broadcast_to(t["ry"][:, None], (H, W)), np.ones((H, W))], -1)
    dz, az = (dP * r).sum(-1), (aP * np.abs(r)).sum(-1)
    z, ok, d, A = t["z"], t["ok"], t["d"], t["A"]
    with np.errstate(all="ignore"):
        if inverse:   # z = A / depth
            dz_dd, dz_dA = np.where(ok, -z / d, 0.0), np.where(ok, 1.0 / d, 0.0)
        else:         # z = depth / A
            dz_dd, dz_dA = np.where(ok, 1.0 / A, 0.0), np.where(ok, -z / A, 0.0)
    return dz * dz_dd, dz * dz_dA, az * np.abs(dz_dd), az * np.abs(dz_dA)


def has_normal(normal):
    return (np.asarray(normal) != 0).any(-1)


def normal_prior_loss(normal, prior, weight):
    """(loss, dL/dn [H,W,3], absolute): weight / P x sum of 1 - n . prior / |prior| over has_normal & prior != 0."""
    n, p = np.asarray(normal, np.float64), np.asarray(prior, np.float64)
    scale = _f32(weight) / (n.shape[0] * n.shape[1])
    length = np.sqrt((p * p).sum(-1))
    valid = has_normal(n) & (length > 0) & np.isfinite(length)
    with np.errstate(all="ignore"):
        u = np.where(valid[..., None], p / length[..., None], 0.0)
    loss = scale * np.where(valid, 1.0 - (n * u).sum(-1), 0.0).sum()
    grad = -scale * u
    return loss, grad, np.abs(grad)


def normal_smoothness_loss(normal, image, weight, edge_scale=1.0):
    """(loss, dL/dn [H,W,3], absolute): weight / P x sum over adjacent pairs with a normal of w sum_c |n_a,c - n_b,c|,
    w = exp(-edge_scale x mean_c |I_a,c - I_b,c|), or 1 without an image; sign(0) = 0."""
    n = np.asarray(normal, np.float64)
    H, W = n.shape[:2]
    scale, es = _f32(weight) / (H * W), _f32(edge_scale)
    I = None if image is None else np.asarray(image, np.float64)
    has = has_normal(n)
    grad, absolute, total = np.zeros_like(n), np.zeros_like(n), 0.0
    for a, b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))),    # (x, y) with (x + 1, y)
                 ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):   # (x, y) with (x, y + 1)
        both = (has[a] & has[b])[..., None]
        w = np.ones(both.shape) if I is None else np.exp(-es * (np.abs(I[a] - I[b]).sum(-1, keepdims=True) / 3.0))
        w = np.where(both, w, 0.0)
        d = n[a] - n[b]
        total += (w * np.abs(d)).sum()
        grad[a] += w * np.sign(d)
        grad[b] -= w * np.sign(d)
        absolute[a] += w * np.abs(np.sign(d))
        absolute[b] += w * np.abs(np.sign(d))
    return scale * total, scale * grad, scale * absolute

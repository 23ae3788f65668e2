"""Reference for depth mode's options (gsplat_context_set_depth_mode), composed from the CPU oracle's operators exactly as
tests/depth_reference.py is.

With s = z (or s = 1/z, `inverse`) of every compacted gaussian, the maps D = sum w s, A = sum w and Q = sum w s^2 (w = alpha T)
are the three channels of the image render_image gives for the colour (s, 1, s^2) over background 0.  Their gradient is
render_image_backward on that colour with the pixel gradient (G_D, G_A, G_Q), added to the image's own compositing
gradient; dL/ds = that call's grad_rgb[:, 0] + 2 s grad_rgb[:, 2], and dL/dz = dL/ds x (inverse ? -s^2 : 1) is added to
dL/d xyz_c[:, 2] ahead of the view-transform backward.

Also the two regularisers on those maps in numpy float64 (gsplat_distortion_loss, gsplat_depth_prior_loss)."""
import numpy as np


def s_values(ref, inverse, dtype=np.float32):
    z = np.asarray(ref["xyz_c"], dtype)[:, 2]
    return (np.dtype(dtype).type(1.0) / z) if inverse else z


def aux_colour(ref, inverse, dtype=np.float32):
    s = s_values(ref, inverse, dtype)
    return np.stack([s, np.ones_like(s), s * s], 1)


def maps(orc, ref, W, H, inverse, dtype=np.float32, threads=1):
    """(D [H,W], A [H,W], Q [H,W]) of the oracle's forward `ref`."""
    _, _, img = orc.render_image(ref["uv"], ref["opacity"], ref["conic"], aux_colour(ref, inverse, dtype), 0.0,
                                 ref["sorted"], ref["ranges"], W, H, dtype, threads)
    return img[..., 0], img[..., 1], img[..., 2]


def backward_pass(orc, ref, camera, grad_image, grad_depth, grad_alpha, grad_depth2, bg, l_max, inverse,
                  dtype=np.float32, threads=1):
    """oracle.backward_pass with dL/dD, dL/dA and dL/dQ (any may be None) next to dL/d image."""
    W, H = int(camera["width"]), int(camera["height"])
    zero = np.zeros((H, W), dtype)
    gd, ga, gq = (zero if m is None else np.asarray(m, dtype) for m in (grad_depth, grad_alpha, grad_depth2))
    g = {}
    g["rgb_pre"], g["opacity"], g["uv"], g["conic"] = orc.render_image_backward(
        ref["uv"], ref["opacity"], ref["conic"], ref["rgb"], bg, ref["sorted"], ref["ranges"], ref["n"], ref["T"],
        grad_image, W, H, dtype, threads)
    aux_rgb, aux_op, aux_uv, aux_conic = orc.render_image_backward(
        ref["uv"], ref["opacity"], ref["conic"], aux_colour(ref, inverse, dtype), 0.0, ref["sorted"], ref["ranges"],
        ref["n"], ref["T"], np.stack([gd, ga, gq], -1), W, H, dtype, threads)
    g["opacity"] = g["opacity"] + aux_op
    g["uv"] = g["uv"] + aux_uv
    g["conic"] = g["conic"] + aux_conic
    s = s_values(ref, inverse, dtype)
    two = np.dtype(dtype).type(2.0)
    g["s"] = aux_rgb[:, 0] + two * s * aux_rgb[:, 2]
    g["z"] = g["s"] * (-(s * s)) if inverse else g["s"]
    g["sh"], g["band0"], g["xyz"] = orc.precompute_spherical_harmonics_backward(
        ref["xyz"], ref["band0"], ref["sh"], camera["campos"], g["rgb_pre"], l_max, None, dtype)
    g["J"], g["sigma"] = orc.compute_conic_backward(ref["J"], ref["sigma"], camera["view"], ref["conic"], g["conic"],
                                                    None, None, dtype)
    rt = np.dtype(dtype).type
    fx, fy = rt(camera["fx"]), rt(camera["fy"])
    tan_fovx = np.tan(rt(2.0) * np.arctan(rt(W) / (rt(2.0) * fx)) * rt(0.5))
    tan_fovy = np.tan(rt(2.0) * np.arctan(rt(H) / (rt(2.0) * fy)) * rt(0.5))
    g["xyz_c"] = orc.compute_projection_jacobian_backward(ref["xyz_c"], fx, fy, tan_fovx, tan_fovy, g["J"], None, dtype)
    g["quaternion"], g["scale"] = orc.compute_sigma_backward(ref["quaternion"], ref["scale"], g["sigma"], dtype)
    g["xyz_c"] = orc.project_to_screen_backward(ref["xyz_c"], camera["proj"], g["uv"], W, H, g["xyz_c"], dtype)
    g["xyz_c"] = np.array(g["xyz_c"], dtype).reshape(-1, 3)
    g["xyz_c"][:, 2] += g["z"]
    g["xyz"] = orc.compute_camera_space_points_backward(ref["xyz"], camera["view"], g["xyz_c"], g["xyz"], dtype)
    return g


def distortion_loss(T, D, Q, weight):
    """(loss, dL/dA, dL/dD, dL/dQ) in float64: loss = weight x mean(A Q - D^2), A = 1 - T."""
    T, D, Q = (np.asarray(m, np.float64) for m in (T, D, Q))
    A = 1.0 - T
    scale = float(weight) / T.size
    return scale * (A * Q - D * D).sum(), scale * Q, scale * (-2.0 * D), scale * A


def depth_prior_loss(depth, target, weight):
    """(loss, dL/d depth) in float64: weight x mean over ALL pixels of |depth - target| on the pixels with target > 0."""
    depth, target = np.asarray(depth, np.float64), np.asarray(target, np.float64)
    diff = np.where(target > 0, depth - target, 0.0)
    scale = float(weight) / depth.size
    return scale * np.abs(diff).sum(), scale * np.sign(diff)

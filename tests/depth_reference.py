"""Reference for the depth / opacity maps (gsplat_context_set_depth) composed from the CPU oracle's operators.

depth and alpha are channels 0 and 1 of the image render_image gives for the per-gaussian colour (z, 1, 0) over background
0 (z = xyz_c[:, 2]); their gradient is render_image_backward on that colour with the pixel gradient (G_D, G_A, 0), added
to the image's own compositing gradient, and dL/dz = that call's grad_rgb[:, 0] added to dL/d xyz_c[:, 2] ahead of the
view-transform backward.

At float32 the composited depth is itself up to a few 1e-5 (relative) from its float64 evaluation on a few pixels in
four million (2048x2048 and 2064x2048, 20 000 gaussians: four pixels each): a depth bar of 1e-5 relative on images of
that size wants dtype=np.float64 here (tests/test_tile_grid_gpu.py), as the small scenes of tests/test_depth_gpu.py
do not."""
import numpy as np


def aux_colour(ref, dtype=np.float32):
    z = np.asarray(ref["xyz_c"], dtype)[:, 2]
    return np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)


def depth_alpha(orc, ref, W, H, dtype=np.float32, threads=1):
    """(depth [H,W], alpha [H,W]) of the oracle's forward `ref`."""
    _, _, img = orc.render_image(ref["uv"], ref["opacity"], ref["conic"], aux_colour(ref, dtype), 0.0, ref["sorted"],
                                 ref["ranges"], W, H, dtype, threads)
    return img[..., 0], img[..., 1]


def backward_pass(orc, ref, camera, grad_image, grad_depth, grad_alpha, bg, l_max, dtype=np.float32, threads=1):
    """oracle.backward_pass with dL/d depth and dL/d alpha (either may be None) next to dL/d image."""
    W, H = int(camera["width"]), int(camera["height"])
    gd = np.zeros((H, W), dtype) if grad_depth is None else np.asarray(grad_depth, dtype)
    ga = np.zeros((H, W), dtype) if grad_alpha is None else np.asarray(grad_alpha, dtype)
    g = {}
    g["rgb_pre"], g["opacity"], g["uv"], g["conic"] = orc.render_image_backward(
        ref["uv"], ref["opacity"], ref["conic"], ref["rgb"], bg, ref["sorted"], ref["ranges"], ref["n"], ref["T"],
        grad_image, W, H, dtype, threads)
    aux_rgb, aux_op, aux_uv, aux_conic = orc.render_image_backward(
        ref["uv"], ref["opacity"], ref["conic"], aux_colour(ref, dtype), 0.0, ref["sorted"], ref["ranges"], ref["n"],
        ref["T"], np.stack([gd, ga, np.zeros_like(gd)], -1), W, H, dtype, threads)
    g["opacity"] = g["opacity"] + aux_op
    g["uv"] = g["uv"] + aux_uv
    g["conic"] = g["conic"] + aux_conic
    g["z"] = aux_rgb[:, 0]
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

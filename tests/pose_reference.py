"""Reference for the camera gradient (gsplat_backward_gaussians_camera / gsplat_backward_pass_camera) composed from the
CPU oracle's operators, as tests/depth_reference.py composes the depth terms.

view = [R|t] (its first twelve entries) and campos are two independent inputs.  Per visible gaussian j with world
position p_j:
  c_j  = dL/d xyz_c, the chain's final camera-space gradient (Jacobian path, screen projection, depth term),
  dM_j = dL/dM for M = J R: compute_conic_backward returns J_grad = dM R^T, so dM = J_grad (R^T)^-1,
  s_j  = the position gradient through the SH view direction (precompute_spherical_harmonics_backward),
and
  grad_view[4r + c] = sum_j c_j[r] p_j[c] + sum_j (J_j^T dM_j)[r][c]   (r, c < 3)
  grad_view[4r + 3] = sum_j c_j[r]
  grad_campos       = -sum_j s_j
in float64, with the per-component L1 mass m_k = sum_j |term_jk| the GPU tests scale their bars by."""
import numpy as np

import depth_reference


def terms(xyz, J, xyz_c_grad, dM, s):
    """Per-gaussian contributions [M, 15] in float64 (columns: grad_view[0..11], grad_campos[0..2])."""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    c = np.asarray(xyz_c_grad, np.float64).reshape(-1, 3)
    Jm = np.asarray(J, np.float64).reshape(-1, 2, 3)
    dMm = np.asarray(dM, np.float64).reshape(-1, 2, 3)
    jt_dm = np.einsum("jkr,jkc->jrc", Jm, dMm)
    view = np.concatenate([c[:, :, None] * p[:, None, :] + jt_dm, c[:, :, None]], 2).reshape(-1, 12)
    return np.concatenate([view, -np.asarray(s, np.float64).reshape(-1, 3)], 1)


def dM_from_J_grad(J_grad, view):
    R = np.asarray(view, np.float64).reshape(4, 4)[:3, :3]
    return np.asarray(J_grad, np.float64).reshape(-1, 2, 3) @ np.linalg.inv(R.T)


def from_chain(orc, ref, camera, g, l_max, dtype=np.float32):
    """terms() of an oracle backward `g` (oracle.backward_pass / depth_reference.backward_pass / chain) of forward `ref`."""
    _, _, s = orc.precompute_spherical_harmonics_backward(ref["xyz"], ref["band0"], ref["sh"], camera["campos"],
                                                          g["rgb_pre"], l_max, None, dtype)
    return terms(ref["xyz"], ref["J"], g["xyz_c"], dM_from_J_grad(g["J"], camera["view"]), s)


def chain(orc, ref, camera, g_rgb, g_conic, g_uv, g_z, dtype=np.float32):
    """The per-gaussian chain from given compositing gradients (what oracle.backward_pass does after
    render_image_backward): {rgb_pre, J, xyz_c}."""
    W, H = int(camera["width"]), int(camera["height"])
    rt = np.dtype(dtype).type
    fx, fy = rt(camera["fx"]), rt(camera["fy"])
    tan_fovx = np.tan(rt(2.0) * np.arctan(rt(W) / (rt(2.0) * fx)) * rt(0.5))
    tan_fovy = np.tan(rt(2.0) * np.arctan(rt(H) / (rt(2.0) * fy)) * rt(0.5))
    J_grad, _ = orc.compute_conic_backward(ref["J"], ref["sigma"], camera["view"], ref["conic"], g_conic, None, None, dtype)
    c = orc.compute_projection_jacobian_backward(ref["xyz_c"], fx, fy, tan_fovx, tan_fovy, J_grad, None, dtype)
    c = np.array(orc.project_to_screen_backward(ref["xyz_c"], camera["proj"], g_uv, W, H, c, dtype), dtype).reshape(-1, 3)
    if g_z is not None:
        c[:, 2] += g_z
    return dict(rgb_pre=g_rgb, J=J_grad, xyz_c=c)


def camera_gradient(orc, ref, camera, grad_image, grad_depth, grad_alpha, bg, l_max, dtype=np.float32, threads=1):
    """(grad [15], mass [15]) for L with dL/d image, dL/d depth, dL/d alpha (the last two may be None)."""
    g = depth_reference.backward_pass(orc, ref, camera, grad_image, grad_depth, grad_alpha, bg, l_max, dtype, threads)
    t = from_chain(orc, ref, camera, g, l_max, dtype)
    return t.sum(0), np.abs(t).sum(0)

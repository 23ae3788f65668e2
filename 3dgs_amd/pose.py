"""Camera pose from the rasterizer's camera gradient (RasterContext.backward_pass_camera / backward_gaussians_camera).

The library differentiates with respect to view[0..11] = [R|t] and campos as two independent inputs, as the forward
reads them.  A camera whose campos is the centre of its view, campos = -R^T t (scene.make_camera, the COLMAP reader),
has one pose; these helpers turn the fifteen numbers into the gradient of that pose and apply a step to it.  Host code on
fifteen numbers, in float64: no kernel.
"""
import math

import numpy as np
import torch


def _f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", torch.float64).numpy()
    return np.asarray(x, np.float64)


def _rt(cam):
    v = _f64(cam["view"]).reshape(4, 4)
    return v[:3, :3], v[:3, 3]


def pose_gradient(cam, grad_view, grad_campos):
    """(dL/dR [3,3], dL/dt [3]) of the whole camera, campos = -R^T t following the view:
    dL/dR = G_view[:, :3] - t g_cp^T, dL/dt = G_view[:, 3] - R g_cp."""
    R, t = _rt(cam)
    gv, gc = _f64(grad_view).reshape(3, 4), _f64(grad_campos).reshape(3)
    return gv[:, :3] - np.outer(t, gc), gv[:, 3] - R @ gc


def pose_tangent_gradient(cam, grad_view, grad_campos):
    """dL/d xi [6] = (rho, phi) for the left perturbation view' = exp(xi^) view (apply_pose_update).  With
    A = G_R R^T + G_t t^T: dL/d rho = G_t, dL/d phi = (A_32 - A_23, A_13 - A_31, A_21 - A_12)."""
    R, t = _rt(cam)
    gR, gt = pose_gradient(cam, grad_view, grad_campos)
    A = gR @ R.T + np.outer(gt, t)
    return np.concatenate([gt, [A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]]])


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """exp(xi^) as a 4x4 float64 matrix, xi = (rho, phi): rotation exp(phi^), translation V(phi) rho."""
    xi = np.asarray(xi, np.float64).reshape(6)
    rho, phi = xi[:3], xi[3:]
    th = math.sqrt(float(phi @ phi))
    K = _hat(phi)
    if th < 1e-6:  # the series, to the order that float64 resolves there
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / th ** 2, (th - math.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    T[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ rho
    return T


def updated_view(view, xi):
    """exp(xi^) view, float64 [16] (view: 16 numbers, row-major)."""
    return (se3_exp(xi) @ _f64(view).reshape(4, 4)).reshape(16)


def apply_pose_update(cam, xi):
    """A copy of the camera dict with view = exp(xi^) view in float32 (a device tensor stays on its device) and campos =
    -R^T t recomputed from that float32 view (a float32 host array; campos_dev follows when present).  proj, fx, fy and
    the image size are kept."""
    v32 = updated_view(cam["view"], xi).astype(np.float32)
    out = dict(cam)
    out["view"] = torch.as_tensor(v32).to(cam["view"].device) if isinstance(cam["view"], torch.Tensor) else v32
    R, t = v32.reshape(4, 4)[:3, :3].astype(np.float64), v32.reshape(4, 4)[:3, 3].astype(np.float64)
    out["campos"] = (-R.T @ t).astype(np.float32)
    if "campos_dev" in cam:
        out["campos_dev"] = torch.as_tensor(out["campos"]).to(cam["campos_dev"].device)
    return out

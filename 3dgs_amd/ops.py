"""Host-side mirror of the reference operator surface on torch device tensors.

Same names, argument order and output semantics ("=" vs "+=") as
/root/reference/include/gsplat_cuda/cuda_forward.cuh:26-131 and cuda_backward.cuh:21-123.
Each function only forwards raw device pointers to the C ABI (include/gsplat_hip.h) on
torch's current HIP stream; torch is used for device memory, nothing else.  Errors come back
as GsplatError (the C++ shim headers in include/gsplat_cuda/ reproduce the reference's
print-and-exit instead).
"""
import ctypes

import torch

from . import _lib
from ._lib import check


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError("expected a torch tensor or None")
    if t.numel() == 0:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _f32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32")
    return t


def compute_camera_space_points(xyz_w, view, N, xyz_c):
    check(_lib.load().gsplat_compute_camera_space_points(_p(_f32(xyz_w, "xyz_w")), _p(view), N, _p(xyz_c), _stream()))


def project_to_screen(xyz, proj, N, width, height, uv):
    check(_lib.load().gsplat_project_to_screen(_p(_f32(xyz, "xyz")), _p(proj), N, width, height, _p(uv), _stream()))


def cull_gaussians(uv, xyz, N, near_thresh, padding, width, height, mask):
    """mask: torch.bool or uint8 tensor [N]; true = keep."""
    check(_lib.load().gsplat_cull_gaussians(_p(uv), _p(xyz), N, near_thresh, padding, width, height, _p(mask), _stream()))


def compute_sigma(quaternion, scale, N, sigma):
    check(_lib.load().gsplat_compute_sigma(_p(quaternion), _p(scale), N, _p(sigma), _stream()))


def compute_conic(xyz, view, sigma, focal_x, focal_y, tan_fovx, tan_fovy, mh_dist, N, J, conic, radius):
    check(_lib.load().gsplat_compute_conic(_p(xyz), _p(view), _p(sigma), focal_x, focal_y, tan_fovx, tan_fovy, mh_dist,
                                           N, _p(J), _p(conic), _p(radius), _stream()))


def compute_conic_antialiased(xyz, view, sigma, focal_x, focal_y, tan_fovx, tan_fovy, mh_dist, N, J, conic, radius,
                              compensation):
    """compute_conic plus compensation[N] = rho, the opacity compensation of anti-aliased mode
    (gsplat_compute_conic_antialiased)."""
    check(_lib.load().gsplat_compute_conic_antialiased(_p(xyz), _p(view), _p(sigma), focal_x, focal_y, tan_fovx, tan_fovy,
                                                       mh_dist, N, _p(J), _p(conic), _p(radius), _p(compensation),
                                                       _stream()))


def get_sorted_gaussian_list(uv, xyz, radius, n_tiles_x, n_tiles_y, N, count, sorted_gaussians, ranges):
    """Two-call protocol.  ``count`` is the in/out size_t of the reference, passed as an int; returns the count
    (call 1: number of candidate pairs; call 2: unchanged)."""
    c = ctypes.c_size_t(int(count))
    check(_lib.load().gsplat_get_sorted_gaussian_list(_p(uv), _p(xyz), _p(radius), n_tiles_x, n_tiles_y, N,
                                                      ctypes.byref(c), _p(sorted_gaussians), _p(ranges), _stream()))
    return int(c.value)


def precompute_spherical_harmonics(xyz, sh_coefficients, sh_coeffs_band_0, campos, l_max, N, rgb):
    check(_lib.load().gsplat_precompute_spherical_harmonics(_p(xyz), _p(sh_coefficients), _p(sh_coeffs_band_0),
                                                            float(campos[0]), float(campos[1]), float(campos[2]),
                                                            l_max, N, _p(rgb), _stream()))


def render_image(uv, opacity, conic, rgb, background_opacity, sorted_splats, splat_range_by_tile, image_width,
                 image_height, splats_per_pixel, weight_per_pixel, image):
    check(_lib.load().gsplat_render_image(_p(uv), _p(opacity), _p(conic), _p(rgb), background_opacity,
                                          _p(sorted_splats), _p(splat_range_by_tile), image_width, image_height,
                                          _p(splats_per_pixel), _p(weight_per_pixel), _p(image), _stream()))


def project_to_screen_backward(xyz_c, proj, uv_grad_out, N, width, height, xyz_c_grad_in):
    check(_lib.load().gsplat_project_to_screen_backward(_p(xyz_c), _p(proj), _p(uv_grad_out), N, width, height,
                                                        _p(xyz_c_grad_in), _stream()))


def compute_camera_space_points_backward(xyz_w, view, xyz_c_grad_out, N, xyz_w_grad_in):
    check(_lib.load().gsplat_compute_camera_space_points_backward(_p(xyz_w), _p(view), _p(xyz_c_grad_out), N,
                                                                  _p(xyz_w_grad_in), _stream()))


def compute_projection_jacobian_backward(xyz_c, focal_x, focal_y, tan_fovx, tan_fovy, J_grad_out, N, xyz_c_grad_in):
    check(_lib.load().gsplat_compute_projection_jacobian_backward(_p(xyz_c), focal_x, focal_y, tan_fovx, tan_fovy,
                                                                  _p(J_grad_out), N, _p(xyz_c_grad_in), _stream()))


def compute_conic_backward(J, sigma, view, conic, conic_grad_out, N, J_grad_in, sigma_grad_in):
    check(_lib.load().gsplat_compute_conic_backward(_p(J), _p(sigma), _p(view), _p(conic), _p(conic_grad_out), N,
                                                    _p(J_grad_in), _p(sigma_grad_in), _stream()))


def compute_conic_antialiased_backward(J, sigma, view, conic, conic_grad_out, compensation_grad_out, N, J_grad_in,
                                       sigma_grad_in):
    """compute_conic_backward plus the covariance term of compensation_grad_out[N] = dL/d rho; J_grad_in +=,
    sigma_grad_in += (gsplat_compute_conic_antialiased_backward)."""
    check(_lib.load().gsplat_compute_conic_antialiased_backward(_p(J), _p(sigma), _p(view), _p(conic), _p(conic_grad_out),
                                                                _p(compensation_grad_out), N, _p(J_grad_in),
                                                                _p(sigma_grad_in), _stream()))


def compute_sigma_backward(quaternion, scale, sigma_grad_out, N, quaternion_grad_in, scale_grad_in):
    check(_lib.load().gsplat_compute_sigma_backward(_p(quaternion), _p(scale), _p(sigma_grad_out), N,
                                                    _p(quaternion_grad_in), _p(scale_grad_in), _stream()))


def precompute_spherical_harmonics_backward(xyz_c, rgb_vals, sh_coeffs, campos, rgb_grad_out, l_max, N, sh_grad_in,
                                            sh_grad_band_0_in, xyz_c_grad_in):
    check(_lib.load().gsplat_precompute_spherical_harmonics_backward(
        _p(xyz_c), _p(rgb_vals), _p(sh_coeffs), float(campos[0]), float(campos[1]), float(campos[2]),
        _p(rgb_grad_out), l_max, N, _p(sh_grad_in), _p(sh_grad_band_0_in), _p(xyz_c_grad_in), _stream()))


def render_image_backward(uvs, opacity, conic, rgb, background_opacity, sorted_splats, splat_range_by_tile,
                          num_splats_per_pixel, final_weight_per_pixel, grad_image, image_width, image_height,
                          grad_rgb, grad_opacity, grad_uv, grad_conic):
    check(_lib.load().gsplat_render_image_backward(
        _p(uvs), _p(opacity), _p(conic), _p(rgb), background_opacity, _p(sorted_splats), _p(splat_range_by_tile),
        _p(num_splats_per_pixel), _p(final_weight_per_pixel), _p(grad_image), image_width, image_height, _p(grad_rgb),
        _p(grad_opacity), _p(grad_uv), _p(grad_conic), _stream()))


def fused_loss(predicted_data, gt_data, rows, cols, ssim_weight, image_grad, blocking=True):
    """fused_loss(...) -> loss (cuda_forward.cuh:146-147).  blocking=False skips the read-back and returns None."""
    out = ctypes.c_float(0.0)
    check(_lib.load().gsplat_fused_loss(_p(predicted_data), _p(gt_data), rows, cols, ssim_weight, _p(image_grad),
                                        ctypes.byref(out) if blocking else None, _stream()))
    return float(out.value) if blocking else None


def _map(t, name, shape=None):
    """An [H,W] float32 device map for the depth regularisers; None stays None."""
    if t is None:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
            or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape))):
        raise ValueError(f"{name} must be a contiguous [H,W] float32 device tensor" + (f" of shape {tuple(shape)}" if shape else ""))
    return t


def distortion_loss(fwd, weight, grad_alpha, grad_depth, grad_depth2, accumulate=False, blocking=False):
    """The distortion loss of a forward that ran with the moment option (RasterContext.set_depth(True, moment=True)):
    weight x mean over the pixels of A Q - D^2, A = 1 - fwd["T"], D = fwd["depth"], Q = fwd["depth2"], which is
    sum_{j<i} w_i w_j (s_i - s_j)^2 of the pixel's splats (gsplat_distortion_loss; evaluated in double).  The three [H,W]
    gradient maps (any may be None) get weight / P x (Q, -2 D, A) -- grad_alpha is dL/d(1 - T), what the backwards take --
    overwritten, or added to with accumulate=True.  blocking=True returns the loss (a read-back), otherwise None."""
    if "depth2" not in fwd:
        raise ValueError("the forward did not render the second moment (RasterContext.set_depth(True, moment=True))")
    T = _map(fwd["T"], "T")
    H, W = T.shape
    out = torch.empty(1, dtype=torch.float32, device=T.device) if blocking else None
    check(_lib.load().gsplat_distortion_loss(
        _p(T), _p(_map(fwd["depth"], "depth", (H, W))), _p(_map(fwd["depth2"], "depth2", (H, W))), int(H), int(W),
        float(weight), int(bool(accumulate)), _p(_map(grad_alpha, "grad_alpha", (H, W))),
        _p(_map(grad_depth, "grad_depth", (H, W))), _p(_map(grad_depth2, "grad_depth2", (H, W))), _p(out), _stream()))
    return float(out.item()) if blocking else None


def depth_prior_loss(depth, target, weight, grad_depth, accumulate=False, blocking=False):
    """weight x mean over all H x W pixels of |depth - target| on the pixels with target > 0 (the others add nothing to
    the loss or the gradient); grad_depth gets weight / P x sign(depth - target), overwritten or, with accumulate=True,
    added to (gsplat_depth_prior_loss).  Whether the two maps hold z or 1/z is the caller's business.  blocking=True
    returns the loss (a read-back), otherwise None."""
    depth = _map(depth, "depth")
    H, W = depth.shape
    out = torch.empty(1, dtype=torch.float32, device=depth.device) if blocking else None
    check(_lib.load().gsplat_depth_prior_loss(_p(depth), _p(_map(target, "target", (H, W))), int(H), int(W), float(weight),
                                              int(bool(accumulate)), _p(_map(grad_depth, "grad_depth", (H, W))), _p(out),
                                              _stream()))
    return float(out.item()) if blocking else None


def _map3(t, name, shape=None):
    """An [H,W,3] float32 device map (a normal map, an image or a gradient of either); None stays None."""
    if t is None:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
            or t.dim() != 3 or t.shape[2] != 3 or (shape is not None and tuple(t.shape[:2]) != tuple(shape))):
        raise ValueError(f"{name} must be a contiguous [H,W,3] float32 device tensor" + (f" of size {tuple(shape)}" if shape else ""))
    return t


def pixel_intrinsics(cam):
    """(fx, fy, cx, cy) in pixels of a camera dict (scene.make_camera, app.camera_from_colmap, raster.device_camera), such
    that project_to_screen of z ((x - cx) / fx, (y - cy) / fy, 1) is the pixel (x, y) -- which the compositor samples at
    its integer coordinate: fx = proj[0] W / 2, cx = (proj[2] + 1) W / 2, and the same in y.  Python floats that are
    float32 values, as the C ABI takes them."""
    import numpy as np
    proj = cam["proj"]
    proj = (proj.detach().cpu().numpy() if isinstance(proj, torch.Tensor) else np.asarray(proj)).astype(np.float64).reshape(-1)
    W, H = float(cam["width"]), float(cam["height"])
    vals = (proj[0] * W / 2.0, proj[5] * H / 2.0, (proj[2] + 1.0) * W / 2.0, (proj[6] + 1.0) * H / 2.0)
    return tuple(float(np.float32(v)) for v in vals)


def _stencil_args(fwd, cam, inverse, alpha_min):
    """What depth_to_normal and its backward check before any launch -> (depth, T, H, W, fx, fy, cx, cy, inverse, alpha_min)."""
    import math
    if "depth" not in fwd:
        raise ValueError("the forward did not render depth (RasterContext.set_depth(True))")
    T = _map(fwd["T"], "T")
    H, W = T.shape
    depth = _map(fwd["depth"], "depth", (H, W))
    intr = cam if isinstance(cam, (tuple, list)) else pixel_intrinsics(cam)
    if len(intr) != 4 or not all(math.isfinite(v) for v in intr) or intr[0] == 0 or intr[1] == 0:
        raise ValueError("the pixel intrinsics (fx, fy, cx, cy) must be finite, fx and fy not 0")
    if not (0.0 < float(alpha_min) <= 1.0):
        raise ValueError("alpha_min must lie in (0, 1]")
    return (_p(depth), _p(T), int(H), int(W)) + tuple(float(v) for v in intr) + (int(bool(inverse)), float(alpha_min))


def depth_to_normal(fwd, cam, inverse, alpha_min=0.5, out=None):
    """The [H,W,3] normal map of a depth-mode forward (gsplat_depth_to_normal): camera coordinates, facing the camera, from
    central differences of the back-projected expected depth z = fwd["depth"] / (1 - fwd["T"]) (`inverse`: the forward
    composited 1/z, RasterContext.set_depth(True, inverse=True)).  A pixel without a normal -- the border, an opacity
    below alpha_min at it or at one of its four neighbours -- is (0,0,0).  cam: a camera dict, or (fx, fy, cx, cy) as
    pixel_intrinsics gives them.  out: the map to write, or None for a new one."""
    args = _stencil_args(fwd, cam, inverse, alpha_min)
    H, W = args[2], args[3]
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.float32, device=fwd["T"].device)
    check(_lib.load().gsplat_depth_to_normal(*args, _p(_map3(out, "out", (H, W))), _stream()))
    return out


def depth_to_normal_backward(fwd, cam, inverse, grad_normal, grad_depth, grad_alpha, alpha_min=0.5, accumulate=False):
    """dL/d normal ([H,W,3]) of depth_to_normal's map -> grad_depth = dL/d fwd["depth"] and grad_alpha = dL/d(1 - fwd["T"])
    ([H,W] maps as the backwards take them; either may be None), overwritten or, with accumulate=True, added to
    (gsplat_depth_to_normal_backward)."""
    args = _stencil_args(fwd, cam, inverse, alpha_min)
    H, W = args[2], args[3]
    if grad_normal is None:
        raise ValueError("grad_normal is required")
    check(_lib.load().gsplat_depth_to_normal_backward(
        *args, _p(_map3(grad_normal, "grad_normal", (H, W))), int(bool(accumulate)),
        _p(_map(grad_depth, "grad_depth", (H, W))), _p(_map(grad_alpha, "grad_alpha", (H, W))), _stream()))


def normal_prior_loss(normal, prior, weight, grad_normal, accumulate=False, blocking=False):
    """weight x mean over all H x W pixels of 1 - n . prior / |prior| on the pixels with a normal and a non-zero prior
    ([H,W,3], camera coordinates); grad_normal ([H,W,3] or None) gets -weight / P x prior / |prior| there and 0 elsewhere,
    overwritten or added to (gsplat_normal_prior_loss).  blocking=True returns the loss (a read-back), otherwise None."""
    normal = _map3(normal, "normal")
    if prior is None:
        raise ValueError("prior is required")
    H, W = normal.shape[:2]
    out = torch.empty(1, dtype=torch.float32, device=normal.device) if blocking else None
    check(_lib.load().gsplat_normal_prior_loss(_p(normal), _p(_map3(prior, "prior", (H, W))), int(H), int(W), float(weight),
                                               int(bool(accumulate)), _p(_map3(grad_normal, "grad_normal", (H, W))),
                                               _p(out), _stream()))
    return float(out.item()) if blocking else None


def normal_smoothness_loss(normal, image, weight, grad_normal, edge_scale=1.0, accumulate=False, blocking=False):
    """weight x (1 / P) x the sum over the horizontally or vertically adjacent pairs of pixels with a normal of
    w sum_c |n_a,c - n_b,c|, w = exp(-edge_scale x mean_c |I_a,c - I_b,c|) for `image` ([H,W,3], a constant) or 1 when it is
    None; grad_normal ([H,W,3] or None) gets the subgradient (sign(0) = 0), overwritten or added to
    (gsplat_normal_smoothness_loss).  blocking=True returns the loss (a read-back), otherwise None."""
    import math
    normal = _map3(normal, "normal")
    H, W = normal.shape[:2]
    if not math.isfinite(float(edge_scale)):
        raise ValueError("edge_scale must be finite")
    out = torch.empty(1, dtype=torch.float32, device=normal.device) if blocking else None
    check(_lib.load().gsplat_normal_smoothness_loss(_p(normal), _p(_map3(image, "image", (H, W))), int(H), int(W),
                                                    float(weight), float(edge_scale), int(bool(accumulate)),
                                                    _p(_map3(grad_normal, "grad_normal", (H, W))), _p(out), _stream()))
    return float(out.item()) if blocking else None


def _fmap(t, name, shape=None):
    """An [H,W,C] float32 device feature map (or a gradient or target of one), 1 <= C <= 512; None stays None."""
    if t is None:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
            or t.dim() != 3 or not 1 <= t.shape[2] <= 512 or (shape is not None and tuple(t.shape) != tuple(shape))):
        raise ValueError(f"{name} must be a contiguous [H,W,C] float32 device tensor, 1 <= C <= 512"
                         + (f", of shape {tuple(shape)}" if shape else ""))
    return t


def _pixel_map(t, name, dtype, shape):
    """An [H,W] device map of `dtype` (labels: int32, validity: uint8); None stays None."""
    if t is None:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous()
            or tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be a contiguous {tuple(shape)} {dtype} device tensor")
    return t


def feature_ce_loss(fmap, labels, weight, grad_map, accumulate=False, blocking=False):
    """Softmax cross-entropy of a feature map ([H,W,C], the channels as logits: RasterContext.render_features) against
    labels ([H,W] int32; a pixel takes part when 0 <= label < C, every other label is ignored): weight x the sum over those
    pixels of logsumexp - the label's logit, divided by ALL H x W pixels; grad_map ([H,W,C] or None) gets weight / P x
    (softmax - onehot) there and exactly 0 elsewhere, overwritten or, with accumulate=True, added to
    (gsplat_feature_ce_loss).  blocking=True returns the loss (a read-back), otherwise None."""
    fmap = _fmap(fmap, "fmap")
    if labels is None:
        raise ValueError("labels is required")
    H, W, C = fmap.shape
    out = torch.empty(1, dtype=torch.float32, device=fmap.device) if blocking else None
    check(_lib.load().gsplat_feature_ce_loss(_p(fmap), _p(_pixel_map(labels, "labels", torch.int32, (H, W))), int(H), int(W),
                                             int(C), float(weight), int(bool(accumulate)),
                                             _p(_fmap(grad_map, "grad_map", (H, W, C))), _p(out), _stream()))
    return float(out.item()) if blocking else None


def _feature_target_loss(fn, fmap, target, valid, weight, grad_map, accumulate, blocking):
    fmap = _fmap(fmap, "fmap")
    if target is None:
        raise ValueError("target is required")
    H, W, C = fmap.shape
    out = torch.empty(1, dtype=torch.float32, device=fmap.device) if blocking else None
    check(fn(_p(fmap), _p(_fmap(target, "target", (H, W, C))), _p(_pixel_map(valid, "valid", torch.uint8, (H, W))), int(H),
             int(W), int(C), float(weight), int(bool(accumulate)), _p(_fmap(grad_map, "grad_map", (H, W, C))), _p(out),
             _stream()))
    return float(out.item()) if blocking else None


def feature_l1_loss(fmap, target, weight, grad_map, valid=None, accumulate=False, blocking=False):
    """weight x the mean over all H x W x C elements of |fmap - target| on the pixels whose byte of `valid` ([H,W] uint8;
    None: every pixel) is set; grad_map gets weight / (P C) x sign(fmap - target) there (sign(0) = 0) and 0 elsewhere,
    overwritten or added to (gsplat_feature_l1_loss).  blocking=True returns the loss (a read-back), otherwise None."""
    return _feature_target_loss(_lib.load().gsplat_feature_l1_loss, fmap, target, valid, weight, grad_map, accumulate, blocking)


def feature_cosine_loss(fmap, target, weight, grad_map, valid=None, accumulate=False, blocking=False):
    """weight x the sum over the valid pixels with a non-zero map row f and a non-zero target row t of 1 - f.t / (|f||t|),
    divided by all H x W pixels; grad_map gets the gradient through the normalisation of f there and exactly 0 elsewhere,
    overwritten or added to (gsplat_feature_cosine_loss).  blocking=True returns the loss (a read-back), otherwise None."""
    return _feature_target_loss(_lib.load().gsplat_feature_cosine_loss, fmap, target, valid, weight, grad_map, accumulate,
                                blocking)


def feature_adam_step(compact_to_global, num_culled, features, exp_avg, exp_avg_sq, grad_global, lr, b1, b2, eps, bias1,
                      bias2):
    """The Adam step of the feature column on the rows a view saw (gsplat_feature_adam_step): features, exp_avg,
    exp_avg_sq and grad_global are [N,C] float32 in global gaussian order, compact_to_global the forward's int32 row map
    with at least num_culled entries.  The rows compact_to_global names are updated in place from their rows of
    grad_global -- the element step of gsplat_optimizer_step, bit for bit -- and those gradient rows are zeroed; no other
    row of any of the four is read or written."""
    M = int(num_culled)
    if features.dim() != 2 or not 1 <= features.shape[1] <= 512:
        raise ValueError("features must be [N,C] with 1 <= C <= 512")
    for name, t in (("features", features), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("grad_global", grad_global)):
        if _f32(t, name).shape != features.shape:
            raise ValueError(f"{name} must be shaped as features, {tuple(features.shape)}")
    if M < 0 or M > features.shape[0]:
        raise ValueError("num_culled must lie in 0 .. N")
    if M and (compact_to_global is None or compact_to_global.dtype != torch.int32 or compact_to_global.numel() < M):
        raise ValueError("compact_to_global must be int32 with at least num_culled entries")
    check(_lib.load().gsplat_feature_adam_step(_p(compact_to_global) if M else None, M, int(features.shape[1]),
                                               _p(features), _p(exp_avg), _p(exp_avg_sq), _p(grad_global), float(lr),
                                               float(b1), float(b2), float(eps), float(bias1), float(bias2), _stream()))


def _bilagrid(t, name, shape=None):
    """A [12,L,Hg,Wg] float32 device bilateral grid (or a gradient of one) -> (tensor, Wg, Hg, L); None stays None."""
    if t is None:
        return None
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
            or t.dim() != 4 or t.shape[0] != 12 or (shape is not None and tuple(t.shape) != tuple(shape))):
        raise ValueError(f"{name} must be a contiguous [12,L,Hg,Wg] float32 device tensor"
                         + (f" of shape {tuple(shape)}" if shape else ""))
    return t


def identity_bilagrid(grid_w, grid_h, grid_l, views=None, device="cuda"):
    """The grid that gives every image back: channels 0, 5 and 10 (the diagonal of the 3x4 affine) one, the others zero;
    [12,L,Hg,Wg], or [views,12,L,Hg,Wg]."""
    grid = torch.zeros((12, int(grid_l), int(grid_h), int(grid_w)), dtype=torch.float32, device=device)
    grid[[0, 5, 10]] = 1.0
    return grid if views is None else grid.unsqueeze(0).repeat(int(views), 1, 1, 1, 1).contiguous()


def bilagrid_slice(grid, image, out=None):
    """The image corrected by a bilateral grid (gsplat_bilagrid_slice): per pixel the 3x4 affine interpolated from `grid`
    ([12,L,Hg,Wg]) at the pixel's position and luma, applied to its colour; image and out are [H,W,3].  out: the map to
    write, or None for a new one."""
    grid = _bilagrid(grid, "grid")
    image = _map3(image, "image")
    if grid is None or image is None:
        raise ValueError("grid and image are required")
    H, W = image.shape[:2]
    if out is None:
        out = torch.empty_like(image)
    _, L, Hg, Wg = grid.shape
    check(_lib.load().gsplat_bilagrid_slice(_p(grid), int(Wg), int(Hg), int(L), _p(image), int(H), int(W),
                                            _p(_map3(out, "out", (H, W))), _stream()))
    return out


def bilagrid_slice_backward(grid, image, grad_out, grad_image=None, grad_grid=None, accumulate_grid=False):
    """dL/d corrected ([H,W,3]) of bilagrid_slice -> grad_image = dL/d image ([H,W,3] or None; written, never added to;
    must not be grad_out or image) and grad_grid = dL/d grid ([12,L,Hg,Wg] or None; overwritten, or added to with
    accumulate_grid=True) (gsplat_bilagrid_slice_backward)."""
    grid = _bilagrid(grid, "grid")
    image = _map3(image, "image")
    if grid is None or image is None or grad_out is None:
        raise ValueError("grid, image and grad_out are required")
    H, W = image.shape[:2]
    _, L, Hg, Wg = grid.shape
    check(_lib.load().gsplat_bilagrid_slice_backward(
        _p(grid), int(Wg), int(Hg), int(L), _p(image), _p(_map3(grad_out, "grad_out", (H, W))), int(H), int(W),
        int(bool(accumulate_grid)), _p(_map3(grad_image, "grad_image", (H, W))),
        _p(_bilagrid(grad_grid, "grad_grid", grid.shape)), _stream()))


def bilagrid_tv_loss(grid, weight, grad_grid, accumulate=False, blocking=False):
    """The total-variation loss of one bilateral grid: weight x the sum over the three axes of the mean squared difference
    of the adjacent pairs along the axis (all 12 channels; an axis of one vertex adds 0); grad_grid ([12,L,Hg,Wg] or None)
    gets the gradient, overwritten or added to (gsplat_bilagrid_tv_loss).  blocking=True returns the loss (a read-back),
    otherwise None."""
    grid = _bilagrid(grid, "grid")
    if grid is None:
        raise ValueError("grid is required")
    _, L, Hg, Wg = grid.shape
    out = torch.empty(1, dtype=torch.float32, device=grid.device) if blocking else None
    check(_lib.load().gsplat_bilagrid_tv_loss(_p(grid), int(Wg), int(Hg), int(L), float(weight), int(bool(accumulate)),
                                              _p(_bilagrid(grad_grid, "grad_grid", grid.shape)), _p(out), _stream()))
    return float(out.item()) if blocking else None


VQ_MAX_D, VQ_MAX_K = 64, 65536


def _vq_rows(t, name, cols=None):
    """A contiguous [rows, D] float32 device tensor with 1 <= D <= 64 (and D == cols when given)."""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
            or t.dim() != 2 or not 1 <= t.shape[1] <= VQ_MAX_D or (cols is not None and t.shape[1] != cols)):
        raise ValueError(f"{name} must be a contiguous [rows,D] float32 device tensor, 1 <= D <= {VQ_MAX_D}"
                         + (f", D = {cols}" if cols is not None else ""))
    return t


def _vq_codebook(t, D):
    t = _vq_rows(t, "codebook", D)
    if not 1 <= t.shape[0] <= VQ_MAX_K:
        raise ValueError(f"codebook must have 1 .. {VQ_MAX_K} rows")
    return t


def _vq_column(t, name, n, dtype):
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous()
            or tuple(t.shape) != (n,)):
        raise ValueError(f"{name} must be a contiguous [{n}] {dtype} device tensor")
    return t


def vq_assign(x, codebook, index=None, dist=None):
    """The nearest centroid of every row (gsplat_vq_assign): x [N,D], codebook [K,D] -> index [N] int32 (written into
    `index` when given).  dist: None, or an [N] float32 tensor that gets the squared distance to the chosen centroid.
    Ties resolve to the lowest index."""
    x = _vq_rows(x, "x")
    N, D = x.shape
    codebook = _vq_codebook(codebook, D)
    index = torch.empty(N, dtype=torch.int32, device=x.device) if index is None else _vq_column(index, "index", N, torch.int32)
    if dist is not None:
        _vq_column(dist, "dist", N, torch.float32)
    check(_lib.load().gsplat_vq_assign(_p(x), _p(codebook), int(N), int(D), int(codebook.shape[0]), _p(index), _p(dist),
                                       _stream()))
    return index


def vq_update(x, index, codebook):
    """Every centroid becomes the mean of the rows assigned to it, in place (gsplat_vq_update); a centroid without rows
    keeps its bits.  The rows are ordered by (index, row) with a stable sort: the sums have one order."""
    x = _vq_rows(x, "x")
    N, D = x.shape
    codebook = _vq_codebook(codebook, D)
    K = codebook.shape[0]
    _vq_column(index, "index", N, torch.int32)
    if N:
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= K:
            raise ValueError("index must lie in 0 .. K-1")
    order = torch.sort(index, stable=True).indices.to(torch.int32).contiguous()
    start = torch.zeros(K + 1, dtype=torch.int32, device=x.device)
    start[1:] = torch.cumsum(torch.bincount(index, minlength=K), 0)
    check(_lib.load().gsplat_vq_update(_p(x), _p(order), _p(start), int(N), int(D), int(K), _p(codebook), _stream()))
    return codebook


def vq_fit(x, K, iterations=10, seed=0):
    """k-means (Lloyd) over the rows of x [N,D] -> (codebook [K,D], index [N] int32, objective per assign).  K is clamped
    to N.  The initial centroids are the first K rows of a seeded permutation.  Each of `iterations` rounds is an assign,
    a re-seeding -- every empty cluster, in index order, takes one of the rows with the largest distance (descending,
    ties by row index) and that row moves to it -- and an update; a last assign makes `index` nearest for the codebook
    returned.  objective[t] is the sum of the squared distances after assign t (iterations + 1 values, never increasing
    beyond what the assign's rounding allows).  The same seed reproduces codebook and index bit for bit."""
    x = _vq_rows(x, "x")
    N, D = x.shape
    if not isinstance(K, int) or K < 1:
        raise ValueError("K must be a positive integer")
    if N < 1:
        raise ValueError("x has no rows")
    if not isinstance(iterations, int) or iterations < 0:
        raise ValueError("iterations must be a non-negative integer")
    K = min(K, N)
    if K > VQ_MAX_K:
        raise ValueError(f"K must be at most {VQ_MAX_K}")
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:K]
    codebook = x[perm.to(x.device)].contiguous()
    index = torch.empty(N, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, dtype=torch.float32, device=x.device)
    objective = []
    for it in range(iterations + 1):
        vq_assign(x, codebook, index, dist)
        objective.append(float(dist.sum(dtype=torch.float64)))
        if it == iterations:
            break
        empty = (torch.bincount(index, minlength=K) == 0).nonzero().flatten()
        if empty.numel():
            donors = torch.sort(dist, descending=True, stable=True).indices[:empty.numel()]
            codebook[empty] = x[donors]
            index[donors] = empty.to(torch.int32)
        vq_update(x, index, codebook)
    return codebook, index, objective


TSDF_MAX_NODES = 2 ** 31 - 1  # GSPLAT_TSDF_MAX_NODES


def tsdf_volume(origin, voxel, dims, color=True, device="cuda"):
    """A zeroed TSDF volume: dict(tsdf [nz,ny,nx], weight [nz,ny,nx], color [nz,ny,nx,3] or None, origin, voxel, dims).
    Node (i,j,k) sits at origin + voxel * (i,j,k); dims = (nx, ny, nz), x fastest in memory.  origin and voxel are kept as
    the float32 values the kernels take (Python floats)."""
    import numpy as np
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 1 or nx * ny * nz > TSDF_MAX_NODES:
        raise ValueError(f"dims must be positive and hold at most {TSDF_MAX_NODES} nodes")
    origin = tuple(float(np.float32(v)) for v in origin)
    voxel = float(np.float32(voxel))
    if len(origin) != 3 or not all(np.isfinite(origin)) or not (np.isfinite(voxel) and voxel > 0.0):
        raise ValueError("origin must be three finite numbers and voxel finite and positive")
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
    return dict(tsdf=z(nz, ny, nx), weight=z(nz, ny, nx), color=z(nz, ny, nx, 3) if color else None, origin=origin,
                voxel=voxel, dims=(nx, ny, nz))


def _tsdf_grid(volume):
    """The checked device arrays of a tsdf_volume -> (tsdf, weight, color or None, (nx, ny, nz), origin as float[3])."""
    nx, ny, nz = (int(d) for d in volume["dims"])
    tsdf, weight, color = volume["tsdf"], volume["weight"], volume.get("color")
    for t, name, shape in ((tsdf, "tsdf", (nz, ny, nx)), (weight, "weight", (nz, ny, nx)), (color, "color", (nz, ny, nx, 3))):
        if t is None and name == "color":
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                or tuple(t.shape) != shape):
            raise ValueError(f"volume['{name}'] must be a contiguous float32 device tensor of shape {shape}")
    return tsdf, weight, color, (nx, ny, nz), (ctypes.c_float * 3)(*[float(v) for v in volume["origin"]])


def _host_rows(t, name, rows, cols):
    """[rows, cols] float32 on the host (from a tensor, device or not, or anything numpy takes), as a ctypes pointer."""
    import numpy as np
    a = np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)), dtype=np.float32)
    if a.shape != (rows, cols):
        raise ValueError(f"{name} must be [{rows},{cols}]")
    return a, a.ctypes.data_as(ctypes.c_void_p)


def tsdf_integrate(volume, depth, T, view, intrinsics, image=None, inverse=False, alpha_min=0.5, trunc=None, near=0.0,
                   max_depth=0.0, max_weight=0.0, surface=False):
    """Fuse K views of one size into `volume` in place (gsplat_tsdf_integrate): depth, T [K,H,W] as a depth-mode forward
    renders them (`inverse`: the forward composited 1/z), image [K,H,W,3] exactly when the volume has colour, view [K,12]
    row-major [R|t] (the first twelve numbers of a camera dict's view), intrinsics [K,4] as pixel_intrinsics gives them.
    Per node and view, in batch order: skip unless z > near, the nearest pixel lies in the image, is ok (1 - T >= alpha_min,
    depth > 0) and its surface depth d = depth / (1 - T) is at most max_depth (<= 0: no limit) and d - z >= -trunc; then
    tsdf = (w tsdf + min(1, (d - z) / trunc)) / (w + 1), colour likewise, w = min(w + 1, max_weight) (<= 0: no cap).
    trunc: 4 voxels unless given.  The volume is read and written once per gsplat_tsdf_views_per_pass() views, and a batch
    is bit for bit its views one call at a time.  Returns the volume.
    surface=True (gsplat_tsdf_integrate_surface): depth holds the surface depth d itself -- RasterContext.median_depth's
    map, or sensor depth -- and a pixel is ok when depth is finite and > 0 and either T is None (no opacity gate) or
    1 - T >= alpha_min; `inverse` must then be left False."""
    if surface and inverse:
        raise ValueError("surface=True takes the surface depth itself: inverse must be False")
    if T is None and not surface:
        raise ValueError("T may be None only with surface=True")
    tsdf, weight, color, (nx, ny, nz), origin = _tsdf_grid(volume)
    for t, name in ((depth, "depth"), (T, "T")):
        if t is None and name == "T":
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                or t.dim() != 3 or t.shape != depth.shape):
            raise ValueError(f"{name} must be a contiguous [K,H,W] float32 device tensor")
    K, H, W = (int(s) for s in depth.shape)
    if (image is None) != (color is None):
        raise ValueError("image goes with a volume that has colour, and only with one")
    if image is not None and (not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or not image.is_cuda
                              or not image.is_contiguous() or tuple(image.shape) != (K, H, W, 3)):
        raise ValueError("image must be a contiguous [K,H,W,3] float32 device tensor")
    if K == 0:
        return volume
    view_a, view_p = _host_rows(view, "view", K, 12)
    intr_a, intr_p = _host_rows(intrinsics, "intrinsics", K, 4)
    trunc = 4.0 * volume["voxel"] if trunc is None else trunc
    if surface:
        check(_lib.load().gsplat_tsdf_integrate_surface(
            _p(tsdf), _p(weight), _p(color), nx, ny, nz, origin, float(volume["voxel"]), _p(depth), _p(T), _p(image),
            view_p, intr_p, K, H, W, float(alpha_min), float(trunc), float(near), float(max_depth), float(max_weight),
            _stream()))
        return volume
    check(_lib.load().gsplat_tsdf_integrate(
        _p(tsdf), _p(weight), _p(color), nx, ny, nz, origin, float(volume["voxel"]), _p(depth), _p(T), _p(image), view_p,
        intr_p, K, H, W, int(bool(inverse)), float(alpha_min), float(trunc), float(near), float(max_depth),
        float(max_weight), _stream()))
    return volume


def tsdf_extract(volume, min_weight=1.0):
    """The zero level set of a TSDF volume as an indexed triangle mesh -> (vertices [Nv,3] float32, faces [Nf,3] int32,
    colors [Nv,3] float32 or None), device tensors; marching tetrahedra on the Freudenthal split of every cell whose eight
    nodes have weight >= min_weight (gsplat_tsdf_mark, a prefix sum, gsplat_tsdf_emit; include/gsplat_hip.h states the
    vertex, face and winding order).  Watertight wherever the observed cells are; (v1 - v0) x (v2 - v0) points from inside
    (tsdf < 0) to outside.  No atomics and no sort: two runs give the same bits.  One read-back (the two totals)."""
    tsdf, weight, color, (nx, ny, nz), origin = _tsdf_grid(volume)
    dev, n = tsdf.device, nx * ny * nz
    lib = _lib.load()
    cell_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    edge_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    tri_count = torch.empty(n, dtype=torch.int32, device=dev)
    vert_count = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.gsplat_tsdf_mark(_p(tsdf), _p(weight), nx, ny, nz, float(min_weight), _p(cell_ok), _p(tri_count),
                               _p(edge_mask), _p(vert_count), _stream()))
    vert_offset = torch.cumsum(vert_count, 0, dtype=torch.int64)
    tri_offset = torch.cumsum(tri_count, 0, dtype=torch.int64)
    num_vertices, num_faces = (int(v) for v in torch.stack((vert_offset[-1], tri_offset[-1])).tolist())  # the read-back
    if num_vertices > 2 ** 31 - 1 or num_faces > 2 ** 31 - 1:
        raise ValueError("the mesh has more than 2^31 - 1 vertices or faces: extract at a coarser resolution")
    vert_offset -= vert_count  # inclusive -> exclusive
    tri_offset -= tri_count
    del vert_count, tri_count
    vertices = torch.empty(num_vertices, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(num_faces, 3, dtype=torch.int32, device=dev)
    colors = None if color is None else torch.empty(num_vertices, 3, dtype=torch.float32, device=dev)
    if num_vertices or num_faces:
        check(lib.gsplat_tsdf_emit(_p(tsdf), _p(color) if num_vertices else None, nx, ny, nz, origin,
                                   float(volume["voxel"]), _p(cell_ok), _p(edge_mask), _p(vert_offset), _p(tri_offset),
                                   num_vertices, num_faces, _p(vertices), _p(colors), _p(faces), _stream()))
    return vertices, faces, colors


def _mesh_faces(faces, num_vertices):
    if (not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or not faces.is_cuda or not faces.is_contiguous()
            or faces.dim() != 2 or faces.shape[1] != 3):
        raise ValueError("faces must be a contiguous [Nf,3] int32 device tensor")
    if isinstance(num_vertices, bool) or not isinstance(num_vertices, int) or num_vertices < 0:
        raise ValueError("num_vertices must be a non-negative integer")
    if faces.shape[0] and not num_vertices:
        raise ValueError("faces without vertices")


def mesh_components(faces, num_vertices):
    """The connected components of an indexed mesh (gsplat_mesh_components): faces [Nf,3] int32 on the device into
    num_vertices vertices -> dict(label [Nv] int32: the smallest vertex index of the vertex's component, two vertices being
    connected when a face holds both and a vertex in no face labelling itself; face_count [Nv] int32: at a label the number
    of faces of its component, 0 elsewhere; rounds: the hook rounds that ran).  A lock-free union-find, a flatten and a
    count launch; integers only: the same bits in every run.  A face index outside [0, num_vertices) is an error (-3)
    found on the device before anything is written; that check is the call's one read-back."""
    _mesh_faces(faces, num_vertices)
    label = torch.empty(num_vertices, dtype=torch.int32, device=faces.device)
    face_count = torch.empty(num_vertices, dtype=torch.int32, device=faces.device)
    rounds = ctypes.c_int(0)
    check(_lib.load().gsplat_mesh_components(_p(faces), int(faces.shape[0]), num_vertices, _p(label), _p(face_count),
                                             ctypes.byref(rounds), _stream()))
    return dict(label=label, face_count=face_count, rounds=int(rounds.value))


def mesh_filter(vertices, faces, colors=None, min_faces=0, keep_largest=0):
    """Drop connected components of an indexed mesh -> (vertices, faces, colors, report).  A component (mesh_components)
    is kept iff its face_count >= min_faces and, when keep_largest > 0, it is among the keep_largest components ranked by
    (-face_count, label); an unreferenced vertex is a component of 0 faces.  Kept vertices, colours and faces keep their
    order, the face indices are renumbered (gsplat_mesh_compact).  The selection is torch on the device (one sort over the
    vertices, no host loop over components), the prefix sums are torch.cumsum, and one read-back fetches the new sizes.
    report: dict(components, kept, faces_removed, vertices_removed).  With min_faces and keep_largest both 0 the inputs
    are returned as they are and nothing is launched (report: None)."""
    for name, v in (("min_faces", min_faces), ("keep_largest", keep_largest)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be a non-negative integer")
    if (not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32 or not vertices.is_cuda
            or not vertices.is_contiguous() or vertices.dim() != 2 or vertices.shape[1] != 3):
        raise ValueError("vertices must be a contiguous [Nv,3] float32 device tensor")
    nv = int(vertices.shape[0])
    _mesh_faces(faces, nv)
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32 or not colors.is_cuda
                               or not colors.is_contiguous() or tuple(colors.shape) != (nv, 3)):
        raise ValueError("colors must be a contiguous [Nv,3] float32 device tensor or None")
    if min_faces == 0 and keep_largest == 0:
        return vertices, faces, colors, None
    dev, nf = vertices.device, int(faces.shape[0])
    comp = mesh_components(faces, nv)
    label, count = comp["label"].long(), comp["face_count"].long()
    ids = torch.arange(nv, dtype=torch.int64, device=dev)
    is_root = label == ids
    keep_root = is_root & (count >= min_faces)
    if keep_largest > 0:  # rank the roots by (-face_count, label); every non-root sorts behind them
        key = torch.where(is_root, (nf - count) * max(nv, 1) + ids, torch.full_like(ids, torch.iinfo(torch.int64).max))
        rank = torch.empty_like(ids)
        rank[torch.argsort(key)] = ids
        keep_root &= rank < keep_largest
    keep_vertex = keep_root[label]
    keep_face = keep_vertex[faces[:, 0].long()] if nf else torch.zeros(0, dtype=torch.bool, device=dev)
    vertex_offset = torch.cumsum(keep_vertex, 0, dtype=torch.int64)
    face_offset = torch.cumsum(keep_face, 0, dtype=torch.int64)
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    new_nv, new_nf, components, kept = (int(v) for v in torch.stack((
        vertex_offset[-1] if nv else zero, face_offset[-1] if nf else zero, is_root.sum(), keep_root.sum())).tolist())
    keep_u8 = keep_vertex.to(torch.uint8)
    vertex_offset -= keep_u8  # inclusive -> exclusive
    face_offset -= keep_face.to(torch.uint8)
    out_v = torch.empty(new_nv, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(new_nf, 3, dtype=torch.int32, device=dev)
    out_c = None if colors is None else torch.empty(new_nv, 3, dtype=torch.float32, device=dev)
    if new_nv:
        some_faces = new_nf > 0
        check(_lib.load().gsplat_mesh_compact(
            _p(vertices), _p(colors), _p(faces) if some_faces else None, nv, nf if some_faces else 0,
            _p(keep_u8), _p(vertex_offset), _p(face_offset) if some_faces else None, _p(out_v),
            _p(out_c), _p(out_f) if some_faces else None, _stream()))
    report = dict(components=components, kept=kept, faces_removed=nf - new_nf, vertices_removed=nv - new_nv)
    return out_v, out_f, out_c, report


def compute_psnr(predicted_data, gt_data, rows, cols):
    out = ctypes.c_float(0.0)
    check(_lib.load().gsplat_compute_psnr(_p(predicted_data), _p(gt_data), rows, cols, ctypes.byref(out), _stream()))
    return float(out.value)


def adam_step(params, param_grads, exp_avg, exp_avg_sq, lr, b1, b2, eps, bias1, bias2, N, S):
    check(_lib.load().gsplat_adam_step(_p(params), _p(param_grads), _p(exp_avg), _p(exp_avg_sq), lr, b1, b2, eps,
                                       bias1, bias2, N, S, _stream()))


def initialize_gaussians(points_xyz, points_rgb):
    """Gaussians::Initialize (src/gaussian.cpp:38-104) on the GPU.  points_xyz: float64 [N,3] device tensor,
    points_rgb: uint8 [N,3] device tensor.  Returns the parameter dict (xyz rgb opacity scale quaternion)."""
    import torch
    N = int(points_xyz.shape[0])
    assert points_xyz.dtype == torch.float64 and points_rgb.dtype == torch.uint8
    z = lambda *s: torch.empty(*s, dtype=torch.float32, device=points_xyz.device)
    out = dict(xyz=z(N, 3), rgb=z(N, 3), opacity=z(N), scale=z(N, 3), quaternion=z(N, 4))
    check(_lib.load().gsplat_initialize_gaussians(_p(points_xyz.contiguous()), _p(points_rgb.contiguous()), N,
                                                  _p(out["xyz"]), _p(out["rgb"]), _p(out["opacity"]), _p(out["scale"]),
                                                  _p(out["quaternion"]), _stream()))
    return out


def knn_mean_distance(points_xyz, k=3):
    import torch
    N = int(points_xyz.shape[0])
    out = torch.empty(N, dtype=torch.float32, device=points_xyz.device)
    check(_lib.load().gsplat_knn_mean_distance(_p(points_xyz.contiguous()), N, int(k), _p(out), _stream()))
    return out


def compute_morton_codes(N, d_xyz, x_max, y_max, z_max, x_min, y_min, z_min, codes):
    """compute_morton_codes(...) (cuda_forward.cuh:186-188); codes: int64/uint64 device tensor [N]."""
    check(_lib.load().gsplat_compute_morton_codes(N, _p(d_xyz), x_max, y_max, z_max, x_min, y_min, z_min, _p(codes),
                                                  _stream()))


_ATTRS = ("xyz", "rgb", "opacity", "scale", "quaternion", "sh")


def clone_gaussians(N, num_sh_coef, mask, write_ids, src, dst):
    """clone_gaussians(...) (adaptive_density.cuh:27-31); src / dst: dicts xyz rgb opacity scale quaternion sh."""
    check(_lib.load().gsplat_clone_gaussians(N, num_sh_coef, _p(mask), _p(write_ids), *[_p(src.get(k)) for k in _ATTRS],
                                             *[_p(dst.get(k)) for k in _ATTRS], _stream()))


def split_gaussians(N, scale_factor, num_sh_coef, mask, write_ids, src, dst, seed=0):
    """split_gaussians(...) (adaptive_density.cuh:53-57) with an explicit seed."""
    check(_lib.load().gsplat_split_gaussians(N, scale_factor, num_sh_coef, _p(mask), _p(write_ids),
                                             *[_p(src.get(k)) for k in _ATTRS], *[_p(dst.get(k)) for k in _ATTRS],
                                             int(seed), _stream()))


def density_masks(opacity, scale, uv_grad_accum, grad_accum_dur, op_threshold, max_scale, uv_grad_threshold,
                  clone_scale_threshold):
    """Masks of TrainerImpl::adaptive_density_step (cuda/trainer.cu:416-575).
    Returns (prune, clone, split, keep) uint8 tensors and the (pruned, cloned, split) counts."""
    import torch
    N = int(opacity.shape[0])
    m = [torch.empty(N, dtype=torch.uint8, device=opacity.device) for _ in range(4)]
    counts = torch.zeros(3, dtype=torch.int32, device=opacity.device)
    check(_lib.load().gsplat_density_masks(N, _p(opacity), _p(scale), _p(uv_grad_accum), _p(grad_accum_dur),
                                           op_threshold, max_scale, uv_grad_threshold, clone_scale_threshold,
                                           _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]), _p(counts), _stream()))
    return m[0], m[1], m[2], m[3], [int(c) for c in counts.tolist()]


def expand_sh(sh, l_max_old):
    """add_sh_band's re-layout: [N,(l+1)^2-1,3] -> [N,(l+2)^2-1,3] with the new band zero."""
    import torch
    N = int(sh.shape[0])
    out = torch.empty(N, (l_max_old + 2) ** 2 - 1, 3, dtype=torch.float32, device=sh.device)
    check(_lib.load().gsplat_expand_sh(N, l_max_old, _p(sh) if l_max_old > 0 else None, _p(out), _stream()))
    return out


def gather_rows(src, order):
    """out[i] = src[order[i]] along dim 0 (order: int32 device tensor)."""
    import torch
    out = torch.empty_like(src)
    N = int(src.shape[0])
    stride = src.numel() // N if N else 0
    check(_lib.load().gsplat_gather_rows(N, stride, _p(order), _p(src), _p(out), _stream()))
    return out


def sample_by_weight(weights, K, seed, counts=None):
    """K draws from the rows of `weights` ([N] non-negative device tensor) with probability proportional to the weight
    (gsplat_sample_by_weight; the prefix sum is torch.cumsum in float64).  Returns (samples [K] int32, counts [N] int32:
    how often each row was drawn; `counts` given: accumulated into that tensor instead); a row of weight zero is never
    drawn, and a seed reproduces the draw bit for bit.
    All weights zero: ValueError (a blocking read of the sum; this runs once per refinement step)."""
    N, K = int(weights.shape[0]), int(K)
    samples = torch.empty(K, dtype=torch.int32, device=weights.device)
    if counts is None:
        counts = torch.zeros(N, dtype=torch.int32, device=weights.device)
    elif counts.dtype != torch.int32 or counts.numel() != N:
        raise ValueError("counts must be int32 [N]")
    if N == 0 or K == 0:
        if K:
            raise ValueError("sample_by_weight: no rows to draw from")
        return samples, counts
    cdf = torch.cumsum(weights.reshape(-1).to(torch.float64), 0).contiguous()
    if not float(cdf[-1]) > 0.0:
        raise ValueError("sample_by_weight: the weights sum to zero")
    check(_lib.load().gsplat_sample_by_weight(_p(cdf), N, K, int(seed) & 0xFFFFFFFFFFFFFFFF, _p(samples), _p(counts),
                                              _stream()))
    return samples, counts


def mcmc_relocate(opacity, scale, counts, min_opacity=0.005):
    """In place (gsplat_mcmc_relocate): row i with counts[i] > 0 gets the opacity logit and log-scales of one of
    min(counts[i] + 1, 51) coincident copies that together render what it rendered; the other rows are not written."""
    N = int(opacity.shape[0])
    if counts.dtype != torch.int32 or counts.numel() != N or scale.numel() != 3 * N:
        raise ValueError("counts must be int32 [N] and scale [N,3]")
    check(_lib.load().gsplat_mcmc_relocate(N, _p(_f32(opacity, "opacity")), _p(_f32(scale, "scale")), _p(counts),
                                           float(min_opacity), _stream()))


def mcmc_add_noise(xyz, opacity, scale, quaternion, scaler, seed):
    """In place on xyz (gsplat_mcmc_add_noise): xyz[i] += Sigma_i nu with nu = normal * gate(opacity_i) * scaler; only
    nearly transparent gaussians move, and scaler == 0 leaves xyz bit-unchanged."""
    N = int(xyz.shape[0])
    if opacity.numel() != N or scale.numel() != 3 * N or quaternion.numel() != 4 * N or xyz.numel() != 3 * N:
        raise ValueError("xyz [N,3], opacity [N], scale [N,3] and quaternion [N,4] must have the same N")
    check(_lib.load().gsplat_mcmc_add_noise(N, _p(_f32(xyz, "xyz")), _p(_f32(opacity, "opacity")),
                                            _p(_f32(scale, "scale")), _p(_f32(quaternion, "quaternion")), float(scaler),
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()))


def mcmc_regularize(compact_to_global, opacity, scale, w_opacity, w_scale, grad_opacity, grad_scale, M=None):
    """grad_opacity[j] += w_opacity * s (1 - s), grad_scale[j] += w_scale * exp(scale[i]) for j < M with
    i = compact_to_global[j], s = sigmoid(opacity[i]) (gsplat_mcmc_regularize).  M defaults to the rows of grad_opacity."""
    M = int(grad_opacity.shape[0]) if M is None else int(M)
    if compact_to_global.dtype != torch.int32 or compact_to_global.numel() < M:
        raise ValueError("compact_to_global must be int32 with at least M entries")
    if grad_opacity.numel() < M or grad_scale.numel() < 3 * M:
        raise ValueError("the gradient arrays are shorter than M rows")
    check(_lib.load().gsplat_mcmc_regularize(M, _p(compact_to_global), _p(_f32(opacity, "opacity")),
                                             _p(_f32(scale, "scale")), float(w_opacity), float(w_scale),
                                             _p(_f32(grad_opacity, "grad_opacity")), _p(_f32(grad_scale, "grad_scale")),
                                             _stream()))


def compact_masked_array(stride, d_source, d_mask, num_culled=None):
    """compact_masked_array<STRIDE>(d_source, d_mask, num_culled) -> new tensor [num_culled*stride].  With num_culled
    given the count is trusted, as the reference's template does (cuda_data.cuh:106-127): no read-back, the call stays
    asynchronous; without it the library reads the count back (blocks the host)."""
    N = int(d_mask.numel())
    if num_culled is not None:
        out = torch.empty(max(int(num_culled) * stride, 1), dtype=torch.float32, device=d_mask.device if N else "cuda")
        # the room of `out` is stated: a count that is too small drops rows, it does not write past the tensor (r05)
        check(_lib.load().gsplat_compact_masked_array_bounded(_p(d_source), _p(d_mask), N, stride, _p(out), int(num_culled),
                                                              None, _stream()))
        return out[: int(num_culled) * stride]
    out = torch.empty(max(N * stride, 1), dtype=torch.float32, device=d_mask.device if N else "cuda")
    n = ctypes.c_int(0)
    check(_lib.load().gsplat_compact_masked_array(_p(d_source), _p(d_mask), N, stride, _p(out), ctypes.byref(n),
                                                  _stream()))
    return out[: n.value * stride]


def scatter_masked_array(stride, d_compacted, d_mask, d_destination):
    check(_lib.load().gsplat_scatter_masked_array(_p(d_compacted), _p(d_mask), int(d_mask.numel()), stride,
                                                  _p(d_destination), _stream()))


def camera_arrays(cams, device="cuda"):
    """The device camera arrays compute_filter3d reads, from a list of camera dicts (scene.make_camera /
    raster.device_camera): views [V,16], projs [V,16], focal_x [V] float32 and sizes [V,2] int32 (width, height)."""
    import numpy as np

    def host(m):
        return (m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)).astype(np.float32).reshape(16)

    views = torch.as_tensor(np.stack([host(c["view"]) for c in cams])).to(device).contiguous()
    projs = torch.as_tensor(np.stack([host(c["proj"]) for c in cams])).to(device).contiguous()
    focal = torch.as_tensor(np.asarray([float(c["fx"]) for c in cams], np.float32)).to(device)
    sizes = torch.as_tensor(np.asarray([[int(c["width"]), int(c["height"])] for c in cams], np.int32)).to(device)
    return views, projs, focal, sizes.contiguous()


def compute_filter3d(xyz, views, projs, focal_x, sizes, near=0.2, out=None):
    """The 3D smoothing filter of every gaussian (gsplat_compute_filter3d): filter3d[i] = sqrt(0.2) * the smallest
    z / focal_x over the cameras that sample gaussian i; a gaussian no camera samples takes the largest value of the
    sampled ones.  Camera arrays as camera_arrays() returns them.  Returns the [N] float32 device tensor."""
    N, V = int(xyz.shape[0]), int(focal_x.shape[0])
    if views.numel() != 16 * V or projs.numel() != 16 * V or sizes.numel() != 2 * V or sizes.dtype != torch.int32:
        raise ValueError("views / projs must be [V,16] float32, sizes [V,2] int32")
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=xyz.device)
    check(_lib.load().gsplat_compute_filter3d(_p(_f32(xyz, "xyz")), N, _p(_f32(views, "views")), _p(_f32(projs, "projs")),
                                              _p(_f32(focal_x, "focal_x")), _p(sizes), V, float(near),
                                              _p(_f32(out, "out")), _stream()))
    return out


def filter3d_apply(scale, opacity, filter3d, scale_eff=None, opacity_eff=None):
    """(scale [N,3], opacity [N], filter3d [N]) -> (scale_eff, opacity_eff): the parameters a filtered gaussian enters the
    rasterizer with (gsplat_filter3d_apply); rows with filter3d == 0 come back bit-identical."""
    N = int(opacity.shape[0])
    scale_eff = torch.empty_like(scale) if scale_eff is None else scale_eff
    opacity_eff = torch.empty_like(opacity) if opacity_eff is None else opacity_eff
    check(_lib.load().gsplat_filter3d_apply(_p(_f32(scale, "scale")), _p(_f32(opacity, "opacity")),
                                            _p(_f32(filter3d, "filter3d")), N, _p(_f32(scale_eff, "scale_eff")),
                                            _p(_f32(opacity_eff, "opacity_eff")), _stream()))
    return scale_eff, opacity_eff


def filter3d_apply_backward(scale, opacity, filter3d, grad_scale, grad_opacity, rows=None):
    """The filter's chain rule, in place (gsplat_filter3d_apply_backward): grad_scale [M,3] / grad_opacity [M] hold the
    gradients with respect to scale_eff / opacity_eff and leave as those with respect to scale / opacity.  Gradient row j
    belongs to gaussian rows[j] (int32 device tensor; None: j).  The two gradient tensors may be column views of a wider
    row-major buffer (common[:, 4:7], common[:, 3]): only their rows' stride has to be uniform."""
    M = int(grad_opacity.shape[0])
    if grad_scale.dim() != 2 or grad_scale.shape[1] != 3 or grad_scale.shape[0] != M or grad_opacity.dim() != 1:
        raise ValueError("grad_scale must be [M,3] and grad_opacity [M]")
    if M > 1 and grad_scale.stride(1) != 1:
        raise ValueError("the three scale gradients of a row must be adjacent")
    if rows is not None and (rows.dtype != torch.int32 or rows.numel() != M):
        raise ValueError("rows must be an int32 tensor with one entry per gradient row")
    _f32(grad_scale, "grad_scale"), _f32(grad_opacity, "grad_opacity")
    if M == 0:
        return
    check(_lib.load().gsplat_filter3d_apply_backward(
        _p(_f32(scale, "scale")), _p(_f32(opacity, "opacity")), _p(_f32(filter3d, "filter3d")), _p(rows), M,
        ctypes.c_void_p(grad_scale.data_ptr()), int(grad_scale.stride(0)) if M > 1 else 3,
        ctypes.c_void_p(grad_opacity.data_ptr()), int(grad_opacity.stride(0)) if M > 1 else 1, _stream()))

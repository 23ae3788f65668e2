"""Per-view forward/backward on the device-resident context (binding of gsplat_rasterize_image /
gsplat_backward_pass, include/gsplat_hip.h).

Mirrors the two call sites of the reference trainer: ``rasterize_image(...)``
(/root/reference/cuda/raster.cu:12-136, called at cuda/trainer.cu:1350) and the operator
chain of ``TrainerImpl::backward_pass`` (cuda/trainer.cu:941-1012).  All tensors are torch
device tensors; results are zero-copy views into the context's workspace (valid until the
next forward on the same context).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check


class _DevView:
    """Expose a raw device pointer to torch through __cuda_array_interface__ (zero copy)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(int(s) for s in shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2}
        self._owner = owner


def _view(ptr, shape, typestr, owner):
    if ptr is None and int(np.prod(shape)) != 0:
        return None  # an output the library did not produce (render-only context)
    if ptr is None or int(np.prod(shape)) == 0:
        dt = {"<f4": torch.float32, "<i4": torch.int32, "|u1": torch.uint8}[typestr]
        return torch.empty(tuple(shape), dtype=dt, device="cuda")
    return torch.as_tensor(_DevView(ptr, shape, typestr, owner), device="cuda")


_EAGER_VIEWS = bool(int(__import__("os").environ.get("GSPLAT_EAGER_VIEWS", "0")))  # debugging: build every view at once


class _LazyViews(dict):
    """The forward's result: counts are plain entries, every array is turned into a tensor view the first time it is
    asked for.  A view costs ~15 us of host time (torch queries the pointer), sixteen of them per call were most of the
    host's work between the forward's record and the launch of whatever consumes the image -- and a training loop
    reads two of them."""

    def __init__(self, plain, specs, owner):
        super().__init__(plain)
        self._specs, self._owner = specs, owner
        self._derived = {}  # entries computed from the others on first use: name -> f(views) (no closure over self: a
        # cycle would keep the views, and the context they hold, alive until the cyclic collector runs)

    def __missing__(self, key):
        if key in self._derived:
            value = self._derived.pop(key)(self)
        else:
            ptr, shape, typestr = self._specs.pop(key)  # KeyError for unknown names, as a dict
            value = _view(ptr, shape, typestr, self._owner)
        self[key] = value
        return value

    def _all(self):
        for key in list(self._specs) + list(self._derived):
            self[key]
        return self

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._specs or key in self._derived

    def __iter__(self):
        return dict.__iter__(self._all())

    def __len__(self):
        return dict.__len__(self._all())

    def keys(self):
        return dict.keys(self._all())

    def items(self):
        return dict.items(self._all())

    def values(self):
        return dict.values(self._all())


def _alpha(views):
    return 1.0 - views["T"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _map_ptr(t):
    """A per-pixel gradient map ([H,W] float32, contiguous, on the device) as a pointer; None stays NULL."""
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
        raise ValueError("grad_depth / grad_alpha / grad_depth2 must be contiguous [H,W] float32 device tensors")
    return ctypes.c_void_p(t.data_ptr())


def device_params(params, device="cuda"):
    """numpy parameter dict (scene.make_gaussians) -> dict of contiguous float32 device tensors."""
    return {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(device).contiguous()
            for k, v in params.items()}


def device_camera(cam, device="cuda"):
    out = dict(cam)
    out["view"] = torch.as_tensor(np.asarray(cam["view"], np.float32)).to(device)
    out["proj"] = torch.as_tensor(np.asarray(cam["proj"], np.float32)).to(device)
    out["campos_dev"] = torch.as_tensor(np.asarray(cam["campos"], np.float32)).to(device)  # for the exchange step
    return out


class RasterContext:
    """Owns a gsplat_context (persistent HBM workspace sized for max_gaussians / max image)."""

    def __init__(self, max_gaussians, max_width, max_height):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        check(self._lib.gsplat_context_create(ctypes.byref(h), int(max_gaussians), int(max_width), int(max_height)))
        self._h = h
        self._last = self._last_size = None
        self._depth = self._depth_inverse = self._depth_moment = False
        self._filter3d = self._filter3d_fwd = None
        self.max_gaussians, self.max_width, self.max_height = int(max_gaussians), int(max_width), int(max_height)

    def close(self):
        if self._h:
            self._lib.gsplat_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self):
        return int(self._lib.gsplat_context_bytes(self._h))

    STAGES = ("project_cull", "preprocess", "bin_sort", "reserved", "render_forward", "zero_grad_rows",
              "render_backward", "preprocess_backward")

    def set_binning_route(self, route):
        """0 automatic, 1 LDS counting sort + per-tile depth sort, 2 stable radix sorts (identical results)."""
        check(self._lib.gsplat_context_set_binning_route(self._h, int(route)))

    def set_segment_options(self, poll_budget=-1, thin_layer_blocks=-1, gate=-1.0):
        """Testing / tuning hook of the forward's long-list segments (gsplat_context_set_segment_options); results do not
        depend on it."""
        check(self._lib.gsplat_context_set_segment_options(self._h, int(poll_budget), int(thin_layer_blocks), float(gate)))

    def set_render_only(self, enabled):
        """Serving mode: forwards skip the outputs only a backward reads (see gsplat_context_set_render_only)."""
        check(self._lib.gsplat_context_set_render_only(self._h, int(bool(enabled))))

    def set_lean_forward(self, enabled):
        """Training through backward_pass: the forward stops storing Sigma, J, conic and the SH colour (the fused backward
        recomputes what it needs); those four views are then absent from the forward's result."""
        check(self._lib.gsplat_context_set_lean_forward(self._h, int(bool(enabled))))

    def set_depth(self, enabled, inverse=False, moment=False):
        """Depth mode (gsplat_context_set_depth): every later forward also composites the per-pixel depth
        sum alpha T z (the result's "depth" view), and backward_pass / backward_render / backward_pass_adam accept
        grad_depth / grad_alpha.  Options (gsplat_context_set_depth_mode): inverse -- the composited value is s = 1/z
        instead of z; moment -- the forward also composites sum alpha T s^2 (the result's "depth2" view) and the backwards
        accept grad_depth2.  The moment option has no absgrad form."""
        if enabled and (inverse or moment):
            check(self._lib.gsplat_context_set_depth_mode(self._h, int(bool(inverse)), int(bool(moment))))
        else:
            check(self._lib.gsplat_context_set_depth(self._h, int(bool(enabled))))
        self._depth = bool(enabled)
        self._depth_inverse = bool(enabled and inverse)
        self._depth_moment = bool(enabled and moment)

    def set_absgrad(self, enabled):
        """Absgrad mode (gsplat_context_set_absgrad): from the next backward_render / backward_pass on, the compositing
        backward also sums every pixel's share of dL/d uv by absolute value, and the densification statistics (uv_norm
        of the split form, uv_grad_accum of the fused Adam forms) are the norm of those sums instead of |grad_uv|.  Every
        gradient is unchanged."""
        check(self._lib.gsplat_context_set_absgrad(self._h, int(bool(enabled))))

    def set_antialiased(self, enabled):
        """Anti-aliased mode (gsplat_context_set_antialiased): from the next forward on, every gaussian composites with
        the opacity sigmoid(logit) * rho, rho = sqrt(det(cov) / det(cov + 0.3 I)) -- the compensation for the 0.3 px blur
        of the projected covariance -- and backward_pass / backward_gaussians (whole, range, split) return the gradients
        of that image.  The Adam-inside and camera backwards and the two-kernel forward refuse the mode."""
        check(self._lib.gsplat_context_set_antialiased(self._h, int(bool(enabled))))

    def set_filter3d(self, filter3d):
        """3D smoothing filter (gsplat_context_set_filter3d): filter3d is the [N] float32 device tensor of
        ops.compute_filter3d, in global gaussian order, or None to switch the mode off.  From the next forward on every
        gaussian is rasterized with the scale and opacity of ops.filter3d_apply, and backward_pass / backward_gaussians
        (whole, range, split, camera) return the gradients with respect to the RAW scale and opacity.  The Adam-inside
        backwards refuse the mode.  The context keeps the tensor alive for as long as a forward or backward may read it."""
        if filter3d is not None:
            if (not isinstance(filter3d, torch.Tensor) or filter3d.dtype != torch.float32 or not filter3d.is_cuda
                    or not filter3d.is_contiguous() or filter3d.dim() != 1):
                raise ValueError("filter3d must be a contiguous [N] float32 device tensor or None")
        check(self._lib.gsplat_context_set_filter3d(self._h, _ptr(filter3d)))
        self._filter3d = filter3d if filter3d is not None and filter3d.numel() else None

    def absgrad_uv(self):
        """abs_uv [M,2] of the last compositing backward (compacted order): (sum_p |du_p|, sum_p |dv_p|) over the pixels'
        shares of grad_uv.  Valid until the next forward; an error unless that backward ran in absgrad mode
        (gsplat_context_absgrad_uv)."""
        M = self._last[1] if self._last else 0
        out = torch.empty(M, 2, dtype=torch.float32, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_context_absgrad_uv(self._h, _ptr(out), st))
        return out

    def accumulate_contributions(self, weight_sum=None, weight_max=None, pixels=None):
        """Per-gaussian blend-weight statistics of the last forward, accumulated INTO the given [N] device tensors in
        global gaussian order (gsplat_context_accumulate_contributions): weight_sum (float32) += sum over the pixels of
        alpha * T, weight_max (float32) = max with the largest alpha * T, pixels (int32) += the number of pixels that
        composited the gaussian.  Rows of culled gaussians are untouched, so the arrays can gather a camera set: clear
        them once, call after each view's forward.  weight_max and pixels are bit-reproducible, weight_sum is a float
        atomic sum.  Any of the three may be None, not all.  Works after any forward (render-only included) and after
        its backward."""
        for name, t, dt in (("weight_sum", weight_sum, torch.float32), ("weight_max", weight_max, torch.float32),
                            ("pixels", pixels, torch.int32)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda
                                  or not t.is_contiguous() or t.dim() != 1):
                raise ValueError("%s must be a contiguous [N] %s device tensor or None" % (name, str(dt).split(".")[1]))
        given = [t for t in (weight_sum, weight_max, pixels) if t is not None]
        if any(t.numel() != given[0].numel() for t in given):
            raise ValueError("weight_sum, weight_max and pixels must have the same length")
        n = given[0].numel() if given else (self._last[0] if self._last else 0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_context_accumulate_contributions(self._h, int(n), _ptr(weight_sum), _ptr(weight_max),
                                                                _ptr(pixels), st))

    def median_depth(self, threshold=0.5, out=None, index=None):
        """The median (quantile) depth map of the last forward (gsplat_context_median_depth) -> [H,W] float32: per pixel
        the camera-space z of the first composited gaussian behind which the transmittance is <= threshold (0.5: the
        median), 0 where it never gets there.  Always z, whatever the context's depth mode; depth mode is not needed.
        `out`: an [H,W] float32 device tensor to write into, else a new one; returned.  `index`: an [H,W] int32 device
        tensor that receives that gaussian's position in its tile's list, -1 where there is none.  No atomics: the
        same bits in every run.  Works after any forward (render-only included), before or after its backward."""
        import math
        threshold = float(threshold)
        if not (math.isfinite(threshold) and 0.0 < threshold < 1.0):
            raise ValueError("threshold must be finite and in (0, 1), not %r" % threshold)
        H, W = self._feature_map_shape()
        for name, t, dt in (("out", out, torch.float32), ("index", index, torch.int32)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda
                                  or not t.is_contiguous() or tuple(t.shape) != (H, W)):
                raise ValueError("%s must be a contiguous [%d,%d] %s device tensor or None"
                                 % (name, H, W, str(dt).split(".")[1]))
        if out is None:
            out = torch.empty(H, W, dtype=torch.float32, device="cuda")
        n = self._last[0] if self._last else 0
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_context_median_depth(self._h, int(n), threshold, _ptr(out), _ptr(index), st))
        return out

    @staticmethod
    def _dense(name, t, dims):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous()
                or t.dim() != dims):
            raise ValueError("%s must be a contiguous %s float32 device tensor" % (name, "[N,C]" if dims == 2 else "[H,W,C]"))
        return t

    def render_features(self, features, out=None):
        """The caller's per-gaussian channels through the last forward (gsplat_context_render_features): features [N,C]
        float32 in global gaussian order -> the [H,W,C] map out[p, c] = sum over the gaussians the forward composited
        at p of alpha * T * features[j, c], in the forward's own weights (no background term: fwd["T"] is what is left
        of the pixel).  `out`: an [H,W,C] tensor to write into, else a new one; returned.  1 <= C <= 512.  Every pixel is
        summed in list order without atomics: the map is bit-reproducible, and with the forward's colours it is the
        forward's image at background 0.  Works after any forward (render-only included), before or after its backward.
        The gradient of a loss on the map with respect to `features` is lift_features of the loss's gradient map; its
        gradient with respect to opacity, conic and position is features_backward, behind backward_render."""
        self._dense("features", features, 2)
        N, C = int(features.shape[0]), int(features.shape[1])
        if not 1 <= C <= 512:
            raise ValueError("features must have 1 .. 512 channels, not %d" % C)
        H, W = self._feature_map_shape()
        if out is None:
            out = torch.empty(H, W, C, dtype=torch.float32, device=features.device)
        elif tuple(self._dense("out", out, 3).shape) != (H, W, C):
            raise ValueError("out must be [%d,%d,%d], not %s" % (H, W, C, list(out.shape)))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_context_render_features(self._h, N, C, _ptr(features), _ptr(out), st))
        return out

    def lift_features(self, map, out):
        """render_features' adjoint (gsplat_context_lift_features): map [H,W,C] float32 of the last forward's size ->
        out[j, c] += sum over the pixels that composited gaussian j of alpha * T * map[p, c]; out is [N,C] float32 in
        global gaussian order, accumulated INTO and returned.  Rows of culled gaussians, and of gaussians no pixel
        composited, are untouched, so one array gathers a camera set: clear it once, call after each view's forward.
        With a map of ones this is accumulate_contributions' weight_sum; the quotient of the two is the weighted mean
        of what a gaussian's pixels said (label lifting).  The sums are float atomics: order-dependent in their last
        bits."""
        self._dense("map", map, 3)
        self._dense("out", out, 2)
        N, C = int(out.shape[0]), int(out.shape[1])
        if not 1 <= C <= 512:
            raise ValueError("out must have 1 .. 512 channels, not %d" % C)
        H, W = self._feature_map_shape()
        if tuple(map.shape) != (H, W, C):
            raise ValueError("map must be [%d,%d,%d], not %s" % (H, W, C, list(map.shape)))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_context_lift_features(self._h, N, C, _ptr(map), _ptr(out), st))
        return out

    def features_backward(self, features, grad_map):
        """The feature map's gradient with respect to the geometry (gsplat_context_features_backward): features [N,C]
        float32 in global gaussian order, grad_map [H,W,C] = dL/d render_features(features).  Call it between
        backward_render of the last forward and the per-gaussian call (backward_gaussians, _range, _split, _adam,
        _camera): the loss's d/d opacity logit, conic and uv are ADDED to the gradient rows the compositing backward left,
        so the per-gaussian call returns the gradient of the total down to xyz, opacity, scale and quaternion (for a
        feature loss alone: backward_render with a zero grad_image).  Calling it twice adds twice.  The absgrad
        statistic does not include the feature term, the signed grad_uv does.  The gradient with respect to `features`
        is lift_features(grad_map)."""
        self._dense("features", features, 2)
        self._dense("grad_map", grad_map, 3)
        N, C = int(features.shape[0]), int(features.shape[1])
        if not 1 <= C <= 512:
            raise ValueError("features must have 1 .. 512 channels, not %d" % C)
        H, W = self._feature_map_shape()
        if tuple(grad_map.shape) != (H, W, C):
            raise ValueError("grad_map must be [%d,%d,%d], not %s" % (H, W, C, list(grad_map.shape)))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_context_features_backward(self._h, N, C, _ptr(features), _ptr(grad_map), st))

    def _feature_map_shape(self):
        if self._last_size is None:  # (the library's own answer to a call before the first forward)
            raise _lib.GsplatError(-3, "no forward pass recorded in this context")
        return self._last_size

    def set_preprocess_split(self, mode):
        """How the per-gaussian forward is launched: 0 (default) the single fused kernel, 1 SH colour then geometry on the
        caller's stream, 2 the two side by side on two streams (gsplat_context_set_preprocess_split); every output is
        bit-identical in all modes, 1 and 2 measure slower (profiles/r06_ab_preprocess_split.txt)."""
        check(self._lib.gsplat_context_set_preprocess_split(self._h, int(mode)))

    def set_compact_lists(self, enabled):
        """Compact lists for the compositing backward (gsplat_context_set_compact_lists; on by default): from the next
        forward on, the backward walks only the tile-list entries that can touch a pixel of their tile.  Forward outputs
        are the same bits either way, gradients the same sums in another order."""
        check(self._lib.gsplat_context_set_compact_lists(self._h, int(bool(enabled))))

    def set_dir_sums(self, enabled):
        """The SH direction sums (gsplat_context_set_dir_sums; on by default): from the next forward on, the fused per-gaussian
        forward leaves the nine sums over each SH row that the backward needs, and the plain per-gaussian backward and
        backward_gaussians_adam with mode 1 read those instead of the rows (the other forms read the rows: a context that
        only runs those should switch this off -- the sums cost the forward about 10 us per 1e6 gaussians).  Forward outputs and gradients are the same bits either way."""
        check(self._lib.gsplat_context_set_dir_sums(self._h, int(bool(enabled))))

    def counters(self):
        """What the context's forwards did so far (gsplat_context_get_counters).  useful_entries is summed on the device's
        results when asked for: this call waits for the device."""
        v = (ctypes.c_longlong * 14)()
        self._lib.gsplat_context_get_counters(self._h, v, 14)
        return dict(forwards=int(v[0]), tail_redone=int(v[1]), compact_walks=int(v[2]), instance_growths=int(v[3]),
                    ordered_backwards=int(v[4]), segmented_backwards=int(v[5]), segmented_forwards=int(v[6]),
                    longest_chain=int(v[7]), chain_sum=int(v[8]), segment_fallbacks=int(v[9]),
                    compact_list_backwards=int(v[10]), useful_entries=int(v[11]),
                    dir_sums_backwards=int(v[12]), dir_sums_fallbacks=int(v[13]))

    def set_timing(self, enabled, stages=None):
        """Per-stage HIP-event timing on / off; `stages`: names from STAGES to time only those (each timed stage costs
        two event records per call)."""
        if enabled and stages is not None:
            mask = 0
            for name in stages:
                mask |= 1 << self.STAGES.index(name)
            check(self._lib.gsplat_context_set_timing_stages(self._h, mask))
        else:
            check(self._lib.gsplat_context_set_timing(self._h, int(bool(enabled))))

    def get_timing(self):
        """{stage: (mean ms per launch, launches)} since timing was enabled (HIP events on the launch stream)."""
        ms = (ctypes.c_double * 8)()
        cnt = (ctypes.c_longlong * 8)()
        self._lib.gsplat_context_get_timing(self._h, ms, cnt, 8)
        return {s: ((ms[i] / cnt[i]) if cnt[i] else 0.0, int(cnt[i])) for i, s in enumerate(self.STAGES)}

    @staticmethod
    def _structs(params, cam, l_max):
        g = _lib.Gaussians()
        g.num_gaussians = int(params["xyz"].shape[0])
        g.xyz, g.rgb, g.opacity = _ptr(params["xyz"]), _ptr(params["rgb"]), _ptr(params["opacity"])
        g.scale, g.quaternion = _ptr(params["scale"]), _ptr(params["quaternion"])
        g.sh = _ptr(params["sh"]) if l_max > 0 else None
        c = _lib.Camera()
        c.width, c.height = int(cam["width"]), int(cam["height"])
        c.focal_x, c.focal_y = float(cam["fx"]), float(cam["fy"])
        for k in range(3):
            c.campos[k] = float(cam["campos"][k])
        c.view, c.proj = _ptr(cam["view"]), _ptr(cam["proj"])
        return g, c

    def rasterize_image(self, params, cam, config, bg_color, l_max):
        """params: dict of device tensors (xyz rgb sh opacity scale quaternion); sh must be stored with the
        current band's stride, [N,(l_max+1)^2-1,3] (cuda_data.cuh layout).  Returns a dict of views."""
        g, c = self._structs(params, cam, l_max)
        if self._filter3d is not None and self._filter3d.numel() != g.num_gaussians:
            raise ValueError("the 3D filter has %d rows for %d gaussians" % (self._filter3d.numel(), g.num_gaussians))
        self._filter3d_fwd = self._filter3d  # the backwards of this forward read the same array
        if l_max > 0:
            want = ((l_max + 1) ** 2 - 1) * 3
            if params["sh"].numel() != g.num_gaussians * want:
                raise ValueError("sh must be packed at the current band's stride")
        cfg = _lib.RasterConfig(float(config["near_thresh"]), float(config["mh_dist"]), int(config["cull_mask_padding"]))
        fv = _lib.ForwardView()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_rasterize_image(self._h, ctypes.byref(g), ctypes.byref(c), ctypes.byref(cfg),
                                               float(bg_color), int(l_max), ctypes.byref(fv), st))
        N, M, S = g.num_gaussians, int(fv.num_culled), int(fv.num_splats)
        W, H = c.width, c.height
        T = ((W + 15) // 16) * ((H + 15) // 16)
        out = _LazyViews(
            dict(num_culled=M, num_pairs=int(fv.num_pairs), num_splats=S),
            dict(mask=(fv.mask, (N,), "|u1"), uv_all=(fv.uv, (N, 2), "<f4"), xyz_c_all=(fv.xyz_c, (N, 3), "<f4"),
                 compact_to_global=(fv.compact_to_global, (M,), "<i4"), sigma=(fv.sigma, (M, 6), "<f4"),
                 conic=(fv.conic, (M, 3), "<f4"), J=(fv.J, (M, 6), "<f4"), rgb=(fv.precomputed_rgb, (M, 3), "<f4"),
                 radius=(fv.radius, (M, 4), "<f4"), uv=(fv.uv_selected, (M, 2), "<f4"),
                 xyz_c=(fv.xyz_c_selected, (M, 3), "<f4"), sorted=(fv.sorted_gaussians, (S,), "<i4"),
                 ranges=(fv.splat_start_end_idx_by_tile_idx, (T + 1,), "<i4"), image=(fv.image, (H, W, 3), "<f4"),
                 T=(fv.weight_per_pixel, (H, W), "<f4"), n=(fv.splats_per_pixel, (H, W), "<i4")), self)
        if self._depth:
            dp = ctypes.c_void_p()
            check(self._lib.gsplat_context_depth_map(self._h, ctypes.byref(dp)))
            out._specs["depth"] = (dp.value, (H, W), "<f4")
            if self._depth_moment:
                qp = ctypes.c_void_p()
                check(self._lib.gsplat_context_depth_moment_map(self._h, ctypes.byref(qp)))
                out._specs["depth2"] = (qp.value, (H, W), "<f4")
        out._derived["alpha"] = _alpha  # the opacity map: 1 - the final transmittance
        self._last = (g.num_gaussians, M, l_max)
        self._last_size = (H, W)
        return out._all() if _EAGER_VIEWS else out

    def alloc_gradients(self, M, l_max, intermediates=False, device="cuda", factored_sh=False):
        """Leaf gradients in compacted order; intermediates=True adds the reference's six intermediate gradient arrays
        (cuda_data.cuh:28-36), an iterable of their names only those (the kernel skips the ones that are absent).
        factored_sh: no `sh` array -- the backward skips the SH gradients and AdamOptimizer.step rebuilds them from
        `precompute_rgb` (added) and the viewing direction (gsplat_optimizer_step_sh_factored)."""
        n_rest = (l_max + 1) ** 2 - 1
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
        g = dict(xyz=z(M, 3), rgb=z(M, 3), sh=z(M, n_rest, 3), opacity=z(M), scale=z(M, 3), quaternion=z(M, 4))
        shapes = dict(conic=(M, 3), uv=(M, 2), J=(M, 6), sigma=(M, 6), xyz_c=(M, 3), precompute_rgb=(M, 3))
        wanted = shapes if intermediates is True else tuple(intermediates or ())  # True: all six; or an iterable of names
        if factored_sh and l_max > 0:
            g["sh"] = None
            if "precompute_rgb" not in wanted:
                wanted = tuple(wanted) + ("precompute_rgb",)
        g.update({k: z(*shapes[k]) for k in wanted})
        return g

    @staticmethod
    def _grad_struct(grads):
        gs = _lib.Gradients()
        gs.grad_xyz, gs.grad_rgb, gs.grad_sh = _ptr(grads["xyz"]), _ptr(grads.get("rgb")), _ptr(grads.get("sh"))
        gs.grad_opacity, gs.grad_scale = _ptr(grads.get("opacity")), _ptr(grads.get("scale"))
        gs.grad_quaternion = _ptr(grads.get("quaternion"))
        for k in ("conic", "uv", "J", "sigma", "xyz_c", "precompute_rgb"):
            setattr(gs, "grad_" + k, _ptr(grads.get(k)))
        return gs

    def backward_pass(self, params, cam, grad_image, bg_color, l_max, grads, grad_depth=None, grad_alpha=None,
                      grad_depth2=None, feature_grads=None):
        """grads: dict from alloc_gradients (compacted order); every leaf gradient is overwritten.  grad_depth /
        grad_alpha ([H,W], depth mode, either may be None): dL/d of the forward's "depth" / "alpha" views, added to the
        image's gradient (gsplat_backward_pass_depth).  grad_depth2: dL/d of the "depth2" view (the moment option;
        gsplat_backward_pass_depth2).  feature_grads: (features [N,C], grad_map [H,W,C]) of a loss on
        render_features(features) -- its gradient with respect to the geometry is added (backward_render ->
        features_backward -> backward_gaussians); None: the calls made are exactly the ones above."""
        if feature_grads is not None:
            features, grad_map = feature_grads
            self.backward_render(grad_image, bg_color, grad_depth=grad_depth, grad_alpha=grad_alpha, grad_depth2=grad_depth2)
            self.features_backward(features, grad_map)
            return self.backward_gaussians(params, cam, l_max, grads)
        g, c = self._structs(params, cam, l_max)
        gs = self._grad_struct(grads)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if grad_depth2 is not None:
            check(self._lib.gsplat_backward_pass_depth2(self._h, ctypes.byref(g), ctypes.byref(c), _ptr(grad_image),
                                                        _map_ptr(grad_depth), _map_ptr(grad_alpha), _map_ptr(grad_depth2),
                                                        float(bg_color), int(l_max), ctypes.byref(gs), st))
        elif grad_depth is None and grad_alpha is None:
            check(self._lib.gsplat_backward_pass(self._h, ctypes.byref(g), ctypes.byref(c), _ptr(grad_image),
                                                 float(bg_color), int(l_max), ctypes.byref(gs), st))
        else:
            check(self._lib.gsplat_backward_pass_depth(self._h, ctypes.byref(g), ctypes.byref(c), _ptr(grad_image),
                                                       _map_ptr(grad_depth), _map_ptr(grad_alpha), float(bg_color),
                                                       int(l_max), ctypes.byref(gs), st))
        return grads

    def backward_pass_adam(self, params, cam, grad_image, bg_color, l_max, adam, grads=None, grad_depth=None,
                           grad_alpha=None, grad_depth2=None, feature_grads=None):
        """backward_pass with the optimizer step inside (single-GPU training): the compositing backward, then ONE
        per-gaussian kernel that differentiates every visible gaussian and applies the masked Adam step to its rows of the
        parameters (`params`, in place), the moments and the densification statistics (gsplat_backward_gaussians_adam).
        adam: an _lib.AdamFused (AdamOptimizer.fused_state); grads: optional gradient arrays to fill as well;
        grad_depth / grad_alpha / grad_depth2 / feature_grads: as in backward_pass."""
        self.backward_render(grad_image, bg_color, grad_depth=grad_depth, grad_alpha=grad_alpha, grad_depth2=grad_depth2)
        if feature_grads is not None:
            self.features_backward(*feature_grads)
        self.backward_gaussians_adam(params, cam, l_max, adam, grads)

    def backward_gaussians_adam(self, params, cam, l_max, adam, grads=None):
        """Second half of backward_pass_adam: the per-gaussian chain with the optimizer step inside."""
        g, c = self._structs(params, cam, l_max)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        gs = ctypes.byref(self._grad_struct(grads)) if grads is not None else None
        check(self._lib.gsplat_backward_gaussians_adam(self._h, ctypes.byref(g), ctypes.byref(c), int(l_max),
                                                       ctypes.byref(adam), gs, st))

    def backward_render(self, grad_image, bg_color, rgb_global=None, common=None, uv_norm=None, grad_depth=None,
                        grad_alpha=None, grad_depth2=None):
        """First half of backward_pass: compositing backward; optionally this view's g_rgb in global order [N,3].
        common [N,12] (and uv_norm [N]): the split exchange's rows -- the rows of the gaussians this view culled are
        cleared here, the others are written by backward_gaussians_split (gsplat_backward_render_split).
        grad_depth / grad_alpha / grad_depth2: as in backward_pass; whichever per-gaussian call follows takes the depth
        term along (gsplat_backward_render_depth, gsplat_backward_render_depth2)."""
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if grad_depth2 is not None:
            check(self._lib.gsplat_backward_render_depth2(self._h, _ptr(grad_image), _map_ptr(grad_depth),
                                                          _map_ptr(grad_alpha), _map_ptr(grad_depth2), float(bg_color),
                                                          _ptr(rgb_global), _ptr(common), _ptr(uv_norm), st))
        elif grad_depth is None and grad_alpha is None:
            check(self._lib.gsplat_backward_render_split(self._h, _ptr(grad_image), float(bg_color), _ptr(rgb_global),
                                                         _ptr(common), _ptr(uv_norm), st))
        else:
            check(self._lib.gsplat_backward_render_depth(self._h, _ptr(grad_image), _map_ptr(grad_depth),
                                                         _map_ptr(grad_alpha), float(bg_color), _ptr(rgb_global),
                                                         _ptr(common), _ptr(uv_norm), st))

    def backward_gaussians_split(self, params, cam, l_max, common, uv_norm=None, first=0, end=None):
        """Second half of backward_pass for a view-sharded step: the twelve direction-independent gradient columns go
        straight into common[N,12] at the gaussians' global indices (|grad_uv| into uv_norm[N]); no compacted gradient
        array is written, the colour gradients are rebuilt by the optimizer from the gathered g_rgb."""
        g, c = self._structs(params, cam, l_max)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_backward_gaussians_split(self._h, ctypes.byref(g), ctypes.byref(c), int(l_max), _ptr(common),
                                                        _ptr(uv_norm), int(first), int(g.num_gaussians if end is None else end), st))

    def backward_gaussians(self, params, cam, l_max, grads):
        """Second half of backward_pass: the per-gaussian operator chain."""
        g, c = self._structs(params, cam, l_max)
        gs = self._grad_struct(grads)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_backward_gaussians(self._h, ctypes.byref(g), ctypes.byref(c), int(l_max), ctypes.byref(gs), st))
        return grads

    def backward_pass_camera(self, params, cam, grad_image, bg_color, l_max, grads=None, grad_depth=None, grad_alpha=None):
        """backward_pass that also returns dL/d view[0..11] as grad_view [3,4] and dL/d campos as grad_campos [3] (device
        float32 tensors; view and campos taken as two independent inputs -- 3dgs_amd/pose.py turns them into the pose's
        gradient).  grads=None: only the camera gradient (pose refinement, localisation against frozen gaussians);
        otherwise filled bit-identically to backward_pass.  Returns (grads, grad_view, grad_campos)
        (gsplat_backward_pass_camera)."""
        g, c = self._structs(params, cam, l_max)
        gv, gc = self._camera_grads()
        gs = ctypes.byref(self._grad_struct(grads)) if grads is not None else None
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_backward_pass_camera(self._h, ctypes.byref(g), ctypes.byref(c), _ptr(grad_image),
                                                    _map_ptr(grad_depth), _map_ptr(grad_alpha), float(bg_color),
                                                    int(l_max), gs, _ptr(gv), _ptr(gc), st))
        return grads, gv, gc

    def backward_gaussians_camera(self, params, cam, l_max, grads=None):
        """backward_pass_camera's second half, after backward_render (gsplat_backward_gaussians_camera)."""
        g, c = self._structs(params, cam, l_max)
        gv, gc = self._camera_grads()
        gs = ctypes.byref(self._grad_struct(grads)) if grads is not None else None
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_backward_gaussians_camera(self._h, ctypes.byref(g), ctypes.byref(c), int(l_max), gs,
                                                         _ptr(gv), _ptr(gc), st))
        return grads, gv, gc

    @staticmethod
    def _camera_grads():
        return (torch.empty(3, 4, dtype=torch.float32, device="cuda"), torch.empty(3, dtype=torch.float32, device="cuda"))

    def backward_gaussians_range(self, params, cam, l_max, grads, first, end):
        """The per-gaussian chain for the gaussians with global index in [first, end) (chunked exchange)."""
        g, c = self._structs(params, cam, l_max)
        gs = self._grad_struct(grads)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_backward_gaussians_range(self._h, ctypes.byref(g), ctypes.byref(c), int(l_max),
                                                        ctypes.byref(gs), int(first), int(end), st))
        return grads

    def pack_gradients_global(self, grads, l_max, num_gaussians, packed):
        gs = self._grad_struct(grads)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.gsplat_pack_gradients_global(self._h, ctypes.byref(gs), int(l_max), int(num_gaussians),
                                                     _ptr(packed), st))
        return packed


def pack_gradients_factored(ctx, grads, num_gaussians, rank, world, factored):
    gs = RasterContext._grad_struct(grads)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_pack_gradients_factored(ctx._h, ctypes.byref(gs), int(num_gaussians), int(rank), int(world),
                                                     _ptr(factored), st))
    return factored


def unpack_gradients_factored(xyz, campos_all, factored, l_max, num_gaussians, world, packed):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_unpack_gradients_factored(_ptr(xyz), _ptr(campos_all), _ptr(factored), int(l_max),
                                                       int(num_gaussians), int(world), _ptr(packed), st))
    return packed


def pack_gradients_split(ctx, grads, num_gaussians, common, rgb):
    gs = RasterContext._grad_struct(grads)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_pack_gradients_split(ctx._h, ctypes.byref(gs), int(num_gaussians), _ptr(common), _ptr(rgb), st))


def pack_gradients_split_range(ctx, grads, num_gaussians, first, end, common, rgb=None):
    gs = RasterContext._grad_struct(grads)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_pack_gradients_split_range(ctx._h, ctypes.byref(gs), int(num_gaussians), int(first), int(end),
                                                        _ptr(common), _ptr(rgb), st))


def pack_uv_grad_norm(ctx, grads, num_gaussians, uv_norm):
    """This view's |grad_uv| in global gaussian order (0 where culled): gsplat_pack_uv_grad_norm."""
    gs = RasterContext._grad_struct(grads)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_pack_uv_grad_norm(ctx._h, ctypes.byref(gs), int(num_gaussians), _ptr(uv_norm), st))
    return uv_norm


def pack_absgrad_norm(ctx, num_gaussians, uv_norm):
    """This view's absnorm = |(sum_p |du_p|, sum_p |dv_p|)| in global gaussian order (0 where culled), after a compositing
    backward in absgrad mode: gsplat_pack_absgrad_norm, the counterpart of pack_uv_grad_norm."""
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_pack_absgrad_norm(ctx._h, int(num_gaussians), _ptr(uv_norm), st))
    return uv_norm


def unpack_gradients_split(xyz, common, rgb_all, rank_stride, l_max, num_gaussians, world, packed):
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(_lib.load().gsplat_unpack_gradients_split(_ptr(xyz), _ptr(common), _ptr(rgb_all), int(rank_stride), int(l_max),
                                                    int(num_gaussians), int(world), _ptr(packed), st))
    return packed


def factored_gradient_width(world):
    return int(_lib.load().gsplat_factored_gradient_width(int(world)))


def packed_gradient_width(l_max):
    return int(_lib.load().gsplat_packed_gradient_width(int(l_max)))

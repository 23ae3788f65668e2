"""Host-side mirror of the reference's training loop (TrainerImpl, cuda/trainer.cu) -- SURVEY.md section 8f, row f4.

Only the SCHEDULE lives here (what runs at which iteration, config thresholds); every data-parallel step is a HIP
kernel behind the C ABI: rasterize / loss / backward / masked Adam (rows a-f2) and, for the density policy, the masks,
clone / split, compaction, SH band re-layout, Morton codes and the row gather of gs_density.hip (config key mcmc: its
sampling, relocation, noise and regulariser kernels).  torch is used for device memory, for the key sort of the Morton
re-order and for the row copies of an MCMC refinement step.  There is no CPU fallback.

Parity note: the reference's density control is not reproducible (cuRAND seeded from time(NULL), std::random_device for
the view order), so this loop is judged statistically (PSNR, gaussian counts), not bit for bit; with a fixed seed it is
itself deterministic.
"""
import math
import os

import numpy as np
import torch

from . import ops, raster
from .dist import TorchComm, ViewShardedStep
from .optimizer import B1, B2, EPS, AdamOptimizer, DEFAULT_LR
from .rows import MOMENT, PARAM, STAT, RowTable

DISTORTION_WEIGHT = 10.0  # the default of config key distortion_weight (README, "Depth regularisers")
NORMAL_PRIOR_WEIGHT = 0.2   # the defaults of config keys normal_prior_weight and normal_smooth_weight: README, "Normal
NORMAL_SMOOTH_WEIGHT = 0.2  # maps from rendered depth", has the numbers they come from

# config/base.yaml of the reference: the keys the loop reads
DEFAULT_CONFIG = dict(
    DEFAULT_LR, near_thresh=0.3, mh_dist=3.0, cull_mask_padding=100, ssim_frac=0.2, use_background=True,
    use_background_end=2000, reset_opacity_interval=3000, reset_opacity_value=0.05, reset_opacity_start=1050,
    reset_opacity_end=5000, max_sh_band=3, add_sh_band_interval=1000, use_split=True, use_clone=True, use_delete=True,
    adaptive_control_start=500, adaptive_control_end=5000, adaptive_control_interval=100, max_gaussians=4250000,
    delete_opacity_threshold=0.02, uv_grad_threshold=0.0002, split_scale_factor=1.6,
    # absgrad: uv_grad_accum sums, per view, the norm of the ABSOLUTE sums of the pixels' shares of grad_uv instead of
    # |grad_uv| (RasterContext.set_absgrad); uv_grad_threshold is compared as given and has to be raised with it (README)
    absgrad=False,
    # antialiased: every gaussian composites with sigmoid(opacity) * rho, the opacity compensation for the 0.3 px blur of
    # its projected covariance (RasterContext.set_antialiased), in training and in evaluate(); the optimizer step then
    # runs behind the backward (the GSPLAT_FUSED_ADAM=0 choreography), which has no Adam-inside form in the mode
    antialiased=False,
    # filter3d: the 3D smoothing filter, the other half of Mip-Splatting (RasterContext.set_filter3d): every gaussian is
    # rasterized as Sigma + f^2 I with its opacity scaled by sqrt(det Sigma / det(Sigma + f^2 I)), f = sqrt(0.2) * the
    # smallest depth / focal length over the training views that see it (closer than filter3d_near: not seen), in
    # training and in evaluate().  f is recomputed every filter3d_interval iterations and whenever the gaussian set or
    # its order changes; the optimizer step runs behind the backward, as with antialiased
    filter3d=False, filter3d_interval=100, filter3d_near=0.2,
    # prune_contribution: every prune_contribution_interval iterations from adaptive_control_end on (nothing regrows then
    # and the last opacity reset is past), remove the gaussians that no pixel of any training view composites or whose
    # largest blend weight alpha * T over all of them stays below prune_contribution_threshold
    # (Trainer.prune_by_contribution; RasterContext.accumulate_contributions)
    prune_contribution=False, prune_contribution_threshold=0.01, prune_contribution_interval=1000,
    # mcmc: the densification of "3D Gaussian Splatting as Markov Chain Monte Carlo" (gsplat's MCMCStrategy) in place of
    # clone / split / prune and the opacity reset: at the adaptive_control cadence the gaussians at or below
    # mcmc_min_opacity are moved onto live ones drawn by opacity and the set grows by mcmc_grow_factor up to exactly
    # max_gaussians (Trainer.mcmc_relocate, mcmc_grow); every iteration adds opacity-gated noise of the gaussian's own
    # shape to the positions (scaled by mcmc_noise_lr * the position learning rate) and the gradient of
    # mcmc_opacity_reg * mean sigmoid(opacity) + mcmc_scale_reg * mean exp(scale) to the rows the view saw.  One rank
    # only; the optimizer step runs behind the backward, as with antialiased
    mcmc=False, mcmc_min_opacity=0.005, mcmc_noise_lr=5e5, mcmc_grow_factor=1.05, mcmc_opacity_reg=0.01,
    mcmc_scale_reg=0.01,
    # distortion: from iteration distortion_start on (2DGS: 3000) every step adds distortion_weight x the mean over the
    # pixels of sum_{j<i} w_i w_j (s_i - s_j)^2, the Mip-NeRF 360 distortion loss (ops.distortion_loss), with s = 1/z when
    # distortion_inverse (the default: in raw z an unbounded capture's loss is its far content's) and s = z otherwise.
    # distortion_weight: README, "Depth regularisers", has the numbers the default comes from.
    # depth_prior: a view given as (camera, image, target) -- target an [H,W] float32 device tensor of inverse depth, <= 0
    # where there is no data -- also adds w(it) x the mean of |depth - target| over the target's pixels
    # (ops.depth_prior_loss), w decaying exponentially from depth_prior_weight_init to depth_prior_weight_final over
    # num_iters like the position learning rate (Inria's depth regularisation); views without a target skip the term.
    # With either key the context renders depth (RasterContext.set_depth, inverse as distortion_inverse, the second
    # moment only with distortion).  One rank only; distortion has no absgrad form.
    distortion=False, distortion_weight=DISTORTION_WEIGHT, distortion_start=3000, distortion_inverse=True,
    depth_prior=False, depth_prior_weight_init=1.0, depth_prior_weight_final=0.01,
    # normal_prior / normal_smooth: from iteration normal_start on every step derives the normal map of the rendered depth
    # (ops.depth_to_normal: central differences of the back-projected expected depth; no normal where the opacity of a
    # pixel or of one of its four neighbours is below normal_alpha_min) and adds
    #   normal_prior:  normal_prior_weight x the mean of 1 - n . prior / |prior| for a view given as (camera, image, depth
    #                  target or None, prior) -- prior an [H,W,3] float32 device tensor of camera-space normals facing the
    #                  camera, zero where there is no data (ops.normal_prior_loss); views without one skip the term;
    #   normal_smooth: normal_smooth_weight x the mean over adjacent pixel pairs of exp(-normal_edge_scale x the mean
    #                  absolute colour difference of the ground truth) x |n_a - n_b|_1 (ops.normal_smoothness_loss:
    #                  DN-Splatter's edge-aware form).
    # Their gradient goes through ops.depth_to_normal_backward into the depth and opacity maps' gradients, beside the two
    # terms above.  The context renders depth as for those (inverse as distortion_inverse).  One rank only.
    normal_prior=False, normal_prior_weight=NORMAL_PRIOR_WEIGHT, normal_smooth=False,
    normal_smooth_weight=NORMAL_SMOOTH_WEIGHT, normal_edge_scale=1.0, normal_start=3000, normal_alpha_min=0.5,
    # features: C > 0 gives every gaussian a row of C trainable channels (Trainer.features: a column of the row table with
    # both Adam moments, carried by every row edit; initial value: Trainer(..., features=), default zeros).  From iteration
    # feature_start on, a view given as (camera, image, depth target or None, normal prior or None, feature target) also
    # renders the column (RasterContext.render_features) and adds feature_weight x
    #   feature_loss "ce":     the softmax cross-entropy of the map's channels against the target, an [H,W] int32 label map
    #                          (a label outside 0 .. C-1 is ignored), over all pixels (ops.feature_ce_loss);
    #   feature_loss "l1":     the mean of |map - target| for an [H,W,C] float32 target, or a pair (target, valid) with an
    #                          [H,W] uint8 validity map (ops.feature_l1_loss);
    #   feature_loss "cosine": the mean of 1 - cos(map, target) over the valid pixels where neither is zero
    #                          (ops.feature_cosine_loss).
    # The loss's gradient map is lifted onto the column (RasterContext.lift_features) and the rows the view saw take an
    # Adam step at feature_lr (ops.feature_adam_step) behind the optimizer step of the other groups.  feature_geometry:
    # the loss also reaches opacity, conic and position (features_backward inside whichever backward the iteration runs);
    # off, the image term's calls are exactly those of a run without the key.  Views without a target skip the term.  One
    # rank only.  feature_lr: README, "Training a feature field", has the numbers behind the default.
    features=0, feature_loss="ce", feature_weight=1.0, feature_start=0, feature_lr=0.0025, feature_geometry=False,
    # bilagrid: per-view appearance compensation ("Bilateral Guided Radiance Field Processing", Wang et al. 2024; gsplat's
    # lib_bilagrid).  Every training view owns a bilateral grid of 3x4 colour affines (Trainer.bilagrids
    # [V,12,L,Hg,Wg], identity at the start, addressed by the view's index in Trainer.views: train_step(view_index=)),
    # bilagrid_shape = (Wg, Hg, L); (1, 1, 1) is one colour affine per view: exposure and white balance.  From iteration
    # bilagrid_start on the render is corrected by the view's grid (ops.bilagrid_slice) before the L1 + SSIM loss, the
    # loss's gradient goes back through it (ops.bilagrid_slice_backward) to the render -- the backward and the optimizer
    # step see only that dL/d image, in every GSPLAT_FUSED_ADAM mode -- and to the grid, which also takes the gradient of
    # bilagrid_tv_weight x its total variation (ops.bilagrid_tv_loss) and an Adam step at bilagrid_lr with the bias
    # corrections of the view's own step count.  The depth, normal and feature terms keep reading the raw forward, and
    # evaluate() scores the raw render; Trainer.render_corrected gives a training view's corrected one.  One rank only.
    # The defaults of shape, rate and weight are gsplat's published ones (its bilateral-grid example: a 16 x 16 x 8 grid,
    # learning rate 2e-3, TV weight 10); nothing here has tuned them.
    bilagrid=False, bilagrid_shape=(16, 16, 8), bilagrid_lr=0.002, bilagrid_tv_weight=10.0, bilagrid_start=0)

FEATURE_LOSSES = ("ce", "l1", "cosine")


def _logit(p):
    return math.log(p) - math.log(1.0 - p)


def _compact_rows(t, keep, keep_n):
    """The keep_n rows of t ([N, ...] float32) whose byte of `keep` ([N] uint8) is set, in order."""
    stride = t.numel() // t.shape[0]
    return ops.compact_masked_array(stride, t.reshape(-1), keep, keep_n).reshape((keep_n,) + tuple(t.shape[1:]))


def contribution_prune_mask(weight_max, pixels, threshold):
    """The pruning policy on the two bit-reproducible statistics ([N] tensors, any device): True where a gaussian goes --
    no pixel composited it, or its largest blend weight is below `threshold` (0: only the never-composited ones).  Never
    everything: a mask that would leave no gaussian comes back all False."""
    remove = (pixels == 0) | (weight_max < float(threshold))
    if bool(remove.all()):
        remove = torch.zeros_like(remove)
    return remove


def mcmc_growth(n, grow_factor, max_gaussians):
    """How many gaussians one MCMC refinement step adds to n: up to int(grow_factor * n) in all, never past the cap."""
    return max(0, min(int(max_gaussians), int(grow_factor * n)) - n)


def draw_view_indices(rng, iteration, world, num_views):
    """View indices of one iteration, one per rank, identical on every rank that shares the generator's seed.  The
    reference walks the first two images in order and then draws uniformly (cuda/trainer.cu:1438-1444); with W ranks
    an iteration consumes W consecutive draws of that sequence (rank r trains on the r-th)."""
    draws = []
    for k in range(world):
        g = iteration * world + k
        draws.append(g if g < 2 else int(rng.integers(0, num_views)))
    return [d % num_views for d in draws]


class Trainer:
    """params: dict of device tensors (xyz rgb opacity scale quaternion, optionally sh) as gsplat_initialize_gaussians
    returns them; views: list of (camera dict for raster.device_camera, ground-truth image tensor [H,W,3] on device) or,
    for config key depth_prior, (camera, image, inverse-depth target [H,W] float32 on device) or, for config key
    normal_prior, (camera, image, that target or None, normal prior [H,W,3] float32 on device) or, for config key features,
    (camera, image, that target or None, that prior or None, feature target); features: the initial [N,C] float32 feature
    column of config key features (default: zeros)."""

    def __init__(self, params, views, config=None, scene_extent=1.0, seed=0, exchange="split", comm=None, features=None):
        """With an initialised torch.distributed group of W > 1 ranks the loop is view-sharded: every
        rank holds the same parameters and the same seed, one iteration = W training views (rank r takes the r-th of
        the iteration's W draws), the per-gaussian gradients and |grad_uv| are summed over the ranks
        (ViewShardedStep) and every rank applies the identical packed optimizer step and density control, so the
        replicas stay bit-identical without ever exchanging parameters."""
        self.cfg = dict(DEFAULT_CONFIG, **(config or {}))
        self.views = views
        # the ranks of the group: torch.distributed's default group, or in-process rank threads (dist.ThreadGroup)
        self.comm = comm if comm is not None else TorchComm()
        self.world, self.rank = self.comm.world, self.comm.rank
        self.exchange = exchange
        # r06, one rank: where the optimizer step runs (GSPLAT_FUSED_ADAM; every form leaves parameters, moments and
        # statistics bit-identical -- tests/test_optimizer_gpu.py; kernel times at 1e6 gaussians, SH 3, from one trace:
        # profiles/r06_two_kernel_adam.txt):
        #   1 (default): band 0, opacity, scale, rotation and the statistics inside the per-gaussian backward, then
        #     gsplat_optimizer_step_sh_factored (which takes its directions from positions that must not have moved yet) and
        #     gsplat_optimizer_step on the position group alone: 122 + 183 + 24 us against 72 + 176 + 94 -- 20 us of an
        #     iteration's 1100, and only the position and colour gradients are stored;
        #   3: two kernels -- sh_adam_dir_kernel in front reads the SH rows once (the SH group's step and the sums over the
        #     rows that the position gradient needs), then the backward with the five small groups' steps and no SH rows:
        #     219 + 113 us, 10 us of the 1100, no gradient arrays at all;
        #   2: all six groups inside the backward (one fat kernel at three waves per SIMD: 356 us, 2 % slower);
        #   0: the backward stores its gradients, the two optimizer kernels read them (r01-r05).
        self.fused_adam = int(os.environ.get("GSPLAT_FUSED_ADAM", "1") or 0)
        if self.cfg["antialiased"] or self.cfg["filter3d"]:
            self.fused_adam = 0  # whatever the environment says: the Adam-inside backward refuses the modes
        if self.cfg["mcmc"]:
            if self.world > 1:
                raise ValueError("mcmc trains on one rank: the sharded optimizer steps have no place for its regulariser")
            self.fused_adam = 0  # the regulariser is added to stored gradients, between the backward and the step
        self.mcmc_steps = []  # (iteration, gaussians relocated, gaussians added) of every MCMC refinement step
        if self.cfg["distortion"] or self.cfg["depth_prior"]:
            if self.world > 1:
                raise ValueError("distortion / depth_prior train on one rank: the view-sharded step takes no depth gradients")
            if self.cfg["distortion"] and self.cfg["absgrad"]:
                raise ValueError("distortion has no absgrad form: the compositing backward refuses the second moment's "
                                 "gradient in absgrad mode")
        if (self.cfg["normal_prior"] or self.cfg["normal_smooth"]) and self.world > 1:
            raise ValueError("normal_prior / normal_smooth train on one rank: the view-sharded step takes no depth gradients")
        if self.feature_channels:
            if self.world > 1:
                raise ValueError("features train on one rank: the view-sharded step has no place for the feature column")
            if not 1 <= self.feature_channels <= 512:
                raise ValueError("features must be 0 (off) or a channel count in 1 .. 512")
            if self.cfg["feature_loss"] not in FEATURE_LOSSES:
                raise ValueError("feature_loss must be one of %s" % (FEATURE_LOSSES,))
        elif features is not None:
            raise ValueError("a feature tensor needs config key features = its channel count")
        self.bilagrids = None        # [V,12,L,Hg,Wg]: the views' bilateral grids (config key bilagrid; None: off)
        self._bilagrid_state = None  # (exp_avg, exp_avg_sq as bilagrids, the views' Adam step counts, dL/d grid [12,L,Hg,Wg])
        self._grad_render = {}       # (H, W) -> dL/d render behind the grid, allocated once per image size
        if self.cfg["bilagrid"]:
            if self.world > 1:
                raise ValueError("bilagrid trains on one rank: the view-sharded step has no place for the views' grids")
            shape = self.cfg["bilagrid_shape"]
            if (not isinstance(shape, (tuple, list)) or len(shape) != 3 or not all(isinstance(v, int) for v in shape)
                    or not (1 <= shape[0] <= 64 and 1 <= shape[1] <= 64 and 1 <= shape[2] <= 16)):
                raise ValueError("bilagrid_shape must be (Wg, Hg, L) with 1 <= Wg, Hg <= 64 and 1 <= L <= 16")
        self._feat = None        # (features, exp_avg, exp_avg_sq), [N,C] each: the row table's feature column (_install)
        self._feat_grad = None   # [capacity,C]: dL/d features in global order, all zero between two steps
        self._feat_maps = {}     # (H, W) -> (feature map, dL/d feature map), [H,W,C] each, allocated once
        self._depth_maps = {}  # (H, W) -> the three gradient maps (dL/d alpha, dL/d depth, dL/d depth2), allocated once
        self._normal_maps = {}  # (H, W) -> (normal map, dL/d normal), [H,W,3] each, allocated once (normal_prior / _smooth)
        self._intrinsics = {}   # id(camera dict) -> (camera, ops.pixel_intrinsics of it): read from the device once
        self.last_regularisers = {}  # what the last train_step added: name -> weight
        self._filter3d = None       # [N] device tensor of the current gaussians; None: to be (re)computed
        self._filter3d_cams = None  # the training views' device camera arrays, built once
        self._sharded = None  # (key, ViewShardedStep) for the current gaussian count / SH degree
        self._grad_image = {}  # (H, W) -> dL/dimage buffer, allocated once per image size
        self._grads = None     # (capacity, l_max, dict): per-view gradient arrays, reused across iterations
        self._grads2 = None    # (capacity, dict): the two arrays behind a partial backward_pass_adam, reused likewise
        self.scene_extent = float(scene_extent)
        self.seed = int(seed)
        self.rng = np.random.default_rng(seed)
        self.iter = 0
        self.l_max = 0 if params.get("sh") is None or params["sh"].numel() == 0 else \
            int(round(math.sqrt(params["sh"].shape[1] + 1))) - 1
        self.params = {k: params[k].contiguous() for k in ("xyz", "rgb", "opacity", "scale", "quaternion")}
        n = self.num_gaussians
        self.params["sh"] = params["sh"].contiguous() if self.l_max > 0 else \
            torch.zeros(n, 0, 3, dtype=torch.float32, device=self.params["xyz"].device)
        W = max(int(v[0]["width"]) for v in views)
        H = max(int(v[0]["height"]) for v in views)
        self.ctx = self._new_context(max(n, 1), W, H)
        self.ctx_capacity = n
        self._install(RowTable.fresh(self.params, self._initial_features(features, n)))
        self.history = []
        self.contribution_prunes = []  # (iteration, gaussians removed) of every scheduled prune_by_contribution
        self._set_filter3d(self.ctx)
        if self.cfg["bilagrid"]:
            Wg, Hg, L = self.cfg["bilagrid_shape"]
            dev = self.params["xyz"].device
            self.bilagrids = ops.identity_bilagrid(Wg, Hg, L, views=len(views), device=dev)
            self._bilagrid_state = (torch.zeros_like(self.bilagrids), torch.zeros_like(self.bilagrids), [0] * len(views),
                                    torch.empty(12, L, Hg, Wg, dtype=torch.float32, device=dev))

    # ------------------------------------------------------------------ state
    _feat = None       # (a run without config key features has no column and no accumulator)
    _feat_grad = None

    @property
    def feature_channels(self):
        """C of config key features; 0: off."""
        return int(self.cfg["features"])

    @property
    def num_gaussians(self):
        return int(self.params["xyz"].shape[0])

    def _rows(self):
        """Everything that has a row per gaussian, as it stands."""
        o = self.opt
        return RowTable(self.params, o.exp_avg, o.exp_avg_sq, o.uv_grad_accum, o.grad_accum_dur, self._feat)

    def _initial_features(self, features, n):
        """The feature column a run starts with (config key features; None when it is off): the caller's [N,C] tensor,
        or zeros."""
        C = self.feature_channels
        if not C:
            return None
        dev = self.params["xyz"].device
        if features is None:
            return torch.zeros(n, C, dtype=torch.float32, device=dev)
        if (not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.device != dev
                or tuple(features.shape) != (n, C)):
            raise ValueError("features must be a float32 [%d,%d] tensor on %s: one row per gaussian, config key features "
                             "channels" % (n, C, dev))
        return features.contiguous()

    @property
    def features(self):
        """The feature column ([N,C] float32 device tensor, one row per gaussian in the current order: what
        render_features, feature_gradients and lift_maps take); None when config key features is off."""
        return None if self._feat is None else self._feat[0]

    def _install(self, rows):
        """Make `rows` (a RowTable) the run's state: the parameters, the SH degree their `sh` column has, and an
        AdamOptimizer over those very tensors that goes on from the table's moments and statistics.  The one place a new
        row set or row order comes in, so what depends on either is dropped here."""
        rows.check()
        sh = rows.params["sh"]
        l_max = math.isqrt(sh.shape[1] + 1) - 1 if sh.dim() == 3 else -1
        if tuple(sh.shape[1:]) != ((l_max + 1) ** 2 - 1, 3):
            raise ValueError("sh is %s: not the coefficients of an SH degree" % (tuple(sh.shape),))
        if (rows.features is not None) != bool(self.feature_channels) or \
                (rows.features is not None and rows.features[0].shape[1] != self.feature_channels):
            raise ValueError("the table's feature column does not match config key features = %d" % self.feature_channels)
        self.l_max = l_max
        self._feat = rows.features
        if self._feat_grad is not None and self._feat_grad.shape[0] < rows.num_rows:
            self._feat_grad = None  # (all zero between steps, whatever the row order: only its size follows the rows)
        self.params = dict(rows.params)
        self.opt = AdamOptimizer({g: self.params[g] for g in rows.exp_avg}, self.l_max, lr_config=self.cfg,
                                 scene_extent=self.scene_extent,
                                 state=(rows.exp_avg, rows.exp_avg_sq, rows.uv_grad_accum, rows.grad_accum_dur))
        self._sharded = None   # the exchange step is bound to the tensors that were replaced
        self._filter3d = None  # the gaussian set or its order changed

    def _new_context(self, n, W, H):
        ctx = raster.RasterContext(n, W, H)
        ctx.set_lean_forward(True)  # the loop only runs the fused backward, which recomputes Sigma / J / conic
        ctx.set_absgrad(bool(self.cfg["absgrad"]))
        ctx.set_antialiased(bool(self.cfg["antialiased"]))
        # the forward leaves the SH direction sums only where the iteration's backward reads them: the plain backward and
        # the one with the small groups' Adam inside; the other two forms read the rows, and the sums would be dead weight
        ctx.set_dir_sums(self.fused_adam in (0, 1))
        if self._depth_keys():  # (all off: the context is never put in depth mode)
            ctx.set_depth(True, inverse=bool(self.cfg["distortion_inverse"]), moment=bool(self.cfg["distortion"]))
        return ctx

    def _context_for(self, n):
        if n > self.ctx_capacity:  # the workspace is sized for a gaussian count: grow it geometrically
            self.ctx_capacity = int(n * 1.5) + 1
            self.ctx = self._new_context(self.ctx_capacity, self.ctx.max_width, self.ctx.max_height)
        self._set_filter3d(self.ctx)
        return self.ctx

    @property
    def filter3d(self):
        """The 3D smoothing filter of the current gaussians ([N] device tensor; None when the config key is off),
        computed from all training views (ops.compute_filter3d) when positions, set or order have changed since."""
        if not self.cfg["filter3d"] or self.num_gaussians == 0:
            return None
        if self._filter3d is None:
            if self._filter3d_cams is None:
                self._filter3d_cams = ops.camera_arrays([v[0] for v in self.views], self.params["xyz"].device)
            self._filter3d = ops.compute_filter3d(self.params["xyz"], *self._filter3d_cams,
                                                  near=float(self.cfg["filter3d_near"]))
        return self._filter3d

    def _set_filter3d(self, ctx):
        if self.cfg["filter3d"] and ctx._filter3d is not self.filter3d:
            ctx.set_filter3d(self.filter3d)

    def _refresh_filter3d(self, it):
        if self.cfg["filter3d"] and it % int(self.cfg["filter3d_interval"]) == 0 and it > 0:
            self._filter3d = None  # the positions have moved

    # ------------------------------------------------------------------ one iteration (cuda/trainer.cu:1338-1362)
    def _grad_image_for(self, H, W, device):
        buf = self._grad_image.get((H, W))
        if buf is None:
            buf = self._grad_image[(H, W)] = torch.empty(H, W, 3, dtype=torch.float32, device=device)
        return buf

    def _gradients_for(self, ctx, m):
        """Per-view gradient arrays in compacted order: allocated for the current gaussian count, sliced per view."""
        n = self.num_gaussians
        if self._grads is None or self._grads[0] < n or self._grads[1] != self.l_max:
            # density statistics need |grad_uv|; the SH gradients are not stored: the optimizer rebuilds them from the 24
            # bytes they are made of (AdamOptimizer.step, gsplat_optimizer_step_sh_factored) -- single-GPU training only,
            # the view-sharded step exchanges packed rows
            self._grads = (n, self.l_max, ctx.alloc_gradients(n, self.l_max, intermediates=("uv",), factored_sh=True))
        return {k: (v[:m] if v is not None else None) for k, v in self._grads[2].items()}

    def _partial_gradients_for(self, ctx, m):
        """The two arrays the optimizer kernels behind a partial backward_pass_adam read: grad_xyz, grad_precompute_rgb."""
        n = self.num_gaussians
        if self._grads2 is None or self._grads2[0] < n:
            dev = self.params["xyz"].device
            self._grads2 = (n, dict(xyz=torch.empty(n, 3, device=dev), precompute_rgb=torch.empty(n, 3, device=dev)))
        return {k: v[:m] for k, v in self._grads2[1].items()}

    def _depth_keys(self):
        """Whether any term on the depth maps is configured: the context then renders depth."""
        c = self.cfg
        return bool(c["distortion"] or c["depth_prior"] or c["normal_prior"] or c["normal_smooth"])

    def _intrinsics_of(self, cam):
        hit = self._intrinsics.get(id(cam))
        if hit is None or hit[0] is not cam:
            hit = self._intrinsics[id(cam)] = (cam, ops.pixel_intrinsics(cam))
        return hit[1]

    def depth_prior_weight(self, it):
        """The depth prior's weight at iteration `it`: exponential from depth_prior_weight_init to depth_prior_weight_final
        over num_iters."""
        c = self.cfg
        w0, w1 = float(c["depth_prior_weight_init"]), float(c["depth_prior_weight_final"])
        return w0 * (w1 / w0) ** (float(it) / float(c["num_iters"]))

    def _depth_regularisers(self, fwd, it, H, W, depth_target, cam=None, gt_image=None, normal_target=None):
        """The depth terms of this iteration (config keys distortion, depth_prior, normal_prior, normal_smooth), evaluated
        into the three reusable [H,W] maps: dict(grad_alpha=, grad_depth=, grad_depth2=) for the backward -- empty when no
        term is active, and then nothing here launches anything."""
        c = self.cfg
        self.last_regularisers = {}
        distortion = bool(c["distortion"]) and it >= int(c["distortion_start"])
        prior = bool(c["depth_prior"]) and depth_target is not None
        normals = it >= int(c["normal_start"])
        n_prior = normals and bool(c["normal_prior"]) and normal_target is not None
        n_smooth = normals and bool(c["normal_smooth"])
        if not (distortion or prior or n_prior or n_smooth):
            return {}
        maps = self._depth_maps.get((H, W))
        if maps is None:
            dev = fwd["T"].device
            maps = self._depth_maps[(H, W)] = tuple(torch.empty(H, W, dtype=torch.float32, device=dev) for _ in range(3))
        g_alpha, g_depth, g_depth2 = maps
        out = {}
        if distortion:
            w = float(c["distortion_weight"])
            ops.distortion_loss(fwd, w, g_alpha, g_depth, g_depth2)
            out = dict(grad_alpha=g_alpha, grad_depth=g_depth, grad_depth2=g_depth2)
            self.last_regularisers["distortion"] = w
        if prior:
            w = self.depth_prior_weight(it)
            ops.depth_prior_loss(fwd["depth"], depth_target, w, g_depth, accumulate=distortion)
            out["grad_depth"] = g_depth
            self.last_regularisers["depth_prior"] = w
        if n_prior or n_smooth:
            nmaps = self._normal_maps.get((H, W))
            if nmaps is None:
                dev = fwd["T"].device
                nmaps = self._normal_maps[(H, W)] = tuple(torch.empty(H, W, 3, dtype=torch.float32, device=dev) for _ in range(2))
            normal, g_normal = nmaps
            intr, inverse, a_min = self._intrinsics_of(cam), bool(c["distortion_inverse"]), float(c["normal_alpha_min"])
            ops.depth_to_normal(fwd, intr, inverse, alpha_min=a_min, out=normal)
            if n_prior:
                w = float(c["normal_prior_weight"])
                ops.normal_prior_loss(normal, normal_target, w, g_normal)
                self.last_regularisers["normal_prior"] = w
            if n_smooth:
                w = float(c["normal_smooth_weight"])
                ops.normal_smoothness_loss(normal, gt_image, w, g_normal, edge_scale=float(c["normal_edge_scale"]),
                                           accumulate=n_prior)
                self.last_regularisers["normal_smooth"] = w
            # added to what distortion / the depth prior wrote; a map neither wrote starts from zero
            if (distortion or prior) and "grad_alpha" not in out:
                g_alpha.zero_()
            ops.depth_to_normal_backward(fwd, intr, inverse, g_normal, g_depth, g_alpha, alpha_min=a_min,
                                         accumulate=distortion or prior)
            out["grad_depth"], out["grad_alpha"] = g_depth, g_alpha
        return out

    def _begin_step(self):
        """What an iteration starts with on one rank and on many: -> (iteration, background, context).  The SH band is
        added first: the context is sized and its 3D filter set for the gaussians the step trains."""
        c, it = self.cfg, self.iter
        # cuda/trainer.cu:1341-1343: the background cycles for the whole run (use_background_end is parsed but never read)
        bg = (it % 255) / 255.0 if c["use_background"] else 0.0
        if it % c["add_sh_band_interval"] == 0 and it >= c["add_sh_band_interval"]:
            self.add_sh_band()
        self._refresh_filter3d(it)
        return it, bg, self._context_for(self.num_gaussians)

    def _feature_target(self, target, H, W):
        """A view's feature target as the configured loss takes it -> (target, valid or None); ValueError otherwise."""
        C, kind = self.feature_channels, self.cfg["feature_loss"]
        valid = None
        if kind != "ce" and isinstance(target, (tuple, list)):
            if len(target) != 2:
                raise ValueError("a feature target with a validity map is the pair (target, valid)")
            target, valid = target
        want = (torch.int32, (H, W)) if kind == "ce" else (torch.float32, (H, W, C))
        if not isinstance(target, torch.Tensor) or target.dtype != want[0] or tuple(target.shape) != want[1] or not target.is_cuda:
            raise ValueError("the feature target of loss '%s' must be a %s device tensor of shape %s" % (kind, want[0], want[1]))
        if valid is not None and (not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8
                                  or tuple(valid.shape) != (H, W) or not valid.is_cuda):
            raise ValueError("the validity map of a feature target must be a uint8 device tensor of shape %s" % ((H, W),))
        return target.contiguous(), None if valid is None else valid.contiguous()

    def _feature_loss(self, fmap, target, valid, weight, grad_map, blocking=False):
        kind = self.cfg["feature_loss"]
        if kind == "ce":
            return ops.feature_ce_loss(fmap, target, weight, grad_map, blocking=blocking)
        fn = ops.feature_l1_loss if kind == "l1" else ops.feature_cosine_loss
        return fn(fmap, target, weight, grad_map, valid=valid, blocking=blocking)

    def _feature_term(self, ctx, it, H, W, feature_target):
        """The feature term of this iteration (config key features): the column rendered through the forward that just
        ran, the loss's gradient map, and that map lifted into the all-zero accumulator -> (features, grad_map) for the
        backward and the step, or None when the term is not active (nothing is launched or allocated then)."""
        c = self.cfg
        if not self.feature_channels or feature_target is None or it < int(c["feature_start"]):
            return None
        target, valid = self._feature_target(feature_target, H, W)
        feats, C, dev = self._feat[0], self.feature_channels, self.params["xyz"].device
        maps = self._feat_maps.get((H, W))
        if maps is None:
            maps = self._feat_maps[(H, W)] = tuple(torch.empty(H, W, C, dtype=torch.float32, device=dev) for _ in range(2))
        fmap, grad_map = maps
        n = self.num_gaussians
        if self._feat_grad is None:
            self._feat_grad = torch.zeros(max(n, self.ctx_capacity), C, dtype=torch.float32, device=dev)
        ctx.render_features(feats, out=fmap)
        w = float(c["feature_weight"])
        self._feature_loss(fmap, target, valid, w, grad_map)
        ctx.lift_features(grad_map, self._feat_grad[:n])
        self.last_regularisers["feature"] = w
        return feats, grad_map

    def _feature_step(self, it, fwd):
        """The feature column's Adam step on the rows the view saw, from the accumulator (which is all zero again after)."""
        f, m, v = self._feat
        b1c, b2c = self.opt.bias_corrections(it)
        ops.feature_adam_step(fwd["compact_to_global"], int(fwd["num_culled"]), f, m, v, self._feat_grad[:f.shape[0]],
                              float(self.cfg["feature_lr"]), B1, B2, EPS, b1c, b2c)

    def _bilagrid_view(self, view_index):
        """The index of a training view as config key bilagrid addresses its grid; ValueError when it names none."""
        if view_index is None:
            raise ValueError("config key bilagrid: train_step needs view_index=, the view's index in Trainer.views")
        v = int(view_index)
        if not 0 <= v < self.bilagrids.shape[0]:
            raise ValueError("view_index must lie in 0 .. %d" % (self.bilagrids.shape[0] - 1))
        return v

    def _bilagrid_step(self, v):
        """The Adam step of view v's grid from the gradient the iteration left, at the view's own step count."""
        m, sq, steps, grad = self._bilagrid_state
        b1c, b2c = self.opt.bias_corrections(steps[v])
        ops.adam_step(self.bilagrids[v], grad, m[v], sq[v], float(self.cfg["bilagrid_lr"]), B1, B2, EPS, b1c, b2c,
                      grad.numel(), 1)
        steps[v] += 1

    def train_step(self, cam, gt_image, want_loss=True, depth_target=None, normal_target=None, feature_target=None,
                   view_index=None):
        """depth_target: this view's inverse-depth prior (config key depth_prior), or None; normal_target: its normal prior
        (config key normal_prior), or None; feature_target: its feature target (config key features: an [H,W] int32 label
        map for feature_loss "ce", an [H,W,C] float32 map or (map, [H,W] uint8 validity) for "l1" / "cosine"), or None;
        view_index: the view's index in Trainer.views (config key bilagrid, which needs it: the view's grid)."""
        if self.world > 1:
            return self._train_step_sharded(cam, gt_image, want_loss)
        c = self.cfg
        bview = self._bilagrid_view(view_index) if c["bilagrid"] else None
        it, bg, ctx = self._begin_step()
        p = dict(self.params)
        H, W = int(cam["height"]), int(cam["width"])
        try:
            fwd = ctx.rasterize_image(p, cam, c, bg, self.l_max)
        except Exception as e:  # no gaussian in view: the reference warns and skips the iteration
            if getattr(e, "code", None) != -5:
                raise
            self.iter += 1
            return None
        grad_image = self._grad_image_for(H, W, gt_image.device)
        # the loss value is a blocking read-back: only fetched when the caller logs it
        bgrid = self.bilagrids[bview] if bview is not None and it >= int(c["bilagrid_start"]) else None
        if bgrid is None:
            loss = ops.fused_loss(fwd["image"], gt_image, H, W, float(c["ssim_frac"]), grad_image, blocking=want_loss)
        else:
            # config key bilagrid: the loss sees the render corrected by the view's grid; its gradient goes back through
            # the grid into a second buffer, which is the dL/d image of everything below, and into the grid's gradient
            grad_corrected, grad_image = grad_image, self._grad_render.get((H, W))
            if grad_image is None:
                grad_image = self._grad_render[(H, W)] = torch.empty_like(grad_corrected)
            corrected = ops.bilagrid_slice(bgrid, fwd["image"], out=grad_image)  # (the buffer is free until the backward)
            loss = ops.fused_loss(corrected, gt_image, H, W, float(c["ssim_frac"]), grad_corrected, blocking=want_loss)
            grad_grid = self._bilagrid_state[3]
            ops.bilagrid_slice_backward(bgrid, fwd["image"], grad_corrected, grad_image, grad_grid)
            ops.bilagrid_tv_loss(bgrid, float(c["bilagrid_tv_weight"]), grad_grid, accumulate=True)
        # the depth terms (config keys distortion, depth_prior, normal_prior, normal_smooth; {} when none is active: the
        # plain backward, exactly) ride with whichever backward the iteration runs -- the Adam-inside forms take the depth
        # row as it is
        dmaps = self._depth_regularisers(fwd, it, H, W, depth_target, cam, gt_image, normal_target) \
            if self._depth_keys() else {}
        # the feature term (config key features; None when it is off, not yet started or the view has no target: no launch):
        # the backward takes (features, grad_map) only with feature_geometry -- without it its calls are the plain ones
        if (self.feature_channels or c["bilagrid"]) and not self._depth_keys():
            self.last_regularisers = {}
        if bgrid is not None:
            self.last_regularisers["bilagrid_tv"] = float(c["bilagrid_tv_weight"])
        fterm = self._feature_term(ctx, it, H, W, feature_target) if self.feature_channels else None
        if fterm is not None and c["feature_geometry"]:
            dmaps = dict(dmaps, feature_grads=fterm)
        fused_adam = self.fused_adam  # (0 with antialiased, filter3d or mcmc: decided in __init__)
        if fused_adam == 3:
            # r06: the SH group's step in a kernel that reads the coefficient rows once (update + the sums the position
            # gradient needs), then the per-gaussian backward with the five small groups' steps inside: no gradient arrays
            ctx.backward_pass_adam(p, cam, grad_image, bg, self.l_max, self.opt.fused_state(it, mode=2), **dmaps)
        elif fused_adam == 2:
            # r06: the per-gaussian backward applies the optimizer step itself (no gradient arrays at all)
            ctx.backward_pass_adam(p, cam, grad_image, bg, self.l_max, self.opt.fused_state(it), **dmaps)
        elif fused_adam == 1:
            g2 = self._partial_gradients_for(ctx, fwd["num_culled"])
            ctx.backward_pass_adam(p, cam, grad_image, bg, self.l_max, self.opt.fused_state(it, mode=1), g2, **dmaps)
            self.opt.step_after_partial_backward(it, fwd, g2, cam["campos"])
        else:
            grads = self._gradients_for(ctx, fwd["num_culled"])
            ctx.backward_pass(p, cam, grad_image, bg, self.l_max, grads, **dmaps)
            if c["absgrad"]:  # the optimizer kernel takes the norm of what it is given as grad_uv: the absolute sums
                grads = dict(grads, uv=ctx.absgrad_uv())
            if c["mcmc"]:
                n = self.num_gaussians
                ops.mcmc_regularize(fwd["compact_to_global"], p["opacity"], p["scale"], float(c["mcmc_opacity_reg"]) / n,
                                    float(c["mcmc_scale_reg"]) / (3 * n), grads["opacity"], grads["scale"])
            self.opt.step(it, fwd, grads, campos=cam["campos"])
            if c["mcmc"]:
                ops.mcmc_add_noise(p["xyz"], p["opacity"], p["scale"], p["quaternion"],
                                   float(c["mcmc_noise_lr"]) * self.opt.learning_rates(it)["xyz"], self._mcmc_seed(it))
        if fterm is not None:
            self._feature_step(it, fwd)
        if bgrid is not None:
            self._bilagrid_step(bview)
        self.iter += 1
        return loss

    def _train_step_sharded(self, cam, gt_image, want_loss):
        """One iteration of a W-rank group: this rank's view -> loss -> backward -> exchange -> the same optimizer step on
        every rank, incl. the densification statistics (split exchange: AdamOptimizer.step_split on common + rgb_all;
        the other payloads: gsplat_optimizer_step_packed on the packed rows)."""
        c = self.cfg
        it, bg, ctx = self._begin_step()  # (the step below runs on this context, with the current 3D filter set)
        key = (self.num_gaussians, self.l_max)
        if self._sharded is None or self._sharded[0] != key:
            p = dict(self.params)
            self._sharded = (key, ViewShardedStep(p, self.l_max, ctx.max_width, ctx.max_height, c, 0.0,
                                                  exchange=self.exchange, with_uv_norm=True, ctx=ctx, comm=self.comm,
                                                  absgrad=bool(c["absgrad"]), antialiased=bool(c["antialiased"])))
        step = self._sharded[1]
        H, W = int(cam["height"]), int(cam["width"])
        out = {}

        def grad_fn(fwd):
            g = self._grad_image_for(H, W, gt_image.device)
            out["loss"] = ops.fused_loss(fwd["image"], gt_image, H, W, float(c["ssim_frac"]), g, blocking=want_loss)
            return g

        step.step(cam, grad_fn=grad_fn, bg=bg)
        if step.exchange == "split" and not step.materialize:
            # the exchange's own factored form feeds the optimizer: the colour groups rebuild sum_r g_rgb^r x Y_k(dir^r)
            # inside their Adam (gsplat_optimizer_step_sh_views), no packed[N, 12 + 3 n] rows are written or read
            self.opt.step_split(it, step.common, step.rgb_all, step.uv_norm_sum)
        else:
            self.opt.step_packed(it, step.packed, step.uv_norm_sum)
        self.iter += 1
        return out.get("loss")

    def maintenance(self):
        """Density control and opacity reset at the reference's cadence (cuda/trainer.cu:1394-1406); call after
        train_step.  Uses the iteration index the step just ran with.  Config key mcmc: relocation and growth at the
        density cadence instead of both (every step is recorded in mcmc_steps)."""
        c, it = self.cfg, self.iter - 1
        density = it > c["adaptive_control_start"] and it % c["adaptive_control_interval"] == 0 and it < c["adaptive_control_end"]
        if c["mcmc"]:  # relocation and growth at the same cadence; no thresholds, no opacity reset
            if density:
                relocated = self.mcmc_relocate()
                added = self.mcmc_grow()
                self.sort_gaussians()
                self.mcmc_steps.append((it, relocated, added))
        else:
            if density:
                self.adaptive_density_step()
                self.sort_gaussians()
                self.reset_grad_accum()
            if it > c["reset_opacity_start"] and it % c["reset_opacity_interval"] == 0 and it < c["reset_opacity_end"]:
                self.reset_opacity()
                self.reset_grad_accum()
        if c["prune_contribution"] and it >= c["adaptive_control_end"] and it % int(c["prune_contribution_interval"]) == 0:
            self.contribution_prunes.append((it, self.prune_by_contribution()))

    def draw_views(self):
        return draw_view_indices(self.rng, self.iter, self.world, len(self.views))

    def train(self, num_iters, log_every=0, loss_every=1, eval_every=0, eval_views=None, on_eval=None):
        """loss_every: read the loss value back every that many iterations (each read blocks the host; 0 = never);
        eval_every / eval_views / on_eval: `evaluate(eval_views)` at that cadence (the reference: every 3000
        iterations, cuda/trainer.cu:1388), reported through on_eval(iteration, psnr)."""
        for _ in range(num_iters):
            v = self.draw_views()[self.rank]
            cam, gt = self.views[v][:2]
            extra = {}  # (config keys depth_prior, normal_prior: passed only when the view has one)
            if len(self.views[v]) > 2 and self.views[v][2] is not None:
                extra["depth_target"] = self.views[v][2]
            if len(self.views[v]) > 3 and self.views[v][3] is not None:
                extra["normal_target"] = self.views[v][3]
            if len(self.views[v]) > 4 and self.views[v][4] is not None:  # (config key features)
                extra["feature_target"] = self.views[v][4]
            if self.cfg["bilagrid"]:
                extra["view_index"] = v
            want = bool(loss_every) and (self.iter % loss_every == 0 or (log_every and (self.iter + 1) % log_every == 0))
            loss = self.train_step(cam, gt, want_loss=want, **extra)
            if eval_every and (self.iter - 1) % eval_every == 0 and eval_views:
                psnr = self.evaluate(eval_views)
                if on_eval:
                    on_eval(self.iter - 1, psnr)
            self.maintenance()
            if loss is not None:
                self.history.append((self.iter, loss, self.num_gaussians))
            if log_every and self.iter % log_every == 0 and self.rank == 0:
                print(f"iter {self.iter}: loss {loss} gaussians {self.num_gaussians}", flush=True)
        return self.history

    def evaluate(self, views=None):
        """Mean PSNR over the views at background 0 (TrainerImpl::evaluate, cuda/trainer.cu:263-360), rendered in the
        mode the run trains in (config keys antialiased, filter3d)."""
        total, views = 0.0, (views or self.views)
        ctx = self._context_for(self.num_gaussians)
        ctx.set_render_only(True)  # nothing here runs a backward
        try:
            for cam, gt in (v[:2] for v in views):
                fwd = ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
                total += ops.compute_psnr(fwd["image"], gt, int(cam["height"]), int(cam["width"]))
        finally:
            ctx.set_render_only(False)
        return total / len(views)

    def render_corrected(self, view_index):
        """The render of training view `view_index` corrected by its bilateral grid (config key bilagrid): the forward on
        the render-only context at background 0, as evaluate() renders it, then ops.bilagrid_slice -> [H,W,3]."""
        if not self.cfg["bilagrid"]:
            raise ValueError("render_corrected needs config key bilagrid")
        v = self._bilagrid_view(view_index)
        cam = self.views[v][0]
        ctx = self._context_for(self.num_gaussians)
        ctx.set_render_only(True)
        try:
            fwd = ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
            return ops.bilagrid_slice(self.bilagrids[v], fwd["image"])
        finally:
            ctx.set_render_only(False)

    def evaluate_features(self, views=None):
        """The feature term over `views` (default: the training views) that carry a feature target, at feature_weight 1 and
        background 0 on the render-only context: dict(loss=the mean of the configured loss over those views, views=their
        number) and, for feature_loss "ce", accuracy=the share of the labelled pixels (0 <= label < C) of all those views
        whose largest channel is their label.  None when no view has a target.  Evaluation only: the accuracy is torch."""
        if not self.feature_channels:
            raise ValueError("evaluate_features needs config key features")
        views = [v for v in (self.views if views is None else views) if len(v) > 4 and v[4] is not None]
        if not views:
            return None
        ctx = self._context_for(self.num_gaussians)
        total, hits, labelled = 0.0, 0, 0
        ctx.set_render_only(True)
        try:
            for v in views:
                cam = v[0]
                H, W = int(cam["height"]), int(cam["width"])
                target, valid = self._feature_target(v[4], H, W)
                try:
                    ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
                    fmap = ctx.render_features(self._feat[0])
                except Exception as e:  # no gaussian in view: the map is zero
                    if getattr(e, "code", None) != -5:
                        raise
                    fmap = torch.zeros(H, W, self.feature_channels, dtype=torch.float32, device=target.device)
                total += self._feature_loss(fmap, target, valid, 1.0, None, blocking=True)
                if self.cfg["feature_loss"] == "ce":
                    on = (target >= 0) & (target < self.feature_channels)
                    hits += int(((fmap.argmax(-1) == target) & on).sum().item())
                    labelled += int(on.sum().item())
        finally:
            ctx.set_render_only(False)
        out = dict(loss=total / len(views), views=len(views))
        if self.cfg["feature_loss"] == "ce":
            out["accuracy"] = hits / labelled if labelled else float("nan")
        return out

    def render_normals(self, cam, alpha_min=None):
        """The [H,W,3] normal map of the current gaussians from `cam` (ops.depth_to_normal on a render-only forward at
        background 0, in the mode the run trains in): camera coordinates, facing the camera, (0,0,0) where there is none.
        alpha_min: config key normal_alpha_min unless given."""
        ctx = self._context_for(self.num_gaussians)
        inverse = bool(self.cfg["distortion_inverse"])
        mode = (ctx._depth, ctx._depth_inverse, ctx._depth_moment)
        ctx.set_render_only(True)
        try:
            if not mode[0]:  # a run without depth terms: depth mode for this forward only
                ctx.set_depth(True, inverse=inverse)
            fwd = ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
            return ops.depth_to_normal(fwd, self._intrinsics_of(cam), inverse if not mode[0] else mode[1],
                                       alpha_min=float(self.cfg["normal_alpha_min"] if alpha_min is None else alpha_min))
        finally:
            if not mode[0]:
                ctx.set_depth(False)
            ctx.set_render_only(False)

    def render_median_depth(self, cam, threshold=0.5):
        """The [H,W] median depth map of the current gaussians from `cam` (RasterContext.median_depth on a render-only
        forward at background 0, in the mode the run trains in): camera-space z of the gaussian at which the
        transmittance falls to `threshold`, 0 where it never does.  The context's flags are as before afterwards."""
        ctx = self._context_for(self.num_gaussians)
        ctx.set_render_only(True)
        try:
            ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
            return ctx.median_depth(threshold)
        finally:
            ctx.set_render_only(False)

    def extract_mesh(self, path=None, resolution=256, bounds=None, voxel=None, trunc=None, views=None, alpha_min=None,
                     max_depth=None, min_weight=1.0, batch=4, color=True, depth="expected", median_threshold=0.5,
                     min_component_faces=0, keep_largest=0):
        """A triangle mesh of the current gaussians: the depth maps of `views` ((camera, ...) tuples or camera dicts;
        default: the training views) fused into a TSDF volume (ops.tsdf_integrate) whose zero level set is extracted by
        marching tetrahedra (ops.tsdf_extract) -- the last step of 2DGS, RaDe-GS and GOF, what the depth, distortion and
        normal regularisers are for.  Returns dict(vertices [Nv,3] float32, faces [Nf,3] int32, colors [Nv,3] float32 or
        None, volume), device tensors, and writes a binary PLY (mesh.save_ply) when `path` is given.

        The views are rendered on the render-only context at background 0 in the mode the run trains in; a run without
        depth terms gets depth mode for this call only, as render_normals does, with `inverse` from config key
        distortion_inverse.  Up to `batch` views of one size are stacked into reusable buffers and integrated in one
        call (the volume is read and written once per call up to gsplat_tsdf_views_per_pass() views; the default 4 is the
        smallest batch beyond which the measured per-view time improves by less than 5 %); views of
        another size start another batch; a view in which nothing is visible is skipped.
        bounds: ((x0, y0, z0), (x1, y1, z1)); default: the cube centred at the mean camera position with half-side
        scene_extent -- a guess that suits an object the cameras surround at about that distance; a real capture wants
        an explicit box around what is to be meshed.  voxel: the longest side / resolution unless given.  trunc:
        4 voxels unless given -- a choice inside the 4..5 voxels the examples of Open3D and 2DGS use, not a tuned value.
        alpha_min: config key normal_alpha_min unless given.  max_depth: surface depths beyond it are ignored (None: no
        limit).  min_weight: a cell is meshed when all its eight nodes were observed that often.  One rank only.
        depth: "expected" fuses the expected depth sum alpha T z / (1 - T) as above; "median" fuses the median depth
        (RasterContext.median_depth at median_threshold: z of the gaussian at which the transmittance falls through it)
        with the surface form of the integration, gated by 1 - T >= alpha_min -- the context is not put into depth mode
        for it.  min_component_faces, keep_largest: ops.mesh_filter on the extracted mesh before it is written (both 0:
        no filter); its report is returned under the key `filter` (None without a filter)."""
        import math
        from . import mesh as mesh_io
        if self.world > 1:
            raise ValueError("extract_mesh runs on one rank only")
        if depth not in ("expected", "median"):
            raise ValueError('depth must be "expected" or "median"')
        median = depth == "median"
        median_threshold = float(median_threshold)
        if median and not (math.isfinite(median_threshold) and 0.0 < median_threshold < 1.0):
            raise ValueError("median_threshold must be finite and in (0, 1)")
        for name, v in (("min_component_faces", min_component_faces), ("keep_largest", keep_largest)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{name} must be a non-negative integer")
        if not isinstance(batch, int) or batch < 1:
            raise ValueError("batch must be a positive integer")
        cams = [v if isinstance(v, dict) else v[0] for v in (self.views if views is None else views)]
        if not cams:
            raise ValueError("extract_mesh needs at least one view")
        host = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)
        if bounds is None:
            centre = np.mean([host(c["campos"]).reshape(3) for c in cams], 0)
            lo, hi = centre - self.scene_extent, centre + self.scene_extent
        else:
            lo, hi = host(bounds[0]).reshape(3), host(bounds[1]).reshape(3)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
            raise ValueError("bounds must be a finite box with hi > lo")
        voxel = float((hi - lo).max()) / float(resolution) if voxel is None else float(voxel)
        if not (math.isfinite(voxel) and voxel > 0.0):
            raise ValueError("voxel (or resolution) must be finite and positive")
        dims = tuple(int(math.ceil(float(s) / voxel - 1e-9)) + 1 for s in (hi - lo))  # nodes: the cells cover the box
        dev = self.params["xyz"].device
        volume = ops.tsdf_volume(lo, voxel, dims, color=bool(color), device=dev)
        trunc = 4.0 * volume["voxel"] if trunc is None else float(trunc)
        alpha_min = float(self.cfg["normal_alpha_min"] if alpha_min is None else alpha_min)
        n = self.num_gaussians
        if n:
            ctx = self._context_for(n)
            inverse = bool(self.cfg["distortion_inverse"])
            mode = (ctx._depth, ctx._depth_inverse, ctx._depth_moment)
            if mode[0]:
                inverse = bool(mode[1])
            bufs, pending = {}, []  # (H, W) -> (depth, T, image) of `batch` views; the views stacked so far

            def flush(size):
                if pending:
                    k = len(pending)
                    d, t, im = bufs[size]
                    ops.tsdf_integrate(volume, d[:k], t[:k], np.stack([p[0] for p in pending]),
                                       np.asarray([p[1] for p in pending], np.float32), image=im[:k] if color else None,
                                       inverse=inverse and not median, alpha_min=alpha_min, trunc=trunc, near=0.0,
                                       max_depth=0.0 if max_depth is None else float(max_depth), surface=median)
                    del pending[:]

            ctx.set_render_only(True)
            try:
                if not mode[0] and not median:  # a run without depth terms: depth mode for these forwards only
                    ctx.set_depth(True, inverse=inverse)
                size = None
                for cam in cams:
                    this = (int(cam["height"]), int(cam["width"]))
                    if this != size or len(pending) == batch:
                        flush(size)
                        size = this
                    try:
                        fwd = ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
                    except Exception as e:  # no gaussian in view
                        if getattr(e, "code", None) != -5:
                            raise
                        continue
                    if size not in bufs:
                        z = lambda *s: torch.empty(batch, *s, dtype=torch.float32, device=dev)
                        bufs[size] = (z(*size), z(*size), z(*size, 3) if color else None)
                    k = len(pending)
                    if median:
                        ctx.median_depth(median_threshold, out=bufs[size][0][k])
                    else:
                        bufs[size][0][k].copy_(fwd["depth"])
                    bufs[size][1][k].copy_(fwd["T"])
                    if color:
                        bufs[size][2][k].copy_(fwd["image"])
                    pending.append((host(cam["view"]).reshape(-1)[:12].astype(np.float32), self._intrinsics_of(cam)))
                flush(size)
            finally:
                if not mode[0] and not median:
                    ctx.set_depth(False)
                ctx.set_render_only(False)
        vertices, faces, colors = ops.tsdf_extract(volume, min_weight=min_weight)
        vertices, faces, colors, report = ops.mesh_filter(vertices, faces, colors, min_faces=min_component_faces,
                                                          keep_largest=keep_largest)
        if path is not None:
            mesh_io.save_ply(path, vertices, faces, colors)
        return dict(vertices=vertices, faces=faces, colors=colors, volume=volume, filter=report)

    def contribution_scores(self, views=None):
        """dict(weight_sum, weight_max, pixels): [N] device tensors, the blend-weight statistics of every gaussian
        accumulated over `views` ((camera, image) pairs; default: all training views) -- sum and maximum of alpha * T
        over the pixels that composite it, and their number (RasterContext.accumulate_contributions).  Rendered at
        background 0 on the render-only context in the mode the run trains in (config keys antialiased, filter3d), as
        evaluate() does; a view in which nothing is visible contributes nothing."""
        n, dev = self.num_gaussians, self.params["xyz"].device
        out = dict(weight_sum=torch.zeros(n, dtype=torch.float32, device=dev),
                   weight_max=torch.zeros(n, dtype=torch.float32, device=dev),
                   pixels=torch.zeros(n, dtype=torch.int32, device=dev))
        if n == 0:
            return out
        ctx = self._context_for(n)
        ctx.set_render_only(True)
        try:
            for cam in (v[0] for v in (self.views if views is None else views)):
                try:
                    ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
                except Exception as e:  # no gaussian in view
                    if getattr(e, "code", None) != -5:
                        raise
                    continue
                ctx.accumulate_contributions(**out)
        finally:
            ctx.set_render_only(False)
        return out

    def render_features(self, cam, features):
        """The [H,W,C] map of the caller's per-gaussian channels `features` ([N,C] float32 device tensor, one row per
        gaussian in the current order) from `cam`: a render-only forward at background 0 in the mode the run trains in,
        then RasterContext.render_features on it (sum of alpha * T * features over the gaussians a pixel composites;
        no background term).  Nothing is differentiated here: feature_gradients returns the gradients of a loss on the
        map with respect to the gaussians and the features.

        A tensor of the caller's own is not a column of the trainer's row table: whatever changes the set or the order of
        the gaussians (densification, pruning, relocation, the Morton re-order) invalidates it.  The trainer's own
        column (config key features: Trainer.features) follows every such edit and may be passed here."""
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != self.num_gaussians:
            raise ValueError("features must be an [N,C] tensor with one row per gaussian (N = %d)" % self.num_gaussians)
        ctx = self._context_for(self.num_gaussians)
        ctx.set_render_only(True)
        try:
            ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
            return ctx.render_features(features)
        finally:
            ctx.set_render_only(False)

    def feature_gradients(self, cam, features, grad_fn):
        """The gradients of a loss on the feature map of `cam` with respect to the gaussians AND the features:
        a training forward of the current state in the mode the run trains in, fmap = render_features(features),
        grad_map = grad_fn(fmap) ([H,W,C] float32, dL/d fmap), then a compositing backward of a zero image gradient,
        RasterContext.features_backward and the plain per-gaussian backward (the 3D filter's chain rule inside it, as in
        train_step's unfused path).  Returns dict(xyz [N,3], opacity [N], scale [N,3], quaternion [N,4], features [N,C])
        in the current order of the gaussians, zero for the gaussians the view culled; `features` is
        lift_features(grad_map).  Nothing is trained: no iteration is counted, no moment or densification statistic is
        touched -- a semantic or mask loss that should move the gaussians is stepped by the caller.  One rank only.

        `features` is the caller's tensor (see render_features)."""
        if self.world > 1:
            raise ValueError("feature_gradients runs on one rank only")
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != self.num_gaussians:
            raise ValueError("features must be an [N,C] tensor with one row per gaussian (N = %d)" % self.num_gaussians)
        n, dev = self.num_gaussians, self.params["xyz"].device
        ctx = self._context_for(n)
        p = dict(self.params)
        H, W = int(cam["height"]), int(cam["width"])
        fwd = ctx.rasterize_image(p, cam, self.cfg, 0.0, self.l_max)
        fmap = ctx.render_features(features)
        grad_map = grad_fn(fmap)
        m = int(fwd["num_culled"])
        grads = ctx.alloc_gradients(m, self.l_max, device=dev)
        ctx.backward_render(torch.zeros(H, W, 3, dtype=torch.float32, device=dev), 0.0)
        ctx.features_backward(features, grad_map)
        ctx.backward_gaussians(p, cam, self.l_max, grads)
        c2g = fwd["compact_to_global"].long()
        out = {}
        for k, shape in (("xyz", (n, 3)), ("opacity", (n,)), ("scale", (n, 3)), ("quaternion", (n, 4))):
            out[k] = torch.zeros(*shape, dtype=torch.float32, device=dev)
            out[k][c2g] = grads[k].reshape((m,) + shape[1:])
        out["features"] = ctx.lift_features(grad_map, torch.zeros_like(features))
        return out

    def lift_maps(self, views_and_maps, normalize=True):
        """[N,C] float32: the maps of `views_and_maps` ((camera, map [H,W,C] float32 device tensor) pairs) lifted onto
        the gaussians that produced their pixels (RasterContext.lift_features on a render-only forward at background 0
        of every view, in the mode the run trains in), summed over the views.  normalize: divided by the gaussian's
        summed blend weight over the same views (accumulate_contributions' weight_sum) -- the weighted mean of what
        its pixels said: label lifting.  Rows no pixel composited stay 0; a view in which nothing is visible
        contributes nothing.  The rows follow the current order of the gaussians (see render_features)."""
        views_and_maps = list(views_and_maps)
        if not views_and_maps:
            raise ValueError("lift_maps needs at least one (camera, map) pair")
        for _, m in views_and_maps:
            if not isinstance(m, torch.Tensor) or m.dim() != 3 or m.shape[2] != views_and_maps[0][1].shape[2]:
                raise ValueError("every map must be an [H,W,C] tensor with the same C")
        n, dev = self.num_gaussians, self.params["xyz"].device
        lifted = torch.zeros(n, int(views_and_maps[0][1].shape[2]), dtype=torch.float32, device=dev)
        weight = torch.zeros(n, dtype=torch.float32, device=dev)
        if n == 0:
            return lifted
        ctx = self._context_for(n)
        ctx.set_render_only(True)
        try:
            for cam, m in views_and_maps:
                try:
                    ctx.rasterize_image(dict(self.params), cam, self.cfg, 0.0, self.l_max)
                except Exception as e:  # no gaussian in view
                    if getattr(e, "code", None) != -5:
                        raise
                    continue
                ctx.lift_features(m, lifted)
                if normalize:
                    ctx.accumulate_contributions(weight_sum=weight)
        finally:
            ctx.set_render_only(False)
        if normalize:
            lifted = torch.where(weight[:, None] > 0, lifted / weight[:, None].clamp_min(1e-38), torch.zeros_like(lifted))
        return lifted

    def prune_by_contribution(self, threshold=None, views=None, scores=None):
        """Remove the gaussians that no pixel of `views` composites (pixels == 0) or whose largest blend weight over them
        is below `threshold` (default: the config's prune_contribution_threshold; 0 removes only the never-composited
        ones); `scores`: a contribution_scores() result to decide from instead of walking the views.  Survivors keep
        their order; parameters, both Adam moments of every group and the densification statistics are compacted with
        the same mask.  Never leaves zero gaussians: that prune changes nothing.  Returns the number removed.

        The decision reads only weight_max and pixels, which carry the same bits in every run.  With world > 1 every
        rank walks ALL training views itself and prunes from them, so the replicas stay bit-identical with no exchange."""
        n = self.num_gaussians
        if n == 0:
            return 0
        if scores is None:
            scores = self.contribution_scores(views)
        thr = self.cfg["prune_contribution_threshold"] if threshold is None else threshold
        remove = contribution_prune_mask(scores["weight_max"], scores["pixels"], thr)
        n_remove = int(remove.sum().item())
        if n_remove == 0:
            return 0
        keep, keep_n = (~remove).to(torch.uint8).contiguous(), n - n_remove
        # parameters, moments and statistics alike: the survivors' rows move up
        self._install(self._rows().map(lambda kind, name, t: _compact_rows(t, keep, keep_n)))
        return n_remove

    # ------------------------------------------------------------------ policy steps
    def reset_grad_accum(self):  # cuda/trainer.cu:233-236
        self.opt.uv_grad_accum.zero_()
        self.opt.grad_accum_dur.zero_()

    def reset_opacity(self):  # cuda/trainer.cu:238-245
        self.params["opacity"].fill_(_logit(float(self.cfg["reset_opacity_value"])))
        self.opt.exp_avg["opacity"].zero_()
        self.opt.exp_avg_sq["opacity"].zero_()

    def add_sh_band(self):  # cuda/trainer.cu:377-413
        if self.l_max >= self.cfg["max_sh_band"]:
            return
        # the same rows with a wider `sh` column, so not a map: `sh` and its two moments are re-laid out with the new band
        # zero (the first band's moments start at zero: there were none); the other groups and the statistics are kept
        old, rows = self.l_max, self._rows()
        sh = ops.expand_sh(rows.params["sh"], old)
        m, v = (ops.expand_sh(mom["sh"], old) if old else torch.zeros_like(sh) for mom in (rows.exp_avg, rows.exp_avg_sq))
        self._install(RowTable(dict(rows.params, sh=sh), dict(rows.exp_avg, sh=m), dict(rows.exp_avg_sq, sh=v),
                               rows.uv_grad_accum, rows.grad_accum_dur, rows.features))

    def adaptive_density_step(self):  # cuda/trainer.cu:518-779
        c, n = self.cfg, self.num_gaussians
        if os.environ.get("GSPLAT_DEBUG_DENSITY") and self.rank == 0:
            avg = (self.opt.uv_grad_accum / self.opt.grad_accum_dur.clamp(min=1).float())
            q = torch.quantile(avg[:: max(1, n // 500000)], torch.tensor([0.5, 0.9, 0.99, 0.999], device=avg.device)).tolist()
            print(f"[density] iter {self.iter}: n {n}, avg |grad_uv| quantiles 50/90/99/99.9 % = "
                  + " ".join(f"{v:.2e}" for v in q) + f", threshold {c['uv_grad_threshold']:.1e}, mean views seen "
                  f"{self.opt.grad_accum_dur.float().mean().item():.1f}", flush=True)
        max_scale = self.scene_extent * 0.1
        clone_thresh = self.scene_extent * 0.01
        prune, clone, split, keep, (n_prune, n_clone, n_split) = ops.density_masks(
            self.params["opacity"], self.params["scale"], self.opt.uv_grad_accum, self.opt.grad_accum_dur,
            _logit(float(c["delete_opacity_threshold"])), max_scale, float(c["uv_grad_threshold"]), clone_thresh)
        if not c["use_delete"]:
            n_prune = 0
            keep = (1 - split).to(torch.uint8)
        if not c["use_clone"]:
            n_clone, clone = 0, torch.zeros_like(clone)
        if not c["use_split"]:
            n_split, split = 0, torch.zeros_like(split)
            keep = (1 - prune).to(torch.uint8) if c["use_delete"] else torch.ones_like(keep)
        n_add = n_clone + 2 * n_split
        new_n = n - n_prune - n_split + n_add
        if new_n > c["max_gaussians"] or (n_add == 0 and n_prune == 0):
            return dict(pruned=0, cloned=0, split=0, skipped=new_n > c["max_gaussians"])
        nsh = (self.l_max + 1) ** 2 - 1 if self.l_max > 0 else 0
        dev = self.params["xyz"].device
        src = dict(self.params)
        src["sh"] = self.params["sh"].reshape(n, -1)

        def fresh(rows):
            return dict(xyz=torch.empty(rows, 3, device=dev), rgb=torch.empty(rows, 3, device=dev),
                        opacity=torch.empty(rows, device=dev), scale=torch.empty(rows, 3, device=dev),
                        quaternion=torch.empty(rows, 4, device=dev), sh=torch.empty(rows, nsh * 3, device=dev))

        def write_ids(mask):
            m = mask.to(torch.int32)
            return (torch.cumsum(m, 0, dtype=torch.int32) - m).contiguous()

        clones, splits = fresh(n_clone), fresh(2 * n_split)
        if n_clone:
            ops.clone_gaussians(n, nsh, clone, write_ids(clone), src, clones)
        if n_split:
            ops.split_gaussians(n, float(c["split_scale_factor"]), nsh, split, write_ids(split), src, splits,
                                seed=self.seed * 1000003 + self.iter)
        keep_n = n - n_prune - n_split

        def relayout(kind, g, t):  # -> [kept | clones | split pairs]
            if kind == STAT:  # zero: maintenance() resets the statistics behind every density step anyway
                return t.new_zeros(new_n)
            kept, row = _compact_rows(t, keep, keep_n), tuple(t.shape[1:])
            if kind == MOMENT:  # kept rows keep their moments, new rows start at zero (cuda/trainer.cu:703-742)
                return torch.cat([kept, t.new_zeros((n_add,) + row)], 0)
            if g == "features":
                # the kernels know nothing of the column: a clone takes its source's row, both children of a split their
                # parent's, in the kernels' row order -- clone k is the k-th flagged gaussian (write_ids), the children
                # of the k-th flagged split are rows 2 k and 2 k + 1 (gs_density.hip)
                return torch.cat([kept, t[clone.bool()], t[split.bool()].repeat_interleave(2, 0)], 0)
            return torch.cat([kept, clones[g].reshape((n_clone,) + row), splits[g].reshape((2 * n_split,) + row)], 0)

        self._install(self._rows().map(relayout))
        return dict(pruned=n_prune, cloned=n_clone, split=n_split, skipped=False)

    # ------------------------------------------------------------------ MCMC densification (config key mcmc)
    def _mcmc_seed(self, it):
        return self.seed * 1000003 + it

    def mcmc_relocate(self, seed=None):
        """Move the dead gaussians (opacity at or below mcmc_min_opacity) onto live ones drawn with probability
        proportional to their opacity.  A source drawn c times and its c copies take the opacity and scale that make the
        c + 1 of them render what the source rendered (ops.mcmc_relocate), the copies every other attribute of the source;
        both Adam moments of the sources and the moved rows restart at zero.  seed: default, the one of the iteration the
        last train_step ran.  Returns the number of gaussians moved (0 when none or all are dead)."""
        c, n = self.cfg, self.num_gaussians
        opacity = self.params["opacity"]
        dead = opacity <= _logit(float(c["mcmc_min_opacity"]))
        dead_idx = dead.nonzero().reshape(-1)
        k = int(dead_idx.numel())
        if k == 0 or k == n:
            return 0
        weights = torch.sigmoid(opacity).masked_fill(dead, 0.0)
        samples, counts = ops.sample_by_weight(weights, k, self._mcmc_seed(self.iter - 1) if seed is None else seed)
        ops.mcmc_relocate(opacity, self.params["scale"], counts, float(c["mcmc_min_opacity"]))
        src = samples.long()
        restart = torch.cat([src, dead_idx])

        def relocate(kind, name, t):
            if kind == PARAM:  # after the update: the copies carry the new opacity and scale
                t[dead_idx] = t[src]
            elif kind == MOMENT:
                t[restart] = 0
            return t  # the statistics: kept

        # in place: the row set and every tensor stay, so there is nothing to install and the exchange step stays bound
        self._rows().map(relocate)
        self._filter3d = None  # positions changed
        return k

    def mcmc_grow(self, seed=None):
        """Add mcmc_growth(N, mcmc_grow_factor, max_gaussians) gaussians as copies of sources drawn with probability
        proportional to their opacity, corrected like a relocation; the moments of the sources and the new rows are zero.
        seed: default, the one of the last iteration plus 2^32.  Returns the number added."""
        c, n = self.cfg, self.num_gaussians
        k = mcmc_growth(n, float(c["mcmc_grow_factor"]), c["max_gaussians"])
        if k == 0 or n == 0:
            return 0
        samples, counts = ops.sample_by_weight(torch.sigmoid(self.params["opacity"]), k,
                                               self._mcmc_seed(self.iter - 1) + 2 ** 32 if seed is None else seed)
        ops.mcmc_relocate(self.params["opacity"], self.params["scale"], counts, float(c["mcmc_min_opacity"]))
        src = samples.long()

        def grow(kind, name, t):  # -> [old | copies of src]
            if kind == PARAM:
                return torch.cat([t, t[src]], 0)
            if kind == STAT:  # zero: no step of the mode reads the statistics
                return t.new_zeros(n + k)
            t = torch.cat([t, t.new_zeros((k,) + tuple(t.shape[1:]))], 0)
            t[src] = 0
            return t

        self._install(self._rows().map(grow))
        self._context_for(n + k)
        return k

    def sort_gaussians(self):  # cuda/trainer.cu:853-922: Morton order of the positions
        n = self.num_gaussians
        if n == 0:
            return
        xyz = self.params["xyz"]
        lo, hi = xyz.min(0).values.tolist(), xyz.max(0).values.tolist()
        codes = torch.empty(n, dtype=torch.int64, device=xyz.device)
        ops.compute_morton_codes(n, xyz, hi[0], hi[1], hi[2], lo[0], lo[1], lo[2], codes)
        order = torch.sort(codes, stable=True).indices.to(torch.int32).contiguous()  # codes use 63 bits: int64 order is unsigned order
        # parameters, moments and statistics alike: every row moves to its place in the order
        self._install(self._rows().map(lambda kind, name, t: ops.gather_rows(t, order)))

    def save_to_ply(self, path, raw=False):
        """With the 3D smoothing filter on, the file holds the FUSED scale and opacity (ops.filter3d_apply: what the run
        rasterizes), so that an ordinary viewer shows what was trained; raw=True writes the raw parameters.
        TrainerImpl::save_to_ply (cuda/trainer.cu:1166-1196): the device quaternion (kernel order w,x,y,z) is
        memcpy'd into Eigen's (x,y,z,w) storage and normalised, so the file's rot_0..3 are the unit quaternion in
        DEVICE order.  gsplat_save_ply writes its (w,x,y,z) input as (x,y,z,w) (Gaussians' Eigen convention), so the
        columns are pre-rotated here to land unchanged."""
        from . import dataset
        params = dict(self.params)
        if self.cfg["filter3d"] and not raw and self.num_gaussians:
            params["scale"], params["opacity"] = ops.filter3d_apply(params["scale"], params["opacity"], self.filter3d)
        p = {k: v.detach().cpu().numpy() for k, v in params.items()}
        q = p["quaternion"].astype(np.float32)
        norm = np.sqrt((q.astype(np.float64) ** 2).sum(1, keepdims=True))
        q = (q / np.where(norm > 0, norm, 1.0)).astype(np.float32)
        dataset.save_ply(path, p["xyz"], p["rgb"], p["opacity"], p["scale"], np.roll(q, 1, axis=1),
                         p["sh"].reshape(len(p["xyz"]), -1) if self.l_max > 0 else None)

    def save_compressed(self, path, raw=False, codebook_size=65536, iterations=10, seed=0):
        """The scene as a compressed .npz (compress.py: SH rows vector-quantised into a codebook by ops.vq_fit, the other
        attributes in 8 or 16 bits), readable with compress.load_scene.  As in save_to_ply the file holds the FUSED scale
        and opacity under the 3D smoothing filter unless raw=True.  Returns the arrays written, with the k-means
        objective per assign under "objective" (not part of the file)."""
        from . import compress
        params = dict(self.params)
        if self.cfg["filter3d"] and not raw and self.num_gaussians:
            params["scale"], params["opacity"] = ops.filter3d_apply(params["scale"], params["opacity"], self.filter3d)
        p = {k: v.detach().cpu().numpy() for k, v in params.items()}
        objective = []

        def fit(rows, K, its, sd):  # the rows are on the device already
            codebook, index, obj = ops.vq_fit(params["sh"].reshape(self.num_gaussians, -1).contiguous(), K,
                                              iterations=its, seed=sd)
            objective.extend(obj)
            return codebook.cpu().numpy(), index.cpu().numpy()

        arrays = compress.save_scene(path, p, fit=fit, codebook_size=codebook_size, iterations=iterations, seed=seed)
        return dict(arrays, objective=np.asarray(objective, np.float64))

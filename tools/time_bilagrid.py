"""The bilateral-grid entry points (gsplat_bilagrid_slice, gsplat_bilagrid_slice_backward, gsplat_bilagrid_tv_loss) at
1920x1080 under a (1,1,1) and a (16,16,8) grid, on a noise image and on a render, by events, warm, beside what a caller
did before they existed, in the same session: the torch expression that produces the same outputs with autograd (a 5-D
grid_sample with align_corners and border padding + the per-pixel 3x4 product; forward and backward timed together) and
the TV loss as torch differences.  With the algorithmic bytes of a launch the achieved bytes per second are printed.
Then the whole training step at 1e6 gaussians (config3) with the key on against the plain step, alternating.
Warm: 10 calls before the 50 that count; medians.

usage: python tools/time_bilagrid.py [--no-step]   (JSON lines on stdout)"""
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("3dgs_amd.ops")
raster = importlib.import_module("3dgs_amd.raster")
scene = importlib.import_module("3dgs_amd.scene")
trainer_mod = importlib.import_module("3dgs_amd.trainer")

GRIDS = ((1, 1, 1), (16, 16, 8))
H, W = 1080, 1920
TV_WEIGHT = 10.0


def by_events(fn, warm=10, reps=50):
    ts = []
    for rep in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warm:
            ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def torch_slice(grid, image):
    Hh, Ww, _ = image.shape
    g = image[..., 0] * 0.299 + image[..., 1] * 0.587 + image[..., 2] * 0.114
    xs = (torch.arange(Ww, device=image.device, dtype=torch.float32) + 0.5) / Ww
    ys = (torch.arange(Hh, device=image.device, dtype=torch.float32) + 0.5) / Hh
    coords = torch.stack([xs[None, :].expand(Hh, Ww), ys[:, None].expand(Hh, Ww), g.clamp(0.0, 1.0)], -1) * 2.0 - 1.0
    A = torch.nn.functional.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True,
                                        padding_mode="border")
    A = A[0, :, 0].permute(1, 2, 0).reshape(Hh, Ww, 3, 4)
    return (A[..., :3] * image[:, :, None, :]).sum(-1) + A[..., 3]


def torch_forward_backward(grid, image, grad_out):
    g, im = grid.detach().requires_grad_(True), image.detach().requires_grad_(True)
    out = torch_slice(g, im)
    out.backward(grad_out)
    return out.detach(), im.grad, g.grad


def torch_tv(grid):
    g = grid.detach().requires_grad_(True)
    loss = 0.0
    for axis in (1, 2, 3):
        if g.shape[axis] > 1:
            loss = loss + torch.diff(g, dim=axis).square().mean()
    if not isinstance(loss, torch.Tensor):
        return torch.zeros_like(g)
    (TV_WEIGHT * loss).backward()
    return g.grad


def kernels():
    rng = np.random.default_rng(5)
    P = H * W
    grad_out = torch.as_tensor(rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)).cuda()
    # two images: uniform noise in [-0.2, 1.3] (every z-cell in every tile, a tenth of the pixels clamped) and what the
    # trainer hands the slice, a render (config3, view 0: a tile sits in one or two z-cells)
    N, Wd, Hd, l_max, _ = scene.WORKLOADS["config3"]
    assert (Hd, Wd) == (H, W)
    ctx = raster.RasterContext(N, W, H)
    ctx.set_render_only(True)
    render = ctx.rasterize_image(raster.device_params(scene.make_workload_gaussians("config3")),
                                 raster.device_camera(scene.make_camera(W, H, 0)), scene.CONFIG, 0.0, l_max)["image"].clone()
    del ctx
    noise = torch.as_tensor(rng.uniform(-0.2, 1.3, (H, W, 3)).astype(np.float32)).cuda()
    for (Wg, Hg, L), (what, image) in ((g, im) for g in GRIDS for im in (("noise", noise), ("render", render))):
        grid = ops.identity_bilagrid(Wg, Hg, L) + torch.as_tensor(rng.uniform(-0.5, 0.5, (12, L, Hg, Wg)).astype(np.float32)).cuda()
        out, gi, gg, gtv = torch.empty_like(image), torch.empty_like(image), torch.empty_like(grid), torch.empty_like(grid)
        ops.bilagrid_slice(grid, image, out=out)
        ops.bilagrid_slice_backward(grid, image, grad_out, gi, gg)
        ops.bilagrid_tv_loss(grid, TV_WEIGHT, gtv)
        t_out, t_gi, t_gg = torch_forward_backward(grid, image, grad_out)
        diffs = dict(out=float((out - t_out).abs().max()), grad_image=float((gi - t_gi).abs().max()),
                     grad_grid_relative=float((gg - t_gg).abs().max() / t_gg.abs().max()),
                     tv=float((gtv - torch_tv(grid)).abs().max()))
        # where dL/d image differs from the float32 torch expression: the pixels and the float64 luma of the worst one
        # (the derivative with respect to the luma jumps at a z-knot and at the two clamps)
        off = (gi - t_gi).abs().amax(-1)
        worst = int(off.argmax())
        luma = (image.double() * torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64, device="cuda")).sum(-1)
        diffs.update(grad_image_pixels_above_1e_3=int((off > 1e-3).sum()), worst_pixel_luma=float(luma.reshape(-1)[worst]),
                     worst_pixel_luma_times_levels=float(luma.reshape(-1)[worst]) * (L - 1))
        grid_bytes = grid.numel() * 4
        # bytes a launch has to move: the image read once and written once (forward), image and dL/d out read once and
        # dL/d image written once (backward to the image), image and dL/d out read once and the grid written once (to the grid)
        bytes_of = dict(slice=P * 24 + grid_bytes, grad_image=P * 36 + grid_bytes, grad_grid=P * 24 + grid_bytes,
                        backward=P * 36 + 2 * grid_bytes, tv=3 * grid_bytes)
        us = dict(slice=by_events(lambda: ops.bilagrid_slice(grid, image, out=out)),
                  grad_image=by_events(lambda: ops.bilagrid_slice_backward(grid, image, grad_out, gi, None)),
                  grad_grid=by_events(lambda: ops.bilagrid_slice_backward(grid, image, grad_out, None, gg)),
                  backward=by_events(lambda: ops.bilagrid_slice_backward(grid, image, grad_out, gi, gg)),
                  tv=by_events(lambda: ops.bilagrid_tv_loss(grid, TV_WEIGHT, gtv)),
                  tv_with_loss_readback=by_events(lambda: ops.bilagrid_tv_loss(grid, TV_WEIGHT, gtv, blocking=True)))
        t_fb = by_events(lambda: torch_forward_backward(grid, image, grad_out))
        with torch.no_grad():
            t_f = by_events(lambda: torch_slice(grid, image))
        t_tv = by_events(lambda: torch_tv(grid))
        line = dict(grid=[Wg, Hg, L], image=what, width=W, height=H, max_abs_difference_to_torch=diffs,
                    torch_forward_us=round(t_f, 1), torch_forward_backward_us=round(t_fb, 1), torch_tv_us=round(t_tv, 1),
                    torch_over_kernels=round(t_fb / (us["slice"] + us["backward"]), 1),
                    torch_forward_over_slice=round(t_f / us["slice"], 1), torch_tv_over_kernel=round(t_tv / us["tv"], 1))
        for k, v in us.items():
            line[k + "_us"] = round(v, 1)
            if k in bytes_of:
                line[k + "_gbytes_per_s"] = round(bytes_of[k] / v * 1e-3, 1)
        print(json.dumps(line), flush=True)


def step(name="config3", warm=10, reps=40):
    """The whole train_step (no density control, no read-back) with and without the key, alternating."""
    N, Wd, Hd, L, _ = scene.WORKLOADS[name]
    cam = raster.device_camera(scene.make_camera(Wd, Hd, 0))
    gt = torch.rand(Hd, Wd, 3, device="cuda")
    cfg = dict(adaptive_control_start=10 ** 9, reset_opacity_start=10 ** 9, add_sh_band_interval=10 ** 9, max_sh_band=L,
               use_background=False, max_gaussians=2 * N)
    dp = raster.device_params(scene.make_workload_gaussians(name))
    runs = {}
    for key, keys in (("plain", {}), ("bilagrid_1x1x1", dict(bilagrid=True, bilagrid_shape=(1, 1, 1))),
                      ("bilagrid_16x16x8", dict(bilagrid=True))):
        runs[key] = trainer_mod.Trainer({k: v.clone() for k, v in dp.items()}, [(cam, gt)], dict(cfg, **keys), scene_extent=5.0)
    times = {k: [] for k in runs}
    for rep in range(warm + reps):
        for key, t in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.train_step(cam, gt, want_loss=False, view_index=0)
            e1.record()
            torch.cuda.synchronize()
            if rep >= warm:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    out = dict(workload=name, gaussians=N, width=Wd, height=Hd)
    out.update({f"train_step_{k}_us": round(float(np.median(v)), 1) for k, v in times.items()})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    kernels()
    if "--no-step" not in sys.argv[1:]:
        step()

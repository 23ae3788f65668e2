"""The feature losses (gsplat_feature_ce_loss, gsplat_feature_l1_loss, gsplat_feature_cosine_loss) at 1920x1080 and
C = 3, 16 and 64 by events, warm, beside what a caller did before they existed, in the same session: the torch expression
of the same loss with autograd producing the same gradient map (log_softmax + nll_loss with ignore_index; the masked L1
mean; the masked cosine) -- forward and backward timed together, since the kernels produce both in one launch.  With the
algorithmic bytes of a launch (map read once, gradient written once, labels or target and validity read once) the achieved
bytes per second are printed.  Then the feature column's Adam step at 1e6 gaussians with half the rows visible, and the
whole training step at 1e6 gaussians (config3) with features: 16 against the plain step.
Warm: 10 calls before the 50 that count; medians.

usage: python tools/time_feature_loss.py [--no-step]   (JSON lines on stdout)"""
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

CHANNELS = (3, 16, 64)
H, W = 1080, 1920
WEIGHT = 1.0


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


def torch_ce(fmap, labels):
    x = fmap.detach().requires_grad_(True)
    loss = torch.nn.functional.nll_loss(torch.log_softmax(x.reshape(-1, x.shape[-1]), -1), labels.reshape(-1).long(),
                                        ignore_index=-1, reduction="sum") * (WEIGHT / labels.numel())
    loss.backward()
    return x.grad


def torch_l1(fmap, target, valid):
    x = fmap.detach().requires_grad_(True)
    loss = ((x - target).abs() * valid[..., None]).sum() * (WEIGHT / x.numel())
    loss.backward()
    return x.grad


def torch_cosine(fmap, target, valid):
    x = fmap.detach().requires_grad_(True)
    cos = torch.nn.functional.cosine_similarity(x, target, dim=-1, eps=0.0)
    loss = ((1.0 - cos) * valid).sum() * (WEIGHT / valid.numel())
    loss.backward()
    return x.grad


def losses():
    rng = np.random.default_rng(5)
    P = H * W
    for C in CHANNELS:
        fmap = torch.as_tensor(rng.uniform(-3, 3, (H, W, C)).astype(np.float32)).cuda()
        target = torch.as_tensor(rng.uniform(-3, 3, (H, W, C)).astype(np.float32)).cuda()
        labels = rng.integers(0, C, (H, W)).astype(np.int32)
        labels[rng.random((H, W)) < 0.25] = -1
        labels = torch.as_tensor(labels).cuda()
        labels64 = labels.long()  # (the conversion is not charged to torch)
        valid = torch.as_tensor((rng.random((H, W)) > 0.25).astype(np.uint8)).cuda()
        validf = valid.float()
        grad = torch.empty(H, W, C, device="cuda")
        part = float((labels >= 0).float().mean())
        share = float(validf.mean())
        # bytes a launch has to move: a pixel that takes no part is not read, its gradient row is still written
        algorithmic = dict(ce=P * 4 + P * C * 4 * (part + 1.0), l1=P + P * C * 4 * (2 * share + 1.0),
                           cosine=P + P * C * 4 * (2 * share + 1.0))
        runs = dict(ce=(lambda: ops.feature_ce_loss(fmap, labels, WEIGHT, grad),
                        lambda: torch_ce(fmap, labels64)),
                    l1=(lambda: ops.feature_l1_loss(fmap, target, WEIGHT, grad, valid=valid),
                        lambda: torch_l1(fmap, target, validf)),
                    cosine=(lambda: ops.feature_cosine_loss(fmap, target, WEIGHT, grad, valid=valid),
                            lambda: torch_cosine(fmap, target, validf)))
        for kind, (kernel, baseline) in runs.items():
            kernel()
            err = float((grad - baseline()).abs().max())  # the two compute the same thing
            k_us, t_us = by_events(kernel), by_events(baseline)
            k_loss_us = by_events(lambda: {"ce": ops.feature_ce_loss, "l1": ops.feature_l1_loss,
                                           "cosine": ops.feature_cosine_loss}[kind](
                fmap, labels if kind == "ce" else target, WEIGHT, grad, **({} if kind == "ce" else dict(valid=valid)),
                blocking=True))
            print(json.dumps(dict(loss=kind, width=W, height=H, channels=C, kernel_us=round(k_us, 2),
                                  kernel_with_loss_readback_us=round(k_loss_us, 2), torch_autograd_us=round(t_us, 2),
                                  torch_over_kernel=round(t_us / k_us, 2), algorithmic_bytes=int(algorithmic[kind]),
                                  kernel_gbytes_per_s=round(algorithmic[kind] / k_us * 1e-3, 1),
                                  max_abs_difference_to_torch=err)), flush=True)


def adam(N=1000000, C=16):
    rng = np.random.default_rng(6)
    rows = torch.as_tensor(np.sort(rng.permutation(N)[: N // 2]).astype(np.int32)).cuda()
    f, m, v = (torch.zeros(N, C, device="cuda") for _ in range(3))
    g = torch.as_tensor(rng.standard_normal((N, C)).astype(np.float32)).cuda()
    us = by_events(lambda: ops.feature_adam_step(rows, N // 2, f, m, v, g, 0.0025, 0.9, 0.999, 1e-8, 0.1, 0.001))
    moved = (N // 2) * C * 4 * 8  # features, two moments and the gradient, read and written
    print(json.dumps(dict(feature_adam_step_us=round(us, 2), gaussians=N, visible=N // 2, channels=C, bytes=moved,
                          gbytes_per_s=round(moved / us * 1e-3, 1))), flush=True)


def step(name="config3", C=16, warm=10, reps=40):
    """The whole train_step (no density control, no read-back) with and without the feature term, alternating."""
    N, Wd, Hd, L, _ = scene.WORKLOADS[name]
    cam = raster.device_camera(scene.make_camera(Wd, Hd, 0))
    gt = torch.rand(Hd, Wd, 3, device="cuda")
    labels = torch.randint(-1, C, (Hd, Wd), dtype=torch.int32, device="cuda")
    cfg = dict(adaptive_control_start=10 ** 9, reset_opacity_start=10 ** 9, add_sh_band_interval=10 ** 9, max_sh_band=L,
               use_background=False, max_gaussians=2 * N)
    dp = raster.device_params(scene.make_workload_gaussians(name))
    runs = {}
    for key, keys in (("plain", {}), ("features", dict(features=C)), ("features_geometry", dict(features=C, feature_geometry=True))):
        runs[key] = trainer_mod.Trainer({k: v.clone() for k, v in dp.items()}, [(cam, gt)], dict(cfg, **keys), scene_extent=5.0)
    times = {k: [] for k in runs}
    for rep in range(warm + reps):
        for key, t in runs.items():
            extra = {} if key == "plain" else dict(feature_target=labels)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.train_step(cam, gt, want_loss=False, **extra)
            e1.record()
            torch.cuda.synchronize()
            if rep >= warm:
                times[key].append(e0.elapsed_time(e1) * 1e3)
    out = dict(workload=name, gaussians=N, width=Wd, height=Hd, channels=C)
    out.update({f"train_step_{k}_us": round(float(np.median(v)), 1) for k, v in times.items()})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    losses()
    adam()
    if "--no-step" not in sys.argv[1:]:
        step()

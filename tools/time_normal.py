"""The four normal-map launches (gsplat_depth_to_normal, gsplat_normal_prior_loss, gsplat_normal_smoothness_loss,
gsplat_depth_to_normal_backward) by events on the maps of a workload's depth-mode forward, and the whole step -- forward,
the four launches, backward -- against the same step in depth mode alone (constant gradient maps) and the plain step, the
three alternating in one process.  Medians of `rounds` x `steps` steps.

usage: python tools/time_normal.py [workload ...]   (default: config3; JSON lines on stdout)"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
raster = importlib.import_module("3dgs_amd.raster")
scene = importlib.import_module("3dgs_amd.scene")
ops = importlib.import_module("3dgs_amd.ops")

MODES = ("plain", "depth", "normal")


def run(name, rounds=6, steps=20):
    N, W, H, L, _ = scene.WORKLOADS[name]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_workload_gaussians(name))
    cam = scene.make_camera(W, H, 0)
    dc = raster.device_camera(cam)
    intr = ops.pixel_intrinsics(cam)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    rng = np.random.default_rng(3)
    gd, ga = (torch.as_tensor(rng.uniform(-1, 1, (H, W)).astype(np.float32) / (W * H)).cuda() for _ in range(2))
    image = torch.as_tensor(rng.uniform(0, 1, (H, W, 3)).astype(np.float32)).cuda()
    prior = torch.as_tensor(rng.normal(size=(H, W, 3)).astype(np.float32)).cuda()
    normal, g_normal = (torch.empty(H, W, 3, device="cuda") for _ in range(2))
    nd, na = torch.empty(H, W, device="cuda"), torch.empty(H, W, device="cuda")
    ctxs = {}
    for mode in MODES:
        ctx = raster.RasterContext(N, W, H)
        if mode != "plain":
            ctx.set_depth(True, inverse=True)
        ctxs[mode] = (ctx, ctx.alloc_gradients(N, L))

    launches = dict(
        depth_to_normal=lambda f: ops.depth_to_normal(f, intr, True, out=normal),
        normal_prior_loss=lambda f: ops.normal_prior_loss(normal, prior, 0.2, g_normal),
        normal_smoothness_loss=lambda f: ops.normal_smoothness_loss(normal, image, 0.2, g_normal, accumulate=True),
        depth_to_normal_backward=lambda f: ops.depth_to_normal_backward(f, intr, True, g_normal, nd, na))

    def step(mode):
        ctx, grads = ctxs[mode]
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        sub = {k: v[:f["num_culled"]] for k, v in grads.items()}
        kw = {}
        if mode == "depth":
            kw = dict(grad_depth=gd, grad_alpha=ga)
        if mode == "normal":
            for fn in launches.values():
                fn(f)
            kw = dict(grad_depth=nd, grad_alpha=na)
        ctx.backward_pass(dp, dc, gi, c["bg"], L, sub, **kw)
        return f

    for mode in MODES:
        for _ in range(10):
            f = step(mode)
    has = (normal != 0).any(-1)
    print(json.dumps(dict(workload=name, width=W, height=H, pixels_with_a_normal=int(has.sum()))))
    # the launches one by one, by events, on the last forward's maps (f is the normal mode's)
    each = {}
    for k, fn in launches.items():
        ts = []
        for rep in range(60):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(f)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 10:
                ts.append(e0.elapsed_time(e1) * 1e3)
        each[k] = float(np.median(ts))
    print(json.dumps(dict(workload=name, launch_us={k: round(v, 2) for k, v in each.items()},
                          four_launches_us=round(sum(each.values()), 2))))
    wall = {m: [] for m in MODES}
    for r in range(rounds):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(mode)
            torch.cuda.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {m: float(np.median(v)) for m, v in wall.items()}
    print(json.dumps(dict(workload=name, step_ms={m: round(v, 4) for m, v in med.items()},
                          step_normal_vs_depth=round(med["normal"] / med["depth"], 4),
                          step_normal_vs_plain=round(med["normal"] / med["plain"], 4),
                          step_depth_vs_plain=round(med["depth"] / med["plain"], 4))))


if __name__ == "__main__":
    for name in sys.argv[1:] or ["config3"]:
        run(name)

"""Stage times of a plain, a depth-mode and an inverse-depth + second-moment (gsplat_context_set_depth_mode(1, 1)) forward +
backward, the three alternating in one process, through the context's per-stage timing (set_timing / get_timing: the
dispatches' own stamps); plus the whole step's wall time.  Medians of `rounds` x `steps` steps.  The baseline of the new
mode is depth mode and the plain step measured next to it, never the new mode alone.

usage: python tools/time_depth_moment.py [workload ...]   (default: config3 veiled1200k; JSON lines on stdout)"""
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

MODES = ("plain", "depth", "moment")


def run(name, rounds=6, steps=20):
    N, W, H, L, _ = scene.WORKLOADS[name]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_workload_gaussians(name))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    rng = np.random.default_rng(3)
    gd, ga, gq = (torch.as_tensor(rng.uniform(-1, 1, (H, W)).astype(np.float32) / (W * H)).cuda() for _ in range(3))
    ctxs = {}
    for mode in MODES:
        ctx = raster.RasterContext(N, W, H)
        if mode == "depth":
            ctx.set_depth(True)
        if mode == "moment":
            ctx.set_depth(True, inverse=True, moment=True)
        ctxs[mode] = (ctx, ctx.alloc_gradients(N, L))
    kws = dict(plain={}, depth=dict(grad_depth=gd, grad_alpha=ga), moment=dict(grad_depth=gd, grad_alpha=ga, grad_depth2=gq))

    def step(mode):
        ctx, grads = ctxs[mode]
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        sub = {k: v[:f["num_culled"]] for k, v in grads.items()}
        ctx.backward_pass(dp, dc, gi, c["bg"], L, sub, **kws[mode])

    for mode in MODES:
        for _ in range(10):
            step(mode)
    stages = {m: {} for m in MODES}
    wall = {m: [] for m in MODES}
    for r in range(rounds):
        for mode in MODES:
            ctx = ctxs[mode][0]
            ctx.set_timing(True)
            for _ in range(steps):
                step(mode)
            t = ctx.get_timing()
            ctx.set_timing(False)
            for k, (ms, n) in t.items():
                if n:
                    stages[mode].setdefault(k, []).append(ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(mode)
            torch.cuda.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {}
    for mode in MODES:
        med[mode] = {k: float(np.median(v)) for k, v in stages[mode].items()}
        med[mode]["step_ms"] = float(np.median(wall[mode]))
        print(json.dumps(dict(workload=name, mode=mode, **{k: round(v, 4) for k, v in med[mode].items()})))
    ratio = lambda a, b, k: round(med[a][k] / med[b][k], 4)
    print(json.dumps(dict(workload=name,
                          forward_moment_vs_depth=ratio("moment", "depth", "render_forward"),
                          backward_moment_vs_depth=ratio("moment", "depth", "render_backward"),
                          step_moment_vs_plain=ratio("moment", "plain", "step_ms"),
                          step_moment_vs_depth=ratio("moment", "depth", "step_ms"),
                          step_depth_vs_plain=ratio("depth", "plain", "step_ms"))))


if __name__ == "__main__":
    for name in sys.argv[1:] or ["config3", "veiled1200k"]:
        run(name)

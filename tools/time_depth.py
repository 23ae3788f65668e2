"""Stage times of a plain vs a depth-mode forward + backward (gsplat_context_set_depth), alternating the two in one
process, through the context's per-stage timing (set_timing / get_timing); plus the whole step's wall time.

usage: python tools/time_depth.py [workload ...]   (default: config3 veiled1200k; JSON lines on stdout)"""
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


def run(name, rounds=6, steps=20):
    N, W, H, L, _ = scene.WORKLOADS[name]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_workload_gaussians(name))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    rng = np.random.default_rng(3)
    gd = torch.as_tensor(rng.uniform(-1, 1, (H, W)).astype(np.float32) / (W * H)).cuda()
    ga = torch.as_tensor(rng.uniform(-1, 1, (H, W)).astype(np.float32) / (W * H)).cuda()
    ctxs = {}
    for depth in (False, True):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_depth(depth)
        ctxs[depth] = (ctx, ctx.alloc_gradients(N, L))

    def step(depth):
        ctx, grads = ctxs[depth]
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        sub = {k: v[:f["num_culled"]] for k, v in grads.items()}
        kw = dict(grad_depth=gd, grad_alpha=ga) if depth else {}
        ctx.backward_pass(dp, dc, gi, c["bg"], L, sub, **kw)

    for depth in (False, True):
        for _ in range(10):
            step(depth)
    stages = {False: {}, True: {}}
    wall = {False: [], True: []}
    for r in range(rounds):
        for depth in (False, True):
            ctx = ctxs[depth][0]
            ctx.set_timing(True)
            for _ in range(steps):
                step(depth)
            t = ctx.get_timing()
            ctx.set_timing(False)
            for k, (ms, n) in t.items():
                if n:
                    stages[depth].setdefault(k, []).append(ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(depth)
            torch.cuda.synchronize()
            wall[depth].append((time.perf_counter() - t0) * 1e3 / steps)
    for depth in (False, True):
        out = {k: round(float(np.median(v)), 4) for k, v in stages[depth].items()}
        out["step_ms"] = round(float(np.median(wall[depth])), 4)
        print(json.dumps(dict(workload=name, depth=depth, **out)))
    p = {k: float(np.median(v)) for k, v in stages[False].items()}
    d = {k: float(np.median(v)) for k, v in stages[True].items()}
    comp = (d["render_forward"] + d["render_backward"]) / (p["render_forward"] + p["render_backward"])
    print(json.dumps(dict(workload=name, render_fwd_plus_bwd_ratio=round(comp, 4),
                          step_ratio=round(float(np.median(wall[True]) / np.median(wall[False])), 4))))


if __name__ == "__main__":
    for name in sys.argv[1:] or ["config3", "veiled1200k"]:
        run(name)

"""Cost of anti-aliased mode (gsplat_context_set_antialiased): a forward + backward with the mode off and on, alternating
the two in one process.  Stage times come from the context's per-stage timing (set_timing / get_timing: preprocess and
preprocess_backward, the two kernels the mode instantiates, are stamped by their own dispatches), the whole step from the
wall clock around synchronised blocks of steps.  The compositing stages are printed too: the mode dims sub-pixel splats,
so their footprints and lists shrink and those stages may get FASTER.

Under a kernel trace the script is the thing to run as it is -- the mode's instantiations of preprocess_kernel and
preprocess_bwd_kernel are the ones with a trailing `true` template argument:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_antialias.py config3 veiled1200k

usage: python tools/time_antialias.py [workload ...]   (default: config3 veiled1200k; JSON lines on stdout)"""
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
    ctxs = {}
    for mode in (False, True):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_antialiased(mode)
        ctxs[mode] = (ctx, ctx.alloc_gradients(N, L))

    def step(mode):
        ctx, grads = ctxs[mode]
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        sub = {k: v[:f["num_culled"]] for k, v in grads.items()}
        ctx.backward_pass(dp, dc, gi, c["bg"], L, sub)

    for mode in (False, True):
        for _ in range(10):
            step(mode)
    stages = {False: {}, True: {}}
    wall = {False: [], True: []}
    for r in range(rounds):
        for mode in (False, True):
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
    for mode in (False, True):
        out = {k: round(float(np.median(v)), 4) for k, v in stages[mode].items()}
        out["step_ms"] = round(float(np.median(wall[mode])), 4)
        out["step_ms_series"] = [round(x, 4) for x in wall[mode]]
        print(json.dumps(dict(workload=name, antialiased=mode, **out)))
    ratio = lambda k: round(float(np.median(stages[True][k]) / np.median(stages[False][k])), 4)
    print(json.dumps(dict(workload=name, preprocess_ratio=ratio("preprocess"),
                          preprocess_backward_ratio=ratio("preprocess_backward"),
                          step_ratio=round(float(np.median(wall[True]) / np.median(wall[False])), 4))))


if __name__ == "__main__":
    for name in sys.argv[1:] or ["config3", "veiled1200k"]:
        run(name)

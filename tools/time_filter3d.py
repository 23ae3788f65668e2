"""Cost of the 3D smoothing filter (gsplat_context_set_filter3d): a forward + backward with the mode off and on,
alternating the two in one process, the way tools/time_depth.py does for depth.  The whole step comes from the wall clock
around synchronised blocks of steps; the two added passes (filter3d_apply_kernel in front of the forward,
filter3d_apply_bwd_kernel behind the per-gaussian backward) are also timed by themselves with device events around the
stand-alone operators on the same arrays.  Under a kernel trace the script is the thing to run as it is:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_filter3d.py config3 1

usage: python tools/time_filter3d.py [workload [rounds]]   (default: config3 6; JSON lines on stdout)"""
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


def run(name, rounds=6, steps=20):
    N, W, H, L, _ = scene.WORKLOADS[name]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_workload_gaussians(name))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    cams = ops.camera_arrays([scene.make_camera(W, H, k) for k in range(8)])
    filt = ops.compute_filter3d(dp["xyz"], *cams, near=0.2)
    ctxs = {}
    for mode in (False, True):
        ctx = raster.RasterContext(N, W, H)
        ctx.set_filter3d(filt if mode else None)
        ctxs[mode] = (ctx, ctx.alloc_gradients(N, L))

    def step(mode):
        ctx, grads = ctxs[mode]
        f = ctx.rasterize_image(dp, dc, c, c["bg"], L)
        sub = {k: v[:f["num_culled"]] for k, v in grads.items()}
        ctx.backward_pass(dp, dc, gi, c["bg"], L, sub)
        return f

    for mode in (False, True):
        for _ in range(10):
            f = step(mode)
    M, rows = f["num_culled"], f["compact_to_global"].clone()
    wall = {False: [], True: []}
    for r in range(rounds):
        for mode in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(mode)
            torch.cuda.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e3 / steps)

    def events(fn, reps=200):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    se, oe = torch.empty_like(dp["scale"]), torch.empty_like(dp["opacity"])
    g_s, g_o = torch.randn(M, 3, device="cuda"), torch.randn(M, device="cuda")
    out = dict(workload=name, gaussians=N, visible=M, cameras=8,
               compute_filter3d_ms=round(events(lambda: ops.compute_filter3d(dp["xyz"], *cams, near=0.2, out=filt), 50), 4),
               apply_ms=round(events(lambda: ops.filter3d_apply(dp["scale"], dp["opacity"], filt, se, oe)), 4),
               apply_backward_ms=round(events(lambda: ops.filter3d_apply_backward(dp["scale"], dp["opacity"], filt, g_s, g_o, rows)), 4))
    for mode in (False, True):
        out["step_ms_on" if mode else "step_ms_off"] = round(float(np.median(wall[mode])), 4)
        out["series_on" if mode else "series_off"] = [round(x, 4) for x in wall[mode]]
    out["step_ratio"] = round(float(np.median(wall[True]) / np.median(wall[False])), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    run(sys.argv[1] if len(sys.argv) > 1 else "config3", int(sys.argv[2]) if len(sys.argv) > 2 else 6)

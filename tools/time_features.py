"""The three feature-map launches (gsplat_context_render_features, gsplat_context_lift_features,
gsplat_context_features_backward) at C = 3, 16 and 64 by events on a workload's recorded forward, beside the
accumulate_contributions call on the same forward (the same walk, reduced per gaussian) and the context's own
render_forward and render_backward stages (per-stage timing).  Warm: 10 calls before the 50 that count; medians.

usage: python tools/time_features.py [workload ...]   (default: config3, 1e6 gaussians at 1920x1080; JSON lines on stdout)"""
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
raster = importlib.import_module("3dgs_amd.raster")
scene = importlib.import_module("3dgs_amd.scene")

CHANNELS = (3, 16, 64)


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


def run(name):
    N, W, H, L, _ = scene.WORKLOADS[name]
    c = scene.CONFIG
    dp = raster.device_params(scene.make_workload_gaussians(name))
    dc = raster.device_camera(scene.make_camera(W, H, 0))
    ctx = raster.RasterContext(N, W, H)
    ctx.set_timing(True, stages=("render_forward",))
    for _ in range(30):
        fwd = ctx.rasterize_image(dp, dc, c, 0.0, L)
    torch.cuda.synchronize()
    forward_us = ctx.get_timing()["render_forward"][0] * 1e3
    ctx.set_timing(False)
    fwd = ctx.rasterize_image(dp, dc, c, 0.0, L)
    rng = np.random.default_rng(3)
    weight_sum = torch.zeros(N, device="cuda")
    out = dict(workload=name, gaussians=N, width=W, height=H, visible=int(fwd["num_culled"]), list_entries=int(fwd["num_splats"]),
               render_forward_us=round(forward_us, 2),
               accumulate_contributions_us=round(by_events(lambda: ctx.accumulate_contributions(weight_sum=weight_sum)), 2))
    for C in CHANNELS:
        feats = torch.as_tensor(rng.uniform(-1, 1, (N, C)).astype(np.float32)).cuda()
        fmap = torch.as_tensor(rng.uniform(-1, 1, (H, W, C)).astype(np.float32)).cuda()
        image, lifted = torch.empty(H, W, C, device="cuda"), torch.zeros(N, C, device="cuda")
        out[f"render_features_C{C}_us"] = round(by_events(lambda: ctx.render_features(feats, out=image)), 2)
        out[f"lift_features_C{C}_us"] = round(by_events(lambda: ctx.lift_features(fmap, lifted)), 2)
    # the feature map's gradient with respect to the geometry, behind a compositing backward of the same forward (which
    # is timed by the context's own render_backward stage, beside it)
    gi = torch.as_tensor(scene.make_grad_image(W, H)).cuda()
    ctx.set_timing(True, stages=("render_backward",))
    for _ in range(30):
        ctx.rasterize_image(dp, dc, c, 0.0, L)
        ctx.backward_render(gi, 0.0)
    torch.cuda.synchronize()
    out["render_backward_us"] = round(ctx.get_timing()["render_backward"][0] * 1e3, 2)
    ctx.set_timing(False)
    for C in CHANNELS:
        feats = torch.as_tensor(rng.uniform(-1, 1, (N, C)).astype(np.float32)).cuda()
        gmap = torch.as_tensor(rng.uniform(-1, 1, (H, W, C)).astype(np.float32)).cuda()
        out[f"features_backward_C{C}_us"] = round(by_events(lambda: ctx.features_backward(feats, gmap)), 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    for name in sys.argv[1:] or ["config3"]:
        run(name)

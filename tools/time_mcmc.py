"""Per-iteration cost of the MCMC densification mode (config key mcmc): the two kernels every iteration runs, timed by
themselves with device events at the workload's gaussian count, and the Trainer's step with the mode off and on,
alternating in one process the way tools/time_filter3d.py does (wall clock around synchronised blocks of steps).

The mode runs the optimizer step behind the backward (the GSPLAT_FUSED_ADAM=0 choreography), so the step is timed three
ways on the same scene: off as the environment has it, off with the stored-gradient step forced, and on.  The difference
of the last two is what the regulariser and the noise add; the first two differ by the choreography.  No refinement step
falls into the timed window (that cost is paid once per adaptive_control_interval iterations and is reported apart).

mcmc_add_noise is timed twice: on the workload's opacities, where the gate closes for most rows and they are left after
one load, and with every gaussian transparent, where each row moves (56 bytes per gaussian).

usage: python tools/time_mcmc.py [workload [rounds]]   (default: config3 6; one JSON line on stdout)"""
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
trainer_mod = importlib.import_module("3dgs_amd.trainer")


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


def run(name, rounds=6, steps=20):
    N, W, H, L, _ = scene.WORKLOADS[name]
    truth = scene.make_workload_gaussians(name)
    dp = raster.device_params(truth)
    ctx = raster.RasterContext(N, W, H)
    views = []
    for v in range(4):
        cam = raster.device_camera(scene.make_camera(W, H, v))
        views.append((cam, ctx.rasterize_image(dp, cam, scene.CONFIG, 0.0, L)["image"].clone()))
    M = int(ctx.rasterize_image(dp, views[0][0], scene.CONFIG, 0.0, L)["num_culled"])
    del ctx

    # ---- the two kernels by themselves
    xyz = dp["xyz"].clone()
    open_gate = torch.full_like(dp["opacity"], -6.0)
    scaler = 5e5 * 8e-4 * 1e-3  # mcmc_noise_lr * a position learning rate, scaled down: 200 steps must not move the scene
    rows = torch.randperm(N, device="cuda")[:M].sort().values.to(torch.int32)
    g_o, g_s = torch.zeros(M, device="cuda"), torch.zeros(M, 3, device="cuda")
    moving = float((torch.sigmoid(dp["opacity"]) < 0.893).float().mean())
    out = dict(workload=name, gaussians=N, visible=M, rows_with_open_gate=round(moving, 4),
               add_noise_ms=round(events(lambda: ops.mcmc_add_noise(xyz, dp["opacity"], dp["scale"], dp["quaternion"], scaler, 7)), 4),
               add_noise_all_moving_ms=round(events(lambda: ops.mcmc_add_noise(xyz, open_gate, dp["scale"], dp["quaternion"], scaler, 7)), 4),
               regularize_ms=round(events(lambda: ops.mcmc_regularize(rows, dp["opacity"], dp["scale"], 1e-8, 1e-8, g_o, g_s)), 4))
    out["add_noise_all_moving_GBps"] = round(56.0 * N / out["add_noise_all_moving_ms"] / 1e6, 1)
    out["regularize_GBps"] = round(52.0 * M / out["regularize_ms"] / 1e6, 1)  # 4 index + 16 read + 16 read + 16 written
    del xyz, open_gate, rows, g_o, g_s

    # ---- the Trainer's step: off (as the environment has it), off with the stored-gradient step, on
    cfg = dict(adaptive_control_start=10 ** 9, reset_opacity_start=10 ** 9, add_sh_band_interval=10 ** 9, max_sh_band=L,
               use_background=False, max_gaussians=2 * N)
    init = {k: v.clone() for k, v in dp.items()}
    init["rgb"] = init["rgb"] * 0.9  # something to learn

    def make(mode):
        t = trainer_mod.Trainer({k: v.clone() for k, v in init.items()}, views, dict(cfg, mcmc=(mode == "on")),
                                scene_extent=5.0, seed=3)
        if mode == "off_stored":
            t.fused_adam = 0
        return t

    modes = ("off", "off_stored", "on")
    trainers = {m: make(m) for m in modes}

    def block(t):
        for _ in range(steps):
            cam, gt = views[t.draw_views()[0]]
            t.train_step(cam, gt, want_loss=False)

    for m in modes:
        block(trainers[m])
    wall = {m: [] for m in modes}
    for r in range(rounds):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            block(trainers[m])
            torch.cuda.synchronize()
            wall[m].append((time.perf_counter() - t0) * 1e3 / steps)
    for m in modes:
        out[f"step_ms_{m}"] = round(float(np.median(wall[m])), 4)
        out[f"series_{m}"] = [round(x, 4) for x in wall[m]]
    out["fused_adam_off"] = trainers["off"].fused_adam
    out["on_minus_off_stored_ms"] = round(out["step_ms_on"] - out["step_ms_off_stored"], 4)
    out["on_over_off"] = round(out["step_ms_on"] / out["step_ms_off"], 4)

    # ---- one refinement step (relocation of the dead, 5 % growth, Morton re-order), by the wall clock
    t = trainers["on"]
    t.params["opacity"][:: 50] = -8.0  # 2 % dead
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    relocated, added = t.mcmc_relocate(), t.mcmc_grow()
    t.sort_gaussians()
    torch.cuda.synchronize()
    out.update(refinement_ms=round((time.perf_counter() - t0) * 1e3, 2), relocated=relocated, added=added)
    print(json.dumps(out))


if __name__ == "__main__":
    run(sys.argv[1] if len(sys.argv) > 1 else "config3", int(sys.argv[2]) if len(sys.argv) > 2 else 6)

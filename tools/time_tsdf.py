"""TSDF fusion and mesh extraction by events, medians of warm runs (JSON lines on stdout):

  integrate   gsplat_tsdf_integrate at 256^3 and 512^3, with and without colour, 1920x1080 maps of an analytic sphere seen
              from 16 cameras on a ring, integrated in calls of 1, 2, 4, 8 and 16 views: per-view time, and the
              volume's nominal traffic (one read and one write of tsdf, weight and colour per pass of 8 views) per second
              against the 6.3 TB/s copy rate; the same
              update as a torch expression (index arithmetic plus gather, float64) for one view in the same session
  extract     ops.tsdf_extract (mark, two prefix sums, the read-back, emit) on the sphere fused from those views
  dataset     Trainer.extract_mesh over the training views of a generated dataset (tools/make_colmap_dataset.py) at
              resolution 256 and 512, wall clock, from its SfM-initialised gaussians

usage: python tools/time_tsdf.py [integrate] [extract] [dataset=<root>/<name>] [sizes=256,512]"""
import importlib
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("3dgs_amd.ops")
W, H = 1920, 1080
COPY_RATE = 6.3e12  # bytes/s, the measured device copy rate


def events(fn, reps=12, warm=3, calls=1):
    """ms per call: the median over the warm repetitions of `calls` back-to-back calls between two events (several calls
    keep the device busy where one call is shorter than the host's work to issue it)."""
    ts = []
    for rep in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warm:
            ts.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ts))


def ring_cameras(K):
    """K cameras on a ring of radius 3 around the origin looking inwards -> view [K,12], intrinsics [K,4] (60 degrees)."""
    view, intr = np.empty((K, 12), np.float32), np.empty((K, 4), np.float32)
    fx = W / (2.0 * math.tan(math.radians(30.0)))
    for v in range(K):
        a = 2.0 * math.pi * v / K + 0.1
        eye = np.array([3.0 * math.cos(a), 0.4 * math.sin(2 * a), 3.0 * math.sin(a)])
        f = -eye / np.linalg.norm(eye)
        r = np.cross(f, np.array([0.0, -1.0, 0.0]))
        r /= np.linalg.norm(r)
        R = np.stack([r, np.cross(f, r), f])
        view[v] = np.concatenate([R, (-R @ eye)[:, None]], 1).reshape(12)
        intr[v] = (fx, fx, W / 2.0, H / 2.0)
    return view, intr


def sphere_maps(view, intr, radius=1.0):
    """depth (z of the unit sphere along every pixel's ray), T (0 on the sphere, 1 off it) and a colour image, on the GPU."""
    K = len(view)
    depth = torch.zeros(K, H, W, device="cuda")
    T = torch.ones(K, H, W, device="cuda")
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float64),
                          torch.arange(W, device="cuda", dtype=torch.float64), indexing="ij")
    for v in range(K):
        m = torch.as_tensor(view[v].astype(np.float64)).cuda().reshape(3, 4)
        fx, fy, cx, cy = (float(s) for s in intr[v])
        ray = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)], -1)  # camera space, z = 1
        c = m[:, 3]  # the sphere's centre (the origin) in camera space
        a, b, cc = (ray * ray).sum(-1), (ray * c).sum(-1), (c * c).sum() - radius * radius
        disc = b * b - a * cc
        hit = disc > 0
        z = (b - torch.sqrt(disc.clamp_min(0))) / a
        depth[v] = torch.where(hit, z, torch.zeros_like(z)).float()
        T[v] = torch.where(hit, torch.zeros_like(z), torch.ones_like(z)).float()
    image = torch.rand(K, H, W, 3, device="cuda")
    return depth, T, image


def torch_update(vol, depth, T, image, view, intr, trunc, alpha_min=0.5):
    """One view of the integration rule as a torch expression (float64 index arithmetic, gathers, where)."""
    nx, ny, nz = vol["dims"]
    o, h = vol["origin"], vol["voxel"]
    dev = vol["tsdf"].device
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float64), torch.arange(ny, device=dev, dtype=torch.float64),
                             torch.arange(nx, device=dev, dtype=torch.float64), indexing="ij")
    px, py, pz = o[0] + h * i, o[1] + h * j, o[2] + h * k
    m = [float(s) for s in view]
    fx, fy, cx, cy = (float(s) for s in intr)
    z = m[8] * px + m[9] * py + m[10] * pz + m[11]
    zs = torch.where(z > 0, z, torch.ones_like(z))
    fu = torch.floor(fx * (m[0] * px + m[1] * py + m[2] * pz + m[3]) / zs + cx + 0.5)
    fv = torch.floor(fy * (m[4] * px + m[5] * py + m[6] * pz + m[7]) / zs + cy + 0.5)
    live = (z > 0) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    pix = (torch.where(live, fv, torch.zeros_like(fv)) * W + torch.where(live, fu, torch.zeros_like(fu))).long()
    A = 1.0 - T.reshape(-1)[pix].double()
    d = depth.reshape(-1)[pix].double()
    live &= (A >= alpha_min) & (d > 0)
    s = d / A.clamp_min(1e-30) - z
    live &= s >= -trunc
    val = (s / trunc).clamp_max(1.0)
    w = vol["weight"].double()
    vol["tsdf"] = torch.where(live, ((w * vol["tsdf"].double() + val) / (w + 1.0)).float(), vol["tsdf"])
    if vol["color"] is not None:
        c = image.reshape(-1, 3)[pix].double()
        vol["color"] = torch.where(live[..., None], ((w[..., None] * vol["color"].double() + c) / (w[..., None] + 1.0)).float(),
                                   vol["color"])
    vol["weight"] = torch.where(live, (w + 1.0).float(), vol["weight"])


def time_integrate(sizes):
    view, intr = ring_cameras(16)
    depth, T, image = sphere_maps(view, intr)
    per_pass = importlib.import_module("3dgs_amd._lib").load().gsplat_tsdf_views_per_pass()
    for n in sizes:
        for color in (False, True):
            vol = ops.tsdf_volume((-1.5, -1.5, -1.5), 3.0 / (n - 1), (n, n, n), color=color)
            node_bytes = 2 * (8 + (12 if color else 0))  # read + write
            for B in (1, 2, 4, 8, 16):  # the same 16 views every time, B per call
                chunks = [(depth[i:i + B], T[i:i + B], view[i:i + B], intr[i:i + B], image[i:i + B] if color else None)
                          for i in range(0, 16, B)]

                def all_views():
                    for d, t, vw, it, im in chunks:
                        ops.tsdf_integrate(vol, d, t, vw, it, image=im, max_weight=64.0)

                ms = events(all_views)
                # nominal: every node read and written once per pass (a node no view of the pass updates is not written)
                traffic = n ** 3 * node_bytes * len(chunks) * math.ceil(B / per_pass)
                print(json.dumps(dict(what="integrate", grid=n, color=color, views=16, batch=B, total_ms=round(ms, 4),
                                      per_view_ms=round(ms / 16, 4),
                                      nominal_grid_TB_per_s=round(traffic / (ms * 1e-3) / 1e12, 3),
                                      of_copy_rate=round(traffic / (ms * 1e-3) / COPY_RATE, 3))), flush=True)
            ms = events(lambda: torch_update(vol, depth[0], T[0], image[0], view[0], intr[0], 4.0 * vol["voxel"]), reps=5, warm=2)
            print(json.dumps(dict(what="integrate_torch", grid=n, color=color, K=1, per_view_ms=round(ms, 3))), flush=True)
            del vol
            torch.cuda.empty_cache()


def time_extract(sizes):
    view, intr = ring_cameras(16)
    depth, T, image = sphere_maps(view, intr)
    for n in sizes:
        vol = ops.tsdf_volume((-1.5, -1.5, -1.5), 3.0 / (n - 1), (n, n, n), color=True)
        ops.tsdf_integrate(vol, depth, T, view, intr, image=image)
        out = []
        ms = events(lambda: out.__setitem__(slice(None), ops.tsdf_extract(vol)), reps=8, warm=2)
        r = np.linalg.norm(out[0].double().cpu().numpy(), axis=1)
        print(json.dumps(dict(what="extract", grid=n, ms=round(ms, 3), vertices=int(out[0].shape[0]), faces=int(out[1].shape[0]),
                              radius_error_voxels_max=round(float(np.abs(r - 1.0).max() / vol["voxel"]), 4))), flush=True)
        del vol, out
        torch.cuda.empty_cache()


def time_dataset(base, sizes):
    dataset = importlib.import_module("3dgs_amd.dataset")
    app = importlib.import_module("3dgs_amd.app")
    raster = importlib.import_module("3dgs_amd.raster")
    trainer = importlib.import_module("3dgs_amd.trainer")
    sparse = os.path.join(base, "sparse", "0")
    cameras = dataset.ReadCamerasBinary(os.path.join(sparse, "cameras.bin"), 4)
    images = dataset.ReadImagesBinary(os.path.join(sparse, "images.bin"), base + "/", 4)
    _, xyz, rgb = dataset.ReadPoints3DArrays(os.path.join(sparse, "points3D.bin"))
    params = ops.initialize_gaussians(torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda())
    ordered = sorted(images.values(), key=lambda im: im["name"])
    cams = [raster.device_camera(app.camera_from_colmap(cameras[im["camera_id"]], im)) for im in ordered]
    gt = torch.zeros(cams[0]["height"], cams[0]["width"], 3, device="cuda")
    t = trainer.Trainer(params, [(c, gt) for c in cams], None, scene_extent=1.1 * dataset.computeMaxDiagonal(images))
    box = ((-2.5, -2.0, -2.5), (2.5, 0.5, 2.5))
    for n in sizes:
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = t.extract_mesh(resolution=n, bounds=box)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        print(json.dumps(dict(what="extract_mesh", views=len(cams), width=int(cams[0]["width"]), height=int(cams[0]["height"]),
                              gaussians=t.num_gaussians, resolution=n, dims=got["volume"]["dims"], wall_s=round(wall, 3),
                              vertices=int(got["vertices"].shape[0]), faces=int(got["faces"].shape[0]))), flush=True)
        del got
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:] or ["integrate", "extract"]
    sizes = [256, 512]
    for a in args:
        if a.startswith("sizes="):
            sizes = [int(s) for s in a[6:].split(",")]
    for a in args:
        if a == "integrate":
            time_integrate(sizes)
        elif a == "extract":
            time_extract(sizes)
        elif a.startswith("dataset="):
            time_dataset(a[8:], sizes)

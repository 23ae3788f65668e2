"""Median depth and the mesh component filter by events, medians of warm runs (JSON lines on stdout):

  median      gsplat_context_median_depth (thresholds 0.5 and 0.9, with and without the index map) on a workload's recorded
              forward, beside accumulate_contributions on the same forward (the same walk, reduced per gaussian with
              atomics) and the context's own render_forward stage (per-stage timing)
  filter      ops.mesh_components and ops.mesh_filter(keep_largest=50) on the sphere mesh extracted from a 512^3 volume
              (tools/time_tsdf.py's sphere), beside ops.tsdf_extract of that volume; and on that mesh with 2000 floaters
              (small tetrahedra) appended
  dataset     Trainer.extract_mesh over the training views of a generated dataset (tools/make_colmap_dataset.py), wall
              clock, depth expected and median, with and without keep_largest=50, with the face and component counts

usage: python tools/time_mesh.py [median[=workload]] [filter] [dataset=<root>/<name>] [sizes=512]"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ops = importlib.import_module("3dgs_amd.ops")
raster = importlib.import_module("3dgs_amd.raster")
scene = importlib.import_module("3dgs_amd.scene")


def by_events(fn, warm=10, reps=50):
    """microseconds per call: the median over `reps` calls after `warm` that do not count"""
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


def time_median(name):
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
    weight_sum = torch.zeros(N, device="cuda")
    depth = torch.empty(H, W, device="cuda")
    index = torch.empty(H, W, dtype=torch.int32, device="cuda")
    out = dict(what="median", workload=name, gaussians=N, width=W, height=H, visible=int(fwd["num_culled"]),
               list_entries=int(fwd["num_splats"]), render_forward_us=round(forward_us, 2),
               accumulate_contributions_us=round(by_events(lambda: ctx.accumulate_contributions(weight_sum=weight_sum)), 2))
    for threshold in (0.5, 0.9):
        out[f"median_depth_{threshold}_us"] = round(by_events(lambda: ctx.median_depth(threshold, out=depth)), 2)
        out[f"median_depth_{threshold}_index_us"] = round(by_events(lambda: ctx.median_depth(threshold, out=depth, index=index)), 2)
        out[f"surface_pixels_{threshold}"] = int((index >= 0).sum())
        out[f"mean_index_{threshold}"] = round(float(index[index >= 0].float().mean()), 2)
    out["mean_stop_index"] = round(float(fwd["n"].float().mean()), 2)
    print(json.dumps(out), flush=True)


def floaters(vertices, faces, colors, num, seed=5):
    """`num` small tetrahedra scattered around the mesh, appended -> (vertices, faces, colors)"""
    rng = np.random.default_rng(seed)
    centre = torch.as_tensor(rng.uniform(-1.4, 1.4, (num, 1, 3)).astype(np.float32)).cuda()
    corner = torch.as_tensor((0.01 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])).astype(np.float32)).cuda()
    v = (centre + corner[None]).reshape(-1, 3)
    tet = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32, device="cuda")
    f = (tet[None] + 4 * torch.arange(num, dtype=torch.int32, device="cuda")[:, None, None]).reshape(-1, 3) + len(vertices)
    return (torch.cat([vertices, v]).contiguous(), torch.cat([faces, f.int()]).contiguous(),
            torch.cat([colors, torch.full_like(v, 0.5)]).contiguous())


def time_filter(sizes):
    tsdf = importlib.import_module("time_tsdf")
    view, intr = tsdf.ring_cameras(16)
    depth, T, image = tsdf.sphere_maps(view, intr)
    for n in sizes:
        vol = ops.tsdf_volume((-1.5, -1.5, -1.5), 3.0 / (n - 1), (n, n, n), color=True)
        ops.tsdf_integrate(vol, depth, T, view, intr, image=image)
        extract_us = by_events(lambda: ops.tsdf_extract(vol), warm=2, reps=6)
        mesh = ops.tsdf_extract(vol)
        del vol
        torch.cuda.empty_cache()
        for label, (v, f, c) in (("sphere", mesh), ("sphere + 2000 floaters", floaters(*mesh, 2000))):
            comp = ops.mesh_components(f, len(v))
            got = ops.mesh_filter(v, f, c, keep_largest=50)
            print(json.dumps(dict(
                what="filter", grid=n, mesh=label, vertices=len(v), faces=len(f), extract_us=round(extract_us, 1),
                mesh_components_us=round(by_events(lambda: ops.mesh_components(f, len(v)), warm=3, reps=12), 1),
                mesh_filter_keep50_us=round(by_events(lambda: ops.mesh_filter(v, f, c, keep_largest=50), warm=3, reps=12), 1),
                rounds=comp["rounds"], report=got[3])), flush=True)
        del mesh
        torch.cuda.empty_cache()


def time_dataset(base, sizes):
    dataset = importlib.import_module("3dgs_amd.dataset")
    app = importlib.import_module("3dgs_amd.app")
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
        for depth, keep in (("expected", 0), ("expected", 50), ("median", 0), ("median", 50)):
            for rep in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = t.extract_mesh(resolution=n, bounds=box, depth=depth, keep_largest=keep)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
            print(json.dumps(dict(what="extract_mesh", views=len(cams), width=int(cams[0]["width"]),
                                  height=int(cams[0]["height"]), gaussians=t.num_gaussians, resolution=n, depth=depth,
                                  keep_largest=keep, wall_s=round(wall, 3), vertices=int(got["vertices"].shape[0]),
                                  faces=int(got["faces"].shape[0]), filter=got["filter"])), flush=True)
            del got
            torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:] or ["median", "filter"]
    sizes = [512]
    for a in args:
        if a.startswith("sizes="):
            sizes = [int(s) for s in a[6:].split(",")]
    for a in args:
        if a == "median" or a.startswith("median="):
            time_median(a[7:] or "config3")
        elif a == "filter":
            time_filter(sizes)
        elif a.startswith("dataset="):
            time_dataset(a[8:], sizes)

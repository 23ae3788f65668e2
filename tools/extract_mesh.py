#!/usr/bin/env python3
"""A triangle mesh from a trained scene: the scene's depth maps from the COLMAP cameras of a dataset are fused into a TSDF
volume and its zero level set is written as a binary PLY (Trainer.extract_mesh).

    python tools/extract_mesh.py <scene.ply|scene.npz> <dataset root> <out.ply>
        [--resolution 256] [--bounds x0 y0 z0 x1 y1 z1] [--trunc T] [--max-depth D] [--downsample 1] [--no-color]
        [--depth expected|median] [--median-threshold 0.5] [--min-component-faces 0] [--keep-largest 0]

<dataset root> holds sparse/0/{cameras,images}.bin.  Without --bounds the box is the cube around the mean camera position
with the cameras' extent as half-side, which suits an object the cameras surround; a real capture wants an explicit box.
--depth median fuses the median depth (the gaussian at which the transmittance falls through --median-threshold) instead of
the expected depth; --min-component-faces / --keep-largest drop connected components from the mesh before it is written."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("dataset")
    ap.add_argument("out")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--trunc", type=float, default=None)
    ap.add_argument("--max-depth", type=float, default=None)
    ap.add_argument("--downsample", type=int, default=1)
    ap.add_argument("--no-color", action="store_true")
    ap.add_argument("--depth", choices=("expected", "median"), default="expected")
    ap.add_argument("--median-threshold", type=float, default=0.5)
    ap.add_argument("--min-component-faces", type=int, default=0)
    ap.add_argument("--keep-largest", type=int, default=0)
    args = ap.parse_args(argv)

    import torch
    compress = importlib.import_module("3dgs_amd.compress")
    dataset = importlib.import_module("3dgs_amd.dataset")
    app = importlib.import_module("3dgs_amd.app")
    raster = importlib.import_module("3dgs_amd.raster")
    trainer = importlib.import_module("3dgs_amd.trainer")
    if not torch.cuda.is_available():
        print("error: no GPU (the HIP path has no CPU fallback)", file=sys.stderr)
        return 1
    scene = compress.load_scene(args.scene)
    params = raster.device_params({k: v for k, v in scene.items() if k != "l_max"})
    sparse = os.path.join(args.dataset, "sparse", "0")
    cameras = dataset.ReadCamerasBinary(os.path.join(sparse, "cameras.bin"), args.downsample)
    images = dataset.ReadImagesBinary(os.path.join(sparse, "images.bin"), args.dataset.rstrip("/") + "/", args.downsample)
    ordered = sorted(images.values(), key=lambda im: im["name"])
    cams = [raster.device_camera(app.camera_from_colmap(cameras[im["camera_id"]], im)) for im in ordered]
    blank = torch.zeros(1, 1, 3, device="cuda")  # (the views of a Trainer are (camera, image) pairs; nothing reads the image here)
    t = trainer.Trainer(params, [(c, blank) for c in cams], None, scene_extent=1.1 * dataset.computeMaxDiagonal(images))
    bounds = None if args.bounds is None else (args.bounds[:3], args.bounds[3:])
    got = t.extract_mesh(path=args.out, resolution=args.resolution, bounds=bounds, trunc=args.trunc,
                         max_depth=args.max_depth, color=not args.no_color, depth=args.depth,
                         median_threshold=args.median_threshold, min_component_faces=args.min_component_faces,
                         keep_largest=args.keep_largest)
    vol = got["volume"]
    if got["filter"] is not None:
        f = got["filter"]
        print(f"filter: kept {f['kept']} of {f['components']} components, removed {f['faces_removed']} faces and "
              f"{f['vertices_removed']} vertices")
    print(f"{args.out}: {got['vertices'].shape[0]} vertices, {got['faces'].shape[0]} faces from {len(cams)} views; "
          f"volume {vol['dims'][0]}x{vol['dims'][1]}x{vol['dims'][2]} nodes of {vol['voxel']:.6g} at "
          f"{np.round(vol['origin'], 4).tolist()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

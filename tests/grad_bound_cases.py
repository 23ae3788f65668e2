"""The scenes of tests/test_grad_bound_cpu.py and tests/test_grad_bound_gpu.py, and the comparison both make: a set of
gradient arrays (the float32 oracle's on the CPU, the HIP kernels' on the GPU) against the float64 terms that
tests/render_bwd_reference.py derives from the SAME forward record."""
import numpy as np

import edge_scenes
import grad_bound
import render_bwd_reference as rbr
from conftest import pkg

# name -> (N, W, H, l_max, view); the basic sizes of the issue
BASIC = {"tiny_v0": ("tiny", 0), "tiny_v2": ("tiny", 2), "small_v0": ("small", 0), "small_v2": ("small", 2),
         "sh0": (3000, 200, 120, 0, 3), "sh1": (3000, 200, 120, 1, 3), "sh2": (3000, 200, 120, 2, 3),
         "odd_1": (1, 17, 9, 0, 1), "odd_37": (37, 100, 7, 2, 1), "odd_257": (257, 130, 66, 3, 1)}
SCENES = tuple(BASIC) + ("culled", "long", "edge", "depth")
# got-array name -> (reference term, key of oracle.backward_pass, key of RasterContext gradients)
ARRAYS = (("precompute_rgb", "rgb_pre", "precompute_rgb"), ("opacity", "opacity", "opacity"), ("conic", "conic", "conic"),
          ("uv", "uv", "uv"), ("leaf_xyz", "xyz", "xyz"), ("leaf_band0", "band0", "rgb"), ("leaf_sh", "sh", "sh"),
          ("leaf_scale", "scale", "scale"), ("leaf_quaternion", "quaternion", "quaternion"))
EDGE_FWD_SEED = 0x3D65 + 105  # scene.SEED + 105: 0.44 % (seeds + 102 .. + 109 give 0.44 % .. 0.95 %: large splats sit near integers)
_CACHE = {}


def long_list_scene(scene):
    """The scene of test_fused_gpu.test_long_lists_split_into_segments_for_the_backward."""
    N, W, H, L = 24000, 160, 96, 1
    params = scene.make_gaussians(N, W, H, L)
    cam = scene.make_camera(W, H)
    rng = np.random.default_rng(11)
    for lo, hi, (cu, cv), spread in ((2000, 4200, (24.0, 24.0), 5.0), (4200, 9200, (88.0, 40.0), 7.0),
                                     (9200, 16200, (136.0, 72.0), 4.0), (16200, 18200, (40.0, 72.0), 3.0)):
        k = hi - lo
        z = rng.uniform(3.0, 9.0, k)
        u, v = cu + rng.uniform(-spread, spread, k), cv + rng.uniform(-spread, spread, k)
        params["xyz"][lo:hi, 0] = (u - W / 2) * z / cam["fx"]
        params["xyz"][lo:hi, 1] = (v - H / 2) * z / cam["fy"]
        params["xyz"][lo:hi, 2] = z
        params["scale"][lo:hi] = np.log(rng.uniform(0.004, 0.012, (k, 3)))
        params["opacity"][lo:hi] = rng.choice([-5.0, -4.0, -3.0, -1.0, 3.0], size=k, p=[0.45, 0.3, 0.15, 0.08, 0.02])
    return params, cam, L


def depth_maps(W, H, seed=3):
    """dL/d depth and dL/d alpha, non-zero everywhere (tests/test_depth_gpu.py: _maps)."""
    rng = np.random.default_rng(seed)
    gd = (rng.uniform(0.2, 1.0, (H, W)) * rng.choice([-1.0, 1.0], (H, W)) / (W * H)).astype(np.float32)
    ga = (rng.uniform(0.2, 1.0, (H, W)) * rng.choice([-1.0, 1.0], (H, W)) / (W * H)).astype(np.float32)
    return gd, ga


def make(name):
    """dict params cam L W H cfg bg gi pops (global rows per population, or None) gd ga (depth mode, or None)."""
    if name in _CACHE:
        return _CACHE[name]
    scene = pkg("scene")
    cfg, pops, gd, ga = dict(scene.CONFIG), None, None, None
    if name in BASIC:
        spec = BASIC[name]
        N, W, H, L, view = (scene.WORKLOADS[spec[0]][:4] + (spec[1],)) if len(spec) == 2 else spec
        params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, view)
    elif name in ("culled", "depth"):
        N, W, H, L = scene.WORKLOADS["small"][:4]
        params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 2)
        if name == "culled":
            params = scene.cull_half(params)
        else:
            gd, ga = depth_maps(W, H)
    elif name == "long":
        params, cam, L = long_list_scene(scene)
    elif name in ("edge", "edge_fwd"):
        # edge_fwd: the same populations from another seed, for tests/test_forward_bound_*.py -- with the default seed
        # 0.53 % of the rows have a pre-ceil radius within its bar of an integer, above the 0.5 % those tests allow
        params, cam, pops = edge_scenes.make_edge_scene("small", None if name == "edge" else EDGE_FWD_SEED)
        L = edge_scenes.SIZES["small"][3]
        cfg = dict(near_thresh=0.3, mh_dist=3.0, cull_mask_padding=100, bg=0.5)
    else:
        raise KeyError(name)
    W, H = int(cam["width"]), int(cam["height"])
    _CACHE[name] = dict(name=name, params=params, cam=cam, L=L, W=W, H=H, cfg=cfg, bg=cfg["bg"],
                        gi=scene.make_grad_image(W, H), pops=pops, gd=gd, ga=ga)
    return _CACHE[name]


def visible_leaves(case, rows):
    """The float32 leaf parameters of the visible rows (global indices `rows`) in compacted order."""
    p, L = case["params"], case["L"]
    out = {"xyz": p["xyz"][rows], "band0": p["rgb"][rows], "opacity": p["opacity"][rows], "scale": p["scale"][rows],
           "quaternion": p["quaternion"][rows], "sh": None}
    if L > 0:
        nc = (L + 1) ** 2
        out["sh"] = np.asarray(p["sh"]).reshape(len(p["xyz"]), -1)[:, :(nc - 1) * 3][rows]
    return out


def terms(case, record, rows, z=None, checkpoints=None):
    """The float64 terms for a forward record (uv conic rgb sorted ranges n T as produced) whose compacted rows are the
    global indices `rows`; opacity and the leaves come from the input parameters.  z: the record's camera-space depths
    (depth mode).  checkpoints: dict(image, entries, split_min) when the backward walked long lists in segments."""
    leaves = visible_leaves(case, rows)
    rec = {k: np.asarray(record[k]) for k in ("uv", "conic", "rgb", "sorted", "ranges", "n", "T")}
    rec["opacity"] = leaves["opacity"]
    t = rbr.bound_terms(rec, leaves, case["cam"], case["gi"], case["bg"], case["L"], case["cfg"]["mh_dist"],
                        case["gd"], case["ga"], z if case["gd"] is not None else None, checkpoints)
    t["position"] = grad_bound.deepest_position(rec["sorted"], rec["ranges"], len(rows))
    t["rows"] = np.asarray(rows)
    return t


def oracle_case(case, orc):
    """The float32 oracle's forward and backward of a scene and the float64 terms of that record (computed once)."""
    if "oracle" in case:
        return case["oracle"]
    import depth_reference
    cfg = case["cfg"]
    ref = orc.rasterize(case["params"], case["cam"], cfg["near_thresh"], cfg["mh_dist"], cfg["cull_mask_padding"],
                        case["bg"], case["L"], threads=8)
    rows = np.nonzero(ref["mask"])[0]
    if len(rows) == 0:
        case["oracle"] = None
        return None
    tf = edge_scenes.backward_tan_fov(case["cam"])
    if case["gd"] is None:
        bref = orc.backward_pass(ref, case["cam"], case["gi"], case["bg"], case["L"], threads=8, tan_fov=tf)
    else:
        bref = depth_reference.backward_pass(orc, ref, case["cam"], case["gi"], case["gd"], case["ga"], case["bg"],
                                             case["L"], threads=8)
    case["oracle"] = dict(ref=ref, bref=bref, rows=rows, terms=terms(case, ref, rows, ref["xyz_c"][:, 2]))
    return case["oracle"]


def populations_of(case, rows):
    """population name -> compacted rows, or None."""
    if case["pops"] is None:
        return None
    slot = {int(g): i for i, g in enumerate(rows)}
    return {k: np.array([slot[int(g)] for g in v if int(g) in slot], np.int64) for k, v in case["pops"].items()}


def compare(t, got):
    """got: name -> array for the names of ARRAYS (+ "z").  Returns name -> the worst ratio (grad_bound.observed_K)."""
    return {name: grad_bound.observed_K(arr, *t[name]) for name, arr in got.items() if arr is not None and name in t}


def oracle_arrays(bref):
    got = {name: bref.get(key) for name, key, _ in ARRAYS}
    if "z" in bref:
        got["z"] = bref["z"]
    return got

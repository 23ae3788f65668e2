"""The scenes of tests/test_features_bwd_cpu.py and tests/test_features_bwd_gpu.py and what both feed the feature
backward: columns of ONE seeded 35-channel array per scene (tests/feature_reference.py: seeded_rows, the seeds of
tests/test_features_gpu.py), so that the C-channel case is the first C columns."""
import numpy as np

import feature_reference as fr
from conftest import pkg

CMAX = 35
# scene -> the channel count its K_obs and its loose share are measured at (the widest the GPU tests run on it)
TABLE_CHANNELS = {"tiny": CMAX, "partial": CMAX, "small": 16, "long": 4}
_CACHE = {}


def make(name):
    """dict N W H L params cam cfg feats [N,CMAX] (global order) gmap [H,W,CMAX]."""
    if name in _CACHE:
        return _CACHE[name]
    scene = pkg("scene")
    if name == "partial":  # 70 x 45: partial tiles in both directions
        N, W, H, L = 300, 70, 45, 1
        params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
    elif name == "long":   # 32 x 32, one list of ~2400 entries
        from test_contribution_gpu import _long_list_scene
        N, W, H, L, params, cam = _long_list_scene(scene)
    else:
        N, W, H, L = scene.WORKLOADS[name][:4]
        params, cam = scene.make_gaussians(N, W, H, L), scene.make_camera(W, H, 0)
    _CACHE[name] = dict(name=name, N=N, W=W, H=H, L=L, params=params, cam=cam, cfg=dict(scene.CONFIG),
                        feats=fr.seeded_rows(N, CMAX, 21), gmap=fr.seeded_rows(H * W, CMAX, 22).reshape(H, W, CMAX))
    return _CACHE[name]


def oracle_forward(case, orc):
    """The float32 oracle's forward of the scene at background 0 (computed once) and its visible rows."""
    if "ref" not in case:
        c = case["cfg"]
        case["ref"] = orc.rasterize(case["params"], case["cam"], c["near_thresh"], c["mh_dist"], c["cull_mask_padding"], 0.0,
                                    case["L"], threads=8)
        case["rows"] = np.nonzero(np.asarray(case["ref"]["mask"]))[0]
    return case["ref"], case["rows"]


def record_of(fwd, opacity):
    """The forward record the references walk: uv conic sorted ranges n T as produced, `opacity` the logits the forward
    composited, in compacted order."""
    rec = {k: np.asarray(fwd[k]) for k in ("uv", "conic", "sorted", "ranges", "n", "T")}
    rec["opacity"] = np.asarray(opacity)
    return rec


def visible_leaves(case, rows, params=None):
    p, L = params or case["params"], case["L"]
    out = {"xyz": p["xyz"][rows], "band0": p["rgb"][rows], "opacity": p["opacity"][rows], "scale": p["scale"][rows],
           "quaternion": p["quaternion"][rows], "sh": None}
    if L > 0:
        nc = (L + 1) ** 2
        out["sh"] = np.asarray(p["sh"]).reshape(len(p["xyz"]), -1)[:, :(nc - 1) * 3][rows]
    return out

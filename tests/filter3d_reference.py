"""Float64 numpy references for the 3D smoothing filter (include/gsplat_hip.h: gsplat_compute_filter3d,
gsplat_filter3d_apply, gsplat_filter3d_apply_backward), written from the definitions, and the scene the CPU and GPU
tests share."""
import numpy as np

MARGIN = 0.15
VARIANCE = 0.2  # Mip-Splatting's s: filter3d = sqrt(0.2) * min z / focal


def project(cam, xyz):
    """(zc, u, v) in float64 by gs::camera_space and gs::to_screen's expressions."""
    view = np.asarray(cam["view"], np.float64).reshape(4, 4)
    proj = np.asarray(cam["proj"], np.float64).reshape(4, 4)
    x = np.asarray(xyz, np.float64)
    c = x @ view[:3, :3].T + view[:3, 3]
    x_clip = c @ proj[0, :3] + proj[0, 3]
    y_clip = c @ proj[1, :3] + proj[1, 3]
    w_clip = c @ proj[3, :3] + proj[3, 3]
    with np.errstate(all="ignore"):
        u = (x_clip / (w_clip + 1e-6) * 0.5 + 0.5) * float(cam["width"])
        v = (y_clip / (w_clip + 1e-6) * 0.5 + 0.5) * float(cam["height"])
    return c[:, 2], u, v


def _bounds(cam):
    W, H = float(cam["width"]), float(cam["height"])
    return (-MARGIN * W, (1 + MARGIN) * W), (-MARGIN * H, (1 + MARGIN) * H)


def sampled_by(cam, xyz, near):
    z, u, v = project(cam, xyz)
    (u0, u1), (v0, v1) = _bounds(cam)
    return (z > near) & (u >= u0) & (u <= u1) & (v >= v0) & (v <= v1), z


def compute_filter3d(xyz, cams, near):
    """(filter3d [N], sampled [N] bool, sampled_by [V,N] bool)."""
    n = len(xyz)
    t = np.full(n, np.inf)
    per_cam = np.zeros((len(cams), n), bool)
    for k, cam in enumerate(cams):
        s, z = sampled_by(cam, xyz, near)
        per_cam[k] = s
        t = np.where(s, np.minimum(t, z / float(cam["fx"])), t)
    sampled = per_cam.any(0)
    fill = t[sampled].max() if sampled.any() else 0.0
    return np.sqrt(VARIANCE) * np.where(sampled, t, fill), sampled, per_cam


def fragile(xyz, cams, near, rel=1e-4):
    """Gaussians whose sampling decision a float32 evaluation may take the other way: for some camera zc - near, or u or v
    against a margin bound, lies within `rel` relative of the boundary."""
    out = np.zeros(len(xyz), bool)
    for cam in cams:
        z, u, v = project(cam, xyz)
        out |= np.abs(z - near) <= rel * abs(near)
        for val, bounds in zip((u, v), _bounds(cam)):
            for b in bounds:
                out |= np.abs(val - b) <= rel * abs(b)
    return out


def _log_terms(scale, opacity, f):
    """log f, d = scale - scale_eff [n,3], log o, 1 - o, all without cancellation; rows with f == 0: d = 0."""
    scale, x, f = np.asarray(scale, np.float64), np.asarray(opacity, np.float64), np.asarray(f, np.float64)
    with np.errstate(divide="ignore"):
        lf = np.log(f)[:, None]
    d = -0.5 * np.logaddexp(0.0, 2.0 * (lf - scale))
    lo = -np.logaddexp(0.0, -x) + d.sum(1)
    return lf, d, lo, -np.expm1(lo)


def apply(scale, opacity, f):
    """(scale_eff [n,3], opacity_eff [n], o [n], rho3 [n]): scale_eff_k = 1/2 log(s_k^2 + f^2), o = sigmoid(opacity) rho3,
    opacity_eff = logit(o); f == 0 is the identity."""
    scale, x, f = np.asarray(scale, np.float64), np.asarray(opacity, np.float64), np.asarray(f, np.float64)
    lf, d, lo, om = _log_terms(scale, x, f)
    with np.errstate(all="ignore"):
        scale_eff = 0.5 * np.logaddexp(2.0 * scale, 2.0 * lf)
        op_eff = lo - np.log(om)
    off = f == 0
    scale_eff[off], op_eff[off] = scale[off], x[off]
    return scale_eff, op_eff, np.exp(lo), np.exp(d.sum(1))


def apply_backward(scale, opacity, f, g_scale, g_opacity):
    """(grad_scale, grad_opacity) from the gradients with respect to the effective values:
    grad_scale_k = g_s_k w_k + g_o (1 - w_k) / (1 - o), grad_opacity = g_o (1 - sigma) / (1 - o); both opacity factors 0
    where 1 - o == 0; f == 0 passes through."""
    scale, x, f = np.asarray(scale, np.float64), np.asarray(opacity, np.float64), np.asarray(f, np.float64)
    g_s, g_o = np.asarray(g_scale, np.float64), np.asarray(g_opacity, np.float64)
    lf, d, lo, om = _log_terms(scale, x, f)
    a = 2.0 * (scale - lf)
    with np.errstate(all="ignore"):
        w = np.exp(-np.logaddexp(0.0, -a))
        wc = np.exp(-np.logaddexp(0.0, a))
        k = np.where(om == 0, 0.0, g_o / om)
    one_minus_sigma = np.exp(-np.logaddexp(0.0, x))
    grad_scale = g_s * w + k[:, None] * wc
    grad_opacity = k * one_minus_sigma
    off = f == 0
    grad_scale[off], grad_opacity[off] = g_s[off], g_o[off]
    return grad_scale, grad_opacity


# ---------------------------------------------------------------- the shared scene
SCENE_SEED = 11
CAMERAS = ((200, 120, 1.0), (160, 96, 1.4), (256, 144, 1.2), (128, 128, 2.0), (320, 200, 0.5))  # (W, H, zoom); view k
NEAR = 0.2


def make_cameras(scene):
    """Five cameras of differing size and focal length: scene.make_camera's poses with the focal length (and the
    projection's two scale entries) multiplied by `zoom`.  The last one is the wide one."""
    cams = []
    for k, (W, H, zoom) in enumerate(CAMERAS):
        cam = scene.make_camera(W, H, k)
        cam["fx"], cam["fy"] = float(np.float32(cam["fx"] * zoom)), float(np.float32(cam["fy"] * zoom))
        cam["proj"] = cam["proj"].copy()
        cam["proj"][0] *= np.float32(zoom)
        cam["proj"][5] *= np.float32(zoom)
        cams.append(cam)
    return cams


def make_scene(scene, seed=SCENE_SEED):
    """(xyz [3000,3] float32, cameras, populations): 2400 gaussians in front of camera 0 and three populations of 200
    placed by construction -- behind every camera, in front but outside every camera's 15 % margin, and inside the wide
    camera's view only."""
    rng = np.random.default_rng(seed)
    base = scene.make_gaussians(2400, 200, 120, 0)["xyz"].astype(np.float64)
    n = 200
    z = rng.uniform(2.0, 12.0, (3, n))
    behind = np.stack([rng.uniform(-1, 1, n) * z[0], rng.uniform(-1, 1, n) * z[0], -z[0]], 1)
    side = rng.choice([-1.0, 1.0], n)
    outside = np.stack([side * rng.uniform(3.5, 5.0, n) * z[1], rng.uniform(-0.3, 0.3, n) * z[1], z[1]], 1)
    z2 = rng.uniform(6.0, 12.0, n)
    one = np.stack([rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 1.2, n) * z2, rng.uniform(-0.1, 0.1, n) * z2, z2], 1)
    xyz = np.concatenate([base, behind, outside, one]).astype(np.float32)
    order = rng.permutation(len(xyz))  # the populations interleave
    where = np.empty(len(xyz), np.int64)
    where[order] = np.arange(len(xyz))
    pops = dict(base=where[:2400], behind=where[2400:2600], outside=where[2600:2800], one=where[2800:3000])
    return np.ascontiguousarray(xyz[order]), make_cameras(scene), pops


def transform_rows(seed=3):
    """Rows for the transform and its chain rule, by population: scale [n,3], opacity [n], filter [n], populations.
    |inputs| <= 16; logits from -8 to 12."""
    rng = np.random.default_rng(seed)
    n = 600
    scale = rng.uniform(-6.0, 1.0, (4 * n, 3))
    mean = scale.mean(1)
    ratio = np.concatenate([rng.uniform(-9.0, -5.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.0, 7.0, n),
                            rng.uniform(-9.0, 1.0, n)])  # log(f / s): f << s, f ~ s, f >> s, high logits
    f = np.exp(mean + ratio)
    opacity = np.concatenate([rng.uniform(-8.0, 8.0, 3 * n), rng.uniform(8.0, 12.0, n)])
    zero = np.arange(0, 4 * n, 37)  # a row in 37 of every population has no filter
    f[zero] = 0.0
    idx = np.arange(4 * n)
    live = f > 0
    pops = {"f<<s": idx[:n][live[:n]], "f~s": idx[n:2 * n][live[n:2 * n]], "f>>s": idx[2 * n:3 * n][live[2 * n:3 * n]],
            "logit>8": idx[3 * n:][live[3 * n:]], "f=0": zero}
    return scale.astype(np.float32), opacity.astype(np.float32), f.astype(np.float32), pops

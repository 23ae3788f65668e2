"""Compressed scene files and the scene loader (numpy only; the k-means of the SH codebook is handed in).

The format follows "Compressed 3D Gaussian Splatting" (Niedermayr et al. 2024) and gsplat's PngCompression: the higher
SH bands -- 45 of the 59 parameters at degree 3 -- are vector-quantised into a codebook of up to 65 536 rows, everything
else is stored in 8 or 16 bits.  A scene is a dict of arrays, written with np.savez_compressed:

  version                int32[1]     FORMAT_VERSION
  l_max                  int32[1]     SH degree
  xyz_q                  uint16[N,3]  min-max per axis of t = sign(v) log1p(|v|) (gsplat's transform)
  rgb_q                  uint8[N,3]   min-max per column
  opacity_q              uint8[N]     min-max of the raw logit
  scale_q                uint8[N,3]   min-max per column of the raw (log) scale
  quaternion_q           uint8[N,4]   normalised, sign flipped so that w >= 0, over the fixed range [-1, 1]; (w, x, y, z)
  sh_index               uint16[N]    row of the codebook                       } absent at SH degree 0
  sh_codebook_q          uint8[K,3R]  min-max per column, R = (l_max + 1)^2 - 1 }
  <name>_lo, <name>_hi   float64      the ranges (xyz, rgb, opacity, scale, sh_codebook)

Min-max rule with L = 2^bits - 1: q = rint((v - lo) / (hi - lo) L), decoded as lo + q (hi - lo) / L in double and rounded
to float once; hi == lo stores q = 0 and decodes to lo exactly.  The codebook is fitted, quantised, decoded, and the rows
are then assigned once more against the DECODED codebook: the stored indices are nearest for what a loader sees.

19 bytes per gaussian at SH 3 (6 + 3 + 1 + 3 + 4 + 2) against the PLY's 248, plus a codebook of at most 2.9 MB, before
zlib; the trainer's Morton order is what gives zlib something to find in the position and index columns.
"""
import os

import numpy as np

FORMAT_VERSION = 1
_RANGED = ("xyz", "rgb", "opacity", "scale", "sh_codebook")


def quantise(v, bits, lo=None, hi=None):
    """Min-max quantisation per column (axis 0 is the row axis) -> (q, lo, hi); lo/hi float64 of shape v.shape[1:]."""
    v = np.asarray(v, np.float64)
    levels = float(2 ** bits - 1)
    if lo is None:
        lo = v.min(axis=0) if v.shape[0] else np.zeros(v.shape[1:])
        hi = v.max(axis=0) if v.shape[0] else np.zeros(v.shape[1:])
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span = hi - lo
    q = np.rint((v - lo) / np.where(span > 0, span, 1.0) * levels)
    q = np.where(span > 0, np.clip(q, 0.0, levels), 0.0)
    return q.astype(np.uint8 if bits <= 8 else np.uint16), lo, hi


def dequantise(q, bits, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + np.asarray(q, np.float64) * (hi - lo) / float(2 ** bits - 1)).astype(np.float32)


def _log_transform(v):
    v = np.asarray(v, np.float64)
    return np.sign(v) * np.log1p(np.abs(v))


def _log_inverse(t):
    return np.sign(t) * np.expm1(np.abs(t))


def _device_fit(x, K, iterations, seed):
    import torch
    from . import ops
    codebook, index, objective = ops.vq_fit(torch.as_tensor(x).cuda().contiguous(), int(K), iterations=int(iterations),
                                            seed=int(seed))
    return codebook.cpu().numpy(), index.cpu().numpy(), objective


def _device_assign(x, codebook):
    import torch
    from . import ops
    return ops.vq_assign(torch.as_tensor(x).cuda().contiguous(), torch.as_tensor(codebook).cuda().contiguous()).cpu().numpy()


def _l_max_of(sh, n):
    rest = 0 if sh is None else int(np.asarray(sh).size // max(n, 1))
    l_max = int(round(np.sqrt(rest // 3 + 1))) - 1
    if rest != 3 * ((l_max + 1) ** 2 - 1):
        raise ValueError(f"sh holds {rest} floats per gaussian: not 3 ((l_max + 1)^2 - 1)")
    return l_max


def encode(params, fit=None, assign=None, codebook_size=65536, iterations=10, seed=0):
    """params (xyz [N,3], rgb [N,3], opacity [N], scale [N,3], quaternion [N,4] as (w,x,y,z), sh [N,R,3] or None) -> the
    dict of arrays above.  fit(x, K, iterations, seed) -> (codebook [K',D], index [N], ...) and assign(x, codebook) ->
    index [N] on float32 numpy arrays; by default ops.vq_fit / ops.vq_assign on the device."""
    fit, assign = fit or _device_fit, assign or _device_assign
    if not isinstance(codebook_size, int) or not 1 <= codebook_size <= 65536:
        raise ValueError("codebook_size must be 1 .. 65536")
    xyz = np.asarray(params["xyz"], np.float32).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        raise ValueError("the scene has no gaussians")
    f32 = lambda k, w: np.asarray(params[k], np.float32).reshape(n, w)
    l_max = _l_max_of(params.get("sh"), n)
    out = dict(version=np.array([FORMAT_VERSION], np.int32), l_max=np.array([l_max], np.int32))
    out["xyz_q"], out["xyz_lo"], out["xyz_hi"] = quantise(_log_transform(xyz), 16)
    out["rgb_q"], out["rgb_lo"], out["rgb_hi"] = quantise(f32("rgb", 3), 8)
    out["opacity_q"], out["opacity_lo"], out["opacity_hi"] = quantise(f32("opacity", 1).reshape(n), 8)
    out["scale_q"], out["scale_lo"], out["scale_hi"] = quantise(f32("scale", 3), 8)
    q = f32("quaternion", 4).astype(np.float64)
    norm = np.sqrt((q ** 2).sum(1, keepdims=True))
    q = q / np.where(norm > 0, norm, 1.0)
    q = np.where(q[:, :1] < 0, -q, q)
    out["quaternion_q"] = quantise(q, 8, lo=-1.0, hi=1.0)[0]
    if l_max > 0:
        rows = np.ascontiguousarray(np.asarray(params["sh"], np.float32).reshape(n, -1))
        codebook = np.asarray(fit(rows, min(codebook_size, n), iterations, seed)[0], np.float32)
        out["sh_codebook_q"], out["sh_codebook_lo"], out["sh_codebook_hi"] = quantise(codebook, 8)
        seen = dequantise(out["sh_codebook_q"], 8, out["sh_codebook_lo"], out["sh_codebook_hi"])
        index = np.asarray(assign(rows, seen))
        if index.shape != (n,) or index.min() < 0 or index.max() >= len(codebook):
            raise ValueError("assign returned indices outside the codebook")
        out["sh_index"] = index.astype(np.uint16)
    return out


def decode(arrays):
    """The dict of arrays of encode / a loaded .npz -> params as float32 numpy (xyz, rgb, opacity, scale, quaternion, sh
    [N,R,3]) plus l_max."""
    version = int(np.asarray(arrays["version"]).reshape(-1)[0])
    if version != FORMAT_VERSION:
        raise ValueError(f"compressed scene format version {version}: this reader knows version {FORMAT_VERSION}")
    l_max = int(np.asarray(arrays["l_max"]).reshape(-1)[0])
    rng = lambda k: (arrays[k + "_lo"], arrays[k + "_hi"])
    t = np.asarray(arrays["xyz_q"], np.float64) * (np.asarray(arrays["xyz_hi"], np.float64) - arrays["xyz_lo"]) / 65535.0
    out = dict(xyz=_log_inverse(np.asarray(arrays["xyz_lo"], np.float64) + t).astype(np.float32),
               rgb=dequantise(arrays["rgb_q"], 8, *rng("rgb")),
               opacity=dequantise(arrays["opacity_q"], 8, *rng("opacity")),
               scale=dequantise(arrays["scale_q"], 8, *rng("scale")),
               quaternion=dequantise(arrays["quaternion_q"], 8, -1.0, 1.0))
    n = len(out["xyz"])
    if l_max > 0:
        codebook = dequantise(arrays["sh_codebook_q"], 8, *rng("sh_codebook"))
        out["sh"] = codebook[np.asarray(arrays["sh_index"], np.int64)].reshape(n, -1, 3)
    else:
        out["sh"] = np.zeros((n, 0, 3), np.float32)
    out["l_max"] = l_max
    return out


def save_scene(path, params, **encode_options):
    """encode(params, **encode_options) -> path (.npz, zlib-compressed); returns the arrays."""
    arrays = encode(params, **encode_options)
    with open(path, "wb") as f:  # a file object: np.savez would append ".npz" to another extension
        np.savez_compressed(f, **arrays)
    return arrays


def read_ply(path):
    """The file gsplat_save_ply writes (binary little-endian floats: x y z nx ny nz f_dc_0..2 f_rest_* opacity scale_0..2
    rot_0..3) -> params.  The writer stores its (w,x,y,z) input as (x,y,z,w) and Trainer.save_to_ply pre-rotates the columns
    for it, so rot_0..3 of a training run's file ARE the device order (w,x,y,z) and are taken as they stand; a file written
    with dataset.save_ply directly holds (x,y,z,w) and wants np.roll(quaternion, 1, axis=1) afterwards."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path} is not a PLY file")
        names, n, binary = [], None, False
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            w = line.decode("ascii", "replace").split()
            if w[:1] == ["end_header"]:
                break
            if w[:1] == ["format"]:
                binary = w[1:2] == ["binary_little_endian"]
            elif w[:2] == ["element", "vertex"]:
                n = int(w[2])
            elif w[:1] == ["element"]:
                raise ValueError(f"{path}: element {w[1]} is not part of a gaussian scene")
            elif w[:1] == ["property"]:
                if w[1] != "float":
                    raise ValueError(f"{path}: property {w[-1]} is {w[1]}, not float")
                names.append(w[2])
        rest = len(names) - 17
        want = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(rest)]
                + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
        if not binary or n is None or rest < 0 or names != want:
            raise ValueError(f"{path}: not the binary little-endian layout gsplat_save_ply writes")
        data = np.fromfile(f, "<f4", n * len(names))
    if data.size != n * len(names):
        raise ValueError(f"{path}: truncated")
    data = data.reshape(n, len(names)).astype(np.float32)
    l_max = _l_max_of(data[:, 9:9 + rest], n) if n else 0
    tail = data[:, 9 + rest:]
    return dict(xyz=data[:, 0:3].copy(), rgb=data[:, 6:9].copy(), sh=data[:, 9:9 + rest].reshape(n, -1, 3).copy(),
                opacity=tail[:, 0].copy(), scale=tail[:, 1:4].copy(), quaternion=tail[:, 4:8].copy(),
                l_max=l_max)


def load_scene(path):
    """A scene by extension: .npz (the compressed format above) or .ply (gsplat_save_ply's) -> the params dict Trainer
    takes, as float32 numpy, plus l_max."""
    ext = os.path.splitext(os.fspath(path))[1].lower()
    if ext == ".npz":
        with np.load(path) as z:
            return decode({k: z[k] for k in z.files})
    if ext == ".ply":
        return read_ply(path)
    raise ValueError(f"{path}: unknown scene file extension {ext!r} (.npz or .ply)")

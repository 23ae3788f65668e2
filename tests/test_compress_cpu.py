"""The compressed scene format and the scene loader (3dgs_amd/compress.py) without a device: the k-means is handed in from
tests/vq_reference.py, the decoder is compared with the reference decoder bit for bit, the PLY reader with the bytes
libgsplat_host.so's writer stored."""
import numpy as np
import pytest

import vq_reference as vqr
from conftest import pkg

N = 500


def _fit(x, K, iterations, seed):
    return vqr.fit(x, K, iterations=min(iterations, 3), seed=seed)


def _assign(x, c):
    return vqr.assign(x, c)[0]


def _params(scene, l_max, n=N):
    p = scene.make_gaussians(n, 160, 96, l_max)
    p["xyz"][:7, 0] *= -1.0  # both signs through the log transform
    return p


@pytest.fixture(scope="module")
def compress():
    return pkg("compress")


@pytest.fixture(scope="module")
def encoded(scene, compress):
    p = _params(scene, 3)
    return p, compress.encode(p, fit=_fit, assign=_assign, codebook_size=32, iterations=3, seed=1)


@pytest.mark.parametrize("bits", [8, 16])
def test_quantiser_round_trip_is_within_half_a_step(compress, bits):
    rng = np.random.default_rng(bits)
    v = (rng.standard_normal((1000, 5)) * [1e-3, 1.0, 50.0, 1.0, 1.0] + [0, 0, 7.0, -3.0, 0]).astype(np.float32)
    v[:, 4] = 0.37  # a constant column
    for mod in (compress, vqr):
        q, lo, hi = mod.quantise(v, bits)
        assert q.dtype == (np.uint8 if bits == 8 else np.uint16) and q.shape == v.shape
        assert (lo == v.min(0)).all() and (hi == v.max(0)).all()
        back = mod.dequantise(q, bits, lo, hi)
        assert back.dtype == np.float32
        # half a quantisation step, plus the one float32 rounding of the decoded value
        bound = (hi - lo) / (2.0 * (2 ** bits - 1)) * (1 + 1e-12) + np.abs(back) * 2.0 ** -24
        assert (np.abs(back.astype(np.float64) - v) <= bound).all()
        assert (q[:, 4] == 0).all() and (back[:, 4] == np.float32(0.37)).all()  # constant columns are exact
        assert q.min() == 0 and q.max() == 2 ** bits - 1
    a, b = compress.quantise(v, bits), vqr.quantise(v, bits)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_every_attribute_is_within_its_step(encoded, compress):
    p, arrays = encoded
    out = compress.decode(arrays)
    assert out["l_max"] == 3 and all(out[k].dtype == np.float32 for k in ("xyz", "rgb", "opacity", "scale", "quaternion", "sh"))
    assert {k: arrays[k].dtype for k in ("xyz_q", "rgb_q", "opacity_q", "scale_q", "quaternion_q", "sh_index",
                                         "sh_codebook_q")} == dict(xyz_q=np.uint16, rgb_q=np.uint8, opacity_q=np.uint8,
                                                                   scale_q=np.uint8, quaternion_q=np.uint8,
                                                                   sh_index=np.uint16, sh_codebook_q=np.uint8)
    for k, shape in (("rgb", (N, 3)), ("opacity", (N,)), ("scale", (N, 3))):
        v = p[k].astype(np.float64)
        step = (v.max(0) - v.min(0)) / 255.0
        assert out[k].shape == shape
        assert (np.abs(out[k] - v) <= step / 2 * (1 + 1e-12) + np.abs(out[k]) * 2.0 ** -24).all(), k
    # positions: half a step of the transformed value, carried through expm1 (derivative 1 + |v|; second order below 1e-9)
    v = p["xyz"].astype(np.float64)
    t = np.sign(v) * np.log1p(np.abs(v))
    step = (t.max(0) - t.min(0)) / 65535.0
    bound = (1 + np.abs(v)) * np.expm1(step / 2) * (1 + 1e-9) + np.abs(out["xyz"]) * 2.0 ** -24
    assert (np.abs(out["xyz"] - v) <= bound).all()
    assert (np.sign(out["xyz"][:7, 0]) == np.sign(p["xyz"][:7, 0])).all()


def test_quaternion_keeps_the_rotation(encoded, compress):
    p, arrays = encoded
    q = compress.decode(arrays)["quaternion"]
    assert (arrays["quaternion_q"][:, 0] >= 127).all() and (q[:, 0] >= -1 / 255).all()  # w >= 0 up to half a step
    unit = p["quaternion"].astype(np.float64)
    unit = unit / np.linalg.norm(unit, axis=1, keepdims=True)
    unit = np.where(unit[:, :1] < 0, -unit, unit)
    assert (np.abs(q - unit) <= 1 / 255 * (1 + 1e-12) + 2.0 ** -24).all()  # (w, x, y, z) stays in device order
    # as a rotation: every component off by at most e = 1/255.  An entry of the matrix is a quadratic form of the unit
    # quaternion whose gradient has 1-norm at most 2 sum|q_i| <= 4: 4 e; renormalising a quaternion whose norm is within
    # sum|q_i| e <= 2 e of one scales the entries (at most 1 in magnitude) by up to 1 +- 4 e: 8 e together, second order 9 e
    assert np.abs(vqr.rotation(q) - vqr.rotation(p["quaternion"])).max() <= 9 / 255
    assert (p["quaternion"][:, 0] < 0).any()  # the sign flip was exercised


def test_indices_are_nearest_for_the_decoded_codebook(encoded, compress):
    p, arrays = encoded
    book = vqr.dequantise(arrays["sh_codebook_q"], 8, arrays["sh_codebook_lo"], arrays["sh_codebook_hi"])
    assert book.shape == (32, 45)
    rows = p["sh"].reshape(N, -1)
    assert (arrays["sh_index"] == vqr.assign(rows, book)[0]).all()
    assert compress.decode(arrays)["sh"].tobytes() == book[arrays["sh_index"]].reshape(N, 15, 3).tobytes()


@pytest.mark.parametrize("l_max", [0, 1, 3])
def test_file_round_trip_equals_the_reference_decoder(scene, compress, tmp_path, l_max):
    p = _params(scene, l_max, 200)
    path = tmp_path / "scene.npz"
    arrays = compress.save_scene(path, p, fit=_fit, assign=_assign, codebook_size=16, iterations=2, seed=0)
    assert ("sh_index" in arrays) == (l_max > 0) and ("sh_codebook_q" in arrays) == (l_max > 0)
    loaded, direct, ref = compress.load_scene(path), compress.decode(arrays), vqr.decode(arrays)
    assert loaded["l_max"] == direct["l_max"] == ref["l_max"] == l_max
    for k in ("xyz", "rgb", "opacity", "scale", "quaternion", "sh"):
        assert loaded[k].dtype == np.float32 and loaded[k].shape == p[k].shape, k
        assert loaded[k].tobytes() == direct[k].tobytes() == ref[k].tobytes(), k


def test_codebook_is_clamped_to_the_gaussian_count(scene, compress):
    p = _params(scene, 1, 10)
    arrays = compress.encode(p, fit=_fit, assign=_assign, codebook_size=65536, iterations=1)
    assert arrays["sh_codebook_q"].shape == (10, 9)


def test_unknown_version_and_bad_arguments_are_refused(encoded, compress, tmp_path):
    p, arrays = encoded
    with pytest.raises(ValueError, match="version"):
        compress.decode(dict(arrays, version=np.array([compress.FORMAT_VERSION + 1], np.int32)))
    path = tmp_path / "future.npz"
    np.savez_compressed(path, **dict(arrays, version=np.array([99], np.int32)))
    with pytest.raises(ValueError, match="version"):
        compress.load_scene(path)
    with pytest.raises(ValueError):
        compress.load_scene(tmp_path / "scene.splat")
    for size in (0, 65537, 2.5):
        with pytest.raises(ValueError):
            compress.encode(p, fit=_fit, assign=_assign, codebook_size=size)
    with pytest.raises(ValueError):
        compress.encode(dict(p, sh=p["sh"][:, :4]), fit=_fit, assign=_assign)  # 12 floats: no SH degree
    with pytest.raises(ValueError):
        compress.encode(p, fit=_fit, assign=lambda x, c: np.full(len(x), len(c)), codebook_size=8)


@pytest.mark.parametrize("l_max", [0, 2])
def test_ply_round_trip_is_bit_exact(scene, compress, tmp_path, l_max):
    """The library reads its own product: what Trainer.save_to_ply hands the host writer comes back bit for bit."""
    ds = pkg("dataset")
    ds.build()
    p = _params(scene, l_max, 300)
    path = tmp_path / "gaussians.ply"
    n = len(p["xyz"])
    # as save_to_ply: the writer stores its (w,x,y,z) input as (x,y,z,w), so the columns are pre-rotated
    ds.save_ply(path, p["xyz"], p["rgb"], p["opacity"], p["scale"], np.roll(p["quaternion"], 1, axis=1),
                p["sh"].reshape(n, -1) if l_max else None)
    out = compress.load_scene(path)
    assert out["l_max"] == l_max
    for k in ("xyz", "rgb", "opacity", "scale", "quaternion", "sh"):
        assert out[k].dtype == np.float32 and out[k].shape == p[k].shape, k
        assert out[k].tobytes() == p[k].tobytes(), k
    with open(path, "rb") as f:
        data = f.read()
    bad = tmp_path / "short.ply"
    bad.write_bytes(data[:-4])
    with pytest.raises(ValueError, match="truncated"):
        compress.load_scene(bad)
    bad.write_bytes(data.replace(b"property float opacity", b"property float opaqueness"))
    with pytest.raises(ValueError):
        compress.load_scene(bad)

"""GPU tests of gsplat_mesh_components / gsplat_mesh_compact (ops.mesh_components, ops.mesh_filter) against the numpy
reference (tests/mesh_filter_reference.py).  Everything is integers or gathered floats: labels, counts, filtered vertices,
colours and faces are equal exactly.  Shapes: the empty meshes, one triangle, disjoint and touching pieces, unreferenced
vertices, strips either side of a wave (64) and of a workgroup (256), a strip of 20 000 triangles (diameter 20 000)
numbered forwards, backwards and at random, 30 000 components of 1 to 4 triangles, and the sphere of
tsdf_reference.field("sphere") with a translated copy."""
import ctypes

import numpy as np
import pytest

import mesh_filter_reference as mfr
import tsdf_reference as tr
from conftest import pkg

pytestmark = pytest.mark.gpu

FILTERS = ((5, 0), (0, 1), (0, 3), (5, 2), (10 ** 9, 0))


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _sphere_pair():
    f = tr.field("sphere")
    v, faces, c = tr.extract(f["tsdf"], f["weight"], f["color"], f["origin"], f["voxel"])[:3]
    shift = np.array([4.0 * (v[:, 0].max() - v[:, 0].min()), 0.0, 0.0], np.float32)
    return (np.concatenate([v, v + shift]).astype(np.float32), np.concatenate([faces, faces + len(v)]).astype(np.int32),
            np.concatenate([c, 1.0 - c]).astype(np.float32))


_CASES = {}  # name -> dict(faces, nv, vertices, colors, label, count): the reference is computed once and left alone


def _case(name):
    if name not in _CASES:
        colors = None
        if name in mfr.hand_cases():
            faces, nv = mfr.hand_cases()[name]
        elif name.startswith("strip_20000_"):
            faces, nv = mfr.strip(20000, name[len("strip_20000_"):], seed=7)
        elif name == "small_components":
            faces, nv = mfr.small_components(30000, seed=1)
        else:
            vertices, faces, colors = _sphere_pair()
            nv = len(vertices)
        if colors is None:
            rng = np.random.default_rng(3)
            vertices = rng.normal(size=(nv, 3)).astype(np.float32)
            colors = rng.uniform(size=(nv, 3)).astype(np.float32)
        label, count = mfr.components(faces, nv)
        _CASES[name] = dict(faces=faces, nv=nv, vertices=vertices, colors=colors, label=label, count=count)
    return _CASES[name]


NAMES = sorted(mfr.hand_cases()) + ["strip_20000_forward", "strip_20000_backward", "strip_20000_shuffled",
                                    "small_components", "sphere_pair"]


@pytest.mark.parametrize("name", NAMES)
def test_components_and_filter_match_the_reference(gpu, name):
    torch, ops = gpu, pkg("ops")
    case = _case(name)
    faces = torch.as_tensor(case["faces"]).cuda().reshape(-1, 3)
    got = ops.mesh_components(faces, case["nv"])
    torch.cuda.synchronize()
    assert got["label"].dtype == torch.int32 and got["face_count"].dtype == torch.int32
    assert np.array_equal(_np(got["label"]), case["label"]) and np.array_equal(_np(got["face_count"]), case["count"])
    print(f"{name}: {case['nv']} vertices, {len(case['faces'])} faces, "
          f"{int((case['label'] == np.arange(case['nv'])).sum())} components, rounds {got['rounds']}")
    # per-edge propagation would need as many rounds as the strip is long; far above log2(Nv) all the same
    assert got["rounds"] <= 64
    again = ops.mesh_components(faces, case["nv"])
    assert torch.equal(again["label"], got["label"]) and torch.equal(again["face_count"], got["face_count"])
    v, c = torch.as_tensor(case["vertices"]).cuda(), torch.as_tensor(case["colors"]).cuda()
    same = ops.mesh_filter(v, faces, c)  # both arguments 0: the very same tensors
    assert same[0] is v and same[1] is faces and same[2] is c and same[3] is None
    for min_faces, keep_largest in FILTERS:
        for colors in (c, None):
            out = ops.mesh_filter(v, faces, colors, min_faces=min_faces, keep_largest=keep_largest)
            ref = mfr.mesh_filter(case["vertices"], case["faces"], None if colors is None else case["colors"],
                                  min_faces=min_faces, keep_largest=keep_largest, labelled=(case["label"], case["count"]))
            what = f"{name}, min_faces {min_faces}, keep_largest {keep_largest}"
            assert out[3] == ref[3], what
            assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32
            assert out[0].shape == ref[0].shape and out[1].shape == ref[1].shape, what
            assert np.array_equal(_np(out[0]).view(np.uint32), ref[0].view(np.uint32)), what
            assert np.array_equal(_np(out[1]), ref[1]), what
            if colors is None:
                assert out[2] is None
            else:
                assert np.array_equal(_np(out[2]).view(np.uint32), ref[2].view(np.uint32)), what
        twice = ops.mesh_filter(v, faces, c, min_faces=min_faces, keep_largest=keep_largest)
        assert all(torch.equal(a, b) for a, b in zip(out[:2], twice[:2]))
    if min_faces == 10 ** 9:
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3)


def test_the_tie_goes_to_the_lower_label(gpu):
    torch, ops = gpu, pkg("ops")
    case = _case("sphere_pair")
    half = case["nv"] // 2
    roots = np.nonzero(case["label"] == np.arange(case["nv"]))[0]
    assert roots.tolist() == [0, half] and case["count"][0] == case["count"][half] > 100  # two equal components
    v, f = torch.as_tensor(case["vertices"]).cuda(), torch.as_tensor(case["faces"]).cuda()
    ov, of, _, rep = ops.mesh_filter(v, f, None, keep_largest=1)
    assert torch.equal(ov, v[:half]) and torch.equal(of, f[: len(f) // 2])
    assert rep == dict(components=2, kept=1, faces_removed=len(f) // 2, vertices_removed=half)


def test_bad_face_indices_are_refused_and_nothing_is_written(gpu):
    torch, ops, lib_mod = gpu, pkg("ops"), pkg("_lib")
    lib = lib_mod.load()
    nv = 300
    faces, _ = mfr.strip(nv - 2)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bad in (nv, -1, 2 ** 31 - 1, -2 ** 31):
        f = faces.copy()
        f[137, 1] = bad
        dev = torch.as_tensor(f).cuda()
        label = torch.full((nv,), 7, dtype=torch.int32, device="cuda")
        count = torch.full((nv,), 7, dtype=torch.int32, device="cuda")
        rounds = ctypes.c_int(-5)
        rc = lib.gsplat_mesh_components(ctypes.c_void_p(dev.data_ptr()), len(f), nv, ctypes.c_void_p(label.data_ptr()),
                                        ctypes.c_void_p(count.data_ptr()), ctypes.byref(rounds), st)
        torch.cuda.synchronize()
        assert rc == -3, (bad, rc)
        assert bool((label == 7).all()) and bool((count == 7).all()), bad
        with pytest.raises(lib_mod.GsplatError) as e:
            ops.mesh_components(dev, nv)
        assert e.value.code == -3
        with pytest.raises(lib_mod.GsplatError):
            ops.mesh_filter(torch.zeros(nv, 3, device="cuda"), dev, min_faces=1)
    good = ops.mesh_components(torch.as_tensor(faces).cuda(), nv)  # the library works on after a refusal
    assert bool((good["label"] == 0).all()) and int(good["face_count"][0]) == nv - 2
    # host pointers and wrong tensors
    label = torch.full((nv,), 7, dtype=torch.int32, device="cuda")
    host = np.zeros(nv, np.int32)
    dev = torch.as_tensor(faces).cuda()
    assert lib.gsplat_mesh_components(ctypes.c_void_p(dev.data_ptr()), len(faces), nv, ctypes.c_void_p(host.ctypes.data),
                                      ctypes.c_void_p(label.data_ptr()), None, st) != 0
    assert bool((label == 7).all()) and not host.any()
    for call in (lambda: ops.mesh_components(dev.long(), nv), lambda: ops.mesh_components(dev[:, :2].contiguous(), nv),
                 lambda: ops.mesh_components(dev, -1), lambda: ops.mesh_components(dev.t().contiguous().t(), nv),
                 lambda: ops.mesh_filter(torch.zeros(nv + 1, 3, device="cuda"), dev, torch.zeros(nv, 3, device="cuda"), 1),
                 lambda: ops.mesh_filter(torch.zeros(nv, 3, device="cuda").double(), dev, None, 1)):
        with pytest.raises(ValueError):
            call()

"""CPU tests of the mesh component filter: the numpy reference (tests/mesh_filter_reference.py) against scipy's connected
components and against hand-made answers, the declared entry points, and the Python argument checks."""
import os
import re

import numpy as np
import pytest

import mesh_filter_reference as mfr
from conftest import ROOT, pkg


def _all_cases():
    cases = dict(mfr.hand_cases())
    for order in ("forward", "backward", "shuffled"):
        cases[f"strip_2000_{order}"] = mfr.strip(2000, order, seed=5)
    cases["small_components"] = mfr.small_components(3000, seed=1)
    return cases


def test_labels_match_scipy():
    sp = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    for name, (faces, nv) in _all_cases().items():
        label, count = mfr.components(faces, nv)
        if nv == 0:
            assert label.shape == (0,) and count.shape == (0,)
            continue
        f = faces.astype(np.int64)
        rows = np.concatenate([f[:, 0], f[:, 0]])
        cols = np.concatenate([f[:, 1], f[:, 2]])
        graph = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv))
        n, comp = csgraph.connected_components(graph, directed=False)
        smallest = np.full(n, nv, np.int64)
        np.minimum.at(smallest, comp, np.arange(nv))
        assert np.array_equal(label, smallest[comp]), name
        assert int((label == np.arange(nv)).sum()) == n, name
        want = np.zeros(nv, np.int64)
        np.add.at(want, label[f[:, 0]], 1)
        assert np.array_equal(count, want) and count.sum() == len(faces), name
        assert (count[label != np.arange(nv)] == 0).all(), name


def test_hand_cases():
    cases = mfr.hand_cases()
    label, count = mfr.components(*cases["no_faces_5"])
    assert label.tolist() == [0, 1, 2, 3, 4] and count.tolist() == [0] * 5
    label, count = mfr.components(*cases["two_triangles"])
    assert label.tolist() == [0, 0, 0, 3, 3, 3] and count.tolist() == [1, 0, 0, 1, 0, 0]
    label, count = mfr.components(*cases["two_tetrahedra_one_vertex"])
    assert label.tolist() == [0] * 7 and count.tolist() == [8, 0, 0, 0, 0, 0, 0]
    label, count = mfr.components(*cases["unreferenced"])
    assert label.tolist() == [0, 1, 1, 3, 4, 1, 6, 6, 6, 9] and count.tolist() == [0, 1, 0, 0, 0, 0, 2, 0, 0, 0]
    for order in ("forward", "backward", "shuffled"):
        faces, nv = mfr.strip(500, order, seed=3)
        label, count = mfr.components(faces, nv)
        assert (label == 0).all() and count[0] == 500 and count[1:].sum() == 0
    with pytest.raises(ValueError):
        mfr.components(np.array([[0, 1, 3]]), 3)
    with pytest.raises(ValueError):
        mfr.components(np.array([[0, -1, 2]]), 3)


def test_filter_rule_on_the_hand_cases():
    faces, nv = mfr.hand_cases()["unreferenced"]
    v = np.arange(nv * 3, dtype=np.float32).reshape(nv, 3)
    c = v + 0.5
    same = mfr.mesh_filter(v, faces, c)
    assert same[0] is not None and np.array_equal(same[0], v) and same[3] is None
    # min_faces = 1 drops the four unreferenced vertices, nothing else
    ov, of, oc, rep = mfr.mesh_filter(v, faces, c, min_faces=1)
    assert np.array_equal(ov, v[[1, 2, 5, 6, 7, 8]]) and np.array_equal(oc, c[[1, 2, 5, 6, 7, 8]])
    assert of.tolist() == [[0, 1, 2], [3, 4, 5], [5, 4, 3]]
    assert rep == dict(components=6, kept=2, faces_removed=0, vertices_removed=4)
    # the largest: {6, 7, 8}; the two largest: it and {1, 2, 5}; the three largest: vertex 0 as well (0 faces, lowest label)
    ov, of, _, rep = mfr.mesh_filter(v, faces, None, keep_largest=1)
    assert np.array_equal(ov, v[[6, 7, 8]]) and of.tolist() == [[0, 1, 2], [2, 1, 0]] and rep["faces_removed"] == 1
    ov, of, _, rep = mfr.mesh_filter(v, faces, None, keep_largest=3)
    assert np.array_equal(ov, v[[0, 1, 2, 5, 6, 7, 8]]) and rep["kept"] == 3 and rep["vertices_removed"] == 3
    ov, of, _, rep = mfr.mesh_filter(v, faces, None, min_faces=1, keep_largest=3)  # ... unless min_faces forbids it
    assert np.array_equal(ov, v[[1, 2, 5, 6, 7, 8]]) and rep["kept"] == 2
    ov, of, oc, rep = mfr.mesh_filter(v, faces, c, min_faces=10 ** 9)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and oc.shape == (0, 3) and rep["kept"] == 0
    # ties in face_count go to the lower label
    faces, nv = mfr.hand_cases()["two_triangles"]
    ov, of, _, _ = mfr.mesh_filter(np.arange(18, dtype=np.float32).reshape(6, 3), faces, None, keep_largest=1)
    assert ov[:, 0].tolist() == [0.0, 3.0, 6.0] and of.tolist() == [[0, 1, 2]]


def test_abi_declares_the_entry_points():
    lib_mod = pkg("_lib")
    lib = lib_mod.load()
    header = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(gsplat_\w+)\s*\(([^;]*)\)\s*;", header)}
    for name, nargs in (("gsplat_mesh_components", 7), ("gsplat_mesh_compact", 12)):
        assert name in decl, name
        args = re.sub(r"/\*.*?\*/", "", decl[name], flags=re.S)
        assert len(lib_mod.SIGNATURES[name][1]) == args.count(",") + 1 == nargs, name
        assert callable(getattr(lib, name))
    assert lib_mod.ABI_VERSION == int(re.search(r"#define\s+GSPLAT_ABI_VERSION\s+(\d+)\b", header).group(1)) == 9
    assert "gs_mesh.hip" in open(os.path.join(ROOT, "3dgs_amd", "csrc", "Makefile")).read()
    # what the library can refuse without a device
    assert lib.gsplat_mesh_components(None, -1, 3, None, None, None, None) == -3
    assert lib.gsplat_mesh_components(None, 2, 0, None, None, None, None) == -3
    assert lib.gsplat_mesh_components(None, 0, 0, None, None, None, None) == 0
    assert lib.gsplat_mesh_compact(None, None, None, 0, 0, None, None, None, None, None, None, None) == 0
    assert lib.gsplat_mesh_compact(None, None, None, 3, -1, None, None, None, None, None, None, None) == -3


def test_python_argument_checks_need_no_device():
    import torch
    ops = pkg("ops")
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)  # host tensors: refused before any library call
    for call in (lambda: ops.mesh_components(f, 4),
                 lambda: ops.mesh_components(np.zeros((2, 3), np.int32), 4),
                 lambda: ops.mesh_filter(v, f, min_faces=1),
                 lambda: ops.mesh_filter(v, f, min_faces=-1),
                 lambda: ops.mesh_filter(v, f, keep_largest=1.5),
                 lambda: ops.mesh_filter(v, f, keep_largest=True)):
        with pytest.raises(ValueError):
            call()

"""CPU checks of the TSDF mesh extraction: the float64 marching-tetrahedra reference (tests/tsdf_reference.py) on analytic
fields -- closed, oriented, of the right genus --, the host mesh helpers (3dgs_amd/mesh.py), the new names in header and
binding, and the margins of the GPU integration cases: every decision of every case of tests/test_tsdf_gpu.py lies at
least 1e-9 (relative) from its boundary, so that comparison excludes no node."""
import os
import re

import numpy as np
import pytest

import tsdf_reference as tr
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name in tr.FIELDS:
        f = tr.field(name)
        out[name] = (f,) + tr.extract(f["tsdf"], f["weight"], f["color"], f["origin"], f["voxel"])[:4]
    return out


def _euler(vertices, faces, report):
    return len(vertices) - report["edges"] + len(faces)


def _face_normals(vertices, faces):
    v = vertices.astype(np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


def test_sphere_is_closed_oriented_and_of_genus_0(meshes):
    mesh = pkg("mesh")
    f, v, faces, colors, _ = meshes["sphere"]
    rep = mesh.edge_report(faces)
    assert len(faces) > 100 and rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["oriented"], rep
    assert _euler(v, faces, rep) == 2
    assert faces.min() == 0 and faces.max() == len(v) - 1 and len(np.unique(faces)) == len(v)  # no orphan vertex
    vol = mesh.signed_volume(v, faces)
    exact = 4.0 / 3.0 * np.pi * (3.7 * 0.25) ** 3
    assert 0.9 * exact < vol < 1.02 * exact, (vol, exact)  # (a chordal surface of a convex body lies inside it)
    nrm = _face_normals(v, faces)
    area = np.linalg.norm(nrm, axis=1)
    keep = area > 1e-12
    cen = v[faces].astype(np.float64).mean(1)
    dots = np.einsum("ij,ij->i", nrm[keep], f["grad"](cen[keep]))
    assert (dots > 0).all(), int((dots <= 0).sum())
    assert colors.shape == v.shape and colors.min() >= 0.0 and colors.max() <= 1.0


def test_torus_has_genus_1(meshes):
    mesh = pkg("mesh")
    _, v, faces, _, _ = meshes["torus"]
    rep = mesh.edge_report(faces)
    assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["oriented"], rep
    assert _euler(v, faces, rep) == 0
    assert mesh.signed_volume(v, faces) > 0


def test_plane_is_an_open_sheet_with_its_boundary_on_the_grids_boundary(meshes):
    mesh = pkg("mesh")
    f, v, faces, _, ends = meshes["plane"]
    rep = mesh.edge_report(faces)
    assert rep["boundary"] > 0 and rep["nonmanifold"] == 0 and rep["oriented"], rep
    assert _euler(v, faces, rep) == 1  # a disc
    # every boundary edge joins two vertices that lie on one face of the grid's box
    a = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]]).astype(np.int64)
    b = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]]).astype(np.int64)
    key = np.minimum(a, b) * len(v) + np.maximum(a, b)
    uniq, count = np.unique(key, return_counts=True)
    nx, ny, nz = f["dims"]
    lo = np.asarray(f["origin"], np.float32).astype(np.float64)
    hi = lo + float(np.float32(f["voxel"])) * (np.array([nx, ny, nz]) - 1)
    for k in uniq[count == 1]:
        p, q = ends[k // len(v)], ends[k % len(v)]  # [2,3] each: the grid edges the two vertices sit on
        on_face = [(np.abs(np.concatenate([p, q])[:, ax] - side[ax]) < 1e-9).all() for ax in range(3) for side in (lo, hi)]
        assert any(on_face), (p, q)
    nrm = _face_normals(v, faces)
    assert (nrm @ np.array([0.31, 0.52, 0.8]) > 0).all()


def test_exact_zeros_keep_the_bookkeeping_and_the_zero_area_faces(meshes):
    mesh = pkg("mesh")
    f, v, faces, _, _ = meshes["exact_zeros"]
    rep = mesh.edge_report(faces)
    assert rep["nonmanifold"] == 0 and rep["oriented"], rep
    assert _euler(v, faces, rep) == 1  # the sheet x = 3 across the box
    area = np.linalg.norm(_face_normals(v, faces), axis=1)
    assert (area == 0).any() and (area > 0).any()
    # f = i - 3 has its zeros AT the nodes i = 3, which count as outside: every vertex lands on that plane
    x3 = float(np.float32(f["origin"][0])) + float(np.float32(f["voxel"])) * 3
    assert np.abs(v[:, 0] - x3).max() < 1e-6


def test_one_inside_corner_gives_7_vertices_and_6_faces(meshes):
    mesh = pkg("mesh")
    f, v, faces, _, _ = meshes["one_corner"]
    assert v.shape == (7, 3) and faces.shape == (6, 3)
    rep = mesh.edge_report(faces)
    assert rep["manifold"] == 6 and rep["boundary"] == 6 and rep["oriented"], rep
    o, h = np.asarray(f["origin"], np.float32).astype(np.float64), float(np.float32(f["voxel"]))
    dirs = np.array([[d & 1, d >> 1 & 1, d >> 2 & 1] for d in tr.EDGE_DIRS], np.float64)
    assert np.abs(v - (o + 0.5 * h * dirs)).max() < 1e-6  # vertex order = edge type order, t = 1/2 on every edge
    assert (_face_normals(v, faces) @ np.ones(3) > 0).all()  # away from the inside corner


def test_an_all_positive_field_is_empty(meshes):
    _, v, faces, colors, _ = meshes["positive"]
    assert v.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3)


def test_no_face_touches_a_cell_with_an_unobserved_node(meshes):
    f, v, faces, _, ends = meshes["sphere_half_seen"]
    assert len(faces) > 20
    x_limit = float(np.float32(f["origin"][0])) + float(np.float32(f["voxel"])) * 5  # nodes i >= 6 are unobserved
    assert ends[np.unique(faces)][..., 0].max() <= x_limit + 1e-9
    _, full_v, full_faces, _, _ = meshes["sphere"]
    assert 0 < len(faces) < len(full_faces)


def test_all_seven_edge_types_carry_vertices(meshes):
    mesh = pkg("mesh")
    _, v, faces, _, ends = meshes["all_edges"]
    d = np.rint((ends[:, 1] - ends[:, 0]) / float(np.float32(0.25))).astype(int)
    assert sorted(set(map(tuple, d))) == sorted((x & 1, x >> 1 & 1, x >> 2 & 1) for x in range(1, 8))
    assert len(v) == 14  # the 14 edges of the triangulation at a node
    rep = mesh.edge_report(faces)
    assert rep["boundary"] == 0 and rep["nonmanifold"] == 0 and rep["oriented"] and _euler(v, faces, rep) == 2
    assert mesh.signed_volume(v, faces) > 0


def test_ply_round_trip_and_reports_on_a_tetrahedron(tmp_path):
    mesh = pkg("mesh")
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)  # outward
    colors = np.array([[0, 0, 0], [1, 0.5, 0.25], [0.2, 1.7, -3], [1, 1, 1]], np.float32)
    rep = mesh.edge_report(faces)
    assert rep == dict(boundary=0, manifold=6, nonmanifold=0, edges=6, oriented=True)
    assert abs(mesh.signed_volume(v, faces) - 1.0 / 6.0) < 1e-12
    assert abs(mesh.signed_volume(v, faces[:, ::-1]) + 1.0 / 6.0) < 1e-12
    flipped = faces.copy()
    flipped[3] = flipped[3, ::-1]
    assert not mesh.edge_report(flipped)["oriented"]
    assert mesh.edge_report(faces[:3]) == dict(boundary=3, manifold=3, nonmanifold=0, edges=6, oriented=True)
    fan = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32)
    assert mesh.edge_report(fan)["nonmanifold"] == 1
    p = str(tmp_path / "t.ply")
    mesh.save_ply(p, v, faces, colors)
    head = open(p, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
    assert b"property float x" in head and b"property uchar red" in head
    v2, f2, c2 = mesh.load_ply(p)
    assert v2.dtype == np.float32 and f2.dtype == np.int32 and c2.dtype == np.uint8
    assert (v2 == v).all() and (f2 == faces).all()
    assert c2.tolist() == [[0, 0, 0], [255, 128, 64], [51, 255, 0], [255, 255, 255]]
    mesh.save_ply(p, v, faces)
    v3, f3, c3 = mesh.load_ply(p)
    assert (v3 == v).all() and (f3 == faces).all() and c3 is None
    mesh.save_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v4, f4, _ = mesh.load_ply(p)
    assert v4.shape == (0, 3) and f4.shape == (0, 3)


def test_header_and_binding_name_the_new_entry_points():
    lib_mod = pkg("_lib")
    text = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gsplat_tsdf_integrate", "gsplat_tsdf_views_per_pass", "gsplat_tsdf_mark", "gsplat_tsdf_emit"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in lib_mod.SIGNATURES, name
    assert re.search(r"#define\s+GSPLAT_ABI_VERSION\s+9\b", text) and lib_mod.ABI_VERSION == 9
    assert re.search(r"#define\s+GSPLAT_TSDF_MAX_NODES\s+2147483647LL", text)
    assert pkg("ops").TSDF_MAX_NODES == 2147483647
    lib = lib_mod.load()
    assert lib.gsplat_abi_version() == 9
    assert lib.gsplat_tsdf_views_per_pass() >= 1


@pytest.fixture(scope="module")
def integration():
    cases = tr.integration_cases()
    return {name: (c, tr.start_state(c), tr.run_reference(c, tr.start_state(c))) for name, c in cases.items()}


def test_the_gpu_integration_cases_cover_what_they_should_and_sit_off_every_boundary(integration):
    lib = pkg("_lib").load()
    per_pass = lib.gsplat_tsdf_views_per_pass()
    Ks = {c["K"] for c, _, _ in integration.values()}
    assert {1, 2, 5, 9} <= Ks and max(Ks) > per_pass and max(Ks) % per_pass != 0  # a full pass plus a remainder
    assert {c["dims"] for c, _, _ in integration.values()} == set(tr.GRIDS)
    for what in ("inverse", "max_depth", "max_weight"):
        assert {bool(c[what]) for c, _, _ in integration.values()} == {False, True}, what
    assert {c["image"] is None for c, _, _ in integration.values()} == {False, True}
    changed_any = 0
    for name, (c, start, ref) in integration.items():
        assert ref["margin"] >= 1e-9, (name, ref["margin"])
        changed = int((ref["weight"] != start["weight"]).sum() + (ref["tsdf"] != start["tsdf"]).sum())
        if name in ("behind", "miss"):
            assert changed == 0, name
            if c["image"] is not None:
                assert (ref["color"] == start["color"]).all()
        elif np.prod(c["dims"]) > 1:
            assert changed > 0, name
        changed_any += changed
        if c["max_weight"] > 0:
            assert ref["weight"].max() <= c["max_weight"]
        assert np.isfinite(ref["tsdf"]).all() and ref["tsdf"].max() <= 1.0
    # the maps hold what they are meant to hold
    c = integration["K9_color_limits"][0]
    A = 1.0 - c["T"].astype(np.float64)
    assert (A < c["alpha_min"]).any() and (A == c["alpha_min"]).any() and np.isnan(c["depth"]).any()
    assert (c["depth"] == 0).any() and (c["depth"] < 0).any()
    ref = integration["K9_color_limits"][2]
    assert (ref["tsdf"] == 1.0).any() and ((ref["tsdf"] > -1.0) & (ref["tsdf"] < 1.0) & (ref["weight"] > 0)).any()

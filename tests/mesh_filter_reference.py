"""numpy versions of gsplat_mesh_components and ops.mesh_filter, written from their description in include/gsplat_hip.h
and 3dgs_amd/ops.py; plus the meshes the tests share.

components(faces, Nv): a union-find on the host (union by smaller root, path compression).  Two vertices are connected
when a face holds both; label[v] = the smallest vertex index of v's component; face_count[r] = the faces of the component
labelled r, 0 at every index that is not a label.

mesh_filter(vertices, faces, colors, min_faces, keep_largest): a component is kept iff face_count >= min_faces and, when
keep_largest > 0, it is among the keep_largest components ranked by (-face_count, label); kept vertices, colours and faces
keep their order, the faces are renumbered."""
import numpy as np


def components(faces, num_vertices):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= num_vertices):
        raise ValueError("a face index lies outside [0, num_vertices)")
    parent = list(range(num_vertices))

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r

    for a, b, c in faces.tolist():
        for x, y in ((a, b), (a, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    label = np.array([find(v) for v in range(num_vertices)], np.int32).reshape(num_vertices)
    face_count = np.bincount(label[faces[:, 0]], minlength=num_vertices).astype(np.int32) if len(faces) \
        else np.zeros(num_vertices, np.int32)
    return label, face_count


def mesh_filter(vertices, faces, colors=None, min_faces=0, keep_largest=0, labelled=None):
    """-> (vertices, faces, colors, report) as ops.mesh_filter returns them (report None when both arguments are 0).
    labelled: components(faces, Nv) when the caller has it already."""
    vertices, faces = np.asarray(vertices, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    if min_faces == 0 and keep_largest == 0:
        return vertices, faces, colors, None
    nv = len(vertices)
    label, count = components(faces, nv) if labelled is None else labelled
    roots = np.nonzero(label == np.arange(nv))[0]
    keep = set(int(r) for r in roots if count[r] >= min_faces)
    if keep_largest > 0:
        ranked = sorted((int(r) for r in roots), key=lambda r: (-int(count[r]), r))
        keep &= set(ranked[:keep_largest])
    keep_root = np.zeros(nv, bool)
    keep_root[list(keep)] = True
    keep_vertex = keep_root[label] if nv else np.zeros(0, bool)
    keep_face = keep_vertex[faces[:, 0]] if len(faces) else np.zeros(0, bool)
    new_index = np.cumsum(keep_vertex) - 1
    out_f = new_index[faces[keep_face]].astype(np.int32).reshape(-1, 3)
    out_c = None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)[keep_vertex]
    report = dict(components=len(roots), kept=len(keep), faces_removed=int(len(faces) - keep_face.sum()),
                  vertices_removed=int(nv - keep_vertex.sum()))
    return vertices[keep_vertex], out_f, out_c, report


# ---------------------------------------------------------------------------------------------------------------------
# the meshes of the tests: name -> (faces [Nf,3] int32, num_vertices)

def strip(num_triangles, order="forward", seed=0, num_vertices=None):
    """A triangle strip (i, i+1, i+2): one component of diameter ~num_triangles.  order: how the vertices are numbered
    along it -- "forward", "backward" or "shuffled" (a seeded permutation; the faces are shuffled with it)."""
    n = num_triangles + 2 if num_triangles else 0
    i = np.arange(num_triangles)
    f = np.stack([i, i + 1, i + 2], 1)
    if order == "backward":
        f = n - 1 - f
    elif order == "shuffled":
        rng = np.random.default_rng(seed)
        f = rng.permutation(n)[f][rng.permutation(num_triangles)]
    return f.astype(np.int32).reshape(-1, 3), (n if num_vertices is None else num_vertices)


def small_components(num=30000, seed=1):
    """`num` components of 1 to 4 triangles each (fans around one vertex), vertices and faces shuffled: many ties in
    face_count."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 5, num)
    faces, base = [], 0
    for s in sizes.tolist():
        for k in range(s):
            faces.append((base, base + k + 1, base + k + 2))
        base += s + 2
    perm = rng.permutation(base)
    f = perm[np.asarray(faces)][rng.permutation(len(faces))]
    return f.astype(np.int32), base


def hand_cases():
    tetra = lambda o: [(o, o + 1, o + 2), (o, o + 1, o + 3), (o, o + 2, o + 3), (o + 1, o + 2, o + 3)]
    cases = {
        "empty": (np.zeros((0, 3), np.int32), 0),
        "no_faces_5": (np.zeros((0, 3), np.int32), 5),
        "one_triangle": (np.array([[0, 1, 2]], np.int32), 3),
        "two_triangles": (np.array([[0, 1, 2], [5, 4, 3]], np.int32), 6),
        # two tetrahedra that share vertex 3: one component
        "two_tetrahedra_one_vertex": (np.asarray(tetra(0) + tetra(3), np.int32), 7),
        # vertices 0, 3, 4 and 9 are in no face; {1, 2, 5} has one face, {6, 7, 8} two
        "unreferenced": (np.array([[1, 2, 5], [6, 7, 8], [8, 7, 6]], np.int32), 10),
    }
    for nv in (63, 64, 65, 255, 256, 257):
        cases[f"strip_nv{nv}"] = strip(nv - 2)
    return cases

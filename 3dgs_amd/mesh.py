"""Triangle meshes on the host (numpy only): binary PLY in and out, and the two checks a surface extraction is judged by --
the edge bookkeeping of a closed oriented surface and the signed volume.  The meshes come from ops.tsdf_extract /
Trainer.extract_mesh."""
import numpy as np


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def save_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY: float32 x y z, uchar red green blue when `colors` ([Nv,3] in [0,1]; clipped, rounded to
    nearest) is given, faces as `list uchar int vertex_indices`."""
    v = np.ascontiguousarray(_host(vertices), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(_host(faces), dtype="<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
              "property float z"]
    if colors is not None:
        c = np.asarray(_host(colors), dtype=np.float64).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("colors must have one row per vertex")
        c = np.floor(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(len(v), dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"], face["i"] = 3, f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vert.tobytes())
        out.write(face.tobytes())


def load_ply(path):
    """What save_ply wrote -> (vertices [Nv,3] float32, faces [Nf,3] int32, colors [Nv,3] uint8 or None).  Reads binary
    little-endian PLY with float x y z, optional uchar red green blue in that order, and triangles only."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or "format binary_little_endian 1.0" not in lines:
        raise ValueError("not a binary little-endian PLY")
    nv = nf = 0
    props, element = [], None
    for line in lines:
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            elif element == "face":
                nf = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
    names = [p[0] for p in props]
    if names[:3] != ["x", "y", "z"] or names[3:] not in ([], ["red", "green", "blue"]):
        raise ValueError("unsupported vertex properties: " + " ".join(names))
    vdt = np.dtype(props)
    vert = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    face = np.frombuffer(data, dtype=fdt, count=nf, offset=end + nv * vdt.itemsize)
    if nf and not (face["n"] == 3).all():
        raise ValueError("only triangles are supported")
    vertices = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
    colors = np.stack([vert["red"], vert["green"], vert["blue"]], 1) if len(names) == 6 else None
    return vertices, face["i"].astype(np.int32).reshape(-1, 3), colors


def edge_report(faces):
    """The edge bookkeeping of an indexed triangle mesh: dict(boundary=edges with one incident face, manifold=with two,
    nonmanifold=with more, edges=all of them, oriented=every two-face edge is traversed once in each direction by its two
    faces).  A closed oriented surface has boundary = nonmanifold = 0 and oriented = True."""
    f = np.asarray(_host(faces), dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return dict(boundary=0, manifold=0, nonmanifold=0, edges=0, oriented=True)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    forward = (a < b).astype(np.int64)  # a degenerate half-edge (a == b) counts as backward
    key = lo * (int(hi.max()) + 1) + hi
    _, inverse, count = np.unique(key, return_inverse=True, return_counts=True)
    fwd = np.bincount(inverse.reshape(-1), weights=forward, minlength=len(count)).astype(np.int64)
    two = count == 2
    return dict(boundary=int((count == 1).sum()), manifold=int(two.sum()), nonmanifold=int((count > 2).sum()),
                edges=int(len(count)), oriented=bool((fwd[two] == 1).all()))


def signed_volume(vertices, faces):
    """sum over the faces of v0 . (v1 x v2) / 6 in float64: the enclosed volume of a closed surface whose normals
    (v1 - v0) x (v2 - v0) point outwards, its negative when they point inwards."""
    v = np.asarray(_host(vertices), dtype=np.float64).reshape(-1, 3)
    f = np.asarray(_host(faces), dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return 0.0
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)

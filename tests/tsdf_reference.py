"""numpy float64 versions of gsplat_tsdf_integrate and of the marching-tetrahedra extraction (gsplat_tsdf_mark /
gsplat_tsdf_emit), written from their description in include/gsplat_hip.h; plus the analytic fields the extraction tests
share (tests/test_tsdf_cpu.py, tests/test_tsdf_gpu.py)."""
import itertools

import numpy as np

EDGE_DIRS = (1, 2, 4, 3, 5, 6, 7)  # edge type -> direction bits (x = 1, y = 2, z = 4): axes, face diagonals, body diagonal
EDGE_TYPE = {d: e for e, d in enumerate(EDGE_DIRS)}
TETS = tuple(itertools.permutations((1, 2, 4)))  # (a, b, c) in lexicographic order: xyz, xzy, yxz, yzx, zxy, zyx


def node_positions(origin, voxel, dims):
    """[nz,ny,nx,3] float64: origin + voxel * (i,j,k) from the float32 values the kernels are given."""
    nx, ny, nz = dims
    o = np.asarray(origin, np.float32).astype(np.float64)
    h = float(np.float32(voxel))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + h * i, o[1] + h * j, o[2] + h * k], -1)


def integrate(state, origin, voxel, dims, depth, T, image, view, intrinsics, inverse, alpha_min, trunc, near=0.0,
              max_depth=0.0, max_weight=0.0):
    """state: dict(tsdf, weight [nz,ny,nx] float32, color [nz,ny,nx,3] float32 or None), updated IN A COPY that is
    returned with: bound_tsdf / bound_color = |old| + |val| of every element's last update (0 where there was none), and
    margin = the smallest relative distance of any decision that was reached from its boundary:
    u + 0.5 and v + 0.5 from the nearest integer, z - near, s + trunc, d - max_depth."""
    f32, f64 = np.float32, np.float64
    tsdf, weight = state["tsdf"].astype(f32).copy(), state["weight"].astype(f32).copy()
    color = None if state.get("color") is None else state["color"].astype(f32).copy()
    p = node_positions(origin, voxel, dims)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    K, H, W = depth.shape
    alpha_min, trunc, near, max_depth = (float(f32(v)) for v in (alpha_min, trunc, near, max_depth))
    max_weight = f32(max_weight)
    bound_tsdf = np.zeros(tsdf.shape, f64)
    bound_color = None if color is None else np.zeros(color.shape, f64)
    margin = np.inf
    tiny = 1e-300

    def rel_min(dist, scale, where):
        if not where.any():
            return np.inf
        return float((np.abs(dist[where]) / np.maximum(scale[where], tiny)).min())

    with np.errstate(all="ignore"):
        for v in range(K):
            m = np.asarray(view[v], f32).astype(f64)
            fx, fy, cx, cy = (float(x) for x in np.asarray(intrinsics[v], f32).astype(f64))
            z = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11]
            live = z > near
            margin = min(margin, rel_min(z - near, np.maximum(np.abs(z), abs(near)), np.isfinite(z)))
            xc = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
            yc = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7]
            zs = np.where(live, z, 1.0)
            uh = (fx * xc / zs + cx) + 0.5
            vh = (fy * yc / zs + cy) + 0.5
            for h in (uh, vh):
                margin = min(margin, rel_min(h - np.round(h), np.maximum(1.0, np.abs(h)), live))
            fu, fv = np.floor(uh), np.floor(vh)
            live = live & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            ix, iy = np.where(live, fu, 0).astype(np.int64), np.where(live, fv, 0).astype(np.int64)
            A = 1.0 - T[v][iy, ix].astype(f64)
            d = depth[v][iy, ix].astype(f64)
            live = live & (A >= alpha_min) & (A < np.inf) & (d > 0.0) & (d < np.inf)
            As, ds = np.where(live, A, 1.0), np.where(live, d, 1.0)
            surf = As / ds if inverse else ds / As
            if max_depth > 0.0:
                margin = min(margin, rel_min(surf - max_depth, np.full(surf.shape, max_depth), live))
                live = live & ~(surf > max_depth)
            s = surf - z
            margin = min(margin, rel_min(s + trunc, np.abs(surf) + np.abs(z) + trunc, live))
            live = live & (s >= -trunc)
            val = np.minimum(1.0, s / trunc)
            wd = weight.astype(f64)
            wn = wd + 1.0
            new = ((wd * tsdf.astype(f64) + val) / wn).astype(f32)
            bound_tsdf = np.where(live, np.abs(tsdf.astype(f64)) + np.abs(val), bound_tsdf)
            tsdf = np.where(live, new, tsdf)
            if color is not None:
                pix = image[v][iy, ix].astype(f64)
                newc = ((wd[..., None] * color.astype(f64) + pix) / wn[..., None]).astype(f32)
                bound_color = np.where(live[..., None], np.abs(color.astype(f64)) + np.abs(pix), bound_color)
                color = np.where(live[..., None], newc, color)
            wnew = wn.astype(f32)
            if max_weight > 0:
                wnew = np.minimum(wnew, max_weight)
            weight = np.where(live, wnew, weight)
    return dict(tsdf=tsdf, weight=weight, color=color, bound_tsdf=bound_tsdf, bound_color=bound_color, margin=margin)


def _odd(p):
    return sum(p[x] > p[y] for x in range(4) for y in range(x + 1, 4)) & 1


def tet_case(mask):
    """The triangles of a positively oriented tetrahedron whose inside corners are the bits of `mask`, as triples of local
    edges (p, q), p < q."""
    e = lambda p, q: (min(p, q), max(p, q))
    ins = [c for c in range(4) if mask >> c & 1]
    out = [c for c in range(4) if not mask >> c & 1]
    if len(ins) == 1:
        i, (o0, o1, o2) = ins[0], out
        if _odd((i, o0, o1, o2)):
            o1, o2 = o2, o1
        return [(e(i, o0), e(i, o1), e(i, o2))]
    if len(ins) == 3:
        o, (i0, i1, i2) = out[0], ins
        if _odd((o, i0, i1, i2)):
            i1, i2 = i2, i1
        return [(e(o, i0), e(o, i2), e(o, i1))]
    if len(ins) == 2:
        (i0, i1), (o0, o1) = ins, out
        if _odd((i0, i1, o0, o1)):
            o0, o1 = o1, o0
        q = (e(i0, o0), e(i0, o1), e(i1, o1), e(i1, o0))
        return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return []


def extract(tsdf, weight, color, origin, voxel, min_weight=1.0):
    """(vertices [Nv,3] float32, faces [Nf,3] int32, colors [Nv,3] float32 or None, ends [Nv,2,3] float64: the positions
    of every vertex's two nodes, color_ends [Nv,2,3] float64 or None: their colours), as plain loops over the cells."""
    tsdf, weight = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    pos = node_positions(origin, voxel, (nx, ny, nz)).reshape(-1, 3)
    f = tsdf.reshape(-1).astype(np.float64)
    col = None if color is None else np.asarray(color, np.float32).reshape(-1, 3).astype(np.float64)
    inside = tsdf < 0
    seen = weight >= np.float32(min_weight)
    off = lambda c: (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
    cell_ok = np.zeros((nz, ny, nx), bool)
    if min(nx, ny, nz) > 1:
        ok = np.ones((nz - 1, ny - 1, nx - 1), bool)
        n_in = np.zeros((nz - 1, ny - 1, nx - 1), int)
        for c in range(8):
            sl = (slice(c >> 2 & 1, nz - 1 + (c >> 2 & 1)), slice(c >> 1 & 1, ny - 1 + (c >> 1 & 1)),
                  slice(c & 1, nx - 1 + (c & 1)))
            ok &= seen[sl]
            n_in += inside[sl]
        cell_ok[:-1, :-1, :-1] = ok & (n_in > 0) & (n_in < 8)
    inside = inside.reshape(-1)
    tris = []  # triples of (lower node, edge type)
    for n in np.flatnonzero(cell_ok.reshape(-1)):
        for (a, b, c) in TETS:
            corner = (0, a, a | b, 7)
            odd = _odd((0,) + tuple({1: 1, 2: 2, 4: 3}[x] for x in (a, b, c)))
            mask = sum(int(inside[n + off(corner[l])]) << l for l in range(4))
            for tri in tet_case(mask):
                keys = [(int(n + off(corner[p])), EDGE_TYPE[corner[p] ^ corner[q]]) for p, q in tri]
                if odd:
                    keys[1], keys[2] = keys[2], keys[1]
                tris.append(keys)
    keys = sorted({k for t in tris for k in t})
    index = {k: i for i, k in enumerate(keys)}
    faces = np.asarray([[index[k] for k in t] for t in tris], np.int32).reshape(-1, 3)
    lower = np.asarray([k[0] for k in keys], np.int64)
    upper = lower + np.asarray([off(EDGE_DIRS[k[1]]) for k in keys], np.int64)
    t = (f[lower] / (f[lower] - f[upper]))[:, None] if keys else np.zeros((0, 1))
    vertices = (pos[lower] + t * (pos[upper] - pos[lower])).astype(np.float32).reshape(-1, 3)
    colors = None if col is None else (col[lower] + t * (col[upper] - col[lower])).astype(np.float32).reshape(-1, 3)
    ends = np.stack([pos[lower], pos[upper]], 1).reshape(-1, 2, 3)
    color_ends = None if col is None else np.stack([col[lower], col[upper]], 1).reshape(-1, 2, 3)
    return vertices, faces, colors, ends, color_ends


# ---------------------------------------------------------------------------------------- analytic fields, shared
def _ijk(dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                          np.arange(nx, dtype=np.float64), indexing="ij")
    return i, j, k


def field(name):
    """name -> dict(tsdf, weight, color [.., 3], origin, voxel, dims, grad: positions [M,3] -> analytic gradient or None).
    Grids are deliberately unequal in x, y and z."""
    origin, voxel = (-0.7, 0.35, 1.2), 0.25
    weight = None
    grad = None
    if name == "sphere" or name == "sphere_half_seen":
        dims = (12, 11, 13)
        i, j, k = _ijk(dims)
        c = np.array([5.3, 4.9, 6.2])
        f = np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2) - 3.7
        centre = np.asarray(origin, np.float32).astype(np.float64) + float(np.float32(voxel)) * c
        grad = lambda p: (p - centre) / np.linalg.norm(p - centre, axis=-1, keepdims=True)
        if name == "sphere_half_seen":
            weight = np.ones(f.shape, np.float32)
            weight[:, :, 6:] = 0.0
    elif name == "torus":
        dims = (20, 18, 9)
        i, j, k = _ijk(dims)
        f = np.sqrt((np.sqrt((i - 9.4) ** 2 + (j - 8.6) ** 2) - 5.6) ** 2 + (k - 4.1) ** 2) - 2.3
    elif name == "plane":
        dims = (9, 8, 7)
        i, j, k = _ijk(dims)
        f = 0.31 * (i - 4.2) + 0.52 * (j - 3.4) + 0.8 * (k - 2.9)
    elif name == "exact_zeros":
        dims = (7, 5, 4)
        i, j, k = _ijk(dims)
        f = i - 3.0
    elif name == "one_corner":
        dims = (2, 2, 2)
        f = np.ones((2, 2, 2))
        f[0, 0, 0] = -1.0
    elif name == "positive":
        dims = (5, 4, 3)
        f = np.full((3, 4, 5), 0.5)
    elif name == "long_x":  # x beyond one wave of 64
        dims = (70, 3, 3)
        i, j, k = _ijk(dims)
        f = np.sin(0.37 * i + 0.2) + 0.4 * (j - 1.0) + 0.3 * (k - 0.9)
    elif name == "all_edges":  # one inside node in the middle of 3x3x3: the surface crosses all seven edge types twice
        dims = (3, 3, 3)
        f = np.full((3, 3, 3), 0.75)
        f[1, 1, 1] = -0.5
    else:
        raise KeyError(name)
    f = (f * 0.2).astype(np.float32)  # (a TSDF's range; the scale leaves the level set where it is)
    i, j, k = _ijk(dims)
    color = np.stack([0.1 + 0.05 * i, 0.9 - 0.04 * j, 0.3 + 0.02 * k + 0.01 * i], -1).astype(np.float32)
    if weight is None:
        weight = np.ones(f.shape, np.float32)
    return dict(tsdf=f, weight=weight, color=color, origin=origin, voxel=voxel, dims=dims, grad=grad)


FIELDS = ("sphere", "torus", "plane", "exact_zeros", "one_corner", "positive", "sphere_half_seen", "long_x", "all_edges")


# ---------------------------------------------------------------------------------------- integration cases, shared
def synthetic_maps(K, H, W, alpha_min, seed, inverse):
    """Seeded maps: a smooth depth plus a step edge, T with regions below alpha_min and exactly at it, a few NaN, zero and
    negative depths.  depth holds what a depth-mode forward composites: A z (inverse: A / z)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.empty((K, H, W), np.float32)
    T = np.empty((K, H, W), np.float32)
    for v in range(K):
        zs = 2.0 + 0.3 * np.sin(0.21 * x + v) + 0.2 * np.cos(0.17 * y - v) + rng.uniform(0.0, 0.05, (H, W))
        zs = zs + 0.6 * (x > 0.55 * W)  # the step edge
        t = rng.uniform(0.0, 0.45, (H, W)).astype(np.float32)
        r = rng.uniform(size=(H, W))
        if H * W > 1:
            t[r < 0.08] = np.float32(0.9)                  # A = 0.1: below alpha_min
            t[(r >= 0.08) & (r < 0.14)] = np.float32(1.0) - np.float32(alpha_min)  # A == alpha_min: still ok
        A = 1.0 - t.astype(np.float64)
        d = (A / zs if inverse else A * zs).astype(np.float32)
        if H * W > 4:
            r2 = rng.uniform(size=(H, W))
            d[r2 < 0.03] = np.nan
            d[(r2 >= 0.03) & (r2 < 0.06)] = 0.0
            d[(r2 >= 0.06) & (r2 < 0.09)] = -1.0
        depth[v], T[v] = d, t
    image = rng.uniform(0.0, 1.0, (K, H, W, 3)).astype(np.float32)
    return depth, T, image


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """[12] float32, row-major [R|t] of a camera at `eye` looking at `target` (+z forward, +x right, +y down)."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    if np.linalg.norm(right) < 1e-8:
        right = np.cross(fwd, np.array([1.0, 0.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return np.concatenate([R, (-R @ eye)[:, None]], 1).astype(np.float32).reshape(12)


GRIDS = ((1, 1, 1), (3, 5, 7), (33, 17, 9), (65, 2, 2))
IMAGES = ((1, 1), (5, 3), (40, 24))  # (W, H)
ALPHA_MIN = 0.5


def integration_case(dims, size, K, inverse, color, limits, seed, special=None):
    """One seeded GPU integration case: the volume's geometry, K cameras around it, the maps and the rule.
    limits: max_depth and max_weight on.  special: None, "behind" (every camera looks away from the volume: z <= near at
    every node) or "miss" (the frustum of every camera misses the volume)."""
    rng = np.random.default_rng(1000 + seed)
    W, H = size
    nx, ny, nz = dims
    voxel = 0.11
    origin = (-0.5 * voxel * (nx - 1) + 0.013, -0.5 * voxel * (ny - 1) - 0.021, 2.2 - 0.5 * voxel * (nz - 1))
    centre = np.array([0.013, -0.021, 2.2])
    view = np.empty((K, 12), np.float32)
    intr = np.empty((K, 4), np.float32)
    for v in range(K):
        eye = rng.normal(size=3) * 0.15
        target = centre + rng.normal(size=3) * 0.05
        if special == "behind":
            target = eye - (centre - eye)
        elif special == "miss":
            target = eye + np.array([1.0, 0.2, 0.05])
        view[v] = look_at(eye, target, up=(0.02, 1.0, 0.03))
        # a frustum that sees the whole volume from ~2.2 away: the grid spans at most 65 * 0.11 = 7.2 across
        extent = max(voxel * max(nx, ny), 0.5)
        focal = 0.45 * W * 2.2 / extent * rng.uniform(0.9, 1.1) * (4.0 if special == "miss" else 1.0)
        intr[v] = (focal, focal * 1.03, 0.5 * W - 0.27 + 0.02 * v, 0.5 * H - 0.31)
    depth, T, image = synthetic_maps(K, H, W, ALPHA_MIN, 2000 + seed, inverse)
    return dict(dims=dims, origin=origin, voxel=voxel, view=view, intrinsics=intr, depth=depth, T=T,
                image=image if color else None, inverse=bool(inverse), alpha_min=ALPHA_MIN, trunc=0.35, near=0.05,
                max_depth=2.6 if limits else 0.0, max_weight=3.0 if limits else 0.0, K=K)


def integration_cases():
    """name -> case: every grid x image once, and K, inverse, colour and the limits varied over them; plus the two cameras
    that change nothing."""
    cases = {}
    seed = 0
    Ks = (1, 2, 5, 9)
    for gi, dims in enumerate(GRIDS):
        for si, size in enumerate(IMAGES):
            n = gi * len(IMAGES) + si
            K, inverse, color, limits = Ks[n % 4], bool((n // 2) % 2), bool(n % 3 != 1), bool((n // 3) % 2)
            cases[f"g{'x'.join(map(str, dims))}_i{size[0]}x{size[1]}_K{K}_inv{int(inverse)}_c{int(color)}_l{int(limits)}"] = \
                integration_case(dims, size, K, inverse, color, limits, seed)
            seed += 1
    cases["K9_color_limits"] = integration_case((33, 17, 9), (40, 24), 9, False, True, True, 50)
    cases["K9_inverse_plain"] = integration_case((3, 5, 7), (40, 24), 9, True, False, False, 51)
    cases["behind"] = integration_case((3, 5, 7), (5, 3), 2, False, True, False, 52, special="behind")
    cases["miss"] = integration_case((33, 17, 9), (40, 24), 2, False, True, False, 53, special="miss")
    return cases


def start_state(case, seed=7):
    """A non-trivial state to integrate into: some nodes already observed."""
    nx, ny, nz = case["dims"]
    rng = np.random.default_rng(seed)
    weight = rng.integers(0, 3, (nz, ny, nx)).astype(np.float32)
    tsdf = np.where(weight > 0, rng.uniform(-1.0, 1.0, (nz, ny, nx)), 0.0).astype(np.float32)
    color = None
    if case["image"] is not None:
        color = np.where(weight[..., None] > 0, rng.uniform(0.0, 1.0, (nz, ny, nx, 3)), 0.0).astype(np.float32)
    return dict(tsdf=tsdf, weight=weight, color=color)


def run_reference(case, state):
    return integrate(state, case["origin"], case["voxel"], case["dims"], case["depth"], case["T"], case["image"],
                     case["view"], case["intrinsics"], case["inverse"], case["alpha_min"], case["trunc"], case["near"],
                     case["max_depth"], case["max_weight"])

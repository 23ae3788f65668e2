"""float64 numpy reference of the vector quantisation (ops.vq_assign / vq_update / vq_fit) and of the compressed scene
format (3dgs_amd/compress.py): brute-force nearest centroid with lowest-index ties, the condition sums the GPU tests bound
errors by, cluster means, the Lloyd loop with the library's seeding and re-seeding rules, the quantisers and the decoder.
Written apart from the package: nothing here imports it."""
import numpy as np


def distances(x, c):
    """[N,K] squared distances, summed coordinate by coordinate in float64."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.zeros((len(x), len(c)))
    for d in range(x.shape[1]):
        out += (x[:, d:d + 1] - c[None, :, d]) ** 2
    return out


def assign(x, c, chunk=4096):
    """-> (index [N] int32 with the lowest index winning ties, dist [N] float64)."""
    x = np.asarray(x, np.float64)
    index, dist = np.empty(len(x), np.int32), np.empty(len(x))
    for a in range(0, len(x), chunk):
        d = distances(x[a:a + chunk], c)
        index[a:a + chunk] = np.argmin(d, axis=1)  # (the first of equal minima)
        dist[a:a + chunk] = d[np.arange(len(d)), index[a:a + chunk]]
    return index, dist


def cond(x, c):
    """The condition sum of row n against ITS centroid c[n]: sum_d (x^2 + c^2 + 2 |x c|)."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (x * x + c * c + 2.0 * np.abs(x * c)).sum(1)


def distance_to(x, c):
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return ((x - c) ** 2).sum(1)


def update(x, index, c):
    """Means of the members; an empty cluster keeps its centroid.  -> (float32 codebook, sum |x| / count per centroid)."""
    x = np.asarray(x, np.float64)
    out, mag = np.array(c, np.float32), np.zeros(np.shape(c))
    for k in range(len(out)):
        rows = x[np.asarray(index) == k]
        if len(rows):
            out[k] = (rows.sum(0) / len(rows)).astype(np.float32)
            mag[k] = np.abs(rows).sum(0) / len(rows)
    return out, mag


def fit(x, K, iterations=10, seed=0, perm=None):
    """The Lloyd loop of ops.vq_fit on float32 rows: `perm` is the seeded permutation (torch.randperm in the library; any
    permutation here), K clamped to N; each round assign, re-seed the empty clusters in index order from the rows of
    largest distance (descending, ties by row), update; a last assign.  -> (codebook float32, index, objectives)."""
    x = np.asarray(x, np.float32)
    K = min(int(K), len(x))
    if perm is None:
        perm = np.random.default_rng(seed).permutation(len(x))
    c = x[np.asarray(perm)[:K]].copy()
    objective = []
    for it in range(iterations + 1):
        index, dist = assign(x, c)
        dist = dist.astype(np.float32)
        objective.append(float(dist.astype(np.float64).sum()))
        if it == iterations:
            break
        empty = np.flatnonzero(np.bincount(index, minlength=K) == 0)
        if len(empty):
            donors = np.argsort(-dist.astype(np.float64), kind="stable")[:len(empty)]
            c[empty] = x[donors]
            index[donors] = empty
        c = update(x, index, c)[0]
    return c, index, objective


# ---------------------------------------------------------------- the compressed scene format
def quantise(v, bits, lo=None, hi=None):
    v = np.asarray(v, np.float64)
    L = 2.0 ** bits - 1.0
    if lo is None:
        lo, hi = v.min(0), v.max(0)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.rint((v - lo) / (hi - lo) * L)
    q = np.where(hi > lo, q, 0.0)  # a constant column: 0 / 0 above
    return q.astype(np.uint8 if bits <= 8 else np.uint16), lo, hi


def dequantise(q, bits, lo, hi):
    L = 2.0 ** bits - 1.0
    return (np.asarray(lo, np.float64) + np.asarray(q, np.float64) * (np.asarray(hi, np.float64) - lo) / L).astype(np.float32)


def decode(a):
    """The arrays of a compressed scene -> float32 params (the module docstring of 3dgs_amd/compress.py is the format)."""
    assert int(a["version"][0]) == 1
    l_max = int(a["l_max"][0])
    t = np.asarray(a["xyz_lo"], np.float64) + np.asarray(a["xyz_q"], np.float64) * (a["xyz_hi"] - a["xyz_lo"]) / 65535.0
    out = dict(xyz=(np.sign(t) * np.expm1(np.abs(t))).astype(np.float32),
               rgb=dequantise(a["rgb_q"], 8, a["rgb_lo"], a["rgb_hi"]),
               opacity=dequantise(a["opacity_q"], 8, a["opacity_lo"], a["opacity_hi"]),
               scale=dequantise(a["scale_q"], 8, a["scale_lo"], a["scale_hi"]),
               quaternion=dequantise(a["quaternion_q"], 8, -1.0, 1.0), l_max=l_max)
    n = len(out["xyz"])
    if l_max > 0:
        book = dequantise(a["sh_codebook_q"], 8, a["sh_codebook_lo"], a["sh_codebook_hi"])
        out["sh"] = book[a["sh_index"].astype(np.int64)].reshape(n, -1, 3)
    else:
        out["sh"] = np.zeros((n, 0, 3), np.float32)
    return out


def rotation(q):
    """(w, x, y, z) rows -> [N,3,3] rotation matrices of the normalised quaternions."""
    q = np.asarray(q, np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)

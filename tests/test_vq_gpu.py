"""ops.vq_assign / vq_update / vq_fit on the GPU against tests/vq_reference.py (float64).

Assign.  The score |c|^2 - 2 x.c is a k-ordered float fmaf chain on the matrix cores, about 1.5e-7 x sum |a b| off the exact
value, so the returned centroid may be a near-tie of the float64 argmin: the condition is on the DISTANCE,
    d64(x_n, c_i) <= min_k d64(x_n, c_k) + 1e-6 max(cond(n, i), cond(n, k*)),   cond(n, k) = sum_d (x^2 + c^2 + 2 |x c|),
the project's bar (1e-6 x the condition sum, tests/test_bilagrid_gpu.py).  On small integers every product and sum is exact
in float32, and there the index must be the float64 brute force's with lowest-index ties, element for element.

Shapes: each axis varied around (N = 257, K = 33, D = 45) -- N and K either side of the 32-wide tiles, odd and even D for the
padded k-pair, D = 64 and K = 65 536 at the limits -- plus N = 1100 (three workgroups of 512 points, the last one partial)
against K = 300 (several LDS stages of 64 or, above D = 48, 128 centroids, the last one partial, its last 32-centroid tile
too), and D either side of 16, 32 and 48, where the kernel's register sizing changes."""
import ctypes

import numpy as np
import pytest

import vq_reference as vqr
from conftest import pkg

pytestmark = pytest.mark.gpu

BAR, FLOOR = 1e-6, 2.0 ** -149
INVALID_ARG = -3
BASE = (257, 33, 45)
SHAPES = sorted({(n, BASE[1], BASE[2]) for n in (1, 31, 32, 33, 65, 257)}
                | {(BASE[0], k, BASE[2]) for k in (1, 2, 31, 33, 256, 4099)}
                | {(BASE[0], BASE[1], d) for d in (1, 2, 3, 9, 24, 45, 46, 64)}
                | {(BASE[0], BASE[1], d) for d in (16, 17, 32, 33, 48, 49)}  # either side of the kernel's register buckets
                | {(65, 65536, 45), (1100, 300, 45), (1100, 300, 64), (33, 31, 1), (1, 1, 64)})
_CACHE = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(shape):
    """SH-like rows and centroids (centroids drawn near rows, as a codebook's are) and the float64 reference; built once."""
    if shape not in _CACHE:
        n, k, d = shape
        rng = np.random.default_rng([4, n, k, d])
        x = (0.1 * rng.standard_normal((n, d))).astype(np.float32)
        c = (x[rng.integers(0, n, k)] + 0.02 * rng.standard_normal((k, d))).astype(np.float32)
        index, dist = vqr.assign(x, c)
        for a in (x, c, index, dist):
            a.setflags(write=False)
        _CACHE[shape] = dict(x=x, c=c, index=index, dist=dist)
    return _CACHE[shape]


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def _meets_assign_condition(what, x, c, got, ref_index, ref_dist):
    got = np.asarray(got, np.int64)
    assert got.min() >= 0 and got.max() < len(c), f"{what}: an index outside the codebook"
    d_got = vqr.distance_to(x, c[got])
    bar = BAR * np.maximum(vqr.cond(x, c[got]), vqr.cond(x, c[ref_index])) + FLOOR
    frac = (d_got - ref_dist) / bar
    print(f"[{what}] worst {float(frac.max()):.4f} of the bar, {int((got != ref_index).sum())} of {len(got)} indices "
          "differ from the float64 argmin")
    assert (frac <= 1.0).all(), f"{what}: a row at {float(frac.max()):.3f} of its bar"
    return bar


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-K%d-D%d" % s)
def test_assign_random(gpu, shape):
    ops, case = pkg("ops"), _case(shape)
    x, c = _dev(gpu, case["x"]), _dev(gpu, case["c"])
    index = gpu.full((shape[0],), -7, dtype=gpu.int32, device="cuda")
    dist = gpu.full((shape[0],), -7.0, device="cuda")
    assert ops.vq_assign(x, c, index, dist) is index
    got = _np(index)
    _meets_assign_condition("assign %s" % (shape,), case["x"], case["c"], got, case["index"], case["dist"])
    # dist is the double-precision distance to the RETURNED centroid, rounded once
    want = vqr.distance_to(case["x"], case["c"][got])
    frac = np.abs(_np(dist).astype(np.float64) - want) / (BAR * want + FLOOR)
    print(f"[dist {shape}] worst {float(frac.max()):.4f} of the bar")
    assert (frac <= 1.0).all()
    # without dist, into a new tensor, and again: the same bits
    again = ops.vq_assign(x, c)
    assert again.dtype == gpu.int32 and _np(again).tobytes() == got.tobytes()
    assert _np(ops.vq_assign(x, c, dist=None)).tobytes() == got.tobytes()


@pytest.mark.parametrize("shape", [(257, 300, 45), (257, 300, 2), (600, 33, 7), (64, 4099, 46)], ids=lambda s: "N%d-K%d-D%d" % s)
def test_assign_exact_data_resolves_ties_to_the_lowest_index(gpu, shape):
    ops = pkg("ops")
    n, k, d = shape
    rng = np.random.default_rng([5, n, k, d])
    c = rng.integers(-8, 9, (k, d)).astype(np.float32)
    # duplicates across the two half-waves of a tile (rows 3 / 5), across tiles of 32, across LDS stages of 128
    pairs = [(3, 5), (1, 32), (10, k - 2), (6, 20)] + ([(33, 64), (70, 140), (129, 257)] if k >= 258 else [])
    for a, b in pairs:
        c[b] = c[a]
    x = rng.integers(-8, 9, (n, d)).astype(np.float32)
    planted = [b for _, b in pairs] + [a for a, _ in pairs]
    x[:len(planted)] = c[planted]
    ref_index, ref_dist = vqr.assign(x, c)
    assert (ref_dist[:len(planted)] == 0).all() and (ref_index[:len(pairs)] <= [a for a, _ in pairs]).all()
    dist = gpu.empty(n, device="cuda")
    got = _np(ops.vq_assign(_dev(gpu, x), _dev(gpu, c), dist=dist))
    assert (got == ref_index).all(), f"{int((got != ref_index).sum())} of {n} indices differ on exact data"
    assert (_np(dist).astype(np.float64) == ref_dist).all()


def test_assign_with_pointers_off_the_16_byte_boundary(gpu):
    ops, case = pkg("ops"), _case(BASE)
    n, k, d = BASE

    def shifted(a, dtype):
        flat = gpu.zeros(a.size + 1, dtype=dtype, device="cuda")
        flat[1:] = _dev(gpu, a).reshape(-1)
        t = flat[1:].view(a.shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    x, c = shifted(case["x"], gpu.float32), shifted(case["c"], gpu.float32)
    index, dist = shifted(np.zeros(n, np.int32), gpu.int32), shifted(np.zeros(n, np.float32), gpu.float32)
    ops.vq_assign(x, c, index, dist)
    aligned_dist = gpu.empty(n, device="cuda")
    aligned = ops.vq_assign(_dev(gpu, case["x"]), _dev(gpu, case["c"]), dist=aligned_dist)
    assert _np(index).tobytes() == _np(aligned).tobytes() and _np(dist).tobytes() == _np(aligned_dist).tobytes()


def test_assign_of_no_rows_and_refusals(gpu):
    ops, lib = pkg("ops"), pkg("_lib").load()
    c = _dev(gpu, _case(BASE)["c"])
    empty = ops.vq_assign(gpu.zeros(0, 45, device="cuda"), c)
    assert empty.shape == (0,) and empty.dtype == gpu.int32
    n, k, d = 40, 33, 45
    x = _dev(gpu, _case(BASE)["x"][:n])
    index = gpu.full((n,), -7, dtype=gpu.int32, device="cuda")
    dist = gpu.full((n,), -7.0, device="cuda")
    book = c.clone()
    order = gpu.arange(n, dtype=gpu.int32, device="cuda")
    start = gpu.zeros(k + 1, dtype=gpu.int32, device="cuda")
    start[1:] = n
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.gsplat_vq_assign(None, None, 0, d, k, None, None, None) == 0  # N = 0: a successful no-op
    for args in ((p(x), p(c), n, 0, k, p(index), p(dist)), (p(x), p(c), n, 65, k, p(index), p(dist)),
                 (p(x), p(c), n, d, 0, p(index), p(dist)), (p(x), p(c), n, d, 65537, p(index), p(dist)),
                 (p(x), p(c), -1, d, k, p(index), p(dist)), (None, p(c), n, d, k, p(index), p(dist)),
                 (p(x), None, n, d, k, p(index), p(dist)), (p(x), p(c), n, d, k, None, p(dist))):
        assert lib.gsplat_vq_assign(*args, None) == INVALID_ARG, args
        assert b"gsplat_vq_assign" in lib.gsplat_last_error()
    for args in ((p(x), p(order), p(start), n, 0, k, p(book)), (p(x), p(order), p(start), n, 65, k, p(book)),
                 (p(x), p(order), p(start), n, d, 0, p(book)), (p(x), p(order), p(start), n, d, 65537, p(book)),
                 (p(x), p(order), p(start), -1, d, k, p(book)), (None, p(order), p(start), n, d, k, p(book)),
                 (p(x), None, p(start), n, d, k, p(book)), (p(x), p(order), None, n, d, k, p(book)),
                 (p(x), p(order), p(start), n, d, k, None)):
        assert lib.gsplat_vq_update(*args, None) == INVALID_ARG, args
    gpu.cuda.synchronize()
    assert (_np(index) == -7).all() and (_np(dist) == -7.0).all() and _np(book).tobytes() == _np(c).tobytes()


UPDATES = {  # name -> (N, K, D, the index of every row)
    "random-with-empty-clusters": (1000, 37, 45, lambda rng, n, k: np.where((i := rng.integers(0, k, n)) % 5 == 3, 0, i)),
    "one-cluster-holds-all": (257, 4, 45, lambda rng, n, k: np.full(n, 2)),
    "every-cluster-one-row": (257, 257, 24, lambda rng, n, k: rng.permutation(n)),
    "64-lanes-per-sum": (5000, 3, 9, lambda rng, n, k: rng.integers(0, k, n) % 2),
    "odd-width": (300, 70, 1, lambda rng, n, k: rng.integers(0, k, n)),
}


@pytest.mark.parametrize("name", list(UPDATES))
def test_update(gpu, name):
    ops = pkg("ops")
    n, k, d, make = UPDATES[name]
    rng = np.random.default_rng([6, n, k, d])
    x = (0.1 * rng.standard_normal((n, d)) + 0.05).astype(np.float32)
    index = np.asarray(make(rng, n, k), np.int32)
    c0 = rng.standard_normal((k, d)).astype(np.float32)
    want, mag = vqr.update(x, index, c0)
    ref = np.array(c0, np.float64)
    for j in np.unique(index):
        ref[j] = x[index == j].astype(np.float64).sum(0) / (index == j).sum()
    book = _dev(gpu, c0)
    assert ops.vq_update(_dev(gpu, x), _dev(gpu, index), book) is book
    got = _np(book)
    empty = np.bincount(index, minlength=k) == 0
    assert got[empty].tobytes() == c0[empty].tobytes()  # an empty cluster keeps its bits
    frac = np.abs(got.astype(np.float64) - ref)[~empty] / (BAR * mag[~empty] + FLOOR)
    print(f"[update {name}] worst {float(frac.max()):.4f} of the bar, {int(empty.sum())} empty clusters")
    assert (frac <= 1.0).all()
    book2 = _dev(gpu, c0)
    ops.vq_update(_dev(gpu, x), _dev(gpu, index), book2)
    assert _np(book2).tobytes() == got.tobytes()


def _perm(torch, n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).numpy()


def test_fit_is_reproducible_and_its_objective_never_increases(gpu):
    ops = pkg("ops")
    rng = np.random.default_rng(7)
    n, k, d = 3000, 64, 45
    centres = 0.1 * rng.standard_normal((20, d))
    x = (centres[rng.integers(0, 20, n)] + 0.03 * rng.standard_normal((n, d))).astype(np.float32)
    xd = _dev(gpu, x)
    book, index, objective = ops.vq_fit(xd, k, iterations=6, seed=5)
    book2, index2, objective2 = ops.vq_fit(xd, k, iterations=6, seed=5)
    assert _np(book).tobytes() == _np(book2).tobytes() and _np(index).tobytes() == _np(index2).tobytes()
    assert objective == objective2 and len(objective) == 7
    assert tuple(book.shape) == (k, d) and index.dtype == gpu.int32
    other = ops.vq_fit(xd, k, iterations=6, seed=6)[0]
    assert _np(other).tobytes() != _np(book).tobytes()
    # Every centroid is a row or a mean of rows, so |c| <= max |x| and cond(n, k) <= 2 (|x_n|^2 + max_m |x_m|^2): the sum of
    # that over the rows bounds sum_n bar_n of any round without knowing the round's centroids.  (The float32 roundings of
    # dist and of the means are 6e-8 of smaller quantities.)
    sq = (x.astype(np.float64) ** 2).sum(1)
    slack = BAR * 2.0 * (sq + sq.max()).sum()
    print("[fit] objective per assign:", " ".join(f"{o:.6g}" for o in objective), f"(slack {slack:.3g})")
    assert all(b <= a + slack for a, b in zip(objective, objective[1:]))
    assert objective[-1] < 0.5 * objective[0]
    # the outputs: index is nearest for the codebook returned, and the last objective is theirs
    c, i = _np(book), _np(index)
    ref_index, ref_dist = vqr.assign(x, c)
    _meets_assign_condition("fit", x, c, i, ref_index, ref_dist)
    recomputed = vqr.distance_to(x, c[i]).sum()
    assert abs(recomputed - objective[-1]) <= 1e-6 * recomputed
    # the first K rows of the seeded permutation are the initial centroids
    first = ops.vq_fit(xd, k, iterations=0, seed=5)
    assert _np(first[0]).tobytes() == x[_perm(gpu, n, 5)[:k]].tobytes() and len(first[2]) == 1


def test_fit_reproduces_rows_when_the_codebook_can_hold_them(gpu):
    ops = pkg("ops")
    rng = np.random.default_rng(8)
    values = rng.integers(-8, 9, (12, 9)).astype(np.float32)
    x = values[rng.integers(0, 12, 200)]
    # K = 16 for 12 distinct rows: the 16 initial rows miss some of the 12, and only the re-seeding brings them in (the
    # float64 reference with the same permutation: 16636, 5934, 3368, 1994, 556, then 0)
    book, index, objective = ops.vq_fit(_dev(gpu, x), 16, iterations=10, seed=0)
    print("[fit, 12 distinct rows, K = 16] objective per assign:", objective)
    assert objective[0] > 0.0 and objective[-1] == 0.0
    c, i = _np(book), _np(index)
    assert c[i].tobytes() == x.tobytes()
    # K clamped to N
    book, index, objective = ops.vq_fit(_dev(gpu, x[:5]), 64, iterations=1, seed=0)
    assert tuple(book.shape) == (5, 9) and _np(book)[_np(index)].tobytes() == x[:5].tobytes()


def test_fit_reseeds_empty_clusters(gpu):
    ops = pkg("ops")
    rng = np.random.default_rng(9)
    values = rng.integers(-8, 9, (5, 6)).astype(np.float32)
    x = values[rng.integers(0, 5, 300)]
    seed = 0
    initial = x[_perm(gpu, 300, seed)[:8]]
    assert len(np.unique(initial, axis=0)) < 8  # duplicate initial centroids: the higher index of each gets no row
    book, index, objective = ops.vq_fit(_dev(gpu, x), 8, iterations=4, seed=seed)
    c, i = _np(book), _np(index)
    assert np.isfinite(c).all() and all(np.isfinite(objective)) and objective[-1] == 0.0
    assert c[i].tobytes() == x.tobytes()
    assert _np(ops.vq_assign(_dev(gpu, x), book)).tobytes() == i.tobytes()

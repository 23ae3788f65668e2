"""The vector-quantisation reference (tests/vq_reference.py) against an independent formulation, the Lloyd loop's
monotonicity, and what of ops.vq_* can be checked without a device: the declared bindings and the argument checks, which
come before any launch."""
import numpy as np
import pytest
from scipy.spatial.distance import cdist

import vq_reference as vqr
from conftest import pkg


def _rows(seed, n, d, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("n,k,d", [(1, 1, 1), (33, 7, 3), (257, 33, 45), (64, 300, 24)])
def test_reference_assign_against_cdist(n, k, d):
    x, c = _rows([1, n, k, d], n, d), _rows([2, n, k, d], k, d)
    index, dist = vqr.assign(x, c, chunk=50)
    full = cdist(x.astype(np.float64), c.astype(np.float64), "sqeuclidean")
    assert index.dtype == np.int32 and index.shape == (n,)
    # the chosen centroid is a nearest one of the independent matrix, and the distance is that matrix's
    np.testing.assert_allclose(dist, full[np.arange(n), index], rtol=1e-12, atol=1e-300)
    assert (dist <= full.min(1) * (1 + 1e-12)).all()
    np.testing.assert_allclose(vqr.distance_to(x, c[index]), dist, rtol=1e-12, atol=1e-300)
    assert (vqr.cond(x, c[index]) >= dist).all()  # (x - c)^2 <= x^2 + c^2 + 2 |x c|


def test_reference_ties_take_the_lowest_index():
    rng = np.random.default_rng(3)
    c = rng.integers(-8, 9, (20, 5)).astype(np.float32)
    c[11] = c[4]
    c[17] = c[4]
    x = np.concatenate([c[[4, 17, 11]], rng.integers(-8, 9, (30, 5)).astype(np.float32)])
    index, dist = vqr.assign(x, c)
    assert list(index[:3]) == [4, 4, 4] and (dist[:3] == 0).all()
    full = cdist(x.astype(np.float64), c.astype(np.float64), "sqeuclidean")  # exact on small integers
    assert (index == np.argmin(full, 1)).all()


def test_reference_update_is_the_mean_and_keeps_empty_clusters():
    x = _rows(5, 100, 9)
    index = np.random.default_rng(6).integers(0, 7, 100).astype(np.int32)
    index[index == 3] = 2  # cluster 3 is empty
    c0 = _rows(7, 7, 9)
    c, mag = vqr.update(x, index, c0)
    assert c.dtype == np.float32 and c[3].tobytes() == c0[3].tobytes() and (mag[3] == 0).all()
    for k in (0, 2, 6):
        want = x[index == k].astype(np.float64).mean(0)
        np.testing.assert_allclose(c[k], want, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_lloyd_objective_never_increases(seed):
    x = _rows([8, seed], 400, 12)
    c, index, objective = vqr.fit(x, 24, iterations=8, seed=seed)
    assert len(objective) == 9 and c.shape == (24, 12) and c.dtype == np.float32
    # float64 sums of float32-rounded distances, centroids rounded to float32: one rounding of each per round
    slack = 1e-6 * objective[0]
    assert all(b <= a + slack for a, b in zip(objective, objective[1:])), objective
    assert objective[-1] < 0.9 * objective[0]
    np.testing.assert_allclose(vqr.distance_to(x, c[index]).sum(), objective[-1], rtol=1e-6)
    assert (index == vqr.assign(x, c)[0]).all()


def test_lloyd_reseeds_empty_clusters_and_reproduces_few_distinct_rows():
    rng = np.random.default_rng(9)
    values = rng.integers(-8, 9, (5, 6)).astype(np.float32)
    x = values[rng.integers(0, 5, 300)]
    c, index, objective = vqr.fit(x, 8, iterations=6, seed=0)
    assert np.isfinite(c).all() and objective[-1] == 0.0
    assert c[index].tobytes() == x.tobytes()


def test_k_is_clamped_to_n():
    x = _rows(10, 5, 3)
    c, index, objective = vqr.fit(x, 64, iterations=2, seed=0)
    assert c.shape == (5, 3) and sorted(index) == [0, 1, 2, 3, 4] and objective[-1] == 0.0


def test_bindings_are_declared():
    lib = pkg("_lib")
    P, I = lib._P, lib._I
    assert lib.SIGNATURES["gsplat_vq_assign"] == (I, [P, P, I, I, I, P, P, P])
    assert lib.SIGNATURES["gsplat_vq_update"] == (I, [P, P, P, I, I, I, P, P])
    with open(lib.os.path.join(lib._HERE, "..", "include", "gsplat_hip.h")) as f:
        header = f.read()
    assert "int gsplat_vq_assign(" in header and "int gsplat_vq_update(" in header
    with open(lib.os.path.join(lib._CSRC, "Makefile")) as f:
        assert "gs_vq.hip" in f.read()


def test_wrappers_refuse_bad_arguments_before_any_launch(monkeypatch):
    import torch
    ops, lib = pkg("ops"), pkg("_lib")

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(lib, "load", no_launch)
    host = torch.zeros(8, 4)
    for call in (lambda: ops.vq_assign(host, host),                                  # not on the device
                 lambda: ops.vq_assign(np.zeros((8, 4), np.float32), host),          # not a tensor
                 lambda: ops.vq_update(host, torch.zeros(8, dtype=torch.int32), host),
                 lambda: ops.vq_fit(host, 4),
                 lambda: ops.vq_fit(host.double(), 4)):
        with pytest.raises(ValueError):
            call()
    # the shape rules, on stand-ins that say they are device tensors
    class Dev(torch.Tensor):
        is_cuda = True
    dev = lambda t: t.as_subclass(Dev)
    x = dev(torch.zeros(8, 4))
    for call in (lambda: ops.vq_assign(x, dev(torch.zeros(3, 5))),                   # D differs
                 lambda: ops.vq_assign(dev(torch.zeros(8, 65)), dev(torch.zeros(3, 65))),  # D > 64
                 lambda: ops.vq_assign(dev(torch.zeros(8, 0)), dev(torch.zeros(3, 0))),    # D = 0
                 lambda: ops.vq_assign(x, dev(torch.zeros(0, 4))),                   # K = 0
                 lambda: ops.vq_assign(x, dev(torch.zeros(65537, 4))),               # K > 65536
                 lambda: ops.vq_assign(dev(torch.zeros(8, 8))[:, :4], dev(torch.zeros(3, 4))),  # not contiguous
                 lambda: ops.vq_assign(x, dev(torch.zeros(3, 4)), index=dev(torch.zeros(8, dtype=torch.int64))),
                 lambda: ops.vq_assign(x, dev(torch.zeros(3, 4)), index=dev(torch.zeros(7, dtype=torch.int32))),
                 lambda: ops.vq_assign(x, dev(torch.zeros(3, 4)), dist=dev(torch.zeros(8, dtype=torch.float64))),
                 lambda: ops.vq_update(x, dev(torch.zeros(8, dtype=torch.int32)), dev(torch.zeros(3, 5))),
                 lambda: ops.vq_update(x, dev(torch.zeros(8, dtype=torch.int64)), dev(torch.zeros(3, 4))),
                 lambda: ops.vq_update(x, dev(torch.full((8,), 3, dtype=torch.int32)), dev(torch.zeros(3, 4))),  # index = K
                 lambda: ops.vq_fit(x, 0),
                 lambda: ops.vq_fit(x, 2.5),
                 lambda: ops.vq_fit(x, 4, iterations=-1),
                 lambda: ops.vq_fit(dev(torch.zeros(0, 4)), 4)):
        with pytest.raises(ValueError):
            call()

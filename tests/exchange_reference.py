"""Float64 restatement of the view-sharded exchange (3dgs_amd/csrc/gs_exchange.hip, 3dgs_amd/dist.py, 3dgs_amd/optimizer.py):
the row layouts a rank packs, the rebuild of the SH-coefficient gradients from every rank's g_rgb, and the unpacked row.

Row layouts (n = (L + 1)^2 coefficients, W ranks; culled rows are zero, `seen` is 1.0 on kept rows):
  global    [xyz3 | rgb3 | sh 3(n-1) | opacity | scale3 | quat4 | seen]                 12 + 3n floats
  factored  [xyz3 | opacity | scale3 | quat4 | seen | g_rgb slot 0 .. slot W-1]         12 + 3W floats
  split     common[N,12] = [xyz3 | opacity | scale3 | quat4 | seen]  +  rgb[N,3] = g_rgb
  uv_norm   [N] = |grad_uv|
The pack functions only MOVE floats (the arrays keep their dtype), so a float32 input gives the kernels' bits.

SH rebuild: full[i] = sum_r g_rgb^r[i] (x) Y_k(dir(xyz_i, campos_r)), ranks in order.  The per-rank term is the oracle's
precompute_spherical_harmonics_backward: its band-0 and SH gradients are exactly g (x) Y_k, so basis and direction
come from oracle/gsplat_oracle_impl.h, not from gs_math.h.  A rank whose g_rgb row is all zero contributes nothing.

The generator of the GPU tests' synthetic inputs (`synthetic_case`) lives here too, so that tests/test_exchange_cpu.py
measures the error constant K and checks the input condition on the very arrays tests/test_exchange_gpu.py uses.
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32

# K[L]: the rebuilt SH columns of a float32 implementation lie within K[L] * U * S_ic * Ybar_L of the float64 value, where
# S_ic = sum_r |g^r_ic| and Ybar_L = the largest |Y_k| over the case's directions.  K = 4 * K_obs, K_obs = what the
# oracle's own float32 run shows on the grid of synthetic_case (measured and asserted by tests/test_exchange_cpu.py,
# which records the K_obs values).
K_OBS = {0: 3.8, 1: 4.2, 2: 5.3, 3: 6.4}
K = {L: 4.0 * k for L, k in K_OBS.items()}

GRID_N = (1, 63, 64, 65, 255, 256, 257, 321)
GRID_L = (0, 1, 2, 3)
GRID_WORLD = (1, 2, 3, 8)


def n_coeffs(l_max):
    return (l_max + 1) ** 2


def packed_width(l_max):
    return 12 + 3 * n_coeffs(l_max)


def sh_columns(l_max):
    """Columns of the unpacked row that the SH half writes: band 0 and the SH coefficients."""
    return np.arange(3, 3 + 3 * n_coeffs(l_max))


def common_columns(l_max):
    """Columns of the unpacked row that the common half writes: xyz, then opacity, scale, quaternion, seen."""
    n3 = 3 * n_coeffs(l_max)
    return np.concatenate([np.arange(0, 3), np.arange(3 + n3, 12 + n3)])


# ---------------------------------------------------------------------------------------------------- pack
def _scatter(mask, c2g, compact, width):
    compact = np.asarray(compact)
    out = np.zeros((len(mask), width), compact.dtype)
    c2g = np.asarray(c2g, np.int64)
    assert mask[c2g].all() and len(c2g) == int(mask.sum()) and len(np.unique(c2g)) == len(c2g)
    out[c2g] = compact.reshape(len(c2g), width)
    return out


def common_rows(mask, c2g, grads):
    """common[N,12]: [xyz3 | opacity | scale3 | quat4 | seen]."""
    mask = np.asarray(mask).astype(bool)
    dt = np.asarray(grads["xyz"]).dtype
    seen = np.ones((len(c2g), 1), dt)
    return np.concatenate([_scatter(mask, c2g, grads["xyz"], 3), _scatter(mask, c2g, grads["opacity"], 1),
                           _scatter(mask, c2g, grads["scale"], 3), _scatter(mask, c2g, grads["quaternion"], 4),
                           _scatter(mask, c2g, seen, 1)], 1)


def global_rows(mask, c2g, grads, l_max):
    mask = np.asarray(mask).astype(bool)
    com = common_rows(mask, c2g, grads)
    n_rest3 = 3 * (n_coeffs(l_max) - 1)
    sh = _scatter(mask, c2g, grads["sh"], n_rest3) if n_rest3 else np.zeros((len(mask), 0), com.dtype)
    return np.concatenate([com[:, :3], _scatter(mask, c2g, grads["rgb"], 3), sh, com[:, 3:]], 1)


def factored_rows(mask, c2g, grads, rank, world):
    mask = np.asarray(mask).astype(bool)
    com = common_rows(mask, c2g, grads)
    slots = np.zeros((len(mask), 3 * world), com.dtype)
    slots[:, 3 * rank:3 * rank + 3] = _scatter(mask, c2g, grads["precompute_rgb"], 3)
    return np.concatenate([com, slots], 1)


def split_rows(mask, c2g, grads):
    """(common[N,12], rgb[N,3])."""
    mask = np.asarray(mask).astype(bool)
    return common_rows(mask, c2g, grads), _scatter(mask, c2g, grads["precompute_rgb"], 3)


def uv_norm(mask, c2g, grad_uv):
    """sqrt(u^2 + v^2) in float64, per global row (0 where culled)."""
    mask = np.asarray(mask).astype(bool)
    g = np.asarray(grad_uv, np.float64).reshape(-1, 2)
    return _scatter(mask, c2g, np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2), 1)[:, 0]


# ---------------------------------------------------------------------------------------------- SH rebuild
def _orc():
    from oracle import oracle
    return oracle


def rank_terms(xyz, campos, g_rgb, l_max, dtype=np.float64):
    """[N, 3n]: g_rgb (x) Y_k(dir(xyz, campos)) of one rank, band 0 first; zero where the g_rgb row is all zero."""
    xyz = np.asarray(xyz).reshape(-1, 3)
    g_rgb = np.asarray(g_rgb).reshape(-1, 3)
    N = len(xyz)
    sh_grad, band0_grad, _ = _orc().precompute_spherical_harmonics_backward(
        xyz, np.zeros((N, 3)), np.zeros((N, n_coeffs(l_max) - 1, 3)), campos, g_rgb, l_max, dtype=dtype)
    term = np.concatenate([band0_grad, sh_grad.reshape(N, -1)], 1)
    term[(g_rgb == 0).all(1)] = 0
    return term


def basis(xyz, campos, l_max):
    """[N, n]: Y_k of the direction from campos to every gaussian, float64 (the rebuild with g_rgb = 1)."""
    N = len(np.asarray(xyz).reshape(-1, 3))
    return rank_terms(xyz, campos, np.ones((N, 3)), l_max)[:, 0::3]


def sh_rebuild(xyz, campos_all, rgb_all, l_max, dtype=np.float64, skip=()):
    """[N, 3n] = sum over ranks (in order, in `dtype`) of rank_terms; `skip`: (rank, row) pairs left out."""
    rgb_all = np.asarray(rgb_all)
    N = rgb_all.shape[1]
    acc = np.zeros((N, 3 * n_coeffs(l_max)), dtype)
    for r in range(rgb_all.shape[0]):
        term = rank_terms(xyz, np.asarray(campos_all)[r], rgb_all[r], l_max, dtype).astype(dtype)
        for rr, row in skip:
            if rr == r:
                term[row] = 0
        acc = (acc + term).astype(dtype)
    return acc


def rebuild_scale(xyz, campos_all, rgb_all, l_max):
    """(S[N,3n], Ybar): S_ic = sum_r |g^r_ic| repeated over k, Ybar = max |Y_k| over every rank's directions."""
    rgb_all = np.asarray(rgb_all, np.float64)
    S = np.tile(np.abs(rgb_all).sum(0), (1, n_coeffs(l_max)))
    ybar = max(np.abs(basis(xyz, c, l_max)).max() for c in np.asarray(campos_all))
    return S, float(ybar)


def rebuild_bound(xyz, campos_all, rgb_all, l_max):
    S, ybar = rebuild_scale(xyz, campos_all, rgb_all, l_max)
    return K[l_max] * U * S * ybar


# ---------------------------------------------------------------------------------------------------- unpack
def _assemble(common, sh, l_max):
    n3 = 3 * n_coeffs(l_max)
    full = np.zeros((len(common), 12 + n3), np.result_type(common.dtype, sh.dtype))
    full[:, :3], full[:, 3:3 + n3], full[:, 3 + n3:] = common[:, :3], sh, common[:, 3:]
    return full


def unpack_split(common, rgb_all, campos_all, xyz, l_max, dtype=np.float64):
    """full[N, 12 + 3n] from common[N,12] (already summed over the ranks) and rgb_all[W,N,3]."""
    return _assemble(np.asarray(common), sh_rebuild(xyz, campos_all, rgb_all, l_max, dtype), l_max)


def unpack_factored(factored, campos_all, xyz, l_max, dtype=np.float64):
    """full[N, 12 + 3n] from the summed factored rows [N, 12 + 3W]."""
    factored = np.asarray(factored)
    W = (factored.shape[1] - 12) // 3
    rgb_all = np.stack([factored[:, 12 + 3 * r:15 + 3 * r] for r in range(W)])
    return unpack_split(factored[:, :12], rgb_all, campos_all, xyz, l_max, dtype)


# ------------------------------------------------------------------------------- the GPU tests' synthetic inputs
def synthetic_case(N, l_max, world, seed=20):
    """Inputs of the unpack tests, float32: xyz[N,3], campos[W,3], common[N,12], rgb[W,N,3], and `pinned` = (rank, row):
    that rank's camera sits ON that gaussian, whose g_rgb in that rank is zero (the skip rule).
    About a third of the (rank, row) g_rgb entries are exactly zero; rows with i % 13 == 3 are zero in every rank; with two
    ranks or more, rank 1's camera is 1e-3 away from rank 0's and on rows with i % 11 == 5 its g_rgb is -(1 + 2^-10)
    times rank 0's, so that the two terms cancel to a thousandth of their size."""
    rng = np.random.default_rng([seed, N, l_max, world])
    xyz = (2.0 * rng.standard_normal((N, 3))).astype(np.float32)
    campos = (3.0 * rng.standard_normal((world, 3))).astype(np.float32)
    rgb = rng.standard_normal((world, N, 3)) * 10.0 ** rng.uniform(-4, 0, (world, N, 1))
    rgb[rng.random((world, N)) < 0.3] = 0.0
    rgb = rgb.astype(np.float32)
    rows = np.arange(N)
    pinned = (0, N // 2)
    campos[0] = xyz[pinned[1]]
    if world > 1:
        campos[1] = campos[0] + np.float32(1e-3) * rng.standard_normal(3).astype(np.float32)
        cancel = rows % 11 == 5
        rgb[0, cancel] = (rng.standard_normal((int(cancel.sum()), 3)) + 2.0).astype(np.float32)
        rgb[1, cancel] = -(rgb[0, cancel] * np.float32(1.0 + 2.0 ** -10))
    rgb[:, rows % 13 == 3] = 0.0
    rgb[pinned[0], pinned[1]] = 0.0
    common = rng.standard_normal((N, 12)).astype(np.float32)
    common[:, 11] = rng.integers(0, world + 1, N)
    return dict(xyz=xyz, campos=campos, common=common, rgb=rgb, pinned=pinned)

"""float64 reference of the four MCMC densification kernels (3dgs_amd/csrc/gs_density.hip: gsplat_sample_by_weight,
gsplat_mcmc_relocate, gsplat_mcmc_add_noise, gsplat_mcmc_regularize), in numpy and plain python.

The random bits are the kernels' own (splitmix64 with np.uint64 wrap-around), so the sampler is compared bit for bit; the
normals are Box-Muller in float64 from the same bit fields the kernels feed to float32 logf / cosf."""
import math

import numpy as np

_M64 = (1 << 64) - 1
FLT_ONE_MINUS_EPS = 1.0 - 1.1920929e-7
RELOCATE_MAX_N = 51
LOG_FLT_MAX = math.log(float(np.finfo(np.float32).max))  # expf of anything larger is inf in float32


def splitmix64(x):
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def bits(seed, counters):
    """bits(seed, c) = splitmix64(splitmix64(seed) ^ (c * 0xD1342543DE82EF95 + 1)) for an array of counters."""
    c = np.asarray(counters, np.uint64)
    with np.errstate(over="ignore"):
        return splitmix64(splitmix64(np.uint64(int(seed) & _M64)) ^ (c * np.uint64(0xD1342543DE82EF95) + np.uint64(1)))


def uniform(seed, counters):
    """u in [0, 1): the 53 high bits."""
    return (bits(seed, counters) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def normal(seed, counters):
    """Box-Muller on the two 24-bit fields: u1 in (0, 1], u2 in [0, 1)."""
    b = bits(seed, counters)
    u1 = ((b >> np.uint64(40)) + np.uint64(1)).astype(np.float64) / 16777216.0
    u2 = ((b >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


NORMAL_MAX = math.sqrt(2.0 * math.log(2.0 ** 24))  # u1 = 2^-24: 5.77, the largest normal the generator can emit


def sample_by_weight(weights, K, seed):
    """(samples [K], counts [N]) of K draws; cdf as the caller of the kernel builds it (float64 cumulative sum)."""
    cdf = np.cumsum(np.asarray(weights, np.float64))
    total = cdf[-1]
    assert total > 0
    t = np.minimum(uniform(seed, np.arange(K)) * total, np.nextafter(total, 0.0))
    samples = np.searchsorted(cdf, t, side="right")  # the smallest i with cdf[i] > t
    return samples.astype(np.int32), np.bincount(samples, minlength=len(cdf)).astype(np.int32)


def relocation(o, n):
    """(o', coefficient): the opacity of each of n coincident copies of a gaussian of opacity o and the factor on its
    scale, o / den, with the double sum as the paper writes it."""
    on = -math.expm1(math.log1p(-o) / n) if o < 1.0 else 1.0
    den = math.fsum(math.comb(i - 1, k) * (-1) ** k * on ** (k + 1) / math.sqrt(k + 1)
                    for i in range(1, n + 1) for k in range(i))
    return on, o / den


def relocate(opacity_logit, log_scale, counts, min_opacity):
    """New (logits [N], log-scales [N,3]) in float64; rows with counts <= 0 (or o == 0) keep their values."""
    logit = np.asarray(opacity_logit, np.float64).copy()
    scale = np.asarray(log_scale, np.float64).copy()
    for i, cnt in enumerate(np.asarray(counts)):
        if cnt <= 0:
            continue
        n = min(int(cnt) + 1, RELOCATE_MAX_N)
        o = 1.0 / (1.0 + math.exp(-logit[i]))
        if o == 0.0:
            continue
        on, coef = relocation(o, n)
        scale[i] += math.log(coef)
        oc = min(max(on, float(min_opacity)), FLT_ONE_MINUS_EPS)
        logit[i] = math.log(oc / (1.0 - oc))
    return logit, scale


def rotation(quaternion):
    """[N,3,3] from un-normalised (w, x, y, z) rows."""
    q = np.asarray(quaternion, np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def gate(opacity_logit):
    """g = 1 / (1 + exp(100 (o - 0.005))); where float32's expf overflows the kernel's gate is exactly 0, by definition."""
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity_logit, np.float64)))
    x = 100.0 * (o - 0.005)
    return np.where(x > LOG_FLT_MAX, 0.0, 1.0 / (1.0 + np.exp(np.minimum(x, LOG_FLT_MAX))))


def noise(opacity_logit, log_scale, quaternion, scaler, seed):
    """(displacement [N,3], gate [N], row sums of |Sigma| [N,3])."""
    R = rotation(quaternion)
    e2 = np.exp(np.asarray(log_scale, np.float64)) ** 2
    sigma = np.einsum("nak,nk,nbk->nab", R, e2, R)
    g = gate(opacity_logit)
    N = len(g)
    nu = normal(seed, np.arange(3 * N)).reshape(N, 3) * g[:, None] * float(scaler)
    return np.einsum("nab,nb->na", sigma, nu), g, np.abs(sigma).sum(2)


def regularize(compact_to_global, opacity_logit, log_scale, w_opacity, w_scale):
    """The two additions (to grad_opacity [M], to grad_scale [M,3])."""
    i = np.asarray(compact_to_global)
    s = 1.0 / (1.0 + np.exp(-np.asarray(opacity_logit, np.float64)[i]))
    return w_opacity * s * (1.0 - s), w_scale * np.exp(np.asarray(log_scale, np.float64)[i])

"""The forward in float64 with, for every output element, the float32 rounding error a correct evaluation may carry.

The bar is tests/grad_bound.py's: every element  |got - value64| <= K u unit + borderline,  u = 2^-24.  `unit` is the
element's absolute float32 error in multiples of u, by first-order running-error propagation; `borderline` is what the
step functions on the path (alpha > 1/255, T (1 - alpha) < 1e-4, ceil, the cull) are worth where two correct float32
evaluations may decide them differently.  Two stages, each from float32 inputs widened to float64:

STAGE A, the per-gaussian forward in plain mode (per_gaussian): leaf parameters and camera -> xyz_c, uv, sigma, J, conic,
rgb, the two pre-ceil extents rho = mh_dist sqrt(lambda_1,2), the orientation angle theta.  The units come from the value
type E below, which carries (value, e) through + - * / sqrt exp: a result's e is what its operands' e are worth through
the partial derivatives' magnitudes, plus |result| for its own rounding (a product with a power of two is exact; exp,
a library function, counts two).  Every product of a sum is rounded, so every addend of every sum enters by its
magnitude, and every input's own unit by |d result / d input|.  The statements are those of oracle/gsplat_oracle_impl.h
in its order; 3dgs_amd/csrc/gs_math.h (camera_space, to_screen, rot_scale, sigma_from, jacobian, mv_from, conic_radius,
view_dir, sh_basis, sh_to_rgb) forms every quantity of this stage by the same statements, so one walk serves both (the
kernels' sincosf and expf against libm are inside the library-function allowance).  Where each term enters:

  xyz_c   sum_j |R_kj x_j| from the three products, the partial sums and |t_k| through the additions.
  uv      the clip-space sums x_clip, y_clip, w_clip as above; ndc = clip / (w + 1e-6): e_clip / |w| + |ndc| e_w / |w|;
          then (ndc 0.5 + 0.5) W: the addition's rounding is |ndc 0.5 + 0.5| W, so a uv near 0 carries the bar of a
          coordinate of size W / 2 (its ndc error is scaled by W / 2 whatever uv is).
  sigma   the quaternion's norm and the division by norm + 1e-6; 1 - 2 (y^2 + z^2), 2 (xy -+ wz) as differences (their
          operands' roundings stay when the difference is small); exp(scale) with the error of its argument (none: the
          argument is an input) and the library's own; the three-product sums R S S R^T by their magnitudes.
  J       fx / z and -(fx x) / z^2 with x the CLAMPED coordinate min(lim, max(-lim, x / z)) z: the clamp is continuous,
          a row beyond it takes lim = 1.3 tan_fov (two roundings) instead of x / z, only the derivative changes.
  conic   M = J W, V = Sigma M^T, cov = M V + 0.3 I with all their term sums; det = cov00 cov11 - cov01^2 carries
          |cov00 cov11| + cov01^2 from its two products plus the propagated parts; a conic element entry / det carries
          relatively e_entry / |entry| + e_det / |det|, which is what makes a needle's bar wide and nobody else's.
  rgb     the direction (xyz - campos) / (|.| + 1e-9); every basis function by the sum of its monomials' magnitudes
          (E walks the polynomial: Y_k near a nodal line keeps the error of its terms; per element, not a global 1.5);
          the SH constants are float32 roundings of the real constants, one u each; the sum over coefficients by
          magnitude, plus 0.5.  This project's SH forward has no clamp at 0 (oracle: "no clamp, no sigmoid", and
          sh_to_rgb likewise), so no clamp borderline exists: a negative colour must come out negative.
  rho     mid +- sqrt(max(0.1, mid^2 - det)), mid = (cov00 + cov11) / 2: lambda_2 is again a difference; below the 0.1
          floor the root is the constant's.  sqrt and the product with mh_dist follow.
  theta   0.5 atan2(y, x), y = 2 cov01, x = cov00 - cov11: e = 0.5 (|x| e_y + |y| e_x) / (x^2 + y^2) + |theta| + the
          library's two: it grows like 1 / (lambda_1 - lambda_2).  On atan2's cut (x < 0, y within its bar of 0) theta may
          come out half a turn away: (sin, cos) with the other sign, the same axis.

decisions of stage A (mask_terms, radius_failures): see those functions.

STAGE B, the compositing forward (compositing): the record's uv, conic, rgb, the input opacity logit of the compacted
rows, sorted and ranges -> per pixel image, T, n (and in depth mode the auxiliary channels of tests/depth_reference.py /
depth_moment_reference.py).  The walk is per list position over all tiles at once, as render_bwd_reference's
compositing_sums walks backwards.  Per composited entry i of a pixel:

  alpha_i = min(0.99, sigma exp(power)): relative error  ra_i = pw_i + rs + 2, with pw_i the sum of the magnitudes of
      the power's terms -- the oracle's row polynomial on the lane's base row, basic + linear i + quad i^2, or the
      kernels' 2^(a2 dx^2 + b2 dx dy + c2 dy^2 + log2 sigma) on the pixel's own offsets (gs_render.h: stage_record,
      staged_alpha_capped), whose exponent carries |ln sigma| as a term: whichever sum is larger -- and rs = (1 - sigma)
      (|logit| + 2) + 2 the error of sigma = 1 / (1 + exp(-logit)).  A clamped alpha is 0.99 within CLAMP_REL (the
      kernels cap in the exponent domain, two ulps under log2 0.99).
  T_i = prod_{j<i} (1 - alpha_j): relative error  rT_i = sum_{j<i} (1 + alpha_j / (1 - alpha_j) ra_j).  T_final's unit is
      T_final rT_final: over 140 entries it reaches 1e3 u relative, by construction.
  a channel: sum_i |c_i| w_i (1 + rc + ra_i + rT_i) + |acc_i| (the running sum's own rounding) and at the end
      |bg| T_final (1 + rT_final) + |value|; rc is the colour's own error (0 for a stored colour, LIB for 1/z, 2 LIB + 1 for its
      square).  A pixel that composites nothing is bg exactly: unit 0.  alpha = 1 - T adds 1 + T.
  the segmented forward (gs_render_fwd.hip: fwd_segments_combine_kernel, gs_render.h: TileSegments): a list longer than
      SEG_SPLIT_MIN is walked in segments of SEG_ENTRIES; a segment's partial colour is formed from the published prefix
      transmittance and added to the sum of the segments in front.  Per boundary a pixel passes: one more rounding of T
      (rT + 1) and of the sum (|acc| at the boundary), and once the segments' own products (sum |c| w).

borderline, per pixel, exact to first order: for every (pixel, entry) whose float64 alpha lies within ALPHA_REL_TOL of
1/255 (composited or not) |alpha_i T_i (c_i - B_i)| with B_i the float64 colour behind entry i, and alpha_i T_final for T.
The stop: at the first entry whose T (1 - alpha) lies within T_REL_TOL (plus the alphas of the borderline pairs in front,
which move T by that much) of 1e-4 a second walk takes the other decision; its image, T and n against the first walk's
are the borderline terms, and n may be either walk's -- on every other pixel n is the float64 n."""
import numpy as np

U = 2.0 ** -24
ALPHA_REL_TOL = 2e-3   # parity_tools.explain: alpha_rel_tol, as render_bwd_reference
T_REL_TOL = 2e-3       # parity_tools.explain: the same figure for T (1 - alpha) against 1e-4
SLACK_TOL_PX = 1e-3    # parity_tools.explain: slack_tol_px
CLAMP_REL = 4.0
SEG_ENTRIES, SEG_SPLIT_MIN = 496, 1488  # gs_render.h: kSegEntries, kSegSplitMin
LIB = 2.0              # a library function (exp, atan2, sin, cos): one ulp = 2 u


def f32c(c):
    """A float literal of the sources ((R)0.3f): rounded to float32, then exact."""
    return float(np.float32(c))


class E:
    """(value, e): e is the absolute error, in multiples of u, a correct float32 evaluation of the value may carry."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(np.float64(x))

    @staticmethod
    def rounded(c):
        """A real constant stored as its float32 rounding."""
        return E(np.float64(c), abs(c))

    def __neg__(self):
        return E(-self.v, self.e)

    def __add__(self, o):
        o = E.of(o)
        v = self.v + o.v
        exact = ((self.v == 0) & (self.e == 0)) | ((o.v == 0) & (o.e == 0))  # an exact zero added: no rounding
        return E(v, self.e + o.e + np.where(exact, 0.0, np.abs(v)))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-E.of(o))

    def __rsub__(self, o):
        return E.of(o) + (-self)

    def __mul__(self, o):
        exact = not isinstance(o, E) and float(o) != 0 and np.frexp(abs(float(o)))[0] == 0.5  # a power of two
        o = E.of(o)
        v = self.v * o.v
        with np.errstate(invalid="ignore"):
            e = np.abs(self.v) * o.e + np.abs(o.v) * self.e
        return E(v, np.nan_to_num(e, posinf=np.inf) + (0.0 if exact else np.abs(v)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            e = self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v) + np.abs(v)
        return E(v, e)

    def __rtruediv__(self, o):
        return E.of(o) / self


def e_sqrt(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.sqrt(a.v)
        e = np.where(a.e > 0, a.e / (2 * v), 0.0) + np.abs(v)
    return E(v, e)


def e_exp(a):
    v = np.exp(a.v)
    return E(v, v * a.e + LIB * v)


def e_where(m, a, b):
    a, b = E.of(a), E.of(b)
    return E(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def e_clip(a, lim):
    """min(lim, max(-lim, a))"""
    return e_where(a.v > lim.v, lim, e_where(a.v < -lim.v, -lim, a))


def _cols(a, rows=None):
    a = np.asarray(a, np.float32).astype(np.float64)
    a = a.reshape(len(a), -1)
    return [E(a[:, j]) for j in range(a.shape[1])]


def _stack(es):
    return np.stack([x.v for x in es], 1), np.stack([x.e for x in es], 1)


SH_C = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396,
        0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277)


def _sh_basis(l_max, x, y, z):
    C = [E.rounded(c) for c in SH_C]
    Y = [C[0]]
    if l_max >= 1:
        Y += [C[1] * y, C[1] * z, C[1] * x]
    if l_max >= 2:
        xx, yy, zz = x * x, y * y, z * z
        Y += [C[2] * (x * y), C[2] * (y * z), C[3] * (2.0 * zz - xx - yy), C[2] * (x * z), C[4] * (xx - yy)]
    if l_max >= 3:
        Y += [C[5] * (y * (3.0 * xx - yy)), C[6] * (x * y * z), C[7] * (y * (4.0 * zz - xx - yy)),
              C[8] * (z * (2.0 * zz - 3.0 * xx - 3.0 * yy)), C[7] * (x * (4.0 * zz - xx - yy)), C[9] * (z * (xx - yy)),
              C[5] * (x * (xx - 3.0 * yy))]
    return Y


def per_gaussian(params, cam, mh_dist, l_max):
    """Stage A for ALL rows of `params` (float32 leaves: xyz rgb sh scale quaternion): dict name -> (value64, unit),
    [N, d] each, for xyz_c uv sigma J conic rgb rho (2: major, minor; NaN where lambda_2 < 0), plus theta (value, e) [N],
    lambda2 (value, e) [N] and tan_fov."""
    with np.errstate(all="ignore"):
        return _per_gaussian(params, cam, mh_dist, l_max)


def _per_gaussian(params, cam, mh_dist, l_max):
    N = len(params["xyz"])
    W, H = int(cam["width"]), int(cam["height"])
    view = np.asarray(cam["view"], np.float32).astype(np.float64).reshape(16)
    proj = np.asarray(cam["proj"], np.float32).astype(np.float64).reshape(16)
    campos = np.asarray(cam["campos"], np.float32).astype(np.float64).reshape(3)
    fx, fy = f32c(cam["fx"]), f32c(cam["fy"])
    out = {}
    wx, wy, wz = _cols(params["xyz"])
    # P1 camera_space
    x = view[0] * wx + view[1] * wy + view[2] * wz + view[3]
    y = view[4] * wx + view[5] * wy + view[6] * wz + view[7]
    z = view[8] * wx + view[9] * wy + view[10] * wz + view[11]
    out["xyz_c"] = _stack([x, y, z])
    # P2 to_screen
    xc = proj[0] * x + proj[1] * y + proj[2] * z + proj[3]
    yc = proj[4] * x + proj[5] * y + proj[6] * z + proj[7]
    wc = proj[12] * x + proj[13] * y + proj[14] * z + proj[15]
    den = wc + f32c(1e-6)
    u = ((xc / den) * 0.5 + 0.5) * float(W)
    v = ((yc / den) * 0.5 + 0.5) * float(H)
    out["uv"] = _stack([u, v])
    # G1 rot_scale, sigma_from
    qw, qx, qy, qz = _cols(params["quaternion"])
    inv = 1.0 / (e_sqrt(qw * qw + qx * qx + qy * qy + qz * qz) + f32c(1e-6))
    qw, qx, qy, qz = qw * inv, qx * inv, qy * inv, qz * inv
    x2, y2, z2, xy, xz, yz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz
    wqx, wqy, wqz = qw * qx, qw * qy, qw * qz
    r00, r01, r02 = 1.0 - 2.0 * (y2 + z2), 2.0 * (xy - wqz), 2.0 * (xz + wqy)
    r10, r11, r12 = 2.0 * (xy + wqz), 1.0 - 2.0 * (x2 + z2), 2.0 * (yz - wqx)
    r20, r21, r22 = 2.0 * (xz - wqy), 2.0 * (yz + wqx), 1.0 - 2.0 * (x2 + y2)
    sx, sy, sz = (e_exp(s) for s in _cols(params["scale"]))
    rs00, rs10, rs20 = r00 * sx, r10 * sx, r20 * sx
    rs01, rs11, rs21 = r01 * sy, r11 * sy, r21 * sy
    rs02, rs12, rs22 = r02 * sz, r12 * sz, r22 * sz
    s00 = rs00 * rs00 + rs01 * rs01 + rs02 * rs02
    s01 = rs00 * rs10 + rs01 * rs11 + rs02 * rs12
    s02 = rs00 * rs20 + rs01 * rs21 + rs02 * rs22
    s11 = rs10 * rs10 + rs11 * rs11 + rs12 * rs12
    s12 = rs10 * rs20 + rs11 * rs21 + rs12 * rs22
    s22 = rs20 * rs20 + rs21 * rs21 + rs22 * rs22
    out["sigma"] = _stack([s00, s01, s02, s11, s12, s22])
    # G2a jacobian
    tan_x, tan_y = E(float(W)) / E(2.0 * fx), E(float(H)) / E(2.0 * fy)
    limx, limy = f32c(1.3) * tan_x, f32c(1.3) * tan_y
    cx, cy = e_clip(x / z, limx) * z, e_clip(y / z, limy) * z
    flat = np.abs(z.v) < f32c(1e-6)
    zero = E(np.zeros(N))
    j00, j02 = e_where(flat, zero, fx / z), e_where(flat, zero, -(fx * cx) / (z * z))
    j11, j12 = e_where(flat, zero, fy / z), e_where(flat, zero, -(fy * cy) / (z * z))
    j01 = j10 = zero
    out["J"] = _stack([j00, j01, j02, j10, j11, j12])
    # G2b mv_from, conic_radius
    w00, w01, w02, w10, w11, w12, w20, w21, w22 = (view[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    m00, m01, m02 = j00 * w00 + j01 * w10 + j02 * w20, j00 * w01 + j01 * w11 + j02 * w21, j00 * w02 + j01 * w12 + j02 * w22
    m10, m11, m12 = j10 * w00 + j11 * w10 + j12 * w20, j10 * w01 + j11 * w11 + j12 * w21, j10 * w02 + j11 * w12 + j12 * w22
    v00, v01 = s00 * m00 + s01 * m01 + s02 * m02, s00 * m10 + s01 * m11 + s02 * m12
    v10, v11 = s01 * m00 + s11 * m01 + s12 * m02, s01 * m10 + s11 * m11 + s12 * m12
    v20, v21 = s02 * m00 + s12 * m01 + s22 * m02, s02 * m10 + s12 * m11 + s22 * m12
    cov00 = m00 * v00 + m01 * v10 + m02 * v20 + f32c(0.3)
    cov01 = m00 * v01 + m01 * v11 + m02 * v21
    cov11 = m10 * v01 + m11 * v11 + m12 * v21 + f32c(0.3)
    det = cov00 * cov11 - cov01 * cov01
    inv_det = 1.0 / det
    out["conic"] = _stack([cov11 * inv_det, (-cov01) * inv_det, cov00 * inv_det])
    out["cov"] = _stack([cov00, cov01, cov11])
    out["det"] = (det.v, det.e)
    mid = 0.5 * (cov00 + cov11)
    disc = mid * mid - det
    root = e_sqrt(e_where(disc.v > f32c(0.1), disc, E(np.full(N, f32c(0.1)))))
    l1, l2 = mid + root, mid - root
    out["rho"] = _stack([float(mh_dist) * e_sqrt(l1), float(mh_dist) * e_sqrt(l2)])
    out["lambda2"] = (l2.v, l2.e)
    ty, tx = 2.0 * cov01, cov00 - cov11
    theta = 0.5 * np.arctan2(ty.v, tx.v)
    out["theta"] = (theta, 0.5 * (np.abs(tx.v) * ty.e + np.abs(ty.v) * tx.e) / (tx.v ** 2 + ty.v ** 2) + np.abs(theta) + LIB)
    out["theta_yx"] = (ty.v, ty.e, tx.v)
    # S1 view_dir, sh_to_rgb
    dx, dy, dz = wx - campos[0], wy - campos[1], wz - campos[2]
    ln = e_sqrt(dx * dx + dy * dy + dz * dz) + f32c(1e-9)
    Y = _sh_basis(l_max, dx / ln, dy / ln, dz / ln)
    band0 = _cols(params["rgb"])
    nc = (l_max + 1) ** 2
    sh = None if nc == 1 else np.asarray(params["sh"], np.float32).astype(np.float64).reshape(N, -1)[:, :(nc - 1) * 3]
    rgb = []
    for ch in range(3):
        acc = band0[ch] * Y[0] + 0.5
        for k in range(nc - 1):
            acc = acc + E(sh[:, 3 * k + ch]) * Y[k + 1]
        rgb.append(acc)
    out["rgb"] = _stack(rgb)
    out["tan_fov"] = (tan_x.v, tan_y.v)
    return out


ROW_ARRAYS = ("xyz_c", "uv", "sigma", "J", "conic", "rgb")


def mask_terms(pg, cfg, W, H, K_xyz, K_uv):
    """(mask64 [N], free [N]): the float64 keep decision, and the rows whose z, u or v lies within its bar (K u unit) of
    near_thresh or the padded image bounds -- those may go either way, every other row must equal mask64."""
    z, ez = pg["xyz_c"][0][:, 2], pg["xyz_c"][1][:, 2]
    uv, euv = pg["uv"]
    pad = float(int(cfg["cull_mask_padding"]))
    near = f32c(cfg["near_thresh"])
    with np.errstate(invalid="ignore"):
        keep = (z >= near) & (uv[:, 0] >= -pad) & (uv[:, 0] <= W + pad) & (uv[:, 1] >= -pad) & (uv[:, 1] <= H + pad)
        free = np.abs(z - near) <= K_xyz * U * ez
        for col, hi in ((0, W + pad), (1, H + pad)):
            bar = K_uv * U * euv[:, col]
            free |= (np.abs(uv[:, col] + pad) <= bar) | (np.abs(uv[:, col] - hi) <= bar)
    return keep, free & np.isfinite(z)


def radius_terms(pg, rows, K):
    """For the compacted rows: (ceil64 [M, 2], either [M, 2], nan_must [M], nan_may [M], theta, e_theta): either -- an
    integer lies within the bar of rho64, both neighbours pass; r_minor is NaN exactly where lambda_2 is below minus its
    bar, and may be where |lambda_2| is within it."""
    rho, erho = pg["rho"][0][rows], pg["rho"][1][rows]
    l2, el2 = pg["lambda2"][0][rows], pg["lambda2"][1][rows]
    bar = K * U * erho
    with np.errstate(invalid="ignore"):
        either = ((np.ceil(rho - bar) != np.ceil(rho + bar)) | ~np.isfinite(bar)) & ~np.isnan(rho)
    nan_may = np.abs(l2) <= K * U * el2
    nan_must = (l2 < 0) & ~nan_may
    # lambda_2 within its bar of 0: rho_minor is sqrt of it, anything from NaN to mh sqrt(bar) -- free
    either[:, 1] |= nan_may
    return np.ceil(rho), either, nan_must, nan_may, pg["theta"][0][rows], pg["theta"][1][rows]


def radius_failures(radius, pg, rows, K):
    """Holds a [M, 4] radius array {r_major, r_minor, sin, cos} to the float64 decisions; returns (list of messages,
    dict of figures)."""
    radius = np.asarray(radius, np.float64).reshape(-1, 4)
    want, either, nan_must, nan_may, th, eth = radius_terms(pg, rows, K)
    msgs = []
    got = radius[:, :2]
    isnan = np.isnan(got)
    if isnan[:, 0].any():
        msgs.append(f"{int(isnan[:, 0].sum())} NaN major radii")
    bad_nan = (isnan[:, 1] != nan_must) & ~nan_may
    if bad_nan.any():
        msgs.append(f"r_minor NaN where lambda_2 is clear of 0 (or the reverse) on {int(bad_nan.sum())} rows, first {int(np.nonzero(bad_nan)[0][0])}")
    with np.errstate(invalid="ignore"):
        exact = (got == want) | (isnan & np.isnan(want))
        near = np.abs(got - want) <= 1.0
    bad = ~exact & ~(either & (near | isnan | np.isnan(want)))
    bad[:, 1] &= ~nan_may
    if bad.any():
        r, c = np.argwhere(bad)[0]
        msgs.append(f"radius[{r}, {c}] = {got[r, c]} but ceil(rho64) = {want[r, c]} (rho64 {pg['rho'][0][rows][r, c]:.9g}, "
                    f"bar {K * U * pg['rho'][1][rows][r, c]:.3g}); {int(bad.sum())} such")
    s, c = radius[:, 2], radius[:, 3]
    loose = ~(eth < 1.0 / (K * U))  # K u e_theta >= 1: the near-isotropic splat
    bar = K * U * (eth + 1.0 + LIB)
    err = np.maximum(np.abs(s - np.sin(th)), np.abs(c - np.cos(th)))
    # atan2's cut: with x < 0 and y within its bar of 0 the angle 2 theta may come out near +pi or -pi, theta half a turn
    # apart, (sin, cos) with the other sign -- the same axis
    y, ey, x = (a[rows] for a in pg["theta_yx"])
    cut = (x < 0) & (np.abs(y) <= K * U * ey)
    err = np.where(cut, np.minimum(err, np.maximum(np.abs(s + np.sin(th)), np.abs(c + np.cos(th)))), err)
    bad_t = ~loose & ~(err <= bar)
    if bad_t.any():
        r = int(np.argmax(np.where(bad_t, err / bar, 0)))
        msgs.append(f"(sin, cos)[{r}] = ({s[r]:.9g}, {c[r]:.9g}) off theta64 {th[r]:.9g} by {err[r]:.3g} > {bar[r]:.3g}; {int(bad_t.sum())} such")
    unit_norm = np.abs(s * s + c * c - 1.0)
    if not (unit_norm <= 8 * U).all():
        msgs.append(f"sin^2 + cos^2 off 1 by {np.nanmax(unit_norm):.3g}")
    with np.errstate(invalid="ignore", divide="ignore"):
        worst_t = float(np.nanmax(np.where(loose, 0.0, err / (U * (eth + 1.0 + LIB))))) if len(th) else 0.0
    figs = dict(either=int(either.any(1).sum()), nan=int(isnan[:, 1].sum()), loose_theta=int(loose.sum()), theta_ratio=worst_t,
                differs=int((~exact).any(1).sum()))
    return msgs, figs


def list_failures(orc, record, W, H):
    """sorted and ranges against orc.get_sorted_gaussian_list on the record's OWN uv, xyz_c and radius: an instance may
    differ only where parity_tools.sat_slack is within SLACK_TOL_PX."""
    import parity_tools
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    s, r, _ = orc.get_sorted_gaussian_list(record["uv"], record["xyz_c"], record["radius"], ntx, nty)
    got_s, got_r = np.asarray(record["sorted"]), np.asarray(record["ranges"])
    if len(s) == len(got_s) and (s == got_s).all() and (np.asarray(r) == got_r).all():
        return [], dict(differ=0)
    kg, kr = parity_tools.instance_keys(got_s, got_r), parity_tools.instance_keys(s, r)
    diff = np.concatenate([np.setdiff1d(kg, kr), np.setdiff1d(kr, kg)])
    msgs = []
    if len(diff):
        tile, g = (diff >> 32).astype(np.int64), (diff & 0xFFFFFFFF).astype(np.int64)
        slack = np.abs(parity_tools.sat_slack(record["uv"], record["radius"], g, tile, ntx))
        if not (slack <= SLACK_TOL_PX).all():
            msgs.append(f"{int((slack > SLACK_TOL_PX).sum())} instances differ although the OBB clears the tile edge by up to {slack.max():.3g} px")
    else:
        msgs.append("the same instances in another order")
    return msgs, dict(differ=int(len(diff)))


# ------------------------------------------------------------------------------------------------------------ stage B
def sigmoid_terms(logit):
    """sigma = 1 / (1 + exp(-logit)) in float64 and its relative error in u.  The kernels' form sets it (gs_render.h:
    sigmoid_fast evaluates exp as 2^(-l log2 e), whose argument's rounding is worth |l|): exp(-l) is off by |l| + LIB
    relatively, 1 + exp(-l) by (1 - sigma) times that plus its own rounding, the quotient by one more."""
    l = np.asarray(logit, np.float32).astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-l))
    return s, (1.0 - s) * (np.abs(l) + LIB) + 2.0


def compositing(record, logit, bg, W, H, aux=None, aux_rel=None, segmented=False):
    """record: uv conic rgb sorted ranges (float32 / int32 as produced); logit: the opacity logits of the compacted rows.
    aux [M, k]: further channels composited over background 0 (float64 colours), aux_rel [k]: their colours' own relative
    error in u.  Returns dict: image, T (and aux) -> (value64, unit, borderline) with [H, W, C] / [H, W]; n64, n_alt
    [H, W] (the two stop indices a pixel may report; equal where nothing is borderline); composited [H, W] (entries
    composited); last_w, last_alpha, last_g [H, W] (weight, alpha and compacted row of the last composited entry)."""
    f8 = np.float64
    uv = np.asarray(record["uv"], np.float32).astype(f8).reshape(-1, 2)
    conic = np.asarray(record["conic"], np.float32).astype(f8).reshape(-1, 3)
    col = np.asarray(record["rgb"], np.float32).astype(f8).reshape(-1, 3)
    bgc = np.full(3, f32c(bg))
    crel = np.zeros(3)
    if aux is not None:
        aux = np.asarray(aux, f8).reshape(len(col), -1)
        col = np.concatenate([col, aux], 1)
        bgc = np.concatenate([bgc, np.zeros(aux.shape[1])])
        crel = np.concatenate([crel, np.zeros(aux.shape[1]) if aux_rel is None else np.asarray(aux_rel, f8)])
    C = col.shape[1]
    opa_all, rs_all = sigmoid_terms(logit)
    lnopa = np.abs(np.log(opa_all))
    sorted_ids, ranges = np.asarray(record["sorted"]), np.asarray(record["ranges"])
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    nt = ntx * nty
    t = np.arange(nt)
    ly, lx = np.divmod(np.arange(256), 16)
    px = (t % ntx)[:, None] * 16 + lx[None, :]
    py = (t // ntx)[:, None] * 16 + ly[None, :]
    by = (t // ntx)[:, None] * 16 + (ly // 8 * 8)[None, :]
    ii = np.broadcast_to((ly % 8).astype(f8)[None, :], px.shape)
    valid = (px < W) & (py < H)
    pxf, pyf, byf = px.astype(f8), py.astype(f8), by.astype(f8)
    length = np.diff(ranges)[:nt]
    split = segmented & (length > SEG_SPLIT_MIN)
    a_max, a_min, t_min = f32c(0.99), f32c(0.00392156862), f32c(0.0001)
    shape = px.shape
    # the two walks: 0 takes the float64 decisions, 1 the other decision at the first borderline stop
    T = np.ones((2,) + shape)
    acc = np.zeros((2,) + shape + (C,))
    n = np.zeros((2,) + shape, np.int64)
    done = np.zeros((2,) + shape, bool)
    done[:] = ~valid
    flipped = np.zeros(shape, bool)
    rT = np.zeros(shape)               # relative error of T, in u (walk 0)
    accabs = np.zeros(shape + (C,))    # sum |c| w
    unit = np.zeros(shape + (C,))
    ncomp = np.zeros(shape, np.int64)
    last_w, last_alpha = np.zeros(shape), np.zeros(shape)
    last_g = np.full(shape, -1, np.int64)
    cumnear = np.zeros(shape)
    near_rec = []                      # (tile, lane, w as if composited, colour, acc after, T after)
    top = int(length.max()) if nt else 0
    for idx in range(top):
        act = np.nonzero((length > idx) & ~done[:, :, :].all((0, 2)))[0]
        if not len(act):
            break
        g = sorted_ids[ranges[act] + idx]
        a, b, c = conic[g, 0][:, None], conic[g, 1][:, None], conic[g, 2][:, None]
        opa, rs = opa_all[g][:, None], rs_all[g][:, None]
        dx, dyb, dyp = uv[g, 0][:, None] - pxf[act], uv[g, 1][:, None] - byf[act], uv[g, 1][:, None] - pyf[act]
        i = ii[act]
        basic = -0.5 * (a * dx * dx + 2.0 * b * dx * dyb + c * dyb * dyb)
        linear, quad = c * dyb + b * dx, -0.5 * c
        with np.errstate(invalid="ignore", over="ignore"):
            power = np.minimum(0.0, basic + linear * i + quad * i * i)
            raw = opa * np.exp(power)
            alpha_c = np.minimum(a_max, raw)
            vs = alpha_c > a_min                                   # NaN: no splat
            nearp = np.abs(raw - a_min) <= ALPHA_REL_TOL * a_min
            pw_or = (0.5 * (np.abs(a) * dx * dx + 2.0 * np.abs(b * dx * dyb) + np.abs(c) * dyb * dyb)
                     + (np.abs(c * dyb) + np.abs(b * dx)) * i + 0.5 * np.abs(c) * i * i)
            pw_k = 0.5 * np.abs(a) * dx * dx + np.abs(b * dx * dyp) + 0.5 * np.abs(c) * dyp * dyp + lnopa[g][:, None]
        ra = np.where(raw >= a_max, CLAMP_REL, np.maximum(pw_or, pw_k) + rs + LIB)
        cg = col[g][:, None, :]
        if segmented and idx > 0 and idx % SEG_ENTRIES == 0:        # a boundary of the segmented forward
            pas = (split[act][:, None] & ~done[0][act])
            rT[act] += pas
            unit[act] += pas[..., None] * accabs[act]
        for k in (0, 1):
            reach = ~done[k][act]
            comp = reach & vs
            al = np.where(comp, alpha_c, 0.0)
            Tk = T[k][act]
            w = al * Tk
            acc_new = acc[k][act] + w[..., None] * cg
            test = Tk * (1.0 - al)
            stop = reach & (test < t_min)
            if k == 0:
                rTa = rT[act]
                cw = np.abs(cg) * w[..., None]
                unit[act] += cw * ((1.0 + ra + rTa)[..., None] + crel) + np.where(comp[..., None], np.abs(acc_new), 0.0)
                accabs[act] += cw
                with np.errstate(invalid="ignore"):
                    rT[act] = rTa + np.where(comp, 1.0 + al / (1.0 - al) * ra, 0.0)
                ncomp[act] += comp
                last_w[act] = np.where(comp, w, last_w[act])
                last_alpha[act] = np.where(comp, al, last_alpha[act])
                last_g[act] = np.where(comp, g[:, None], last_g[act])
                nr = reach & nearp
                cum = cumnear[act] + np.where(nr, alpha_c, 0.0)
                cumnear[act] = cum
                if nr.any():
                    ti, li = np.nonzero(nr)
                    T_after = np.where(comp, test, Tk)
                    near_rec.append((act[ti], li, (alpha_c * Tk)[ti, li], np.broadcast_to(cg, acc_new.shape)[ti, li],
                                     acc_new[ti, li], T_after[ti, li], alpha_c[ti, li]))
                flip = comp & ~flipped[act] & (np.abs(test - t_min) <= (T_REL_TOL + cum) * t_min)
                flipped[act] |= flip
            else:
                stop = stop ^ (flip & reach)
            n[k][act] += reach
            T[k][act] = np.where(reach, test, Tk)
            acc[k][act] = acc_new
            done[k][act] |= stop
    image = acc + T[..., None] * bgc
    any_c = (ncomp > 0)[..., None]
    unit = unit + np.where(any_c, np.abs(bgc) * (T[0] * (1.0 + rT))[..., None] + np.abs(image[0]), 0.0)
    if segmented:
        unit = unit + split[:, None, None] * accabs
    b_img = np.abs(image[0] - image[1])
    b_T = np.abs(T[0] - T[1])
    for ti, li, w_i, c_i, acc_i, T_i, al_i in near_rec:
        with np.errstate(invalid="ignore", divide="ignore"):
            behind = np.where(T_i[:, None] > 0, (image[0][ti, li] - acc_i) / T_i[:, None], 0.0)
        np.add.at(b_img, (ti, li), np.abs(w_i[:, None] * (c_i - behind)))
        np.add.at(b_T, (ti, li), al_i * T[0][ti, li])

    def to_image(x):  # [tiles, 256, ...] -> [H, W, ...]
        out = np.zeros((H, W) + x.shape[2:], x.dtype)
        out[py[valid], px[valid]] = x[valid]
        return out

    res = dict(image=(to_image(image[0][..., :3]), to_image(unit[..., :3]), to_image(b_img[..., :3])),
               T=(to_image(T[0]), to_image(T[0] * rT), to_image(b_T)),
               n64=to_image(n[0]), n_alt=to_image(n[1]), composited=to_image(ncomp), last_w=to_image(last_w),
               last_alpha=to_image(last_alpha), last_g=to_image(last_g),
               stop_borderline=to_image(flipped))
    if C > 3:
        res["aux"] = (to_image(image[0][..., 3:]), to_image(unit[..., 3:]), to_image(b_img[..., 3:]))
    Tv, Tu, Tb = res["T"]
    res["alpha"] = (1.0 - Tv, Tu + np.where(Tu > 0, 1.0 + Tv, 0.0), Tb)
    return res

"""Numpy float64 reference of the bilateral-grid slice, its backward and the grid's TV loss (gsplat_bilagrid_slice,
gsplat_bilagrid_slice_backward, gsplat_bilagrid_tv_loss; definitions: include/gsplat_hip.h).

A grid is [12,L,Hg,Wg], an image [H,W,3].  For pixel (x, y) with colour r: g = 0.299 r0 + 0.587 r1 + 0.114 r2;
gx = (x + 0.5) / W (Wg - 1), gy = (y + 0.5) / H (Hg - 1), gz = clamp(g, 0, 1) (L - 1); per axis of n vertices
i0 = min(floor(c), max(n - 2, 0)), i1 = min(i0 + 1, n - 1), t = c - i0; A = the 12 trilinearly interpolated values as a
row-major 3x4 matrix; out = A[:, :3] r + A[:, 3].

Every function returns, beside each value, its condition sum: the sum of the absolute values of the terms the value is
made of -- the bar of the tests is a fraction of it, as for tests/feature_loss_reference.py."""
import numpy as np

LUMA = np.array([0.299, 0.587, 0.114])
KNOT = 1e-6


def identity_grid(Wg, Hg, L):
    grid = np.zeros((12, L, Hg, Wg), np.float32)
    grid[[0, 5, 10]] = 1.0
    return grid


def _cells(c, n):
    i0 = np.minimum(np.floor(c).astype(np.int64), max(n - 2, 0))
    return i0, np.minimum(i0 + 1, n - 1), c - i0


def _pixels(grid, image):
    """Per pixel (flattened, P = H W): colour [P,3], guidance [P], and the eight corners as (flat vertex index [P], weight
    [P], z corner 0/1, flat xy weight [P])."""
    grid, r = np.asarray(grid, np.float64), np.asarray(image, np.float64)
    _, L, Hg, Wg = grid.shape
    H, W, _ = r.shape
    g = (0.299 * r[..., 0] + 0.587 * r[..., 1]) + 0.114 * r[..., 2]
    gx = np.broadcast_to(((np.arange(W) + 0.5) / W * (Wg - 1))[None, :], (H, W))
    gy = np.broadcast_to(((np.arange(H) + 0.5) / H * (Hg - 1))[:, None], (H, W))
    gz = np.clip(g, 0.0, 1.0) * (L - 1)
    (x0, x1, tx), (y0, y1, ty), (z0, z1, tz) = _cells(gx, Wg), _cells(gy, Hg), _cells(gz, L)
    corners = []
    for dz, (zi, wz) in enumerate(((z0, 1.0 - tz), (z1, tz))):
        for yi, wy in ((y0, 1.0 - ty), (y1, ty)):
            for xi, wx in ((x0, 1.0 - tx), (x1, tx)):
                corners.append((((zi * Hg + yi) * Wg + xi).reshape(-1), (wx * wy * wz).reshape(-1), dz, (wx * wy).reshape(-1)))
    return grid.reshape(12, -1), r.reshape(-1, 3), g.reshape(-1), corners


def _coefficients(flat, corners):
    """A [P,12] and its condition sum."""
    A = sum(w[:, None] * flat[:, idx].T for idx, w, _, _ in corners)
    A_abs = sum(np.abs(w[:, None] * flat[:, idx].T) for idx, w, _, _ in corners)
    return A, A_abs


def slice_image(grid, image):
    """-> (out [H,W,3], out_abs [H,W,3])."""
    flat, r, _, corners = _pixels(grid, image)
    A, A_abs = _coefficients(flat, corners)
    A, A_abs = A.reshape(-1, 3, 4), A_abs.reshape(-1, 3, 4)
    out = (A[:, :, :3] * r[:, None, :]).sum(-1) + A[:, :, 3]
    out_abs = (A_abs[:, :, :3] * np.abs(r)[:, None, :]).sum(-1) + A_abs[:, :, 3]
    return out.reshape(np.shape(image)), out_abs.reshape(np.shape(image))


def knot_mask(grid_l, image):
    """[H,W] bool: the pixels left out of the grad_image comparison -- the derivative with respect to the guidance jumps
    at a z-knot and at the two clamps."""
    r = np.asarray(image, np.float64)
    g = (0.299 * r[..., 0] + 0.587 * r[..., 1]) + 0.114 * r[..., 2]
    if grid_l <= 1:
        return np.zeros(g.shape, bool)
    z = g * (grid_l - 1)
    at_knot = (g > 0) & (g < 1) & (np.abs(z - np.round(z)) <= KNOT)
    return at_knot | (np.abs(g) <= KNOT) | (np.abs(g - 1.0) <= KNOT)


def slice_backward(grid, image, grad_out):
    """-> (grad_image [H,W,3], grad_image_abs, grad_grid [12,L,Hg,Wg], grad_grid_abs, mask [H,W])."""
    flat, r, g, corners = _pixels(grid, image)
    L = np.shape(grid)[1]
    G = np.asarray(grad_out, np.float64).reshape(-1, 3)
    A, A_abs = _coefficients(flat, corners)
    A, A_abs = A.reshape(-1, 3, 4), A_abs.reshape(-1, 3, 4)
    direct = (A[:, :, :3] * G[:, :, None]).sum(1)
    direct_abs = (A_abs[:, :, :3] * np.abs(G)[:, :, None]).sum(1)
    # through the guidance: the difference of the cell's two z-levels, bilinear in xy
    lo, hi = corners[:4], corners[4:]
    dA = sum(wxy[:, None] * (flat[:, ih].T - flat[:, il].T) for (il, _, _, wxy), (ih, _, _, _) in zip(lo, hi))
    dA_abs = sum(wxy[:, None] * (np.abs(flat[:, ih].T) + np.abs(flat[:, il].T)) for (il, _, _, wxy), (ih, _, _, _) in zip(lo, hi))
    dA, dA_abs = dA.reshape(-1, 3, 4), dA_abs.reshape(-1, 3, 4)
    r1, r1_abs = np.concatenate([r, np.ones((len(r), 1))], 1), np.concatenate([np.abs(r), np.ones((len(r), 1))], 1)
    s = (G[:, :, None] * dA * r1[:, None, :]).sum((1, 2))
    s_abs = (np.abs(G)[:, :, None] * dA_abs * r1_abs[:, None, :]).sum((1, 2))
    active = ((g > 0) & (g < 1) & (L > 1)).astype(np.float64)  # (0 at the two ends themselves, as grid_sample has it)
    grad_image = direct + (active * s * (L - 1))[:, None] * LUMA[None, :]
    grad_image_abs = direct_abs + (active * s_abs * (L - 1))[:, None] * LUMA[None, :]
    # the grid: every corner of every pixel adds w G_row [r,1]_col to channel row x 4 + col
    n = flat.shape[1]
    grad_grid, grad_grid_abs = np.zeros((12, n)), np.zeros((12, n))
    for idx, w, _, _ in corners:
        for row in range(3):
            for col in range(4):
                term = w * G[:, row] * r1[:, col]
                np.add.at(grad_grid[row * 4 + col], idx, term)
                np.add.at(grad_grid_abs[row * 4 + col], idx, np.abs(term))
    shape = np.shape(image)
    return (grad_image.reshape(shape), grad_image_abs.reshape(shape), grad_grid.reshape(np.shape(grid)),
            grad_grid_abs.reshape(np.shape(grid)), knot_mask(L, image))


def tv_loss(grid, weight):
    """-> (loss, grad [12,L,Hg,Wg], grad_abs, loss_abs): weight x the sum over the three axes of (the sum over the
    adjacent pairs along the axis, all 12 channels, of the squared difference / the number of such pairs).  The weight goes
    through float32 first, as the C ABI takes it."""
    v = np.asarray(grid, np.float64)
    w = float(np.float32(weight))
    loss, grad, grad_abs = 0.0, np.zeros(v.shape), np.zeros(v.shape)
    for axis in (1, 2, 3):
        if v.shape[axis] < 2:
            continue
        d = np.diff(v, axis=axis)  # d[i] = v[i + 1] - v[i]
        loss += (d * d).sum() / d.size
        term = 2.0 * w * d / d.size
        hi = [slice(None)] * 4
        lo = [slice(None)] * 4
        hi[axis], lo[axis] = slice(1, None), slice(None, -1)
        grad[tuple(hi)] += term
        grad[tuple(lo)] -= term
        grad_abs[tuple(hi)] += np.abs(term)
        grad_abs[tuple(lo)] += np.abs(term)
    return w * loss, grad, grad_abs, abs(w) * loss

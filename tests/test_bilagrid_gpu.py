"""The bilateral-grid slice, its backward and the TV loss on the GPU against tests/bilagrid_reference.py.

The bar is that of tests/test_normal_gpu.py and tests/test_feature_loss_gpu.py, for the same reason: the kernels evaluate in
double from the float inputs and round once, so every element lies within 1e-6 of its condition sum (one float32 rounding is
6e-8 of the value, the value is at most its condition sum), plus 2^-149, half the spacing of the subnormals.

Grids (Wg, Hg, L) from one colour affine to the limits; images from one pixel (a grid finer than the image: almost every
vertex sees no pixel and must be an exact zero) to 70 x 130 under 16 x 16 x 8, which spans 3 x 5 of the backward's 32 x 32
pixel tiles with partial tiles at both edges."""
import ctypes

import numpy as np
import pytest

import bilagrid_reference as bgr
from conftest import pkg

pytestmark = pytest.mark.gpu

GRIDS = ((1, 1, 1), (2, 2, 2), (3, 5, 4), (16, 16, 8), (64, 64, 16))  # (Wg, Hg, L)
IMAGES = ((1, 1), (1, 67), (35, 67))                                  # (H, W)
CASES = [(g, s) for g in GRIDS for s in IMAGES] + [((16, 16, 8), (70, 130))]
BAR, FLOOR = 1e-6, 2.0 ** -149
TV_WEIGHT = 10.0
INVALID_ARG = -3
_CACHE = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(shape, size):
    """Inputs and the float64 reference of one case, computed once and never written to."""
    key = (shape, size)
    if key not in _CACHE:
        (Wg, Hg, L), (H, W) = shape, size
        rng = np.random.default_rng([0, Wg, Hg, L, H, W])
        grid = (bgr.identity_grid(Wg, Hg, L) + rng.uniform(-0.5, 0.5, (12, L, Hg, Wg))).astype(np.float32)
        image = rng.uniform(-0.2, 1.3, (H, W, 3)).astype(np.float32)  # 8-13 % of the pixels clamp at either end
        grad_out = rng.uniform(-1.0, 1.0, (H, W, 3)).astype(np.float32)
        case = dict(grid=grid, image=image, grad_out=grad_out, out=bgr.slice_image(grid, image),
                    bwd=bgr.slice_backward(grid, image, grad_out), tv=bgr.tv_loss(grid, TV_WEIGHT))
        for a in (grid, image, grad_out):
            a.setflags(write=False)
        _CACHE[key] = case
    return _CACHE[key]


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached arrays are read-only)


def _within(what, got, ref, ref_abs, mask=None):
    """Every element of got within the bar of ref; exact zeros where the condition sum is zero."""
    got = np.asarray(got, np.float64)
    frac = np.abs(got - ref) / (BAR * ref_abs + FLOOR)
    if mask is not None:
        frac = np.where(mask, 0.0, frac)
    print(f"[{what}] worst {float(np.max(frac)):.4f} of the bar")
    assert np.isfinite(got).all()
    assert (frac <= 1.0).all(), f"{what}: an element at {float(np.max(frac)):.3f} of its bar"
    zero = (ref_abs == 0) if mask is None else (ref_abs == 0) & ~mask
    assert (got[zero] == 0).all(), f"{what}: an element with a zero condition sum is not an exact zero"


def _backward(torch, ops, grid, image, grad_out, want_image=True, want_grid=True, base=None):
    """-> (grad_image, grad_grid) as numpy (None where not asked for); base: what grad_grid holds, added to."""
    gi = torch.full(tuple(image.shape), 7.0, device="cuda") if want_image else None  # (nothing of the 7 may survive)
    gg = None
    if want_grid:
        gg = torch.full(tuple(grid.shape), 7.0, device="cuda") if base is None else _dev(torch, base)
    ops.bilagrid_slice_backward(grid, image, grad_out, gi, gg, accumulate_grid=base is not None)
    torch.cuda.synchronize()
    return (None if gi is None else _np(gi)), (None if gg is None else _np(gg))


@pytest.mark.parametrize("shape,size", CASES, ids=lambda v: "x".join(map(str, v)))
def test_slice_and_backward_against_the_reference(gpu, shape, size):
    torch, ops = gpu, pkg("ops")
    c = _case(shape, size)
    what = "grid %dx%dx%d image %dx%d" % (shape + size)
    grid, image, grad_out = (_dev(torch, c[k]) for k in ("grid", "image", "grad_out"))
    out = ops.bilagrid_slice(grid, image, out=torch.full(tuple(image.shape), 7.0, device="cuda"))
    torch.cuda.synchronize()
    _within(what + ": out", _np(out), *c["out"])
    ref_gi, gi_abs, ref_gg, gg_abs, mask = c["bwd"]
    assert mask.mean() <= 1e-3, "more than 0.1 % of the pixels sit on a z-knot"
    gi, gg = _backward(torch, ops, grid, image, grad_out)
    _within(what + ": grad_image", gi, ref_gi, gi_abs, mask=np.broadcast_to(mask[..., None], gi.shape))
    _within(what + ": grad_grid", gg, ref_gg, gg_abs)
    # two runs: the same bits -- grad_grid too (a slab of per-tile sums, reduced in a fixed order; no atomics)
    out2 = ops.bilagrid_slice(grid, image)
    gi2, gg2 = _backward(torch, ops, grid, image, grad_out)
    assert _np(out2).tobytes() == _np(out).tobytes() and gi2.tobytes() == gi.tobytes() and gg2.tobytes() == gg.tobytes()
    # accumulate_grid adds the once-rounded value to a non-zero base
    base = np.random.default_rng(5).uniform(-1e-2, 1e-2, c["grid"].shape).astype(np.float32)
    _, acc = _backward(torch, ops, grid, image, grad_out, want_image=False, base=base)
    assert acc.tobytes() == (base + gg).astype(np.float32).tobytes()
    # either output without the other
    gi3, none = _backward(torch, ops, grid, image, grad_out, want_grid=False)
    none2, gg3 = _backward(torch, ops, grid, image, grad_out, want_image=False)
    assert none is None and none2 is None and gi3.tobytes() == gi.tobytes() and gg3.tobytes() == gg.tobytes()


@pytest.mark.parametrize("shape", GRIDS[1:], ids=lambda v: "x".join(map(str, v)))
def test_guidance_part_is_an_exact_zero_where_the_guidance_clamps(gpu, shape):
    """A grid of offsets only (the 3x3 part is zero): dL/d image is the guidance part alone, so its condition sum is zero
    at every pixel whose guidance lies outside [0, 1] -- and the kernel's value an exact zero."""
    torch, ops = gpu, pkg("ops")
    c = _case(shape, IMAGES[2])
    offsets = np.zeros_like(c["grid"])
    offsets[[3, 7, 11]] = c["grid"][[3, 7, 11]]
    ref_gi, gi_abs, _, _, mask = bgr.slice_backward(offsets, c["image"], c["grad_out"])
    r = c["image"].astype(np.float64)
    g = (0.299 * r[..., 0] + 0.587 * r[..., 1]) + 0.114 * r[..., 2]
    clamped = (g < 0) | (g > 1)
    assert 0.05 < clamped.mean() < 0.3 and (gi_abs[clamped] == 0).all() and (gi_abs[~clamped] > 0).any()
    gi, _ = _backward(torch, ops, _dev(torch, offsets), _dev(torch, c["image"]), _dev(torch, c["grad_out"]), want_grid=False)
    # ... and at the lower end itself (a render's black background: g = 0 exactly), as grid_sample's border padding has it
    black = np.zeros((2, 2, 3), np.float32)
    black[1] = (0.5, 0.25, 0.125)
    go = np.ones((2, 2, 3), np.float32)
    at_end, _ = _backward(torch, ops, _dev(torch, offsets), _dev(torch, black), _dev(torch, go), want_grid=False)
    assert (at_end[0] == 0).all() and (at_end[1] != 0).any()
    _within("offsets only %dx%dx%d: grad_image" % shape, gi, ref_gi, gi_abs, mask=np.broadcast_to(mask[..., None], gi.shape))
    assert (gi[clamped] == 0).all()


@pytest.mark.parametrize("shape", GRIDS, ids=lambda v: "x".join(map(str, v)))
def test_tv_loss_against_the_reference(gpu, shape):
    torch, ops = gpu, pkg("ops")
    c = _case(shape, IMAGES[0])
    ref_loss, ref_grad, grad_abs, loss_abs = c["tv"]
    grid = _dev(torch, c["grid"])
    grad = torch.full(tuple(grid.shape), 7.0, device="cuda")
    loss = ops.bilagrid_tv_loss(grid, TV_WEIGHT, grad, blocking=True)
    what = "tv %dx%dx%d" % shape
    _within(what + ": gradient", _np(grad), ref_grad, grad_abs)
    frac = abs(loss - ref_loss) / (BAR * loss_abs + FLOOR)
    print(f"[{what}] loss {loss:.9g} against {ref_loss:.9g}: {frac:.4f} of the bar")
    assert frac <= 1.0
    if shape == (1, 1, 1):
        assert loss == 0.0 and (_np(grad) == 0).all()
    # two runs: the same bits, the loss included
    grad2 = torch.empty_like(grad)
    loss2 = ops.bilagrid_tv_loss(grid, TV_WEIGHT, grad2, blocking=True)
    assert np.float32(loss).tobytes() == np.float32(loss2).tobytes() and _np(grad2).tobytes() == _np(grad).tobytes()
    # accumulate adds the once-rounded gradient to what was there
    base = np.random.default_rng(6).uniform(-1e-2, 1e-2, c["grid"].shape).astype(np.float32)
    acc = _dev(torch, base)
    assert ops.bilagrid_tv_loss(grid, TV_WEIGHT, acc, accumulate=True) is None
    torch.cuda.synchronize()
    assert _np(acc).tobytes() == (base + _np(grad)).astype(np.float32).tobytes()
    # the loss without the gradient
    assert np.float32(ops.bilagrid_tv_loss(grid, TV_WEIGHT, None, blocking=True)).tobytes() == np.float32(loss).tobytes()


@pytest.mark.parametrize("shape", GRIDS, ids=lambda v: "x".join(map(str, v)))
def test_identity_grid_is_the_identity(gpu, shape):
    torch, ops = gpu, pkg("ops")
    c = _case(shape, IMAGES[2])
    ident = ops.identity_bilagrid(*shape)
    assert _np(ident).tobytes() == bgr.identity_grid(*shape).tobytes()
    image, grad_out = _dev(torch, c["image"]), _dev(torch, c["grad_out"])
    out = ops.bilagrid_slice(ident, image)
    gi, _ = _backward(torch, ops, ident, image, grad_out)
    assert _np(out).tobytes() == c["image"].tobytes()
    assert gi.tobytes() == c["grad_out"].tobytes()


def test_pointers_that_are_not_16_byte_aligned(gpu):
    torch, ops = gpu, pkg("ops")
    shape, size = (16, 16, 8), (35, 67)
    c = _case(shape, size)
    H, W = size

    def shifted(a):
        t = torch.empty(a.size + 1, device="cuda")[1:].view(a.shape)
        t.copy_(torch.from_numpy(np.array(a)))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    grid, image, grad_out = shifted(c["grid"]), shifted(c["image"]), shifted(c["grad_out"])
    out, gi, gg = (shifted(np.full(a.shape, 7.0, np.float32)) for a in (c["image"], c["image"], c["grid"]))
    ops.bilagrid_slice(grid, image, out=out)
    ops.bilagrid_slice_backward(grid, image, grad_out, gi, gg)
    torch.cuda.synchronize()
    ref_gi, gi_abs, ref_gg, gg_abs, mask = c["bwd"]
    _within("unaligned: out", _np(out), *c["out"])
    _within("unaligned: grad_image", _np(gi), ref_gi, gi_abs, mask=np.broadcast_to(mask[..., None], ref_gi.shape))
    _within("unaligned: grad_grid", _np(gg), ref_gg, gg_abs)


def test_every_refusal(gpu):
    torch, ops, lib_mod = gpu, pkg("ops"), pkg("_lib")
    lib = lib_mod.load()
    H, W = 4, 5
    grid = ops.identity_bilagrid(3, 2, 2)
    image, go = torch.zeros(H, W, 3, device="cuda"), torch.zeros(H, W, 3, device="cuda")
    gi, out = torch.full((H, W, 3), 3.0, device="cuda"), torch.full((H, W, 3), 3.0, device="cuda")
    gg, loss = torch.full(tuple(grid.shape), 3.0, device="cuda"), torch.full((1,), 5.0, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    fwd = lambda g, w, h, l, im, r, c, o: lib.gsplat_bilagrid_slice(P(g), w, h, l, P(im), r, c, P(o), None)
    bwd = lambda g, w, h, l, im, gr, r, c, a, b: lib.gsplat_bilagrid_slice_backward(P(g), w, h, l, P(im), P(gr), r, c, 0,
                                                                                    P(a), P(b), None)
    tv = lambda g, w, h, l, a, b: lib.gsplat_bilagrid_tv_loss(P(g), w, h, l, 1.0, 0, P(a), P(b), None)
    bad = []
    for w, h, l in ((0, 2, 2), (3, 0, 2), (3, 2, 0), (65, 2, 2), (3, 65, 2), (3, 2, 17)):
        bad += [fwd(grid, w, h, l, image, H, W, out), bwd(grid, w, h, l, image, go, H, W, gi, gg), tv(grid, w, h, l, gg, loss)]
    for r, c in ((0, W), (H, 0), (-1, W)):
        bad += [fwd(grid, 3, 2, 2, image, r, c, out), bwd(grid, 3, 2, 2, image, go, r, c, gi, gg)]
    bad += [fwd(None, 3, 2, 2, image, H, W, out), fwd(grid, 3, 2, 2, None, H, W, out), fwd(grid, 3, 2, 2, image, H, W, None),
            bwd(None, 3, 2, 2, image, go, H, W, gi, gg), bwd(grid, 3, 2, 2, None, go, H, W, gi, gg),
            bwd(grid, 3, 2, 2, image, None, H, W, gi, gg), bwd(grid, 3, 2, 2, image, go, H, W, None, None),
            bwd(grid, 3, 2, 2, image, go, H, W, go, gg), bwd(grid, 3, 2, 2, image, go, H, W, image, gg),
            tv(None, 3, 2, 2, gg, loss), tv(grid, 3, 2, 2, None, None)]
    torch.cuda.synchronize()
    assert bad == [INVALID_ARG] * len(bad)
    for t in (gi, out, gg):
        assert bool((t == 3.0).all())
    assert float(loss) == 5.0  # nothing was launched
    host = np.zeros(64, np.float32)
    assert lib.gsplat_bilagrid_slice(ctypes.c_void_p(host.ctypes.data), 1, 1, 1, P(image), H, W, P(out), None) == -2  # not device
    # the binding's own checks
    for call in (lambda: ops.bilagrid_slice(grid[:11], image), lambda: ops.bilagrid_slice(grid.double(), image),
                 lambda: ops.bilagrid_slice(grid, image[..., :2]), lambda: ops.bilagrid_slice(grid, image, out=out[:2]),
                 lambda: ops.bilagrid_slice(grid.cpu(), image), lambda: ops.bilagrid_slice(None, image),
                 lambda: ops.bilagrid_slice_backward(grid, image, None, gi, gg),
                 lambda: ops.bilagrid_slice_backward(grid, image, go, gi[:2], gg),
                 lambda: ops.bilagrid_slice_backward(grid, image, go, gi, gg[:, :1]),
                 lambda: ops.bilagrid_tv_loss(grid, 1.0, gg[:, :1]), lambda: ops.bilagrid_tv_loss(None, 1.0, gg)):
        with pytest.raises((ValueError, TypeError)):
            call()
    for call in (lambda: ops.bilagrid_slice_backward(grid, image, go, None, None), lambda: ops.bilagrid_tv_loss(grid, 1.0, None),
                 lambda: ops.bilagrid_slice_backward(grid, image, go, go, gg)):
        with pytest.raises(lib_mod.GsplatError):
            call()

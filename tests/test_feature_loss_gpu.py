"""The three feature losses and the feature column's Adam step on the GPU against tests/feature_loss_reference.py.

The bar is tests/test_normal_gpu.py's, for the same reason: the kernels evaluate every pixel in double from the float maps
and round once, so a gradient element (and the loss) lies within 1e-6 of its condition sum -- one float32 rounding is
6e-8 of the value, and the value is at most its condition sum.  A float32 result cannot be closer to anything than half the
spacing of the subnormals, so the bar of an element is 1e-6 x its condition sum + 2^-149: that term is what a softmax
probability of e^-160 (logits of +-80) is held to, which no float32 can represent.

Channel counts: every lanes-per-pixel choice of the kernels (1, 4, 16, 64 lanes), the counts either side of each boundary
(4 | 5, 16 | 17, 64 | 65), rows of whole 16-byte pieces and not, the register-resident limit (256 | 257) and the channel
limit (512)."""
import ctypes

import numpy as np
import pytest

import feature_loss_reference as flr
from conftest import pkg

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 4, 5, 16, 17, 35, 64, 65)
LARGE_CHANNELS = (256, 257, 512)  # at the largest map only
SIZES = ((1, 1), (1, 67), (35, 67))
BAR, FLOOR = 1e-6, 2.0 ** -149
WEIGHT = 0.75
INVALID_ARG = -3
_WORST = {}


def _np(t):
    return t.detach().cpu().numpy()


def _sizes(C):
    return SIZES[-1:] if C in LARGE_CHANNELS else SIZES


def _inputs(kind, H, W, C, seed=0, span=3.0):
    rng = np.random.default_rng([seed, H, W, C])
    fmap = rng.uniform(-span, span, (H, W, C)).astype(np.float32)
    if kind == "ce":
        labels = rng.integers(0, C, (H, W)).astype(np.int32)
        labels[rng.random((H, W)) < 1 / 3] = -1       # a third ignored
        labels.reshape(-1)[(H * W) // 2] = C          # one out of range
        if H * W > 2:
            labels.reshape(-1)[1] = C - 1             # (and the last channel labelled somewhere)
        return fmap, labels, None
    target = rng.uniform(-span, span, (H, W, C)).astype(np.float32)
    valid = (rng.random((H, W)) > 0.3).astype(np.uint8) if H * W > 1 else None
    return fmap, target, valid


def _run(torch, kind, fmap, second, valid, grad=None, accumulate=False, weight=WEIGHT):
    """-> (loss, grad_map as numpy): the ops call on device copies; grad: the tensor to write or add to."""
    ops = pkg("ops")
    f = fmap if isinstance(fmap, torch.Tensor) else torch.from_numpy(fmap).cuda()
    s = torch.from_numpy(second).cuda()
    if grad is None:
        grad = torch.full(tuple(f.shape), 7.0, device="cuda")  # (overwritten: nothing of the 7 may survive)
    if kind == "ce":
        loss = ops.feature_ce_loss(f, s, weight, grad, accumulate=accumulate, blocking=True)
    else:
        v = None if valid is None else torch.from_numpy(valid).cuda()
        fn = ops.feature_l1_loss if kind == "l1" else ops.feature_cosine_loss
        loss = fn(f, s, weight, grad, valid=v, accumulate=accumulate, blocking=True)
    torch.cuda.synchronize()
    return loss, _np(grad)


def _reference(kind, fmap, second, valid, weight=WEIGHT):
    return flr.ce_loss(fmap, second, weight) if kind == "ce" else flr.LOSSES[kind](fmap, second, valid, weight)


def _check(kind, what, loss, grad, ref):
    ref_loss, ref_grad, grad_abs, loss_abs = ref
    frac = np.abs(grad.astype(np.float64) - ref_grad) / (BAR * grad_abs + FLOOR)
    loss_frac = abs(loss - ref_loss) / (BAR * loss_abs + FLOOR)
    worst = max(float(frac.max()), float(loss_frac))
    _WORST[kind] = max(_WORST.get(kind, 0.0), worst)
    print(f"[{kind} {what}] gradient: worst {float(frac.max()):.3f} of the bar; loss {loss:.9g} against {ref_loss:.9g}: "
          f"{loss_frac:.3f} of the bar (largest of this loss so far: {_WORST[kind]:.3f})")
    assert np.isfinite(grad).all() and np.isfinite(loss)
    assert (frac <= 1.0).all(), f"{kind} {what}: a gradient element at {float(frac.max()):.3f} of its bar"
    assert loss_frac <= 1.0, f"{kind} {what}: loss {loss!r} against {ref_loss!r}"
    assert (grad[grad_abs == 0] == 0).all(), f"{kind} {what}: an element that takes no part is not an exact zero"


@pytest.mark.parametrize("C", CHANNELS + LARGE_CHANNELS)
@pytest.mark.parametrize("kind", ["ce", "l1", "cosine"])
def test_loss_and_gradient_against_the_reference(gpu, kind, C):
    torch = gpu
    for H, W in _sizes(C):
        fmap, second, valid = _inputs(kind, H, W, C)
        ref = _reference(kind, fmap, second, valid)
        loss, grad = _run(torch, kind, fmap, second, valid)
        _check(kind, f"{H}x{W}x{C}", loss, grad, ref)
        # two runs: the same bits, the loss included
        loss2, grad2 = _run(torch, kind, fmap, second, valid)
        assert np.float32(loss).tobytes() == np.float32(loss2).tobytes() and grad.tobytes() == grad2.tobytes()
        # accumulate adds the once-rounded gradient to what was there
        base = np.random.default_rng(C).uniform(-1e-3, 1e-3, fmap.shape).astype(np.float32)
        _, acc = _run(torch, kind, fmap, second, valid, grad=torch.from_numpy(base.copy()).cuda(), accumulate=True)
        assert acc.tobytes() == (base + grad).astype(np.float32).tobytes()
    if kind != "ce":  # no validity map: every pixel takes part
        H, W = _sizes(C)[-1]
        fmap, second, _ = _inputs(kind, H, W, C, seed=1)
        _check(kind, f"{H}x{W}x{C} without a validity map", *_run(torch, kind, fmap, second, None), _reference(kind, fmap, second, None))


@pytest.mark.parametrize("C", (5, 16, 64, 257))
def test_ce_at_logits_of_80_and_at_equal_channels(gpu, C):
    torch = gpu
    H, W = 35, 67
    fmap, labels, _ = _inputs("ce", H, W, C, seed=2, span=80.0)
    fmap.reshape(-1, C)[0] = -80.0
    fmap.reshape(-1, C)[0, C - 1] = 80.0  # the widest row there is
    labels.reshape(-1)[0] = 0
    loss, grad = _run(torch, "ce", fmap, labels, None)
    _check("ce", f"{H}x{W}x{C}, logits in +-80", loss, grad, _reference("ce", fmap, labels, None))
    flat = np.full((H, W, C), 1.25, np.float32)
    loss, grad = _run(torch, "ce", flat, labels, None)
    _check("ce", f"{H}x{W}x{C}, all channels equal", loss, grad, _reference("ce", flat, labels, None))
    part = (labels >= 0) & (labels < C)
    assert abs(loss - WEIGHT * np.log(C) * part.mean()) <= 1e-6 * max(loss, 1e-30)  # a uniform softmax: ln C per pixel


@pytest.mark.parametrize("C", (3, 16, 65))
def test_ce_with_every_label_ignored(gpu, C):
    torch = gpu
    H, W = 35, 67
    fmap, labels, _ = _inputs("ce", H, W, C, seed=3)
    labels[:] = -1
    labels[3, 4] = C
    loss, grad = _run(torch, "ce", fmap, labels, None)
    assert loss == 0.0 and (grad == 0).all()
    base = torch.full((H, W, C), 0.5, device="cuda")
    _, acc = _run(torch, "ce", fmap, labels, None, grad=base, accumulate=True)
    assert (acc == 0.5).all()


@pytest.mark.parametrize("C", (3, 16, 35, 256))
def test_target_losses_at_zero_rows_and_equal_channels(gpu, C):
    torch = gpu
    H, W = 35, 67
    for kind in ("l1", "cosine"):
        fmap, target, valid = _inputs(kind, H, W, C, seed=4)
        valid[0, :3] = 1
        fmap[0, 0], target[0, 1] = 0.0, 0.0         # a zero map row, a zero target row
        fmap[0, 2] = target[0, 2]                   # a row that meets its target: sign(0) = 0, cosine 1
        fmap[1], target[2] = 0.5, -2.0              # all channels equal
        loss, grad = _run(torch, kind, fmap, target, valid)
        _check(kind, f"{H}x{W}x{C}, zero and constant rows", loss, grad, _reference(kind, fmap, target, valid))
        if kind == "cosine":
            assert (grad[0, 0] == 0).all() and (grad[0, 1] == 0).all()
        else:
            assert (grad[0, 2] == 0).all()


def test_rows_that_are_not_16_byte_aligned(gpu):
    """C % 4 == 0 on a map that starts one float into its allocation takes the 4-byte path."""
    torch = gpu
    H, W, C = 35, 67, 16
    for kind in ("ce", "cosine"):
        fmap, second, valid = _inputs(kind, H, W, C, seed=5)
        shifted = torch.empty(H * W * C + 1, device="cuda")[1:].view(H, W, C)
        shifted.copy_(torch.from_numpy(fmap))
        assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        loss2, grad2 = _run(torch, kind, shifted, second, valid)
        _check(kind, f"{H}x{W}x{C}, unaligned", loss2, grad2, _reference(kind, fmap, second, valid))


def test_loss_without_gradient_and_gradient_without_loss(gpu):
    torch, ops = gpu, pkg("ops")
    H, W, C = 35, 67, 17
    fmap, labels, _ = _inputs("ce", H, W, C, seed=6)
    loss, grad = _run(torch, "ce", fmap, labels, None)
    f, lab = torch.from_numpy(fmap).cuda(), torch.from_numpy(labels).cuda()
    assert np.float32(ops.feature_ce_loss(f, lab, WEIGHT, None, blocking=True)).tobytes() == np.float32(loss).tobytes()
    g = torch.empty(H, W, C, device="cuda")
    assert ops.feature_ce_loss(f, lab, WEIGHT, g) is None
    torch.cuda.synchronize()
    assert _np(g).tobytes() == grad.tobytes()


def test_every_refusal(gpu):
    torch, ops, lib_mod = gpu, pkg("ops"), pkg("_lib")
    lib = lib_mod.load()
    H, W, C = 4, 5, 6
    f, g = torch.zeros(H, W, C, device="cuda"), torch.full((H, W, C), 3.0, device="cuda")
    lab, valid = torch.zeros(H, W, dtype=torch.int32, device="cuda"), torch.ones(H, W, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), 5.0, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ce = lambda m, l, r, c, ch, gm, lo: lib.gsplat_feature_ce_loss(P(m), P(l), r, c, ch, 1.0, 0, P(gm), P(lo), None)
    bad = [ce(None, lab, H, W, C, g, out), ce(f, None, H, W, C, g, out), ce(f, lab, H, W, C, None, None),
           ce(f, lab, 0, W, C, g, out), ce(f, lab, H, -1, C, g, out), ce(f, lab, H, W, 0, g, out), ce(f, lab, H, W, 513, g, out)]
    for fn in (lib.gsplat_feature_l1_loss, lib.gsplat_feature_cosine_loss):
        tl = lambda m, t, r, c, ch, gm, lo: fn(P(m), P(t), P(valid), r, c, ch, 1.0, 0, P(gm), P(lo), None)
        bad += [tl(None, f, H, W, C, g, out), tl(f, None, H, W, C, g, out), tl(f, f, H, W, C, None, None),
                tl(f, f, 0, W, C, g, out), tl(f, f, H, 0, C, g, out), tl(f, f, H, W, 0, g, out), tl(f, f, H, W, 513, g, out)]
    torch.cuda.synchronize()
    assert bad == [INVALID_ARG] * len(bad)
    assert bool((g == 3.0).all()) and float(out) == 5.0  # nothing was launched
    host = np.zeros(4, np.float32)
    assert lib.gsplat_feature_ce_loss(ctypes.c_void_p(host.ctypes.data), P(lab), 1, 1, 1, 1.0, 0, P(g), None, None) == -2  # not device
    # the binding's own checks
    for call in (lambda: ops.feature_ce_loss(f, lab.long(), 1.0, g), lambda: ops.feature_ce_loss(f, lab[:2], 1.0, g),
                 lambda: ops.feature_ce_loss(f, None, 1.0, g), lambda: ops.feature_ce_loss(f.double(), lab, 1.0, g),
                 lambda: ops.feature_ce_loss(f, lab, 1.0, g[..., :3]), lambda: ops.feature_l1_loss(f, f[:2], 1.0, g),
                 lambda: ops.feature_l1_loss(f, None, 1.0, g), lambda: ops.feature_cosine_loss(f, f, 1.0, g, valid=valid.int()),
                 lambda: ops.feature_cosine_loss(f.cpu(), f, 1.0, g)):
        with pytest.raises((ValueError, TypeError)):
            call()
    with pytest.raises(lib_mod.GsplatError):
        ops.feature_ce_loss(f, lab, 1.0, None)  # nothing asked for


# ---------------------------------------------------------------- the feature column's Adam step
ADAM = dict(lr=0.0025, b1=0.9, b2=0.999, eps=1e-8)


def _adam_case(torch, N, C, seed):
    rng = np.random.default_rng([seed, N, C])
    visible = np.sort(rng.permutation(N)[: max(1, N // 2)]).astype(np.int32)
    state = dict(p=rng.standard_normal((N, C)), m=rng.standard_normal((N, C)) * 1e-4, v=rng.random((N, C)) * 1e-8,
                 g=rng.standard_normal((N, C)) * 1e-3)
    state["g"][visible[0], 0] = np.nan  # (counts as 0, as in the optimizer's kernel)
    return visible, {k: a.astype(np.float32) for k, a in state.items()}


@pytest.mark.parametrize("C", (1, 3, 16, 17))
@pytest.mark.parametrize("N", (1, 63, 64, 65, 1000))
def test_adam_step_is_the_optimizer_steps_bit_for_bit(gpu, N, C):
    torch, ops, lib_mod = gpu, pkg("ops"), pkg("_lib")
    lib = lib_mod.load()
    visible, s = _adam_case(torch, N, C, 7)
    M, it = len(visible), 11
    b1c, b2c = 1.0 - ADAM["b1"] ** (it + 1), 1.0 - ADAM["b2"] ** (it + 1)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    c2g = dev(visible)
    # gsplat_optimizer_step: one group of stride C, the same gradient gathered into compacted order
    p0, m0, v0 = dev(s["p"]), dev(s["m"]), dev(s["v"])
    compacted = dev(s["g"][visible])
    arr = (lib_mod.AdamGroup * 1)()
    arr[0].param, arr[0].exp_avg, arr[0].exp_avg_sq, arr[0].grad = p0.data_ptr(), m0.data_ptr(), v0.data_ptr(), compacted.data_ptr()
    arr[0].stride, arr[0].packed_column, arr[0].lr = C, 0, ADAM["lr"]
    lib_mod.check(lib.gsplat_optimizer_step(ctypes.c_void_p(c2g.data_ptr()), M, arr, 1, ADAM["b1"], ADAM["b2"], ADAM["eps"],
                                            b1c, b2c, None, None, None, None))
    p1, m1, v1, g1 = dev(s["p"]), dev(s["m"]), dev(s["v"]), dev(s["g"])
    ops.feature_adam_step(c2g, M, p1, m1, v1, g1, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], b1c, b2c)
    torch.cuda.synchronize()
    for name, a, b in (("features", p1, p0), ("exp_avg", m1, m0), ("exp_avg_sq", v1, v0)):
        assert _np(a).tobytes() == _np(b).tobytes(), name
    hidden = np.ones(N, bool)
    hidden[visible] = False
    for name, a in (("features", p1), ("exp_avg", m1), ("exp_avg_sq", v1), ("gradient", g1)):
        start = s[{"features": "p", "exp_avg": "m", "exp_avg_sq": "v", "gradient": "g"}[name]]
        assert _np(a)[hidden].tobytes() == start[hidden].tobytes(), name + ": a row the view did not see changed"
    assert (_np(g1)[visible] == 0).all() and not np.signbit(_np(g1)[visible]).any()
    if N > 1:
        assert (_np(p1)[visible] != s["p"][visible]).any() and hidden.any()
    # and the step is Adam: the float32 reference, at the tolerance of tests/test_optimizer_gpu.py's single step
    rp, rm, rv = flr.adam_step(s["p"][visible], s["g"][visible], s["m"][visible], s["v"][visible], ADAM["lr"], ADAM["b1"],
                               ADAM["b2"], ADAM["eps"], b1c, b2c)
    np.testing.assert_allclose(_np(m1)[visible], rm, rtol=2e-6, atol=1e-12)
    np.testing.assert_allclose(_np(v1)[visible], rv, rtol=2e-6, atol=1e-20)
    np.testing.assert_allclose(_np(p1)[visible], rp, rtol=2e-6, atol=1e-7)
    # num_culled = 0: nothing happens
    before = [_np(t).copy() for t in (p1, m1, v1, g1)]
    ops.feature_adam_step(None, 0, p1, m1, v1, g1, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], b1c, b2c)
    torch.cuda.synchronize()
    assert all(_np(t).tobytes() == b.tobytes() for t, b in zip((p1, m1, v1, g1), before))


def test_adam_step_refusals(gpu):
    torch, ops = gpu, pkg("ops")
    z = lambda *s: torch.zeros(*s, device="cuda")
    c2g = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = (0.0025, 0.9, 0.999, 1e-8, 0.1, 0.001)
    for call in (lambda: ops.feature_adam_step(c2g, 2, z(4, 3), z(4, 3), z(4, 2), z(4, 3), *args),
                 lambda: ops.feature_adam_step(c2g, 2, z(4, 3), z(4, 3), z(4, 3), z(3, 3), *args),
                 lambda: ops.feature_adam_step(c2g, 5, z(4, 3), z(4, 3), z(4, 3), z(4, 3), *args),
                 lambda: ops.feature_adam_step(c2g.long(), 2, z(4, 3), z(4, 3), z(4, 3), z(4, 3), *args),
                 lambda: ops.feature_adam_step(c2g, 2, z(4, 513), z(4, 513), z(4, 513), z(4, 513), *args),
                 lambda: ops.feature_adam_step(c2g, 2, z(4, 3).double(), z(4, 3), z(4, 3), z(4, 3), *args)):
        with pytest.raises((ValueError, TypeError)):
            call()

"""Numpy float64 reference of the three losses on a feature map (gsplat_feature_ce_loss, gsplat_feature_l1_loss,
gsplat_feature_cosine_loss; definitions: include/gsplat_hip.h) and of the feature column's Adam step
(gsplat_feature_adam_step).

A map is [H,W,C], P = H x W.  The weight goes through float32 first, as the C ABI takes it; the maps are taken as they are
given.  Every loss returns (loss, grad [H,W,C], grad_abs [H,W,C], loss_abs): the gradient of every element and, per element
and for the loss, the sum of the absolute values of the terms it is made of (its condition sum) -- the bar of the tests is a
fraction of it, as for tests/normal_reference.py."""
import numpy as np


def _f32(v):
    return float(np.float32(v))


def ce_loss(fmap, labels, weight):
    """Softmax cross-entropy with the channels as logits; a pixel takes part when 0 <= label < C.
    loss = weight / P x sum (logsumexp - x_label): its terms are the logsumexp and the label's logit of every pixel;
    grad = weight / P x (softmax - onehot): its terms are the softmax and the one."""
    x, lab = np.asarray(fmap, np.float64), np.asarray(labels)
    H, W, C = x.shape
    scale = _f32(weight) / (H * W)
    part = (lab >= 0) & (lab < C)
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    z = e.sum(-1, keepdims=True)
    lse = (np.log(z) + m)[..., 0]
    onehot = (np.arange(C)[None, None, :] == np.where(part, lab, -1)[..., None]).astype(np.float64)
    x_lab = (x * onehot).sum(-1)
    loss = scale * np.where(part, lse - x_lab, 0.0).sum()
    loss_abs = scale * np.where(part, np.abs(lse) + np.abs(x_lab), 0.0).sum()
    grad = np.where(part[..., None], scale * (e / z - onehot), 0.0)
    grad_abs = np.where(part[..., None], scale * (e / z + onehot), 0.0)
    return loss, grad, grad_abs, loss_abs


def _valid(valid, shape):
    return np.ones(shape, bool) if valid is None else np.asarray(valid) != 0


def l1_loss(fmap, target, valid, weight):
    """weight / (P C) x sum |map - target| over the valid pixels; the gradient is its sign (sign(0) = 0)."""
    x, t = np.asarray(fmap, np.float64), np.asarray(target, np.float64)
    H, W, C = x.shape
    scale = _f32(weight) / (H * W * C)
    d = np.where(_valid(valid, (H, W))[..., None], x - t, 0.0)
    loss = scale * np.abs(d).sum()
    grad = scale * np.sign(d)
    return loss, grad, np.abs(grad), loss


def cosine_loss(fmap, target, valid, weight):
    """weight / P x sum (1 - f.t / (|f||t|)) over the valid pixels with |f| > 0 and |t| > 0;
    grad = -weight / P x (t - (f.t / |f|^2) f) / (|f||t|), its condition sum carried through the dot product."""
    f, t = np.asarray(fmap, np.float64), np.asarray(target, np.float64)
    H, W, C = f.shape
    scale = _f32(weight) / (H * W)
    dot, dot_abs = (f * t).sum(-1), np.abs(f * t).sum(-1)
    ff, tt = (f * f).sum(-1), (t * t).sum(-1)
    part = _valid(valid, (H, W)) & (ff > 0) & (tt > 0) & np.isfinite(ff) & np.isfinite(tt)
    with np.errstate(all="ignore"):
        inv = np.where(part, 1.0 / (np.sqrt(ff) * np.sqrt(tt)), 0.0)
        along, along_abs = np.where(part, dot / ff, 0.0), np.where(part, dot_abs / ff, 0.0)
    loss = scale * np.where(part, 1.0 - dot * inv, 0.0).sum()
    loss_abs = scale * np.where(part, 1.0 + dot_abs * inv, 0.0).sum()
    grad = -scale * inv[..., None] * (t - along[..., None] * f)
    grad_abs = scale * inv[..., None] * (np.abs(t) + along_abs[..., None] * np.abs(f))
    return loss, grad, grad_abs, loss_abs


LOSSES = {"ce": ce_loss, "l1": l1_loss, "cosine": cosine_loss}


def adam_step(p, g, m, v, lr, b1, b2, eps, bias1, bias2, dtype=np.float32):
    """One Adam step in the order of operations of the library's element update (gs::adam_values): NaN gradients count
    as 0, bias-corrected moments.  dtype float32 rounds as the kernel does; float64 is the exact value.  -> (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    lr, b1, b2, eps, bias1, bias2 = (dtype(np.float32(a)) for a in (lr, b1, b2, eps, bias1, bias2))
    g = np.where(np.isnan(g), dtype(0), g)
    one = dtype(1)
    mi = b1 * m + (one - b1) * g
    vi = b2 * v + (one - b2) * g * g
    m_hat, v_hat = mi / bias1, vi / bias2
    return (p + (-lr * m_hat / (np.sqrt(v_hat) + eps))).astype(dtype), mi.astype(dtype), vi.astype(dtype)

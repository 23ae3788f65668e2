"""GPU parity of gsplat_fused_loss, gsplat_compute_psnr, gsplat_adam_step and the masked optimizer kernels on the inputs
a training loop produces (tests/loss_cases.py), against the float64 oracle on the same float32 inputs.

The bar (loss_cases.bars): err_kernel <= K * err_oracle32 + floor, where err_oracle32 is the float32 oracle's error
against float64 ON THE SAME INPUT, computed at run time -- a kernel may be as inaccurate as float32 makes the reference's
own formula on that input, times K, and no more.  No bar is looser than 1e-3 of the largest gradient entry.

Measured on the MI355X (kernel error / float32 error on the same input, the floor taken off; every test prints its
figures, run with -s):
  families, largest gradient error   noise 0.18, flat grey 1.44, ramps 1.03 .. 1.96, blob 1.04, near-white 1.02, half
                                     identical 0.19, black 0, background band 1.61, unclamped 0, dark 0.43, seam edge 1.82
  families, relative L2              all 0 .. 1.56, but background band 96x160 at lambda 0.2: 4.24 (the worst of all)
  families, loss value               near-white 1.05 .. 1.18, seam edge 0.95 .. 2.20, the others below 0.75
  geometry sweep (437 shapes)        noise 3.63 / 0.90 / 0.51 (emax / L2 / loss), seam edge 2.69 / 2.46 / 3.35
  tile counts (11 shapes)            noise under the floor, seam edge 1.75 / 1.53 / 1.70
K = 8 is twice the worst (4.24); FLOOR_ULPS = 4.  For the loss value the float32 error is the larger of two float32
evaluations (loss_cases.oracle_pair says why): against the float32 oracle alone the seam-edge images measured 21 to 3559,
because that oracle's per-region errors happen to cancel to 1e-9 .. 1e-6 where a plain numpy float32 evaluation is 2.70e-5
off and the kernel 2.79e-5 (96x160, lambda 1).
PSNR: the kernel's error equals the float32 oracle's to the printed digits but at 1080p with an offset of 1e-3 (2.9e-6 dB
against 9.4e-7 dB); the largest error seen is 5.65e-6 dB (2160x3840, offset 1e-6, 119.885 dB), all inside the floor of four
ulps of the value, so K_PSNR = 4 is not strained.  Adam: every non-NaN entry of p, m and v has the float32 oracle's bits at
every size and setting, so ADAM_EQUAL_BITS asserts bit equality.  The file runs in 8 s.
"""
import numpy as np
import pytest

import loss_cases
from conftest import pkg
from loss_cases import EPS32

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 0.2, 1.0)
SIZES = [(96, 160), (13, 27)]  # 5 x 6 = 30 tiles with no partial tile; one partial tile smaller than its halo in y
FULL_HD = (1080, 1920)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _loss(ops, pred, gt, lam, blocking=True):
    """(loss or None, gradient tensor pre-filled with NaN so that an unwritten pixel shows)."""
    import torch
    H, W = pred.shape[:2]
    g = torch.full((H, W, 3), float("nan"), device="cuda")
    return ops.fused_loss(_dev(pred), _dev(gt), H, W, float(lam), g, blocking=blocking), g


_REF = {}


def _ref(orc, name, H, W, lam, threads=1):
    """Inputs, float64 oracle and float32 yardstick of one case; the full-size ones are computed once per session."""
    key = (name, H, W, lam)
    if key not in _REF:
        pred, gt = loss_cases.family(name, H, W)
        if len(_REF) > 64:
            _REF.pop(next(k for k in _REF if k[1:3] != FULL_HD))
        loss64, grad64, fig32 = loss_cases.oracle_pair(orc, pred, gt, lam, threads=16 if (H, W) == FULL_HD else threads)
        _REF[key] = (pred, gt, loss64, grad64, loss_cases.pooled_yardstick(orc, name, H, W, lam, fig32))
    return _REF[key]


def _judge(what, loss, grad, loss64, grad64, fig32, worst=None):
    """Figures of one kernel evaluation against the bar; returns the list of misses (empty = within the bar)."""
    g = grad.cpu().numpy() if hasattr(grad, "cpu") else grad
    fig = loss_cases.error_figures(loss64 if loss is None else loss, g, loss64, grad64)
    bar = loss_cases.bars(fig32, loss64)
    r = loss_cases.ratios(fig, fig32, loss64)
    if worst is not None:
        for k in r:
            if r[k] > worst.get(k, (0.0, ""))[0]:
                worst[k] = (r[k], what)
    else:
        print(f"  RATIO {what:44s} emax {fig['emax']:.3e} / {fig32['emax']:.3e} -> {r['emax']:6.2f}   "
              f"l2 {fig['l2']:.3e} / {fig32['l2']:.3e} -> {r['l2']:6.2f}   "
              f"loss {fig['loss']:.3e} / {fig32['loss']:.3e} -> {r['loss']:6.2f}")
    miss = []
    finite64 = np.isfinite(grad64)
    if not np.isfinite(g[finite64]).all():
        miss.append(f"{what}: non-finite gradient where the oracle's is finite")
    for k in ("emax", "l2") + (("loss",) if loss is not None else ()):
        if not fig[k] <= bar[k]:
            miss.append(f"{what}: {k} {fig[k]:.4e} > bar {bar[k]:.4e} (float32 oracle {fig32[k]:.4e})")
    return miss


# ------------------------------------------------------------------------------------------------ 3. the families
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("shape", SIZES)
@pytest.mark.parametrize("name", loss_cases.FAMILY_NAMES)
def test_family_matches_f64_oracle(gpu, orc, name, shape, lam):
    ops = pkg("ops")
    H, W = shape
    pred, gt, loss64, grad64, fig32 = _ref(orc, name, H, W, lam)
    loss, grad = _loss(ops, pred, gt, lam)
    assert _judge(f"{name} {H}x{W} lambda {lam}", loss, grad, loss64, grad64, fig32) == []
    if lam == 0.0:
        # only the L1 term is left: the gradient is +-(1 - lambda) / (3 H W) bit for bit (-1 where pred == gt) ...
        want = np.where(pred > gt, np.float32(1), np.float32(-1)) * (np.float32(1) / np.float32(H * W * 3))
        assert np.array_equal(grad.cpu().numpy(), want)
        # ... and the loss is the mean of |pred - gt| within float32 rounding of the sum: fabsf(x - y) rounds once, the
        # non-negative terms pass through 5 additions in a thread, 6 in the wave's butterfly and ceil(4 n / 256) - 1 on a
        # spread counter (each at most half an ulp of a partial sum no larger than the total), the quotient rounds once.
        n_tiles = -(-H // loss_cases.TILE_H) * -(-W // loss_cases.TILE_W)
        depth = 5 + 6 + max(-(-4 * n_tiles // 256) - 1, 0) + 2
        mean64 = float(np.abs(pred.astype(np.float64) - gt.astype(np.float64)).mean())
        assert abs(loss - mean64) <= depth * 0.5 * EPS32 * mean64, (loss, mean64)


# ------------------------------------------------------------------------------------------------ 4. geometry sweep
SWEEP_H = (1, 2, 5, 6, 10, 11, 15, 16, 17, 21, 22, 26, 27, 31, 32, 33, 47, 48, 49)
SWEEP_W = (1, 2, 3, 4, 5, 6, 10, 11, 27, 28, 31, 32, 33, 37, 38, 42, 43, 63, 64, 65, 95, 96, 97)
# shapes chosen for their tile count n = ntx * nty: per = ceil(n / 8) of tile_of(), its early-return workgroups (n not a
# multiple of 8) and the counter clear of tile 0; half of them end in partial tiles
TILE_COUNT_SHAPES = {1: (13, 30), 2: (16, 64), 7: (9, 200), 8: (32, 128), 9: (40, 96), 15: (48, 150), 16: (64, 128),
                     17: (16, 544), 63: (105, 288), 64: (128, 256), 65: (80, 400)}


def _sweep(ops, orc, name, shapes, lam=0.2):
    import torch
    miss, worst = [], {}
    for (H, W) in shapes:
        pred, gt = loss_cases.family(name, H, W)
        loss64, grad64, fig32 = loss_cases.oracle_pair(orc, pred, gt, lam)
        fig32 = loss_cases.pooled_yardstick(orc, name, H, W, lam, fig32)  # (images of a few pixels: see there)
        loss, grad = _loss(ops, pred, gt, lam)
        miss += _judge(f"{name} {H}x{W}", loss, grad, loss64, grad64, fig32, worst)
        none, grad_nb = _loss(ops, pred, gt, lam, blocking=False)
        torch.cuda.synchronize()
        if none is not None or not torch.equal(grad_nb, grad):
            miss.append(f"{name} {H}x{W}: the non-blocking call leaves other bits than the blocking call")
    print(f"  SWEEP {name}: {len(shapes)} shapes, worst ratios " +
          ", ".join(f"{k} {v[0]:.2f} ({v[1]})" for k, v in worst.items()))
    return miss


@pytest.mark.parametrize("name", ["noise", "seam_edge"])
def test_geometry_sweep(gpu, orc, name):
    """Every (H, W) of SWEEP_H x SWEEP_W: images smaller than the halo (every row a clamp), every boundary of the
    four-wide horizontal quads, the last partial tile in x and in y."""
    miss = _sweep(pkg("ops"), orc, name, [(H, W) for H in SWEEP_H for W in SWEEP_W])
    assert miss == [], "\n".join(miss[:20])


@pytest.mark.parametrize("name", ["noise", "seam_edge"])
def test_tile_counts(gpu, orc, name):
    for n, (H, W) in TILE_COUNT_SHAPES.items():
        assert -(-H // loss_cases.TILE_H) * -(-W // loss_cases.TILE_W) == n
    miss = _sweep(pkg("ops"), orc, name, list(TILE_COUNT_SHAPES.values()))
    assert miss == [], "\n".join(miss[:20])


# ------------------------------------------------------------------------------------- 5. counter and stream state
K_PSNR = 4.0  # on the float32 oracle's dB error, as K of loss_cases; the floor is FLOOR_ULPS float32 ulps of the dB value


def _psnr_bar(p64, p32):
    return min(K_PSNR * abs(p32 - p64) + loss_cases.FLOOR_ULPS * EPS32 * abs(p64), 1e-3)


# ten calls from a 1-tile image to 1080p; the family changes with the size
SEQUENCE = [("noise", 13, 30), ("near_white", 1080, 1920), ("flat_grey", 96, 160), ("seam_edge", 37, 53),
            ("near_white", 1080, 1920), ("bg_band", 16, 32), ("ramp_xy", 128, 200), ("unclamped", 96, 160),
            ("noise", 1, 1), ("half_identical", 48, 96)]
PSNR_PROBE = ("noise", 7, 13)


def _run_sequence(torch, ops, orc, streams=None, lam=0.2):
    """The sequence twice: blocking calls at the even positions first, then at the odd ones, so that every size returns
    a loss after every kind of predecessor.  Between the calls a compute_psnr on a probe pair, whose value must not
    depend on what ran before it.  streams: alternate between these (synchronised between calls)."""
    import contextlib
    probe = loss_cases.family(*PSNR_PROBE)
    psnr0 = ops.compute_psnr(_dev(probe[0]), _dev(probe[1]), *PSNR_PROBE[1:])
    p64, p32 = orc.compute_psnr(*probe, dtype=np.float64), orc.compute_psnr(*probe, dtype=np.float32)
    assert abs(psnr0 - p64) <= _psnr_bar(p64, p32)
    miss, call = [], 0
    for phase in (0, 1):
        for i, (name, H, W) in enumerate(SEQUENCE):
            pred, gt, loss64, grad64, fig32 = _ref(orc, name, H, W, lam)
            blocking = i % 2 == phase
            ctx = torch.cuda.stream(streams[call % len(streams)]) if streams else contextlib.nullcontext()
            with ctx:
                loss, grad = _loss(ops, pred, gt, lam, blocking=blocking)
                assert (loss is not None) == blocking
                psnr = ops.compute_psnr(_dev(probe[0]), _dev(probe[1]), *PSNR_PROBE[1:])
            if streams:
                torch.cuda.synchronize()
            miss += _judge(f"call {call} {name} {H}x{W} {'blocking' if blocking else 'non-blocking'}", loss, grad, loss64,
                           grad64, fig32, {})
            if psnr != psnr0:
                miss.append(f"call {call}: PSNR of the probe {psnr!r} != {psnr0!r}")
            call += 1
    return miss


def test_mixed_sequence_on_one_stream(gpu, orc):
    miss = _run_sequence(gpu, pkg("ops"), orc)
    assert miss == [], "\n".join(miss)


def test_mixed_sequence_across_two_streams(gpu, orc):
    """Every call on the other stream than the one before: the counters are re-primed on each (`primed.stream != st`)."""
    torch = gpu
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    miss = _run_sequence(torch, pkg("ops"), orc, streams=streams)
    torch.cuda.synchronize()
    assert miss == [], "\n".join(miss)


def test_two_thread_ranks_equal_single_thread(gpu, orc):
    """Two host threads (dist.ThreadGroup ranks), each with its own stream and its own images, 20 blocking calls each at
    the same time: every loss and gradient has the bits of the single-threaded call.  (At most 64 tiles per image, so
    that every spread counter receives one addition and the loss is a deterministic sum; blocking calls, because the
    library's scratch is process-wide and its lock covers a call up to its read-back -- gsplat_hip.h, Threading.)"""
    torch, ops, gdist = gpu, pkg("ops"), pkg("dist")
    cases = [[("seam_edge", 96, 160), ("noise", 37, 53), ("near_white", 128, 256), ("ramp_x", 16, 32)],
             [("flat_grey", 128, 256), ("bg_band", 96, 160), ("unclamped", 13, 27), ("blob", 48, 96)]]
    single = [[_loss(ops, *loss_cases.family(*c), 0.2) for c in rank_cases] for rank_cases in cases]
    torch.cuda.synchronize()
    for rank_cases, res in zip(cases, single):  # the baseline itself is held to the bar
        for c, (loss, grad) in zip(rank_cases, res):
            _, _, loss64, grad64, fig32 = _ref(orc, *c, 0.2)
            assert _judge("single " + c[0], loss, grad, loss64, grad64, fig32, {}) == []

    def body(comm):
        stream = torch.cuda.Stream()
        bad = []
        with torch.cuda.stream(stream):
            comm.barrier()
            for it in range(20):
                k = it % len(cases[comm.rank])
                loss, grad = _loss(ops, *loss_cases.family(*cases[comm.rank][k]), 0.2)
                stream.synchronize()
                want_loss, want_grad = single[comm.rank][k]
                if np.float32(loss).tobytes() != np.float32(want_loss).tobytes() or not torch.equal(grad, want_grad):
                    bad.append((comm.rank, it, cases[comm.rank][k], loss, want_loss))
        return bad

    bad = gdist.ThreadGroup(2).run(body)
    torch.cuda.synchronize()
    assert bad == [[], []], bad


@pytest.mark.parametrize("image,value", [("pred", float("nan")), ("pred", float("inf")), ("gt", float("nan"))])
def test_non_finite_pixel_poisons_its_neighbourhood_only(gpu, orc, image, value):
    """One NaN or +inf pixel: the non-finite gradient entries are the oracle's, the finite ones meet the bar, the loss
    is NaN exactly when the oracle's is -- and the next clean call on the stream returns a finite loss within the bar:
    the call after a poisoned one uses the other counter set, and clears the poisoned one for the call after that."""
    ops = pkg("ops")
    H, W, lam = 96, 160, 0.2
    pred, gt = (a.copy() for a in loss_cases.family("ramp_xy", H, W))
    (pred if image == "pred" else gt)[47, 95, 1] = value  # beside a tile seam in x and in y
    with np.errstate(all="ignore"):
        loss64, grad64, fig32 = loss_cases.oracle_pair(orc, pred, gt, lam)
    assert 0 < (~np.isfinite(grad64)).sum() <= 21 * 21 and np.isnan(loss64)
    loss, grad = _loss(ops, pred, gt, lam)
    g = grad.cpu().numpy()
    assert np.array_equal(np.isfinite(g), np.isfinite(grad64))
    assert np.isnan(loss) == np.isnan(loss64)
    assert _judge(f"{image} {value}", None, g, loss64, grad64, fig32) == []
    for _ in range(3):  # both counter sets come round
        cpred, cgt, closs64, cgrad64, cfig32 = _ref(orc, "ramp_xy", H, W, lam)
        closs, cgrad = _loss(ops, cpred, cgt, lam)
        assert np.isfinite(closs)
        assert _judge("clean call after " + str(value), closs, cgrad, closs64, cgrad64, cfig32) == []


# ---------------------------------------------------------------------------------------------------------- 6. PSNR
PSNR_SIZES = [(1, 1), (1, 2), (7, 13), (16, 16), (255, 257), (1080, 1920), (2160, 3840)]


@pytest.mark.parametrize("shape", PSNR_SIZES)
def test_psnr_matches_f64_oracle(gpu, orc, shape):
    """mse_kernel sums floats per thread, per wave and per counter where the float32 oracle sums float squares in a
    double, so its error is its own: the bar is the float32 oracle's dB error against float64 on the same input times
    K_PSNR plus four float32 ulps of the value, and never above the 1e-3 dB of test_fused_loss_full_hd."""
    ops = pkg("ops")
    H, W = shape
    rng = np.random.default_rng([H, W])
    gt = (0.25 + 0.5 * rng.random((H, W, 3))).astype(np.float32)
    inputs = {"noise": rng.random((H, W, 3), dtype=np.float32), "offset 1e-3": gt + np.float32(1e-3),
              "offset 1e-6": gt + np.float32(1e-6), "identical": gt.copy()}
    d_gt = _dev(gt)
    for what, pred in inputs.items():
        got = ops.compute_psnr(_dev(pred), d_gt, H, W)
        p64, p32 = orc.compute_psnr(pred, gt, dtype=np.float64), orc.compute_psnr(pred, gt, dtype=np.float32)
        err, err32 = abs(got - p64), abs(p32 - p64)
        print(f"  PSNR {H}x{W} {what:12s} kernel {got:.6f} f64 {p64:.6f}  |err| {err:.2e} dB  (float32 oracle {err32:.2e} dB)")
        if what == "identical":
            assert got == 100.0 and p64 == 100.0
            continue
        assert got != 100.0 and np.isfinite(got), what  # an MSE of 1e-12 is not 0
        assert err <= _psnr_bar(p64, p32), (what, got, p64, p32)


# ---------------------------------------------------------------------------------------------------------- 7. Adam
def _same_class(got, want):
    """NaN where NaN, +inf where +inf, -inf where -inf, finite where finite."""
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and
            np.array_equal(np.isneginf(got), np.isneginf(want)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _adam_plain(ops, p, g, m, v, h):
    dp, dm, dv = _dev(p), _dev(m), _dev(v)
    ops.adam_step(dp, _dev(g), dm, dv, *[float(x) for x in h], 1, p.size)
    return dp.cpu().numpy(), dm.cpu().numpy(), dv.cpu().numpy()


ADAM_EQUAL_BITS = True  # measured: every non-NaN entry of p, m and v has the float32 oracle's bits, at every n and setting


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 59000])
def test_adam_step_edge_table(gpu, orc, n):
    """(a) gsplat_adam_step on the edge table, repeated to N * S = n elements, for every hyper-parameter setting.  The
    float32 oracle decides: where its result is finite the kernel stays within test_adam_step_matches_oracle's
    tolerances, where it is not the class (NaN, +inf, -inf) is the oracle's -- an infinite gradient is NOT zeroed by the
    reference and turns the parameter into NaN."""
    import torch
    ops = pkg("ops")
    p, g, m, v = (np.resize(a, max(n, 1)) for a in loss_cases.adam_table())
    equal_bits = True
    for h in loss_cases.adam_hypers():
        if n == 0:  # nothing is touched
            dp = torch.full((4,), 7.0, device="cuda")
            ops.adam_step(dp, dp.clone(), dp.clone(), dp.clone(), *[float(x) for x in h], 0, 59)
            assert (dp == 7.0).all()
            continue
        with np.errstate(all="ignore"):
            po, mo, vo = orc.adam_step(p, g, m, v, *h)
        got = _adam_plain(ops, p, g, m, v, h)
        for what, a, o, rtol, atol in (("p", got[0], po, 2e-6, 1e-7), ("m", got[1], mo, 1e-6, 1e-8), ("v", got[2], vo, 1e-6, 1e-9)):
            assert _same_class(a, o), (what, h)
            fin = np.isfinite(o)
            np.testing.assert_allclose(a[fin], o[fin], rtol=rtol, atol=atol, err_msg=f"{what} {h}")
            same = np.array_equal(_bits(a)[~np.isnan(o)], _bits(o)[~np.isnan(o)])
            equal_bits &= same
            if ADAM_EQUAL_BITS:
                assert same, (what, h)
    if n:
        print(f"  ADAM n={n}: kernel bits == float32 oracle bits on every non-NaN entry: {equal_bits}")


def _group(lib_mod, p, m, v, grad, stride, lr):
    arr = (lib_mod.AdamGroup * 1)()
    arr[0].param, arr[0].exp_avg, arr[0].exp_avg_sq = p.data_ptr(), m.data_ptr(), v.data_ptr()
    arr[0].grad = grad.data_ptr() if grad is not None else None
    arr[0].stride, arr[0].packed_column, arr[0].lr = stride, 0, float(lr)
    return arr


def test_masked_optimizer_steps_equal_adam_step_bit_for_bit(gpu, orc):
    """(b) gsplat_optimizer_step with the table as one group's compacted gradient and a permuted compact_to_global, and
    (c) gsplat_optimizer_step_packed with the table in the live rows of a packed array, against (a) gsplat_adam_step on
    the table itself: gs::adam_values repeats adam_kernel's arithmetic, and the copies must agree on every row, NaN
    payloads aside.  Rows outside the mask keep every bit of p, m and v."""
    import ctypes
    import torch
    ops, lib_mod = pkg("ops"), pkg("_lib")
    lib, check = lib_mod.load(), lib_mod.check
    p, g, m, v = loss_cases.adam_table()
    S = 8
    M, N = p.size // S, 40
    assert M * S == p.size and M < N
    rng = np.random.default_rng(11)
    rows = rng.permutation(N)[:M].astype(np.int32)  # compacted row r lives in global row rows[r]; not sorted
    outside = np.setdiff1d(np.arange(N), rows)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def global_arrays():
        out = []
        for a in (p, m, v):
            full = rng.standard_normal((N, S)).astype(np.float32)
            full[outside[0]] = np.float32([np.nan, np.inf, -np.inf, 1e-40, -0.0, 0.0, 1.0, -1.0])  # bits that must survive
            full[rows] = a.reshape(M, S)
            out.append(full)
        return out

    for h in loss_cases.adam_hypers():
        lr, b1, b2, eps, bias1, bias2 = (float(x) for x in h)
        plain = _adam_plain(ops, p, g, m, v, h)
        with np.errstate(all="ignore"):
            oracle = orc.adam_step(p, g, m, v, *h)
        # (b) compacted gradients + compact_to_global
        start = global_arrays()
        d = [_dev(a) for a in start]
        d_grad, d_rows = _dev(g.reshape(M, S)), _dev(rows)
        check(lib.gsplat_optimizer_step(ctypes.c_void_p(d_rows.data_ptr()), M, _group(lib_mod, *d, d_grad, S, lr), 1, b1, b2,
                                        eps, bias1, bias2, None, None, None, stream()))
        res_b = [t.cpu().numpy() for t in d]
        # (c) packed rows [N, S + 1]: the last column counts the views that saw the row
        packed = rng.standard_normal((N, S + 1)).astype(np.float32)
        packed[:, S] = 0.0
        packed[outside[1], S], packed[outside[2], S] = np.nan, -1.0  # not live either: `> 0` decides
        packed[rows, :S] = g.reshape(M, S)
        packed[rows, S] = 1.0 + (np.arange(M) % 3)
        d2 = [_dev(a) for a in start]
        d_packed = _dev(packed)
        check(lib.gsplat_optimizer_step_packed(ctypes.c_void_p(d_packed.data_ptr()), N, S + 1, _group(lib_mod, *d2, None, S, lr),
                                               1, b1, b2, eps, bias1, bias2, None, None, None, stream()))
        res_c = [t.cpu().numpy() for t in d2]
        for what, a, rb, rc, s0, o in zip("pmv", plain, res_b, res_c, start, oracle):
            a = a.reshape(M, S)
            o = o.reshape(M, S)
            for route, r in (("optimizer_step", rb), ("optimizer_step_packed", rc)):
                assert _same_class(r[rows], o), (route, what, h)
                notnan = ~np.isnan(a)
                assert np.array_equal(_bits(r[rows])[notnan], _bits(a)[notnan]), (route, what, h)
                assert np.array_equal(_bits(r[outside]), _bits(s0[outside])), (route, what, h, "rows outside the mask")
            assert np.array_equal(_bits(rb), _bits(rc)), (what, h)  # the two masked routes: the same function, NaNs included

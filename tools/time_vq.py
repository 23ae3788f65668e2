"""The vector-quantisation entry points (gsplat_vq_assign, gsplat_vq_update) at the sizes of the compressed export -- 1e6
SH-like rows of D = 45 (SH degree 3) against K = 4096 and K = 65 536 centroids, and D = 24 (degree 2) against 65 536 -- by
events, warm, beside what a caller could write without them, in the same session: the chunked torch expression
(x_chunk @ C.T, the norms added, argmin) for the assign and index_add_ / bincount for the update.  Prints the achieved
TFLOP/s of the assign (2 N K (D + 1) FLOP) against the 157.3 TF peak of the f32-input matrix cores, how many rows the two
assigns disagree on, and the wall time of a 10-iteration ops.vq_fit.
Warm: 2 calls before the 7 that count; medians.

usage: python tools/time_vq.py [--no-fit]   (JSON lines on stdout)"""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("3dgs_amd.ops")

SIZES = ((1_000_000, 45, 4096), (1_000_000, 45, 65536), (1_000_000, 24, 65536))  # (N, D, K)
PEAK_TF = 157.3
CHUNK = 8192  # rows per torch chunk: an [8192, 65536] float matrix is 2 GB


def by_events(fn, warm=2, reps=7):
    ts = []
    for rep in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warm:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))  # ms


def torch_assign(x, c, out):
    norms = (c * c).sum(1)
    ct = c.t().contiguous()
    for a in range(0, x.shape[0], CHUNK):
        out[a:a + CHUNK] = torch.addmm(norms, x[a:a + CHUNK], ct, alpha=-2.0).argmin(1)
    return out


def torch_update(x, index, c):
    sums = torch.zeros_like(c).index_add_(0, index, x)
    counts = torch.bincount(index, minlength=c.shape[0]).to(torch.float32)[:, None]
    return torch.where(counts > 0, sums / counts.clamp(min=1.0), c)


def main(fit=True):
    for N, D, K in SIZES:
        g = torch.Generator(device="cuda").manual_seed(N + D + K)
        # SH-like rows: a few thousand loose clusters, as a trained scene's bands form
        centres = 0.1 * torch.randn(2048, D, device="cuda", generator=g)
        x = (centres[torch.randint(0, 2048, (N,), device="cuda", generator=g)]
             + 0.03 * torch.randn(N, D, device="cuda", generator=g)).contiguous()
        c = x[torch.randperm(N, device="cuda", generator=g)[:K]].contiguous()
        index, dist = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, device="cuda")
        t_index = torch.empty(N, dtype=torch.int64, device="cuda")
        ops.vq_assign(x, c, index, dist)
        torch_assign(x, c, t_index)
        differ = int((index.long() != t_index).sum())
        flop = 2.0 * N * K * (D + 1)
        ms = dict(assign=by_events(lambda: ops.vq_assign(x, c, index)),
                  assign_with_dist=by_events(lambda: ops.vq_assign(x, c, index, dist)),
                  torch_assign=by_events(lambda: torch_assign(x, c, t_index)))
        # the update: the kernel alone (order and start made once), the wrapper with its sort, and torch's atomics
        order = torch.sort(index, stable=True).indices.to(torch.int32).contiguous()
        start = torch.zeros(K + 1, dtype=torch.int32, device="cuda")
        start[1:] = torch.cumsum(torch.bincount(index, minlength=K), 0)
        book = c.clone()
        lib, p = importlib.import_module("3dgs_amd._lib"), ops._p
        ms["update_kernel"] = by_events(lambda: lib.check(lib.load().gsplat_vq_update(
            p(x), p(order), p(start), N, D, K, p(book), ops._stream())))
        ms["update_with_sort"] = by_events(lambda: ops.vq_update(x, index, book))
        idx64 = index.long()
        ms["torch_update"] = by_events(lambda: torch_update(x, idx64, c))
        line = dict(N=N, D=D, K=K, rows_where_the_two_assigns_differ=differ, largest_cluster=int(torch.bincount(index).max()),
                    assign_tflops=round(flop / ms["assign"] * 1e-9, 1),
                    assign_fraction_of_peak=round(flop / ms["assign"] * 1e-9 / PEAK_TF, 3),
                    torch_assign_tflops=round(flop / ms["torch_assign"] * 1e-9, 1),
                    torch_over_assign=round(ms["torch_assign"] / ms["assign"], 2))
        line.update({k + "_ms": round(v, 3) for k, v in ms.items()})
        if fit:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, objective = ops.vq_fit(x, K, iterations=10, seed=0)
            torch.cuda.synchronize()
            line["fit_10_iterations_wall_s"] = round(time.perf_counter() - t0, 3)
            line["fit_objective_per_assign"] = [float(f"{o:.6g}") for o in objective]
        print(json.dumps(line), flush=True)
        del x, c, index, dist, t_index, order, start, book, idx64


if __name__ == "__main__":
    main(fit="--no-fit" not in sys.argv[1:])

"""The per-gaussian state of a training run as one table: every tensor that has a row per gaussian, named once.

A row edit of the Trainer (compaction, Morton re-order, densification, MCMC growth and relocation) is a function of one
column, mapped over the table; Trainer._install then makes the result the run's state.  Nothing here touches the HIP
library -- the row functions (ops.gather_rows, ops.compact_masked_array, torch.cat, indexing) are handed in -- so the table
is the same thing on CPU tensors (tests/test_rows_cpu.py).
"""
import torch

GROUPS = ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")

# the kind of a column: what a row edit has to decide for it
PARAM, MOMENT, STAT = "param", "moment", "stat"


def _with_coefficients(params):
    """The groups that have bytes per row: all but `sh` while it is [N,0,3]."""
    return [g for g in GROUPS if g != "sh" or params["sh"].shape[1] > 0]


class RowTable:
    """params: dict group -> [N, ...] float32, all six groups, `sh` [N,0,3] while there are no SH coefficients;
    exp_avg / exp_avg_sq: dict group -> the Adam moments, shaped as their parameter (no `sh` entry at SH degree 0);
    uv_grad_accum [N] float32 and grad_accum_dur [N] int32: the densification statistics;
    features: None, or (features, exp_avg, exp_avg_sq), three [N,C] float32 -- the feature column of a run that trains a
    per-gaussian feature field (config key features) and its Adam moments.  It is not one of GROUPS: the optimizer's group
    list does not step it (ops.feature_adam_step does), but every row edit carries it."""

    def __init__(self, params, exp_avg, exp_avg_sq, uv_grad_accum, grad_accum_dur, features=None):
        self.params = {g: params[g] for g in GROUPS}
        self.exp_avg = {g: exp_avg[g] for g in GROUPS if g in exp_avg}
        self.exp_avg_sq = {g: exp_avg_sq[g] for g in GROUPS if g in exp_avg_sq}
        self.uv_grad_accum, self.grad_accum_dur = uv_grad_accum, grad_accum_dur
        self.features = None if features is None else tuple(features)
        if self.features is not None and len(self.features) != 3:
            raise ValueError("features must be (features, exp_avg, exp_avg_sq)")

    @classmethod
    def fresh(cls, params, features=None):
        """The table of a run that starts from `params` (and the [N,C] feature column `features`, if it has one): moments
        and statistics at zero."""
        n, dev = params["xyz"].shape[0], params["xyz"].device
        with_moments = _with_coefficients(params)
        return cls(params, {g: torch.zeros_like(params[g]) for g in with_moments},
                   {g: torch.zeros_like(params[g]) for g in with_moments},
                   torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                   None if features is None else (features, torch.zeros_like(features), torch.zeros_like(features)))

    @property
    def num_rows(self):
        return int(self.params["xyz"].shape[0])

    def map(self, fn):
        """A new table of fn(kind, name, tensor) for every column -- kind: PARAM, MOMENT or STAT; name: the group of a
        parameter or moment, the attribute of a statistic.  Two columns never reach fn.  The `sh` parameter without
        coefficients has no bytes to move: it comes back as [n,0,3] at the new row count.  grad_accum_dur is handed over
        as a float32 view of its int32 and viewed back, because the row functions move float32 words; they only copy,
        so every bit pattern survives, NaNs and denormals included.  A table with the feature column hands it over
        last, as PARAM "features", and its two moments as MOMENT "features"."""
        params = {g: fn(PARAM, g, self.params[g]) for g in _with_coefficients(self.params)}
        params.setdefault("sh", self.params["sh"].new_empty((params["xyz"].shape[0], 0, 3)))
        out = RowTable(params, {g: fn(MOMENT, g, t) for g, t in self.exp_avg.items()},
                       {g: fn(MOMENT, g, t) for g, t in self.exp_avg_sq.items()},
                       fn(STAT, "uv_grad_accum", self.uv_grad_accum),
                       fn(STAT, "grad_accum_dur", self.grad_accum_dur.view(torch.float32)).view(torch.int32))
        if self.features is not None:
            f, m, v = self.features
            out.features = (fn(PARAM, "features", f), fn(MOMENT, "features", m), fn(MOMENT, "features", v))
        return out

    def check(self):
        """What the kernels take on trust, from the tensors' metadata alone (nothing is read back): every column has
        num_rows rows, its dtype and is contiguous; every group with coefficients has both moments, shaped as it is; the
        feature column, when there is one, is [N,C] with 1 <= C <= 512 and so are its moments."""
        n = self.num_rows
        with_moments = _with_coefficients(self.params)
        if list(self.exp_avg) != with_moments or list(self.exp_avg_sq) != with_moments:
            raise ValueError("moments of %s and %s for the groups %s" % (list(self.exp_avg), list(self.exp_avg_sq), with_moments))
        columns = [("params." + g, t, torch.float32, None) for g, t in self.params.items()]
        for g in with_moments:
            columns += [("exp_avg." + g, self.exp_avg[g], torch.float32, self.params[g].shape),
                        ("exp_avg_sq." + g, self.exp_avg_sq[g], torch.float32, self.params[g].shape)]
        columns += [("uv_grad_accum", self.uv_grad_accum, torch.float32, (n,)),
                    ("grad_accum_dur", self.grad_accum_dur, torch.int32, (n,))]
        if self.features is not None:
            f = self.features[0]
            if f.dim() != 2 or not 1 <= f.shape[1] <= 512:
                raise ValueError("features has shape %s: not [N,C] with 1 <= C <= 512" % (tuple(f.shape),))
            columns += [("features", f, torch.float32, None), ("exp_avg.features", self.features[1], torch.float32, f.shape),
                        ("exp_avg_sq.features", self.features[2], torch.float32, f.shape)]
        for name, t, dtype, shape in columns:
            if t.dim() == 0 or t.shape[0] != n or (shape is not None and tuple(t.shape) != tuple(shape)):
                raise ValueError("%s has shape %s in a table of %d rows" % (name, tuple(t.shape), n))
            if t.dtype != dtype:
                raise ValueError("%s is %s, not %s" % (name, t.dtype, dtype))
            if not t.is_contiguous():
                raise ValueError("%s is not contiguous" % name)

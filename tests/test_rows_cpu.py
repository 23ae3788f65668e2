"""The Trainer's table of per-gaussian columns (3dgs_amd/rows.py) on CPU tensors: a gather, compactions and an append
through RowTable.map with torch indexing standing in for the library's row functions, and what Trainer._install refuses.
No library is loaded."""
import numpy as np
import pytest
import torch

from conftest import pkg

N, K = 37, 5
GROUPS = ("xyz", "rgb", "sh", "opacity", "scale", "quaternion")
# read as float32: a quiet NaN with a payload, the smallest denormal, minus zero, another NaN; and small counts
COUNTS = np.array([0x7FC00001, 0x00000001, 0x80000000, 0xFFFFFFFF, 3, 12, 0, 7], np.uint32).view(np.int32)
M_TAG, V_TAG, UV_TAG = 0.25, 0.5, 0.75  # a column holds its row id plus this


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def load():
        raise AssertionError("the table and its installation need no library")
    monkeypatch.setattr(pkg("_lib"), "load", load)


def _table(degree):
    """N rows at SH degree `degree`: every element of row i of a parameter is i, of exp_avg i + 0.25, of exp_avg_sq
    i + 0.5, uv_grad_accum[i] = i + 0.75, and grad_accum_dur cycles through COUNTS."""
    rows = pkg("rows")
    row = dict(xyz=(3,), rgb=(3,), sh=((degree + 1) ** 2 - 1, 3), opacity=(), scale=(3,), quaternion=(4,))
    ids = torch.arange(N, dtype=torch.float32)

    def col(g, tag):
        return (ids + tag).reshape((N,) + (1,) * len(row[g])).expand((N,) + row[g]).contiguous()

    moments = [g for g in GROUPS if g != "sh" or degree > 0]
    return rows.RowTable({g: col(g, 0.0) for g in GROUPS}, {g: col(g, M_TAG) for g in moments},
                         {g: col(g, V_TAG) for g in moments}, ids + UV_TAG, torch.from_numpy(np.resize(COUNTS, N)))


def _columns(t):
    return ([("params." + g, c, 0.0) for g, c in t.params.items()] + [("exp_avg." + g, c, M_TAG) for g, c in t.exp_avg.items()]
            + [("exp_avg_sq." + g, c, V_TAG) for g, c in t.exp_avg_sq.items()] + [("uv_grad_accum", t.uv_grad_accum, UV_TAG)])


def _assert_rows(got, before, want_ids, want_counts, degree):
    """`got` holds the rows want_ids of `before`, in that order, in every column."""
    n = len(want_ids)
    got.check()
    assert got.num_rows == n
    for (name, c, tag), (_, old, _) in zip(_columns(got), _columns(before)):
        assert c.shape == (n,) + old.shape[1:] and c.dtype == old.dtype == torch.float32, name
        assert torch.equal(c, (want_ids.float() + tag).reshape((n,) + (1,) * (c.dim() - 1)).expand_as(c)), name
    assert got.grad_accum_dur.dtype == torch.int32 and got.grad_accum_dur.shape == (n,)
    assert got.grad_accum_dur.numpy().tobytes() == want_counts.numpy().tobytes()
    assert list(got.params) == list(GROUPS) and got.params["sh"].shape == (n, (degree + 1) ** 2 - 1, 3)
    moments = [g for g in GROUPS if g != "sh" or degree > 0]
    assert list(got.exp_avg) == moments and list(got.exp_avg_sq) == moments


def _mask(kind):
    keep = torch.zeros(N, dtype=torch.bool)
    if kind == "some":
        keep[torch.randperm(N, generator=torch.Generator().manual_seed(5))[:19]] = True
    elif kind == "one":
        keep[23] = True
    else:
        keep[:] = True
    return keep


@pytest.mark.parametrize("degree", [0, 2])
def test_gather_compact_and_append_move_every_column_alike(degree):
    rows = pkg("rows")
    table = _table(degree)
    ids, counts = torch.arange(N), table.grad_accum_dur.clone()
    seen = []

    def through(edit):
        def fn(kind, name, t):
            seen.append((kind, name, t.dtype, tuple(t.shape[1:])))
            return edit(t)
        return fn

    order = torch.randperm(N, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(order, ids)
    got = table.map(through(lambda t: t[order]))
    _assert_rows(got, table, ids[order], counts[order], degree)
    # what the function was handed: every column once, float32 only, never a column without bytes
    assert len(seen) == (20 if degree else 17) and all(s[2] == torch.float32 and 0 not in s[3] for s in seen)
    assert sorted(s[0] for s in seen) == sorted([rows.PARAM] * (6 if degree else 5) + [rows.MOMENT] * (12 if degree else 10)
                                                + [rows.STAT] * 2)
    assert [s[1] for s in seen if s[0] == rows.STAT] == ["uv_grad_accum", "grad_accum_dur"]
    for kind in ("some", "all", "one"):
        keep = _mask(kind)
        assert int(keep.sum()) == dict(some=19, all=N, one=1)[kind]
        got = table.map(through(lambda t: t[keep]))
        _assert_rows(got, table, ids[keep], counts[keep], degree)
    src = torch.tensor([3, 36, 3, 0, 17])
    assert len(src) == K
    got = table.map(through(lambda t: torch.cat([t, t[src]], 0)))
    _assert_rows(got, table, torch.cat([ids, ids[src]]), torch.cat([counts, counts[src]]), degree)
    # edits compose: the table that came out of one goes into the next
    again = got.map(through(lambda t: t[:N])).map(through(lambda t: t[order]))
    _assert_rows(again, table, ids[order], counts[order], degree)
    _assert_rows(table, table, ids, counts, degree)  # and the table mapped from is as it was


def test_fresh_table_starts_at_zero():
    rows = pkg("rows")
    for degree in (0, 2):
        src = _table(degree)
        t = rows.RowTable.fresh(src.params)
        t.check()
        assert all(t.params[g] is src.params[g] for g in GROUPS)
        assert list(t.exp_avg) == list(src.exp_avg) and list(t.exp_avg_sq) == list(src.exp_avg_sq)
        for g in t.exp_avg:
            assert t.exp_avg[g].shape == src.params[g].shape and not t.exp_avg[g].any() and not t.exp_avg_sq[g].any()
            assert t.exp_avg[g].data_ptr() != t.exp_avg_sq[g].data_ptr()
        assert t.uv_grad_accum.shape == (N,) and t.uv_grad_accum.dtype == torch.float32 and not t.uv_grad_accum.any()
        assert t.grad_accum_dur.shape == (N,) and t.grad_accum_dur.dtype == torch.int32 and not t.grad_accum_dur.any()


def _uninstalled_trainer():
    """A Trainer that has been given nothing but what _install reads: no context, no views, no device."""
    trainer_mod = pkg("trainer")
    t = object.__new__(trainer_mod.Trainer)
    t.cfg, t.scene_extent = dict(trainer_mod.DEFAULT_CONFIG), 1.0
    t._sharded, t._filter3d = "stale", "stale"
    return t


@pytest.mark.parametrize("degree", [0, 2])
def test_install_binds_the_optimizer_to_the_tables_tensors(degree):
    table = _table(degree)
    t = _uninstalled_trainer()
    t._install(table)
    assert t.l_max == t.opt.l_max == degree and t.num_gaussians == N
    assert t._sharded is None and t._filter3d is None
    assert list(t.params) == list(GROUPS) and all(t.params[g] is table.params[g] for g in GROUPS)
    assert t.opt.names == [g for g in GROUPS if g != "sh" or degree > 0] == list(t.opt.params)
    for g in t.opt.names:
        assert t.opt.params[g] is t.params[g]
        assert t.opt.exp_avg[g] is table.exp_avg[g] and t.opt.exp_avg_sq[g] is table.exp_avg_sq[g]
    assert t.opt.uv_grad_accum is table.uv_grad_accum and t.opt.grad_accum_dur is table.grad_accum_dur
    back = t._rows()
    assert all(back.params[g] is table.params[g] for g in GROUPS) and list(back.exp_avg) == list(table.exp_avg)
    # a second table over the first: nothing of the old one stays bound
    t._sharded, t._filter3d = "stale", "stale"
    second = back.map(lambda kind, name, c: c[:N - 4].clone())
    t._install(second)
    assert t.num_gaussians == N - 4 and t._sharded is None and t._filter3d is None
    for g in t.opt.names:
        assert t.opt.params[g] is t.params[g] is second.params[g] and t.opt.exp_avg[g] is second.exp_avg[g]
    assert t.opt.grad_accum_dur.shape == (N - 4,) and t.opt.grad_accum_dur.dtype == torch.int32


def _one_row_short(t):
    t.uv_grad_accum = t.uv_grad_accum[:N - 1].clone()


def _short_parameter(t):
    t.params["scale"] = t.params["scale"][1:].clone()


def _float64_moment(t):
    t.exp_avg_sq["opacity"] = t.exp_avg_sq["opacity"].double()


def _float32_counts(t):
    t.grad_accum_dur = t.grad_accum_dur.float()


def _strided_column(t):
    t.exp_avg["quaternion"] = torch.zeros(N, 8)[:, ::2]


def _strided_parameter(t):
    t.params["xyz"] = torch.zeros(3, N).t()


def _moment_of_another_shape(t):
    t.exp_avg["sh"] = torch.zeros(N, 3, 3)


def _missing_moment(t):
    del t.exp_avg_sq["rgb"]


@pytest.mark.parametrize("spoil, says", [
    (_one_row_short, "uv_grad_accum has shape"), (_short_parameter, "has shape"), (_float64_moment, "exp_avg_sq.opacity is"),
    (_float32_counts, "grad_accum_dur is"), (_strided_column, "exp_avg.quaternion is not contiguous"),
    (_strided_parameter, "params.xyz is not contiguous"), (_moment_of_another_shape, "exp_avg.sh has shape"),
    (_missing_moment, "moments of")], ids=lambda v: getattr(v, "__name__", None))
def test_install_refuses_a_table_the_kernels_could_not_take(spoil, says):
    table = _table(2)
    t = _uninstalled_trainer()
    t._install(table)
    spoil(table)
    with pytest.raises(ValueError, match=says):
        t._install(table)
    assert t.num_gaussians == N and t.opt.params["xyz"] is t.params["xyz"]  # the state before it stands


def test_install_refuses_an_sh_column_of_no_degree():
    table = _table(2)
    for g in ("params", "exp_avg", "exp_avg_sq"):
        getattr(table, g)["sh"] = torch.zeros(N, 5, 3)
    table.check()
    with pytest.raises(ValueError, match="SH degree"):
        _uninstalled_trainer()._install(table)

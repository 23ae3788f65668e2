"""CPU checks of the MCMC densification: the float64 reference (tests/mcmc_reference.py) against values computed with
60-digit arithmetic, the sampler's guarantee on zero-weight rows, the config keys and the growth schedule."""
import numpy as np
import pytest

import mcmc_reference as ref
from conftest import pkg


def test_relocation_of_one_copy_changes_nothing():
    for o in (0.005, 0.5, 0.99, 0.999999):
        on, coef = ref.relocation(o, 1)
        assert on == pytest.approx(o, rel=1e-15) and coef == pytest.approx(1.0, rel=1e-15)


# (o, n) -> o' = 1 - (1 - o)^(1/n) and the scale coefficient o / den, from 60-digit arithmetic (twelve figures kept)
TABLE = [((0.5, 2), 0.292893218813, 0.952151953766), ((0.99, 51), 0.0863406273608, 0.642124406974),
         ((0.999999, 51), 0.237301414098, 0.515304035384)]


@pytest.mark.parametrize("case,o_new,coef", TABLE, ids=[f"o{c[0][0]}-n{c[0][1]}" for c in TABLE])
def test_relocation_reproduces_the_high_precision_values(case, o_new, coef):
    got_o, got_c = ref.relocation(*case)
    assert got_o == pytest.approx(o_new, rel=1e-7)
    assert got_c == pytest.approx(coef, rel=1e-7)


def test_hockey_stick_form_equals_the_double_sum():
    """The n-term sum the kernel evaluates, sum_k C(n, k+1) (-1)^k o'^(k+1) / sqrt(k+1), in the kernel's own order and
    plain double arithmetic, against the reference's exactly summed double sum: the alternating series costs double
    nothing that float32 storage could show."""
    import math
    for o in (0.005, 0.5, 0.9, 0.99, 0.999999, 1.0 / (1.0 + math.exp(-20.0))):
        for n in (2, 3, 10, 50, 51):
            on, coef = ref.relocation(o, n)
            den, binom, power = 0.0, 1.0, 1.0
            for k in range(n):
                binom = binom * (n - k) / (k + 1)
                assert binom == math.comb(n, k + 1)
                power *= on
                term = binom * power / math.sqrt(k + 1)
                den += -term if k & 1 else term
            assert o / den == pytest.approx(coef, rel=1e-10), (o, n)


def test_sampler_never_returns_a_zero_weight_row():
    rng = np.random.default_rng(11)
    w = rng.random(1000)
    zero = rng.random(1000) < 0.3
    zero[[0, 999]] = True
    w[zero] = 0.0
    for seed in (0, 1, 2 ** 40 + 7):
        samples, counts = ref.sample_by_weight(w, 4096, seed)
        assert samples.min() >= 0 and samples.max() < 1000
        assert not zero[samples].any()
        assert counts.sum() == 4096 and (counts[zero] == 0).all()
    # a single live row in front of / behind zeros takes every draw
    for live in (0, 999, 500):
        w1 = np.zeros(1000)
        w1[live] = 3.0
        assert (ref.sample_by_weight(w1, 64, 5)[0] == live).all()


def test_uniforms_and_normals_of_the_reference_generator():
    u = ref.uniform(3, np.arange(100000))
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 5e-3
    z = ref.normal(3, np.arange(100000))
    assert abs(z.mean()) < 1e-2 and abs(z.std() - 1.0) < 1e-2 and np.abs(z).max() <= ref.NORMAL_MAX


def test_config_defaults_and_extension_key(tmp_path):
    cfg = pkg("trainer").DEFAULT_CONFIG
    assert cfg["mcmc"] is False
    assert cfg["mcmc_min_opacity"] == 0.005 and cfg["mcmc_noise_lr"] == 5e5 and cfg["mcmc_grow_factor"] == 1.05
    assert cfg["mcmc_opacity_reg"] == 0.01 and cfg["mcmc_scale_reg"] == 0.01
    ds = pkg("dataset")
    f = tmp_path / "c.yaml"
    f.write_text("num_iters: 5\nmcmc: true\nmcmc_noise_lr: 1000\n")
    assert ds.parseExtensions(f) == {"mcmc": True}  # (the numeric keys are dict-only)
    f.write_text("num_iters: 5\n")
    assert ds.parseExtensions(f) == {}


def test_growth_sequence_to_the_cap():
    growth = pkg("trainer").mcmc_growth
    n, seen = 1000, []
    for _ in range(8):
        n += growth(n, 1.05, 1300)
        seen.append(n)
    assert seen == [1050, 1102, 1157, 1214, 1274, 1300, 1300, 1300]
    assert growth(1300, 1.05, 1300) == 0 and growth(2000, 1.05, 1300) == 0 and growth(0, 1.05, 1300) == 0
    assert growth(10, 1.05, 1300) == 0  # int(10.5) = 10: a set this small does not grow at 5 %

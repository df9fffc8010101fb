"""Host builders of the coefficient rows for many parameter draws (parambasis.gaussian_rows_many / bias_rows_many,
marginal.joint_gaussian_rows_many): draw for draw the bits of the scalar builders they vectorise."""
import numpy as np
import pytest

import cfg3_util as U


def _draws(n, seed=3):
    rng = np.random.default_rng(seed)
    f = np.repeat(rng.uniform(0.6, 0.9, 4), [3, 0, 5, n - 8])  # draws of one walker share its growth rate
    return rng, f


@pytest.mark.parametrize("cross", [False, True])
def test_westcoast_rows_many_equal_the_scalar_rows(cross):
    from eftpipe_amd.parambasis import gaussian_rows, gaussian_rows_many

    rng, f = _draws(12)
    ngA = np.stack([rng.uniform(1.5, 2.5, 12), rng.normal(0, 1, 12), rng.normal(0, 1, 12)], axis=1)
    ngB = np.stack([rng.uniform(1.0, 1.8, 12), rng.normal(0, 1, 12), rng.normal(0, 1, 12)], axis=1) if cross else None
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5, kmB=0.45, krB=0.35, ndB=3e-4) if cross else dict(kmA=0.7, krA=0.35, ndA=4.5e-5)
    many = gaussian_rows_many(f, ngA, ngB, **sc)
    for i in range(12):
        one = gaussian_rows(float(f[i]), [float(v) for v in ngA[i]], None if ngB is None else [float(v) for v in ngB[i]], **sc)
        assert many[i].shape == one.shape
        assert np.array_equal(many[i], one), i
    # one growth rate for every draw
    assert np.array_equal(gaussian_rows_many(0.77, ngA, ngB, **sc)[5], gaussian_rows(0.77, list(ngA[5]), None if ngB is None else list(ngB[5]), **sc))


def test_eastcoast_rows_many_equal_the_scalar_rows():
    from eftpipe_amd.parambasis import gaussian_rows, gaussian_rows_many

    rng, f = _draws(10, seed=5)
    f = f + rng.uniform(0, 1e-3, 10)  # every draw its own growth rate (the per-draw powers of f)
    ng = np.stack([rng.uniform(1.5, 2.5, 10), rng.normal(0, 1, 10), rng.normal(0, 1, 10)], axis=1)
    many = gaussian_rows_many(f, ng, basis="eastcoast", kmA=0.7, krA=0.25, ndA=3e-4)
    for i in range(10):
        assert np.array_equal(many[i], gaussian_rows(float(f[i]), [float(v) for v in ng[i]], basis="eastcoast", kmA=0.7, krA=0.25, ndA=3e-4)), i


@pytest.mark.parametrize("counterform", ["westcoast", "eastcoast"])
def test_bias_rows_many_equal_bias_row(counterform):
    from eftpipe_amd.parambasis import bias_row, bias_rows_many

    rng = np.random.default_rng(11)
    N = 9
    f = rng.uniform(0.6, 0.9, N)
    bsA, bsB, es = rng.normal(1, 1, (N, 7)), rng.normal(1, 1, (N, 7)), rng.normal(0, 1, (N, 3))
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5, kmB=0.6, krB=0.3, ndB=2e-4)
    for B_ in (None, bsB):
        many = bias_rows_many(f, bsA, B_, es, counterform=counterform, **sc)
        for i in range(N):
            one = bias_row(float(f[i]), [float(v) for v in bsA[i]], None if B_ is None else [float(v) for v in B_[i]], tuple(float(v) for v in es[i]),
                           counterform=counterform, **sc)
            assert np.array_equal(many[i], one), i


def test_cfg3_joint_rows_many_equal_the_scalar_rows(golden):
    from eftpipe_amd.marginal import joint_gaussian_rows, joint_gaussian_rows_many

    g = golden("cfg3")
    p = U.params(g)
    names = [str(n) for n in g["full_names"]]
    f = [float(g[t + "_f"]) for t in U.TRACERS]
    N = 7
    rng = np.random.default_rng(2)
    draws = {k: np.full(N, v) for k, v in p.items()}
    for k in ("LRG_NGC_b1", "ELG_NGC_b1", "LRG_NGC_b2", "ELG_NGC_b4"):
        draws[k] = p[k] + 0.1 * rng.normal(size=N)
    fs = [np.full(N, ft) for ft in f]
    fs[1][4:] *= 0.99
    many = joint_gaussian_rows_many(U.bases(), fs, draws, names, U.scales(g))
    assert many.shape == (N, 3, len(names) + 1, 24)
    for i in range(N):
        one = joint_gaussian_rows(U.bases(), [float(x[i]) for x in fs], {k: float(v[i]) for k, v in draws.items()}, names, U.scales(g))
        assert np.array_equal(many[i], one), i
    # parameters shared by every draw may stay scalars
    shared = dict(p, LRG_NGC_b1=draws["LRG_NGC_b1"])
    assert np.array_equal(joint_gaussian_rows_many(U.bases(), f, shared, names, U.scales(g))[3],
                          joint_gaussian_rows(U.bases(), f, dict(p, LRG_NGC_b1=float(draws["LRG_NGC_b1"][3])), names, U.scales(g)))


def test_rows_many_shape_errors():
    from eftpipe_amd.marginal import joint_gaussian_rows_many
    from eftpipe_amd.parambasis import bias_rows_many, gaussian_rows_many

    with pytest.raises(ValueError):
        gaussian_rows_many(np.ones(4), np.ones((4, 2)))  # three non-Gaussian parameters per draw
    with pytest.raises(ValueError):
        gaussian_rows_many(np.ones(3), np.ones((4, 3)))  # f for another number of draws
    with pytest.raises(ValueError):
        gaussian_rows_many(0.7, np.ones(3))  # one draw still comes as [1, 3]
    with pytest.raises(ValueError):
        gaussian_rows_many(0.7, np.ones((4, 3)), np.ones((5, 3)))
    with pytest.raises(ValueError):
        bias_rows_many(0.7, np.ones((4, 6)))
    with pytest.raises(ValueError):
        bias_rows_many(0.7, np.ones((4, 7)), es=np.ones((3, 3)))
    with pytest.raises(ValueError):
        joint_gaussian_rows_many(U.bases(), [0.7] * 3, {"LRG_NGC_b1": np.ones(4), "ELG_NGC_b1": np.ones(5)}, [], [{}] * 3)

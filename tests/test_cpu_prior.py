"""Gaussian priors beside run-time models, the parts that need no GPU: what with_prior refuses (shape, dtype, device, manifold, kind)
and the argument checks of the five C entries (the C++ adaptor's with_prior compiling with plain g++: tests/test_cpp_prior.py)."""
import types

import pytest
import torch

E_ARG = -1


def _bound(cls, P=4, n=3, dtype=torch.float64, manifold="euclid", kind="residual"):
    """A bound model as with_prior sees it (no GPU: nothing is compiled, nothing is launched)."""
    m = cls.__new__(cls)
    m.res = types.SimpleNamespace(kind=kind, manifold=manifold, n=n)
    m.P, m.n, m.dtype = P, n, dtype
    m.packed = m.data = torch.zeros(1, dtype=dtype)   # (what the model's device is read from)
    return m


@pytest.mark.parametrize("ragged", [False, True])
def test_with_prior_takes_both_forms(ragged):
    import tinyopt_amd as ta
    m = _bound(ta.RaggedJitModel if ragged else ta.JitModel)
    mu = torch.zeros(4, 3, dtype=torch.float64)
    d = m.with_prior(mu, torch.ones(4, 3, dtype=torch.float64))
    assert d is not m and m.prior is None and d.prior[2] == 0            # [P, n]: the diagonal form
    for k in (1, 3):
        f = m.with_prior(mu, torch.ones(4, k, 3, dtype=torch.float64))
        assert f.prior[2] == k                                           # [P, k, n]: the full form, k from the shape
    lf = m.with_loss("huber", 0.5).with_prior(mu, torch.ones(4, 3, dtype=torch.float64))
    assert lf.loss == "huber" and lf.prior is not None                   # composes with with_loss, either way round
    fl = d.with_loss("huber", 0.5)
    assert fl.loss == "huber" and fl.prior is d.prior


@pytest.mark.parametrize("mu_shape,W_shape,kw,why", [
    ((4, 2), (4, 3), {}, r"mu must be \[P, n\]"),
    ((3, 3), (4, 3), {}, r"mu must be \[P, n\]"),
    ((4, 3), (4, 2), {}, r"diagonal W must be \[P, n\]"),
    ((4, 3), (4, 4, 3), {}, "1 <= k <= n"),                       # rows > n
    ((4, 3), (4, 0, 3), {}, "1 <= k <= n"),
    ((4, 3), (4, 2, 4), {}, r"full W must be \[P, k, n\]"),
    ((4, 3), (12,), {}, "1-dimensional"),
    ((4, 3), (4, 3), dict(W_dtype=torch.float32), "W must have the model's dtype"),
    ((4, 3), (4, 3), dict(mu_dtype=torch.float32), "mu must have the model's dtype"),
    ((4, 3), (4, 3), dict(W_device="meta"), "W must be on the model's device"),
    ((4, 3), (4, 3), dict(manifold="se3"), "manifold='se3'"),
    ((4, 3), (4, 3), dict(manifold="user"), "manifold='user'"),
    ((4, 3), (4, 3), dict(kind="cost"), "scalar cost"),
    ((4, 3), (4, 3), dict(kind="cost_grad"), "scalar cost"),
])
def test_with_prior_says_why_it_refuses(mu_shape, W_shape, kw, why):
    import tinyopt_amd as ta
    m = _bound(ta.JitModel, manifold=kw.get("manifold", "euclid"), kind=kw.get("kind", "residual"))
    mu = torch.zeros(mu_shape, dtype=kw.get("mu_dtype", torch.float64))
    W = torch.zeros(W_shape, dtype=kw.get("W_dtype", torch.float64), device=kw.get("W_device", "cpu"))
    with pytest.raises(ValueError, match=why):
        m.with_prior(mu, W)


def test_prior_entries_refuse_a_null_handle(built):
    from tinyopt_amd import _capi
    lib = _capi.load()
    calls = {
        "toa_jit_lm_run_prior": (None, None, 4, 2, None, None, None, None, None, None),
        "toa_jit_accumulate_prior": (None, None, 4, 2, None, None, None, 1, None, None, None, None),
        "toa_jit_lm_run_ragged_prior": (None, None, None, None, 4, 8, 2, None, None, None, None, None, None, 0),
        "toa_jit_accumulate_ragged_prior": (None, None, None, None, 4, 8, 2, None, None, None, 1, None, None, None, None),
        "toa_jit_model_stats_prior": (None, None, 0, None, None, None),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == E_ARG, name
        assert name.encode() in lib.toa_last_error() and b"null handle" in lib.toa_last_error()
    assert lib.toa_abi_version() == 7   # additive
    p = _capi.ToaPrior()
    assert p.rows == 0 and len(p.reserved) == 5

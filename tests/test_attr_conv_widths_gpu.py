"""The standalone convolution op (`mke_attr_conv_fwd` / `mke_attr_conv_bwd`) at the edges of every kernel instantiation,
against the float64 oracle (`forward(...)["flat"]`, `conv_backward`).

  forward            a wavefront per triple,           1..5 positions per lane:  dim 1..320
  backward, dim<=96  two triples per wavefront,        1..3 positions per lane
  backward, dim>96   a wavefront per triple,           2..5 positions per lane

n = 37 is no multiple of any per-block triple count; n = 1 is a single live group; n = 16384 + 3 is the second pass of the
triple loop (the grid caps at 4096 blocks of 4 triples) with a partly dead last pass.  Nine attribute rows: the row atomics
collide.

Tolerance of `flat`: the largest |device - oracle| over all forward cases of this file, measured on the code before the
kernel was split into four, is FLAT_ERR_MEASURED = 1.138e-07 (the fast tanh dominates it); the bound is 4 x that.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import attr_cnn_oracle as ao
from oracle import multike_oracle as mo

pytestmark = pytest.mark.gpu

N_ATTR, N_LIT = 9, 50
FLAT_ERR_MEASURED = 1.138e-07   # dim 33, n = 16387, attr_normalize = 0; every other case 7.6e-08 or less
FLAT_ATOL = 4 * FLAT_ERR_MEASURED

FWD_DIMS = (1, 64, 65, 128, 129, 192, 193, 256, 257, 320)
BWD_HALF_DIMS = (1, 32, 33, 64, 65, 96)
BWD_FULL_DIMS = (97, 128, 129, 192, 193, 256, 257, 320)
EXTRA_N = [(33, 1), (129, 1), (33, 16384 + 3), (65, 16384 + 3)]


@functools.lru_cache(maxsize=None)
def _case(dim, n, attr_norm):
    """Inputs (float32) and the oracle's flat / gradients (float64), computed once per (dim, n, attr_norm)."""
    rng = np.random.default_rng(1000 * dim + 7 * (n % 1000) + attr_norm)
    P = ao.init_params(dim, rng)
    P["gamma"] = 1.0 + 0.1 * rng.standard_normal(dim)
    P["beta"] = 0.05 * rng.standard_normal(dim)
    # b2 away from zero: the width normalisation's backward is conditioned like 1 / ||c2||, and at dim 1 (where the exact
    # gradient is 0) ||c2|| = |tanh(pre2)| of a single position — glorot weights on small inputs leave it near 0.01, which
    # turns the float32 rounding of y = c2 / ||c2|| into an error above any fixed absolute bound
    # (consequences: at dim 1 every reference gradient is ~0, so the dim-1 backward cases only show that the device's is
    # small; and no case here runs the normalisation's backward at a small ||c2||)
    P["b1"], P["b2"] = 0.05 * rng.standard_normal(2), 0.5 + 0.05 * rng.standard_normal(2)
    P = {k: v.astype(np.float32) for k, v in P.items()}
    attr = (0.3 * rng.standard_normal((N_ATTR, dim))).astype(np.float32)
    lit = rng.standard_normal((N_LIT, dim)).astype(np.float32)
    lit /= np.linalg.norm(lit, axis=1, keepdims=True)
    ia, iv = rng.integers(0, N_ATTR, n).astype(np.int32), rng.integers(0, N_LIT, n).astype(np.int32)
    dflat = rng.standard_normal((n, 4 * dim)).astype(np.float32)
    p64 = {k: v.astype(np.float64) for k, v in P.items()}
    a64 = attr.astype(np.float64)
    A = mo.l2_normalize_rows(a64) if attr_norm else a64
    _, c = ao.forward(p64, np.zeros((n, dim)), A[ia], lit.astype(np.float64)[iv])
    g = ao.conv_backward(p64, c, dflat.astype(np.float64))
    g_attr = np.zeros_like(a64)
    np.add.at(g_attr, ia, g.pop("as"))   # w.r.t. the (normalised) rows the kernel read: the view's Jacobian is the update's
    packed = np.concatenate([P[k].ravel() for k in ("gamma", "beta", "K1", "b1", "K2", "b2")])
    g_packed = np.concatenate([g[k].ravel() for k in ("gamma", "beta", "K1", "b1", "K2", "b2")])
    for a in (packed, attr, lit, ia, iv, dflat, c["flat"], g_packed, g_attr):
        a.setflags(write=False)
    return dict(params=packed, attr=attr, lit=lit, ia=ia, iv=iv, dflat=dflat, flat=c["flat"], g_params=g_packed, g_attr=g_attr)


def _dev(a):
    return torch.tensor(a, device="cuda")   # a copy: the cached reference arrays stay read-only


def _grad_close(got, ref, what):
    np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=what)


@pytest.mark.parametrize("attr_norm", [1, 0])
@pytest.mark.parametrize("dim,n", [(d, 37) for d in FWD_DIMS] + EXTRA_N)
def test_forward_flat_vs_oracle(dim, n, attr_norm):
    from multike_amd import _lib
    c = _case(dim, n, attr_norm)
    flat = torch.full((n, 4 * dim), float("nan"), dtype=torch.float32, device="cuda")
    _lib.attr_conv_fwd(_dev(c["attr"]), attr_norm, _dev(c["lit"]), dim, _dev(c["ia"]), _dev(c["iv"]), _dev(c["params"]), flat)
    err = float(np.abs(flat.cpu().numpy().astype(np.float64) - c["flat"]).max())
    print(f"flat: dim={dim} n={n} attr_normalize={attr_norm} max error {err:.3e}")
    assert err <= FLAT_ATOL, (dim, n, attr_norm, err)


def _backward(c, dim, attr_norm, workspace, with_attr=True):
    from multike_amd import _lib
    n = len(c["ia"])
    gp = torch.zeros(2 * dim + 52, dtype=torch.float32, device="cuda")
    ga = torch.zeros(N_ATTR, dim, dtype=torch.float32, device="cuda") if with_attr else None
    touched = torch.zeros(N_ATTR, dtype=torch.int32, device="cuda") if with_attr else None
    ws = torch.zeros(_lib.cnn_workspace_floats(dim), dtype=torch.float32, device="cuda") if workspace else None
    _lib.attr_conv_bwd(_dev(c["attr"]), attr_norm, _dev(c["lit"]), dim, _dev(c["ia"]), _dev(c["iv"]), _dev(c["params"]),
                       _dev(c["dflat"]), gp, ga, touched, 5, ws)
    torch.cuda.synchronize()
    if workspace:
        assert float(ws.abs().max()) == 0.0   # zero-invariant: the fold clears what the blocks added
    _grad_close(gp.cpu().numpy(), c["g_params"], f"grad_params dim={dim} n={n}")
    if with_attr:
        _grad_close(ga.cpu().numpy(), c["g_attr"], f"grad_attr dim={dim} n={n}")
        want = np.zeros(N_ATTR, np.int32)
        want[np.unique(c["ia"])] = 5
        assert np.array_equal(touched.cpu().numpy(), want)


@pytest.mark.parametrize("workspace", [True, False])
@pytest.mark.parametrize("attr_norm", [1, 0])
@pytest.mark.parametrize("dim,n", [(d, 37) for d in BWD_HALF_DIMS + BWD_FULL_DIMS] + EXTRA_N)
def test_backward_gradients_vs_oracle(dim, n, attr_norm, workspace):
    _backward(_case(dim, n, attr_norm), dim, attr_norm, workspace)


@pytest.mark.parametrize("dim", [33, 129])
def test_backward_without_an_attribute_gradient(dim):
    """grad_attr = NULL: the parameter gradients alone (no row atomics, no touched marks)."""
    _backward(_case(dim, 37, 0), dim, 0, workspace=True, with_attr=False)

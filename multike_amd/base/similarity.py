"""base/similarity.py surface of the reference (code/base/similarity.py:9-81): `sim`, `csls_sim`, `calculate_nearest_k`, with
the reference's positional signatures.  They return the n1 x n2 matrix, as the reference's do — that is their contract — so
they are meant for small inputs; the evaluator itself (base.alignment.greedy_alignment with metric / csls_k) never builds it.

NumPy arrays are handled on the host as the reference does (float32 matrix; euclidean and unnormalised cosine through float64,
rounded to float32).  Device tensors go through the package's kernels: the products are the f32 MFMA chains of
`mke_sim_sample`, the k nearest are selected by `mke_topk_long` (no sort)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .alignment import _check_metric, _kpad_for, _padded, _unit


def _device_products(a, b):
    """a . b^T on the device through mke_sim_sample (rows padded to a supported width)."""
    kpad = _kpad_for(a.shape[1], f"sim: rows of {a.shape[1]} floats exceed MKE_MAX_STRIDE")
    return _lib.sim_sample(_padded(a, kpad, a.device), kpad, 0, a.shape[0], _padded(b, kpad, a.device))


def sim(embed1, embed2, metric='inner', normalize=False, csls_k=0, sinkhorn=None):
    """code/base/similarity.py:9-53: the n1 x n2 similarity matrix (float32) under `metric`, CSLS re-scored when csls_k > 0,
    Sinkhorn re-scored with sinkhorn = (iters, tau) (one or the other).  sinkhorn = (iters, tau, cut) is refused: the matrix is
    all here, and the support of the candidate lists belongs to the matrix-free decoders of base.alignment."""
    _check_metric(metric, "sim", "")
    if sinkhorn is not None and len(sinkhorn) != 2:
        raise _lib.MultiKEHipError("sim: sinkhorn=(iters, tau, cut) is the matrix-free decoders' sparse re-scoring (base.alignment); "
                                   "the similarity matrix is re-scored densely: pass sinkhorn=(iters, tau)")
    if sinkhorn is not None and csls_k > 0:
        raise _lib.MultiKEHipError("sim: sinkhorn and csls_k are both set: choose one re-scoring")
    if isinstance(embed1, torch.Tensor) or isinstance(embed2, torch.Tensor):
        dev = embed1.device if isinstance(embed1, torch.Tensor) else embed2.device
        a = torch.as_tensor(embed1, device=dev).float()
        b = torch.as_tensor(embed2, device=dev).float()
        if normalize or metric == "cosine":
            a, b = _unit(a), _unit(b)
        dot = _device_products(a, b)
        if metric == "euclidean":
            sq_a, sq_b = (a * a).sum(1), (b * b).sum(1)
            mat = 1.0 - torch.sqrt(torch.clamp_min(sq_a[:, None] + sq_b[None, :] - 2.0 * dot, 0.0))
        else:
            mat = dot
    else:
        a, b = np.asarray(embed1), np.asarray(embed2)
        if normalize:
            a, b = _unit(a), _unit(b)
        if metric == "inner" or (metric == "cosine" and normalize):
            mat = np.matmul(a, b.T)
        elif metric == "euclidean":       # 1 - euclidean_distances: |a|^2 - 2 a.b + |b|^2 in float64
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            d2 = (a64 * a64).sum(1)[:, None] - 2.0 * (a64 @ b64.T) + (b64 * b64).sum(1)[None, :]
            mat = (1.0 - np.sqrt(np.maximum(d2, 0.0))).astype(np.float32)
        else:                             # 1 - cdist(cosine) in float64
            a64, b64 = _unit(a.astype(np.float64)), _unit(b.astype(np.float64))
            mat = (a64 @ b64.T).astype(np.float32)
    if csls_k > 0:
        mat = csls_sim(mat, csls_k)
    if sinkhorn is not None:
        mat = sinkhorn_sim(mat, *sinkhorn)
    return mat


def sinkhorn_potentials(sim_mat, iters, tau):
    """(a [n1], b [n2]) in float64: a = b = 0, then `iters` times a_i = tau log sum_j exp((s_ij - b_j) / tau) followed by
    b_j = tau log sum_i exp((s_ij - a_i) / tau) (the maximum taken out of every sum)."""
    if int(iters) != iters or iters < 1 or not tau > 0 or not np.isfinite(tau):
        raise _lib.MultiKEHipError(f"sinkhorn_sim: need iters >= 1 and a finite tau > 0, got ({iters}, {tau})")
    if isinstance(sim_mat, torch.Tensor):
        s = sim_mat.double()
        a, b = torch.zeros(s.shape[0], dtype=torch.float64, device=s.device), torch.zeros(s.shape[1], dtype=torch.float64, device=s.device)
        for _ in range(int(iters)):
            a = tau * torch.logsumexp((s - b[None, :]) / tau, dim=1)
            b = tau * torch.logsumexp((s - a[:, None]) / tau, dim=0)
        return a, b
    s = np.asarray(sim_mat, dtype=np.float64)
    a, b = np.zeros(s.shape[0]), np.zeros(s.shape[1])

    def lse(x, axis):
        m = x.max(axis=axis, keepdims=True)
        return np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis))

    for _ in range(int(iters)):
        a = tau * lse((s - b[None, :]) / tau, 1)
        b = tau * lse((s - a[:, None]) / tau, 0)
    return a, b


def sinkhorn_sim(sim_mat, iters, tau):
    """s_ij - a_i - b_j (float32) with the potentials of `iters` Sinkhorn iterations at temperature tau: tau log of the matrix
    exp(S / tau) after `iters` rounds of row normalisation followed by column normalisation.  Computed in float64."""
    a, b = sinkhorn_potentials(sim_mat, iters, tau)
    if isinstance(sim_mat, torch.Tensor):
        return ((sim_mat.double() - a[:, None]) - b[None, :]).float()
    return ((np.asarray(sim_mat, dtype=np.float64) - a[:, None]) - b[None, :]).astype(np.float32)


def csls_sim(sim_mat, k):
    """code/base/similarity.py:56-75: (2 sim - r_T[:, None]) - r_S[None, :]."""
    nearest_values1 = calculate_nearest_k(sim_mat, k)
    nearest_values2 = calculate_nearest_k(sim_mat.T, k)
    return (2 * sim_mat - nearest_values1[:, None]) - nearest_values2[None, :]


def calculate_nearest_k(sim_mat, k):
    """code/base/similarity.py:78-81: per row the mean of the k largest values (1 <= k <= columns - 2)."""
    n = sim_mat.shape[1]
    if not 1 <= k <= n - 2:
        raise _lib.MultiKEHipError(f"calculate_nearest_k: need 1 <= k <= {n - 2} (k = {k})")
    if isinstance(sim_mat, torch.Tensor):
        m = sim_mat.float().contiguous()
        idx = _lib.topk_long(m, k)
        vals = torch.gather(m, 1, idx.long())
        return vals.double().sum(1).div(k).float()
    sorted_mat = -np.partition(-sim_mat, k + 1, axis=1)
    return np.mean(sorted_mat[:, 0:k], axis=1)

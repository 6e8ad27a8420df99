"""Float64 oracle of the Sinkhorn re-scoring (include/multike_hip.h (9d)) and the error bound its tests hold the device to.
NumPy only (the log-sum-exp takes the maximum out, as scipy.special.logsumexp does).

Definition.  S [n1, n2], temperature tau > 0, L >= 1 iterations, a = 0 [n1], b = 0 [n2]; per iteration, rows then columns:
    a_i = tau log sum_j exp((s_ij - b_j) / tau)        b_j = tau log sum_i exp((s_ij - a_i) / tau)
scores = s_ij - a_i - b_j = tau log of the Sinkhorn matrix (L row normalisations each followed by a column normalisation of
exp(S / tau)): after the last column pass every column of exp(scores / tau) sums to 1.

Bound of ONE mke_align_lse call over n columns, M = max|S| + max|sub_b|:
    bound(tau, n, M) = tau (n + 8) 2^-23 + 6 * 2^-24 M
The first term: one v_exp_f32 ulp per term plus the rounding of a sequential f32 sum of n positive terms (relative error
n 2^-24 of the sum, i.e. tau n 2^-24 of tau log sum, doubled for the exp ulps and the rescalings of the running sum).  The
second: the f32 roundings of s - b, of the product with 1 / tau, of 1 / tau itself and of m + log s, each relative 2^-24 of a
quantity bounded by M (or M / tau, multiplied back by tau).  Log-sum-exp is 1-Lipschitz in the sup norm, so an error eps in
sub_b moves the output by at most eps: after L iterations (2 L calls) a potential is within 2 L bound of the oracle's.
"""
from __future__ import annotations

import numpy as np


def logsumexp(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def lse(S, sub_b, tau):
    """tau log sum_j exp((S_ij - sub_b[j]) / tau) per row, float64."""
    S = np.asarray(S, dtype=np.float64)
    sub = np.zeros(S.shape[1]) if sub_b is None else np.asarray(sub_b, dtype=np.float64)
    return tau * logsumexp((S - sub[None, :]) / tau, 1)


def potentials(S, iters, tau):
    """(a [n1], b [n2]) float64 after `iters` iterations."""
    S = np.asarray(S, dtype=np.float64)
    a, b = np.zeros(S.shape[0]), np.zeros(S.shape[1])
    for _ in range(int(iters)):
        a = lse(S, b, tau)
        b = lse(S.T, a, tau)
    return a, b


def scores(S, a, b):
    return (np.asarray(S, dtype=np.float64) - a[:, None]) - b[None, :]


def bound(tau, n, M):
    return tau * (n + 8) * 2.0 ** -23 + 6.0 * 2.0 ** -24 * M


def potentials_bound(S, a, b, iters, tau):
    """2 L bound with n the longer side and M = max|S| + the largest potential."""
    M = float(np.abs(S).max() + max(np.abs(a).max(), np.abs(b).max()))
    return 2 * int(iters) * bound(tau, max(S.shape), M)


def rank_oracle(R):
    """(greater, ties, best column, per-row gap to the nearest other column) of a re-scored matrix, gold column = row index."""
    n = R.shape[0]
    idx = np.arange(n)
    gold = R[idx, idx]
    greater = (R > gold[:, None]).sum(1).astype(np.int64)
    ties = (R == gold[:, None]).sum(1).astype(np.int64)
    dist = np.abs(R - gold[:, None])
    dist[idx, idx] = np.inf
    return greater, ties, np.argmax(R, axis=1).astype(np.int64), dist.min(1)


def metrics(greater, top_k):
    """Hits@k (percent), MR, MRR of tie-free ranks, as code/base/alignment.py:141-163 counts them."""
    g = np.asarray(greater, dtype=np.float64)
    return np.array([np.mean(g < k) * 100 for k in top_k]), float(np.mean(g + 1)), float(np.mean(1.0 / (g + 1)))

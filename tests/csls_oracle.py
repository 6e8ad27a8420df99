"""Float64 oracle of the CSLS evaluator (code/base/similarity.py:9-81 + the rank of code/base/alignment.py:141-163): the
similarity matrix, the exact top-k means r_T / r_S, the CSLS matrix and the gold's greater / tie counts, all in float64 on
the host.  Small inputs only: it builds the matrix."""
import numpy as np


def unit(x):
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.where(n == 0, 1.0, n)


def sim64(e1, e2, metric="inner", normalize=True):
    a, b = np.asarray(e1, np.float64), np.asarray(e2, np.float64)
    if normalize or metric == "cosine":
        a, b = unit(a), unit(b)
    if metric == "euclidean":
        d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
        return 1.0 - np.sqrt(np.maximum(d2, 0.0))
    return a @ b.T


def topk_mean(mat, k):
    """Exact top-k multiset per row, summed in descending order."""
    return -np.sort(-mat, axis=1)[:, :k].sum(1) / k


def csls64(e1, e2, metric="inner", normalize=True, k=10):
    s = sim64(e1, e2, metric, normalize)
    r_t, r_s = topk_mean(s, k), topk_mean(s.T, k)
    return (2.0 * s - r_t[:, None]) - r_s[None, :], r_t, r_s


def counts(mat):
    n1 = mat.shape[0]
    gold = mat[np.arange(n1), np.arange(n1)]
    return (mat > gold[:, None]).sum(1), (mat == gold[:, None]).sum(1)

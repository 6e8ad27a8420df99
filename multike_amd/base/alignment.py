"""base/alignment.py surface of the reference (code/base/alignment.py:8-79): `greedy_alignment` — Hits@k / MR / MRR of
the gold counterpart under the (normalised) inner-product similarity — on the f32 matrix cores via `mke_align_rank`; the
euclidean metric and CSLS re-scoring via `mke_align_topk_mean` + `mke_align_rank_ex`; `stable_alignment` (:82-128) — the
one-to-one Gale-Shapley matching — via `mke_stable_lists` + `mke_stable_rounds` + `mke_stable_finish`; Sinkhorn re-scoring
(`sinkhorn=(iters, tau)`, the soft one-to-one decoder) via `mke_align_lse`, whose potentials ride the CSLS plumbing;
`sinkhorn=(iters, tau, cut)` iterates them on the support of both sides' `cut` best candidates instead (`mke_sparse_support` +
`mke_sparse_lse` of libmultike_sparse.so: two list sweeps, then no sweep per iteration).
`mutual_pairs` / `mutual_alignment` (no counterpart in the reference) — the pairs that are each other's best, with precision /
recall / F1 — via `mke_align_mutual` + `mke_mutual_pairs`: one sweep folds every similarity into both directions.
`assignment_matching` / `assignment_alignment` (no counterpart either) — the one-to-one pairing that maximises the total
similarity over the stable matching's candidate lists, by a parallel auction — via `mke_assign_rounds` + `mke_assign_finish`.
The n1 x n2 similarity matrix is never materialised (the reference holds 60K x 60K fp32 = 14 GB and argsorts its rows
in `nums_threads` worker processes)."""
from __future__ import annotations

import time

import numpy as np
import torch

from .. import _lib


SUPPORTED_METRICS = ("inner", "cosine", "euclidean")


def _unit(x):
    """sklearn.preprocessing.normalize of a tensor or an array: zero rows stay zero (code/base/similarity.py:30-32)."""
    if isinstance(x, torch.Tensor):
        n = torch.linalg.norm(x, dim=1, keepdim=True)
        return x / torch.where(n == 0, torch.ones_like(n), n)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.where(n == 0, 1, n).astype(x.dtype)


def _prep(x, device, normalize):
    t = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(device) if not isinstance(x, torch.Tensor) else x.to(device).float()
    return _unit(t) if normalize else t


def _check_metric(metric, who="greedy_alignment", why="; the other cdist metrics are not GEMM-shaped"):
    if metric not in SUPPORTED_METRICS:
        raise _lib.MultiKEHipError(f"{who}: metric {metric!r} is not built (supported: 'inner', 'cosine', 'euclidean'{why})")


def _kpad_for(d, too_wide=None):
    """The narrowest supported row width >= d (MKE_MAX_STRIDE is the widest: there is no second backend)."""
    if d > _lib.SIM_SELECT_KPADS[-1]:
        raise _lib.MultiKEHipError(too_wide or f"greedy_alignment: rows of {d} floats exceed the widest k_align_rank instantiation "
                                   f"({_lib.SIM_SELECT_KPADS[-1]} = MKE_MAX_STRIDE)")
    return min(x for x in _lib.SIM_SELECT_KPADS if x >= d)


def _padded(x, kpad, device):
    n, d = x.shape
    p = torch.zeros(n, kpad, dtype=torch.float32, device=device)
    p[:, :d] = x
    return p


def prepare_operands(embed1, embed2, metric="inner", normalize=True, device="cuda"):
    """(a, b, kpad, metric code, sq_a, sq_b): the zero-padded f32 operands of the native evaluator.  'cosine' is the inner
    product of unit rows (code/base/similarity.py:34-44: normalised or not, cosine similarity is that); 'euclidean' hands the
    squared row norms over (1 - euclidean_distances, :38-41)."""
    _check_metric(metric)
    a, b = _prep(embed1, device, normalize or metric == "cosine"), _prep(embed2, device, normalize or metric == "cosine")
    kpad = _kpad_for(a.shape[1])
    ap, bp = _padded(a, kpad, device), _padded(b, kpad, device)
    if metric == "euclidean":
        return ap, bp, kpad, _lib.METRIC_EUCLIDEAN, (a * a).sum(1).contiguous(), (b * b).sum(1).contiguous()
    return ap, bp, kpad, _lib.METRIC_INNER, None, None


def csls_means(a, b, kpad, metric_code, sq_a, sq_b, csls_k):
    """(r_T [n1], r_S [n2]) of code/base/similarity.py:69-70 from padded operands: r_T(i) = mean of row i's k largest
    similarities to the n2 targets, r_S(j) = mean of column j's k largest similarities to the n1 sources."""
    r_t = _lib.align_topk_mean(a, b, kpad, csls_k, metric_code, sq_a, sq_b)
    r_s = _lib.align_topk_mean(b, a, kpad, csls_k, metric_code, sq_b, sq_a)
    return r_t, r_s


def _check_rescoring(csls_k, sinkhorn, csls=None):
    """(csls_k as an int, 0 = none; (iters, tau) or (iters, tau, cut) of a `sinkhorn=` argument, or None).  Sinkhorn and CSLS are
    two re-scorings of one similarity, not a chain.  csls_k is truncated first, as greedy_alignment and stable_alignment always
    did: None, a negative or a fraction below 1 is no CSLS.  A third element `cut` >= 1 asks for the potentials on the support
    of the `cut`-long candidate lists (sparse_sinkhorn_potentials); it is clamped to each side's size where the lists are made."""
    csls_k = max(int(csls_k or 0), 0)
    if sinkhorn is None:
        return csls_k, None
    if len(sinkhorn) == 3:
        iters, tau, cut = sinkhorn
    else:
        (iters, tau), cut = sinkhorn, None
    if csls_k > 0 or csls is not None:
        raise _lib.MultiKEHipError("sinkhorn and csls_k are both set: choose one re-scoring")
    if int(iters) != iters or int(iters) < 1 or not (float(tau) > 0.0) or not np.isfinite(float(tau)):
        raise _lib.MultiKEHipError(f"sinkhorn=(iters, tau) needs iters >= 1 and a finite tau > 0, got ({iters}, {tau})")
    if cut is None:
        return csls_k, (int(iters), float(tau))
    if int(cut) != cut or int(cut) < 1:
        raise _lib.MultiKEHipError(f"sinkhorn=(iters, tau, cut) needs a whole cut >= 1, got {cut}")
    return csls_k, (int(iters), float(tau), int(cut))


def sinkhorn_potentials(a, b, kpad, metric_code, sq_a, sq_b, iters, tau):
    """(a-potential [n1], b-potential [n2]) after `iters` Sinkhorn iterations at temperature tau from padded operands, in
    similarity units: a_i = tau log sum_j exp((s_ij - b_j) / tau), then b_j = tau log sum_i exp((s_ij - a_i) / tau), b starting
    at zero — 2 * iters calls of mke_align_lse, no matrix."""
    pa, pb = None, None
    for _ in range(int(iters)):
        pa = _lib.align_lse(a, b, kpad, tau, metric_code, sq_a, sq_b, pb)
        pb = _lib.align_lse(b, a, kpad, tau, metric_code, sq_b, sq_a, pa)
    return pa, pb


def sinkhorn_terms(a, b, kpad, metric_code, sq_a, sq_b, iters, tau):
    """(r_t, r_s) = (2 a-potential, 2 b-potential): as `csls_row` / `csls_col` of the rank and list kernels they turn
    (2 s - r_t[i]) - r_s[j] into 2 (s - a_i - b_j), twice tau log of the Sinkhorn matrix (the doubling is exact in f32)."""
    pa, pb = sinkhorn_potentials(a, b, kpad, metric_code, sq_a, sq_b, iters, tau)
    return 2.0 * pa, 2.0 * pb


def sparse_support(operands, cut):
    """The support of the sparse Sinkhorn re-scoring from prepare_operands' tuple: every pair (i, j) in which j is among row
    i's `cut` best columns or i among column j's `cut` best rows under the plain metric (`cut` clamped to each side's size),
    as a _lib.SparseSupport on the device — two list sweeps (candidate_lists without re-scoring, flagged rows redone as there)
    and mke_sparse_support; a pair both lists name is one entry with the row list's value."""
    a, b, kpad, code, sq_a, sq_b = operands
    n1, n2 = a.shape[0], b.shape[0]
    cut_r, cut_c = max(1, min(int(cut), n2)), max(1, min(int(cut), n1))
    dev = a.device
    empty = lambda n, c: (torch.full((n, c), float("-inf"), dtype=torch.float32, device=dev), torch.full((n, c), -1, dtype=torch.int32, device=dev))
    if n1 == 0 or n2 == 0:                                   # no sweep over nothing: every list is padding
        (val_r, col_r), (val_c, row_c) = empty(n1, cut_r), empty(n2, cut_c)
    else:
        val_r, col_r, _ = candidate_lists(a, b, kpad, cut_r, code, sq_a, sq_b)
        val_c, row_c, _ = candidate_lists(b, a, kpad, cut_c, code, sq_b, sq_a)
    return _lib.sparse_support(val_r.contiguous(), col_r.contiguous(), val_c.contiguous(), row_c.contiguous())


def sparse_sinkhorn_potentials(support, iters, tau):
    """(a-potential [n1], b-potential [n2]) of sinkhorn_potentials' recurrence with every sum restricted to the support:
    a_i = tau log sum_{j: (i, j) in support} exp((s_ij - b_j) / tau), then b_j likewise over its column with the a just
    computed, b starting at zero — 2 * iters calls of mke_sparse_lse, no sweep.  An approximation of the dense potentials,
    equal to them at full support."""
    pa, pb = None, None
    for _ in range(int(iters)):
        pa = _lib.sparse_lse(support, False, tau, pb)
        pb = _lib.sparse_lse(support, True, tau, pa)
    return pa, pb


def sparse_sinkhorn_terms(operands, iters, tau, cut):
    """(r_t, r_s) = twice the sparse potentials, for `csls_row` / `csls_col` of the rank, list and mutual kernels as
    sinkhorn_terms' are."""
    pa, pb = sparse_sinkhorn_potentials(sparse_support(operands, cut), iters, tau)
    return 2.0 * pa, 2.0 * pb


def _rescoring_terms(operands, csls_k, sinkhorn):
    """(row_term [n1], col_term [n2]) of the re-scoring (2 s - row_term[i]) - col_term[j] from prepare_operands' tuple and the
    checked (csls_k, sinkhorn): the CSLS means, or twice the Sinkhorn potentials — dense for (iters, tau), on the lists'
    support for (iters, tau, cut); None when there is no re-scoring."""
    if sinkhorn is not None and len(sinkhorn) == 3:
        return sparse_sinkhorn_terms(operands, *sinkhorn)
    if sinkhorn is not None:
        return sinkhorn_terms(*operands, *sinkhorn)
    return csls_means(*operands, csls_k) if csls_k > 0 else None


def alignment_counts(embed1, embed2, normalize=True, device="cuda", metric="inner", csls_k=0, csls=None, *, sinkhorn=None):
    """(greater [n1] int64, ties [n1] int64, best [n1] int64): greater_i = #{j: sim_ij > sim_ii}, ties_i = #{j: sim_ij ==
    sim_ii} (the gold column included, so >= 1), best_i = argmax_j sim_ij.  `metric` 'inner' / 'cosine' / 'euclidean';
    csls_k > 0 re-scores every similarity by CSLS (code/base/similarity.py:56-75).  `csls` = (r_T, r_S) given by the caller
    (the sharded driver, which computes them over all ranks) in place of computing them here.  `sinkhorn` = (iters, tau)
    re-scores by Sinkhorn normalisation instead (not together with CSLS).  The plain inner product of the rows as they are
    prepared goes through mke_align_rank, everything else through mke_align_rank_ex: one kernel, two rules for a row whose
    similarities are all NaN or -inf (mke_eval.hip)."""
    _check_metric(metric)
    csls_k, sinkhorn = _check_rescoring(csls_k, sinkhorn, csls)
    if len(embed2) < len(embed1):                          # before anything is copied, padded or refused for its width
        raise _lib.MultiKEHipError("greedy_alignment: gold column = row index needs len(embed2) >= len(embed1)")
    operands = prepare_operands(embed1, embed2, metric, normalize, device)
    a, b, kpad, code, sq1, sq2 = operands
    n1, n2 = a.shape[0], b.shape[0]
    terms = csls if csls is not None else _rescoring_terms(operands, csls_k, sinkhorn)
    rank = torch.zeros(n1, dtype=torch.int32, device=device)
    ties = torch.zeros(n1, dtype=torch.int32, device=device)
    best = torch.zeros(n1, dtype=torch.int64, device=device)
    if terms is None and (metric == "inner" or (metric == "cosine" and normalize)):
        _lib.align_rank(a, b, kpad, n1, n2, rank, best, ties)
    else:
        _lib.align_rank_ex(a, b, kpad, rank, ties, best, code, sq1, sq2, *(terms or (None, None)))
    col = 0xFFFFFFFF - (best & 0xFFFFFFFF)
    return rank.long(), ties.long().clamp_min(1), col


def alignment_ranks(embed1, embed2, normalize=True, device="cuda", metric="inner", csls_k=0, *, sinkhorn=None):
    """(rank [n1] float64, best [n1] int64): rank_i = greater_i + (ties_i - 1) / 2 — the gold's EXPECTED 0-based position when
    the columns that tie with it are ordered at random.  The reference's argsort / argpartition leaves the gold at an arbitrary
    position among them (code/base/alignment.py:152-160).  Without ties this is the reference's rank exactly."""
    greater, ties, col = alignment_counts(embed1, embed2, normalize, device, metric=metric, csls_k=csls_k, sinkhorn=sinkhorn)
    return greater.double() + (ties.double() - 1.0) * 0.5, col


def tie_aware_metrics(greater, ties, top_k):
    """Expected Hits@k counts / MR / MRR over a uniformly random order of the columns tied with the gold: the gold's position
    is uniform on [greater, greater + ties - 1], so P(position < k) = clamp((k - greater) / ties, 0, 1) — a gold tied with one
    other column is HALF a Hits@1, not a whole one (a threshold on the mid-rank 0.5 < 1 would count it fully) — E[position + 1]
    = greater + (ties + 1) / 2, E[1 / (position + 1)] = (H(greater + ties) - H(greater)) / ties.  Degenerate inputs (a zero
    name vector ties with every column; duplicated embeddings) therefore score their chance level.  Without ties
    (ties == 1) these are exactly the reference's integer counts (code/base/alignment.py:141-163)."""
    g, t = greater.double(), ties.double()
    ks = torch.as_tensor([float(k) for k in top_k], dtype=torch.float64, device=g.device)
    hits = ((ks[:, None] - g[None, :]) / t[None, :]).clamp(0.0, 1.0).sum(1)
    mr = (g + (t + 1.0) * 0.5).mean()
    rr = 1.0 / (g + 1.0)                                                  # ties == 1: the reference's 1 / (rank + 1) exactly
    tied = ties > 1
    out = torch.cat([hits, mr[None], rr.sum()[None], tied.sum()[None].double()]).cpu().tolist()   # one read-back for all of them
    mrr_sum = out[-2]
    if out[-1] > 0:       # rows whose gold ties with other columns (degenerate inputs): harmonic-number difference, those rows only
        gt, tt = g[tied], t[tied]
        mrr_sum += float(((_harmonic(gt + tt) - _harmonic(gt)) / tt - rr[tied]).sum())
    return out[:-3], out[-3], mrr_sum / max(g.numel(), 1)


_EULER_GAMMA = 0.57721566490153286


def _harmonic(n):
    """H(n) = sum_{j=1..n} 1/j for a float64 tensor of non-negative integers: exact partial sums below 32, the asymptotic series
    ln n + gamma + 1/(2n) - 1/(12 n^2) + 1/(120 n^4) above (next term 1/(252 n^6) < 4e-12).  In place of
    torch.special.digamma(n + 1) + gamma, which this PyTorch build compiles at its first use in a process (0.1-1.7 s on a fresh box)."""
    table = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.float64), 1.0 / torch.arange(1, 32, dtype=torch.float64)]), 0).to(n.device)
    small = n < 32
    m = torch.where(small, torch.full_like(n, 32.0), n)
    i2 = 1.0 / (m * m)
    big = torch.log(m) + _EULER_GAMMA + 0.5 / m - i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0))
    return torch.where(small, table[torch.where(small, n, torch.zeros_like(n)).long()], big)


def greedy_alignment(embed1, embed2, top_k, nums_threads, metric, normalize, csls_k, accurate, want_pairs=True, *, sinkhorn=None):
    """code/base/alignment.py:8-79.  Returns (alignment_rest, hits1, mr, mrr).  `nums_threads` is accepted and ignored
    (one kernel launch; five with CSLS).  Metrics: 'inner', 'cosine' (== inner product of normalised rows), 'euclidean';
    csls_k > 0 re-scores by CSLS (code/base/similarity.py:56-75); the other cdist metrics raise.  want_pairs = False (base.evaluation.valid, which drops them): alignment_rest is None — the set of (row, best
    column) tuples is a Python object per row.  sinkhorn = (iters, tau) re-scores by Sinkhorn normalisation (2 * iters sweeps)
    instead of CSLS; both together raise."""
    _check_metric(metric)
    csls_k, sinkhorn = _check_rescoring(csls_k, sinkhorn)
    assert 1 in top_k
    t = time.time()
    greater, ties, best = alignment_counts(embed1, embed2, normalize, metric=metric, csls_k=csls_k, sinkhorn=sinkhorn)
    num = greater.numel()
    hits, mr, mrr = tie_aware_metrics(greater, ties, top_k)
    hits = np.round(np.array(hits) / num * 100, 3)
    alignment_rest = set(zip(range(num), best.cpu().tolist())) if want_pairs else None
    cost = time.time() - t
    print_results(top_k, hits, mr, mrr, cost, accurate, csls_k, sinkhorn)
    return alignment_rest, hits[0], mr, mrr


STABLE_ROUND_BATCH = 32      # rounds enqueued between two reads of the proposal counter


def candidate_lists(a, b, kpad, cut, metric_code=_lib.METRIC_INNER, sq_a=None, sq_b=None, csls=None, sim_mat=None, sample_cols=0):
    """(val float32 [n1, cut], col int32 [n1, cut], redone): per row its `cut` best columns under the re-scored similarity,
    value descending then column ascending, short lists padded with column -1 (what code/base/alignment.py:131-138 `arg_sort`
    keeps of a row that `galeshapley(.., cut)` can ever look at).  Rows the sweep path flagged (threshold estimate too tight,
    or a candidate segment overflowed) are redone here through the whole-row path; `redone` is how many."""
    r_t, r_s = csls if csls is not None else (None, None)
    if sim_mat is not None:
        val, col, _ = _lib.stable_lists(None, None, 0, cut, sim_mat=sim_mat)
        return val, col, 0
    val, col, flags = _lib.stable_lists(a, b, kpad, cut, metric_code, sq_a, sq_b, r_t, r_s, sample_cols=sample_cols)
    idx = torch.nonzero(flags, as_tuple=False).flatten()      # one read-back: the rows to redo (usually none)
    if idx.numel():
        pick = lambda t: None if t is None else t[idx].contiguous()
        v2, c2, _ = _lib.stable_lists(a[idx].contiguous(), b, kpad, cut, metric_code, pick(sq_a), sq_b, pick(r_t), r_s,
                                      whole_rows=True)
        val[idx], col[idx] = v2, c2
    return val, col, int(idx.numel())


def stable_matching(val, col, n2, batch=STABLE_ROUND_BATCH):
    """(match int32 [n1] on the device, matched, matched golds, rounds): deferred acceptance to its fixed point over the lists
    (code/base/alignment.py:166-219 `galeshapley` without its round limit): suitors = rows, reviewers = the n2 columns."""
    n1, dev = col.shape[0], col.device
    ptr = torch.zeros(n1, dtype=torch.int32, device=dev)
    holder = torch.zeros(n2, dtype=torch.int64, device=dev)
    proposals = torch.zeros(1024, dtype=torch.int32, device=dev)
    match = torch.empty(n1, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    rounds = 0
    while n1 > 0:
        if rounds + batch > proposals.numel():                # a chain longer than the counter array: extend it
            proposals = torch.cat([proposals, torch.zeros_like(proposals)])
        args = _lib.stable_match_args(val, col, n2, ptr, holder, proposals)
        _lib.stable_rounds(args, rounds, batch)
        rounds += batch
        if int(proposals[rounds - 1]) == 0:                   # the only synchronisation: one int per batch of rounds
            break
    _lib.stable_finish(_lib.stable_match_args(val, col, n2, ptr, holder, proposals, match, counts))
    matched, gold = (int(x) for x in counts.cpu().tolist())
    used = int((proposals[:max(rounds, 1)] > 0).sum()) if n1 > 0 else 0
    return match, matched, gold, used


def stable_alignment(embed1, embed2, metric, normalize, csls_k, nums_threads, cut=100, sim_mat=None, *, sinkhorn=None):
    """code/base/alignment.py:82-128.  Returns (match, precision): match int64 [n1] on the host, match[i] = the row of embed2
    matched to row i of embed1 or -1 (the reference returns None); precision = matched golds / matched suitors * 100 (:123-128).
    The result is the suitor-optimal stable matching with every suitor's list truncated to its `cut` best columns, run to its
    fixed point — the reference's result whenever its galeshapley matches every suitor within `cut` rounds.  Ties: a suitor
    prefers the lower column, a reviewer the lower row.  `nums_threads` is accepted and ignored.  `sim_mat`: a float32
    [n1, n2] similarity matrix on the device given by the caller, used in place of sim(embed1, embed2, ...).  `sinkhorn` =
    (iters, tau): the lists are taken under the Sinkhorn re-scored similarity (not with csls_k, not with sim_mat)."""
    _check_metric(metric)
    csls_k, sinkhorn = _check_rescoring(csls_k, sinkhorn)
    if sinkhorn is not None and sim_mat is not None:
        raise _lib.MultiKEHipError("stable_alignment: sinkhorn re-scores the embeddings' similarities; a given sim_mat is used as it is")
    t = time.time()
    if sim_mat is not None:
        if not isinstance(sim_mat, torch.Tensor):
            sim_mat = torch.as_tensor(np.asarray(sim_mat), dtype=torch.float32).to("cuda")
        sim_mat = sim_mat.float().contiguous()
        n1, n2 = sim_mat.shape
        val, col, _ = candidate_lists(None, None, 0, max(1, min(int(cut), n2)), sim_mat=sim_mat)
    else:
        operands = prepare_operands(embed1, embed2, metric, normalize, "cuda")
        a, b, kpad, code, sq1, sq2 = operands
        n1, n2 = a.shape[0], b.shape[0]
        val, col, _ = candidate_lists(a, b, kpad, max(1, min(int(cut), n2)), code, sq1, sq2, _rescoring_terms(operands, csls_k, sinkhorn))
    torch.cuda.synchronize()
    print("generating candidate lists costs time {:.3f} s ".format(time.time() - t))
    t = time.time()
    match, matched, gold, _ = stable_matching(val, col, n2)
    match = match.cpu().numpy().astype(np.int64)
    precision = gold / matched * 100 if matched else 0.0
    cost = time.time() - t
    print("stable alignment precision = {:.3f}%, time = {:.3f} s ".format(precision, cost))
    return match, precision


def _best_value(best):
    """float32 values of packed `best` words (ordered(s) << 32 | ...) on the device; a word of 0 (no best) decodes to NaN."""
    u = (best >> 32) & 0xFFFFFFFF
    bits = torch.where((u & 0x80000000) != 0, u & 0x7FFFFFFF, ~u & 0xFFFFFFFF)
    return (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32)       # the 32 bits as a signed word, then as a float


def mutual_pairs(embed1, embed2, metric="inner", normalize=True, csls_k=0, threshold=None, *, sinkhorn=None):
    """The mutual (bidirectional) nearest-neighbour decoder: (match int32 [n1], score float32 [n1]), both on the device.
    match[i] = j when column j is row i's best AND row i is column j's best under the similarity (the lowest index wins a tie
    in both directions), else -1; score[i] = the similarity of row i's best column, matched or not (NaN for a row whose
    similarities are all NaN).  Any n1, n2 and no gold labels: this is the label-free decoder.  csls_k > 0 or sinkhorn = (iters,
    tau) re-score as greedy_alignment does, and then `score` and `threshold` are in units of the RE-SCORED value the decoder
    compares — (2 s - r_T[i]) - r_S[j] for CSLS, 2 (s - a_i - b_j) for Sinkhorn — not of the raw similarity.  `threshold`
    (None = none) keeps the pairs whose value is >= it.  One sweep (mke_align_mutual) decides both directions on one f32 value."""
    _check_metric(metric, "mutual_pairs")
    csls_k, sinkhorn = _check_rescoring(csls_k, sinkhorn)
    if threshold is not None and np.isnan(float(threshold)):
        raise _lib.MultiKEHipError("mutual_pairs: the threshold is NaN (None = no threshold)")
    match, _, row_best = _mutual(embed1, embed2, metric, normalize, csls_k, threshold, sinkhorn)
    return match, _best_value(row_best)


def _mutual(embed1, embed2, metric, normalize, csls_k, threshold, sinkhorn):
    """(match, counts, row_best) of the checked arguments: the operand path of the other decoders, one sweep, one pairing."""
    return _mutual_decode(_mutual_operands(embed1, embed2, metric, normalize, csls_k, sinkhorn), threshold)


def _mutual_operands(embed1, embed2, metric, normalize, csls_k, sinkhorn):
    """prepare_operands' tuple + (the re-scoring terms or None,): everything the mutual sweep reads.  Whoever re-scores single
    pairs of the same decode afterwards (base.bootstrap.edit_links) takes this tuple, not a second preparation."""
    operands = prepare_operands(embed1, embed2, metric, normalize, "cuda")
    a, b = operands[:2]
    terms = _rescoring_terms(operands, csls_k, sinkhorn) if min(a.shape[0], b.shape[0]) > 0 else None
    return operands + (terms,)


def _mutual_decode(operands, threshold):
    """(match, counts, row_best) of _mutual_operands' tuple: one sweep, one pairing."""
    a, b, kpad, code, sq1, sq2, terms = operands
    row_best, col_best = _lib.align_mutual(a, b, kpad, code, sq1, sq2, *(terms or (None, None)))
    match, counts = _lib.mutual_pairs(row_best, col_best, float("-inf") if threshold is None else float(threshold))
    return match, counts, row_best


def mutual_alignment(embed1, embed2, metric, normalize, csls_k, nums_threads, threshold=None, *, sinkhorn=None):
    """Mutual nearest-neighbour alignment against the gold column = row index.  Returns (match, precision, recall, f1): match
    int64 [n1] on the host as mutual_pairs'; precision = gold pairs / matched rows * 100, recall = gold pairs / n1 * 100, f1
    their harmonic mean, all 0.0 when nothing matched.  `threshold` applies to the value the decoder compares (re-scored when
    csls_k or sinkhorn is set, see mutual_pairs).  `nums_threads` is accepted and ignored."""
    _check_metric(metric, "mutual_alignment")
    csls_k, sinkhorn = _check_rescoring(csls_k, sinkhorn)
    if len(embed2) < len(embed1):
        raise _lib.MultiKEHipError("mutual_alignment: gold column = row index needs len(embed2) >= len(embed1)")
    if threshold is not None and np.isnan(float(threshold)):
        raise _lib.MultiKEHipError("mutual_alignment: the threshold is NaN (None = no threshold)")
    t = time.time()
    match, counts, _ = _mutual(embed1, embed2, metric, normalize, csls_k, threshold, sinkhorn)
    matched, gold = (int(x) for x in counts.cpu().tolist())
    match = match.cpu().numpy().astype(np.int64)
    n1 = match.shape[0]
    precision = gold / matched * 100 if matched else 0.0
    recall = gold / n1 * 100 if matched else 0.0
    f1 = 2 * precision * recall / (precision + recall) if gold else 0.0
    cost = time.time() - t
    print("mutual alignment precision = {:.3f}%, recall = {:.3f}%, f1 = {:.3f}%, matched = {}, time = {:.3f} s ".format(
        precision, recall, f1, matched, cost))
    return match, precision, recall, f1


ASSIGN_ROUND_BATCH = 32      # rounds enqueued between two reads of the auction's progress counters (grid form)
ASSIGN_TAIL_FACTOR = 32      # ... times this many once the tail kernel has taken over: a round is then a loop iteration, not two launches
ASSIGN_VALUE_RANGE = 16.0    # (largest listed value - floor) + eps may not exceed this: the f32 form of the guarantee rests on it


def _auction(val, col, n2, eps, floor, batch, max_rounds, tail_cap, flags):
    """The auction to its fixed point -> (state int32 [n1], price float32 [n2], progress int64 [4], kernel launches enqueued);
    the tensors on the device.  One read-back of two counters per batch of rounds, as stable_matching's loop."""
    if flags & ~_lib.ASSIGN_NO_TAIL:
        raise _lib.MultiKEHipError(f"assignment_matching: flags {flags} (0, or {_lib.ASSIGN_NO_TAIL}: no tail kernel)")
    n1, dev = col.shape[0], col.device
    state = torch.zeros(n1, dtype=torch.int32, device=dev)
    price = torch.zeros(n2, dtype=torch.float32, device=dev)
    owner = torch.zeros(n2, dtype=torch.int32, device=dev)
    bid = torch.zeros(n2, dtype=torch.int64, device=dev)
    progress = torch.zeros(4, dtype=torch.int64, device=dev)
    temp = torch.empty(_lib.assign_temp_bytes(n1, n2, tail_cap) // 4, dtype=torch.int32, device=dev)
    cap = 0 if flags & _lib.ASSIGN_NO_TAIL else min(tail_cap or _lib.ASSIGN_TAIL_CAP, _lib.ASSIGN_TAIL_MAX)
    rounds, bidding, launches = 0, n1, 0
    while bidding > 0:
        if rounds >= max_rounds:
            raise _lib.MultiKEHipError(f"assignment_matching: {bidding} rows are still bidding after {rounds} rounds (max_rounds); "
                                       f"eps = {eps} may be too small for these values: the rounds grow like (value range) / eps")
        tail = 0 < bidding <= cap          # the tail kernel has taken over for good: the number of bidding rows never grows
        n = min(batch * ASSIGN_TAIL_FACTOR if tail else batch, max_rounds - rounds)
        args = _lib.assign_args(val, col, n2, eps, floor, state, price, owner, bid, progress, temp, tail_cap,
                                flags | (_lib.ASSIGN_TAIL_ONLY if tail else 0))
        _lib.assign_rounds(args, n)
        launches += (0 if tail else 2 * n) + (1 if cap else 0)
        rounds, bidding = progress[:2].tolist()      # the only synchronisation: two counters per batch of rounds
    return state, price, progress, launches


def assignment_matching(val, col, n2, eps, floor, batch=ASSIGN_ROUND_BATCH, max_rounds=1 << 20, tail_cap=0, flags=0):
    """(match int32 [n1], price float32 [n2], progress int64 [4]), all on the device: the optimal one-to-one assignment of the
    instance in which every row keeps the columns of its list (val / col [n1, cut] of candidate_lists) and may stay unmatched
    at the value `floor`, by Bertsekas' forward auction (mke_assign_rounds) run to its fixed point.  match[i] = the column of
    row i or -1; total = sum of the matched values + floor * unmatched rows >= the optimum of that instance - n1 * eps (with
    f32 rounding n1 * (eps + 2^-16) while (largest value - floor) + eps <= 16).  progress = rounds run, rows still bidding (0),
    bids made, rows settled unmatched.  More than `max_rounds` rounds raise, naming eps.  `tail_cap` / `flags` select the
    hand-over point of the tail kernel and the form without it (tests, tuning): the result is the same bit for bit."""
    state, price, progress, _ = _auction(val, col, n2, eps, floor, int(batch), int(max_rounds), int(tail_cap), int(flags))
    n1 = col.shape[0]
    match = torch.empty(n1, dtype=torch.int32, device=col.device)
    counts = torch.empty(3, dtype=torch.int32, device=col.device)     # zeroed by the call
    _lib.assign_finish(_lib.assign_args(val, col, n2, eps, floor, state, None, None, None, None, None, match=match, counts=counts))
    return match, price, progress


def assignment_alignment(embed1, embed2, metric, normalize, csls_k, nums_threads, cut=100, eps=1e-3, floor=None, sim_mat=None, *,
                         sinkhorn=None):
    """Optimal one-to-one alignment ("Hungarian") against the gold column = row index, without the matrix.  Returns (match,
    precision, recall, f1): match int64 [n1] on the host, match[i] = the row of embed2 assigned to row i of embed1 or -1; the
    pairing maximises the sum of similarities over the instance in which every row keeps its `cut` best columns (the lists of
    stable_alignment, under the same metric / CSLS / Sinkhorn re-scoring or a given sim_mat), to within n1 * (eps + 2^-16) of
    that instance's optimum (assignment_matching).  `floor` is the value of staying unmatched, in units of the value the lists
    hold (re-scored when csls_k or sinkhorn is set); None = the smallest finite listed value - 1, so that any listed pair beats
    staying unmatched.  (largest listed value - floor) + eps above 16 is refused: the f32 form of the guarantee rests on it.
    precision = gold pairs / matched rows * 100, recall = gold pairs / n1 * 100, f1 their harmonic mean, all 0.0 when nothing
    matched.  `nums_threads` is accepted and ignored."""
    _check_metric(metric, "assignment_alignment")
    csls_k, sinkhorn = _check_rescoring(csls_k, sinkhorn)
    if sinkhorn is not None and sim_mat is not None:
        raise _lib.MultiKEHipError("assignment_alignment: sinkhorn re-scores the embeddings' similarities; a given sim_mat is used as it is")
    if sim_mat is None and len(embed2) < len(embed1):
        raise _lib.MultiKEHipError("assignment_alignment: gold column = row index needs len(embed2) >= len(embed1)")
    if not (np.isfinite(float(eps)) and float(eps) >= _lib.ASSIGN_MIN_EPS):
        raise _lib.MultiKEHipError(f"assignment_alignment: eps = {eps} (needs a finite eps >= 2^-14)")
    t = time.time()
    if sim_mat is not None:
        if not isinstance(sim_mat, torch.Tensor):
            sim_mat = torch.as_tensor(np.asarray(sim_mat), dtype=torch.float32).to("cuda")
        sim_mat = sim_mat.float().contiguous()
        n1, n2 = sim_mat.shape
        if n2 < n1:
            raise _lib.MultiKEHipError("assignment_alignment: gold column = row index needs len(embed2) >= len(embed1)")
        val, col, _ = candidate_lists(None, None, 0, max(1, min(int(cut), n2)), sim_mat=sim_mat)
    else:
        operands = prepare_operands(embed1, embed2, metric, normalize, "cuda")
        a, b, kpad, code, sq1, sq2 = operands
        n1, n2 = a.shape[0], b.shape[0]
        val, col, _ = candidate_lists(a, b, kpad, max(1, min(int(cut), n2)), code, sq1, sq2, _rescoring_terms(operands, csls_k, sinkhorn))
    listed = (col >= 0) & torch.isfinite(val)
    inf = torch.full_like(val, float("inf"))
    lo, hi = torch.stack([torch.where(listed, val, inf).min(), torch.where(listed, val, -inf).max()]).tolist() if n1 > 0 else (0.0, 0.0)
    print("generating candidate lists costs time {:.3f} s ".format(time.time() - t))     # the read-back above synchronised
    if not np.isfinite(lo):                                                               # nothing listed at all
        lo = hi = 0.0
    floor = lo - 1.0 if floor is None else float(floor)
    if not np.isfinite(floor):
        raise _lib.MultiKEHipError(f"assignment_alignment: floor = {floor} is not finite")
    if (hi - floor) + float(eps) > ASSIGN_VALUE_RANGE:
        raise _lib.MultiKEHipError(f"assignment_alignment: (largest listed value {hi} - floor {floor}) + eps {eps} exceeds "
                                   f"{ASSIGN_VALUE_RANGE}: scale the similarities or raise floor")
    t = time.time()
    match, _, progress = assignment_matching(val, col, n2, float(eps), floor)
    match = match.cpu().numpy().astype(np.int64)
    rounds = int(progress[0])
    matched = int((match >= 0).sum())
    gold = int((match == np.arange(n1)).sum())
    precision = gold / matched * 100 if matched else 0.0
    recall = gold / n1 * 100 if matched else 0.0
    f1 = 2 * precision * recall / (precision + recall) if gold else 0.0
    cost = time.time() - t
    print("optimal assignment precision = {:.3f}%, recall = {:.3f}%, f1 = {:.3f}%, matched = {}, rounds = {}, time = {:.3f} s ".format(
        precision, recall, f1, matched, rounds, cost))
    return match, precision, recall, f1


def print_results(top_k, hits, mr, mrr, cost, accurate, csls_k=0, sinkhorn=None):
    """The reference's result lines (code/base/alignment.py:64-73); with sinkhorn = (iters, tau) lines of the same shape."""
    if sinkhorn is not None:
        how = " with sinkhorn: iters={}, tau={},".format(*sinkhorn[:2]) + (" cut={},".format(sinkhorn[2]) if len(sinkhorn) == 3 else "")
    else:
        how = " with csls: csls={},".format(csls_k) if csls_k > 0 else ":"
    rest = ", mr = {:.3f}, mrr = {:.6f}".format(mr, mrr) if accurate else ""
    print("{} results{} hits@{} = {}%{}, time = {:.3f} s ".format("accurate" if accurate else "quick", how, top_k, hits, rest, cost))

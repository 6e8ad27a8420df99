"""Self-training (bootstrapping): links found by the label-free decoder become 'swapping' supervision, in HBM.

The reference swaps its seed links into triples once, on the host (code/base/read.py:130-164; base/kgs.py
`swap_relation_triples` / `swap_attribute_triples`).  Here the same per-triple step runs as a kernel over device columns
(`mke_swap_triples`, an ordered stream compaction), so that a schedule can redo it every few epochs over the links the
mutual nearest-neighbour decoder finds among the unlabelled entities:

    partner_table     a decoder's `match` + the entity ids of its rows and columns -> partner[e] (int32 [n_entities], -1 = none)
    swap_triples      triple columns + partner -> the swapped list, a `TripleArray` whose columns live on the device
    bootstrap_links   embeddings of the candidate rows -> (partner, match, counts): one mutual decode, then partner_table
    edit_links        a link set kept across refreshes + this refresh's match + the decode's operands -> the edited link set
                      (`mke_links_edit`, include/multike_links.h); `LinkStore` holds the set of a model

Tensors or NumPy go in, as with the decoders of base/alignment.py; what cannot be right is refused with `MultiKEHipError`
before the device is touched.  `swap_host` is the same walk in NumPy: the `host()` form of the device-built lists.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from . import alignment
from .kgs import TripleArray

__all__ = ["partner_table", "swap_triples", "bootstrap_links", "bootstrap_options", "swap_host", "BootstrapLinks", "edit_links",
           "LinkStore"]


def _i32(x, name, device="cuda"):
    """A contiguous int32 device vector of a tensor, an array or a list (integer input only)."""
    if isinstance(x, torch.Tensor):
        if x.dtype not in (torch.int32, torch.int64) or x.dim() != 1:
            raise _lib.MultiKEHipError(f"{name}: expected a 1-D integer tensor, got {x.dtype} of shape {tuple(x.shape)}")
        return x.to(device=device, dtype=torch.int32).contiguous()
    a = np.asarray(x)
    if a.size == 0:
        a = a.astype(np.int32)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise _lib.MultiKEHipError(f"{name}: expected a 1-D integer array, got {a.dtype} of shape {a.shape}")
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=device)


def _check_entities(n_entities, who):
    if int(n_entities) != n_entities or not 0 <= int(n_entities) < 2 ** 31:
        raise _lib.MultiKEHipError(f"{who}: n_entities must be an integer in [0, 2^31), got {n_entities!r}")
    return int(n_entities)


def partner_table(match, ids1, ids2, n_entities):
    """The link table of a one-to-one `match` (int [n1]: a column of the decode or -1) over the rows' entity ids `ids1` [n1] and
    the columns' `ids2` [n2]: int32 [n_entities] on the device, partner[ids1[i]] = ids2[match[i]] and back, -1 elsewhere."""
    n_entities = _check_entities(n_entities, "partner_table")
    if len(match) != len(ids1):
        raise _lib.MultiKEHipError(f"partner_table: match has {len(match)} rows, ids1 {len(ids1)}")
    return _lib.boot_partner(_i32(match, "match"), _i32(ids1, "ids1"), _i32(ids2, "ids2"), n_entities)


def _columns(cols):
    """Three int32 device columns of `cols`: three vectors (tensors or arrays), or one [n, 3] array / tensor."""
    if isinstance(cols, (torch.Tensor, np.ndarray)):
        if cols.ndim != 2 or cols.shape[1] != 3:
            raise _lib.MultiKEHipError(f"swap_triples: expected three columns or an [n, 3] array, got shape {tuple(cols.shape)}")
        cols = tuple(cols[:, k] for k in range(3))
    if len(cols) != 3:
        raise _lib.MultiKEHipError(f"swap_triples: expected three columns, got {len(cols)}")
    out = tuple(_i32(c, "swap_triples: column %d" % k) for k, c in enumerate(cols))
    if len({c.numel() for c in out}) != 1:
        raise _lib.MultiKEHipError("swap_triples: the columns differ in length")
    return out


def _check_table(partner, weight):
    if not isinstance(partner, torch.Tensor) or partner.dtype != torch.int32 or partner.dim() != 1:
        raise _lib.MultiKEHipError("swap_triples: partner must be partner_table's int32 device vector")
    if weight is not None and (not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.shape != partner.shape):
        raise _lib.MultiKEHipError("swap_triples: weight must be a float32 device vector with one entry per entity, as partner")


def swap_host(h, p, t, partner, heads_only=False, weight=None):
    """mke_swap_triples in NumPy -> (int64 [m, 3], float64 [m] or None): triple k yields (partner[h], p, t) when its head is
    linked and then, unless heads_only, (h, p, partner[t]) when its tail is, in list order."""
    h, p, t, partner = (np.asarray(x, dtype=np.int64) for x in (h, p, t, partner))

    def linked(e):
        ok = (e >= 0) & (e < len(partner))
        out = np.full(len(e), -1, dtype=np.int64)
        out[ok] = partner[e[ok]]
        return out
    ph = linked(h)
    pt = np.full(len(h), -1, dtype=np.int64) if heads_only else linked(t)
    eh, et = ph >= 0, pt >= 0
    each = eh.astype(np.int64) + et
    first = np.cumsum(each) - each                      # where a triple's entries start
    out = np.empty((int(each.sum()), 3), dtype=np.int64)
    out[first[eh]] = np.stack([ph[eh], p[eh], t[eh]], axis=1)
    out[(first + eh)[et]] = np.stack([h[et], p[et], pt[et]], axis=1)
    if weight is None:
        return out, None
    weight = np.asarray(weight, dtype=np.float64)
    w = np.empty(len(out), dtype=np.float64)
    w[first[eh]] = weight[h[eh]]
    w[(first + eh)[et]] = weight[t[et]]
    return out, w


def _swap_launch(cols, partner, heads_only, weight):
    """Enqueue one mke_swap_triples at the worst-case capacity; nothing is read back.  -> the state `_swap_finish` takes."""
    out, out_w, count = _lib.swap_triples(*cols, partner, heads_only=heads_only, weight=weight)
    return cols, partner, bool(heads_only), weight, out, out_w, count


def _swap_finish(state, n):
    """The list of a `_swap_launch` whose count the caller has read: the first n entries, still on the device."""
    cols, partner, heads_only, weight, out, out_w, _ = state

    def host():     # the same list made on the host, from host copies made only now
        return swap_host(*(c.cpu().numpy() for c in cols), partner.cpu().numpy(), heads_only,
                         None if weight is None else weight.cpu().numpy())
    return TripleArray.on_device(tuple(c[:n] for c in out), None if out_w is None else out_w[:n], host)


def swap_triples(cols, partner, heads_only=False, weight=None):
    """The 'swapping' supervision of the triples `cols` (three columns or [n, 3]) under the link table `partner` ->
    (TripleArray living on the device, its length).  heads_only: attribute triples, whose third column is a value id.
    weight: float32 [n_entities] on the device, the weight an entry takes from the linked entity it replaces (None =
    an unweighted list).  Allocates the worst case (2 n entries, n with heads_only), reads the count back once and slices."""
    _check_table(partner, weight)
    state = _swap_launch(_columns(cols), partner, heads_only, weight)
    n = int(state[-1].item())
    return _swap_finish(state, n), n


def edit_links(held, match, operands, retain=None, new_score=None):
    """One edit of a link set that lives across refreshes -> (out int32 [n1], score float32 [n1], counts int32 [7]), all on the
    device.  `held` [n1]: the column every row is linked to or -1 (the `out` of the edit before; all -1 at the start); `match`
    [n1]: this refresh's one-to-one decode; `operands`: what the decode swept, alignment.prepare_operands' tuple followed by the
    re-scoring terms (alignment._rescoring_terms' pair, or None) — the tuple of alignment._mutual_operands, prepared ONCE for the
    decode and for this.  Per row, the first rule that applies (include/multike_links.h):
        a new pair always wins (nothing is compared: for the mutual decoder each of a new pair's ends is the other's best on the
        same values, so no old link at either end has a larger value; the rule is the same for any other decoder's match);
        an old link one of whose ends is in a new pair is displaced;
        an old link is kept while its value today — metric and re-scoring of the decode, so CSLS units with CSLS — is >= `retain`
        (None: no retention threshold, every undisplaced link is kept; NaN is refused), and expires otherwise.
    score: a kept link's value today, `new_score` (float32 [n1], e.g. the decode's row-best value) copied for a new pair, 0
    elsewhere.  counts = (links, links with out[i] == i, new, re-found, kept, displaced, expired).  Nothing is read back."""
    if retain is not None and np.isnan(float(retain)):
        raise _lib.MultiKEHipError("edit_links: retain is NaN (None = no retention threshold)")
    a, b, kpad, code, sq_a, sq_b = operands[:6]
    terms = operands[6] if len(operands) > 6 else None
    held, match = _i32(held, "held", a.device), _i32(match, "match", a.device)
    return _lib.links_edit(held, match, a, b, kpad, code, sq_a, sq_b, *(terms or (None, None)),
                           retain=float("-inf") if retain is None else float(retain), new_score=new_score)


class LinkStore:
    """The link set of a model between two refreshes: `held(n)` is the int32 device vector edit_links takes (all -1 before the
    first refresh), `update(out)` keeps an edit's result.  The candidates of a model are fixed, so a set of another length is
    refused."""

    def __init__(self):
        self._held = None

    def held(self, n, device="cuda"):
        if self._held is None:
            self._held = torch.full((int(n),), -1, dtype=torch.int32, device=device)
        if self._held.numel() != int(n):
            raise _lib.MultiKEHipError(f"LinkStore: the link set has {self._held.numel()} rows, this refresh {int(n)}")
        return self._held

    def update(self, out):
        if self._held is not None and self._held.numel() != out.numel():
            raise _lib.MultiKEHipError(f"LinkStore: the link set has {self._held.numel()} rows, the edit {out.numel()}")
        self._held = out

    def __len__(self):
        return 0 if self._held is None else self._held.numel()


def bootstrap_links(embeds1, embeds2, ids1, ids2, n_entities, threshold=None, csls_k=0, sinkhorn=None, *, scores=False, store=None,
                    retain=None):
    """One label-free decode of the candidate rows -> (partner, match, counts), all on the device: the mutual nearest-neighbour
    pairs of `embeds1` [n1, d] and `embeds2` [n2, d] (inner product of unit rows, CSLS or Sinkhorn re-scored on request, at or
    above `threshold` in units of the value compared), as base.alignment.mutual_pairs finds them, and their link table over the
    entity ids `ids1` / `ids2`.  counts int32 [2] = (pairs, pairs with match[i] == i).  scores=True appends the float32 [n1]
    value of every row's best column (mutual_pairs' `score`).
    store = a LinkStore: the links accumulate.  The decode's match is edited against the store's set (edit_links, on the
    decode's own operands, `retain` as there), the store keeps the result, and what is returned — `match`, the table made of it,
    counts int32 [7] as edit_links', and with scores=True edit_links' `score` — is the edited set."""
    n_entities = _check_entities(n_entities, "bootstrap_links")
    csls_k, sinkhorn = alignment._check_rescoring(csls_k, sinkhorn)
    if threshold is not None and np.isnan(float(threshold)):
        raise _lib.MultiKEHipError("bootstrap_links: the threshold is NaN (None = no threshold)")
    if len(embeds1) != len(ids1) or len(embeds2) != len(ids2):
        raise _lib.MultiKEHipError(f"bootstrap_links: {len(embeds1)} / {len(embeds2)} rows, {len(ids1)} / {len(ids2)} entity ids")
    ids1, ids2 = _i32(ids1, "ids1"), _i32(ids2, "ids2")
    if store is None:
        match, counts, row_best = alignment._mutual(embeds1, embeds2, "inner", True, csls_k, threshold, sinkhorn)
        partner = _lib.boot_partner(match, ids1, ids2, n_entities)
        return (partner, match, counts) + ((alignment._best_value(row_best),) if scores else ())
    if retain is not None and np.isnan(float(retain)):
        raise _lib.MultiKEHipError("bootstrap_links: retain is NaN (None = no retention threshold)")
    operands = alignment._mutual_operands(embeds1, embeds2, "inner", True, csls_k, sinkhorn)
    match, _, row_best = alignment._mutual_decode(operands, threshold)
    out, score, counts = edit_links(store.held(match.numel(), match.device), match, operands, retain, alignment._best_value(row_best))
    store.update(out)
    partner = _lib.boot_partner(out, ids1, ids2, n_entities)
    return (partner, out, counts) + ((score,) if scores else ())


def bootstrap_options(args):
    """The checked `bootstrap_*` hyper-parameters -> None when self-training is off (`bootstrap_freq` absent or 0), else
    (freq, start, threshold, csls_k, view, weighted); with `bootstrap_accumulate` > 0 (links kept across refreshes, edit_links)
    two more: (.., True, retain), retain = `bootstrap_retain`, or the threshold when that is None (None = no retention
    threshold), in the units of the decode.  `bootstrap_accumulate` without `bootstrap_freq` is ignored."""
    freq = int(getattr(args, "bootstrap_freq", 0) or 0)
    if freq <= 0:
        return None
    start = int(getattr(args, "bootstrap_start", 10))
    threshold = getattr(args, "bootstrap_threshold", None)
    csls_k = max(int(getattr(args, "bootstrap_csls", 0) or 0), 0)
    weighted = int(getattr(args, "bootstrap_weighted", 0) or 0) > 0
    view = getattr(args, "bootstrap_view", None)
    if start < 0:
        raise _lib.MultiKEHipError(f"bootstrap_start must be >= 0, got {start}")
    if threshold is not None and np.isnan(float(threshold)):
        raise _lib.MultiKEHipError("bootstrap_threshold is NaN (None = no threshold)")
    if weighted and csls_k > 0:
        raise _lib.MultiKEHipError("bootstrap_weighted and bootstrap_csls are both set: the weight of a bootstrapped triple is its "
                                   "pair's raw similarity clamped to [0, 1], and CSLS re-scored values are in other units")
    if view not in (None, "nv", "rv", "av", "avg", "final"):
        raise _lib.MultiKEHipError(f"bootstrap_view {view!r}: one of 'nv', 'rv', 'av', 'avg', 'final' or None")
    threshold = None if threshold is None else float(threshold)
    retain = getattr(args, "bootstrap_retain", None)
    if retain is not None and np.isnan(float(retain)):
        raise _lib.MultiKEHipError("bootstrap_retain is NaN (None = bootstrap_threshold)")
    if int(getattr(args, "bootstrap_accumulate", 0) or 0) <= 0:
        return freq, start, threshold, csls_k, view, weighted
    return freq, start, threshold, csls_k, view, weighted, True, threshold if retain is None else float(retain)


class BootstrapLinks:
    """The links of the last refresh: `ids1`, `ids2` are int32 device vectors of the paired entities (made on first use: the
    refresh itself does not wait for them), `host()` the same as a list of (entity of KG1, entity of KG2)."""

    def __init__(self, match, cand1, cand2, n):
        self._match, self._cand1, self._cand2, self.n, self._ids = match, cand1, cand2, int(n), None

    def _pairs(self):
        if self._ids is None:
            rows = torch.nonzero(self._match >= 0).reshape(-1)
            self._ids = (self._cand1[rows].contiguous(), self._cand2[self._match[rows].long()].contiguous())
        return self._ids

    ids1 = property(lambda self: self._pairs()[0])
    ids2 = property(lambda self: self._pairs()[1])

    def __len__(self):
        return self.n

    def host(self):
        return list(zip(self.ids1.cpu().tolist(), self.ids2.cpu().tolist()))

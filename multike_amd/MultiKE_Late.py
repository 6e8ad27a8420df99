"""MultiKE_Late.py surface of the reference (code/MultiKE_Late.py): `valid` / `test` / weighted view averaging
(`wva`, `valid_WVA`, `test_WVA`) and the SSL driver `MultiKE_Late` (late combination: view training, then
`shared_learning_max_epoch` epochs of shared-space mapping).  The callers of the hot path — §8f-1 "next" row: same
phase order, gates (`i > start_predicate_soft_alignment`, `i % eval_freq`, `i % truncated_freq`), step counts and loss
normalisation as the reference; the work itself runs on the GPU through `MultiKE_model.MultiKE`."""
from __future__ import annotations

import math
import time

import numpy as np

from . import _lib
from .base import bootstrap as boot
from .base import evaluation as eva
from .base.alignment import assignment_alignment, mutual_alignment, stable_alignment
from .base.batch import neighbour_table, refresh_seed
from .base.bootstrap import bootstrap_options
from .base.kgs import TripleArray
from .MultiKE_model import MultiKE
from .utils import sinkhorn_option, task_divide


def _view_embeddings(model, embed_choice, w):
    """code/MultiKE_Late.py:15-28 / 40-53: which [|E|, dim] matrix an `embed_choice` denotes (normalised views)."""
    pick = {"nv": model.name_embeds, "rv": model.rv_ent_embeds, "av": model.av_ent_embeds, "final": model.ent_embeds}
    if embed_choice in pick:
        return pick[embed_choice].eval(session=model.session)
    if embed_choice == "avg":
        return (w[0] * model.name_embeds.eval(session=model.session) + w[1] * model.rv_ent_embeds.eval(session=model.session)
                + w[2] * model.av_ent_embeds.eval(session=model.session))
    return model.ent_embeds.eval(session=model.session)


def _device_ids(model, key, entities):
    """int32 device tensor of an entity list of `model.kgs`, made once per model (the lists never change)."""
    import torch
    cache = model.__dict__.setdefault("_eval_ids", {})
    if key not in cache:
        cache[key] = torch.as_tensor(np.asarray(entities(), dtype=np.int32), device=model.device)
    return cache[key]


def _view_rows(model, embed_choice, w, ids):
    """Rows `ids` of the matrix `_view_embeddings` denotes, gathered ON THE DEVICE (HIP gather of the normalised view): the
    evaluator then never sees a host copy — the reference's `.eval(session)` of a whole [|E|, dim] table + fancy indexing is
    a 60 MB read-back and 20 ms of host work per call at 200K entities.  None when the model's tables are not device tables."""
    pick = {"nv": model.name_embeds, "rv": model.rv_ent_embeds, "av": model.av_ent_embeds, "final": model.ent_embeds}
    tabs = [pick[embed_choice]] if embed_choice in pick else \
        ([model.name_embeds, model.rv_ent_embeds, model.av_ent_embeds] if embed_choice == "avg" else [model.ent_embeds])
    if not all(hasattr(t, "lookup") for t in tabs) or getattr(model, "device", None) is None:
        return None
    if embed_choice == "avg":
        return w[0] * tabs[0].lookup(ids) + w[1] * tabs[1].lookup(ids) + w[2] * tabs[2].lookup(ids)
    return tabs[0].lookup(ids)


def _eval_pair(model, embed_choice, w, key1, ents1, key2, ents2):
    ids1 = ids2 = None
    if getattr(model, "device", None) is not None and hasattr(model.ent_embeds, "lookup"):
        ids1, ids2 = _device_ids(model, key1, ents1), _device_ids(model, key2, ents2)
        e1 = _view_rows(model, embed_choice, w, ids1)
        if e1 is not None:
            return e1, _view_rows(model, embed_choice, w, ids2)
    ent_embeds = _view_embeddings(model, embed_choice, w)
    return ent_embeds[ents1(), ], ent_embeds[ents2(), ]


def valid(model, embed_choice='avg', w=(1, 1, 1)):
    """code/MultiKE_Late.py:14-36: valid entities of KG1 against valid+test entities of KG2."""
    k = model.kgs
    embeds1, embeds2 = _eval_pair(model, embed_choice, w, "valid1", lambda: k.valid_entities1,
                                  "valid2+test2", lambda: k.valid_entities2 + k.test_entities2)
    print(embed_choice, 'valid results:')
    _, mrr_12 = eva.valid(embeds1, embeds2, None, model.args.top_k, model.args.test_threads_num, normalize=True)
    return mrr_12


def test(model, embed_choice='avg', w=(1, 1, 1)):
    """code/MultiKE_Late.py:39-61."""
    k = model.kgs
    embeds1, embeds2 = _eval_pair(model, embed_choice, w, "test1", lambda: k.test_entities1, "test2", lambda: k.test_entities2)
    print(embed_choice, 'test results:')
    _, mrr_12 = eva.valid(embeds1, embeds2, None, model.args.top_k, model.args.test_threads_num, normalize=True,
                          csls_k=_csls_k(model), sinkhorn=_sinkhorn(model))
    _stable(model, embeds1, embeds2)
    _mutual(model, embeds1, embeds2)
    _assign(model, embeds1, embeds2)
    return mrr_12


def _csls_k(model):
    """Hyper-parameter `csls` (OpenEA's key; 0 = off): CSLS re-scoring of the test-time evaluations only — validation and
    early stopping stay plain."""
    return int(getattr(model.args, "csls", 0) or 0)


def _sinkhorn(model):
    """Hyper-parameters `sinkhorn_iters` (0 = off) / `sinkhorn_tau`: Sinkhorn re-scoring of the test-time evaluations only,
    as `csls` — validation and early stopping stay plain.  -> (iters, tau) or None."""
    return sinkhorn_option(model.args)


def _stable(model, embeds1, embeds2):
    """Hyper-parameter `stable_cut` (0 = off): after the greedy lines of a test, the one-to-one stable alignment of the same
    rows (code/base/alignment.py:82-128) over every suitor's `stable_cut` best targets, CSLS or Sinkhorn re-scored as the test is."""
    cut = int(getattr(model.args, "stable_cut", 0) or 0)
    if cut > 0:
        stable_alignment(embeds1, embeds2, 'inner', True, _csls_k(model), model.args.test_threads_num, cut=cut,
                         sinkhorn=_sinkhorn(model))


def _mutual(model, embeds1, embeds2):
    """Hyper-parameters `mutual` (0 = off) / `mutual_threshold` (absent or None = none): after the greedy (and stable) lines of
    a test, precision / recall / F1 of the mutual nearest-neighbour pairs of the same rows, CSLS or Sinkhorn re-scored as the
    test is (the threshold is then in units of the re-scored value)."""
    if int(getattr(model.args, "mutual", 0) or 0) > 0:
        mutual_alignment(embeds1, embeds2, 'inner', True, _csls_k(model), model.args.test_threads_num,
                         threshold=getattr(model.args, "mutual_threshold", None), sinkhorn=_sinkhorn(model))


def _assign(model, embeds1, embeds2):
    """Hyper-parameters `assign_cut` (0 = off) / `assign_eps` / `assign_floor` (absent or None = the smallest listed value - 1):
    after the greedy (stable, mutual) lines of a test, precision / recall / F1 of the optimal one-to-one assignment of the same
    rows over every row's `assign_cut` best targets, CSLS or Sinkhorn re-scored as the test is (the floor is then in units of
    the re-scored value)."""
    cut = int(getattr(model.args, "assign_cut", 0) or 0)
    if cut > 0:
        assignment_alignment(embeds1, embeds2, 'inner', True, _csls_k(model), model.args.test_threads_num, cut=cut,
                             eps=float(getattr(model.args, "assign_eps", None) or 1e-3), floor=getattr(model.args, "assign_floor", None),
                             sinkhorn=_sinkhorn(model))


def _unit_rows(x):
    import torch
    if isinstance(x, torch.Tensor):          # device rows
        n = torch.linalg.norm(x, dim=1, keepdim=True)
        return x / torch.where(n == 0, torch.ones_like(n), n)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.where(n == 0, 1.0, n)


def _compute_weight(embeds1, embeds2, embeds3):
    """code/MultiKE_Late.py:64-81: mean cosine between a view and the average of the three views."""
    other = _unit_rows((embeds1 + embeds2 + embeds3) / 3)
    weights = (_unit_rows(embeds1) * other).sum(1)  # the diagonal of the similarity matrix, without the matrix
    mean = np.mean(weights) if isinstance(weights, np.ndarray) else np.float32(float(weights.mean()))
    print(tuple(weights.shape), mean)
    return mean


def wva(embeds1, embeds2, embeds3):
    """code/MultiKE_Late.py:84-88 (the function returns after the three weights; the rest of its body is dead)."""
    return (_compute_weight(embeds1, embeds2, embeds3), _compute_weight(embeds2, embeds1, embeds3),
            _compute_weight(embeds3, embeds1, embeds2))


def _wva_eval(model, ents1, ents2, label, keys=None, csls_k=0, stable=False, sinkhorn=None):
    tabs = (model.name_embeds, model.rv_ent_embeds, model.av_ent_embeds)
    if keys is not None and getattr(model, "device", None) is not None and all(hasattr(t, "lookup") for t in tabs):
        ids1, ids2 = _device_ids(model, keys[0], lambda: ents1), _device_ids(model, keys[1], lambda: ents2)
        v1 = [t.lookup(ids1) for t in tabs]          # rows gathered on the device: no whole-table read-back
        v2 = [t.lookup(ids2) for t in tabs]
    else:
        views = tuple(t.eval() for t in tabs)
        v1 = [v[ents1, ] for v in views]
        v2 = [v[ents2, ] for v in views]
    wsum = np.array(wva(*v1)) + np.array(wva(*v2))
    wsum = wsum / wsum.sum()
    print('weights', *wsum)
    embeds1 = sum(float(w) * v for w, v in zip(wsum, v1))
    embeds2 = sum(float(w) * v for w, v in zip(wsum, v2))
    print(label)
    _, mrr_12 = eva.valid(embeds1, embeds2, None, model.args.top_k, model.args.test_threads_num, normalize=True, csls_k=csls_k,
                          sinkhorn=sinkhorn)
    if stable:
        _stable(model, embeds1, embeds2)
        _mutual(model, embeds1, embeds2)
        _assign(model, embeds1, embeds2)
    return mrr_12


def valid_WVA(model):
    """code/MultiKE_Late.py:99-135."""
    return _wva_eval(model, model.kgs.valid_entities1, model.kgs.valid_entities2 + model.kgs.test_entities2,
                     'wvag valid results:', keys=("valid1", "valid2+test2"))


def test_WVA(model):
    """code/MultiKE_Late.py:138-173."""
    return _wva_eval(model, model.kgs.test_entities1, model.kgs.test_entities2, 'wvag test results:', keys=("test1", "test2"),
                     csls_k=_csls_k(model), stable=True, sinkhorn=_sinkhorn(model))


class _ScheduledMultiKE(MultiKE):
    """What `MultiKE_CV.run` and `MultiKE_Late.run` share (code/MultiKE_CSL.py:36-56, code/MultiKE_Late.py:201-223):
    step counts, supervision lists, the per-epoch view training block and the periodic refreshes."""

    # The evaluation calls of the schedules go through these hooks (module-level functions by default, looked up when called);
    # the multi-GPU drivers (multike_amd/distributed_run.py) override them with rank-sharded evaluation.
    def _valid(self, embed_choice):
        return valid(self, embed_choice=embed_choice)

    def _test(self, embed_choice):
        return test(self, embed_choice=embed_choice)

    def _valid_WVA(self):
        return valid_WVA(self)

    def _test_WVA(self):
        return test_WVA(self)

    defer_predicate_update = False      # set True by the model's constructor on a GPU (instances made without it run in line)

    def _prepare(self):
        kgs, pam, a = self.kgs, self.predicate_align_model, self.args
        rel_n = kgs.kg1.local_relation_triples_num + kgs.kg2.local_relation_triples_num
        attr_n = kgs.kg1.local_attribute_triples_num + kgs.kg2.local_attribute_triples_num
        self._rel_steps = int(math.ceil(rel_n / a.batch_size))
        self._attr_steps = int(math.ceil(attr_n / a.batch_size))  # the reference divides by batch_size here too
        self._rel_tasks = task_divide(list(range(self._rel_steps)), a.batch_threads_num)
        self._attr_tasks = task_divide(list(range(self._attr_steps)), a.batch_threads_num)
        self._ckge_rel_triples = kgs.kg1.sup_relation_triples_list + kgs.kg2.sup_relation_triples_list
        self._ckge_attr_triples = kgs.kg1.sup_attribute_triples_list + kgs.kg2.sup_attribute_triples_list
        self._refresh_predicate_lists()
        self._neighbors = (None, None)
        self._entity_list = kgs.kg1.entities_list + kgs.kg2.entities_list
        self._seed_ckge = (self._ckge_rel_triples, self._ckge_attr_triples)    # what `_bootstrap` appends its lists to
        self.bootstrap_links = None
        bootstrap_options(a)                                                   # refuse a bad combination before the first epoch

    bootstrap_default_view = ('final', (1, 1, 1))     # the embedding the driver validates on (MultiKE_Late: 'avg')

    def _bootstrap(self, i):
        """Self-training refresh at the end of epoch i (hyper-parameters `bootstrap_*`, off unless `bootstrap_freq` > 0): decode
        the unlabelled entities, keep the mutual pairs, swap them into triples ON THE DEVICE and train the two cross-KG
        entity-inference loops on the seed lists plus these until the next refresh replaces them.  The candidates are the valid
        + test entities of each KG, in that order on both sides; no gold link is read to choose pairs (the precision printed
        is a diagnostic: gold = the same index, which the pairing kernel counts anyway).  Decode, link table, both swaps and the
        weight table are enqueued without waiting; one read-back (the two list lengths and the two counters) ends the refresh.
        `bootstrap_accumulate` > 0: the links live across refreshes (`base.bootstrap.edit_links` on the decode's own operands: a
        new pair always wins, an old link with an end in a new pair is displaced, any other old link stays while its value today
        is >= `bootstrap_retain`).  Table, swaps, weights (a kept link's: its value today) and `bootstrap_links` then come from
        the edited set, the seven counters of the edit ride in the same single read-back, and the line ends in ", kept K,
        displaced D, expired X".
        Not done: the sampler's known-triple filter does not grow by the bootstrapped triples, and `kg.add_sup_*` is not called."""
        opt = bootstrap_options(self.args)
        if opt is None:
            return
        freq, start, threshold, csls_k, view, weighted = opt[:6]
        accumulate = len(opt) > 6
        if i < start or (i - start) % freq != 0 or i >= self.args.max_epoch:
            return
        import torch
        t0 = time.time()
        k = self.kgs
        ids1 = _device_ids(self, "valid1+test1", lambda: k.valid_entities1 + k.test_entities1)
        ids2 = _device_ids(self, "valid2+test2", lambda: k.valid_entities2 + k.test_entities2)
        choice, w = (view, (1, 1, 1)) if view is not None else self.bootstrap_default_view
        e1 = _view_rows(self, choice, w, ids1)
        if e1 is None:
            raise _lib.MultiKEHipError("bootstrap_freq > 0: the tables of this model are not device tables")
        e2 = _view_rows(self, choice, w, ids2)
        src = self._bootstrap_sources()
        if accumulate:
            store = self.__dict__.setdefault("_boot_store", boot.LinkStore())
            partner, match, counts, score = boot.bootstrap_links(e1, e2, ids1, ids2, k.entities_num, threshold, csls_k, scores=True,
                                                                 store=store, retain=opt[7])
        else:
            partner, match, counts, score = boot.bootstrap_links(e1, e2, ids1, ids2, k.entities_num, threshold, csls_k, scores=True)
        weight = None
        if weighted:
            # weight[e] = clamp(score of e's pair, 0, 1) for both entities of a pair; unmatched rows write a spare last word
            n = k.entities_num
            m = match >= 0
            spare = torch.full_like(ids1, n)
            weight = torch.zeros(n + 1, dtype=torch.float32, device=self.device)
            val = score.clamp(0.0, 1.0)
            weight[torch.where(m, ids1, spare).long()] = val
            weight[torch.where(m, ids2[match.clamp(min=0).long()], spare).long()] = val
            weight = weight[:n]
        rel = boot._swap_launch(src["rel"], partner, False, weight)
        attr = boot._swap_launch(src["attr"], partner, True, weight)
        n_rel, n_attr, pairs, gold, *edit = torch.cat([rel[-1], attr[-1], counts.long()]).cpu().tolist()      # the one read-back
        lists = (boot._swap_finish(rel, n_rel), boot._swap_finish(attr, n_attr))
        self._ckge_rel_triples, self._ckge_attr_triples = (
            new if seed is None else seed + new for seed, new in zip(self._bootstrap_seeds(weighted), lists))
        self.bootstrap_links = boot.BootstrapLinks(match, ids1, ids2, pairs)
        self._bootstrap_partner = partner
        print("bootstrapping after epoch {}: {} pairs, precision = {:.3f}%, {} relation triples, {} attribute triples, "
              "time = {:.3f} s".format(i, pairs, gold / pairs * 100 if pairs else 0.0, n_rel, n_attr, time.time() - t0) +
              (", kept {}, displaced {}, expired {}".format(*edit[2:5]) if accumulate else ""))
        self._bootstrap_edit = tuple(edit) if accumulate else None      # (new, re-found, kept, displaced, expired) of this refresh

    def _bootstrap_sources(self):
        """Device columns of the KG1 ++ KG2 local (pre-supervision) relation and attribute id-triples: uploaded once per model."""
        src = self.__dict__.get("_boot_sources")
        if src is None:
            import torch
            kg1, kg2 = self.kgs.kg1, self.kgs.kg2

            def up(a, b):
                arr = np.concatenate([np.asarray(a, dtype=np.int32).reshape(-1, 3), np.asarray(b, dtype=np.int32).reshape(-1, 3)])
                t = torch.as_tensor(arr, device=self.device)
                return tuple(t[:, c].contiguous() for c in range(3))
            src = self._boot_sources = {"rel": up(kg1.local_relation_triples_list, kg2.local_relation_triples_list),
                                        "attr": up(kg1.local_attribute_triples_list, kg2.local_attribute_triples_list)}
        return src

    def _bootstrap_seeds(self, weighted):
        """The two seed lists in the form the bootstrapped lists are appended to: their device columns (the ones the training
        loops already hold) as `TripleArray`s, with weights of 1.0 when the bootstrapped triples are weighted.  None for an empty
        seed list.  The lists `_prepare` made stay as they are."""
        key = bool(weighted)
        cache = self.__dict__.setdefault("_boot_seeds", {})
        if cache.get("of") is not self._seed_ckge:
            cache.clear()
            cache["of"] = self._seed_ckge
        if key not in cache:
            import torch
            out = []
            for seed in self._seed_ckge:
                if len(seed) == 0:
                    out.append(None)
                    continue
                lst = self._list(seed)
                ones = torch.ones(lst.n, dtype=torch.float32, device=self.device) if weighted else None

                def host(seed=seed, n=lst.n):
                    return np.asarray([t[:3] for t in seed], dtype=np.int64).reshape(-1, 3), (np.ones(n) if weighted else None)
                out.append(TripleArray.on_device(lst.cols, ones, host))
            cache[key] = tuple(out)
        return cache[key]

    def _refresh_predicate_lists(self):
        pam = self.predicate_align_model
        self._ckgp_rel_triples = pam.sup_relation_alignment_triples1 + pam.sup_relation_alignment_triples2
        self._ckga_attr_triples = pam.sup_attribute_alignment_triples1 + pam.sup_attribute_alignment_triples2

    def _train_views(self, i):
        """One epoch of the six view / cross-KG phases in the reference's order.

        The relation group (relation view -> ckge-rel -> ckgp-rel: rv_ent_embeds, rel_embeds) and the attribute group
        (attribute view -> ckge-attr -> ckga-attr: av_ent_embeds, attr_embeds, the CNNs) touch disjoint state, so they
        commute; with `overlap_views` the two groups are enqueued on two HIP streams and meet again before common-space
        learning.  Each group is a chain of small, launch-floor-dominated kernels that leaves most of the chip idle, and
        nothing synchronises inside the epoch (the loss read-backs are deferred to the end), unlike the per-step overlap
        schemes that were measured and rejected for the relation view alone."""
        a = self.args
        n1, n2 = self._neighbors
        soft = i > a.start_predicate_soft_alignment

        def relation_group_a():
            self.train_relation_view_1epo(i, self._rel_steps, self._rel_tasks, None, n1, n2)
            self.train_cross_kg_entity_inference_relation_view_1epo(i, self._ckge_rel_triples)

        def relation_group_b():
            if soft:
                self.train_cross_kg_relation_inference_1epo(i, self._ckgp_rel_triples)

        def attribute_group_a():
            self.train_attribute_view_1epo(i, self._attr_steps, self._attr_tasks, None, n1, n2)
            self.train_cross_kg_entity_inference_attribute_view_1epo(i, self._ckge_attr_triples)

        def attribute_group_b():
            if soft:
                self.train_cross_kg_attribute_inference_1epo(i, self._ckga_attr_triples)

        if not getattr(self, "overlap_views", True) or a.optimizer not in ("Adagrad", "SGD"):
            relation_group_a()
            self._finish_predicate_update()
            relation_group_b()
            attribute_group_a()
            attribute_group_b()
            return
        import torch
        main = torch.cuda.current_stream()
        if getattr(self, "_side_stream", None) is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
        side = self._side_stream
        self._defer_losses, self._pending = True, []
        try:
            # two streams: 18.0 ms per epoch against 22.0 on one (C2 shape).  Measured and not kept: a higher stream priority
            # for either group (no change), enqueueing the two groups from two host threads (18.9 ms: the device, not the
            # host, is what the two chains share).
            # A predicate refresh deferred from the end of the previous epoch (`_update_predicate_alignment`) replaces the lists
            # three loops read: the relation- and attribute-inference loops, and — through
            # `attribute_triples_w_weights1/2` (code/predicate_alignment.py:170-174, read at code/MultiKE_model.py:325-328) —
            # the attribute VIEW itself.  Only the relation view and its entity-inference loop are list-independent: they are
            # enqueued first, the refresh is finished while the device works through them, and everything else follows it —
            # the order in which the reference's epoch i + 1 sees the lists of the refresh at the end of epoch i
            # (code/MultiKE_CSL.py:80-87).  (Round 4 enqueued the attribute view before the refresh: one epoch on stale weights
            # after every refresh.)
            start = torch.cuda.Event()
            start.record(main)                      # what the side stream must see: everything before this epoch
            relation_group_a()
            rel_a, self._pending = self._pending, []
            self._finish_predicate_update()
            side.wait_event(start)
            with torch.cuda.stream(side):
                attribute_group_a()
                attribute_group_b()
            attr_ab, self._pending = self._pending, []
            attr_a, attr_b = attr_ab, []
            relation_group_b()
            self._pending = rel_a + self._pending + attr_a + attr_b       # the reference prints the relation group's losses first
            main.wait_stream(side)
        finally:
            self._defer_losses = False
        for p in self._pending:
            p.finish()
        self._pending = []

    def _update_predicate_alignment(self):
        """code/MultiKE_CSL.py:80-87 / code/MultiKE_Late.py:244-251 (host-side soft predicate alignment)."""
        pam = self.predicate_align_model
        if getattr(self, "defer_predicate_update", False) and hasattr(pam, "update_predicate_alignment"):
            # The refresh reads rel_embeds / attr_embeds as they are NOW and its lists are first read by the next epoch's
            # relation- / attribute-inference loops.  Snapshot the two (small) tables to pinned host memory without waiting
            # and do the host work when those loops are about to be enqueued (`_finish_predicate_update`, called by
            # `_train_views` after the phases that do not need the lists are on the device): same inputs, same lists, and the
            # device is not idle meanwhile.
            import torch
            snaps = []
            for tab in (self.rel_embeds, self.attr_embeds):
                dev = tab.lookup(None)
                host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
                host.copy_(dev, non_blocking=True)
                snaps.append((dev, host))                    # the device tensor is held until the copy has completed
            ev = torch.cuda.Event()
            ev.record()
            self._pending_predicate = (ev, snaps)
            return
        if hasattr(pam, "update_predicate_alignment"):
            pam.update_predicate_alignment(self.rel_embeds.eval(session=self.session))
            pam.update_predicate_alignment(self.attr_embeds.eval(session=self.session), predicate_type='attribute')
        self._refresh_predicate_lists()

    def _finish_predicate_update(self):
        """The host side of a deferred `_update_predicate_alignment` (no-op when none is pending)."""
        pend = getattr(self, "_pending_predicate", None)
        if pend is None:
            return
        self._pending_predicate = None
        ev, snaps = pend
        ev.synchronize()
        pam = self.predicate_align_model
        import torch
        if getattr(pam, "device", None) is None:
            pam.update_predicate_alignment(snaps[0][1].numpy())
            pam.update_predicate_alignment(snaps[1][1].numpy(), predicate_type='attribute')
            self._refresh_predicate_lists()
            return
        # the lists are built in HBM from static inputs (the KGs' triples) and two small tables: on a stream of their own, so that
        # neither the table uploads nor the gathers queue behind the phases already enqueued on the training streams
        if getattr(self, "_refresh_stream", None) is None:
            self._refresh_stream = torch.cuda.Stream(device=self.device)
        rs = self._refresh_stream
        with torch.cuda.stream(rs):
            pam.update_predicate_alignment(snaps[0][1].numpy())
            pam.update_predicate_alignment(snaps[1][1].numpy(), predicate_type='attribute')
            self._refresh_predicate_lists()
        done = torch.cuda.Event()
        done.record(rs)
        for st in (torch.cuda.current_stream(), getattr(self, "_side_stream", None)):
            if st is not None:
                st.wait_event(done)

    def _refresh_neighbours(self, i):
        """Truncated negative sampling: k-NN candidate lists every `truncated_freq` epochs
        (code/MultiKE_CSL.py:89-102).  Stays on the device: (candidate table, valid flags) per KG."""
        a, kgs = self.args, self.kgs
        if a.neg_sampling != 'truncated' or i % a.truncated_freq != 0:
            return
        t1 = time.time()
        assert 0.0 < a.truncated_epsilon < 1.0
        cap = int(getattr(a, "truncated_cap", 0) or 0)     # > 0: capped tables; 0: the call made without it
        out = []
        for kg, useful in ((kgs.kg1, kgs.useful_entities_list1), (kgs.kg2, kgs.useful_entities_list2)):
            k = int((1 - a.truncated_epsilon) * kg.entities_num)
            # the reference's random.sample(candidates, neg_triple_num) raises ValueError on a shorter list
            # (code/base/batch.py:96-99); say so before the kernels see it
            if min(k, cap or k) < a.neg_triple_num or k > len(useful):
                raise ValueError(f"truncated sampling: {k} neighbours per entity (int((1 - truncated_epsilon) * "
                                 f"{kg.entities_num}))" + (f", capped to truncated_cap = {cap}," if cap else "") +
                                 f" must be >= neg_triple_num ({a.neg_triple_num}) and <= the "
                                 f"{len(useful)} useful entities of the KG")
            emb = self.rv_ent_embeds.lookup(self._ids(useful))
            capped = dict(cap=cap, seed=refresh_seed(getattr(a, "seed", 0), i, len(out))) if cap else {}
            if getattr(a, "truncated_keyed", None) is not None:      # unset: neighbour_table's automatic rule
                capped["keyed"] = bool(int(a.truncated_keyed))
            out.append(neighbour_table(emb, useful, k, kgs.entities_num, device=self.device, **capped))
        self._neighbors = tuple(out)
        print("generating neighbors of {} entities costs {:.3f} s.".format(len(self._entity_list), time.time() - t1) +
              (" (tables capped to {} of the neighbours)".format(cap) if cap else ""))

    def _ids(self, lst):
        import torch
        return torch.as_tensor(np.asarray(lst, dtype=np.int32), device=self.device)


class MultiKE_Late(_ScheduledMultiKE):
    """code/MultiKE_Late.py:176-280 — run_SSL.py's model."""

    bootstrap_default_view = ('avg', (1, 1, 1))

    def __init__(self, data, args, attr_align_model):
        super().__init__(data, args, attr_align_model)
        self.flag1, self.flag2, self.early_stop = -1, -1, False
        self.defer_predicate_update = True       # the soft predicate-alignment refresh's host work under the next epoch's kernels
        if hasattr(self.predicate_align_model, "_refresh_device"):
            self.predicate_align_model.device = self.device    # ... and its per-triple work in HBM (no list upload)
        self._define_variables()
        self._define_name_view_graph()
        self._define_relation_view_graph()
        self._define_attribute_view_graph()
        self._define_cross_kg_entity_reference_relation_view_graph()
        self._define_cross_kg_entity_reference_attribute_view_graph()
        self._define_cross_kg_relation_reference_graph()
        self._define_cross_kg_attribute_reference_graph()
        self._define_common_space_learning_graph()
        self._define_space_mapping_graph()

    def run(self):
        a = self.args
        self._prepare()
        self._valid('nv')
        self._valid('avg')
        for i in range(1, a.max_epoch + 1):
            print('epoch {}:'.format(i))
            self._train_views(i)
            if i >= a.start_valid and i % a.eval_freq == 0:
                self._valid('rv')
                self._valid('av')
                self._valid('avg')
                self._valid_WVA()
                if i >= a.start_predicate_soft_alignment:
                    self._update_predicate_alignment()
            if self.early_stop or i == a.max_epoch:
                break
            self._bootstrap(i)
            self._refresh_neighbours(i)
        for i in range(1, a.shared_learning_max_epoch + 1):
            self.train_shared_space_mapping_1epo(i, self._entity_list)
            if i >= a.start_valid and i % a.eval_freq == 0:
                self._valid('final')
        self._finish_predicate_update()
        self._save_async = True
        self.save()
        results = {k: self._test(k) for k in ('nv', 'rv', 'av', 'avg')}
        results['wva'] = self._test_WVA()
        results['final'] = self._test('final')
        self._join_save()
        return results

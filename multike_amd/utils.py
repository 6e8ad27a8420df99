"""Host-side helpers with the reference's names and semantics (code/utils.py) that the hot path's callers use.
Only what the path needs: args loading, step->producer division, output folder naming, embedding savers."""
from __future__ import annotations

import json
import os
import time

import numpy as np


class ARGs:
    """Attribute bag over the JSON dict (code/utils.py:19-22)."""

    def __init__(self, dic):
        for k, v in dic.items():
            setattr(self, k, v)


def load_args(file_path):
    """code/utils.py:10-16 — same key names as code/args.json."""
    with open(file_path, "r") as f:
        args_dict = json.load(f)
    print("load arguments:", args_dict)
    return ARGs(args_dict)


def default_args(**over):
    """The hyper-parameters the reference ships in code/args.json (:1-52), grouped by what reads them; paths are left
    empty.  `load_args(file)` on a user's own JSON file overrides any subset of them."""
    d = dict(
        # data
        training_data="", output="output/results/", word2vec_path="", dataset_division="631/", alignment_module="swapping",
        # literal auto-encoder (code/literal_encoder.py)
        encoder_epoch=100, encoder_active="thah", encoder_normalize=True, retrain_literal_embeds=False, literal_normalize=True,
        # embeddings and optimisation
        dim=75, optimizer="Adagrad", learning_rate=0.001, relation_learning_rate=0.005, ITC_learning_rate=0.004,
        max_epoch=200, shared_learning_max_epoch=200, batch_size=5000, entity_batch_size=5000, attribute_batch_size=5000,
        # negative sampling
        neg_triple_num=10, neg_sampling="truncated", truncated_epsilon=0.98, truncated_freq=20,
        # capped neighbour tables of the truncated sampler (0 = off, the reference's tables): every refresh keeps a uniform random
        # `truncated_cap`-subset of each entity's exact int((1 - truncated_epsilon) * |E_kg|) neighbours, so the two tables grow
        # with |E| * cap instead of |E|^2; every negative is still uniform over the exact neighbour set
        truncated_cap=0,
        # the matrix-free selection of a capped refresh (`neighbour_table(keyed=)`): None = automatic (large KGs whose k is beyond
        # the thresholded sweep), 0 / 1 = never / always (1 needs truncated_cap below the neighbour count)
        truncated_keyed=None,
        # host-side worker counts of the reference (accepted, unused: batches are produced on the device)
        batch_threads_num=4, test_threads_num=8,
        # validation / early stopping
        start_valid=100, eval_freq=10, stop_metric="mrr", top_k=[1, 5, 10, 50], is_save=True,
        # CSLS re-scoring of the final tests (OpenEA's key `csls`; 0 = off, the reference's evaluation)
        csls=0,
        # one-to-one (Gale-Shapley) alignment of the final tests over every suitor's `stable_cut` best targets (0 = off)
        stable_cut=0,
        # Sinkhorn re-scoring of the final tests: `sinkhorn_iters` iterations (0 = off) at temperature `sinkhorn_tau`; not with `csls`
        # `sinkhorn_cut` > 0 iterates on the support of the `sinkhorn_cut`-long candidate lists of both sides instead of on all pairs
        # (0 = dense): two list sweeps and no sweep per iteration, for million-entity tests
        sinkhorn_iters=0, sinkhorn_tau=0.05, sinkhorn_cut=0,
        # mutual nearest-neighbour alignment of the final tests (0 = off): precision / recall / F1 of the pairs that are each
        # other's best, at or above `mutual_threshold` (None = none; in units of the re-scored value when `csls` / Sinkhorn is on)
        mutual=0, mutual_threshold=None,
        # optimal one-to-one assignment ("Hungarian", by auction) of the final tests over every row's `assign_cut` best targets
        # (0 = off), to within n * `assign_eps` of that instance's optimum; `assign_floor` = the value of staying unmatched (None =
        # the smallest listed value - 1; in units of the re-scored value when `csls` / Sinkhorn is on)
        assign_cut=0, assign_eps=1e-3, assign_floor=None,
        # self-training of the single-GPU schedules (0 = off): from epoch `bootstrap_start` on, every `bootstrap_freq` epochs the
        # mutual nearest-neighbour pairs of the unlabelled (valid + test) entities, at or above `bootstrap_threshold` (None = none),
        # are swapped into the two cross-KG entity-inference lists beside the seed links, replacing the pairs of the refresh before.
        # `bootstrap_csls` > 0 decodes on CSLS re-scored values (the threshold is then in those units); `bootstrap_view` names the
        # embedding decoded (None = the one the driver validates on: 'final' for ITC, 'avg' for SSL); `bootstrap_weighted` = 1
        # weights a bootstrapped triple by its pair's similarity clamped to [0, 1] (seed triples 1.0; not with `bootstrap_csls`)
        # `bootstrap_accumulate` = 1 keeps the links across refreshes instead: a refresh's new pairs always win, an old link with
        # an end in a new pair is dropped, and any other old link stays while its value today is >= `bootstrap_retain` (None =
        # `bootstrap_threshold`; both None = no retention threshold; in the units of the decode, CSLS units with `bootstrap_csls`)
        bootstrap_freq=0, bootstrap_start=10, bootstrap_threshold=None, bootstrap_csls=0, bootstrap_view=None, bootstrap_weighted=0,
        bootstrap_accumulate=0, bootstrap_retain=None,
        # view combination and predicate soft alignment
        orthogonal_weight=2, cv_name_weight=1, cv_weight=1, start_predicate_soft_alignment=10, predicate_soft_sim=0.85,
        predicate_init_sim=0.90)
    d.update(over)
    return ARGs(d)


def sinkhorn_option(args):
    """(iters, tau) of the hyper-parameters `sinkhorn_iters` / `sinkhorn_tau`, or None when off (0, or the keys absent);
    (iters, tau, cut) when `sinkhorn_cut` > 0 (the sparse re-scoring on the candidate lists' support).
    `csls` and `sinkhorn_iters` both set is an error: they are two re-scorings of the same similarity."""
    iters = int(getattr(args, "sinkhorn_iters", 0) or 0)
    if iters <= 0:
        return None
    if int(getattr(args, "csls", 0) or 0) > 0:
        from ._lib import MultiKEHipError
        raise MultiKEHipError("csls and sinkhorn_iters are both set: choose one re-scoring of the final tests")
    cut = int(getattr(args, "sinkhorn_cut", 0) or 0)
    tau = float(getattr(args, "sinkhorn_tau", 0.05))
    return (iters, tau, cut) if cut > 0 else (iters, tau)


def task_divide(idx, n):
    """code/utils.py:35-49: n-1 chunks of total//n and a last chunk with the remainder; degenerate cases
    return a single task."""
    total = len(idx)
    if n <= 0 or total == 0 or n > total:
        return [idx]
    if n == total:
        return [[i] for i in idx]
    size = total // n
    tasks = [idx[k * size:(k + 1) * size] for k in range(n - 1)]
    tasks.append(idx[(n - 1) * size:])
    return tasks


def merge_dic(dic1, dic2):
    return {**dic1, **dic2}


def generate_out_folder(out_folder, training_data_path, div_path, method_name):
    """code/utils.py:52-57."""
    path = training_data_path.strip("/").split("/")[-1]
    folder = out_folder + method_name + "/" + path + "/" + div_path + str(time.strftime("%Y%m%d%H%M%S")) + "/"
    print("results output folder:", folder)
    return folder


def dict2file(file, dic):
    if dic is None:
        return
    with open(file, "w", encoding="utf8") as f:
        for i, j in dic.items():
            f.write(str(i) + "\t" + str(j) + "\n")
    print(file, "saved.")


def save_embeddings(folder, kgs, ent_embeds, nv_ent_embeds, rv_ent_embeds, av_ent_embeds, rel_embeds, attr_embeds):
    """Same file names / formats as code/utils.py:70-91 so downstream tooling keeps working."""
    os.makedirs(folder, exist_ok=True)
    if ent_embeds is not None:
        np.save(folder + "ent_embeds.npy", ent_embeds)
        np.save(folder + "nv_ent_embeds.npy", nv_ent_embeds)
        np.save(folder + "rv_ent_embeds.npy", rv_ent_embeds)
        np.save(folder + "av_ent_embeds.npy", av_ent_embeds)
    if rel_embeds is not None:
        np.save(folder + "rel_embeds.npy", rel_embeds)
    if attr_embeds is not None:
        np.save(folder + "attr_embeds.npy", attr_embeds)
    for name, kg, attr in (("kg1_ent_ids", kgs.kg1, "entities_id_dict"), ("kg2_ent_ids", kgs.kg2, "entities_id_dict"),
                           ("kg1_rel_ids", kgs.kg1, "relations_id_dict"), ("kg2_rel_ids", kgs.kg2, "relations_id_dict"),
                           ("kg1_attr_ids", kgs.kg1, "attributes_id_dict"), ("kg2_attr_ids", kgs.kg2, "attributes_id_dict")):
        dict2file(folder + name, getattr(kg, attr, None))
    print("Embeddings saved!")


# ----------------------------------------------------------------------------------------------------------------
# text-side inputs of the literal view (host-side data preparation, no kernels)
# ----------------------------------------------------------------------------------------------------------------
def read_word2vec(file_path, vector_dimension=300):
    """Text word-vector file, `word v1 ... vD` separated by single spaces; lines with another field count (e.g. the
    `count dim` header) are skipped (code/utils.py:94-105)."""
    word2vec = {}
    with open(file_path, "r", encoding="utf-8") as f:
        for line in f:
            p = line.rstrip("\n").split(" ")
            if len(p) == vector_dimension + 1:
                word2vec[p[0]] = np.asarray(p[1:], dtype=np.float64).astype(np.float32)
    return word2vec


def read_local_name_file(file_path, entities_set):
    """`uri \\t local name`: a trailing "(...)" qualifier is cut at the first '(' and '_' becomes ' '; entities
    without a line get '' (code/utils.py:117-137).  Every line must name an entity of the set."""
    names = {}
    with open(file_path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            p = line.rstrip("\n").split("\t")
            if len(p) != 2:
                raise ValueError(f"{file_path}:{no}: expected 2 tab-separated fields")
            ln = p[1].split("(")[0] if p[1].endswith(")") else p[1]
            names[p[0]] = ln.replace("_", " ")
    for e in entities_set:
        names.setdefault(e, "")
    if len(names) != len(entities_set):
        raise ValueError(f"{file_path}: names for {len(names) - len(entities_set)} entities that are not in the KG")
    return names


def read_local_name(folder_path, entities_set_1, entities_set_2):
    names = read_local_name_file(folder_path + "entity_local_name_1", entities_set_1)
    names.update(read_local_name_file(folder_path + "entity_local_name_2", entities_set_2))
    return names


def is_number(s):
    """code/utils.py:276-290: float()-parsable or a single numeric unicode character."""
    try:
        float(s)
        return True
    except ValueError:
        pass
    try:
        import unicodedata
        unicodedata.numeric(s)
        return True
    except (TypeError, ValueError):
        return False


_DROP = str.maketrans("", "", ".(),\"")
_SPACE = str.maketrans("_-/", "   ")


def clear_attribute_triples(attribute_triples):
    """Literal clean-up before encoding (code/utils.py:233-273): keep attributes with >= 10 triples; cut typed /
    @en suffixes; delete . ( ) , " and turn _ - / into spaces; drop values that still contain 'http'.
    Returns (triples, numeric literals, string literals) -- the literal lists classify the value after the suffix
    cut and before the character clean-up, dropped triples included, as the reference does."""
    triples = dict.fromkeys(attribute_triples)      # the reference's set(): duplicates dropped; here in the input's own order
    freq = {}
    for _, a, _ in triples:
        freq[a] = freq.get(a, 0) + 1
    kept, numbers, strings = [], [], []
    memo = {}                                       # a literal value is cleaned once, however many triples carry it
    for e, a, v in triples:
        if freq[a] < 10:
            continue
        m = memo.get(v)
        if m is None:
            w = v
            cut = w.find('"^^')
            if cut >= 0:
                w = w[:cut]
            if w.endswith('"@en'):
                w = w[:w.index('"@en')]
            c = w.translate(_DROP).translate(_SPACE)
            m = memo[v] = (w, is_number(w), None if "http" in c else c)
        (numbers if m[1] else strings).append(m[0])
        if m[2] is not None:
            kept.append((e, a, m[2]))
    return kept, numbers, strings


class CharHashEmbedder:
    """Vectors for words missing from the word2vec file.  The reference trains gensim character embeddings on the
    unlisted words and averages them per word (code/utils.py:140-172, code/literal_encoder.py:147-156); gensim is
    not a dependency here and that training is itself unseeded, so this stand-in gives every character a fixed
    pseudo-random unit-variance vector (seeded by its code point) and returns the mean over the word's characters.
    Same shape of information (character bag), deterministic, no training."""

    def __init__(self, vector_dimension=300, scale=0.1):
        self.dim, self.scale, self._cache = int(vector_dimension), float(scale), {}

    def _char(self, ch):
        v = self._cache.get(ch)
        if v is None:
            v = np.random.default_rng(ord(ch)).standard_normal(self.dim).astype(np.float32) * self.scale
            self._cache[ch] = v
        return v

    def __call__(self, word):
        if not word:
            return None
        return np.mean([self._char(c) for c in word], axis=0)


_LIBRARY_TOUCHED = set()


def touch_library_kernels(device="cuda"):
    """First use of a PyTorch / rocPRIM kernel family loads its code object: 50-80 ms each on this part, with the GPU idle.
    Round 4's kernel trace of `run()` had five such gaps inside the first training epochs (index / elementwise kernels, the
    blit copies, randperm, rocPRIM's sort and scan, reductions: 0.35 s of a 4.1 s run).  The host side of the drivers uses
    those families for epoch bookkeeping only (shuffles, index lists, loss read-backs); touching each once on a few elements
    when the model is BUILT moves the loads out of the training loop (they cost the same there, but no epoch waits for
    them).  Once per process and device."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda" or (dev.index or 0) in _LIBRARY_TOUCHED:
        return
    _LIBRARY_TOUCHED.add(dev.index or 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n = 257
    p = torch.randperm(n, device=dev, generator=g)                       # randperm + its rocPRIM sort
    i32 = p.to(torch.int32)
    f = torch.rand(n, device=dev, generator=g)
    _ = torch.sort(f)[0], torch.argsort(p, stable=True), torch.sort(i32)[0]
    # long inputs take other sort kernels (radix passes) than short ones, and the k-NN refresh's keyed permutations are int64
    # mix / shift / argsort chains over 100K ids (base/batch.py keyed_perm: 186 ms at its first call, 1 ms later)
    big = torch.arange(1 << 18, dtype=torch.int64, device=dev)
    big = (big ^ (big >> 30)) * -4658895280553007687
    big = big ^ (big >> 27)
    _ = torch.argsort(big, stable=True), torch.sort(big.to(torch.int32))[0], torch.sort(big.float())[0], torch.randperm(1 << 18, device=dev, generator=g)
    _ = f[p], i32[p], p[p], f.to(torch.float64)[p]                       # index kernels
    z = torch.zeros(n, device=dev)
    z[p] = f                                                             # index_put
    z.index_add_(0, p, f)
    _ = torch.cat([f, z]), torch.arange(n, device=dev, dtype=torch.int32), torch.cumsum(p, 0), torch.bincount(p, minlength=n)
    _ = torch.nonzero(f > 0.5), (f * 2 + 1).sum(), f.double().sum(), p.max(), torch.topk(f, 5), torch.repeat_interleave(p[:4], 2)
    _ = torch.full((n,), 0.1, device=dev), torch.empty(n, dtype=torch.uint8, device=dev).fill_(1), z.clone()
    h = torch.empty(n, dtype=torch.float32, pin_memory=True)
    h.copy_(f, non_blocking=True)                                        # blit kernels, both directions
    _ = torch.as_tensor(h.numpy(), device=dev), torch.randint(0, 5, (n,), device=dev, generator=g, dtype=torch.int32)
    torch.cuda.synchronize(dev)

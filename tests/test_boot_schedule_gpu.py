"""Self-training in the schedules (`_ScheduledMultiKE._bootstrap`, hyper-parameters `bootstrap_*`) on the smallest synthetic
folder: 60 pairs, of which 18 are train links and 6 + 36 valid + test pairs are the candidates.

The decoded rows are PLANTED: every candidate pair gets a coordinate of its own in the decoded table, so the mutual pairs are
known (all gold, similarity exactly 1.0) and the link table and both swapped lists can be compared with the definitions of
tests/boot_oracle.py entry for entry."""
import contextlib
import io
import math
import re

import numpy as np
import pytest

import boot_oracle as BO

pytestmark = pytest.mark.gpu

DIM = 48            # >= the 42 candidate pairs + the spare coordinates of the crossed pair


def _args(folder, word_file, **over):
    from multike_amd.synthetic import synthetic_args
    base = dict(training_data=folder, output=folder + "out/", word2vec_path=word_file, dataset_division="631/", encoder_epoch=3,
                encoder_active="tanh", encoder_normalize=True, retrain_literal_embeds=False, literal_normalize=True, dim=DIM,
                batch_size=120, attribute_batch_size=100, entity_batch_size=64, neg_triple_num=4, learning_rate=0.01, max_epoch=4,
                shared_learning_max_epoch=1, start_valid=2, eval_freq=2, start_predicate_soft_alignment=1, truncated_freq=2,
                truncated_epsilon=0.9, is_save=False, bootstrap_freq=1, bootstrap_start=1)
    base.update(over)
    return synthetic_args(**base)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from multike_amd.data_model import DataModel
    from multike_amd.synthetic import write_dataset_folder
    folder = str(tmp_path_factory.mktemp("boot")) + "/"
    wf = write_dataset_folder(folder)
    with contextlib.redirect_stdout(io.StringIO()):
        data = DataModel(_args(folder, wf))                    # trains the literal encoder once; later DataModels load its cache
    return folder, wf, data


def _model(folder, cls=None, **over):
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.predicate_alignment import PredicateAlignModel
    folder, wf, data = folder
    args = _args(folder, wf, **over)
    with contextlib.redirect_stdout(io.StringIO()):
        m = (cls or MultiKE_CV)(data, args, PredicateAlignModel(data.kgs, args))
        m._prepare()
    return m


def _candidates(m):
    k = m.kgs
    return np.array(k.valid_entities1 + k.test_entities1), np.array(k.valid_entities2 + k.test_entities2)


def _plant(m, crossed=None):
    """Candidate pair i <- coordinate i in the table the ITC driver decodes ('final' = ent_embeds).  crossed = (a, b): row a of
    KG1 and row b of KG2 are each other's best at similarity 0.6 (exactly representable parts: 0.6, 0.8 on a spare coordinate),
    their own counterparts sit alone on spare coordinates."""
    import torch
    c1, c2 = _candidates(m)
    n = len(c1)
    assert n == 42 and n + 3 <= DIM
    r1, r2 = np.zeros((n, DIM), dtype=np.float32), np.zeros((n, DIM), dtype=np.float32)
    r1[np.arange(n), np.arange(n)] = 1.0
    r2[np.arange(n), np.arange(n)] = 1.0
    if crossed is not None:
        a, b = crossed
        r2[b] = 0.0
        r2[b, a], r2[b, n] = 0.6, 0.8
        r2[a] = 0.0
        r2[a, n + 1] = 1.0
        r1[b] = 0.0
        r1[b, n + 2] = 1.0
    tab = m.ent_embeds
    for ids, rows in ((c1, r1), (c2, r2)):
        at = torch.as_tensor(ids, device=tab.data.device)
        tab.data[at] = 0.0
        tab.data[at, :DIM] = torch.as_tensor(rows, device=tab.data.device)
    return c1, c2


def _local(m, kind):
    k = m.kgs
    tri = getattr(k.kg1, f"local_{kind}_triples_list") + getattr(k.kg2, f"local_{kind}_triples_list")
    return tuple(np.array(c) for c in zip(*tri))


def _seed(m, kind):
    k = m.kgs
    return np.array(getattr(k.kg1, f"sup_{kind}_triples_list") + getattr(k.kg2, f"sup_{kind}_triples_list"), dtype=np.int64).reshape(-1, 3)


def _refresh(m, i=1):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        m._bootstrap(i)
    return out.getvalue()


LINE = (r"bootstrapping after epoch (\d+): (\d+) pairs, precision = (\d+\.\d{3})%, (\d+) relation triples, (\d+) attribute "
        r"triples, time = \d+\.\d{3} s\n")


def _check_lists(m, table, weight=None, seed_w=None):
    import torch
    for kind, lst, heads_only in (("relation", m._ckge_rel_triples, False), ("attribute", m._ckge_attr_triples, True)):
        seed = _seed(m, kind)
        want, want_w = BO.swap(*_local(m, kind), table, heads_only=heads_only, weight=weight)
        assert len(seed) > 0 and len(want) > 0
        full = np.concatenate([seed, want])
        assert lst.dev is not None and len(lst) == len(full)
        assert np.array_equal(torch.stack(lst.dev[0], dim=1).cpu().numpy(), full)        # what the training loops read
        assert np.array_equal(lst.cols, full)                                              # what a reader of the list gets (host())
        if weight is None:
            assert lst.dev[1] is None and lst.w is None
        else:
            full_w = np.concatenate([np.ones(len(seed), dtype=np.float32), want_w])
            assert np.array_equal(lst.dev[1].cpu().numpy(), full_w) and np.array_equal(lst.w.astype(np.float32), full_w)
    return len(m._ckge_rel_triples), len(m._ckge_attr_triples)


def test_planted_rows_give_the_oracles_table_and_lists(folder):
    m = _model(folder)
    seeds = (m._ckge_rel_triples, m._ckge_attr_triples)
    c1, c2 = _plant(m)
    text = _refresh(m)
    n_ent = m.kgs.entities_num
    table = BO.partner(np.arange(len(c1)), c1, c2, n_ent)
    assert np.array_equal(m._bootstrap_partner.cpu().numpy(), table)
    n_rel, n_attr = _check_lists(m, table)
    got = re.fullmatch(LINE, text)
    assert got, text
    assert got.groups() == ("1", "42", "100.000", str(n_rel - len(_seed(m, "relation"))), str(n_attr - len(_seed(m, "attribute"))))
    assert m._seed_ckge[0] is seeds[0] and m._seed_ckge[1] is seeds[1]                    # the seed lists are kept aside, unchanged
    assert seeds[0] == m.kgs.kg1.sup_relation_triples_list + m.kgs.kg2.sup_relation_triples_list
    links = m.bootstrap_links
    assert len(links) == 42 and links.ids1.is_cuda and links.host() == list(zip(c1.tolist(), c2.tolist()))
    train = set(m.kgs.train_entities1) | set(m.kgs.train_entities2)
    assert not train & (set(c1.tolist()) | set(c2.tolist()))                              # train-linked entities are never candidates
    # a second refresh REPLACES the lists: with the rows of half the pairs gone, only the other half stays.  (The odd ones go: a
    # zeroed column ties at 0 for every row and names row 0, which keeps its own column 0, so no pair forms at similarity 0.)
    import torch
    tab = m.ent_embeds
    tab.data[torch.as_tensor(c2[1::2], device=tab.data.device)] = 0.0
    text = _refresh(m, 2)
    keep = np.where(np.arange(42) % 2 == 0, np.arange(42), -1)
    _check_lists(m, BO.partner(keep, c1, c2, n_ent))
    assert re.fullmatch(LINE, text).group(2) == "21" and len(m.bootstrap_links) == 21


def test_a_crossed_pair_below_the_threshold_is_absent(folder):
    a, b = 5, 17
    m = _model(folder, bootstrap_threshold=0.8)
    c1, c2 = _plant(m, crossed=(a, b))
    text = _refresh(m)
    match = np.arange(42)
    match[[a, b]] = -1
    table = BO.partner(match, c1, c2, m.kgs.entities_num)
    assert np.array_equal(m._bootstrap_partner.cpu().numpy(), table) and table[c1[a]] == -1 and table[c2[b]] == -1
    _check_lists(m, table)
    assert re.fullmatch(LINE, text).groups()[1:3] == ("40", "100.000")
    assert (int(c1[a]), int(c2[b])) not in m.bootstrap_links.host()
    # without the threshold the decoder does find it, and the diagnostic says so (it reads gold only to print)
    m.args.bootstrap_threshold = None
    text = _refresh(m)
    match[a] = b
    assert np.array_equal(m._bootstrap_partner.cpu().numpy(), BO.partner(match, c1, c2, m.kgs.entities_num))
    assert re.fullmatch(LINE, text).groups()[1:3] == ("41", "{:.3f}".format(40 / 41 * 100))
    assert (int(c1[a]), int(c2[b])) in m.bootstrap_links.host()


def _train_and_record(m, epoch):
    seen = {}
    for name in ("train_cross_kg_entity_inference_relation_view_1epo", "train_cross_kg_entity_inference_attribute_view_1epo"):
        def wrapped(i, triples, _orig=getattr(m, name), _name=name):
            out = _orig(i, triples)
            seen[_name] = (triples, m._last_sample)
            return out
        setattr(m, name, wrapped)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        m._train_views(epoch)
    losses = {k: float(v) for k, v in re.findall(r"epoch \d+ of (cross-kg entity inference in \w+\. view), avg\. loss: (\S+),", out.getvalue())}
    return seen, losses


@pytest.mark.parametrize("weighted", [0, 1])
def test_training_consumes_the_new_lists(folder, weighted):
    m = _model(folder, bootstrap_weighted=weighted)
    before = (len(m._ckge_rel_triples), len(m._ckge_attr_triples))
    c1, c2 = _plant(m, crossed=(5, 17))                      # no threshold: the crossed pair is in, at similarity 0.6
    _refresh(m)
    weight = None
    if weighted:
        match = np.arange(42)
        match[5], match[17] = 17, -1
        value = np.ones(42, dtype=np.float32)
        # the 0.6 pair's weight is the f32 similarity the decoder computed: a copied float, read back from the same decode
        from multike_amd.base.alignment import mutual_pairs
        import torch
        rows = lambda ids: m.ent_embeds.lookup(torch.as_tensor(ids.astype(np.int32), device="cuda"))
        dec_match, score = mutual_pairs(rows(c1), rows(c2))
        assert np.array_equal(dec_match.cpu().numpy(), match)
        value = np.clip(score.cpu().numpy(), 0.0, 1.0)
        assert abs(value[5] - 0.6) < 1e-6 and (np.delete(value, [5, 17]) == 1.0).all()
        weight = np.zeros(m.kgs.entities_num, dtype=np.float32)
        on = match >= 0
        weight[c1[on]] = value[on]
        weight[c2[match[on]]] = value[on]
        _check_lists(m, BO.partner(match, c1, c2, m.kgs.entities_num), weight=weight)
    assert len(m._ckge_rel_triples) > before[0] and len(m._ckge_attr_triples) > before[1]
    seen, losses = _train_and_record(m, 2)
    assert set(losses) == {"cross-kg entity inference in rel. view", "cross-kg entity inference in attr. view"}
    assert all(math.isfinite(v) and v > 0 for v in losses.values()), losses
    for name, lst, batch in (("train_cross_kg_entity_inference_relation_view_1epo", m._ckge_rel_triples, m.args.batch_size),
                             ("train_cross_kg_entity_inference_attribute_view_1epo", m._ckge_attr_triples, m.args.attribute_batch_size)):
        triples, (_, _, n, bs, steps) = seen[name]
        assert triples is lst and n == len(lst) and steps == math.ceil(n / batch) and bs == (batch if steps > 1 else n)
    assert seen["train_cross_kg_entity_inference_relation_view_1epo"][1][4] >= 2          # more than one step: the list did grow


def test_off_means_untouched(folder, monkeypatch):
    from multike_amd import _lib

    def never(*a, **k):
        raise AssertionError("a self-training kernel was reached with bootstrap_freq = 0")
    monkeypatch.setattr(_lib, "swap_triples", never)
    monkeypatch.setattr(_lib, "boot_partner", never)
    for over in (dict(bootstrap_freq=0), dict(bootstrap_freq=None)):
        m = _model(folder, max_epoch=2, **over)
        lists = (m._ckge_rel_triples, m._ckge_attr_triples)
        for i in range(0, 4):
            assert _refresh(m, i) == "" and m._bootstrap(i) is None
        assert m._ckge_rel_triples is lists[0] and m._ckge_attr_triples is lists[1] and m.bootstrap_links is None
        assert isinstance(lists[0], list) and lists[0] == m.kgs.kg1.sup_relation_triples_list + m.kgs.kg2.sup_relation_triples_list
    m = _model(folder, max_epoch=2, bootstrap_freq=0)
    del m.args.bootstrap_freq, m.args.bootstrap_start                 # the keys absent, as in an args.json written before them
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = m.run()
    assert "bootstrapping" not in out.getvalue() and all(np.isfinite(v) for v in res.values())
    # and the gate when on: from bootstrap_start, every bootstrap_freq epochs, never after the last epoch
    monkeypatch.undo()
    m = _model(folder, max_epoch=9, bootstrap_freq=3, bootstrap_start=2)
    acted = [i for i in range(0, 12) if _refresh(m, i)]
    assert acted == [2, 5, 8]


def test_late_driver_decodes_the_average_view(folder, monkeypatch):
    from multike_amd import MultiKE_Late as late
    m = _model(folder, cls=late.MultiKE_Late)
    seen = []
    real = late._view_rows
    monkeypatch.setattr(late, "_view_rows", lambda model, choice, w, ids: (seen.append((choice, tuple(w))), real(model, choice, w, ids))[1])
    text = _refresh(m)
    assert seen == [("avg", (1, 1, 1))] * 2
    got = re.fullmatch(LINE, text)
    assert got and int(got.group(2)) > 0, text                          # the name view carries signal from the start
    assert len(m._ckge_rel_triples) == len(_seed(m, "relation")) + int(got.group(4))
    m.args.bootstrap_view = "nv"
    del seen[:]
    _refresh(m)
    assert seen == [("nv", (1, 1, 1))] * 2


@pytest.mark.parametrize("method", ["ITC", "SSL"])
def test_run_with_bootstrapping_from_the_command_line(folder, method, tmp_path):
    import json
    from multike_amd.run import main
    path, wf, _ = folder
    cfg = tmp_path / "args.json"
    cfg.write_text(json.dumps(vars(_args(path, wf, bootstrap_freq=0))))
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = main(["--method", method, "--training_data", path.rstrip("/"), "--args", str(cfg), "--set", "max_epoch=3",
                    "--set", "bootstrap_freq=1", "--set", "bootstrap_start=1", "--set", "bootstrap_threshold=0.5"])
    assert all(np.isfinite(v) for v in res.values())
    assert re.findall(r"bootstrapping after epoch (\d+):", out.getvalue()) == ["1", "2"]       # not after the last epoch

"""Self-training with `bootstrap_accumulate` in the schedules (`_ScheduledMultiKE._bootstrap`) on the smallest synthetic folder:
60 pairs, of which 18 are train links and 6 + 36 valid + test pairs are the candidates (as tests/test_boot_schedule_gpu.py).

The decoded rows are PLANTED: candidate pair i sits on coordinate i of the decoded table, so every refresh's decode is known, and
single rows are then turned so that a link is kept beside a decode that no longer finds it, expires, or is displaced."""
import contextlib
import io
import re

import numpy as np
import pytest

import boot_oracle as BO
import links_oracle as LO

pytestmark = pytest.mark.gpu

DIM = 48            # >= the 42 candidate pairs
N = 42
LINE = (r"bootstrapping after epoch (\d+): (\d+) pairs, precision = (\d+\.\d{3})%, (\d+) relation triples, (\d+) attribute "
        r"triples, time = \d+\.\d{3} s")
EDIT = r", kept (\d+), displaced (\d+), expired (\d+)\n"


def _args(folder, word_file, **over):
    from multike_amd.synthetic import synthetic_args
    base = dict(training_data=folder, output=folder + "out/", word2vec_path=word_file, dataset_division="631/", encoder_epoch=3,
                encoder_active="tanh", encoder_normalize=True, retrain_literal_embeds=False, literal_normalize=True, dim=DIM,
                batch_size=120, attribute_batch_size=100, entity_batch_size=64, neg_triple_num=4, learning_rate=0.01, max_epoch=8,
                shared_learning_max_epoch=1, start_valid=2, eval_freq=2, start_predicate_soft_alignment=1, truncated_freq=2,
                truncated_epsilon=0.9, is_save=False, bootstrap_freq=1, bootstrap_start=1)
    base.update(over)
    return synthetic_args(**base)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from multike_amd.data_model import DataModel
    from multike_amd.synthetic import write_dataset_folder
    folder = str(tmp_path_factory.mktemp("links")) + "/"
    wf = write_dataset_folder(folder)
    with contextlib.redirect_stdout(io.StringIO()):
        data = DataModel(_args(folder, wf))                    # trains the literal encoder once; later DataModels load its cache
    return folder, wf, data


def _model(folder, **over):
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.predicate_alignment import PredicateAlignModel
    folder, wf, data = folder
    args = _args(folder, wf, **over)
    with contextlib.redirect_stdout(io.StringIO()):
        m = MultiKE_CV(data, args, PredicateAlignModel(data.kgs, args))
        m._prepare()
    return m


def _candidates(m):
    k = m.kgs
    return np.array(k.valid_entities1 + k.test_entities1), np.array(k.valid_entities2 + k.test_entities2)


def _plant(m, rows1=None, rows2=None):
    """Candidate pair i <- coordinate i in the table the ITC driver decodes ('final' = ent_embeds); rows1 / rows2 = {candidate:
    {coordinate: value}} replace single rows of KG1 / KG2."""
    import torch
    c1, c2 = _candidates(m)
    assert len(c1) == N and len(c2) == N
    r = [np.zeros((N, DIM), dtype=np.float32) for _ in range(2)]
    for side, over in zip(r, (rows1, rows2)):
        side[np.arange(N), np.arange(N)] = 1.0
        for i, row in (over or {}).items():
            side[i] = 0.0
            for k, v in row.items():
                side[i, k] = v
    tab = m.ent_embeds
    for ids, rows in ((c1, r[0]), (c2, r[1])):
        at = torch.as_tensor(ids, device=tab.data.device)
        tab.data[at] = 0.0
        tab.data[at, :DIM] = torch.as_tensor(rows, device=tab.data.device)
    return c1, c2


def _refresh(m, i):
    with contextlib.redirect_stdout(io.StringIO()) as out:
        m._bootstrap(i)
    return out.getvalue()


def _local(m, kind):
    k = m.kgs
    tri = getattr(k.kg1, f"local_{kind}_triples_list") + getattr(k.kg2, f"local_{kind}_triples_list")
    return tuple(np.array(c) for c in zip(*tri))


def _seed(m, kind):
    k = m.kgs
    return np.array(getattr(k.kg1, f"sup_{kind}_triples_list") + getattr(k.kg2, f"sup_{kind}_triples_list"), dtype=np.int64).reshape(-1, 3)


def _check_lists(m, table, weight=None):
    """Both lists are the seed list followed by `swap_host` of the local triples on the link table (weights: 1.0, then the
    weight of the entity replaced)."""
    import torch
    from multike_amd.base.bootstrap import swap_host
    for kind, lst, heads_only in (("relation", m._ckge_rel_triples, False), ("attribute", m._ckge_attr_triples, True)):
        seed = _seed(m, kind)
        want, want_w = swap_host(*_local(m, kind), table, heads_only, weight)
        assert len(seed) > 0 and len(want) > 0
        full = np.concatenate([seed, want])
        assert lst.dev is not None and len(lst) == len(full)
        assert np.array_equal(torch.stack(lst.dev[0], dim=1).cpu().numpy(), full)
        if weight is None:
            assert lst.dev[1] is None
        else:
            assert np.array_equal(lst.dev[1].cpu().numpy(), np.concatenate([np.ones(len(seed)), want_w]).astype(np.float32))


TURNED = {5: {5: 0.6, 17: 0.8}}     # row 5 of KG1 now prefers column 17 (0.8), which answers row 17 (1.0); its own pair is worth 0.6


def test_a_pair_its_decode_no_longer_finds_stays_only_with_accumulation(folder):
    """The test that fails without the feature: found at one refresh, not found at the next — one end prefers a third entity
    that does not answer — and still above `retain`."""
    links = {}
    for acc in (1, 0):
        m = _model(folder, bootstrap_accumulate=acc, bootstrap_retain=0.5)
        c1, c2 = _plant(m)
        text = _refresh(m, 1)
        assert re.fullmatch(LINE + (EDIT if acc else r"\n"), text).group(2) == "42", text
        pair = (int(c1[5]), int(c2[5]))
        assert pair in m.bootstrap_links.host()
        _plant(m, rows1=TURNED)
        text = _refresh(m, 2)
        got = re.fullmatch(LINE + (EDIT if acc else r"\n"), text)
        assert got, text
        links[acc] = m.bootstrap_links.host()
        match = np.arange(N)
        if acc:
            assert got.groups()[1:3] == ("42", "100.000") and got.groups()[5:] == ("1", "0", "0")
            assert pair in links[acc] and len(m.bootstrap_links) == 42
        else:
            match[5] = -1
            assert got.groups()[1:3] == ("41", "100.000")
            assert pair not in links[acc] and len(m.bootstrap_links) == 41
        table = BO.partner(match, c1, c2, m.kgs.entities_num)
        assert np.array_equal(m._bootstrap_partner.cpu().numpy(), table) and (table[c1[5]] == c2[5]) == bool(acc)
        _check_lists(m, table)
        # the pair's swapped triples are in the lists, or are not
        from multike_amd.base.bootstrap import swap_host
        n_with, n_without = (len(swap_host(*_local(m, "relation"), BO.partner(mt, c1, c2, m.kgs.entities_num))[0])
                             for mt in (np.arange(N), np.where(np.arange(N) == 5, -1, np.arange(N))))
        assert n_with > n_without
        assert len(m._ckge_rel_triples) - len(_seed(m, "relation")) == (n_with if acc else n_without)
    assert set(links[1]) - set(links[0]) == {pair}
    # above `retain` is the condition: at 0.7 the same link expires
    m = _model(folder, bootstrap_accumulate=1, bootstrap_retain=0.7)
    _plant(m)
    _refresh(m, 1)
    _plant(m, rows1=TURNED)
    got = re.fullmatch(LINE + EDIT, _refresh(m, 2))
    assert got.group(2) == "41" and got.groups()[5:] == ("0", "0", "1") and pair not in m.bootstrap_links.host()
    # and `bootstrap_retain` None means the threshold of the decode
    m = _model(folder, bootstrap_accumulate=1, bootstrap_threshold=0.7)
    _plant(m)
    _refresh(m, 1)
    _plant(m, rows1=TURNED)
    assert re.fullmatch(LINE + EDIT, _refresh(m, 2)).groups()[5:] == ("0", "0", "1")


@pytest.mark.parametrize("weighted", [0, 1])
def test_three_refreshes_follow_the_oracle_call_by_call(folder, monkeypatch, weighted):
    from multike_amd.base import bootstrap
    calls = []
    real = bootstrap.edit_links

    def spy(held, match, operands, retain=None, new_score=None):
        out = real(held, match, operands, retain, new_score)
        calls.append(dict(held=held, match=match.cpu().numpy(), operands=operands, retain=retain, new_score=new_score.cpu().numpy(), out=out))
        return out
    monkeypatch.setattr(bootstrap, "edit_links", spy)
    m = _model(folder, bootstrap_accumulate=1, bootstrap_retain=0.5, bootstrap_freq=2, bootstrap_weighted=weighted)
    plants = [dict(),
              dict(rows1=TURNED, rows2={9: {}}),               # (5, 5) is kept at 0.6; column 9 is all zero: (9, 9) expires at 0
              dict(rows1={5: TURNED[5], 30: {5: 1.0}}, rows2={9: {}})]     # row 30 and column 5 pair up: (5, 5) and (30, 30) displaced
    texts = []
    for epoch in range(1, 7):
        if epoch % 2:
            c1, c2 = _plant(m, **plants[epoch // 2])
        text = _refresh(m, epoch)
        assert bool(text) == bool(epoch % 2)
        if not text:
            continue
        texts.append(text)
        call = calls[-1]
        a, b, kpad, code, sq_a, sq_b, terms = call["operands"]
        assert kpad == DIM and terms is None and len(calls) == len(texts)
        S = LO.values(a.cpu().numpy(), b.cpu().numpy(), code)
        held = call["held"].cpu().numpy()
        want = LO.edit(held, call["match"], S, call["retain"], call["new_score"])
        out, score, counts = (x.cpu().numpy() for x in call["out"])
        assert call["retain"] == 0.5 and np.array_equal(out, want[0]) and np.array_equal(counts, want[2])
        kept = (LO.clean(call["match"], N) < 0) & (out >= 0)
        assert np.array_equal(score[~kept].view(np.uint32), want[1][~kept].view(np.uint32)) and np.abs(score[kept] - want[1][kept]).max(initial=0) < 1e-6
        if len(calls) > 1:
            assert call["held"] is calls[-2]["out"][0]      # the set of a call is the result of the call before
        else:
            assert (held == -1).all()
        got = re.fullmatch(LINE + EDIT, text)
        assert got, text
        assert [int(x) for x in got.groups()[:2] + got.groups()[5:]] == [epoch, want[2][0], want[2][4], want[2][5], want[2][6]]
        assert got.group(3) == "{:.3f}".format(want[2][1] / want[2][0] * 100)
        assert m._bootstrap_edit == tuple(want[2][2:].tolist())
        table = BO.partner(want[0], c1, c2, m.kgs.entities_num)
        assert np.array_equal(m._bootstrap_partner.cpu().numpy(), table)
        weight = None
        if weighted:                                         # a kept link's weight is its value today, a new pair's the decode's
            weight = np.zeros(m.kgs.entities_num, dtype=np.float32)
            on = out >= 0
            weight[c1[on]] = np.clip(score[on], 0.0, 1.0)
            weight[c2[out[on]]] = np.clip(score[on], 0.0, 1.0)
            assert abs(weight[c1[5]] - 0.6) < 1e-6 or len(calls) != 2
        _check_lists(m, table, weight)
        assert m.bootstrap_links.host() == [(int(c1[i]), int(c2[j])) for i, j in enumerate(want[0]) if j >= 0]
    assert len(calls) == 3
    # the planted story, by hand: (links, gold, new, re-found, kept, displaced, expired)
    assert [c["out"][2].cpu().tolist() for c in calls] == [[42, 42, 42, 0, 0, 0, 0], [41, 41, 40, 40, 1, 0, 1], [40, 39, 40, 39, 0, 2, 0]]
    assert calls[2]["out"][0].cpu().tolist()[30] == 5 and calls[2]["out"][0].cpu().tolist()[5] == -1


def test_without_accumulation_nothing_of_it_is_reached(folder, monkeypatch):
    from multike_amd import _lib
    from multike_amd.base import bootstrap

    def never(*a, **k):
        raise AssertionError("the link-set edit was reached with bootstrap_accumulate = 0")
    monkeypatch.setattr(bootstrap, "edit_links", never)
    monkeypatch.setattr(_lib, "links_edit", never)
    monkeypatch.setattr(_lib, "links_lib", never)
    monkeypatch.setattr(_lib, "_links", None)
    for over in (dict(bootstrap_accumulate=0), dict(bootstrap_accumulate=None), dict(bootstrap_accumulate=0, bootstrap_retain=0.9)):
        m = _model(folder, **over)
        _plant(m)
        assert re.fullmatch(LINE + r"\n", _refresh(m, 1)).group(2) == "42"
        _plant(m, rows1=TURNED)
        assert re.fullmatch(LINE + r"\n", _refresh(m, 2)).group(2) == "41"       # the line and the replacing lists of before
        assert "_boot_store" not in m.__dict__ and m._bootstrap_edit is None
    m = _model(folder, bootstrap_accumulate=1, bootstrap_freq=0)                # without bootstrap_freq it is ignored
    assert _refresh(m, 1) == "" and m.bootstrap_links is None
    assert _lib._links is None


@pytest.mark.parametrize("method", ["ITC", "SSL"])
def test_run_with_accumulation_from_the_command_line(folder, method, tmp_path):
    import json
    from multike_amd.run import main
    path, wf, _ = folder
    cfg = tmp_path / "args.json"
    cfg.write_text(json.dumps(vars(_args(path, wf, bootstrap_freq=0, max_epoch=4))))
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = main(["--method", method, "--training_data", path.rstrip("/"), "--args", str(cfg), "--set", "max_epoch=4",
                    "--set", "bootstrap_freq=1", "--set", "bootstrap_start=1", "--set", "bootstrap_threshold=0.5",
                    "--set", "bootstrap_accumulate=1", "--set", "bootstrap_retain=0.3"])
    assert all(np.isfinite(v) for v in res.values())
    lines = re.findall(LINE + EDIT, out.getvalue())
    assert [ln[0] for ln in lines] == ["1", "2", "3"]                          # not after the last epoch
    assert lines[0][5:] == ("0", "0", "0") and all(int(ln[1]) >= int(ln[5]) for ln in lines)

"""Self-training support without a GPU: the three symbols are exported, bound and declared (version unchanged), the ctypes
structure matches the header, every argument error returns its code and a prefixed message before any launch, the
hyper-parameters and the host surface refuse what they must, and the NumPy definitions (tests/boot_oracle.py) against a
hand-written list and against the host swapping of base/kgs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import boot_oracle as BO
from conftest import ROOT

NEW = {"mke_boot_partner": "int", "mke_swap_temp_bytes": "int64_t", "mke_swap_triples": "int"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "multike_hip.h")).read()


def test_new_symbols_exported_and_listed(lib):
    from multike_amd import _lib
    raw = C.CDLL(_lib.SO_PATH)
    h = _header()
    for s, ret in NEW.items():
        assert s in _lib.SYMBOLS
        getattr(raw, s)
        assert re.search(r"^" + ret + r"\s+" + s + r"\s*\(", h, flags=re.M), s
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()   # additions only
    assert callable(_lib.boot_partner) and callable(_lib.swap_triples) and callable(_lib.swap_temp_bytes)
    assert int(re.search(r"#define MKE_SWAP_TILE (\d+)", h).group(1)) == _lib.SWAP_TILE


def test_struct_fields_match_header():
    from multike_amd import _lib
    body = re.search(r"typedef struct mke_swap_args \{(.*?)\} mke_swap_args", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\**\s*(\w+)\s*(?=[;,])", body) == [f for f, _ in _lib.SwapArgs._fields_]
    # the types too: a pointer is a void pointer, the sizes are 64-bit, the two switches are ints
    kinds = dict(_lib.SwapArgs._fields_)
    for f in ("n", "n_entities", "capacity", "temp_bytes"):
        assert kinds[f] is C.c_int64 and re.search(r"int64_t[^;]*\b%s\b" % f, body), f
    for f in ("heads_only", "flags"):
        assert kinds[f] is C.c_int and re.search(r"\bint %s;" % f, body), f
    assert all(k is C.c_void_p for f, k in kinds.items() if f not in ("n", "n_entities", "capacity", "temp_bytes", "heads_only", "flags"))


def _args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(h=fake, p=fake, t=fake, n=100, partner=fake, n_entities=50, weight=None, heads_only=0, out_h=fake, out_p=fake,
                out_t=fake, out_w=None, capacity=200, count=fake, temp=fake, temp_bytes=1 << 20, flags=0)
    base.update(over)
    return _lib.SwapArgs(**base)


def test_swap_triples_argument_errors(lib):
    fake = C.c_void_p(0x1000)

    def call(want, text, **over):
        assert lib.mke_swap_triples(C.byref(_args(**over)), None) == want, over
        msg = lib.mke_last_error().decode()
        assert msg.startswith("mke_swap_triples: ") and text in msg, (over, msg)

    assert lib.mke_swap_triples(None, None) == -1 and lib.mke_last_error().decode() == "mke_swap_triples: NULL args"
    for name in ("h", "p", "t", "partner", "out_h", "out_p", "out_t", "count", "temp"):
        call(-1, "NULL pointer", **{name: None})
    call(-2, "n must be in [0, 2^31)", n=-1)
    call(-2, "n must be in [0, 2^31)", n=1 << 31)
    call(-2, "capacity < 0", capacity=-1)
    call(-2, "n_entities must be in [0, 2^31)", n_entities=-1)
    call(-1, "weight and out_w are both NULL or both set", weight=fake)
    call(-1, "weight and out_w are both NULL or both set", out_w=fake)
    call(-3, "unknown flags 1", flags=1)
    call(-3, "heads_only must be 0 or 1, got 2", heads_only=2)
    call(-3, "heads_only must be 0 or 1, got -1", heads_only=-1)
    need = lib.mke_swap_temp_bytes(C.c_int64(100))
    assert need >= 2 * 8 * (100 // 64 + 2)                                  # at least the tile counts and their scan
    call(-2, "below mke_swap_temp_bytes", temp_bytes=need - 1)
    call(-2, "below mke_swap_temp_bytes", temp_bytes=0)
    call(-2, "8-byte aligned", temp=C.c_void_p(0x1004), temp_bytes=need)
    assert lib.mke_swap_temp_bytes(C.c_int64(-1)) == -2 and lib.mke_last_error().decode().startswith("mke_swap_temp_bytes: ")
    assert lib.mke_swap_temp_bytes(C.c_int64(1 << 31)) == -2
    assert lib.mke_swap_temp_bytes(C.c_int64(0)) > 0
    assert lib.mke_swap_temp_bytes(C.c_int64(1 << 20)) >= 2 * 8 * ((1 << 14) + 1)


def test_swap_of_no_triples_is_no_launch(lib):
    """n = 0 needs no input, output or scratch pointer: nothing is walked and no kernel is launched.  count[0] = 0 is written by
    a memset enqueued on the stream, the one thing the call asks of the runtime — so with no GPU the return is that runtime's
    error (> 0, message prefixed), never an argument error; tests/test_boot_exact_gpu.py reads the zero back."""
    empty = dict(n=0, h=None, p=None, t=None, partner=None, out_h=None, out_p=None, out_t=None, temp=None, temp_bytes=0, capacity=0)
    assert lib.mke_swap_triples(C.byref(_args(count=None, **empty)), None) == -1           # ... but it does need `count`
    assert "NULL pointer (count)" in lib.mke_last_error().decode()
    import torch
    if torch.cuda.is_available():
        count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        assert lib.mke_swap_triples(C.byref(_args(count=C.c_void_p(count.data_ptr()), **empty)), None) == 0
        assert int(count.item()) == 0
    else:
        rc = lib.mke_swap_triples(C.byref(_args(**empty)), None)
        assert rc >= 0 and (rc == 0 or lib.mke_last_error().decode().startswith("mke_swap_triples: memset: "))


def test_boot_partner_argument_errors(lib):
    fake = C.c_void_p(0x1000)
    call = lambda n_a=10, n_b=10, n_ent=30, m=fake, a=fake, b=fake, out=fake: lib.mke_boot_partner(
        m, a, C.c_int64(n_a), b, C.c_int64(n_b), out, C.c_int64(n_ent), None)
    for kw in (dict(n_a=-1), dict(n_b=-1), dict(n_a=1 << 31), dict(n_b=1 << 31)):
        assert call(**kw) == -2 and lib.mke_last_error().decode() == "mke_boot_partner: bad n_a / n_b", kw
    for kw in (dict(n_ent=-1), dict(n_ent=1 << 31)):
        assert call(**kw) == -2 and lib.mke_last_error().decode().startswith("mke_boot_partner: n_entities"), kw
    for kw in (dict(m=None), dict(a=None), dict(b=None), dict(out=None), dict(out=None, n_a=0)):
        assert call(**kw) == -1 and lib.mke_last_error().decode() == "mke_boot_partner: NULL pointer", kw
    assert call(n_ent=0, out=None, n_a=0, m=None, a=None) == 0                  # an empty table: nothing to fill


def test_oracle_on_a_hand_written_list():
    #          0   1   2   3   4   5   6   7
    table = [-1,  5, -1,  6, -1,  1,  3, -1]                # links 1 <-> 5 and 3 <-> 6
    triples = [(1, 10, 3),        # both ends linked: head form first, then tail form, never (5, 10, 6)
               (3, 11, 3),        # a linked self-loop: two entries, each with ONE end replaced
               (0, 12, 2),        # unlinked
               (2, 13, 5),        # tail only
               (6, 14, 7),        # head only
               (-1, 15, 8)]       # ids outside the table count as unlinked
    h, p, t = (np.array(c) for c in zip(*triples))
    rows, w = BO.swap(h, p, t, table)
    assert w is None and rows.dtype == np.int32
    assert rows.tolist() == [[5, 10, 3], [1, 10, 6], [6, 11, 3], [3, 11, 6], [2, 13, 1], [3, 14, 7]]
    assert np.array_equal(BO.swap_vector(h, p, t, table)[0], rows)
    heads, _ = BO.swap(h, p, t, table, heads_only=True)       # the third column is a value id: 3, 5 there are not entities
    assert heads.tolist() == [[5, 10, 3], [6, 11, 3], [3, 14, 7]]
    assert np.array_equal(BO.swap_vector(h, p, t, table, heads_only=True)[0], heads)
    weight = np.arange(8, dtype=np.float32) / 8
    rows_w, w = BO.swap(h, p, t, table, weight=weight)
    assert np.array_equal(rows_w, rows) and w.dtype == np.float32
    assert w.tolist() == [1 / 8, 3 / 8, 3 / 8, 3 / 8, 5 / 8, 6 / 8]          # the weight of the entity that was replaced
    assert np.array_equal(BO.swap_vector(h, p, t, table, weight=weight)[1], w)
    # the link table: -1 entries, a match past the columns and ids outside the table leave no trace
    got = BO.partner([1, -1, 0, 7, 2], ids_a=[4, 5, 6, 7, 9], ids_b=[10, 11, 12], n_entities=12)
    want = np.full(12, -1)
    want[4], want[11], want[6], want[10] = 11, 4, 10, 6                         # row 3: match 7 >= n_b; row 4: ids 9 -> 12, 12 is outside
    assert got.tolist() == want.tolist()


def _random_kgs(seed, n1=40, n2=36, n_rel=5, per=4):
    """Duplicate-free id triples of two KGs with disjoint entity ids ([0, n1) and [n1, n1 + n2)) and a one-to-one link map."""
    rng = np.random.default_rng(seed)
    def triples(lo, hi, n):
        return sorted({(int(rng.integers(lo, hi)), int(rng.integers(0, n_rel)), int(rng.integers(lo, hi))) for _ in range(n)})
    t1, t2 = triples(0, n1, n1 * per), triples(n1, n1 + n2, n2 * per)
    m = min(n1, n2) // 2
    links = list(zip(rng.permutation(n1)[:m].tolist(), (n1 + rng.permutation(n2)[:m]).tolist()))
    return t1, t2, links, n1 + n2


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_equals_the_host_swapping_as_a_set(seed):
    from multike_amd.base.kgs import (KG, generate_sup_attribute_triples, generate_sup_relation_triples, swap_attribute_triples,
                                      swap_relation_triples)
    t1, t2, links, n_ent = _random_kgs(seed)
    assert any(h == t for h, _, t in t1 + t2) or seed != 0                 # seed 0 holds self-loops
    m12, m21 = dict(links), {b: a for a, b in links}
    table = BO.partner(np.arange(len(links)), [a for a, _ in links], [b for _, b in links], n_ent)
    assert all(table[a] == b and table[b] == a for a, b in links) and (table >= 0).sum() == 2 * len(links)
    as_set = lambda rows: {tuple(r) for r in rows.tolist()}
    outs = []
    for tri, link_map in ((t1, m12), (t2, m21)):
        h, p, t = (np.array(c) for c in zip(*tri))
        rows, _ = BO.swap(h, p, t, table)
        assert as_set(rows) == swap_relation_triples(set(tri), link_map)
        assert len(as_set(rows)) == len(rows)                              # disjoint KG ids: a swapped triple arises once
        heads, _ = BO.swap(h, p, t, table, heads_only=True)                # the same triples read as (entity, attribute, value)
        assert as_set(heads) == swap_attribute_triples(set(tri), link_map) and len(as_set(heads)) == len(heads)
        outs.append((rows, heads))
    # one walk over KG1 ++ KG2 is the two walks one after the other, and they are generate_sup_*'s two sets
    h, p, t = (np.array(c) for c in zip(*(t1 + t2)))
    both, _ = BO.swap(h, p, t, table)
    assert np.array_equal(both, np.concatenate([outs[0][0], outs[1][0]]))
    kg1, kg2 = KG(t1, []), KG(t2, [])
    new1, new2 = generate_sup_relation_triples(links, kg1.rt_dict, kg1.hr_dict, kg2.rt_dict, kg2.hr_dict)
    assert as_set(both[:len(outs[0][0])]) == new1 and as_set(both[len(outs[0][0]):]) == new2
    heads, _ = BO.swap(h, p, t, table, heads_only=True)
    assert np.array_equal(heads, np.concatenate([outs[0][1], outs[1][1]]))
    a1, a2 = KG([], t1), KG([], t2)
    new1, new2 = generate_sup_attribute_triples(links, a1.av_dict, a2.av_dict)
    assert as_set(heads[:len(outs[0][1])]) == new1 and as_set(heads[len(outs[0][1]):]) == new2
    # the product's own host form (the host() side of a device-built list) is the same walk
    from multike_amd.base.bootstrap import swap_host
    weight = np.random.default_rng(seed).random(n_ent).astype(np.float32)
    for heads_only in (False, True):
        rows, w = BO.swap(h, p, t, table, heads_only=heads_only, weight=weight)
        got, got_w = swap_host(h, p, t, table, heads_only, weight)
        assert np.array_equal(got, rows) and np.array_equal(got_w.astype(np.float32), w)
        assert swap_host(h, p, t, table, heads_only)[1] is None


def test_hyper_parameters_and_the_sharded_driver():
    from multike_amd import _lib
    from multike_amd.base.bootstrap import bootstrap_options
    from multike_amd.distributed_run import _ShardedMixin
    from multike_amd.utils import default_args
    d = default_args()
    assert (d.bootstrap_freq, d.bootstrap_start, d.bootstrap_threshold, d.bootstrap_csls, d.bootstrap_view, d.bootstrap_weighted) == \
        (0, 10, None, 0, None, 0)
    assert bootstrap_options(d) is None                                        # off by default ...
    assert bootstrap_options(default_args(bootstrap_weighted=1, bootstrap_csls=10)) is None     # ... and nothing is looked at
    bare = default_args()
    for k in [k for k in vars(bare) if k.startswith("bootstrap_")]:
        delattr(bare, k)
    assert bootstrap_options(bare) is None                                     # the keys absent: off
    assert bootstrap_options(default_args(bootstrap_freq=5)) == (5, 10, None, 0, None, False)
    assert bootstrap_options(default_args(bootstrap_freq=5, bootstrap_start=3, bootstrap_threshold=0.5, bootstrap_csls=10,
                                          bootstrap_view="rv")) == (5, 3, 0.5, 10, "rv", False)
    with pytest.raises(_lib.MultiKEHipError, match="bootstrap_weighted and bootstrap_csls"):
        bootstrap_options(default_args(bootstrap_freq=5, bootstrap_weighted=1, bootstrap_csls=10))
    with pytest.raises(_lib.MultiKEHipError, match="bootstrap_view"):
        bootstrap_options(default_args(bootstrap_freq=5, bootstrap_view="best"))
    with pytest.raises(_lib.MultiKEHipError, match="bootstrap_threshold is NaN"):
        bootstrap_options(default_args(bootstrap_freq=5, bootstrap_threshold=float("nan")))
    with pytest.raises(_lib.MultiKEHipError, match="bootstrap_freq"):
        _ShardedMixin()._init_sharded(None, default_args(bootstrap_freq=10), None, 0, 2)       # refused before any data is touched


def test_host_surface_refuses_before_the_device():
    import torch
    from multike_amd import _lib
    from multike_amd.base.bootstrap import bootstrap_links, partner_table, swap_triples
    e1, e2 = np.ones((5, 8), dtype=np.float32), np.ones((4, 8), dtype=np.float32)
    ids1, ids2 = np.arange(5), np.arange(5, 9)
    with pytest.raises(_lib.MultiKEHipError, match="match has 4 rows, ids1 5"):
        partner_table(np.zeros(4, dtype=np.int32), ids1, ids2, 9)
    with pytest.raises(_lib.MultiKEHipError, match="n_entities"):
        partner_table(np.zeros(5, dtype=np.int32), ids1, ids2, -1)
    with pytest.raises(_lib.MultiKEHipError, match="1-D integer"):
        partner_table(np.zeros(5, dtype=np.float32), ids1, ids2, 9)
    with pytest.raises(_lib.MultiKEHipError, match="choose one re-scoring"):
        bootstrap_links(e1, e2, ids1, ids2, 9, csls_k=10, sinkhorn=(4, 0.1))
    with pytest.raises(_lib.MultiKEHipError, match="threshold is NaN"):
        bootstrap_links(e1, e2, ids1, ids2, 9, threshold=float("nan"))
    with pytest.raises(_lib.MultiKEHipError, match="5 / 4 rows, 5 / 3 entity ids"):
        bootstrap_links(e1, e2, ids1, ids2[:3], 9)
    cols = np.zeros((6, 3), dtype=np.int64)
    with pytest.raises(_lib.MultiKEHipError, match="partner must be"):
        swap_triples(cols, np.zeros(9, dtype=np.int32))
    with pytest.raises(_lib.MultiKEHipError, match="weight must be"):
        swap_triples(cols, torch.zeros(9, dtype=torch.int32), weight=torch.zeros(8))

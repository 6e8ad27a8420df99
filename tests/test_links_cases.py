"""The definition of mke_links_edit (include/multike_links.h) as tests/links_oracle.py restates it, on the cases of
tests/links_cases.py: every rule and every counter is reached, both counter identities and the one-to-one-ness of the result
hold, subtly wrong edits each fail; the float64 cases of the GPU tests keep every value farther from `retain` than the bound of
the device's rounding; and what needs no device of the library: its generated module, its layout, its symbols, its refusals,
the checked hyper-parameters."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import links_cases as LC
import links_oracle as LO
import mutual_oracle as MO

GRID = [(kpad, metric, terms) for kpad in LC.KPADS for metric in (LO.INNER, LO.EUCLIDEAN) for terms in (False, True)]


def _edit(c, **over):
    kw = dict(held=c["held"], match=c["match"], S=c["S"], retain=c["retain"], new_score=c["new_score"])
    kw.update(over)
    return LO.edit(**kw)


def _held_count(c):
    return int((LO.clean(c["held"], c["n_b"]) >= 0).sum())


def _big(metric=LO.EUCLIDEAN, terms=True, sizes=(257, 257), **kw):
    return LC.exact_case(np.random.default_rng(5), *sizes, 48, metric, terms, **kw)


@pytest.mark.parametrize("metric", [LO.INNER, LO.EUCLIDEAN])
@pytest.mark.parametrize("terms", [False, True])
def test_every_rule_and_every_counter_is_reached(metric, terms):
    c = _big(metric, terms)
    out, score, counts = _edit(c)
    n = dict(zip(LO.COUNTS, counts.tolist()))
    assert all(v > 0 for k, v in n.items() if k != "gold"), n
    h, m = LO.clean(c["held"], 257), LO.clean(c["match"], 257)
    assert (c["held"] != h).any() and (c["match"] != m).any()                  # entries outside [0, n_b) in both inputs
    rows, cols = LC.old_links(c["held"], c["match"], 257)
    vals = c["S"][rows, cols]
    # expired by NaN: a NaN in a row of a (not with euclidean: max(NaN, 0) = 0 there, as in the sweep), a NaN row term
    assert (np.isnan(vals) & (out[rows] < 0)).sum() == int(metric == LO.INNER) + int(terms)
    assert (vals < c["retain"]).any() and (vals == np.float32(c["retain"])).any() and (vals > c["retain"]).any()
    assert (out[rows[vals == np.float32(c["retain"])]] >= 0).all()            # >= keeps the value itself
    # displaced through the row (its own new pair is another column) and through the column (another row took it)
    own = (m >= 0) & (h >= 0) & (m != h)
    taken = np.isin(h, m[m >= 0]) & (m < 0) & (h >= 0)
    assert own.any() and taken.any() and n["displaced"] == own.sum() + taken.sum() and (out[taken] == -1).all()
    assert ((m >= 0) & (m == h)).sum() == n["refound"] > 0                     # a row whose new pair equals its held link
    # score: the value of a kept link, new_score copied bit for bit, 0 elsewhere
    kept = rows[out[rows] >= 0]
    assert np.array_equal(score[kept], c["S"][kept, out[kept]]) and np.array_equal(score[m >= 0].view(np.uint32), c["new_score"][m >= 0].view(np.uint32))
    assert (score[out < 0].view(np.uint32) == 0).all()


@pytest.mark.parametrize("kpad,metric,terms", GRID[::5])
def test_identities_and_one_to_one_on_the_cases_of_the_gpu_tests(kpad, metric, terms):
    for c in LC.exact_cases(kpad, metric, terms):
        for retain in (c["retain"], -np.inf, np.inf):
            out, score, counts = _edit(c, retain=retain)
            assert LO.one_to_one(out) and ((out >= -1) & (out < c["n_b"])).all()
            assert counts[0] == counts[2] + counts[4] == (out >= 0).sum()
            assert _held_count(c) == counts[3] + counts[4] + counts[5] + counts[6]
            assert retain != np.inf or counts[4] == 0                           # no value is +inf


def test_the_two_ends_of_the_rule():
    c = _big(poison=False)
    none = np.full(257, -1, dtype=np.int32)
    out, _, counts = _edit(c, held=none)
    assert np.array_equal(out, LO.clean(c["match"], 257)) and counts[2] == counts[0] and counts[3:].sum() == 0
    out, score, counts = _edit(c, match=none, retain=-np.inf)
    assert np.array_equal(out, LO.clean(c["held"], 257)) and counts[4] == counts[0] == _held_count(c) and counts[[2, 3, 5, 6]].sum() == 0
    assert np.array_equal(score[out >= 0], c["S"][out >= 0, out[out >= 0]])
    with pytest.raises(ValueError):
        _edit(c, retain=np.nan)


@pytest.mark.parametrize("sizes", [(40, 71), (130, 33), (0, 5), (5, 0), (0, 0)])
def test_other_shapes_and_empty_sides(sizes):
    n_a, n_b = sizes
    if min(sizes) == 0:
        out, score, counts = LO.edit(np.arange(n_a), np.arange(n_a)[::-1], np.zeros(sizes, dtype=np.float32))
        assert (out == -1).all() and (score == 0).all() and (counts == 0).all() and len(out) == n_a
        return
    c = _big(sizes=sizes)
    out, _, counts = _edit(c)
    assert LO.one_to_one(out) and out.max() < n_b and counts[2] > 0 and counts[4] > 0 and counts[5] > 0
    assert counts[0] == counts[2] + counts[4] and _held_count(c) == counts[3:].sum()


def test_a_mutual_decodes_new_pair_has_no_larger_old_link_at_either_end():
    """Why rule 1 compares nothing: the pairs of the mutual decoder on S are each other's best on S, so whatever the link set
    held at either end is worth no more on the same S."""
    rng = np.random.default_rng(11)
    S = np.round(rng.standard_normal((60, 75)) * 4) / 4                         # ties in most rows
    match, _ = MO.pairs(S)
    held = np.full(60, -1)
    held[rng.permutation(60)[:40]] = rng.permutation(75)[:40]
    inv = {int(j): i for i, j in enumerate(held) if j >= 0}
    assert (match >= 0).sum() > 10
    for i in np.nonzero(match >= 0)[0]:
        j = match[i]
        assert held[i] < 0 or S[i, held[i]] <= S[i, j]
        assert j not in inv or S[inv[j], j] <= S[i, j]


def _wrong(c, bug):
    """The edit again, vectorised, with one mistake (bug None: none)."""
    n_a, n_b = c["n_a"], c["n_b"]
    h, m = LO.clean(c["held"], n_b), LO.clean(c["match"], n_b)
    S = c["S"]
    if bug == "the CSLS term of the wrong side":
        S = LO.values(c["a"][:, :c["kpad"]], c["b"][:, :c["kpad"]], c["metric"], c["sq_a"], c["sq_b"], c["terms"][::-1]).astype(np.float32)
    taken = np.zeros(n_b + 1, dtype=bool)
    if bug != "column test forgotten":
        taken[m[m >= 0]] = True
    new = m >= 0
    old = ~new & (h >= 0) & ~taken[np.maximum(h, 0)]
    s = S[np.arange(n_a), np.maximum(h, 0)]
    with np.errstate(invalid="ignore"):
        keep = old & ((s > c["retain"]) if bug == "> for >=" else (s >= c["retain"]))
    if bug == "NaN kept":
        keep |= old & np.isnan(s)
    out = np.where(new, m, np.where(keep, h, -1)).astype(np.int32)
    score = np.where(new, c["new_score"], np.where(keep, s, 0)).astype(np.float32)
    refound = new & (m == h) if bug != "re-found counted as displaced" else np.zeros(n_a, dtype=bool)
    displaced = (new & (h >= 0) & ~refound) | (~new & (h >= 0) & ~old)
    counts = [(out >= 0).sum(), (out == np.arange(n_a)).sum(), new.sum(), refound.sum(), keep.sum(), displaced.sum(), (old & ~keep).sum()]
    if bug == "out of range taken as it is":
        out = np.where(c["match"] >= 0, c["match"], out).astype(np.int32)
    return out, score, np.array(counts, dtype=np.int64)


def _same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) and np.array_equal(x[2], y[2])


BUGS = ("column test forgotten", "> for >=", "re-found counted as displaced", "NaN kept", "the CSLS term of the wrong side",
        "out of range taken as it is")


def test_the_vectorised_edit_agrees_and_each_wrong_one_fails():
    cases = [_big(LO.EUCLIDEAN, True), _big(LO.INNER, True), _big(sizes=(130, 33)), _big(sizes=(40, 71))] + LC.exact_cases(16, LO.INNER, True)
    assert all(_same(_wrong(c, None), _edit(c)) for c in cases)
    for bug in BUGS:
        assert not _same(_wrong(cases[0], bug), _edit(cases[0])), bug
    # the column test also guards the one-to-one-ness of the result
    assert not LO.one_to_one(_wrong(cases[0], "column test forgotten")[0])


@pytest.mark.parametrize("kpad,metric,terms", GRID)
def test_float64_cases_stay_away_from_retain(kpad, metric, terms):
    """The CPU half of the float64 tier of tests/test_links_exact_gpu.py: no value that decides lies within the device's
    rounding bound of `retain`, so kept / expired is exact there too; and the bound is of the size its derivation says."""
    for c in LC.unit_cases(kpad, metric, terms):
        assert c["margin"] > 2 * c["bound"] and np.isfinite(c["bound"]), (c["n_a"], c["margin"], c["bound"])
        rows, cols = LC.old_links(c["held"], c["match"], c["n_b"])
        if len(rows) > 4:
            vals = c["S"][rows, cols]
            assert (vals > c["retain"]).any() and (vals < c["retain"]).any()
        assert c["bound"] < (kpad // 16 + 4 + 6) * LC.U * (8 if terms else 4)            # a few u per rounding, values of size <= 4


def test_links_abi_module_layout_and_symbols(tmp_path):
    import abi_header as ah
    from multike_amd import _abi, _abi_keyed, _abi_links, _abi_thin, _lib
    header = os.path.join(os.path.dirname(ah.HEADER), "multike_links.h")
    out = tmp_path / "_abi_links.py"
    subprocess.check_call([sys.executable, ah.GENERATOR, header, str(out)])
    assert out.read_bytes() == open(os.path.join(os.path.dirname(ah.GENERATED), "_abi_links.py"), "rb").read(), \
        "run tools/gen_abi.py include/multike_links.h multike_amd/_abi_links.py and commit it"
    assert list(_abi_links.FUNCTIONS) == ["mke_links_last_error", "mke_links_version", "mke_links_edit"]
    assert not set(_abi_links.FUNCTIONS) & (set(_abi.FUNCTIONS) | set(_abi_thin.FUNCTIONS) | set(_abi_keyed.FUNCTIONS))
    text = open(header).read()
    assert "#include" not in text.replace("#include <stdint.h>", "")                      # the header stands alone
    assert (_abi_links.LINKS_E_NULL, _abi_links.LINKS_E_SHAPE, _abi_links.LINKS_E_UNSUPPORTED, _abi_links.LINKS_E_RANGE) == \
        (_abi.E_NULL, _abi.E_SHAPE, _abi.E_UNSUPPORTED, _abi.E_RANGE)
    assert (_abi_links.LINKS_METRIC_INNER, _abi_links.LINKS_METRIC_EUCLIDEAN) == (_abi.METRIC_INNER, _abi.METRIC_EUCLIDEAN)
    assert _abi_links.LINKS_COUNTS == len(LO.COUNTS)
    # a C compiler's sizeof / offsetof of the header (given to the shared helper under the name it includes)
    (tmp_path / "inc").mkdir()
    (tmp_path / "inc" / "multike_hip.h").write_text(text)
    st = _abi_links.mke_links_args
    consts = ah.header_constant_names(text)
    assert ah.header_struct_names(text) == ["mke_links_args"] and len(consts) == 9
    sizes, fields, values = ah.c_layout(tmp_path, {"mke_links_args": [f for f, _ in st._fields_]}, consts, include_dir=str(tmp_path / "inc"))
    assert sizes == {"mke_links_args": C.sizeof(st)} and len(fields) == len(st._fields_) == 20
    assert all(fields["mke_links_args", f] == (getattr(st, f).offset, getattr(st, f).size) for f, _ in st._fields_)
    assert values == {"MKE_" + k: v for k, v in vars(_abi_links).items() if k.isupper() and isinstance(v, int)}
    if not os.path.exists(_lib.LINKS_SO_PATH):
        import __graft_entry__ as g
        g.build()
    assert ah.exported_symbols(_lib.LINKS_SO_PATH) == set(_abi_links.FUNCTIONS)
    L = _lib.links_lib()
    for name, (restype, argtypes) in _abi_links.FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert L.mke_links_version() == _abi_links.LINKS_VERSION == 1
    assert _lib.SYMBOLS == tuple(_abi.FUNCTIONS)                               # the main library's list does not know the new one


def test_argument_errors_come_before_any_launch():
    """No device is needed: every refusal is made before anything is enqueued (the pointers below are never read)."""
    from multike_amd import _abi_links as al, _lib
    L = _lib.links_lib()
    P = 0x10000                                                                # a non-NULL address nobody dereferences

    def edit(**over):
        kw = dict(held=P, match=P + 0x1000, n_a=100, n_b=90, a=P, lda=16, b=P, ldb=16, kpad=16, metric=0, sq_a=None, sq_b=None,
                  csls_row=None, csls_col=None, retain=0.5, new_score=None, inv=P, out=P + 0x2000, score=None, counts=P)
        kw.update(over)
        return L.mke_links_edit(C.byref(al.mke_links_args(**kw)), None), L.mke_links_last_error()

    assert L.mke_links_edit(None, None) == al.LINKS_E_NULL and b"NULL args" in L.mke_links_last_error()
    for kw in (dict(n_a=-1), dict(n_b=-1), dict(n_a=0x7FFFFF01), dict(n_b=0x7FFFFF01), dict(kpad=0), dict(kpad=24), dict(kpad=336, lda=336, ldb=336),
               dict(lda=12), dict(ldb=18), dict(kpad=32), dict(lda=20, ldb=20, kpad=32)):
        rc, msg = edit(**kw)
        assert rc == al.LINKS_E_SHAPE and msg.startswith(b"mke_links_edit: "), (kw, rc, msg)
    for kw in (dict(kpad=144, lda=144, ldb=144), dict(kpad=224, lda=224, ldb=224), dict(metric=2), dict(metric=-1)):
        rc, msg = edit(**kw)
        assert rc == al.LINKS_E_UNSUPPORTED, (kw, rc, msg)
    assert b"unknown metric 2" in edit(metric=2)[1] and b"unsupported kpad 144" in edit(kpad=144, lda=144, ldb=144)[1]
    for name in ("held", "match", "a", "b", "inv", "out", "counts"):
        rc, msg = edit(**{name: None})
        assert rc == al.LINKS_E_NULL and b"NULL pointer" in msg, name
    for kw in (dict(metric=1), dict(metric=1, sq_a=P), dict(metric=1, sq_b=P)):
        rc, msg = edit(**kw)
        assert rc == al.LINKS_E_NULL and b"euclidean needs sq_a and sq_b" in msg, kw
    for kw in (dict(csls_row=P), dict(csls_col=P)):
        rc, msg = edit(**kw)
        assert rc == al.LINKS_E_NULL and b"both NULL or both set" in msg, kw
    rc, msg = edit(retain=float("nan"))
    assert rc == al.LINKS_E_RANGE and b"NaN" in msg
    for out in (P, P + 4 * 99, P - 4 * 99):                                    # out overlapping held, at either end
        rc, msg = edit(out=out)
        assert rc == al.LINKS_E_UNSUPPORTED and b"overlaps held" in msg, out
    # a wrong argument is reported even when a side is empty; what only a launch would read is not looked at then
    assert edit(n_a=0, metric=7)[0] == al.LINKS_E_UNSUPPORTED and edit(n_b=0, retain=float("nan"))[0] == al.LINKS_E_RANGE
    assert edit(n_a=0, counts=None)[0] == al.LINKS_E_NULL


def test_hyper_parameters():
    from multike_amd._lib import MultiKEHipError
    from multike_amd.base.bootstrap import bootstrap_options
    from multike_amd.utils import default_args
    d = default_args()
    assert d.bootstrap_accumulate == 0 and d.bootstrap_retain is None
    assert bootstrap_options(d) is None
    assert bootstrap_options(default_args(bootstrap_accumulate=1)) is None                # without bootstrap_freq: ignored
    assert bootstrap_options(default_args(bootstrap_accumulate=1, bootstrap_retain=float("nan"))) is None
    six = bootstrap_options(default_args(bootstrap_freq=3))
    assert six == (3, 10, None, 0, None, False)
    assert bootstrap_options(default_args(bootstrap_freq=3, bootstrap_accumulate=0, bootstrap_retain=0.4)) == six
    a = default_args(bootstrap_freq=3)
    del a.bootstrap_accumulate, a.bootstrap_retain                                       # the keys absent, as in an older args.json
    assert bootstrap_options(a) == six
    assert bootstrap_options(default_args(bootstrap_freq=3, bootstrap_accumulate=1)) == six + (True, None)
    assert bootstrap_options(default_args(bootstrap_freq=3, bootstrap_accumulate=1, bootstrap_threshold=0.7)) == (3, 10, 0.7, 0, None, False, True, 0.7)
    assert bootstrap_options(default_args(bootstrap_freq=3, bootstrap_accumulate=1, bootstrap_threshold=0.7, bootstrap_retain=0.25,
                                          bootstrap_csls=5)) == (3, 10, 0.7, 5, None, False, True, 0.25)
    assert bootstrap_options(default_args(bootstrap_freq=3, bootstrap_accumulate=1, bootstrap_retain=float("-inf")))[7] == float("-inf")
    for acc in (0, 1):
        with pytest.raises(MultiKEHipError, match="bootstrap_retain is NaN"):
            bootstrap_options(default_args(bootstrap_freq=3, bootstrap_accumulate=acc, bootstrap_retain=float("nan")))

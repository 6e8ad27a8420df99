"""The evaluator's eight entry points against a table of argument vectors (eval_args_cases.py) without a GPU: every fault
the operand checks know, alone and in every pair, and the n == 0 vectors.  Return code and mke_last_error text are those
recorded from the build before the five copies of the checks became one helper (tests/golden/record_eval_args.py ->
tests/golden/eval_args_golden.json): same code, same text, same winner when two arguments are wrong at once, same early
returns.  Validation runs before any HIP call; pointers are dummy non-NULL addresses."""
import json
import os

import pytest

import eval_args_cases as ea
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    with open(os.path.join(GOLDEN, "eval_args_golden.json")) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(golden):
    ids = [f"{e}/{vid}" for e in ea.ENTRY for vid, _ in ea.vectors(e)]
    assert len(ids) == len(set(ids)) and set(ids) == set(golden)
    assert len(ea.ENTRY) == 8
    for e, d in ea.ENTRY.items():                         # every single fault, and every pair of faults of different arguments
        assert {f"{e}/{s}" for s in d["faults"]} <= set(golden)
        for (ka, a), (kb, b) in ((x, y) for x in d["faults"].items() for y in d["faults"].items() if x[0] < y[0]):
            if not set(a) & set(b) and {ka, kb} != {"row_term_only", "col_term_only"}:
                assert f"{e}/{ka}+{kb}" in golden or f"{e}/{kb}+{ka}" in golden


@pytest.mark.parametrize("entry", list(ea.ENTRY))
def test_code_and_text_are_the_parents(golden, entry):
    wrong = []
    for vid, over in ea.vectors(entry):
        # only a refused vector is ever sent: one with rows that the parent accepted would launch on the dummy addresses
        assert golden[f"{entry}/{vid}"][0] < 0 or not ea.has_rows(entry, over), vid
        got = list(ea.run(entry, over))
        if got != golden[f"{entry}/{vid}"]:
            wrong.append((vid, got, golden[f"{entry}/{vid}"]))
    assert not wrong, f"{len(wrong)} vectors differ, the first: {wrong[:5]}"


def test_the_shared_faults_are_refused_with_the_expected_codes(golden):
    """The recorded table itself says what the issue says it must: spot checks of codes against the header's meaning."""
    assert golden["mke_align_rank/zero:n1_0_null"] == [0, ""]
    assert golden["mke_align_rank/kpad144"] == [-3, "unsupported kpad 144"]
    assert golden["mke_align_rank/na_neg"] == [-2, "bad n1/n2"]
    assert golden["mke_align_rank_ex/na_neg+metric2"][0] == -2 and golden["mke_align_rank_ex/zero:n1_0_metric2"][0] == -3
    for e in ea.STRUCT_OF:
        assert golden[e + "/null_args"][0] == -1 and golden[e + "/kpad144"][0] == -3 and golden[e + "/kpad24"][0] == -2
        assert golden[e + "/metric2"][0] == -3 and golden[e + "/euc_no_sq_a"][0] == -1 and golden[e + "/ld_odd"][0] == -2
        assert golden[e + "/euc_no_sq"][0] == -1
        # the ld check comes before the width check, the kpad form before both: only a composed vector can say so
        assert golden[e + "/kpad144+ld_short"][0] == -2 and golden[e + "/kpad144+ld_odd"][0] == -2
        assert golden[e + "/kpad336+ld_short"][0] == -2 and golden[e + "/kpad336+ld_odd"][0] == -2
    assert golden["mke_align_rank/kpad144+ld_short"][0] == -2
    for e in ea.QUERY_OF:
        assert golden[e + "/temp_short"][0] == -2


def test_alignment_counts_checks_the_row_counts_before_the_operands():
    """Too few columns is refused before the rows are copied, padded or refused for their width (no device needed)."""
    import numpy as np
    from multike_amd import _lib
    from multike_amd.base.alignment import alignment_counts
    wide = _lib.SIM_SELECT_KPADS[-1] + 1
    for kw in ({}, {"metric": "euclidean"}, {"csls_k": 3}):
        with pytest.raises(_lib.MultiKEHipError, match="needs len\\(embed2\\) >= len\\(embed1\\)"):
            alignment_counts(np.ones((5, wide), np.float32), np.ones((3, wide), np.float32), device="cpu", **kw)
    with pytest.raises(_lib.MultiKEHipError, match="exceed the widest"):
        alignment_counts(np.ones((3, wide), np.float32), np.ones((3, wide), np.float32), device="cpu")


def test_rescoring_arguments_are_normalised_in_one_way():
    from multike_amd import _lib
    from multike_amd.base.alignment import _check_rescoring
    assert _check_rescoring(None, None) == (0, None) and _check_rescoring(-3, None) == (0, None)
    assert _check_rescoring(0.5, None) == (0, None) and _check_rescoring(2.7, None) == (2, None)
    assert _check_rescoring(0, (5.0, 1)) == (0, (5, 1.0))
    for bad in ((10, (5, 0.1), None), (0, (5, 0.1), (1, 2))):
        with pytest.raises(_lib.MultiKEHipError, match="sinkhorn and csls_k are both set: choose one re-scoring"):
            _check_rescoring(*bad)
    for st in ((0, 0.1), (1.5, 0.1), (3, 0.0), (3, float("inf"))):
        with pytest.raises(_lib.MultiKEHipError, match="needs iters >= 1 and a finite tau > 0"):
            _check_rescoring(0, st)

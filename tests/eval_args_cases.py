"""Argument vectors of the evaluator's eight entry points (mke_align_rank, mke_align_rank_ex, mke_align_topk_mean, mke_align_lse,
mke_stable_lists and the three *_temp_bytes queries) for tests/test_eval_args_abi.py and tests/golden/record_eval_args.py: every
fault the argument checks know, alone and in every pair, plus the n == 0 vectors.  No GPU: every vector is refused (or returns
at n == 0) before any HIP call, and pointers are dummy non-NULL addresses.  ctypes only.

A fault is a dict of overrides of the entry point's valid base arguments; a value may be a function of the merged vector, so
that faults compose: the base's ld follows kpad, "ld short" is kpad - 16 and "ld odd" kpad + 2 whatever kpad the other fault
of a pair sets (kpad 144 with a short ld pins that the ld check comes before the width check).  A pair merges two faults that
touch different arguments; faults of one argument (the kpad values, the metric codes) are alternatives.
`run(entry, overrides)` returns (rc, text): the return code and, when it is negative, the mke_last_error text (the text of an
earlier call otherwise stays in place and means nothing)."""
import ctypes as C
import itertools

FAKE = 0x1000
BIG = 0x7FFFFF01                       # one past the largest row count the entry points take

# what every sweep client checks about its operands; `a` / `b` name the entry point's own fields
def _shared(n_a, n_b, ld_a, ld_b):
    return {
        "na_neg": {n_a: -1}, "nb_neg": {n_b: -1}, "na_big": {n_a: BIG}, "nb_big": {n_b: BIG},
        "kpad0": {"kpad": 0}, "kpad24": {"kpad": 24}, "kpad336": {"kpad": 336},
        "kpad144": {"kpad": 144},                                  # a multiple of 16 without an instantiation
        "ld_short": {ld_a: lambda v: v["kpad"] - 16}, "ld_odd": {ld_b: lambda v: v["kpad"] + 2},
    }


_LD = lambda v: v["kpad"]              # the base's ld: the width, whichever a fault makes it


def _metric(sq_a, sq_b):
    return {"metric2": {"metric": 2}, "euc_no_sq_a": {"metric": 1, sq_b: FAKE}, "euc_no_sq_b": {"metric": 1, sq_a: FAKE},
            "euc_no_sq": {"metric": 1}}


_TERMS = {"row_term_only": {"csls_row": FAKE}, "col_term_only": {"csls_col": FAKE}}


def _nulls(*fields):
    return {f"null_{f}": {f: None} for f in fields}


ENTRY = {}

ENTRY["mke_align_rank"] = dict(
    base=dict(emb1=FAKE, ld1=_LD, emb2=FAKE, ld2=_LD, kpad=80, n1=100, n2=120, rank=FAKE, ties=FAKE, best=FAKE),
    faults={**_shared("n1", "n2", "ld1", "ld2"), **_nulls("emb1", "emb2", "rank", "best"), "n2_below_n1": {"n2": 99}},
    zeros={"n1_0": {"n1": 0}, "n1_0_null": {"n1": 0, "emb1": None, "emb2": None, "rank": None, "best": None},
           "n2_0": {"n2": 0}, "both_0": {"n1": 0, "n2": 0}, "n1_0_kpad24": {"n1": 0, "kpad": 24}, "n1_0_n2_neg": {"n1": 0, "n2": -1}})

ENTRY["mke_align_rank_ex"] = dict(
    base=dict(emb1=FAKE, ld1=_LD, emb2=FAKE, ld2=_LD, kpad=80, n1=100, n2=120, metric=0, sq1=None, sq2=None, csls_row=None,
              csls_col=None, rank=FAKE, ties=FAKE, best=FAKE),
    faults={**_shared("n1", "n2", "ld1", "ld2"), **_metric("sq1", "sq2"), **_TERMS,
            **_nulls("emb1", "emb2", "rank", "ties", "best"), "n2_below_n1": {"n2": 99}},
    zeros={"n1_0": {"n1": 0}, "n1_0_null": {"n1": 0, "emb1": None, "emb2": None, "rank": None, "ties": None, "best": None},
           "n2_0": {"n2": 0}, "both_0": {"n1": 0, "n2": 0}, "n1_0_metric2": {"n1": 0, "metric": 2}, "n1_0_kpad24": {"n1": 0, "kpad": 24},
           "n1_0_row_term_only": {"n1": 0, "csls_row": FAKE}})

_AB = dict(a=FAKE, lda=_LD, b=FAKE, ldb=_LD, kpad=80, n_a=100, n_b=120, metric=0, sq_a=None, sq_b=None)

ENTRY["mke_align_topk_mean"] = dict(
    base=dict(_AB, k=10, out=FAKE, temp=FAKE, temp_bytes="need"),
    faults={**_shared("n_a", "n_b", "lda", "ldb"), **_metric("sq_a", "sq_b"), **_nulls("a", "b", "out", "temp"),
            "k0": {"k": 0}, "k_high": {"k": 119}, "k_whole_rows_short": {"k": 100, "temp_bytes": 47999}, "temp_short": {"temp_bytes": "need-1"}},
    zeros={"na_0": {"n_a": 0}, "na_0_null": {"n_a": 0, "a": None, "b": None, "out": None, "temp": None, "temp_bytes": 0},
           "nb_0": {"n_b": 0}, "both_0": {"n_a": 0, "n_b": 0}, "na_0_metric2": {"n_a": 0, "metric": 2}, "na_0_kpad24": {"n_a": 0, "kpad": 24},
           "na_0_k0": {"n_a": 0, "k": 0}})

ENTRY["mke_align_lse"] = dict(
    base=dict(_AB, sub_b=None, tau=0.05, out=FAKE, temp=FAKE, temp_bytes="need"),
    faults={**_shared("n_a", "n_b", "lda", "ldb"), **_metric("sq_a", "sq_b"), **_nulls("a", "b", "out", "temp"),
            "tau0": {"tau": 0.0}, "tau_inf": {"tau": float("inf")}, "nb_0": {"n_b": 0}, "temp_short": {"temp_bytes": "need-1"}},
    zeros={"na_0": {"n_a": 0}, "na_0_null": {"n_a": 0, "a": None, "b": None, "out": None, "temp": None, "temp_bytes": 0},
           "both_0": {"n_a": 0, "n_b": 0}, "na_0_metric2": {"n_a": 0, "metric": 2}, "na_0_kpad24": {"n_a": 0, "kpad": 24},
           "na_0_tau0": {"n_a": 0, "tau": 0.0}})

ENTRY["mke_stable_lists"] = dict(
    base=dict(_AB, csls_row=None, csls_col=None, sim_mat=None, ld_sim=0, cut=10, whole_rows=0, sample_cols=0, out_val=FAKE,
              out_col=FAKE, flags=FAKE, temp=FAKE, temp_bytes="need"),
    faults={**_shared("n_a", "n_b", "lda", "ldb"), **_metric("sq_a", "sq_b"), **_TERMS,
            **_nulls("a", "b", "out_val", "out_col", "flags", "temp"),
            "cut0": {"cut": 0}, "cut_high": {"cut": 121}, "sample_neg": {"sample_cols": -1}, "temp_short": {"temp_bytes": "need-1"},
            "given_ld_short": {"sim_mat": FAKE, "ld_sim": 119}},
    zeros={"na_0": {"n_a": 0}, "na_0_null": {"n_a": 0, "a": None, "b": None, "out_val": None, "out_col": None, "flags": None, "temp": None,
                                             "temp_bytes": 0},
           "nb_0": {"n_b": 0}, "both_0": {"n_a": 0, "n_b": 0}, "na_0_metric2": {"n_a": 0, "metric": 2}, "na_0_kpad24": {"n_a": 0, "kpad": 24},
           "na_0_row_term_only": {"n_a": 0, "csls_row": FAKE}, "na_0_given": {"n_a": 0, "sim_mat": FAKE, "kpad": 0}})

_QF = {k: d for k, d in _shared("n_a", "n_b", "lda", "ldb").items() if not k.startswith("ld_")}      # the queries take no ld

ENTRY["mke_align_topk_mean_temp_bytes"] = dict(
    base=dict(n_a=100, n_b=120, kpad=80, k=10),
    faults={**_QF, "k0": {"k": 0}, "k_high": {"k": 119}, "k_2p30": {"n_a": BIG - 1, "n_b": BIG - 1, "k": (1 << 30) + 1}},
    zeros={"valid": {}, "na_0": {"n_a": 0}, "nb_0": {"n_b": 0}, "both_0": {"n_a": 0, "n_b": 0}, "na_0_kpad24": {"n_a": 0, "kpad": 24},
           "whole_rows": {"k": 100}, "large": {"n_a": 60000, "n_b": 60000}})

ENTRY["mke_align_lse_temp_bytes"] = dict(
    base=dict(n_a=100, n_b=120, kpad=80),
    faults={**_QF, "nb_0": {"n_b": 0}},
    zeros={"valid": {}, "na_0": {"n_a": 0}, "both_0": {"n_a": 0, "n_b": 0}, "na_0_kpad24": {"n_a": 0, "kpad": 24},
           "large": {"n_a": 60000, "n_b": 60000}})

ENTRY["mke_stable_lists_temp_bytes"] = dict(
    base=dict(n_a=100, n_b=120, kpad=80, cut=10, whole_rows=0),
    faults={**_QF, "cut0": {"cut": 0}, "cut_high": {"cut": 121}},
    zeros={"valid": {}, "na_0": {"n_a": 0}, "nb_0": {"n_b": 0}, "both_0": {"n_a": 0, "n_b": 0}, "na_0_kpad24": {"n_a": 0, "kpad": 24},
           "whole_rows": {"whole_rows": 1}, "long_cut": {"cut": 120}, "large": {"n_a": 60000, "n_b": 60000}})

QUERY_OF = {"mke_align_topk_mean": ("mke_align_topk_mean_temp_bytes", ("n_a", "n_b", "kpad", "k")),
            "mke_align_lse": ("mke_align_lse_temp_bytes", ("n_a", "n_b", "kpad")),
            "mke_stable_lists": ("mke_stable_lists_temp_bytes", ("n_a", "n_b", "kpad", "cut", "whole_rows"))}
STRUCT_OF = {"mke_align_rank_ex": "AlignArgs", "mke_align_topk_mean": "TopkMeanArgs", "mke_align_lse": "LseArgs",
             "mke_stable_lists": "StableListsArgs"}
_INT64 = ("n1", "n2", "n_a", "n_b")


def vectors(entry):
    """[(id, overrides)] of one entry point: the n == 0 vectors, NULL args where there is a struct, every fault, every pair."""
    e = ENTRY[entry]
    out = [("zero:" + k, v) for k, v in e["zeros"].items()]
    if entry in STRUCT_OF:
        out.append(("null_args", None))
    out += list(e["faults"].items())
    for (ka, a), (kb, b) in itertools.combinations(e["faults"].items(), 2):
        if not set(a) & set(b) and {ka, kb} != set(_TERMS):       # both terms set is no fault: it would launch
            out.append((ka + "+" + kb, {**a, **b}))
    return out


def _query(lib, entry, v):
    name, fields = QUERY_OF.get(entry, (entry, tuple(ENTRY[entry]["base"])))
    return int(getattr(lib, name)(*[(C.c_int64 if f in _INT64 else C.c_int)(v[f]) for f in fields]))


def _call(lib, _lib, entry, over):
    if over is None:
        return getattr(lib, entry)(None, None)
    v = {**ENTRY[entry]["base"], **over}
    v.update({f: x(v) for f, x in v.items() if callable(x)})       # after the merge: kpad is a plain value in every fault
    if entry.endswith("_temp_bytes"):
        return _query(lib, entry, v)
    if entry == "mke_align_rank":
        p = lambda f: C.c_void_p(v[f])
        return lib.mke_align_rank(p("emb1"), C.c_int(v["ld1"]), p("emb2"), C.c_int(v["ld2"]), C.c_int(v["kpad"]), C.c_int64(v["n1"]),
                                  C.c_int64(v["n2"]), p("rank"), p("ties"), p("best"), None)
    if isinstance(v.get("temp_bytes"), str):            # "need" / "need-1": what the query asks for the base's shape
        need = _query(lib, entry, {f: x for f, x in ENTRY[entry]["base"].items() if not callable(x)})
        assert need > 0
        v["temp_bytes"] = need - (1 if v["temp_bytes"] == "need-1" else 0)
    return getattr(lib, entry)(C.byref(getattr(_lib, STRUCT_OF[entry])(**v)), None)


def has_rows(entry, over):
    """Whether the vector would launch if it passed every check: an entry point that launches, with n1 / n_a > 0."""
    return not entry.endswith("_temp_bytes") and over is not None and over.get("n1") != 0 and over.get("n_a") != 0


def run(entry, over):
    """(rc, text) of one vector on the library that multike_amd loads."""
    from multike_amd import _lib
    lib = _lib.lib()
    rc = int(_call(lib, _lib, entry, over))
    return rc, (lib.mke_last_error().decode() if rc < 0 else "")

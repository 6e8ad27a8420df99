#!/usr/bin/env python3
"""Generate tests/golden/csls_golden.npz by EXECUTING THE REFERENCE'S OWN evaluator with CSLS and metrics.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_csls_golden.py [--reference /root/reference]

The reference's `code/base/similarity.py` (`sim(..., csls_k=k)`, `calculate_nearest_k`) and `code/base/alignment.py`
(`greedy_alignment(..., csls_k=k, accurate=True)`, one worker) are imported unmodified, with make_golden.py's stand-in modules
for the imports they never use.  Per case the fixture stores the inputs, the reference's r_T / r_S (calculate_nearest_k over
the plain similarity matrix, both directions), its CSLS matrix's gold rank per row, Hits@k / MR / MRR and the aligned pairs,
plus per row the gap between the gold's CSLS value and the nearest other column's (so that a test knows which rows are decided by
more than rounding).  Only data is written; no reference source text is stored.
"""
import argparse
import contextlib
import importlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TOP_K = [1, 5, 10, 50]

# (name, n1, n2, d, metric, normalize, k, duplicated columns)
CASES = [
    ("inner_k1", 100, 130, 16, "inner", True, 1, False),
    ("inner_k5", 120, 120, 20, "inner", True, 5, False),
    ("inner_k10", 110, 150, 16, "inner", True, 10, False),
    ("euclid", 100, 140, 12, "euclidean", False, 10, False),
    ("euclid_norm", 96, 96, 16, "euclidean", True, 5, False),
    ("cosine_raw", 90, 120, 12, "cosine", False, 10, False),
    ("inner_dup", 80, 112, 12, "inner", True, 10, True),
]


def make_inputs(rng, n1, n2, d, dup):
    """Noisy copies of shared anchors (a realistic alignment task: most golds are found) in float32."""
    base = rng.standard_normal((n2, d)).astype(np.float32)
    e2 = base + 0.15 * rng.standard_normal((n2, d)).astype(np.float32)
    e1 = base[:n1] + 0.9 * rng.standard_normal((n1, d)).astype(np.float32)
    if dup:  # duplicated columns: every 7th target row repeats its predecessor (exact ties in every row)
        for j in range(7, n2, 7):
            e2[j] = e2[j - 1]
    return e1.astype(np.float32), e2.astype(np.float32)


def exact_topk_mean(mat, k):
    """The exact top-k multiset, summed in float64 in descending order."""
    s = -np.sort(-mat.astype(np.float64), axis=1)[:, :k]
    return (s.sum(1) / k).astype(np.float32)


def case(ref_sim, ref_align, rng, name, n1, n2, d, metric, normalize, k, dup, out):
    e1, e2 = make_inputs(rng, n1, n2, d, dup)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = ref_sim.sim(e1, e2, metric=metric, normalize=normalize, csls_k=0)
        csls = ref_sim.sim(e1, e2, metric=metric, normalize=normalize, csls_k=k)
    r_t = ref_sim.calculate_nearest_k(plain, k)
    r_s = ref_sim.calculate_nearest_k(plain.T, k)
    # the reference's partition-order float32 mean equals the exact top-k mean on this data (to float32 rounding)
    np.testing.assert_allclose(r_t, exact_topk_mean(plain, k), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(r_s, exact_topk_mean(plain.T, k), rtol=2e-6, atol=1e-7)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rest, hits1, mr, mrr = ref_align.greedy_alignment(e1, e2, TOP_K, 1, metric, normalize, k, True)
    line = [l for l in buf.getvalue().splitlines() if "csls" in l]
    assert line and f"csls={k}," in line[0], buf.getvalue()
    gold = csls[np.arange(n1), np.arange(n1)]
    rank = (csls > gold[:, None]).sum(1)
    ties = (csls == gold[:, None]).sum(1)
    dist = np.abs(csls.astype(np.float64) - gold[:, None])
    dist[np.arange(n1), np.arange(n1)] = np.inf
    gap = dist.min(1)                           # nearest other column above or below the gold, in the reference's float32 values
    pairs = np.array(sorted(rest), dtype=np.int64)
    hits = np.array([float(np.mean(rank < kk) * 100) for kk in TOP_K])
    assert abs(round(hits[0], 3) - hits1) < 1e-9 or ties.max() > 1
    p = name + "/"
    out.update({p + "e1": e1, p + "e2": e2, p + "r_t": r_t.astype(np.float32), p + "r_s": r_s.astype(np.float32),
                p + "rank": rank.astype(np.int32), p + "ties": ties.astype(np.int32), p + "gap": gap.astype(np.float32),
                p + "pairs": pairs, p + "hits": np.asarray([hits1], dtype=np.float64), p + "mr": np.float64(mr),
                p + "mrr": np.float64(mrr), p + "sim": plain.astype(np.float32)[:16, :24],
                p + "csls": csls.astype(np.float32)[:16, :24],
                p + "meta": np.array([n1, n2, d, k, int(normalize), int(dup)], dtype=np.int64),
                p + "metric": np.array(metric)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    code = os.path.join(a.reference, "code")
    if not os.path.isdir(code):
        sys.exit(f"reference not found at {code} (this script only runs in the build container)")
    sys.path.insert(0, code)
    import make_golden
    make_golden.install_tf_forwarder()
    make_golden.install_empty_standins()
    ref_sim = importlib.import_module("base.similarity")
    ref_align = importlib.import_module("base.alignment")
    rng = np.random.default_rng(20261016)
    out = {}
    for c in CASES:
        case(ref_sim, ref_align, rng, *c, out)
    out["cases"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "csls_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/sinkhorn_golden.npz: the float64 Sinkhorn oracle (tests/sinkhorn_oracle.py) applied to similarity
matrices produced by EXECUTING THE REFERENCE'S OWN `base.similarity.sim`.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_sinkhorn_golden.py [--reference /root/reference]

The reference's `code/base/similarity.py` is imported unmodified, with make_golden.py's stand-in modules for the imports it
never uses; the inputs are make_csls_golden.py's noisy anchors.  Per case the fixture stores the inputs, the oracle's
potentials after L iterations at temperature tau, M (the largest |s| plus the largest potential of any iteration: what the
error bound of the device test needs), the gold's rank / ties / best column under the re-scored matrix s - a - b, Hits@k / MR /
MRR, per row the gap between the gold's re-scored value and the nearest other column's, plain Hits@1 for comparison, a corner
of S, and for the square case the stable matching (tests/stable_oracle.py) of the re-scored matrix, kept only if it is unchanged
under 16 perturbations of the matrix by the rank test's margin.  A row is left out of the exact rank comparison when its gap
is below 4 * 2 L * bound; the script asserts that at most 5 % of a case's rows are, and that two cases leave none out.
Only data is written; no reference source text is stored.
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
sys.path.insert(0, os.path.dirname(HERE))

TOP_K = [1, 5, 10, 50]
SEED = 20261019

# (name, n1, n2, d, metric, normalize, tau, L)
CASES = [
    ("inner_100", 100, 130, 16, "inner", True, 0.05, 10),
    ("inner_sq", 120, 120, 20, "inner", True, 0.05, 10),
    ("inner_wide", 200, 333, 75, "inner", True, 0.05, 10),
    ("euclid", 96, 140, 12, "euclidean", False, 0.1, 30),
]
STABLE_CASE, STABLE_CUT = "inner_sq", 100


def history_max(O, S, iters, tau):
    """The largest |potential| of any iteration (the sub_b of some mke_align_lse call)."""
    a, b, top = np.zeros(S.shape[0]), np.zeros(S.shape[1]), 0.0
    for _ in range(iters):
        a = O.lse(S, b, tau)
        b = O.lse(S.T, a, tau)
        top = max(top, np.abs(a).max(), np.abs(b).max())
    return a, b, float(top)


def case(ref_sim, O, SO, rng, name, n1, n2, d, metric, normalize, tau, iters, out):
    from make_csls_golden import make_inputs
    e1, e2 = make_inputs(rng, n1, n2, d, False)
    with contextlib.redirect_stdout(io.StringIO()):
        S = np.asarray(ref_sim.sim(e1, e2, metric=metric, normalize=normalize, csls_k=0))
    assert S.shape == (n1, n2)
    a, b = O.potentials(S, iters, tau)
    a2, b2, top = history_max(O, S.astype(np.float64), iters, tau)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    R = O.scores(S, a, b)
    np.testing.assert_allclose(np.exp(R / tau).sum(0), 1.0, rtol=0, atol=1e-9)     # columns normalised by the last pass
    M = float(np.abs(S).max()) + top
    pot_bound = iters * (O.bound(tau, n2, M) + O.bound(tau, n1, M))                 # L row calls over n2 + L column calls over n1
    assert pot_bound <= 2 * iters * O.bound(tau, max(n1, n2), M)
    greater, ties, best, gap = O.rank_oracle(R)
    margin = 4 * pot_bound
    left_out = int((gap < margin).sum())
    assert left_out <= 0.05 * n1, (name, left_out)
    assert ties.max() == 1
    hits, mr, mrr = O.metrics(greater, TOP_K)
    plain_hits1 = float(np.mean((S > S[np.arange(n1), np.arange(n1)][:, None]).sum(1) < 1) * 100)
    p = name + "/"
    out.update({p + "e1": e1, p + "e2": e2, p + "a": a, p + "b": b, p + "M": np.float64(M), p + "pot_bound": np.float64(pot_bound),
                p + "rank": greater.astype(np.int32), p + "ties": ties.astype(np.int32), p + "best": best,
                p + "gap": gap, p + "hits": hits, p + "mr": np.float64(mr), p + "mrr": np.float64(mrr),
                p + "plain_hits1": np.float64(plain_hits1), p + "left_out": np.int64(left_out),
                p + "sim": S.astype(np.float32)[:16, :24], p + "score": R[:16, :24],
                p + "meta": np.array([n1, n2, d, int(normalize), iters], dtype=np.int64), p + "tau": np.float64(tau),
                p + "metric": np.array(metric)})
    if name == STABLE_CASE:
        cut = min(STABLE_CUT, n2)
        val, col = SO.lists_from_matrix(R, cut)
        match = SO.deferred_acceptance(val, col, n2)
        prng = np.random.default_rng(7)
        for _ in range(16):
            pv, pc = SO.lists_from_matrix(R + prng.uniform(-margin, margin, size=R.shape), cut)
            assert np.array_equal(SO.deferred_acceptance(pv, pc, n2), match), f"{name}: the matching changes under a {margin:.1e} perturbation"
        out[p + "match"] = match.astype(np.int64)
        out[p + "cut"] = np.int64(STABLE_CUT)
    print(f"{name}: plain Hits@1 {plain_hits1:.1f}, Sinkhorn Hits@1 {hits[0]:.1f}, left out {left_out}, 2L-bound {pot_bound:.2e}")
    return left_out


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
    import sinkhorn_oracle as O
    import stable_oracle as SO
    rng = np.random.default_rng(SEED)
    out = {}
    left = [case(ref_sim, O, SO, rng, *c, out) for c in CASES]
    assert sum(1 for x in left if x == 0) >= 2, left       # the metric comparison needs two cases that leave no row out
    out["cases"] = np.array([c[0] for c in CASES])
    out["top_k"] = np.array(TOP_K, dtype=np.int64)
    path = os.path.join(HERE, "sinkhorn_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/stable_golden.npz by EXECUTING THE REFERENCE'S OWN stable alignment.

Run in the build container only (needs the reference tree, which does not exist on the GPU box):

    python tests/golden/make_stable_golden.py [--reference /root/reference]

The reference's `code/base/similarity.py` (`sim`) and `code/base/alignment.py` (`arg_sort`, `galeshapley`,
`stable_alignment`) are imported unmodified, the way make_csls_golden.py imports them.  Per case the reference's similarity
matrix is argsorted in both directions, `galeshapley(.., 100)` gives the matching, and `stable_alignment(.., nums_threads=1)`
its printed precision.  A case is kept only if (1) the reference converged (every suitor matched: only then is its result
independent of PYTHONHASHSEED), (2) tests/stable_oracle.py on the reference's matrix returns the same matching, and (3) the
matching is unchanged under 16 perturbations of the float64 matrix by uniform +-1e-5 — ten times the similarity band of the
evaluator's tests, so last-ulp differences of the device's similarities cannot flip it.  Otherwise the next seed is tried.
Only data is written (inputs, the matching as an int array, the precision); no reference source text is stored.
"""
import argparse
import contextlib
import copy
import importlib
import io
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

CUT = 100
# (name, n1, n2, d, metric, normalize, csls_k, noise on e1)
CASES = [
    ("inner_sq", 150, 150, 16, "inner", True, 0, 0.9),
    ("inner_wide", 150, 200, 16, "inner", True, 0, 1.2),
    ("inner_csls", 140, 180, 12, "inner", True, 10, 1.0),
    ("euclid", 160, 220, 12, "euclidean", False, 0, 1.0),
    ("euclid_csls", 120, 160, 12, "euclidean", True, 5, 0.9),
    ("cosine_raw", 130, 170, 12, "cosine", False, 0, 1.0),
]


def make_inputs(rng, n1, n2, d, noise):
    """make_csls_golden.make_inputs's recipe (noisy copies of shared anchors) with the noise on e1 as a parameter."""
    base = rng.standard_normal((n2, d)).astype(np.float32)
    e2 = base + 0.15 * rng.standard_normal((n2, d)).astype(np.float32)
    e1 = base[:n1] + noise * rng.standard_normal((n1, d)).astype(np.float32)
    return e1.astype(np.float32), e2.astype(np.float32)


def case(ref_sim, ref_align, oracle, rng, name, n1, n2, d, metric, normalize, csls_k, noise, out):
    e1, e2 = make_inputs(rng, n1, n2, d, noise)
    with contextlib.redirect_stdout(io.StringIO()):
        mat = ref_sim.sim(e1, e2, metric=metric, normalize=normalize, csls_k=csls_k)
    idx1, idx2 = np.arange(n1), np.arange(n2)
    suitors = ref_align.arg_sort(idx1, mat, 'x_', 'y_')
    reviewers = ref_align.arg_sort(idx2, mat.T, 'y_', 'x_')
    matching = ref_align.galeshapley(copy.deepcopy(suitors), reviewers, CUT)
    if len(matching) != n1:
        return f"{name}: the reference matched {len(matching)} of {n1} suitors in {CUT} rounds"
    match = np.full(n1, -1, dtype=np.int64)
    for s, r in matching.items():
        match[int(s.split('_')[-1])] = int(r.split('_')[-1])
    cut = min(CUT, n2)
    val, col = oracle.lists_from_matrix(mat, cut)
    if not np.array_equal(oracle.deferred_acceptance(val, col, n2), match):
        return f"{name}: the oracle differs from the reference"
    prng = np.random.default_rng(n1 * 1000 + n2)
    for _ in range(16):
        pert = mat.astype(np.float64) + prng.uniform(-1e-5, 1e-5, size=mat.shape)
        v, c = oracle.lists_from_matrix(pert, cut)
        if not np.array_equal(oracle.deferred_acceptance(v, c, n2), match):
            return f"{name}: the matching changes under a 1e-5 perturbation"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ref_align.stable_alignment(e1, e2, metric, normalize, csls_k, 1, cut=CUT)
    m = re.search(r"stable alignment precision = ([0-9.]+)%", buf.getvalue())
    assert m and "generating candidate lists costs time" in buf.getvalue(), buf.getvalue()
    precision = float(m.group(1))
    assert abs(precision - round(float(np.mean(match == idx1)) * 100, 3)) < 2e-3, (precision, np.mean(match == idx1))
    greedy = np.argmax(mat, axis=1)
    p = name + "/"
    out.update({p + "e1": e1, p + "e2": e2, p + "match": match, p + "precision": np.float64(precision),
                p + "greedy_differs": np.int64((greedy != match).sum()),
                p + "meta": np.array([n1, n2, d, csls_k, int(normalize), CUT], dtype=np.int64), p + "metric": np.array(metric)})
    return None


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
    import stable_oracle as oracle
    for seed in range(20261017, 20261017 + 20):
        rng = np.random.default_rng(seed)
        out, why = {}, None
        for c in CASES:
            why = case(ref_sim, ref_align, oracle, rng, *c, out)
            if why:
                break
        if why is None:
            break
        print(f"seed {seed}: {why}; next seed")
    else:
        sys.exit("no seed met the three conditions")
    out["cases"] = np.array([c[0] for c in CASES])
    out["seed"] = np.int64(seed)
    path = os.path.join(HERE, "stable_golden.npz")
    np.savez_compressed(path, **out)
    print(f"seed {seed}: wrote {path} ({os.path.getsize(path)} bytes); rows differing from the greedy argmax: "
          + ", ".join(f"{c[0]} {int(out[c[0] + '/greedy_differs'])}" for c in CASES))


if __name__ == "__main__":
    main()

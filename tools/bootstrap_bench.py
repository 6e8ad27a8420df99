"""Time of one self-training refresh, phase by phase, on generated arrays of a dataset's size, beside the host form of the same
per-triple step (base/kgs.py swap_relation_triples / swap_attribute_triples on Python sets).

    python tools/bootstrap_bench.py [--reps 5] [--sizes demo,dbpwd]

The arrays have the shape of the lists a schedule holds: KG1 ids [0, n1), KG2 ids [n1, 2 n1), duplicate-free relation and
attribute id-triples, candidates = the 70 % of the pairs that are not train links, embeddings = unit rows and a noisy copy.
Host clock around synchronised phases, one warm-up, median of --reps; then the refresh as the schedule enqueues it (no
synchronisation between the phases, one read-back).  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multike_amd import _lib  # noqa: E402
from multike_amd.base import alignment, bootstrap  # noqa: E402
from multike_amd.base.kgs import swap_attribute_triples, swap_relation_triples  # noqa: E402

SIZES = {  # pairs, unaligned extra per KG, relation triples / entity, attribute triples / entity, relations, attributes, values
    "demo": dict(n_pairs=3000, n_extra=300, tpe=5.0, ape=3.0, n_rel=40, n_attr=30, n_val=4000),        # tools/learn_demo.py's default folder
    "dbpwd": dict(n_pairs=100_000, n_extra=0, tpe=4.6, ape=3.0, n_rel=550, n_attr=600, n_val=100_000),  # bench.py's C2 shape
}
DIM, NOISE, TRAIN_SHARE = 75, 0.18, 0.3


def unique_rows(a):
    _, first = np.unique(a, axis=0, return_index=True)
    return a[np.sort(first)]


def build(n_pairs, n_extra, tpe, ape, n_rel, n_attr, n_val, seed=3):
    rng = np.random.default_rng(seed)
    n1 = n_pairs + n_extra
    rel, attr = [], []
    for lo in (0, n1):
        m = int(n1 * tpe)
        rel.append(unique_rows(np.stack([lo + rng.integers(0, n1, m), rng.integers(0, n_rel, m), lo + rng.integers(0, n1, m)], 1)))
        m = int(n1 * ape)
        attr.append(unique_rows(np.stack([lo + rng.integers(0, n1, m), rng.integers(0, n_attr, m), rng.integers(0, n_val, m)], 1)))
    cand = np.arange(int(n_pairs * TRAIN_SHARE), n_pairs)
    base = rng.standard_normal((len(cand), DIM)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    other = base + NOISE * rng.standard_normal(base.shape).astype(np.float32)
    return dict(n_ent=2 * n1, n1=n1, rel=rel, attr=attr, ids1=cand.astype(np.int32), ids2=(n1 + cand).astype(np.int32), e1=base, e2=other)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return statistics.median(out) * 1e3, res


def run(name, reps, threshold):
    d = build(**SIZES[name])
    dev = lambda a, dt=torch.int32: torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dt)
    cols = {k: tuple(dev(np.concatenate(d[k])[:, c]) for c in range(3)) for k in ("rel", "attr")}
    ids1, ids2, e1, e2 = dev(d["ids1"]), dev(d["ids2"]), dev(d["e1"], torch.float32), dev(d["e2"], torch.float32)
    n_ent = d["n_ent"]
    out = {"size": name, "entities": n_ent, "relation_triples": int(cols["rel"][0].numel()), "attribute_triples": int(cols["attr"][0].numel()),
           "candidates": int(ids1.numel()), "threshold": threshold, "reps": reps}
    out["sweep_ms"], (match, counts, _) = timed(lambda: alignment._mutual(e1, e2, "inner", True, 0, threshold, None), reps)
    out["partner_ms"], partner = timed(lambda: _lib.boot_partner(match, ids1, ids2, n_ent), reps)
    out["swap_relation_ms"], rel = timed(lambda: _lib.swap_triples(*cols["rel"], partner), reps)
    out["swap_attribute_ms"], attr = timed(lambda: _lib.swap_triples(*cols["attr"], partner, heads_only=True), reps)
    out["read_back_ms"], nums = timed(lambda: torch.cat([rel[2], attr[2], counts.long()]).cpu().tolist(), reps)
    out["pairs"], out["gold_pairs"], out["relation_entries"], out["attribute_entries"] = nums[2], nums[3], nums[0], nums[1]

    def refresh():
        partner, match, counts = bootstrap.bootstrap_links(e1, e2, ids1, ids2, n_ent, threshold)
        a = bootstrap._swap_launch(cols["rel"], partner, False, None)
        b = bootstrap._swap_launch(cols["attr"], partner, True, None)
        n_rel, n_attr, _, _ = torch.cat([a[-1], b[-1], counts.long()]).cpu().tolist()
        return bootstrap._swap_finish(a, n_rel), bootstrap._swap_finish(b, n_attr)
    out["refresh_ms"], lists = timed(refresh, reps)

    # the host form, for the same links: Python sets of tuples, as KGs.__init__ swaps the seed links
    m = match.cpu().numpy()
    on = m >= 0
    links = list(zip(d["ids1"][on].tolist(), d["ids2"][m[on]].tolist()))
    m12, m21 = dict(links), {b: a for a, b in links}
    sets = {k: [set(map(tuple, side.tolist())) for side in d[k]] for k in ("rel", "attr")}
    t = time.perf_counter()
    host_rel = [swap_relation_triples(sets["rel"][0], m12), swap_relation_triples(sets["rel"][1], m21)]
    out["host_relation_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    host_attr = [swap_attribute_triples(sets["attr"][0], m12), swap_attribute_triples(sets["attr"][1], m21)]
    out["host_attribute_ms"] = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for s in host_rel + host_attr:
        np.asarray(sorted(s), dtype=np.int32)
    out["host_sort_and_pack_ms"] = (time.perf_counter() - t) * 1e3
    # the same lists: duplicate-free triples over disjoint ids swap into duplicate-free lists, so set equality is list equality
    out["same_as_host"] = bool(set(map(tuple, lists[0].cols.tolist())) == host_rel[0] | host_rel[1]
                               and len(lists[0]) == len(host_rel[0]) + len(host_rel[1])
                               and set(map(tuple, lists[1].cols.tolist())) == host_attr[0] | host_attr[1]
                               and len(lists[1]) == len(host_attr[0]) + len(host_attr[1]))
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="demo,dbpwd")
    ap.add_argument("--threshold", type=float, default=None)
    a = ap.parse_args()
    for s in a.sizes.split(","):
        run(s, a.reps, a.threshold)

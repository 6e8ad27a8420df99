"""One code-word training step through the C ABI, as mke_relation_steps strings it, held exactly at every joint:

  ids -> mke_neg_codes (code words + the step's bitmap row) -> mke_triple_score_step (k_triple_score<..., CW>, no id arrays, no
  entity flags) -> mke_rows_update_multi (relation table by its flags, entity table by the bitmap and the step's positives)

on "own" batches of score_cases.py (one side replaced by a draw, or the positive drawn as its own negative: what mke_neg_sample
writes).  The bake is compared with the NumPy statement of section (1c) (score_cases.define), from the ids and again in place
from the sampler's words.  After the score launch the buffers are held to score_cases.compare (tier 1: bit patterns; tier 2: the
counted bound) and the gradient scratch is read back.  After the update launch:

  1. every visited entity and relation row is the update_cases.py rule (rows_rule) applied to the device's OWN scratch rows --
     the row, its privatised copies, its hub copies -- as exact inputs, within that rule's counted bound (bit for bit where the
     rule is exact); the sum over m copies is charged (m - 1) u/2 of the sum of absolute values, as score_cases._sum does;
  2. rows finished in place by the score launch and rows nobody referenced are bit-identical to their state after it;
  3. the whole scratch is zero again;
  4. the visited set -- the rows whose ref_count entry the update launch reset, and in tier 2 the rows whose table or accumulator
     changed -- equals the rows the flag form of the score launch flags (the reference's touched_ent == tag).

mke_neg_codes takes groups of up to 64 negatives, so the table's crowded hub-row batch (groups of 65) runs here with 64.

Worst error / bound observed on the MI355X (gfx950) (none above 1; in tier 1 the score launch, SGD's tables and Adagrad's
accumulators matched bit for bit, Adagrad's w is bounded there too); the same for one and two groups per wavefront:

  after the score launch (tier 2)       loss 0.0550   grad_ent 0.1797   grad_rel 0.0637   in-place w 0.4826   in-place acc 0.4539
  after the update launch, entity rows  tier 2: w 0.5194  acc 0.4532      tier 1 (Adagrad): w 0.3826
  after the update launch, relation rows tier 2: w 0.4972  acc 0.4535     tier 1 (Adagrad): w 0.3763

(0.5194: a hub row, whose gradient is the sum of its scratch row and three copies; the sum's own rounding is part of the bound.)
"""
import ctypes as C

import numpy as np
import pytest

import score_cases as sc
import update_cases as uc
from rows_cases import OLD_TAG, SENTINEL, TAG
from test_score_exact_gpu import CODE_PAD, CODE_POISON, addr, dev, host, opt_code, sync

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RC_FILL = 7


def chain_runs(strides, tier, npps):
    """"own" cases of the code-word table in the form without ids and without flags, two and one group per wavefront."""
    cases = {r.case.id: r.case for r in sc.CW_RUNS if r.case.stride in strides and r.case.tier == tier and r.case.kinds == "own"
             and r.case.tag == "" and r.case.npp in npps}
    cases = [c._replace(npp=min(c.npp, BAKE_MAX)) for c in cases.values()]       # the table's crowded hub-row batch has groups of 65
    return [sc.Run(c, f) for c in cases for f in sc.forms_cw() if not f.ids and not f.flags]


BAKE_MAX = 64                                                         # mke_neg_codes takes groups of up to 64 negatives
TIER2 = chain_runs((16, 80, 256), 2, sc.NPPS)
TIER1 = chain_runs((16, 64, 320), 1, (1, 9, 33, 64))


def bake(c, d):
    """mke_neg_codes from the ids, and in place from the sampler's words: (words, bitmap buffer with two poisoned words behind the row)."""
    from multike_amd import _lib
    n_ent, _ = sc.sizes(c)
    words = _lib.neg_code_row_words(n_ent)
    want_codes, want_row = sc.step_codes(c)
    assert words == len(want_row)
    off = dev(np.array([0, c.n_pos], dtype=np.int64))
    out = []
    for inplace in (False, True):
        bits = dev(np.full(words + 2, -1, dtype=np.int32))
        code = dev(np.concatenate([sc.sampler_words(c) if inplace else np.full(c.n_neg, CODE_POISON, np.int32), np.full(CODE_PAD, CODE_POISON, np.int32)]))
        pos = [d["ph"], d["pr"], d["pt"]]
        if inplace:
            _lib.neg_codes_inplace(pos, off, 0, 1, 0, c.n_pos, c.npp, n_ent, bits[:words], code[:c.n_neg])
        else:
            _lib.neg_codes(pos, off, 0, 1, 0, c.n_pos, [d["nh"], d["nr"], d["nt"]], c.npp, n_ent, bits[:words], code[:c.n_neg])
        sync()
        got_bits, got_code = host(bits).view(np.uint32), host(code)
        assert np.array_equal(got_code[:c.n_neg], want_codes) and (got_code[c.n_neg:] == CODE_POISON).all(), (c.id, inplace, "code words")
        assert np.array_equal(got_bits[:words], want_row) and (got_bits[words:] == 0xFFFFFFFF).all(), (c.id, inplace, "bitmap row")
        out.append((code, bits))
    return out[0]


def step(r):
    from multike_amd import _lib
    c, f = r
    o = sc.ops(c)
    n_ent, n_rel = sc.sizes(c)
    st, P = c.stride, c.n_pos
    want = sc.reference(c, f)
    flagged = np.nonzero(sc.reference(c, f._replace(flags=1))["touched_ent"][:n_ent] == TAG)[0]
    d = {k: dev(getattr(o, k)) for k in ("ent", "rel", "acc", "ph", "pr", "pt", "pw", "nh", "nr", "nt", "nw", "hot_slot")}
    rng = np.random.default_rng(c.n_neg)
    rel_acc0 = np.full((n_rel + 1, st), uc.ACC_PAD, dtype=f32)
    rel_acc0[:n_rel, :c.dim] = (0.1 + np.abs(sc.quarters(rng, (n_rel, c.dim)))).astype(f32)
    rel_acc0[n_rel] = np.nan
    d["rel_acc"] = dev(rel_acc0)
    d["neg_code"], d["bits"] = bake(c, d)
    d["partials"] = dev(np.full(sc.LOSS_PARTIALS, np.nan))
    d["touched_rel"] = dev(np.full(n_rel + 64, OLD_TAG, np.int32))
    d["grad_ent"], d["grad_rel"] = dev(sc.initial("grad_ent", want)), dev(sc.initial("grad_rel", want))
    adagrad = c.opt == "adagrad"
    # ---- the score launch: code words alone
    a = _lib.ScoreArgs(ent_table=addr(d["ent"]), n_ent=n_ent, ent_normalize=c.ent_norm, rel_table=addr(d["rel"]), n_rel=n_rel,
                       rel_normalize=c.rel_norm, stride=st, dim=c.dim, pos_h=addr(d["ph"]), pos_r=addr(d["pr"]), pos_t=addr(d["pt"]),
                       pos_w=addr(d["pw"]), n_pos=P, neg_w=addr(d["nw"]), n_neg=c.n_neg, neg_per_pos=c.npp, scale=c.scale,
                       grad_ent=addr(d["grad_ent"]), grad_rel=addr(d["grad_rel"]), grad_rel_copies=c.copies, touched_rel=addr(d["touched_rel"]),
                       tag=TAG, ent_acc=addr(d["acc"]) if adagrad else None, optimizer=opt_code(c), lr=c.lr, loss_partials=addr(d["partials"]),
                       neg_code=addr(d["neg_code"]))
    if c.n_hot:
        a.hot = _lib.HotRowsStruct(addr(d["hot_slot"]), c.n_hot, c.hot_copies, n_ent)
    tune = _lib.tuning(score_splits=f.splits, score_half_groups=f.half, score_offsets32=1, score_lane_ids=1)
    a.tuning = C.addressof(tune)
    assert _lib.lib().mke_triple_score_step(C.byref(a), _lib._stream()) == 0, _lib.lib().mke_last_error()
    sync()
    mid = {k: host(d[k]) for k in ("partials", "ent", "acc", "rel", "grad_ent", "grad_rel", "touched_rel")}
    if not adagrad:
        assert np.array_equal(uc.bits(mid.pop("acc")), uc.bits(o.acc)), "SGD: the accumulator was written"
    problems, ratios = sc.compare(mid, want)
    for name, v in ratios.items():
        print(f"RATIO chain:score-q{sc.qpg_of(c, f)}:{name} {v:.4f} {r.id}")
    assert not problems, (r.id, problems)
    assert np.array_equal(uc.bits(mid["rel"]), uc.bits(o.rel))
    ent1, acc1 = mid["ent"], host(d["acc"])
    ge, gr = mid["grad_ent"].copy(), mid["grad_rel"].copy()
    # rows of the scratch no launch wrote hold SENTINEL (so the comparison above sees a stray add); the loop's scratch is zero there
    n_gent, n_grel = len(ge) - 1, len(gr) - 1
    ge[:n_gent][ge[:n_gent] == SENTINEL], gr[:n_grel][gr[:n_grel] == SENTINEL] = 0.0, 0.0
    d["grad_ent"], d["grad_rel"] = dev(ge), dev(gr)
    d["rc_ent"], d["rc_rel"] = dev(np.full(n_ent + 1, RC_FILL, np.int32)), dev(np.full(n_rel + 1, RC_FILL, np.int32))
    # ---- the update launch: relation table by its flags, entity table by the bitmap and the positives
    arr = (_lib.UpdateTableStruct * 2)()
    t = arr[0]
    t.table, t.acc, t.grad, t.touched = addr(d["rel"]), addr(d["rel_acc"]) if adagrad else None, addr(d["grad_rel"]), addr(d["touched_rel"])
    t.n_rows, t.normalize, t.grad_copies, t.ref_count = n_rel, c.rel_norm, c.copies, addr(d["rc_rel"])
    t = arr[1]
    t.table, t.acc, t.grad, t.touched = addr(d["ent"]), addr(d["acc"]) if adagrad else None, addr(d["grad_ent"]), None
    t.n_rows, t.normalize, t.grad_copies, t.ref_count = n_ent, c.ent_norm, 1, addr(d["rc_ent"])
    t.bits, t.pos_h, t.pos_t, t.n_pos = addr(d["bits"]), addr(d["ph"]), addr(d["pt"]), P
    if c.n_hot:
        t.hot = _lib.HotRowsStruct(addr(d["hot_slot"]), c.n_hot, c.hot_copies, n_ent)
    code = _lib.lib().mke_rows_update_multi(arr, C.c_int(2), C.c_int32(TAG), C.c_int(st), C.c_int(c.dim), C.c_int(opt_code(c)), C.c_float(c.lr),
                                            _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    end = {k: host(d[k]) for k in ("ent", "acc", "rel", "rel_acc", "grad_ent", "grad_rel", "rc_ent", "rc_rel", "touched_rel", "bits")}
    problems = []
    # 4. the visited set
    visited = np.nonzero(end["rc_ent"][:n_ent] == 0)[0]
    if not np.array_equal(visited, flagged):
        problems.append(f"visited entity rows {sorted(set(visited) ^ set(flagged))[:8]} differ from the rows the flag form flags")
    if not (np.isin(end["rc_ent"], (0, RC_FILL)).all() and end["rc_ent"][n_ent] == RC_FILL):
        problems.append("ref_count of the entity table: an entry is neither reset nor kept")
    changed = np.nonzero((uc.bits(end["ent"][:n_ent]) != uc.bits(ent1[:n_ent])).any(1) | (uc.bits(end["acc"][:n_ent]) != uc.bits(acc1[:n_ent])).any(1))[0]
    if not set(changed) <= set(flagged) or (c.tier == 2 and not np.array_equal(changed, flagged)):
        problems.append(f"rows that changed {sorted(set(changed) ^ set(flagged))[:8]} differ from the rows the flag form flags")
    rel_rows = np.nonzero(mid["touched_rel"][:n_rel] == TAG)[0]
    if not np.array_equal(np.nonzero(end["rc_rel"][:n_rel] == 0)[0], rel_rows):
        problems.append("visited relation rows differ from the flagged ones")
    # 2. everything else as the score launch left it (in-place rows, unreferenced rows, the NaN tail rows)
    for name, now, then, rows, n in (("ent", end["ent"], ent1, flagged, n_ent), ("acc", end["acc"], acc1, flagged, n_ent),
                                     ("rel", end["rel"], o.rel, rel_rows, n_rel), ("rel_acc", end["rel_acc"], rel_acc0, rel_rows, n_rel)):
        rest = np.ones(n + 1, bool)
        rest[rows] = False
        if not np.array_equal(uc.bits(now[rest]), uc.bits(then[rest])):
            problems.append(f"{name}: a row outside the visited ones changed in the update launch")
    assert set(want["in_place_rows"]).isdisjoint(flagged)
    # 3. the scratch is zero again (its tail rows keep their poison)
    for name, g, n in (("grad_ent", end["grad_ent"], n_gent), ("grad_rel", end["grad_rel"], n_grel)):
        if g[:n].any() or not (g[n] == SENTINEL).all():
            problems.append(f"{name}: not zero after the update launch (rows {np.nonzero(g[:n].any(1))[0][:8].tolist()})")
    # 1. the update given its gradient: the rule on the device's own scratch rows
    hs = o.hot_slot[:n_ent] if c.n_hot else np.full(n_ent, -1)
    for name, rows, W0, A0, W1, A1, norm, parts in (
            ("ent", flagged, ent1, acc1, end["ent"], end["acc"], c.ent_norm,
             [ge[flagged]] + [np.where((hs[flagged] >= 0)[:, None], ge[n_ent + k * c.n_hot + np.maximum(hs[flagged], 0)], 0.0) for k in range(c.hot_copies if c.n_hot else 0)]),
            ("rel", rel_rows, o.rel, rel_acc0, end["rel"], end["rel_acc"], c.rel_norm, [gr[k * n_rel + rel_rows] for k in range(c.copies)])):
        parts = [p.astype(f64) for p in parts]
        G, tot = sum(parts), sum(np.abs(p) for p in parts)
        m = sum((p != 0).any(1) for p in parts).reshape(-1, 1)                   # a copy of zeros adds nothing: x + 0 = x
        k = np.maximum(m - 1, 0) * 0.5 * uc.U
        case = uc.UCase("rows", n=len(W0) - 1, dim=c.dim, stride=st, opt=c.opt, normalize=norm, lr=c.lr)
        if c.tier == 1:                                                           # every sum exact: g g + a within float64, w - lr g within float32
            assert float(np.abs(G).max(initial=0.0)) ** 2 * 2 ** 27 < 2 ** 52
        ref = uc.rows_rule(case, W0[rows].astype(f64), A0[rows].astype(f64), G,
                           G_err=None if c.tier == 1 else k / (1 - k) * tot + np.where(m > 1, uc.TINY, 0.0))
        for what, got in (("table", W1[rows]), ("acc", A1[rows])):
            if what not in ref:
                continue
            val, err = ref[what]
            if err is None:
                if not np.array_equal(uc.bits(got), uc.bits(np.asarray(val, f32))):
                    problems.append(f"{name} {what}: visited rows differ from the exact rule on the device's gradient")
                continue
            diff = np.abs(got.astype(f64) - val)
            if not np.isfinite(got).all() or (diff[err == 0] != 0).any():
                problems.append(f"{name} {what}: not finite, or an element with bound 0 differs")
                continue
            ratio = float((diff[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
            print(f"RATIO chain:update:{name}-{what} {ratio:.4f} {r.id}")
            if ratio > 1:
                problems.append(f"{name} {what}: error / bound = {ratio:.3g}")
    if not np.array_equal(end["bits"].view(np.uint32)[:-2], sc.step_codes(c)[1]) or not np.array_equal(end["touched_rel"], mid["touched_rel"]):
        problems.append("the update launch wrote the bitmap or the relation flags")
    assert not problems, (r.id, problems)


@pytest.mark.parametrize("stride", (16, 80, 256))
def test_chain_tier2(stride):
    """Collisions, rows finished in place, hub rows in the list walk and the chunk walk, normalised tables, SGD and Adagrad."""
    runs = [r for r in TIER2 if r.case.stride == stride]
    assert {sc.qpg_of(r.case, r.form) for r in runs} == {2, 4} and any(r.case.n_hot for r in runs) and any(r.case.ent_norm for r in runs)
    for r in runs:
        step(r)


@pytest.mark.parametrize("stride", (16, 64, 320))
def test_chain_tier1(stride):
    """Saturated operands: the score launch bit for bit, and the update of the exact gradient rows bit for bit under SGD."""
    runs = [r for r in TIER1 if r.case.stride == stride]
    assert {sc.qpg_of(r.case, r.form) for r in runs} == {2, 4} and any(r.case.opt == "sgd" for r in runs)
    for r in runs:
        step(r)

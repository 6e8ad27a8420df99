"""One code word per negative (mke_neg_codes, mke_codes.hip) and the code-word form of the training kernel
(mke_score_args.neg_code), through the C ABI.

The bake is held against a NumPy statement of the header's definition, exactly: the ids are handed in, not sampled, so
every case is constructed here.  code = entity | MKE_CODE_HEAD | MKE_CODE_FAST | MKE_CODE_EXCL with
  entity  neg_h where it differs from the positive's head, else neg_t
  HEAD    neg_h differs from the positive's head
  FAST    the positive's relation and exactly one side differs
  EXCL    mke_count_entity_refs of the negative's own step gives the entity the count 1
and the bitmap of step s holds, per entity, 00 / 01 / 11 for a count of 0 / 1 / 2 or more.

The score form is held against the reference-count form on score_cases.py's operands: on collision-free batches every
buffer the two launches leave is the same bit pattern; on every other batch the code-word form stays inside the bound
score_cases.py derives for the instantiation it stands beside (tier 1: bit patterns)."""
import ctypes as C

import numpy as np
import pytest
import torch

import score_cases as sc
from rows_cases import OLD_TAG, SENTINEL, TAG

pytestmark = pytest.mark.gpu
f32 = np.float32
POISON = np.int32(-0x5A5A5A5B)
PAD = 16


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def addr(t):
    return None if t is None else t.data_ptr()


def sync():
    """A device error ends the session: nothing more is started on a card that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error: {e}", returncode=3)


# ----------------------------------------------------------------------------------------------------- the definition
from score_cases import define, step_counts          # noqa: E402  (the NumPy statement of section (1c): one definition, in the case module)


def bake(pos, neg, off, s0, s1, npp, n_ent, extra_rows=2):
    """mke_neg_codes on the device -> (codes, the whole bitmap buffer [s1 - s0 + extra_rows, words], the poison pads)."""
    from multike_amd import _lib
    words = _lib.neg_code_row_words(n_ent)
    assert words == (n_ent + 15) // 16
    n = (off[s1] - off[s0]) * npp
    buf = dev(np.full(n + 2 * PAD, POISON, dtype=np.int32))
    bits = dev(np.zeros((s1 - s0 + extra_rows) * words, dtype=np.int32))
    bits[(s1 - s0) * words:] = 0                      # the rows past the chunk: must stay zero
    bits[:(s1 - s0) * words] = -1                     # the chunk's own rows: the call zeroes them itself
    d_pos, d_neg = [dev(x) for x in pos], [dev(x) for x in neg]
    _lib.neg_codes(d_pos, dev(np.asarray(off, dtype=np.int64)), s0, s1, int(off[s0]), int(off[s1]), d_neg, npp, n_ent, bits, buf[PAD:PAD + max(n, 1)])
    sync()
    out = buf.cpu().numpy()
    return out[PAD:PAD + n], bits.cpu().numpy().view(np.uint32).reshape(-1, words), (out[:PAD], out[PAD + n:])


def check(pos, neg, off, s0, s1, npp, n_ent):
    want_c, want_b = define(pos, neg, off, s0, s1, npp, n_ent)
    got_c, got_b, pads = bake(pos, neg, off, s0, s1, npp, n_ent)
    assert (pads[0] == POISON).all() and (pads[1] == POISON).all(), "poison around neg_code"
    assert np.array_equal(got_b[:s1 - s0], want_b), "bitmap of the chunk"
    assert not got_b[s1 - s0:].any(), "bitmap outside the chunk's range"
    assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:5].tolist()
    return got_c


def random_ids(rng, n_pos, npp, n_ent, n_rel=4):
    ph, pr, pt = rng.integers(0, n_ent, n_pos), rng.integers(0, n_rel, n_pos), rng.integers(0, n_ent, n_pos)
    g = np.arange(n_pos * npp) // npp
    nh, nr, nt = ph[g].copy(), pr[g].copy(), pt[g].copy()
    kind = rng.integers(0, 8, len(g))                  # 0-2 head, 3-5 tail, 6 both sides, 7 another relation / nothing
    e = rng.integers(0, n_ent, len(g))                 # may repeat the positive's own entity: a negative equal to its positive
    nh[kind <= 2] = e[kind <= 2]
    nt[(kind >= 3) & (kind <= 5)] = e[(kind >= 3) & (kind <= 5)]
    nh[kind == 6], nt[kind == 6] = e[kind == 6], rng.integers(0, n_ent, int((kind == 6).sum()))
    nr[kind == 7] = (nr[kind == 7] + 1) % n_rel
    return [x.astype(np.int32) for x in (ph, pr, pt)], [x.astype(np.int32) for x in (nh, nr, nt)]


@pytest.mark.parametrize("n_ent", (40, 300))
@pytest.mark.parametrize("npp", (1, 3, 15, 16, 25, 33, 64))
def test_bake_random_steps(n_ent, npp):
    """Four steps, one empty, the last one short; the whole chunk, then steps [1, 3) alone (its negatives laid out from step 1)."""
    rng = np.random.default_rng([n_ent, npp])
    off = np.array([0, 9, 9, 20, 23])
    pos, neg = random_ids(rng, 23, npp, n_ent)
    check(pos, neg, off, 0, 4, npp, n_ent)
    check(pos, [x[off[1] * npp:] for x in neg], off, 1, 3, npp, n_ent)


def test_bake_rows_that_do_not_fit_the_lds():
    """Rows of up to 262,144 entities are marked and read in the LDS by one workgroup per step; wider ones in global memory by a
    mark launch and a bake launch.  The same definition, the same bitmap."""
    rng = np.random.default_rng(7)
    off = np.array([0, 9, 9, 20, 23])
    for n_ent in (262_144, 262_145):
        pos, neg = random_ids(rng, 23, 3, n_ent)
        for x in pos[0], pos[2], neg[0], neg[2]:
            x[x % 5 == 0] = n_ent - 1 - (x[x % 5 == 0] % 7)      # the last words of the row, and repeats among them
        check(pos, neg, off, 0, 4, 3, n_ent)


def test_bake_constructed_cases():
    """The template below runs twice, as step 0 and (entities shifted by 24) as step 1, so a mark of step 0 cannot leak into
    step 1; entity 47 is referenced once in each of the two steps (exclusive in both), entity 46 twice in step 0 and once in
    step 1 (exclusive in step 1 only)."""
    from multike_amd import _lib
    H, F, X = _lib.CODE_HEAD, _lib.CODE_FAST, _lib.CODE_EXCL
    n_ent, npp, SH = 48, 2, 24
    # positives (h, r, t), each with its two negatives and the code expected of them
    template = [
        ((0, 0, 1), [((2, 0, 1), 2 | H | F | X),          # an entity referenced once
                     ((0, 0, 3), 3 | F)]),                # one referenced twice in the step (again below)
        ((4, 1, 5), [((3, 1, 5), 3 | H | F),              # ... the second reference of 3
                     ((4, 1, 6), 6 | F)]),                # 6 is a positive's tail (below) and this one negative: count 2
        ((7, 0, 6), [((7, 0, 6), 6),                      # a negative equal to its positive: slow, entity = its tail, adds nothing
                     ((8, 0, 9), 8 | H | X)]),            # both sides replaced: slow, both counted; 8 and 9 once each
        ((10, 0, 10), [((11, 0, 10), 11 | H | F | X),     # h == t: entity 10 counts 2
                       ((10, 0, 10), 10)]),
        ((12, 1, 13), [((14, 0, 13), 14 | H | X),         # another relation and another head: slow; 14 referenced once
                       ((12, 0, 13), 13 | X)]),           # another relation alone: adds nothing; entity = the tail, referenced once
    ]
    shifted = [((h + SH, r, t + SH), [((a + SH, b, c + SH), code + SH) for (a, b, c), code in negs]) for (h, r, t), negs in template]
    step0 = template + [((16, 0, 17), [((47, 0, 17), 47 | H | F | X), ((16, 0, 46), 46 | F)]),
                        ((18, 0, 19), [((46, 0, 19), 46 | H | F), ((18, 0, 19), 19 | X)])]
    step1 = shifted + [((40, 0, 41), [((47, 0, 41), 47 | H | F | X), ((40, 0, 46), 46 | F | X)]),
                       ((42, 0, 43), [((42, 0, 43), 43 | X), ((45, 0, 43), 45 | H | F | X)])]
    rows = step0 + step1
    pos = [np.array([p[k] for p, _ in rows], dtype=np.int32) for k in range(3)]
    neg = [np.array([n[k] for _, negs in rows for n, _ in negs], dtype=np.int32) for k in range(3)]
    want = np.array([code for _, negs in rows for _, code in negs], dtype=np.int32)
    got = check(pos, neg, np.array([0, len(step0), len(rows)]), 0, 2, npp, n_ent)
    assert np.array_equal(got, want), [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_bake_refusals_launch_nothing():
    from multike_amd import _lib
    L, one = _lib.lib(), C.c_void_p(16)
    args = lambda **kw: [kw.get(k, v) for k, v in (("ph", one), ("pr", one), ("pt", one), ("off", one), ("s0", C.c_int(0)), ("s1", C.c_int(2)),
                                                  ("p0", C.c_int64(0)), ("p1", C.c_int64(8)), ("nh", one), ("nr", one), ("nt", one),
                                                  ("npp", C.c_int(3)), ("n_ent", C.c_int64(40)), ("bits", one), ("words", C.c_int64(6)),
                                                  ("code", one), ("stream", None))]
    assert L.mke_neg_codes(*args(words=C.c_int64(5))) == -2 and b"bitmap" in L.mke_last_error()
    assert L.mke_neg_codes(*args(bits=None)) == -1
    assert L.mke_neg_codes(*args(n_ent=C.c_int64((1 << 26) + 1), words=C.c_int64(1 << 40))) == -4
    assert L.mke_neg_codes(*args(npp=C.c_int(65))) == -3
    assert L.mke_neg_codes(*args(s1=C.c_int(0))) == 0


# ----------------------------------------------------------------------------------------------------- score form against score form
def codes_of(c):
    o = sc.ops(c)
    n_ent, _ = sc.sizes(c)
    return define((o.ph, o.pr, o.pt), (o.nh[:c.n_neg], o.nr[:c.n_neg], o.nt[:c.n_neg]), np.array([0, c.n_pos]), 0, 1, c.npp, n_ent)[0]


def launch(c, f, want, codes):
    """One mke_triple_score_step in the training instantiation on fresh operands: with neg_code (and no ref_count) or with ref_count."""
    from multike_amd import _lib
    o = sc.ops(c)
    n_ent, n_rel = sc.sizes(c)
    st = c.stride
    d = {k: dev(getattr(o, k)) for k in ("ent", "rel", "ph", "pr", "pt", "pw", "nh", "nr", "nt", "nw", "hot_slot")}
    d["acc"] = dev(o.acc) if c.opt == "adagrad" else None
    d["ref_count"] = None if codes else dev(o.ref_count)
    d["neg_code"] = dev(np.concatenate([codes_of(c), np.full(PAD, POISON, np.int32)])) if codes else None
    d["partials"] = dev(np.full(sc.LOSS_PARTIALS, np.nan))
    d["touched_ent"], d["touched_rel"] = dev(np.full(n_ent + 64, OLD_TAG, np.int32)), dev(np.full(n_rel + 64, OLD_TAG, np.int32))
    d["grad_ent"], d["grad_rel"] = dev(sc.initial("grad_ent", want)), dev(sc.initial("grad_rel", want))
    a = _lib.ScoreArgs(ent_table=addr(d["ent"]), n_ent=n_ent, ent_normalize=c.ent_norm, rel_table=addr(d["rel"]), n_rel=n_rel,
                       rel_normalize=c.rel_norm, stride=st, dim=c.dim, pos_h=addr(d["ph"]), pos_r=addr(d["pr"]), pos_t=addr(d["pt"]),
                       pos_w=addr(d["pw"]), n_pos=c.n_pos, neg_h=addr(d["nh"]), neg_r=addr(d["nr"]), neg_t=addr(d["nt"]), neg_w=addr(d["nw"]),
                       n_neg=c.n_neg, neg_per_pos=c.npp, scale=c.scale, grad_ent=addr(d["grad_ent"]), grad_rel=addr(d["grad_rel"]),
                       grad_rel_copies=c.copies, touched_ent=addr(d["touched_ent"]), touched_rel=addr(d["touched_rel"]), tag=TAG,
                       ref_count=addr(d["ref_count"]), ent_acc=addr(d["acc"]), optimizer={"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD}[c.opt],
                       lr=c.lr, loss_partials=addr(d["partials"]), neg_code=addr(d["neg_code"]))
    if c.n_hot:
        a.hot = _lib.HotRowsStruct(addr(d["hot_slot"]), c.n_hot, c.hot_copies, n_ent)
    tune = _lib.tuning(score_splits=f.splits, score_half_groups=f.half, score_offsets32=1, score_lane_ids=1)
    a.tuning = C.addressof(tune)
    code = _lib.lib().mke_triple_score_step(C.byref(a), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    return {k: v.cpu().numpy() for k, v in d.items() if v is not None and k in ("partials", "grad_ent", "grad_rel", "touched_ent", "touched_rel",
                                                                                 "ent", "acc", "rel", "ref_count")}


def training_runs(stride):
    """score_cases.py's runs of the training instantiation (ref_count, 32-bit offsets, lane ids) at this width, no rider."""
    return [r for r in sc.RUNS if r.case.stride == stride and r.form == r.form._replace(det=0, x=1, o32=1, lid=1) and r.case.npp > 0
            and not r.case.fwd_only and not r.case.rider]


@pytest.mark.parametrize("stride", (16, 80, 256))
def test_code_form_equals_count_form_where_nothing_collides(stride):
    """Collision-free batches, two and one group per wavefront: table, accumulator, gradient rows, relation copies, flags and
    loss partials are the same bit patterns in both forms; the reference-count form leaves its counts at zero."""
    cases = [r.case for r in sc.RUNS if r.case.stride == stride and r.case.kinds == "unique"]
    assert cases
    seen = set()
    for c in cases:
        for half in (1000, 0):
            f = sc.Form(0, 1, 1, 1, half, 1)
            want = sc.reference(c, f)
            count, code = launch(c, f, want, False), launch(c, f, want, True)
            seen.add(sc.qpg_of(c, f))
            for k in ("ent", "acc", "grad_ent", "grad_rel", "rel", "touched_ent", "touched_rel", "partials"):
                if k in count:
                    assert np.array_equal(count[k].view(np.int32 if count[k].itemsize == 4 else np.int64),
                                          code[k].view(np.int32 if code[k].itemsize == 4 else np.int64)), (c.id, half, k)
            problems, _ = sc.compare(code, want)
            assert not problems, (c.id, half, problems)
    assert seen == {2, 4}


@pytest.mark.parametrize("stride", (16, 80, 256))
def test_code_form_within_the_derived_bound(stride):
    """Every run score_cases.py lists for the training instantiation at this width (collisions, slow negatives in both id blocks,
    hub rows, slices, weights; tier 1 as bit patterns), now with code words instead of counts: the same reference, the same bound."""
    runs = training_runs(stride)
    assert {sc.qpg_of(r.case, r.form) for r in runs} == {2, 4} and any(r.case.tier == 2 and r.case.kinds == "mixed" for r in runs)
    for r in runs:
        want = sc.reference(r.case, r.form)
        got = launch(r.case, r.form, want, True)
        problems, ratios = sc.compare(got, want)
        for name, v in ratios.items():
            print(f"RATIO codes:q{sc.qpg_of(r.case, r.form)}:{name} {v:.4f} {r.id}")
        o = sc.ops(r.case)
        if not np.array_equal(got["rel"].view(np.int32), o.rel.view(np.int32)):
            problems.append("rel_table changed")
        assert not problems, (r.id, problems)


def test_code_form_falls_back_or_refuses():
    """Where the code-word form is not legal (64-bit offsets asked for) the call runs the reference-count form when it has the
    counts, and refuses when it has not."""
    from multike_amd import _lib
    c = next(r.case for r in sc.RUNS if r.case.stride == 16 and r.case.kinds == "unique")
    o = sc.ops(c)
    n_ent, n_rel = sc.sizes(c)
    want = sc.reference(c, sc.Form(0, 1, 0, 1, 0, 1))
    d = {k: dev(getattr(o, k)) for k in ("ent", "rel", "acc", "ph", "pr", "pt", "pw", "nh", "nr", "nt", "nw", "ref_count")}
    d["grad_ent"], d["grad_rel"] = dev(sc.initial("grad_ent", want)), dev(sc.initial("grad_rel", want))
    d["te"], d["tr"] = dev(np.full(n_ent + 64, OLD_TAG, np.int32)), dev(np.full(n_rel + 64, OLD_TAG, np.int32))
    d["partials"], d["code"] = dev(np.full(sc.LOSS_PARTIALS, np.nan)), dev(codes_of(c))
    tune = _lib.tuning(score_splits=1, score_half_groups=0, score_offsets32=0, score_lane_ids=1)
    a = _lib.ScoreArgs(ent_table=addr(d["ent"]), n_ent=n_ent, ent_normalize=c.ent_norm, rel_table=addr(d["rel"]), n_rel=n_rel,
                       rel_normalize=c.rel_norm, stride=c.stride, dim=c.dim, pos_h=addr(d["ph"]), pos_r=addr(d["pr"]), pos_t=addr(d["pt"]),
                       pos_w=addr(d["pw"]), n_pos=c.n_pos, neg_h=addr(d["nh"]), neg_r=addr(d["nr"]), neg_t=addr(d["nt"]), neg_w=addr(d["nw"]),
                       n_neg=c.n_neg, neg_per_pos=c.npp, scale=c.scale, grad_ent=addr(d["grad_ent"]), grad_rel=addr(d["grad_rel"]),
                       grad_rel_copies=c.copies, touched_ent=addr(d["te"]), touched_rel=addr(d["tr"]), tag=TAG, ref_count=None,
                       ent_acc=addr(d["acc"]) if c.opt == "adagrad" else None, optimizer={"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD}[c.opt],
                       lr=c.lr, loss_partials=addr(d["partials"]), neg_code=addr(d["code"]), tuning=C.addressof(tune))
    assert _lib.lib().mke_triple_score_step(C.byref(a), _lib._stream()) == -3 and b"neg_code" in _lib.lib().mke_last_error()
    a.ref_count = addr(d["ref_count"])
    assert _lib.lib().mke_triple_score_step(C.byref(a), _lib._stream()) == 0, _lib.lib().mke_last_error()
    sync()
    got = {"partials": d["partials"].cpu().numpy(), "ent": d["ent"].cpu().numpy(), "grad_ent": d["grad_ent"].cpu().numpy(),
           "grad_rel": d["grad_rel"].cpu().numpy(), "ref_count": d["ref_count"].cpu().numpy()}
    problems, _ = sc.compare(got, want)
    assert not problems, problems

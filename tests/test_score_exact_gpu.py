"""k_triple_score in its twelve instantiations per row width, k_stage_reduce and k_count_refs (mke_score.hip) against the
reference of score_cases.py, through the C ABI itself: mke_score_args, mke_count_job and the mke_tuning of each call are filled
here, so a form is selected per call (score_splits, score_half_groups, score_offsets32, score_lane_ids), never process-wide.

Tier 1 (saturated operands, see score_cases.py) is compared as bit patterns, the sign of a zero apart: the loss as the sum of
all MKE_LOSS_PARTIALS partials (each written and finite, the rider blocks' zero), every gradient row, relation copy, hub copy and
staging slot with its key, the flags, the in-place rows of table and accumulator, the reference counts, and the poison around
all of them.  Deterministic runs go on through mke_stage_reduce and are compared again.  Tier E holds device runs against
each other on collision-free batches: a negative's own row is the same bit pattern in every form that scatters it, the flushed
h / r / t rows in all forms with the same number of groups per wavefront, the rows finished in place in all forms that finish
them, and those rows again against the two-kernel path (the same step without ref_count, then mke_rows_update).  Tier 2
(normalised or scaled tables, collisions, slices, the in-place Jacobian) is held against float64 within the bound
score_cases.py derives by counting roundings; the bound is not fitted to the device.  test_score_cases.py shows without a
device that seventeen kinds of subtly wrong kernel fail these comparisons.  Every test prints "RATIO ..." before it asserts.

Worst error / bound observed on the MI355X (gfx950), tier 2, per instantiation family and output (none above 1: no finding, and
no hardware-function allowance had to be replaced by a measured one; q2 / q4: two / one group per wavefront):

  form                              loss     grad_ent  grad_rel  slots    after reduce (ent / rel)  in-place w  in-place acc
  deterministic, q2                 0.0326   -         -         0.2340   0.2340 / 0.1362           -           -
  deterministic, q4                 0.0376   -         -         0.2371   0.2371 / 0.1362           -           -
  deterministic + exclusive, q2     0.0326   -         -         0.2340   0.2340 / 0.1362           0.4923      0.4543
  deterministic + exclusive, q4     0.0376   -         -         0.2340   0.2340 / 0.1362           0.4923      0.4543
  exclusive, 32-bit offsets, q2     0.0326   0.2340    0.1362    -        -                         0.4923      0.4543
  exclusive, 32-bit offsets, q4     0.0376   0.2340    0.1362    -        -                         0.4923      0.4543
  the same with lane ids, q2        0.0366   0.2371    0.1362    -        -                         0.4923      0.4545
  the same with lane ids, q4        0.0376   0.2371    0.1362    -        -                         0.4923      0.4544
  plain, q2                         0.0326   0.2340    0.1362    -        -                         -           -
  plain, q4 (slices among them)     0.0376   0.2371    0.1651    -        -                         -           -
  exclusive, 64-bit offsets, q2     0.0326   0.2340    0.1362    -        -                         0.4923      0.4543
  exclusive, 64-bit offsets, q4     0.0376   0.2340    0.1651    -        -                         0.4923      0.4543
  two kernels (step, then mke_rows_update) on the in-place rows                                     0.4910      0.4545

The figures next to 0.5 are elements whose error is the last rounding alone (half an ulp, charged a whole one); the float32
NumPy model of test_score_cases.py gives 0.4923 / 0.4545 / 0.2429 / 0.1357 for w / acc / grad_ent / grad_rel, so the 2 ulp
allowed for rsqrtf, rsq, rcp, exp and log were not needed by these operands.  Tier E found no pair of forms that differs.  The
two-kernel path is NOT bit-identical to the in-place rows: of 52 collision-free batches 19 agree in every element, 31 differ in
the last bit of 1 to 59 table elements and one (stride 320, Adagrad, entity table not normalised) in 1225 of 8640, never in the
accumulator: mke_rows_update associates the Jacobian differently and w - lr g s is not contracted alike at every width.  Both
sit inside the counted bound, and the header says so now.

The code-word forms (k_triple_score<..., CW>: neg_code instead of ref_count; score_cases.CW_RUNS) run the same way: neg_code with
a poisoned pad behind it, neg_h / neg_r / neg_t NULL when ids = 0, touched_ent NULL when flags = 0, a poisoned ref_count that must
come back untouched.  Tier 1 matched bit for bit in all 26 instantiations and all four (ids, flags) combinations; tier E found
the code-word form equal to the ref_count form, ids = 0 equal to ids = 1 and flags = 0 equal to flags = 1 in every buffer they
share.  Worst error / bound, tier 2 (the same for q2 and q4 and for flags = 0 / 1 unless two figures are given):

  form                              loss     grad_ent  grad_rel          in-place w  in-place acc
  code words with ids               0.0550   0.2340    0.1944            0.4921      0.4545
  code words without ids            0.0550   0.1797    0.0653 / 0.0675   0.4921      0.4545

(with ids the "mixed" batches run as well, hence the larger gradient figures).  test_score_cases.py shows that seven kinds of
kernel that route the words wrongly fail these comparisons.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import score_cases as sc
import update_cases as uc
from multike_amd._abi import mke_count_job as CountJob
from rows_cases import OLD_TAG, SENTINEL, STRIDES, TAG

pytestmark = pytest.mark.gpu
f32 = np.float32


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return None if t is None else t.cpu().numpy()


def addr(t):
    return None if t is None else t.data_ptr()


def opt_code(c):
    from multike_amd import _lib
    return {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD}[c.opt]


def sync():
    """A device error ends the session: nothing more is started on a card that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error: {e}", returncode=3)


RC_POISON = 0x5A5A5A5A
CODE_PAD = 64
# what the pad behind neg_code holds: read as a word it would finish row 0 in place (seen by the comparisons) and never leave the tables
CODE_POISON = sc.CODE_FAST | sc.CODE_HEAD | sc.CODE_EXCL


def sentinel(rows, stride):
    return np.full((rows + 1, stride), SENTINEL, dtype=f32)


def launch(c, f, want):
    """One mke_triple_score_step on fresh operands -> the buffers afterwards (and "counted", the rider's ref_count)."""
    from multike_amd import _lib
    o = sc.ops(c)
    n_ent, n_rel = sc.sizes(c)
    st = c.stride
    bwd = not c.fwd_only
    d = {k: dev(getattr(o, k)) for k in ("ent", "rel", "ph", "pr", "pt", "pw", "nh", "nr", "nt", "nw", "hot_slot")}
    d["acc"] = dev(o.acc) if c.opt == "adagrad" else None
    d["ref_count"] = dev(o.ref_count) if (f.x and bwd) else None
    if f.cw:                                                          # the word array with its poisoned pad, a poisoned ref_count
        d["ref_count"] = dev(np.full(n_ent + 1, RC_POISON, np.int32))
        d["neg_code"] = dev(np.concatenate([sc.codes_of(c), np.full(CODE_PAD, CODE_POISON, np.int32)]))
        if not f.ids:
            d["nh"] = d["nr"] = d["nt"] = None
    d["partials"] = dev(np.full(sc.LOSS_PARTIALS, np.nan))
    d["touched_ent"], d["touched_rel"] = dev(np.full(n_ent + 64, OLD_TAG, np.int32)), dev(np.full(n_rel + 64, OLD_TAG, np.int32))
    if f.cw and not f.flags:
        d["touched_ent"] = None
    n_gent = n_ent + (c.hot_copies * c.n_hot if c.n_hot else 0)
    if bwd:
        d["grad_ent"] = dev(sc.initial("grad_ent", want) if "grad_ent" in want else sentinel(n_gent, st))
        d["grad_rel"] = dev(sc.initial("grad_rel", want) if "grad_rel" in want else sentinel(c.copies * n_rel, st))
    a = _lib.ScoreArgs(ent_table=addr(d["ent"]), n_ent=n_ent, ent_normalize=c.ent_norm, rel_table=addr(d["rel"]), n_rel=n_rel,
                       rel_normalize=c.rel_norm, stride=st, dim=c.dim, pos_h=addr(d["ph"]), pos_r=addr(d["pr"]), pos_t=addr(d["pt"]),
                       pos_w=addr(d["pw"]), n_pos=c.n_pos, neg_h=addr(d["nh"]), neg_r=addr(d["nr"]), neg_t=addr(d["nt"]), neg_w=addr(d["nw"]),
                       n_neg=c.n_neg, neg_per_pos=c.npp, scale=c.scale, grad_ent=addr(d.get("grad_ent")), grad_rel=addr(d.get("grad_rel")),
                       grad_rel_copies=c.copies, touched_ent=addr(d["touched_ent"]), touched_rel=addr(d["touched_rel"]), tag=TAG,
                       ref_count=addr(d["ref_count"]), ent_acc=addr(d["acc"]), optimizer=opt_code(c), lr=c.lr, loss_partials=addr(d["partials"]),
                       neg_code=addr(d.get("neg_code")))
    if c.n_hot:
        a.hot = _lib.HotRowsStruct(addr(d["hot_slot"]), c.n_hot, c.hot_copies, n_ent)
    if f.det:
        n_slots = 3 * (c.n_pos * (c.npp + 1) if c.npp else c.n_pos + c.n_neg)
        d["stage_rows"] = dev(sentinel(n_slots, st))
        d["stage_keys"] = dev(np.full(n_slots + 1, sc.KEY_FILL, dtype=np.int64))
        a.stage_rows, a.stage_keys, a.stage_slots = addr(d["stage_rows"]), addr(d["stage_keys"]), n_slots
    tune = _lib.tuning(score_splits=f.splits, score_half_groups=f.half, score_offsets32=f.o32, score_lane_ids=f.lid)
    a.tuning = C.addressof(tune)
    keep = []
    if c.rider:
        cc = sc.count_case(c.rider)
        co = uc.count_ops(cc)
        keep = [dev(v) for v in (co.pos_h, co.pos_t, co.neg_h, co.neg_t, co.ref_count)]
        cj = CountJob(addr(keep[0]), addr(keep[1]), cc.n_pos, addr(keep[2]), addr(keep[3]), cc.n_pos * cc.neg_per_pos, cc.neg_per_pos, addr(keep[4]))
        a.next_count = C.addressof(cj)
    code = _lib.lib().mke_triple_score_step(C.byref(a), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    got = {k: host(v) for k, v in d.items() if v is not None and k in ("partials", "grad_ent", "grad_rel", "stage_rows", "stage_keys", "touched_ent",
                                                                      "touched_rel", "ent", "acc", "ref_count", "rel")}
    if c.rider:
        got["counted"] = host(keep[4])
    if f.cw:                                                          # neither reads nor resets ref_count; the words and their pad stay
        assert (got.pop("ref_count") == RC_POISON).all(), (c.id, f.id, "ref_count was written")
        assert np.array_equal(host(d["neg_code"]), np.concatenate([sc.codes_of(c), np.full(CODE_PAD, CODE_POISON, np.int32)]))
    got["_dev"] = d
    return got


def reduce_staged(c, got, want):
    """Stable sort of the slot keys, mke_stage_reduce -> (grad_ent, grad_rel, touched_ent, touched_rel)."""
    from multike_amd import _lib
    d = got["_dev"]
    n_slots = d["stage_keys"].numel() - 1
    keys, order = torch.sort(d["stage_keys"][:n_slots], stable=True)
    ge, gr = dev(sc.initial("reduced_ent", want)), dev(sc.initial("reduced_rel", want))
    te, tr = dev(np.full(len(want["touched_ent"]), OLD_TAG, np.int32)), dev(np.full(len(want["touched_rel"]), OLD_TAG, np.int32))
    code = _lib.lib().mke_stage_reduce(C.c_void_p(addr(d["stage_rows"])), C.c_void_p(addr(keys)), C.c_void_p(addr(order)), C.c_int64(n_slots),
                                       C.c_int(c.stride), C.c_void_p(addr(ge)), C.c_void_p(addr(gr)), C.c_void_p(addr(te)), C.c_void_p(addr(tr)),
                                       C.c_int32(TAG), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    return host(ge), host(gr), host(te), host(tr)


def report(ratios, r):
    inst = sc.instantiation(r.case, r.form)
    fam = f"cw-i{r.form.ids}f{r.form.flags}-q{inst[2]}" if r.form.cw else f"{inst[1]}{int(inst[2])}-q{inst[3]}"
    for name, v in ratios.items():
        print(f"RATIO score:{fam}:{name} {v:.4f} {r.id}")


def run(r):
    c, f = r
    want = sc.reference(c, f)
    got = launch(c, f, want)
    problems, ratios = sc.compare(got, want)
    report(ratios, r)
    o = sc.ops(c)
    if not np.array_equal(got["rel"].view(np.int32), o.rel.view(np.int32)):
        problems.append("rel_table changed")
    if "ref_count" not in got and not f.cw and not np.array_equal(got["ent"].view(np.int32), o.ent.view(np.int32)):
        problems.append("ent_table changed without the exclusive path")
    if c.fwd_only and not ((got["touched_ent"] == OLD_TAG).all() and (got["touched_rel"] == OLD_TAG).all()):
        problems.append("forward only: a flag was set")
    if f.det and not c.fwd_only:
        if not ((got["grad_ent"] == SENTINEL).all() and (got["grad_rel"] == SENTINEL).all()):
            problems.append("deterministic mode wrote the gradient scratch")
        ge, gr, te, tr = reduce_staged(c, got, want)
        p2, r2 = sc.compare({"partials": got["partials"], "grad_ent": ge, "grad_rel": gr, "touched_ent": te, "touched_rel": tr},
                            dict(want, grad_ent=want["reduced_ent"], grad_rel=want["reduced_rel"], touched_ent=want["reduced_touched"][0],
                                 touched_rel=want["reduced_touched"][1]))
        report({"reduced_" + k: v for k, v in r2.items() if k != "loss"}, r)
        problems += ["after mke_stage_reduce: " + p for p in p2]
    if c.rider and not np.array_equal(got["counted"], uc.count_reference(sc.count_case(c.rider))):
        problems.append("the rider's counts differ from the mke_count_entity_refs rule")
    assert not problems, (r.id, problems)
    return got


def select(stride, **kw):
    return [r for r in sc.RUNS if r.case.stride == stride and all(getattr(r.case, k) == v for k, v in kw.items())]


@pytest.mark.parametrize("stride", STRIDES)
def test_tier1(stride):
    """Structure, bit for bit: rounds, id blocks, slices, flushes, copies, hub rows, flags, in-place rows, slots, the ragged guard."""
    seen = set()
    for r in select(stride, tier=1):
        if r.case.tag in ("pass", "rider"):
            continue
        run(r)
        seen.add(sc.instantiation(r.case, r.form))
    assert len({i for i in seen if i[0] == stride // 16}) == 12, sorted(seen)


@pytest.mark.parametrize("stride", STRIDES)
def test_tier2(stride):
    """The arithmetic against float64 within the derived bound: collisions, slices, normalised tables, the in-place Jacobian."""
    for r in select(stride, tier=2):
        run(r)


@pytest.mark.parametrize("r", [r for r in sc.RUNS if r.case.tag == "pass"], ids=lambda r: r.id)
def test_second_grid_pass(r):
    run(r)


@pytest.mark.parametrize("total", sc.COUNT_TOTALS)
def test_count_rider(total):
    """next_count: the counts follow the rule, the rider blocks' partials are 0, and the step's own outputs are those of the
    launch without the rider (fewer scoring blocks), bit for bit."""
    for r in (r for r in sc.RUNS if r.case.rider == total):
        got = run(r)
        plain = r.case._replace(rider=0)
        alone = launch(plain, r.form, sc.reference(plain, r.form))
        for k in ("grad_ent", "grad_rel", "touched_ent", "touched_rel", "ent", "ref_count"):
            if k in got:
                assert np.array_equal(uc.bits(got[k]), uc.bits(alone[k])), (r.id, k)
        assert got["partials"].sum() == alone["partials"].sum()


def rows_bits(a, rows):
    return sc.canon(a[rows])


@pytest.mark.parametrize("stride", STRIDES)
def test_tier_e_and_two_kernels(stride):
    """Collision-free batches: every atomic lands once on a zero row, so device runs are comparable bit for bit."""
    from multike_amd import _lib
    for c in (r.case for r in select(stride, kinds="unique")):
        o = sc.ops(c)
        n_ent, n_rel = sc.sizes(c)
        P, N, npp = c.n_pos, c.n_neg, c.npp
        g, n = np.arange(N) // npp, np.arange(N) % npp
        head = o.nh[:N] != o.ph[g]
        e = np.where(head, o.nh[:N], o.nt[:N])
        own_slot = sc.stage_slot(g, npp, n, np.where(head, 0, 2))
        gg = np.arange(P)
        flush = {q: None for q in (2, 4)}
        inplace = None
        for f in sc.forms12():
            assert sc.splits_of(c, f) == 1
            if f.det and not f.x:                                     # the slots of this group shape: the yardstick
                got = launch(c, f, sc.reference(c, f))
                q = sc.qpg_of(c, f)
                slots = got["stage_rows"]
                own = sc.canon(slots[own_slot])
                flush[q] = tuple(sc.canon(slots[sc.stage_slot(gg, npp, npp, k)]) for k in range(3))
        for f in sc.forms12():
            got = launch(c, f, sc.reference(c, f))
            q = sc.qpg_of(c, f)
            if f.det:
                rows = tuple(sc.canon(got["stage_rows"][sc.stage_slot(gg, npp, npp, k)]) for k in range(3))
                if not f.x:
                    assert np.array_equal(sc.canon(got["stage_rows"][own_slot]), own), (c.id, f.id, "a negative's row differs between the group shapes")
            else:
                rows = (rows_bits(got["grad_ent"], o.ph), rows_bits(got["grad_rel"], o.pr), rows_bits(got["grad_ent"], o.pt))
                if not f.x:
                    assert np.array_equal(rows_bits(got["grad_ent"], e), own), (c.id, f.id, "a negative's scattered row differs from its slot")
            for k in range(3):
                assert np.array_equal(rows[k], flush[q][k]), (c.id, f.id, "flushed row", k)
            if f.x:                                                   # all of them finish every corrupted row in place
                assert not got["ref_count"][e].any()
                now = (rows_bits(got["ent"], e), rows_bits(got["acc"], e) if "acc" in got else None)
                if inplace is None:
                    inplace = now
                assert np.array_equal(now[0], inplace[0]) and (now[1] is None or np.array_equal(now[1], inplace[1])), (c.id, f.id, "in-place rows")
        # the two-kernel path: the step without ref_count, then mke_rows_update on the same rows
        f = sc.Form(0, 0, 1, 1, 0, 1)
        got = launch(c, f, sc.reference(c, f))
        d = got["_dev"]
        code = _lib.lib().mke_rows_update(C.c_void_p(addr(d["ent"])), C.c_void_p(addr(d["acc"])), C.c_void_p(addr(d["grad_ent"])), C.c_int(1),
                                          C.c_void_p(addr(d["touched_ent"])), C.c_int32(TAG), C.c_int64(n_ent), C.c_int(c.stride), C.c_int(c.dim),
                                          C.c_int(c.ent_norm), C.c_int(opt_code(c)), C.c_float(c.lr), _lib._stream())
        assert code == 0, _lib.lib().mke_last_error()
        sync()
        two = (host(d["ent"])[e], host(d["acc"])[e] if d["acc"] is not None else None)
        nw = int((sc.canon(two[0]) != inplace[0]).sum())
        na = 0 if two[1] is None else int((sc.canon(two[1]) != inplace[1]).sum())
        print(f"TWO-KERNEL {c.id}: {nw} table and {na} accumulator elements of {two[0].size} differ from the in-place rows")
        # not bit for bit (the row kernel associates the Jacobian differently: see the header): both within the counted bound
        problems, ratios = [], {}
        for name, got2, want2 in zip(("two_kernel_ent", "two_kernel_acc"), two, sc.two_kernel_reference(c, e)):
            if got2 is not None:
                sc._cmp(name, got2, want2, problems, ratios)
        for name, v in ratios.items():
            print(f"RATIO score:two-kernel:{name} {v:.4f} {c.id}")
        assert not problems, (c.id, problems)


@pytest.mark.parametrize("rcase", sc.REDUCE_CASES, ids=lambda r: f"n{r.n_slots}-seg{r.seg}-s{r.stride}")
def test_stage_reduce_alone(rcase):
    """Output = float32 of the float64 sum of each segment, exactly; unused slots and the poison around the rows untouched."""
    from multike_amd import _lib
    rows, keys, order, ge, gr, te, tr, R, _ = sc.reduce_ops(rcase)
    d = [dev(x) for x in (rows, keys, order, np.where(ge == SENTINEL, f32(SENTINEL), f32(0)), np.where(gr == SENTINEL, f32(SENTINEL), f32(0)),
                          np.full(len(te), OLD_TAG, np.int32), np.full(len(tr), OLD_TAG, np.int32))]
    code = _lib.lib().mke_stage_reduce(*[C.c_void_p(addr(x)) for x in d[:3]], C.c_int64(rcase.n_slots), C.c_int(rcase.stride),
                                       *[C.c_void_p(addr(x)) for x in d[3:]], C.c_int32(TAG), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    for got, want, name in zip(d[3:], (ge, gr, te, tr), ("grad_ent", "grad_rel", "touched_ent", "touched_rel")):
        assert np.array_equal(uc.bits(host(got)), uc.bits(want)), name
    assert np.array_equal(uc.bits(host(d[0])), uc.bits(rows)) and np.array_equal(host(d[1]), keys)


@pytest.mark.parametrize("total", sc.COUNT_TOTALS)
def test_count_entity_refs_alone(total):
    from multike_amd import _lib
    cc = sc.count_case(total)
    o = uc.count_ops(cc)
    d = [dev(x) for x in (o.pos_h, o.pos_t, o.neg_h, o.neg_t, o.ref_count)]
    code = _lib.lib().mke_count_entity_refs(C.c_void_p(addr(d[0])), C.c_void_p(addr(d[1])), C.c_int64(cc.n_pos), C.c_void_p(addr(d[2])),
                                            C.c_void_p(addr(d[3])), C.c_int64(cc.n_pos * cc.neg_per_pos), C.c_int(cc.neg_per_pos),
                                            C.c_void_p(addr(d[4])), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    assert np.array_equal(host(d[4]), uc.count_reference(cc))


# ----------------------------------------------------------------------------------------------------- the code-word forms
def select_cw(stride, **kw):
    return [r for r in sc.CW_RUNS if r.case.stride == stride and all(getattr(r.case, k) == v for k, v in kw.items())]


def test_code_constants():
    from multike_amd import _lib
    assert (sc.CODE_ENT_BITS, sc.CODE_HEAD, sc.CODE_FAST, sc.CODE_EXCL) == (_lib.CODE_ENT_BITS, _lib.CODE_HEAD, _lib.CODE_FAST, _lib.CODE_EXCL)


@pytest.mark.parametrize("stride", STRIDES)
def test_cw_tier1(stride):
    """k_triple_score<..., CW> bit for bit on the sampler's shape of a batch: with and without id arrays, with and without
    touched_ent, two and one group per wavefront, every group length."""
    seen = set()
    for r in select_cw(stride, tier=1):
        run(r)
        seen.add(sc.instantiation(r.case, r.form) + (r.form.ids, r.form.flags))
    assert {i[:3] for i in seen} == {(stride // 16, "cw", q) for q in (2, 4)} and len(seen) == 8, sorted(seen)


@pytest.mark.parametrize("stride", STRIDES)
def test_cw_tier2(stride):
    """The same against float64 within the derived bound: collisions, rows finished in place by MKE_CODE_EXCL, hub rows, slices,
    the second id block, words without MKE_CODE_FAST with and without ids; at stride 16 a table of 70,000 rows."""
    seen = set()
    for r in select_cw(stride, tier=2):
        run(r)
        seen.add((sc.qpg_of(r.case, r.form), r.form.ids, r.form.flags))
    assert len(seen) == 8


def same_bits(a, b):
    return np.array_equal(a.view(np.int32 if a.itemsize == 4 else np.int64), b.view(np.int32 if b.itemsize == 4 else np.int64))


@pytest.mark.parametrize("stride", STRIDES)
def test_cw_tier_e(stride):
    """Collision-free batches (a row takes one add, or the two of a positive drawn as its own negative, which commute): the
    code-word form against the ref_count form of the same grouping in every buffer both leave, ids = 0 against ids = 1 in every
    buffer, flags = 0 against flags = 1 in every buffer but the entity flags."""
    cases = [r.case for r in select_cw(stride, tag="free")]
    assert len(cases) == 2
    for c in cases:
        for half in (1000, 0):
            base_f = sc.Form(0, 1, 1, 1, half, 1)
            base = launch(c, base_f, sc.reference(c, base_f))
            got = {}
            for f in (f for f in sc.forms_cw() if f.half == half):
                got[f.ids, f.flags] = run(sc.Run(c, f))
            for k in ("partials", "ent", "acc", "rel", "grad_ent", "grad_rel", "touched_ent", "touched_rel"):
                if k in base:
                    assert same_bits(base[k], got[1, 1][k]), (c.id, half, k, "code words against ref_count")
                for ids, flags in ((0, 1), (1, 0), (0, 0)):
                    if k in base and not (k == "touched_ent" and not flags):
                        assert same_bits(got[1, 1][k], got[ids, flags][k]), (c.id, half, k, ids, flags)
            assert "touched_ent" not in got[1, 0] and "touched_ent" not in got[0, 0]
            assert not base["ref_count"][sc.reference(c, base_f)["in_place_rows"]].any()


def refusal_args(c, d, **kw):
    from multike_amd import _lib
    n_ent, n_rel = sc.sizes(c)
    return _lib.ScoreArgs(ent_table=addr(d["ent"]), n_ent=n_ent, ent_normalize=c.ent_norm, rel_table=addr(d["rel"]), n_rel=n_rel,
                          rel_normalize=c.rel_norm, stride=c.stride, dim=c.dim, pos_h=addr(d["ph"]), pos_r=addr(d["pr"]), pos_t=addr(d["pt"]),
                          pos_w=addr(d["pw"]), n_pos=c.n_pos, neg_h=addr(d["nh"]), neg_r=addr(d["nr"]), neg_t=addr(d["nt"]), neg_w=addr(d["nw"]),
                          n_neg=c.n_neg, neg_per_pos=c.npp, scale=c.scale, grad_ent=addr(d["grad_ent"]), grad_rel=addr(d["grad_rel"]),
                          grad_rel_copies=c.copies, touched_ent=addr(d["touched_ent"]), touched_rel=addr(d["touched_rel"]), tag=TAG,
                          ref_count=addr(d["ref_count"]), ent_acc=addr(d["acc"]), optimizer=opt_code(c), lr=c.lr,
                          loss_partials=addr(d["partials"]), neg_code=addr(d["neg_code"]), **kw)


def test_cw_refusals_and_fallbacks():
    """Where the code-word form is not legal -- 64-bit offsets, ids per round, deterministic staging, ungrouped negatives -- a call
    without id arrays, or without touched_ent, is refused before anything is launched (every buffer unchanged), with the code
    score_impl's order of checks gives; with ids, flags and ref_count it runs the ref_count form and resets the counts."""
    from multike_amd import _lib
    L = _lib.lib()
    NULL, SHAPE, UNSUPPORTED = -1, -2, -3
    c = select_cw(16, tag="free")[0].case
    o = sc.ops(c)
    n_ent, n_rel = sc.sizes(c)
    n_slots = 3 * c.n_pos * (c.npp + 1)
    full = sc.Form(0, 1, 1, 1, 0, 1)
    want = sc.reference(c, full)

    def fresh():
        d = {k: dev(getattr(o, k)) for k in ("ent", "rel", "acc", "ph", "pr", "pt", "pw", "nh", "nr", "nt", "nw", "ref_count")}
        d["grad_ent"], d["grad_rel"] = dev(sc.initial("grad_ent", want)), dev(sc.initial("grad_rel", want))
        d["touched_ent"], d["touched_rel"] = dev(np.full(n_ent + 64, OLD_TAG, np.int32)), dev(np.full(n_rel + 64, OLD_TAG, np.int32))
        d["partials"] = dev(np.full(sc.LOSS_PARTIALS, np.nan))
        d["neg_code"] = dev(np.concatenate([sc.codes_of(c), np.full(CODE_PAD, CODE_POISON, np.int32)]))
        d["stage_rows"], d["stage_keys"] = dev(sentinel(n_slots, c.stride)), dev(np.full(n_slots + 1, sc.KEY_FILL, dtype=np.int64))
        return d

    def call(d, where, drop):
        """mke_triple_score_step with the buffers named in `drop` passed as NULL, in the setting `where` that makes the form illegal."""
        use = {k: (None if k in drop else v) for k, v in d.items()}
        knobs = dict(score_splits=1, score_half_groups=0, score_offsets32=int(where != "o64"), score_lane_ids=int(where != "rounds"))
        tune = _lib.tuning(**knobs)
        a = refusal_args(c, use, tuning=C.addressof(tune))
        if where == "det":
            a.stage_rows, a.stage_keys, a.stage_slots = addr(d["stage_rows"]), addr(d["stage_keys"]), n_slots
        if where == "ungrouped":
            a.neg_per_pos = 0
        return L.mke_triple_score_step(C.byref(a), _lib._stream())

    ids, flag, counts = ("nh", "nr", "nt"), ("touched_ent",), ("ref_count",)
    expected = {  # (buffers left out) -> code per setting
        ids + counts: dict(o64=UNSUPPORTED, rounds=UNSUPPORTED, det=UNSUPPORTED, ungrouped=UNSUPPORTED),
        ids: dict(o64=UNSUPPORTED, rounds=UNSUPPORTED, det=UNSUPPORTED, ungrouped=UNSUPPORTED),
        flag + counts: dict(o64=UNSUPPORTED, rounds=UNSUPPORTED, det=UNSUPPORTED, ungrouped=NULL),      # neg_code without ref_count comes first
        flag: dict(o64=NULL, rounds=NULL, det=NULL, ungrouped=NULL),
        ids + flag: dict(o64=UNSUPPORTED, rounds=UNSUPPORTED, det=UNSUPPORTED, ungrouped=UNSUPPORTED),
    }
    for drop, codes in expected.items():
        for where, code in codes.items():
            d = fresh()
            before = {k: v.clone() for k, v in d.items() if v is not None}
            assert call(d, where, drop) == code, (drop, where, L.mke_last_error())
            sync()
            for k, v in before.items():
                assert torch.equal(d[k].view(torch.int32), v.view(torch.int32)), (drop, where, k, "changed by a refused call")
    # the legal setting takes every one of these calls
    for drop in expected:
        tune = _lib.tuning(score_splits=1, score_half_groups=0, score_offsets32=1, score_lane_ids=1)
        d = fresh()
        a = refusal_args(c, {k: (None if k in drop else v) for k, v in d.items()}, tuning=C.addressof(tune))
        assert L.mke_triple_score_step(C.byref(a), _lib._stream()) == 0, (drop, L.mke_last_error())
        sync()
        assert torch.equal(d["ref_count"], dev(o.ref_count))
    # neg_code beside ref_count where the code-word form is not legal: the ref_count form runs and resets the counts
    for where, f in (("o64", sc.Form(0, 1, 0, 1, 0, 1)), ("rounds", sc.Form(0, 1, 1, 0, 0, 1)), ("det", sc.Form(1, 1, 1, 1, 0, 1))):
        d = fresh()
        assert call(d, where, ()) == 0, (where, L.mke_last_error())
        sync()
        w = sc.reference(c, f)
        got = {k: host(d[k]) for k in ("partials", "ent", "acc", "ref_count", "touched_ent", "touched_rel")}
        if where == "det":
            got.update(stage_rows=host(d["stage_rows"]), stage_keys=host(d["stage_keys"]))
        else:
            got.update(grad_ent=host(d["grad_ent"]), grad_rel=host(d["grad_rel"]))
        problems, _ = sc.compare(got, w)
        assert not problems, (where, problems)
        assert not got["ref_count"][w["in_place_rows"]].any() and len(w["in_place_rows"])


def test_refusals_launch_nothing():
    """Those of mke_triple_score_step are held by test_abi.py; the two small entry points refuse before any launch as well."""
    from multike_amd import _lib
    L, one = _lib.lib(), C.c_void_p(16)
    assert L.mke_stage_reduce(one, one, one, C.c_int64(4), C.c_int(20), one, one, one, one, C.c_int32(1), None) == -2 and b"stride" in L.mke_last_error()
    assert L.mke_stage_reduce(one, one, one, C.c_int64(-1), C.c_int(16), one, one, one, one, C.c_int32(1), None) == -2
    assert L.mke_stage_reduce(one, None, one, C.c_int64(4), C.c_int(16), one, one, one, one, C.c_int32(1), None) == -1
    assert L.mke_count_entity_refs(one, one, C.c_int64(2), one, one, C.c_int64(5), C.c_int(2), one, None) == -2 and b"grouped" in L.mke_last_error()
    assert L.mke_count_entity_refs(one, one, C.c_int64(2), one, one, C.c_int64(4), C.c_int(2), None, None) == -1

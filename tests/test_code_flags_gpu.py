"""Code-word steps of mke_relation_steps without entity touched flags ("code_flags", the default) against the same steps with
flags: the update launch finds its rows in the step's row of the bake's bitmap (pair 11: the chunk walk) and among the step's
positives (pair 01: the list walk) instead of scanning flags the score launch stored.

Every case fills a mke_relation_plan by hand and runs three consecutive steps.  Each step is run from ONE state with the option
off and on (the state carried to the next step is the off run's), so both runs of a step see the same bits going in, and the
three steps are run once more in one call with the option on (rows 1 and 2 of the chunk's bitmap).

What is compared bit for bit, on against off: the per-step loss partials; every row outside the step's reference set (also
against its value before the step); every entity row the score launch finishes in place; with one negative per positive also
the rows a single positive names once (one atomic add onto zero).  With more negatives a group's flush may come from several
wavefronts, and every other referenced row is a sum of atomic adds whose order differs from run to run: those rows are held to
the tolerance this project uses between two forms of the same step (tests/test_runner_codes_gpu.py: rtol 1e-4, atol 1e-6).  The
bound of tests/test_update_exact_gpu.py is for the update GIVEN its gradient and does not cover a gradient summed in another
order, so it is not used for them.

Shapes: strides 16, 80 and 256; tables of 15, 16, 17, 33 and 40 rows (bitmap word edges, a last word partly used); 1 and 25
negatives per positive -- 25 only for 33 and 40 rows, the sampler refuses a population smaller than neg_per_pos --; batches of
1, 7 and 300 positives and a step with none; a hub-row declaration; and one table of 20,000 rows (several update blocks, chunk 16;
chunk 64, the whole-wavefront rows, at stride 256).  Step 0 of every batch of 7 or more has a positive with h == t and two
positives sharing a head; the other situations (a positive's tail drawn as a negative, a positive drawn as its own negative, a
row that only a positive's head names, a row one negative names) come out of the sampler, and the last test asserts that the
cases show every one of them.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
N_REL = 5
LR = 0.01


class Case:
    def __init__(self, stride, n_ent, npp, sizes, hub=False, chunk=0):
        self.stride, self.dim, self.n_ent, self.npp, self.sizes, self.hub, self.chunk = stride, stride - 5, n_ent, npp, tuple(sizes), hub, chunk
        self.id = f"s{stride}-e{n_ent}-n{npp}-b{'_'.join(map(str, sizes))}" + ("-hub" if hub else "") + (f"-c{chunk}" if chunk else "")


def _cases():
    out = []
    for stride in (16, 80, 256):
        for n_ent in (15, 16, 17, 33, 40):
            for npp in (1, 25):
                if n_ent < npp:      # mke_neg_sample: MKE_E_SHAPE for a population smaller than neg_per_pos
                    continue
                for b in (1, 7, 300):
                    out.append(Case(stride, n_ent, npp, (b, b, b)))
        out.append(Case(stride, 40, 25, (7, 0, 7)))
        out.append(Case(stride, 40, 1, (7, 0, 7)))
        out.append(Case(stride, 40, 25, (300, 300, 300), hub=True))
        out.append(Case(stride, 40, 1, (7, 7, 7), hub=True))
    out.append(Case(80, 20000, 25, (300, 300, 300)))
    out.append(Case(80, 20000, 1, (300, 300, 300)))
    out.append(Case(256, 20000, 25, (300, 300, 300), chunk=64))
    return out


CASES = _cases()


def _inputs(c):
    rng = np.random.default_rng(abs(hash((c.stride, c.n_ent, c.npp, c.sizes, c.hub))) % (1 << 31))
    n = sum(c.sizes)
    ph, pt = rng.integers(0, c.n_ent, n).astype(np.int32), rng.integers(0, c.n_ent, n).astype(np.int32)
    pr = rng.integers(0, N_REL, n).astype(np.int32)
    if c.sizes[0] >= 7:
        pt[0] = ph[0]            # h == t
        ph[2] = ph[1]            # two positives sharing a head
    off = np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int64)

    def table(rows):
        t = np.zeros((rows, c.stride), np.float32)
        t[:, :c.dim] = rng.normal(0.0, 1.0, (rows, c.dim)) / np.sqrt(c.dim)
        return t
    return ph, pr, pt, off, table(c.n_ent), table(N_REL)


class State:
    """The device buffers of one plan; clone() copies what a step changes."""
    NAMES = ("ent", "rel", "ent_acc", "rel_acc", "ent_grad", "rel_grad", "ent_touched", "rel_touched", "refcount", "loss")

    def __init__(self, c, ent, rel):
        d = "cuda"
        self.n_hot, self.copies = (3, 2) if c.hub else (0, 1)
        self.ent, self.rel = torch.as_tensor(ent, device=d), torch.as_tensor(rel, device=d)
        self.ent_acc, self.rel_acc = torch.full_like(self.ent, 0.1), torch.full_like(self.rel, 0.1)
        self.ent_grad = torch.zeros(c.n_ent + self.n_hot * self.copies, c.stride, device=d)
        self.rel_grad = torch.zeros(2, N_REL, c.stride, device=d)
        self.ent_touched = torch.full((c.n_ent,), SENT, dtype=torch.int32, device=d)
        self.rel_touched = torch.zeros(N_REL, dtype=torch.int32, device=d)
        self.refcount = torch.zeros(2 * c.n_ent, dtype=torch.int32, device=d)
        self.loss = torch.zeros(3, 2048, dtype=torch.float64, device=d)

    def clone(self):
        s = object.__new__(State)
        s.n_hot, s.copies = self.n_hot, self.copies
        for k in self.NAMES:
            setattr(s, k, getattr(self, k).clone())
        return s

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in self.NAMES}


class World:
    """What the steps of a case share and do not change, and the scratch the sampler and the bake write."""

    def __init__(self, c):
        from multike_amd import _lib
        self.c = c
        self.ph, self.pr, self.pt, self.off, ent, rel = _inputs(c)
        d = "cuda"
        self.pos = tuple(torch.as_tensor(x, device=d) for x in (self.ph, self.pr, self.pt))
        self.off_dev = torch.as_tensor(self.off, device=d)
        cap = max(1, sum(c.sizes) * c.npp)
        self.neg = tuple(torch.zeros(cap, dtype=torch.int32, device=d) for _ in range(3))
        self.neg_code = torch.zeros(cap, dtype=torch.int32, device=d)
        self.words = _lib.neg_code_row_words(c.n_ent)
        self.code_bits = torch.zeros(3 * self.words, dtype=torch.int32, device=d)
        self.state0 = State(c, ent, rel)
        self.hot_rows = np.array([0, c.n_ent // 2, c.n_ent - 1], np.int32) if c.hub else np.zeros(0, np.int32)
        slot = np.full(c.n_ent, -1, np.int32)
        slot[self.hot_rows] = np.arange(len(self.hot_rows))
        self.hot_slot = torch.as_tensor(slot, device=d)

    def plan(self, st):
        from multike_amd import _lib
        c, f32, i32 = self.c, torch.float32, torch.int32
        p = _lib.RelationPlanStruct()
        p.ent_table, p.n_ent, p.ent_normalize = _lib.ptr(st.ent, f32, "ent"), c.n_ent, 1
        p.rel_table, p.n_rel, p.rel_normalize = _lib.ptr(st.rel, f32, "rel"), N_REL, 1
        p.ent_acc, p.rel_acc = _lib.ptr(st.ent_acc, f32, "a"), _lib.ptr(st.rel_acc, f32, "a")
        p.ent_grad, p.rel_grad, p.rel_grad_copies = _lib.ptr(st.ent_grad, f32, "g"), _lib.ptr(st.rel_grad, f32, "g"), 2
        p.ent_touched, p.rel_touched = _lib.ptr(st.ent_touched, i32, "t"), _lib.ptr(st.rel_touched, i32, "t")
        p.ent_ref_count = _lib.ptr(st.refcount, i32, "rc")
        p.overlap, p.neg_chunk_capacity = 0, self.neg_code.numel()
        p.stride, p.dim = c.stride, c.dim
        p.pos_h, p.pos_r, p.pos_t = (_lib.ptr(x, i32, "pos") for x in self.pos)
        p.pos_kg = None
        p.step_off, p.n_steps = self.off.ctypes.data, 3
        for k in (0, 1):
            p.sides[k].ent_list, p.sides[k].ent_lo, p.sides[k].n_ent = None, 0, c.n_ent
        p.neg_per_pos, p.max_try, p.sample_chunk, p.negatives_ready = c.npp, 3, 3, 0
        p.neg_h, p.neg_r, p.neg_t = (_lib.ptr(x, i32, "neg") for x in self.neg)
        p.seed_lo, p.seed_hi, p.stream_id = 17, 4, 0
        p.optimizer, p.lr, p.scale = _lib.OPT_ADAGRAD, LR, 1.0
        p.loss_partials, p.loss_ring = _lib.ptr(st.loss, torch.float64, "loss"), 3
        p.tag_base = 1000
        if c.hub:
            p.hot.slot, p.hot.n_hot, p.hot.copies, p.hot.row0 = _lib.ptr(self.hot_slot, i32, "slot"), st.n_hot, st.copies, c.n_ent
        p.step_off_dev = _lib.ptr(self.off_dev, torch.int64, "off")
        p.neg_code = _lib.ptr(self.neg_code, i32, "code")
        p.code_bits, p.code_bits_words = _lib.ptr(self.code_bits, i32, "bits"), self.code_bits.numel()
        return p

    def run(self, st, s0, s1, flags_off):
        """steps [s0, s1) on `st` with code_flags = 0 (flags_off) or 1"""
        from multike_amd import _lib
        old = _lib.set_option("code_flags", 0 if flags_off else 1)
        chunk = _lib.set_option("update_chunk", self.c.chunk)
        try:
            _lib.relation_steps(self.plan(st), s0, s1)
            torch.cuda.synchronize()
        finally:
            _lib.set_option("code_flags", old)
            _lib.set_option("update_chunk", chunk)

    def ids(self, s):
        """What step s referenced, from the words the last run of it alone left: the negatives' ids, the entity rows finished in
        place, the contributions each entity / relation row took in the scratch, the reference set."""
        from multike_amd import _lib
        c = self.c
        lo, hi = int(self.off[s]), int(self.off[s + 1])
        ph, pr, pt = self.ph[lo:hi], self.pr[lo:hi], self.pt[lo:hi]
        code = self.neg_code.cpu().numpy()[:(hi - lo) * c.npp]
        g = np.repeat(np.arange(hi - lo), c.npp)
        e = code & ((1 << _lib.CODE_ENT_BITS) - 1)
        fast, head, excl = (code & _lib.CODE_FAST) != 0, (code & _lib.CODE_HEAD) != 0, (code & _lib.CODE_EXCL) != 0
        nh, nt = np.where(fast & head, e, ph[g]).astype(np.int32), np.where(fast & ~head, e, pt[g]).astype(np.int32)
        refs = np.zeros(c.n_ent, np.int64)
        for x in (ph, pt, e[fast]):
            np.add.at(refs, x, 1)
        assert np.array_equal(excl[fast], refs[e[fast]] == 1), "the bake's exclusive bit"   # (not read in a word without `fast`)
        same = ph[ph == pt]                  # h == t and nothing else on the row: +g and -g cancel exactly, the visit changes nothing
        cancel = np.zeros(c.n_ent, bool)
        cancel[same[refs[same] == 2]] = True
        contrib = np.zeros(c.n_ent, np.int64)
        for x in (ph, pt, e[fast & ~excl], ph[g[~fast]], pt[g[~fast]]):
            np.add.at(contrib, x, 1)
        crel = np.zeros(N_REL, np.int64)
        for x in (pr, pr[g[~fast]]):
            np.add.at(crel, x, 1)
        pair = np.where(refs == 0, 0, np.where(refs == 1, 1, 3))
        return dict(pos=(ph, pr, pt), neg=(nh, pr[g].astype(np.int32), nt), refs=refs, contrib=contrib, crel=crel, pair=pair, cancel=cancel,
                    inplace=np.unique(e[fast & excl]), own=int((~fast).sum()),
                    tail_as_neg=bool(np.isin(e[fast], pt).any()),
                    head_only=bool(((refs[ph] == 1)).any()), neg_once=bool((fast & excl).any()), both=bool((pair == 3).any()))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)))


@functools.lru_cache(maxsize=None)
def _run(k):
    """Every step of case k from one state with the option off and on, then the three steps in one call with it on."""
    c = CASES[k]
    w = World(c)
    st = w.state0.clone()
    steps = []
    for s in range(3):
        st.ent_touched.fill_(SENT)          # the flags the off run of the step before left
        before = st.host()
        on = st.clone()
        w.run(st, s, s + 1, flags_off=True)
        w.run(on, s, s + 1, flags_off=False)
        rows = w.code_bits.cpu().numpy()[:w.words].view(np.uint32).copy()      # row 0: the step's, of the run of it alone
        steps.append(dict(before=before, off=st.host(), on=on.host(), ids=w.ids(s), bits=rows))
    whole = w.state0.clone()
    w.run(whole, 0, 3, flags_off=False)
    return dict(case=c, steps=steps, whole=whole.host(), final=st.host(), world=w)


def _check_tables(c, ids, a, b, exact_also_pos):
    """rows of run a against run b of one step: bit for bit where one contribution or none went in, the form-to-form band else"""
    exact = np.ones(c.n_ent, bool)
    exact[ids["contrib"] > 1] = False
    if not exact_also_pos:
        exact[ids["contrib"] > 0] = False
    exact[ids["inplace"]] = True
    for name in ("ent", "ent_acc"):
        assert _same(a[name][exact], b[name][exact]), name
        np.testing.assert_allclose(a[name][~exact], b[name][~exact], rtol=1e-4, atol=1e-6, err_msg=name)
    rex = (ids["crel"] == 0) | ((ids["crel"] == 1) & exact_also_pos)
    for name in ("rel", "rel_acc"):
        assert _same(a[name][rex], b[name][rex]), name
        np.testing.assert_allclose(a[name][~rex], b[name][~rex], rtol=1e-4, atol=1e-6, err_msg=name)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.id for c in CASES])
def test_bitmap_steps_equal_flag_steps(k):
    r = _run(k)
    c = r["case"]
    for s, st in enumerate(r["steps"]):
        ids, before, off, on = st["ids"], st["before"], st["off"], st["on"]
        # the bitmap row the update read is the definition's
        pair = np.zeros(c.n_ent, np.int64)
        for e in range(c.n_ent):
            pair[e] = (int(st["bits"][e >> 4]) >> ((e & 15) * 2)) & 3
        assert np.array_equal(pair, ids["pair"]), f"step {s}: bitmap"
        assert _same(off["loss"][s], on["loss"][s]), f"step {s}: loss partials"
        _check_tables(c, ids, on, off, exact_also_pos=c.npp == 1)
        for run in (off, on):
            assert not run["ent_grad"].any() and not run["rel_grad"].any(), f"step {s}: gradient scratch not zero"
            assert not run["refcount"].any()
            out = ids["refs"] == 0
            for name in ("ent", "ent_acc"):
                assert _same(run[name][out], before[name][out]), f"step {s}: {name} outside the reference set"
            rout = ids["crel"] == 0
            for name in ("rel", "rel_acc"):
                assert _same(run[name][rout], before[name][rout]), f"step {s}: {name} outside the reference set"
        assert (on["ent_touched"] == SENT).all(), f"step {s}: entity flags written with the option on"
        flagged = off["ent_touched"] != SENT
        assert np.array_equal(flagged, ids["contrib"] > 0), f"step {s}: flags of the flag form"
        # rows that changed: every referenced row has a nonzero gradient, so the accumulator of a visited row grows
        ch_on = (_bits(on["ent_acc"]) != _bits(before["ent_acc"])).any(axis=1)
        ch_off = (_bits(off["ent_acc"]) != _bits(before["ent_acc"])).any(axis=1)
        assert np.array_equal(ch_on, ch_off), f"step {s}: rows visited"
        seen = ~ids["cancel"]
        assert np.array_equal(ch_on[seen], (ids["refs"] > 0)[seen]), f"step {s}: rows visited against the reference set"
    # three steps in one call (rows 1 and 2 of the chunk's bitmap) against the steps one by one
    whole, final = r["whole"], r["final"]
    for name in ("ent", "ent_acc", "rel", "rel_acc"):
        np.testing.assert_allclose(whole[name], final[name], rtol=1e-4, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(whole["loss"].sum(axis=1), final["loss"].sum(axis=1), rtol=2e-6)
    assert not whole["ent_grad"].any() and not whole["rel_grad"].any() and (whole["ent_touched"] == SENT).all()


def test_forty_rows_against_the_float64_oracle():
    """Option on, 40 rows, 25 negatives, batches of 7, against mko_relation_step in float64 on the device's own negatives: the
    tolerance of tests/test_runner_gpu.py for the native loop against the oracle (loss rtol 1e-5, tables rtol 5e-4 / atol 5e-6)."""
    k = next(i for i, c in enumerate(CASES) if c.id == "s80-e40-n25-b7_7_7")
    r = _run(k)
    c, w = r["case"], r["world"]
    h0 = w.state0.host()
    e64, r64 = h0["ent"][:, :c.dim].astype(np.float64), h0["rel"][:, :c.dim].astype(np.float64)
    a64, b64 = np.full_like(e64, 0.1), np.full_like(r64, 0.1)
    orc = co.RelationStepOracle(c.n_ent, N_REL, c.dim, np.float64)
    st = w.state0.clone()
    for s in range(3):
        w.run(st, s, s + 1, flags_off=False)
        ids = w.ids(s)
        want = orc.step(e64, r64, a64, b64, ids["pos"], ids["neg"], LR)
        got = float(st.loss[s].sum())
        np.testing.assert_allclose(got, want, rtol=1e-5)
    got = st.host()
    np.testing.assert_allclose(got["ent"][:, :c.dim], e64, rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(got["rel"][:, :c.dim], r64, rtol=5e-4, atol=5e-6)
    np.testing.assert_allclose(got["ent_acc"][:, :c.dim], a64, rtol=5e-4, atol=5e-6)


def test_cases_show_every_listed_situation():
    seen = dict(own=False, tail_as_neg=False, head_only=False, neg_once=False, both=False, hub_list=False, hub_chunk=False)
    for k, c in enumerate(CASES):
        r = _run(k)
        for st in r["steps"]:
            ids = st["ids"]
            for f in ("own", "tail_as_neg", "head_only", "neg_once", "both"):
                seen[f] = seen[f] or bool(ids[f])
            if c.hub:
                hp = ids["pair"][r["world"].hot_rows]
                seen["hub_list"] = seen["hub_list"] or bool((hp == 1).any())
                seen["hub_chunk"] = seen["hub_chunk"] or bool((hp == 3).any())
    assert all(seen.values()), seen


def test_bitmap_refused_where_no_kernel_takes_it():
    from multike_amd import _lib
    L = _lib.lib()
    n, stride = 40, 16
    f = lambda *s: torch.zeros(*s, device="cuda")
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    table, acc, grad, bits, pos, slot_of, src = f(n, stride) + 1, f(n, stride) + 0.1, f(2, n, stride), i(3), i(4), i(n) - 1, f(4, stride)

    def call(**kw):
        t = (_lib.UpdateTableStruct * 1)()
        t[0].table, t[0].acc, t[0].grad = table.data_ptr(), acc.data_ptr(), grad.data_ptr()
        t[0].n_rows, t[0].normalize, t[0].grad_copies = n, 1, 1
        t[0].bits, t[0].pos_h, t[0].pos_t, t[0].n_pos = bits.data_ptr(), pos.data_ptr(), pos.data_ptr(), 4
        for k, v in kw.items():
            setattr(t[0], k, v)
        rc = L.mke_rows_update_multi(t, 1, 5, stride, stride, _lib.OPT_ADAGRAD, 0.01, None)
        torch.cuda.synchronize()
        return rc
    before = table.clone()
    assert call(grad_copies=2) == _lib.E_UNSUPPORTED
    assert call(slot_of=slot_of.data_ptr(), src_rows=src.data_ptr(), n_ranks=1, capacity=4) == _lib.E_UNSUPPORTED
    assert call(pos_h=None) == _lib.E_NULL
    assert torch.equal(table, before)
    assert call() == _lib.OK          # an all-zero bitmap row: nothing to visit
    assert torch.equal(table, before)

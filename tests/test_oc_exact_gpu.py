"""The owner-computes (sharded) relation step at the C ABI, exactly: every phase alone on staged inputs, then the whole step for
every rank of G — all in ONE process, the test playing the ranks in turn and doing the collectives itself (all-gather = the send
blocks side by side, reduce-scatter / all-reduce = float32 sums in rank order; peer-direct forms staged with n_peers = n_ranks,
peer_v[o] = virtual rank o's send block, peer_g[o] = this rank's slice of virtual rank o's inbox).  Case table, reference, bounds and
mutants: oc_cases.py (test_oc_cases.py proves that the table catches every mutant and that the reference agrees with the dense
oracle).  Values that pass through rsqrtf / __expf / __logf / rcp / adagrad_scale are compared with the float64 reference within
its derived bound; gv_sum, apply, the relation rows and the long rows' partial slots of the second pass (quarter inputs) and
every structural output bit for bit.  Every test prints RATIO lines: the largest |device - reference| / bound it saw.

Measured on the MI355X, the largest |device - reference| / bound over the whole table (information, not a tolerance; a ratio
above 1 is a finding).  No defect was found: every bit-for-bit comparison is equal and
    mke_oc_bases          send block 0.23
    mke_oc_score          g_all 0.33, em_coef 0.25, loss 0.19; atomics form: scratch rows 0.29, rows finished in place 0.43,
                          their accumulators 0.45
    mke_oc_pass2          entity rows 0.41, accumulators 0.45 (long rows through the combine among them, at every width)
    the whole step        entity rows 0.43, accumulators 0.45, relation table 0.14, its accumulator 0.44, loss 0.04
in all five forms (the entity-major forms share their figures to the digit: the same sums in the same order).  The figures near
0.45 are the half ulp of a stored value against the whole ulp `Arith.stored` charges for it.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oc_cases as oc
import oc_owned_util as OU
from multike_amd import _abi, _lib
from rows_cases import OLD_TAG, SENTINEL, TAG

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEV = "cuda"
CASES = {c.id: c for c in oc.CASES}
RUNS_OF = {cid: [r for r in oc.RUNS if r.case.id == cid] for cid in CASES}
SMALL = [cid for cid, c in CASES.items() if c.tag != "trip"]
ATM = [cid for cid in CASES if any(r.form == "atm" for r in RUNS_OF[cid])]
EM = [cid for cid in SMALL if any(r.form != "atm" for r in RUNS_OF[cid])]


def T(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.as_tensor(a, device=DEV) if a.size else torch.zeros(1, dtype=torch.as_tensor(a).dtype, device=DEV)


def N_(t):
    return t.detach().cpu().numpy()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=4)
def _ref(cid, quarter, staged=True):
    return oc.Ref(CASES[cid], quarter, "", staged)


def _report(what, cid, named):
    problems, ratios = oc.compare(named)
    for k, v in ratios.items():
        print(f"RATIO {what}:{k} {v:.4f} {cid}")
    assert not problems, (cid, what, problems)
    return ratios


class Step:
    """The device buffers of one virtual rank and the descriptor of one of its parts."""

    def __init__(self, c, S, g, em=False):
        self.c, self.S, self.g = c, S, g
        self.copies = 1 if em else c.rel_copies
        nl, st = c.n_local, c.stride
        self.n_grad = nl + (c.hot * c.hot_copies if c.hot else 0)
        self.ent, self.acc = T(oc.local_rows(c, S.ent, g)), T(oc.local_rows(c, S.acc_e, g))
        tail = np.full((1, st), np.nan, dtype=f32)
        self.rel, self.rel_acc = T(np.concatenate([S.rel, tail])), T(np.concatenate([S.acc_r, tail]))
        self.ent_grad = torch.zeros(self.n_grad + 1, st, device=DEV)
        self.ent_grad[self.n_grad] = SENTINEL
        self.rel_grad = torch.zeros(self.copies * c.n_rel + 1, st, device=DEV)
        self.rel_grad[-1] = SENTINEL
        self.te, self.tr = (torch.full((n + 64,), OLD_TAG, dtype=torch.int32, device=DEV) for n in (nl, c.n_rel))
        self.te[nl:], self.tr[c.n_rel:] = TAG, TAG
        self.rc = torch.zeros(nl + 1, dtype=torch.int32, device=DEV)
        self.rc[nl] = 9
        self.pos = [T(a, np.int32) for a in (S.ph, S.pr, S.pt, S.sh, S.st)]
        self.codes = OU.dev32(S.codes)
        self.pw = T(S.pw) if S.pw is not None else None
        self.hot = T(S.hot_slot[g]) if S.hot_slot is not None else None
        self.own = [(T(S.own_h[k][g], np.int32), T(S.own_t[k][g], np.int32)) for k in range(len(S.parts))]
        self.keep = []

    def desc(self, k, form="atm", quarter=0, refcount=None):
        c, S, g = self.c, self.S, self.g
        lo, hi = S.parts[k]
        s = _lib.OcStepStruct()
        s.ent, s.ent_acc, s.ent_grad, s.ent_touched = self.ent.data_ptr(), self.acc.data_ptr(), self.ent_grad.data_ptr(), self.te.data_ptr()
        if (c.refcount and form == "atm") if refcount is None else refcount:
            s.ref_count = self.rc.data_ptr()
        s.n_local, s.n_rel, s.rel_grad_copies = c.n_local, c.n_rel, self.copies
        s.rel, s.rel_acc, s.rel_grad, s.rel_touched = self.rel.data_ptr(), self.rel_acc.data_ptr(), self.rel_grad.data_ptr(), self.tr.data_ptr()
        s.stride, s.dim, s.rank, s.n_ranks = c.stride, c.dim, g, c.G
        s.pos_h, s.pos_r, s.pos_t, s.slot_h, s.slot_t = (t.data_ptr() + 4 * lo for t in self.pos)
        s.n_pos, s.per = hi - lo, S.per[k]
        oh, ot = self.own[k]
        s.own_h, s.n_own_h, s.own_t, s.n_own_t = oh.data_ptr(), len(S.own_h[k][g]), ot.data_ptr(), len(S.own_t[k][g])
        s.neg_per_pos, s.capacity = c.N, S.C
        s.codes = self.codes.data_ptr()
        for h in range(c.G):
            s.code_off[h] = S.code_off[k][h]
        s.optimizer, s.lr, s.scale, s.tag = (_lib.OPT_ADAGRAD if c.opt == "adagrad" else _lib.OPT_SGD), c.lr, c.scale, TAG
        if self.pw is not None:
            s.pos_w = self.pw.data_ptr() + 4 * lo
        if self.hot is not None and form == "atm":
            s.hot.slot, s.hot.n_hot, s.hot.copies, s.hot.row0 = self.hot.data_ptr(), c.hot, c.hot_copies, c.n_local
        tun = _lib.tuning(oc_score_quarter=quarter)
        self.keep.append(tun)
        s.tuning = _lib.tuning_ptr(tun)
        return s


def _call(fn, *args):
    rc = fn(*args)
    assert rc == 0, _lib.lib().mke_last_error()


def _void(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


# ---- 1 / 2. bases and the reference counts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SMALL + [cid for cid in ATM if cid not in SMALL])
def test_bases_and_count(cid):
    """HR = h^ + r^, RT = r^ - t^ in slot order, nothing beyond the owned slots; mke_oc_count by enumeration (negatives of every home
    rank, owned heads and tails, hub rows excluded); MKE_OC_BASES | MKE_OC_COUNT in one launch gives both again."""
    c = CASES[cid]
    R, S, g, L = _ref(cid, 0), oc.stage(c), c.rank, _lib.lib()
    named = []
    for k in range(len(S.parts)):
        want_rc = oc.ref_counts(c, S, k, g)
        for both in (False, True):
            dv = Step(c, S, g)
            send = torch.full((2 * S.C + 1, c.stride), SENTINEL, device=DEV)
            s = dv.desc(k, refcount=True)
            if both:
                _call(L.mke_oc_run, C.byref(s), _abi.OC_BASES | _abi.OC_COUNT, _void(send), None, C.c_int64(0), None, None, None, _stream())
            else:
                _call(L.mke_oc_bases, C.byref(s), _void(send), _stream())
                _call(L.mke_oc_count, C.byref(s), _stream())
            torch.cuda.synchronize()
            named += [(f"send{k}{'+count' if both else ''}", N_(send), R.send(k, g))]
            assert np.array_equal(N_(dv.rc), want_rc), (cid, k, both)
            assert np.array_equal(N_(dv.ent), oc.local_rows(c, S.ent, g), equal_nan=True)
    _report("bases", cid, named)


# ---- 3. the score launch ----------------------------------------------------------------------------------------------------------
def _owned(c, S, g):
    codes = ((S.cent << 1) | S.cside)
    if c.N:
        codes[:, 0] |= S.need_hr * oc.NEED_HR + S.need_rt * oc.NEED_RT
    cap = max(1, -(-c.n_pos // c.G) * c.N)
    recv, counts, _ = OU.exchange(codes.ravel(), c.n_pos, c.N, c.G, g, cap)
    own_rec, own_off, _ = OU.owned_index(recv, counts, c.G, cap, c.n_pos)
    return own_rec, own_off


def _score(dv, k, form, quarter, vall, coef=None, own=None):
    """One mke_oc_score on part k: -> (g_all rows of this writer [G 2C + 1, stride], loss partials, mirror or None, inbox or None)."""
    c, S, g = dv.c, dv.S, dv.g
    st, C2 = c.stride, 2 * S.C
    s = dv.desc(k, form, quarter)
    lo, _ = S.parts[k]
    if form != "atm":
        s.em_coef, s.em_pos0, s.em_chunks = coef.data_ptr(), lo, len(S.parts)
    if form in ("own", "mirown"):
        s.own_rec, s.own_off, s.codes = own[0].data_ptr(), own[1].data_ptr() + 4 * lo, None
    lossp = torch.full((_lib.LOSS_PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
    v = T(vall)
    mirror = inbox = None
    if form in ("mir", "mirown"):
        inbox = torch.full((c.G, c.G, C2, st), SENTINEL, device=DEV)          # [owner][writer][slot]
        mirror = torch.full((c.G, C2, st), SENTINEL, device=DEV)
        s.n_peers = c.G
        for o in range(c.G):
            s.peer_v[o], s.peer_g[o] = v.data_ptr() + 4 * o * C2 * st, inbox.data_ptr() + 4 * (o * c.G + g) * C2 * st
        _call(_lib.lib().mke_oc_score, C.byref(s), _void(mirror), C.c_int64(C2 * st), None, _void(lossp), _stream())
    else:
        g_all = torch.full((c.G * C2 + 1, st), SENTINEL, device=DEV)
        _call(_lib.lib().mke_oc_score, C.byref(s), _void(v), C.c_int64(C2 * st), _void(g_all), _void(lossp), _stream())
    torch.cuda.synchronize()
    if inbox is not None:
        ib = N_(inbox)
        others = np.delete(ib, g, axis=1)
        assert (others == SENTINEL).all(), "a slice of another writer was written"
        g_all = np.concatenate([ib[:, g].reshape(c.G * C2, st), np.full((1, st), SENTINEL, dtype=f32)])
    else:
        g_all = N_(g_all)
    return g_all, N_(lossp), None if mirror is None else N_(mirror)


def _atm_initial(dv, want):
    """SENTINEL in every scratch row that must not be written, zeros in the rows that receive adds (the ABI's invariant)."""
    dv.ent_grad.copy_(T(np.where(want["ent_grad"][0] == SENTINEL, f32(SENTINEL), f32(0)).astype(f32)))


@pytest.mark.parametrize("cid", list(CASES))
def test_score(cid):
    """Every (form, kernel) of the case on staged all-gathered vectors: the gradient-vector slots (the rest still SENTINEL), the
    coefficients (entity-major), the loss (NaN-poisoned partials all finite), the mirror bit for bit (peer-direct), and in the
    atomics form the scratch rows, flags, rows finished in place and reference counts."""
    c = CASES[cid]
    S, g = oc.stage(c), c.rank
    own = _owned(c, S, g) if any(r.form in ("own", "mirown") for r in RUNS_OF[cid]) else None
    worst = {}
    for run in RUNS_OF[cid]:
        R = _ref(cid, run.quarter)
        for k in range(len(S.parts)):
            if run.form == "atm" and len(S.parts) > 1:
                continue
            want = R.score(k, g, run.form)
            dv = Step(c, S, g)
            coef = torch.full((c.n_pos * (c.N + 1) + 1,), SENTINEL, device=DEV)
            if run.form == "atm":
                _atm_initial(dv, want)
                dv.rc.copy_(T(oc.ref_counts(c, S, k, g)))
            g_all, lossp, mirror = _score(dv, k, run.form, run.quarter, R.vall(k), coef, own)
            assert np.isfinite(lossp).all(), (run.id, "a loss partial was not written")
            named = [("g_all", g_all, want["g_all"]), ("loss", lossp.sum(), want["loss"])]
            if run.form != "atm":
                named += [("coef", N_(coef), want["coef"])]
                assert np.array_equal(N_(dv.ent), oc.local_rows(c, S.ent, g), equal_nan=True) and not N_(dv.ent_grad)[:-1].any()
            else:
                named += [("ent_grad", N_(dv.ent_grad), want["ent_grad"]), ("ent", N_(dv.ent), want["ent"]), ("acc", N_(dv.acc), want["acc"]),
                          ("touched_ent", N_(dv.te), want["touched_ent"])]
                if c.refcount:
                    named += [("ref_count", N_(dv.rc), want["ref_count"])]
                assert (N_(coef) == SENTINEL).all()
            if mirror is not None:
                named += [("mirror", mirror, (want["mirror"], None))]
            for kk, v in _report(f"score/{run.form}-q{run.quarter}", cid, named).items():
                worst[kk] = max(worst.get(kk, 0.0), v)
    for kk, v in worst.items():
        print(f"RATIO score:worst:{kk} {v:.4f} {cid}")


# ---- 4 / 5. apply and gv_sum on quarters: bit for bit -------------------------------------------------------------------------------
def _quarters(c, shape, seed):
    rng = np.random.default_rng([seed, c.stride, c.dim])
    return np.where(np.arange(c.stride) < c.dim, oc.quarters(rng, shape), 0.0).astype(f32)


@pytest.mark.parametrize("cid", [cid for cid in ATM if cid in SMALL])
def test_apply_is_exact_on_quarters(cid):
    """Collective gv, and the peer inbox summed in rank order: scratch rows, hub copies, relation copies and both flag arrays equal the
    float64 sums (exact: multiples of 1/4) bit for bit; SENTINEL rows stay.  An entity-major step is refused, nothing launched."""
    c = CASES[cid]
    R, S, g, L = _ref(cid, 0), oc.stage(c), c.rank, _lib.lib()
    C2 = 2 * S.C
    inbox = _quarters(c, (c.G, C2 + 1, c.stride), 5)
    gv = inbox[:, :C2].astype(f64).sum(0)
    want = R.apply(0, g, gv, np.zeros_like(gv))
    for peer in (False, True):
        dv = Step(c, S, g)
        dv.ent_grad.copy_(T(np.where(want["ent_grad"][0] == SENTINEL, f32(SENTINEL), f32(0)).astype(f32)))
        dv.rel_grad.copy_(T(np.where(want["rel_grad"][0] == SENTINEL, f32(SENTINEL), f32(0)).astype(f32)))
        s = dv.desc(0)
        src = T(inbox[:, :C2]) if peer else T(gv, f32)
        if peer:
            s.n_peers = c.G
            for o in range(c.G):
                s.peer_v[o] = s.peer_g[o] = src.data_ptr()
        _call(L.mke_oc_apply, C.byref(s), _void(src), _stream())
        torch.cuda.synchronize()
        _report("apply", cid, [(name, N_(buf), (want[name][0], None)) for name, buf in (("ent_grad", dv.ent_grad), ("rel_grad", dv.rel_grad))] +
                [("touched_ent", N_(dv.te), want["touched_ent"]), ("touched_rel", N_(dv.tr), want["touched_rel"])])
    dv = Step(c, S, g)
    s = dv.desc(0)
    s.em_coef, s.em_chunks = dv.ent.data_ptr(), 1
    assert L.mke_oc_apply(C.byref(s), _void(T(gv, f32)), _stream()) == _abi.E_UNSUPPORTED
    assert L.mke_oc_run(C.byref(s), _abi.OC_APPLY, None, None, C.c_int64(0), None, _void(T(gv, f32)), None, _stream()) == _abi.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not N_(dv.ent_grad)[:-1].any() and not N_(dv.rel_grad)[:-1].any() and (N_(dv.te)[:c.n_local] == OLD_TAG).all()


@pytest.mark.parametrize("cid", SMALL)
def test_gv_sum_is_exact_on_quarters(cid):
    """gv[slot] = sum over the writers in rank order, for every owned slot; every other slot of the block keeps its SENTINEL.  Refused
    outside peer-direct entity-major steps."""
    c = CASES[cid]
    S, g, L = oc.stage(c), c.rank, _lib.lib()
    C2 = 2 * S.C
    for k in range(len(S.parts)):
        inbox = _quarters(c, (c.G, C2, c.stride), 11 + k)
        dv = Step(c, S, g)
        s = dv.desc(k, "mir")
        src, out = T(inbox), torch.full((C2 + 1, c.stride), SENTINEL, device=DEV)
        s.em_coef, s.em_chunks, s.n_peers = dv.ent.data_ptr(), 1, c.G
        for o in range(c.G):
            s.peer_v[o] = s.peer_g[o] = src.data_ptr()
        _call(L.mke_oc_gv_sum, C.byref(s), _void(src), _void(out), _stream())
        torch.cuda.synchronize()
        want = np.full((C2 + 1, c.stride), SENTINEL, dtype=f64)
        rows = np.concatenate([np.arange(len(S.own_h[k][g])), S.C + np.arange(len(S.own_t[k][g]))]).astype(np.int64)
        want[rows] = inbox.astype(f64).sum(0)[rows]
        _report("gv_sum", cid, [("gv", N_(out), (want, None))])
        for field, val in (("n_peers", 0), ("em_coef", None)):
            s2 = dv.desc(k, "mir")
            s2.em_coef, s2.em_chunks, s2.n_peers = dv.ent.data_ptr(), 1, c.G
            for o in range(c.G):
                s2.peer_v[o] = s2.peer_g[o] = src.data_ptr()
            setattr(s2, field, val)
            out2 = torch.full((C2 + 1, c.stride), SENTINEL, device=DEV)
            assert L.mke_oc_gv_sum(C.byref(s2), _void(src), _void(out2), _stream()) == _abi.E_UNSUPPORTED
            torch.cuda.synchronize()
            assert (N_(out2) == SENTINEL).all()


# ---- 6. the second pass ---------------------------------------------------------------------------------------------------------------
class Plan:
    """mke_oc_em_plan of the case's one global step for rank g, on the device, checked against the enumeration of oc_cases.em_lists."""

    def __init__(self, c, S, g, own=None):
        codes = ((S.cent << 1) | S.cside)
        if c.N:
            codes[:, 0] |= S.need_hr * oc.NEED_HR + S.need_rt * oc.NEED_RT
        self.L = oc.em_lists(c, S, g)
        self.items, self.longs, self.n_part = oc.em_items(self.L[:, 0])
        capacity = len(self.L) + 17
        kw = dict(own=(own[0], own[1], own[0].numel() // 3)) if own is not None else {}
        out = OU.em_plan(S.ph, S.pr, S.pt, codes.ravel(), c.N, S.sh, S.st, np.array([0, c.n_pos]), c.G, g, c.n_local, c.n_rel, capacity,
                         chunks=len(S.parts), **kw)
        n = int(out["n_refs"][0])
        assert n == len(self.L) <= capacity
        refs = out["refs"].view(np.uint32).reshape(-1, 2)[:n].astype(np.int64)
        assert np.array_equal(refs[:, 0], self.L[:, 4]) and np.array_equal(refs[:, 1], self.L[:, 5]), "the plan's lists differ from the enumeration"
        self.n_items, self.n_long = int(out["steps3"][0][1]), int(out["steps3"][1][1])
        assert self.n_items == len(self.items) and self.n_long == len(self.longs) and int(out["steps3"][2][1]) == self.n_part
        self.t = {k: T(out[k]) for k in ("refs", "item_row", "item_off", "item_part", "long_row", "long_part0")}

    def fill(self, s, c, S, coef, vall, gvs, partials, mode=0):
        s.em_coef, s.em_pos0, s.em_chunks, s.em_block_floats = coef.data_ptr(), 0, len(S.parts), 2 * S.C * c.stride
        s.em_refs, s.em_rows, s.em_off, s.em_n_rows = self.t["refs"].data_ptr(), self.t["item_row"].data_ptr(), self.t["item_off"].data_ptr(), self.n_items
        s.em_part, s.em_long_rows, s.em_long_part0 = (self.t[k].data_ptr() for k in ("item_part", "long_row", "long_part0"))
        s.em_n_long, s.em_part0, s.em_partials, s.em_mode = self.n_long, 0, partials.data_ptr(), mode
        for k in range(len(S.parts)):
            s.em_v[k], s.em_gv[k] = vall[k].data_ptr(), gvs[k].data_ptr()


def _pass2(c, S, g, plan, coef, vall, gvs, modes, rel_start):
    dv = Step(c, S, g, em=True)
    dv.rel_grad.copy_(T(rel_start))
    partials = torch.full((plan.n_part + 1, c.stride + 16), SENTINEL, device=DEV)
    tc, tv, tg = T(coef), [T(v) for v in vall], [T(v) for v in gvs]
    for mode in modes:
        s = dv.desc(0, "em")
        plan.fill(s, c, S, tc, tv, tg, partials, mode)
        _call(_lib.lib().mke_oc_pass2, C.byref(s), _stream())
    torch.cuda.synchronize()
    return {"ent": N_(dv.ent), "acc": N_(dv.acc), "rel_grad": N_(dv.rel_grad), "partials": N_(partials)}


@pytest.mark.parametrize("cid", EM)
def test_pass2_on_quarters(cid):
    """Coefficients +-2^-k, vectors and gradient vectors multiples of 1/4: the stored relation partials (SENTINEL in the rows no list
    names) and the long rows' partial slots (g and the coefficient sum behind it) bit for bit; the entity rows and accumulators
    within the bound; em_mode 1 followed by 2 leaves the bits of em_mode 0; em_n_rows == 0 launches nothing."""
    c = CASES[cid]
    R, S, g = _ref(cid, 0), oc.stage(c), c.rank
    plan = Plan(c, S, g)
    coef, vall, gvs = oc.pass2_inputs(c)
    z = np.zeros
    rel_start = np.full((c.n_rel + 1, c.stride), SENTINEL, dtype=f32)
    want = R.pass2(g, (coef.astype(f64), z(coef.shape)), [(v.astype(f64), z(v.shape)) for v in vall], [(v.astype(f64), z(v.shape)) for v in gvs])
    a = _pass2(c, S, g, plan, coef, vall, gvs, (0,), rel_start)
    b = _pass2(c, S, g, plan, coef, vall, gvs, (1, 2), rel_start)
    for name in a:
        assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), (cid, name, "em_mode 1 + 2 differs from em_mode 0")
    _report("pass2", cid, [("ent", a["ent"], want["ent"]), ("acc", a["acc"], want["acc"]), ("rel_grad", a["rel_grad"], (want["rel_grad"][0], None)),
                           ("partials", a["partials"], want["partials"])])
    dv = Step(c, S, g, em=True)
    dv.rel_grad.copy_(T(rel_start))
    partials = torch.full((plan.n_part + 1, c.stride + 16), SENTINEL, device=DEV)
    s = dv.desc(0, "em")
    tc, tv, tg = T(coef), [T(v) for v in vall], [T(v) for v in gvs]
    plan.fill(s, c, S, tc, tv, tg, partials)
    s.em_n_rows = 0
    _call(_lib.lib().mke_oc_pass2, C.byref(s), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(N_(dv.ent), oc.local_rows(c, S.ent, g), equal_nan=True) and np.array_equal(N_(dv.acc), oc.local_rows(c, S.acc_e, g), equal_nan=True)
    assert (N_(dv.rel_grad) == SENTINEL).all() and (N_(partials) == SENTINEL).all()


# ---- 7. the whole step, every rank ------------------------------------------------------------------------------------------------------
def _rank_sum(blocks):
    """float32 sum in rank order: the reduce-scatter / all-reduce of the test."""
    out = blocks[0].clone()
    for b in blocks[1:]:
        out += b
    return out


def _whole_step(c, S, form, quarter):
    G, st, C2, K, L = c.G, c.stride, 2 * S.C, len(S.parts), _lib.lib()
    atm, peer, owned = form == "atm", form in ("mir", "mirown"), form in ("own", "mirown")
    dvs = [Step(c, S, g, em=not atm) for g in range(G)]
    for dv in dvs:                                     # an entity-major step is handed the counters too: it must leave them alone
        dv.desc = functools.partial(dv.desc, refcount=c.refcount if atm else True)
    coefs = [torch.full((c.n_pos * (c.N + 1) + 1,), SENTINEL, device=DEV) for _ in range(G)]
    owns = [_owned(c, S, g) if owned else None for g in range(G)]
    lossp = torch.full((K, G, _lib.LOSS_PARTIALS), float("nan"), dtype=torch.float64, device=DEV)
    valls, gvs = [], []
    for k in range(K):
        lo, _ = S.parts[k]
        send = torch.full((G, C2, st), SENTINEL, device=DEV)                      # the all-gather: the send blocks side by side
        for g in range(G):
            s = dvs[g].desc(k, form, quarter)
            phases = _abi.OC_BASES | (_abi.OC_COUNT if atm else 0)
            _call(L.mke_oc_run, C.byref(s), phases, C.c_void_p(send.data_ptr() + 4 * g * C2 * st), None, C.c_int64(0), None, None, None, _stream())
        inbox = torch.full((G, G, C2, st), SENTINEL, device=DEV)                  # [owner][writer]
        mirrors = [torch.full((G, C2, st), SENTINEL, device=DEV) for _ in range(G)] if peer else None
        for g in range(G):
            s = dvs[g].desc(k, form, quarter)
            if not atm:
                s.em_coef, s.em_pos0, s.em_chunks = coefs[g].data_ptr(), lo, K
            if owned:
                s.own_rec, s.own_off, s.codes = owns[g][0].data_ptr(), owns[g][1].data_ptr() + 4 * lo, None
            if peer:
                s.n_peers = G
                for o in range(G):
                    s.peer_v[o], s.peer_g[o] = send.data_ptr() + 4 * o * C2 * st, inbox.data_ptr() + 4 * (o * G + g) * C2 * st
                _call(L.mke_oc_score, C.byref(s), _void(mirrors[g]), C.c_int64(C2 * st), None, C.c_void_p(lossp[k, g].data_ptr()), _stream())
            else:
                g_all = torch.empty(G, C2, st, device=DEV)
                g_all.fill_(SENTINEL)
                _call(L.mke_oc_score, C.byref(s), _void(send), C.c_int64(C2 * st), _void(g_all), C.c_void_p(lossp[k, g].data_ptr()), _stream())
                inbox[:, g] = g_all
        torch.cuda.synchronize()
        if peer:
            for g in range(G):                                                    # the mirror IS the all-gathered buffer, bit for bit
                assert torch.equal(mirrors[g].view(torch.int32), send.view(torch.int32)), (form, g, "mirror")
        valls.append(mirrors if peer else [send] * G)
        if peer:                                                                  # the receiving rank sums its inbox: mke_oc_gv_sum
            blocks = []
            for g in range(G):
                s = dvs[g].desc(k, form, quarter)
                s.em_coef, s.em_chunks, s.n_peers = coefs[g].data_ptr(), K, G
                for o in range(G):
                    s.peer_v[o], s.peer_g[o] = send.data_ptr(), inbox.data_ptr()
                out = torch.full((C2, st), SENTINEL, device=DEV)
                _call(L.mke_oc_gv_sum, C.byref(s), _void(inbox[g]), _void(out), _stream())
                blocks.append(out)
            gvs.append(blocks)
        else:
            gvs.append([_rank_sum([inbox[g, w] for w in range(G)]) for g in range(G)])
    if atm:
        for g in range(G):
            s = dvs[g].desc(0, form, quarter)
            _call(L.mke_oc_apply, C.byref(s), _void(gvs[0][g]), _stream())
    else:
        for g in range(G):
            plan = Plan(c, S, g, owns[g])
            dvs[g].rel_grad.zero_()
            partials = torch.full((plan.n_part + 1, st + 16), SENTINEL, device=DEV)
            s = dvs[g].desc(0, form, quarter)
            plan.fill(s, c, S, coefs[g], [valls[k][g] for k in range(K)], [gvs[k][g] for k in range(K)], partials)
            _call(L.mke_oc_pass2, C.byref(s), _stream())
            dvs[g].keep.append((plan, partials))
    torch.cuda.synchronize()
    n = dvs[0].copies * c.n_rel
    total = _rank_sum([dvs[g].rel_grad[:n] for g in range(G)])                    # the all-reduce of the relation gradient
    for g in range(G):
        dvs[g].rel_grad[:n] = total
        s = dvs[g].desc(0, form, quarter)
        if not atm:
            s.em_coef, s.em_chunks = coefs[g].data_ptr(), K
        _call(L.mke_oc_run, C.byref(s), _abi.OC_UPDATE, None, None, C.c_int64(0), None, None, None, _stream())
    torch.cuda.synchronize()
    return dvs, N_(lossp)


@pytest.mark.parametrize("cid", SMALL)
def test_whole_step(cid):
    """Bases -> all-gather -> score -> reduce-scatter (or the peers' inbox and mke_oc_gv_sum) -> apply / second pass -> all-reduce ->
    update, for every rank, in every form of the case: every rank's rows and accumulators, the relation table and its accumulator
    and the loss within the bound of the chained reference; pad columns exactly 0 (0.1 in the accumulators); scratch, reference counts
    and the SENTINEL tails back at their invariant."""
    c = CASES[cid]
    S = oc.stage(c)
    live = np.arange(c.stride) < c.dim
    forms = sorted({(("atm" if r.form == "atm" else r.form), r.quarter) for r in RUNS_OF[cid]})
    if c.tag == "width":                                       # all five forms in one kernel each, alternating
        forms = [(f, (k + c.G) % 2) for k, f in enumerate(oc.FORMS)]
    for form, quarter in forms:
        if form == "atm" and len(S.parts) > 1:
            continue
        want = _ref(cid, quarter, False).step(form)
        dvs, lossp = _whole_step(c, S, form, quarter)
        assert np.isfinite(lossp).all()
        named = [("loss", lossp.sum(), want["loss"])]
        for g in range(c.G):
            ent, acc = N_(dvs[g].ent), N_(dvs[g].acc)
            named += [(f"ent{g}", ent, want["ent"][g]), (f"acc{g}", acc, want["acc"][g])]
            assert not ent[:-1, ~live].any() and (acc[:len(S.ent[g::c.G]), ~live] == oc.ACC_PAD).all(), (form, g, "pad columns")
            assert not N_(dvs[g].ent_grad)[:-1].any() and (N_(dvs[g].ent_grad)[-1] == SENTINEL).all(), (form, g, "scratch")
            assert not N_(dvs[g].rel_grad)[:-1].any() and not N_(dvs[g].rc)[:-1].any() and N_(dvs[g].rc)[-1] == 9, (form, g)
            named += [(f"touched_ent{g}", N_(dvs[g].te), want["touched_ent"][g]), (f"touched_rel{g}", N_(dvs[g].tr), want["touched_rel"][g])]
            named += [(f"rel{g}", N_(dvs[g].rel), want["rel"]), (f"rel_acc{g}", N_(dvs[g].rel_acc), want["rel_acc"])]
        ratios = _report(f"step/{form}-q{quarter}", cid, named)
        for what in ("ent", "acc", "rel", "loss"):
            vals = [v for k, v in ratios.items() if k.startswith(what) and not k.startswith("rel_acc" if what == "rel" else "\0")]
            if vals:
                print(f"RATIO step:worst:{what} {max(vals):.4f} {cid} {form}")


# ---- refusals: rejected before any launch -----------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    c = CASES[[cid for cid in SMALL if CASES[cid].tag == "width"][0]]
    S, g, L = oc.stage(c), c.rank, _lib.lib()
    dv = Step(c, S, g)
    C2 = 2 * S.C
    v = torch.zeros(c.G, C2, c.stride, device=DEV)
    g_all = torch.full((c.G * C2, c.stride), SENTINEL, device=DEV)
    lossp = torch.full((_lib.LOSS_PARTIALS,), float("nan"), dtype=torch.float64, device=DEV)
    own = _owned(c, S, g)

    def score(**over):
        s = dv.desc(0)
        for k, val in over.items():
            setattr(s, k, val)
        return L.mke_oc_score(C.byref(s), _void(v), C.c_int64(C2 * c.stride), _void(g_all), _void(lossp), _stream())

    assert score(own_off=own[1].data_ptr(), own_rec=own[0].data_ptr()) == _abi.E_UNSUPPORTED       # owned lists without em_coef
    assert score(n_peers=1 if c.G > 1 else 2) == _abi.E_SHAPE
    assert score(per=0) == _abi.E_SHAPE and score(neg_per_pos=65) == _abi.E_SHAPE and score(rel_grad_copies=65) == _abi.E_SHAPE
    assert score(codes=None) == _abi.E_NULL and score(optimizer=_lib.OPT_ADAM) == _abi.E_UNSUPPORTED
    s = dv.desc(0)
    assert L.mke_oc_pass2(C.byref(s), _stream()) == _abi.E_UNSUPPORTED                             # not entity-major
    torch.cuda.synchronize()
    assert (N_(g_all) == SENTINEL).all() and np.isnan(N_(lossp)).all() and not N_(dv.ent_grad)[:-1].any()
    assert np.array_equal(N_(dv.ent), oc.local_rows(c, S.ent, g), equal_nan=True)

"""Every client of the f32 MFMA similarity sweep (mke_simtile.h), at every instantiated width and at the tile / chunk / segment
edges, against the exact oracles of sweep_cases.py: integer operands make every dot product exact in any summation order, so
the assertions are equality of integers and of float32 bit patterns — no tolerance, no sampled rows, no share of rows.
Operands lie in NaN-poisoned buffers (ld > kpad, BN NaN rows behind the last row); every call is made twice and must
repeat itself bit for bit."""
import numpy as np
import pytest

import sweep_cases as sc

pytestmark = pytest.mark.gpu

ids = lambda c: c.id


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(x):
    """int32 view of a float32 array (numpy or torch): equality of these is equality of bit patterns."""
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return np.ascontiguousarray(x.detach().cpu().numpy()).view(np.int32)


def _same_bits(got, want):
    g = got.detach().cpu().numpy() if not isinstance(got, np.ndarray) else got
    assert g.dtype == np.float32 and g.shape == want.shape
    assert not np.isnan(g).any()
    assert np.array_equal(_bits(g), _bits(want))


def _operand_tensors(c):
    """(A rows view [rows, ld_a], B rows view [n_b, ld_b], whole A buffer, whole B buffer) on the device."""
    ops = sc.operands(c)
    a_buf, b_buf = sc.buffers(c)
    bd = _dev(b_buf)
    ad = bd if c.client in sc.SELF_CLIENTS else _dev(a_buf)
    return ad[:ops.A.shape[0]], bd[:ops.B.shape[0]], ad, bd


def _guarded(c, vec):
    """The vector on the device as the head of a longer tensor whose tail would win every comparison if it were read."""
    return _dev(sc.guarded(vec, sc.bn_for(c.kpad)))[:vec.shape[0]]


def _mode_args(c, ops):
    from multike_amd import _lib
    code = _lib.METRIC_EUCLIDEAN if c.euclidean else _lib.METRIC_INNER
    sq_a = _guarded(c, ops.sq_a) if c.euclidean else None
    sq_b = _guarded(c, ops.sq_b) if c.euclidean else None
    rt = _guarded(c, ops.rt) if c.csls else None
    rs = _guarded(c, ops.rs) if c.csls else None
    return code, sq_a, sq_b, rt, rs


def _decode_best(best):
    """(column, float32 bits of the best value) of the packed order-preserving keys."""
    b = best.cpu().numpy().view(np.uint64)
    col = (np.uint64(0xFFFFFFFF) - (b & np.uint64(0xFFFFFFFF))).astype(np.int64)
    u = (b >> np.uint64(32)).astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return col, bits.view(np.int32)


def _check_rank(c, rank, ties, best, S):
    greater, raw_ties, best_col, best_val = sc.rank_oracle(S)
    assert np.array_equal(rank.cpu().numpy(), greater)
    if ties is not None:
        t = ties.cpu().numpy()                          # the kernel's own counter, not the host's clamped value
        assert t.min() >= 1
        assert np.array_equal(t, raw_ties)
    col, bits = _decode_best(best)
    assert np.array_equal(col, best_col)
    assert np.array_equal(bits, _bits(best_val))


@pytest.mark.parametrize("c", sc.cases_of("rank"), ids=ids)
def test_align_rank(c):
    import torch
    from multike_amd import _lib
    _, _, ad, bd = _operand_tensors(c)                   # full-width tensors: ld = shape[1] > kpad, NaN rows behind n1 / n2
    S = sc.scores(c)
    outs = []
    for _ in range(2):
        rank = torch.zeros(c.n_a, dtype=torch.int32, device="cuda")
        ties = torch.zeros(c.n_a, dtype=torch.int32, device="cuda") if c.variant == "ties" else None
        best = torch.zeros(c.n_a, dtype=torch.int64, device="cuda")
        _lib.align_rank(ad, bd, c.kpad, c.n_a, c.n_b, rank, best, ties)
        _check_rank(c, rank, ties, best, S)
        outs.append((rank, best))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("c", sc.cases_of("rank_ex"), ids=ids)
def test_align_rank_ex(c):
    import torch
    from multike_amd import _lib
    ops = sc.operands(c)
    a, b, _, _ = _operand_tensors(c)
    code, sq1, sq2, rt, rs = _mode_args(c, ops)
    S = sc.scores(c)
    outs = []
    for _ in range(2):
        rank = torch.zeros(c.n_a, dtype=torch.int32, device="cuda")
        ties = torch.zeros(c.n_a, dtype=torch.int32, device="cuda")
        best = torch.zeros(c.n_a, dtype=torch.int64, device="cuda")
        _lib.align_rank_ex(a, b, c.kpad, rank, ties, best, code, sq1, sq2, rt, rs)
        _check_rank(c, rank, ties, best, S)
        outs.append((rank, ties, best))
    assert all(torch.equal(x, y) for x, y in zip(*outs))


@pytest.mark.parametrize("c", sc.cases_of("topk_mean"), ids=ids)
def test_align_topk_mean(c):
    import torch
    from multike_amd import _lib
    ops = sc.operands(c)
    a, b, _, _ = _operand_tensors(c)
    code, sq_a, sq_b, _, _ = _mode_args(c, ops)
    want = sc.topk_means(sc.scores(c), c.k)
    got = _lib.align_topk_mean(a, b, c.kpad, c.k, code, sq_a, sq_b)
    _same_bits(got, want)
    assert torch.equal(got, _lib.align_topk_mean(a, b, c.kpad, c.k, code, sq_a, sq_b))


def _check_select(c, cand, cnt, S, tau, seg_cap):
    want_cnt, stored = sc.select_oracle(S, tau, sc.chunk_bounds(c), seg_cap)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt)   # the true count even past seg_cap; empty segments report 0
    cidx = cand[..., 0].cpu().numpy()
    csim = cand[..., 1].cpu().numpy()                    # similarity bits
    for r in range(c.n_a):
        for s, cols in enumerate(stored[r]):
            assert np.array_equal(cidx[r, s, :len(cols)], cols)
            assert np.array_equal(csim[r, s, :len(cols)], _bits(S[r, cols]))


@pytest.mark.parametrize("c", sc.cases_of("sim_select"), ids=ids)
def test_sim_select(c):
    import torch
    from multike_amd import _lib
    _, e, _, _ = _operand_tensors(c)
    S = sc.scores(c)
    tau = sc.select_taus(c, S)
    cand, cnt = _lib.sim_select(e, c.kpad, c.row_lo, c.row_hi, _dev(tau), c.n_seg, c.seg_cap)
    _check_select(c, cand, cnt, S, tau, c.seg_cap)
    cand2, cnt2 = _lib.sim_select(e, c.kpad, c.row_lo, c.row_hi, _dev(tau), c.n_seg, c.seg_cap)
    assert torch.equal(cnt, cnt2)
    keep = (torch.arange(c.seg_cap, device="cuda")[None, None, :] < cnt[..., None])[..., None].expand_as(cand)
    assert torch.equal(torch.where(keep, cand, 0), torch.where(keep, cand2, 0))


@pytest.mark.parametrize("c", sc.cases_of("sim_sample"), ids=ids)
def test_sim_sample(c):
    import torch
    from multike_amd import _lib
    ops = sc.operands(c)
    e, samp, _, _ = _operand_tensors(c)
    assert e.stride(0) != samp.stride(0)                  # ld_samp != ld
    out = _lib.sim_sample(e, c.kpad, c.row_lo, c.row_hi, samp)
    _same_bits(out, sc.scores(c))
    assert torch.equal(out, _lib.sim_sample(e, c.kpad, c.row_lo, c.row_hi, samp))
    # the same pairs through the main pass: sample rows that ARE rows of the matrix, everything selected in one segment
    n = ops.A.shape[0]
    cols = np.random.default_rng([n, c.n_b]).integers(0, n, min(c.n_b, 300))
    gathered = e[_dev(cols)].contiguous()                 # keeps the poisoned pad columns
    out2 = _lib.sim_sample(e, c.kpad, c.row_lo, c.row_hi, gathered)
    rows = slice(c.row_lo, c.row_hi)
    _same_bits(out2, sc.int_dots(ops.A[rows], ops.A[cols]).astype(np.float32))
    tau = torch.full((c.n_a,), sc.TAU_ALL, device="cuda")
    cand, cnt = _lib.sim_select(e, c.kpad, c.row_lo, c.row_hi, tau, 1, n)
    assert int(cnt.min()) == n == int(cnt.max())
    assert torch.equal(cand[:, 0, :, 0].cpu(), torch.arange(n, dtype=torch.int32).expand(c.n_a, n))
    sims = cand[:, 0, :, 1].contiguous().view(torch.float32)
    assert torch.equal(sims[:, _dev(cols)], out2)
    _same_bits(sims, sc.int_dots(ops.A[rows], ops.A).astype(np.float32))


@pytest.mark.parametrize("c", sc.cases_of("knn"), ids=ids)
def test_knn_chain(c):
    """sim_sample -> topk_rows (the threshold) -> sim_select -> topk_candidates, topk_long for the rows reported short or
    overflowed: the final table is the exact top-k set, ties by column order, for EVERY row."""
    import torch
    from multike_amd import _lib
    from multike_amd.base.batch import neighbour_table
    ops = sc.operands(c)
    _, e, _, _ = _operand_tensors(c)
    S = sc.scores(c)
    samp, m = sc.knn_plan(c)
    es = e[_dev(samp)].contiguous()
    ss = _lib.sim_sample(e, c.kpad, c.row_lo, c.row_hi, es)
    _same_bits(ss, S[:, samp])
    _, kth, st0 = _lib.topk_rows(ss, m, want_idx=False, want_kth=True)
    tau = sc.kth_largest(S[:, samp], m)
    assert int(st0.abs().sum()) == 0
    _same_bits(kth, tau)
    cand, cnt = _lib.sim_select(e, c.kpad, c.row_lo, c.row_hi, kth, c.n_seg, c.seg_cap)
    _check_select(c, cand, cnt, S, tau, c.seg_cap)
    table, status = _lib.topk_candidates(cand, cnt, c.k)
    want_status = sc.knn_status_oracle(c, S, tau)
    assert np.array_equal(status.cpu().numpy(), want_status)
    bad = torch.nonzero(status).reshape(-1)
    if bad.numel():
        src = e[bad + c.row_lo].contiguous()
        whole = _lib.sim_sample(src, c.kpad, 0, int(src.shape[0]), e)
        _same_bits(whole, S[bad.cpu().numpy()])
        table[bad] = _lib.topk_long(whole, c.k)
    want = sc.topk_sets(S, c.k)
    assert np.array_equal(table.cpu().numpy(), want)
    if c.n_b <= 1100:       # the product's own driver takes unnormalised rows as they are: whole rows at this size
        full = sc.int_dots(ops.B, ops.B).astype(np.float32)
        t2, valid = neighbour_table(_dev(ops.B), np.arange(c.n_b), c.k, c.n_b)
        assert int(valid.min()) == 1
        assert np.array_equal(t2.cpu().numpy(), sc.topk_sets(full, c.k))
        assert np.array_equal(t2[c.row_lo:c.row_hi].cpu().numpy(), want)


@pytest.mark.parametrize("c", sc.cases_of("stable"), ids=ids)
def test_stable_lists(c):
    """Every row ends up checked: rows the sweep flags are redone whole-row by base.alignment.candidate_lists, and which rows
    those are is itself held to the oracle."""
    import torch
    from multike_amd import _lib
    from multike_amd.base.alignment import candidate_lists
    ops = sc.operands(c)
    a, b, _, _ = _operand_tensors(c)
    code, sq_a, sq_b, rt, rs = _mode_args(c, ops)
    csls = (rt, rs) if c.csls else None
    S = sc.scores(c)

    def run():
        if c.variant == "simmat":
            return candidate_lists(None, None, 0, c.k, sim_mat=sim_dev)
        if c.variant == "whole" or c.k > 128:
            val, col, flags = _lib.stable_lists(a, b, c.kpad, c.k, code, sq_a, sq_b, rt, rs, whole_rows=c.variant == "whole")
            return val, col, int(flags.sum())
        return candidate_lists(a, b, c.kpad, c.k, code, sq_a, sq_b, csls, sample_cols=sc.sample_cols_of(c))

    if c.variant == "simmat":                              # the caller's matrix, with NaN entries: short lists end in (-inf, -1)
        S = S.copy()
        S[1, ::2] = np.nan
        S[3, : c.n_b - 5] = np.nan
        S[4, :] = np.nan
        wide = np.full((c.n_a, c.n_b + 3), np.nan, dtype=np.float32)
        wide[:, :c.n_b] = S
        sim_dev = _dev(wide)[:, :c.n_b]                     # ld_sim > n_b
        want_redone = 0
    elif c.variant == "whole" or c.k > 128:
        want_redone = 0
    else:
        sample_cols = sc.sample_cols_of(c)
        want_redone = int(sc.stable_flags_oracle(c, S, sample_cols).sum())
        if c.n_b <= 1024 and not sample_cols:
            assert want_redone == 0                         # the unthresholded sweep has room for every column
    want_val, want_col = sc.stable_lists_oracle(S, c.k)
    val, col, redone = run()
    assert redone == want_redone
    assert np.array_equal(col.cpu().numpy(), want_col)
    v = val.cpu().numpy()
    assert not np.isnan(v).any() and np.array_equal(_bits(v), _bits(want_val))
    val2, col2, _ = run()
    assert torch.equal(col, col2) and torch.equal(val.view(torch.int32), val2.view(torch.int32))

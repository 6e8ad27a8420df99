"""Owner-bucketed negative codes (`codes="owner"`, include/multike_hip.h section 13b) on the GPU: the bucket launch and the owned
index against a NumPy enumeration of their definition, the entity-major plan from the owned list against the plan from the
all-gathered codes (every output, bit for bit) and against the direct enumeration, the score launch on owned lists against its code
scan (coefficients, gradient-vector slots and loss partials, bit for bit), and the trainers of the two forms against each other on
1, 2, 3 and 8 ranks sharing the one GPU (collectives staged through gloo; world 1 also over a real one-rank RCCL communicator).
No multi-GPU link is exercised anywhere here: beyond one rank the collectives run host-staged only."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oc_owned_util as U
import ranks
from multike_amd import _lib

pytestmark = pytest.mark.gpu


# ---- 1. the bucket launch ---------------------------------------------------------------------------------------------------
def _codes_for(seed, G, N, n_mine, one_owner=False):
    """A share of codes as mke_oc_pack_codes writes it: (entity << 1) | side, the need flags in every group's first code."""
    rng = np.random.default_rng(seed)
    ent = rng.integers(0, 5000, n_mine * N)
    if one_owner:
        ent = ent // G * G + (G - 1)                 # every corrupt entity belongs to the last rank
    codes = (ent << 1) | rng.integers(0, 2, n_mine * N)
    if N:
        codes[::N] |= rng.integers(1, 4, n_mine) << 30
    return codes


@pytest.mark.parametrize("G,N,n_mine", [(1, 3, 21), (2, 1, 50), (3, 25, 64), (5, 8, 1), (8, 64, 130), (8, 25, 0)])
def test_buckets_equal_the_enumeration(G, N, n_mine):
    """Records, their (position, n) order inside each destination, the true counts and the positions' need flags; (3, 25, 64)
    sends everything to one owner.  A capacity of the whole share: nothing is cut."""
    pos0 = 1000 + 7 * G
    codes = _codes_for(G * 100 + N, G, N, n_mine, one_owner=(G == 3))
    cap = max(1, n_mine * N)
    need, send, counts, guard = U.bucket(codes, n_mine, N, pos0, G, cap, sentinel=-99)
    want_need, want = U.np_bucket(codes, n_mine, N, pos0, G)
    np.testing.assert_array_equal(need, want_need)
    np.testing.assert_array_equal(counts, [len(w) for w in want])
    for d in range(G):
        np.testing.assert_array_equal(send[d, :len(want[d])], want[d])
        assert (send[d, len(want[d]):] == -99).all()
    assert (guard == -99).all()
    if G == 3:
        assert counts.tolist() == [0, 0, n_mine * N]


def test_buckets_of_a_share_of_more_than_a_thousand_wavefront_ranges():
    """9,000 positions x 64 negatives: 1,125 wavefront ranges, so the per-owner prefix sums more than one count per thread (the
    shapes of a real epoch: 5,600 ranges per rank at 8 ranks of the C2 shape), and a capacity a quarter above the even share."""
    G, N, n_mine, pos0 = 8, 64, 9000, 123456
    assert 1024 < (n_mine * N + 511) // 512 <= _lib.OC_BUCKET_WAVES
    codes = _codes_for(77, G, N, n_mine)
    cap = n_mine * N // G * 5 // 4
    need, send, counts, guard = U.bucket(codes, n_mine, N, pos0, G, cap, sentinel=-99)
    want_need, want = U.np_bucket(codes, n_mine, N, pos0, G)
    np.testing.assert_array_equal(need, want_need)
    np.testing.assert_array_equal(counts, [len(w) for w in want])
    for d in range(G):
        assert len(want[d]) <= cap
        np.testing.assert_array_equal(send[d, :len(want[d])], want[d])
        assert (send[d, len(want[d]):] == -99).all()
    assert (guard == -99).all()


def test_bucket_overflow_keeps_the_true_counts_and_stays_inside_the_capacity():
    """cap = 12 with ~60 records for one destination: the counts are the true ones, the first 12 records of every destination are
    stored, and what lies behind a destination's 12 slots — the next destination's records, the guard behind the last — is what
    it would be without the overflow."""
    G, N, n_mine, cap = 4, 5, 20, 12
    rng = np.random.default_rng(3)
    ent = rng.integers(0, 4000, n_mine * N)
    ent[:60] = ent[:60] // G * G + 1                  # 60 of the 100 negatives belong to rank 1
    codes = (ent << 1) | rng.integers(0, 2, n_mine * N)
    codes[::N] |= 1 << 30
    need, send, counts, guard = U.bucket(codes, n_mine, N, 0, G, cap, sentinel=-99)
    _, want = U.np_bucket(codes, n_mine, N, 0, G)
    np.testing.assert_array_equal(counts, [len(w) for w in want])
    assert counts[1] >= 60 and counts.max() > cap
    for d in range(G):
        k = min(cap, len(want[d]))
        np.testing.assert_array_equal(send[d, :k], want[d][:k])
        assert (send[d, k:] == -99).all()
    assert (guard == -99).all()


# ---- 2. the owned index -----------------------------------------------------------------------------------------------------
def test_owned_index_with_empty_positions_and_an_empty_source():
    """Positions 0, 1 and the last four own nothing, positions 10 .. 19 are a run without an owned negative — the whole range of
    source 1 of 4, which sent nothing — and one source's count exceeds the capacity (clamped): the packed list and own_off equal
    the enumeration."""
    G, cap, n_all = 4, 16, 40
    per = n_all // G
    recs = {0: [(2, 0, 10), (2, 3, 12), (5, 1, 14), (9, 0, 16)], 1: [], 2: [(20, 2, 18), (20, 4, 20), (21, 0, 22)],
            3: [(30 + k // 3, k % 3, 24 + 2 * k) for k in range(16)]}
    assert all(g * per <= p < (g + 1) * per for g, v in recs.items() for p, _, _ in v) and recs[3][-1][0] < n_all - 2
    recv = np.full((G, cap, 3), -5, dtype=np.int32)
    for g, v in recs.items():
        recv[g, :len(v)] = np.asarray(v, dtype=np.int32).reshape(-1, 3)
    counts = [len(recs[0]), 0, len(recs[2]), 23]                       # source 3 had 23 for this rank: 16 arrived
    own_rec, own_off, n_owned = U.owned_index(recv, counts, G, cap, n_all)
    flat = [r for g in range(G) for r in recs[g]]
    assert n_owned == len(flat)
    np.testing.assert_array_equal(own_rec.cpu().numpy()[:3 * n_owned].reshape(-1, 3), flat)
    np.testing.assert_array_equal(own_off.cpu().numpy(), np.searchsorted([p for p, _, _ in flat], np.arange(n_all + 1)))
    assert (own_rec.cpu().numpy()[3 * n_owned:] == -1).all()


# ---- 3. the entity-major plan from the owned list -------------------------------------------------------------------------------
@pytest.mark.parametrize("keys64", [0, 1])
@pytest.mark.parametrize("G,rank,sizes,N,hub", [(1, 0, [7, 5, 9], 3, False), (4, 2, [40, 0, 33, 1], 5, False), (3, 1, [64, 64], 25, False),
                                                  (8, 7, [30] * 5, 8, True), (2, 0, [50, 50, 50], 0, False), (5, 4, [1, 1, 1], 1, False)])
def test_plan_from_the_owned_list_is_the_plan_from_all_codes(G, rank, sizes, N, hub, keys64):
    """The six epochs of tests/test_oc_em_plan_gpu.py::test_lists_equal_the_direct_enumeration, bucketed per home rank on the device,
    indexed, planned from the owned list: every output equals the plan from the all-gathered codes bit for bit, and both equal the
    direct enumeration.  N = 0: empty buckets.  keys64: the 64-bit sort keys."""
    n_ent, n_rel = 97, 6
    n_local = (n_ent + G - 1) // G
    ph, pr, pt, codes, sh, st, step_lo = U.case(G * 100 + rank, G, rank, n_ent, n_rel, sizes, N, hub)
    n_all = len(ph)
    want = U.expected(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, n_local)
    capacity = sum(len(v) for v in want.values()) + 17
    cap = -(-n_all // G) * N                                           # a home rank's whole share: no overflow
    recv, counts, need_all = U.exchange(codes, n_all, N, G, rank, cap)
    if N:
        np.testing.assert_array_equal(need_all, (codes[::N] & U.NEED).astype(np.uint32))
    own_rec, own_off, n_owned = U.owned_index(recv, counts, G, cap, n_all)
    rec_want, off_want = U.np_owned(codes, n_all, N, G, rank)
    assert n_owned == len(rec_want)
    np.testing.assert_array_equal(own_rec.cpu().numpy()[:3 * n_owned].reshape(-1, 3), rec_want)
    np.testing.assert_array_equal(own_off.cpu().numpy(), off_want)
    old = _lib.get_option("oc_em_keys64")
    _lib.set_option("oc_em_keys64", keys64)
    try:
        a = U.em_plan(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, n_local, n_rel, capacity)
        b = U.em_plan(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, n_local, n_rel, capacity, own=(own_rec, own_off, G * cap))
    finally:
        _lib.set_option("oc_em_keys64", old)
    va, vb = U.plan_valid(a), U.plan_valid(b)
    for k in va:
        np.testing.assert_array_equal(va[k], vb[k], err_msg=k)
    U.check_plan(a, want, len(sizes))
    U.check_plan(b, want, len(sizes))


def test_plan_from_the_owned_list_keeps_the_overflow_contract():
    """A reference capacity of a third of the references: MKE_OK and the true count in n_refs, as from the all-gathered codes."""
    G, rank, N = 2, 1, 9
    ph, pr, pt, codes, sh, st, step_lo = U.case(5, G, rank, 97, 6, [60, 60], N)
    want = U.expected(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, 49)
    n_refs = sum(len(v) for v in want.values())
    cap = 60 * N
    recv, counts, _ = U.exchange(codes, 120, N, G, rank, cap)
    own_rec, own_off, _ = U.owned_index(recv, counts, G, cap, 120)
    out = U.em_plan(ph, pr, pt, codes, N, sh, st, step_lo, G, rank, 49, 6, n_refs // 3, own=(own_rec, own_off, G * cap))
    assert int(out["n_refs"][0]) == n_refs


# ---- 4. the score launch on owned lists ---------------------------------------------------------------------------------------
def _score_inputs(G, r, N, n_pos, chunks, seed):
    """One global step of n_pos positives as rank r of G: positives, codes with flags, per-part slots; positive 0 has all its
    negatives owned by r, positive 1 none (G > 1), positive 2 corrupts both sides (needs both vectors)."""
    n_ent, n_rel = 97, 6
    ph, pr, pt, codes, _, _, _ = U.case(seed, G, r, n_ent, n_rel, [n_pos], N)
    codes = codes & U.MASK
    ent, side = codes >> 1, codes & 1
    ent[:N] = ent[:N] // G * G % (n_ent // G * G) + r
    if G > 1:
        ent[N:2 * N] = ent[N:2 * N] // G * G % (n_ent // G * G) + (r + 1) % G
    side[2 * N:3 * N] = np.arange(N) % 2
    codes = (ent << 1) | side
    need_rt = np.array([bool((codes[p * N:(p + 1) * N] & 1).any()) for p in range(n_pos)])
    need_hr = ~need_rt | np.array([bool(((codes[p * N:(p + 1) * N] & 1) == 0).any()) for p in range(n_pos)])
    size = -(-n_pos // chunks)
    parts = [(a, min(n_pos, a + size)) for a in range(0, n_pos, size)]
    sh, st = np.full(n_pos, -1), np.full(n_pos, -1)
    for lo, hi in parts:
        ch, ct = np.zeros(G, int), np.zeros(G, int)
        for p in range(lo, hi):
            if need_hr[p]:
                sh[p] = ch[ph[p] % G]; ch[ph[p] % G] += 1
            if need_rt[p]:
                st[p] = ct[pt[p] % G]; ct[pt[p] % G] += 1
    codes[::N] |= need_hr.astype(np.int64) * 0x40000000 + need_rt.astype(np.int64) * 0x80000000
    owned = [int(((((codes[p * N:(p + 1) * N] & U.MASK) >> 1) % G) == r).sum()) for p in range(3)]
    assert owned[0] == N and (G == 1 or owned[1] == 0) and sh[2] >= 0 and st[2] >= 0
    return ph, pr, pt, codes, sh, st, parts, n_ent, n_rel


@pytest.mark.parametrize("dim", [75, 250])
@pytest.mark.parametrize("G,r", [(1, 0), (2, 1), (3, 1), (8, 7)])
def test_score_on_owned_lists_is_the_code_scan_bit_for_bit(G, r, dim):
    """One staged global step (the all-gathered vectors are random numbers) as rank r of G, N in {3, 25, 64}, the wavefront and the
    quarter-wave kernel, one and two parts: em_coef, the gradient-vector slots (g_all) and the loss partials of the launch on owned
    lists equal those of the code scan bit for bit — every slot, also of positives without an owned negative (the buffers start
    from the same sentinel in both runs, so a slot one form wrote and the other did not shows)."""
    L = _lib.lib()
    dev = "cuda"
    stride = _lib.stride_for(dim)
    n_pos = 70
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for N in (3, 25, 64):
        for chunks in (1, 2):
            ph, pr, pt, codes, sh, st, parts, n_ent, n_rel = _score_inputs(G, r, N, n_pos, chunks, 1000 * G + 10 * N + chunks)
            n_local = (n_ent + G - 1) // G
            gen = torch.Generator(device="cpu").manual_seed(G * 7 + N)
            rnd = lambda *shape: (torch.rand(*shape, generator=gen) - 0.5).to(dev)
            ent, rel = rnd(n_local, stride), rnd(n_rel, stride)
            Cc = n_pos
            v_all = [rnd(G * 2 * Cc * stride) for _ in parts]
            cap = -(-n_pos // G) * N
            recv, counts, _ = U.exchange(codes, n_pos, N, G, r, cap)
            own_rec, own_off, n_owned = U.owned_index(recv, counts, G, cap, n_pos)
            assert n_owned == len(U.np_owned(codes, n_pos, N, G, r)[0])
            i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)
            t = dict(ph=i32(ph), pr=i32(pr), pt=i32(pt), sh=i32(sh), st=i32(st), codes=U.dev32(codes))
            rel_grad, rel_touched = torch.zeros(n_rel, stride, device=dev), torch.zeros(n_rel, dtype=torch.int32, device=dev)
            for quarter in (0, 1):
                tun = _lib.tuning(oc_score_quarter=quarter)
                results = []
                for owned in (False, True):
                    coef = torch.full((n_pos * (N + 1),), 7.5, device=dev)
                    outs = []
                    for c, (lo, hi) in enumerate(parts):
                        g_all = torch.full((G * 2 * Cc * stride,), 7.5, device=dev)
                        lossp = torch.full((_lib.LOSS_PARTIALS,), -1.0, dtype=torch.float64, device=dev)
                        s = _lib.OcStepStruct()
                        s.ent, s.rel, s.rel_grad, s.rel_touched = ent.data_ptr(), rel.data_ptr(), rel_grad.data_ptr(), rel_touched.data_ptr()
                        s.n_local, s.n_rel, s.rel_grad_copies = n_local, n_rel, 1
                        s.stride, s.dim, s.rank, s.n_ranks = stride, dim, r, G
                        s.pos_h, s.pos_r, s.pos_t = (t[k].data_ptr() + 4 * lo for k in ("ph", "pr", "pt"))
                        s.slot_h, s.slot_t = t["sh"].data_ptr() + 4 * lo, t["st"].data_ptr() + 4 * lo
                        s.n_pos, s.per = hi - lo, max(1, -(-(hi - lo) // G))
                        s.neg_per_pos, s.capacity = N, Cc
                        s.optimizer, s.lr, s.scale, s.tag = _lib.OPT_ADAGRAD, 0.01, 1.0, 1
                        s.em_coef, s.em_pos0, s.em_chunks = coef.data_ptr(), lo, len(parts)
                        s.tuning = _lib.tuning_ptr(tun)
                        if owned:
                            s.own_rec, s.own_off = own_rec.data_ptr(), own_off.data_ptr() + 4 * lo      # codes stay NULL
                        else:
                            s.codes = t["codes"].data_ptr()
                            for g in range(G):
                                s.code_off[g] = (lo + g * int(s.per)) * N
                        rc = L.mke_oc_score(C.byref(s), C.c_void_p(v_all[c].data_ptr()), C.c_int64(2 * Cc * stride), C.c_void_p(g_all.data_ptr()),
                                            C.c_void_p(lossp.data_ptr()), stream)
                        assert rc == 0, L.mke_last_error()
                        outs += [g_all, lossp]
                    torch.cuda.synchronize()
                    results.append([coef] + outs)
                for a, b in zip(*results):
                    bits = torch.int64 if a.dtype == torch.float64 else torch.int32
                    assert torch.equal(a.view(bits), b.view(bits)), (N, chunks, quarter)
                assert int((results[0][0] != 7.5).sum()) >= N          # the launches wrote coefficients (positive 0 alone has N)


# ---- 5. the trainers ------------------------------------------------------------------------------------------------------------
CONFIGS = [dict(native=True, zipf=0.0), dict(native=False, zipf=0.0), dict(native=True, zipf=1.0), dict(native=False, zipf=1.0)]


def _run_pair(rank, world, comm, kw, native, kgs=None):
    """The same epochs by a codes="gather" and a codes="owner" trainer; -> (list of mismatching state names, owner trainer's check())."""
    state, info = [], None
    for form in ("gather", "owner"):
        tr = U.make_trainer(rank, world, comm=comm, codes=form, entity_major=True, kgs=kgs, **kw)
        n = 2 * tr.steps + 1                        # two epochs and the first step of the third: two boundaries, plans prefetched
        if native:
            assert tr._native_loop()[0]
            tr.run(0, n)
        else:
            for i in range(n):
                tr.step(i)
        torch.cuda.synchronize()
        assert tr.check()["codes"] == form and (tr._own_off is not None) == (form == "owner" and tr.N > 0)
        state.append(dict(ent=tr.ent.clone(), ent_acc=tr.ent_acc.clone(), rel=tr.rel.clone(), loss_ring=tr.loss_ring.clone(),
                          epoch_loss=torch.tensor(tr.epoch_loss(), dtype=torch.float64)))
        info = tr.check()
    bad = [k for k in state[0] if not torch.equal(state[0][k].view(torch.int64 if state[0][k].dtype == torch.float64 else torch.int32).cpu(),
                                                  state[1][k].view(torch.int64 if state[1][k].dtype == torch.float64 else torch.int32).cpu())]
    return bad, info


def _trainer_worker(rank, world, what):
    """One rank (sharing the GPU with the others) with the whole job of `what`; "rccl": in a one-rank RCCL group."""
    os.environ.pop("MKE_OC_CODES", None)
    rccl = what == "rccl"
    if world == 1:
        os.environ["MKE_OC_FORCE_COLLECTIVES"] = "1"
    from multike_amd.distributed_oc import OcHostStagedComm
    torch.cuda.set_device(0)
    comm = None if rccl else OcHostStagedComm()
    out = []
    if what == "peer":
        # the peer-direct transport of the entity-major form (IPC-mapped send blocks and inboxes, Python step loop, one part):
        # the mirror instantiations of the score kernels on owned lists
        for zipf in (0.0, 1.0):
            kw = dict(n_ent=600, dim=75, neg=8, b=max(1, 700 // world), zipf=zipf, peer_direct=True)
            out.append(_run_pair(rank, world, comm, kw, False))
    elif what == "overflow":
        # nine tenths of the corrupt entities belong to rank 0: the pair capacity 1.06 n_per N / 2 + 4096 does not hold them
        kw = dict(n_ent=400, dim=20, neg=25, b=700)
        bad, info = _run_pair(rank, world, comm, kw, True, kgs=U.SkewKGs())
        out.append((bad, info))
    else:
        for cfg in (CONFIGS[:1] if rccl else CONFIGS):
            kw = dict(n_ent=600, dim=75, neg=8, b=max(1, 700 // world), zipf=cfg["zipf"], chunks=2 if cfg["zipf"] else 1)
            bad, info = _run_pair(rank, world, comm, kw, cfg["native"])
            out.append((bad, info))
    return out


@pytest.mark.timeout(420)
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_owner_trainer_is_the_gather_trainer_bit_for_bit(world):
    """Two epochs and a step, plans prefetched, native step loop and Python loop, uniform triples (one part per step) and Zipf(1.0)
    triples (hub entities: long rows; two parts per step): entity shard, Adagrad slot, relation table, the loss ring and the epoch
    loss are bit-identical between the two forms on every rank.  World 1 forces the collectives (host-staged)."""
    got = ranks.run_ranks(world, _trainer_worker, ("staged",), limit=360)
    for rank, out in got.items():
        assert len(out) == len(CONFIGS)
        for cfg, (bad, info) in zip(CONFIGS, out):
            assert not bad, (rank, cfg, bad)
            assert info["codes"] == "owner" and info["owner_replans"] == 0 and info["entity_major"]
            assert info["communicator"] == "OcHostStagedComm" and info["native_step_loop"]
            assert info["code_bytes_received_per_epoch"] > 0          # (reported; at these sizes the 4,096 records of slack dominate)


@pytest.mark.timeout(300)
def test_owner_trainer_over_a_one_rank_rccl_communicator():
    """World 1 with the collectives forced over the real one-rank RCCL communicator (the flags' and counts' all-gathers and the
    all-to-all issued for real, at the plan's fixed point of the step sequence, native step loop): bit-identical to `gather`."""
    got = ranks.run_ranks(1, _trainer_worker, ("rccl",), limit=240, backend="nccl")
    (bad, info), = got[0]
    assert not bad, bad
    assert info["communicator"] == "OcRcclComm" and info["codes"] == "owner" and info["native_step_loop"]


@pytest.mark.timeout(300)
def test_owner_trainer_on_the_peer_direct_transport():
    """Two ranks, `peer_direct=True, entity_major=True`: the score launch reads the owners' send blocks, mirrors them and writes
    the owners' inboxes — on owned lists (the same kernels with both flags): bit-identical to `gather` on that transport."""
    got = ranks.run_ranks(2, _trainer_worker, ("peer",), limit=240)
    for rank, out in got.items():
        assert len(out) == 2
        for bad, info in out:
            assert not bad, (rank, bad)
            assert info["codes"] == "owner" and info["peer_direct"] and info["entity_major"]


# ---- 6. overflow regrow ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_owner_plan_is_redone_once_when_a_pair_overflows():
    """Two ranks, a KG pair whose corrupt entities are nine tenths rank 0's: the default pair capacity overflows in the first plan,
    every rank sees it in the same counts table and buckets, exchanges and plans again, in line, at the exact maximum (kept for
    the epochs that follow) — and the result is `gather`'s bit for bit."""
    got = ranks.run_ranks(2, _trainer_worker, ("overflow",), limit=240)
    for rank, out in got.items():
        (bad, info), = out
        assert not bad, (rank, bad)
        assert info["owner_replans"] >= 1, info
        assert info["owner_code_capacity_per_pair"] > int(1.06 * 1500 * 25 / 2) + 4096


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_owner_codes_with_the_atomics_form_are_refused():
    with pytest.raises(_lib.MultiKEHipError, match="owner.*entity-major|entity-major.*owner"):
        U.make_trainer(0, 1, codes="owner", entity_major=False)
    with pytest.raises(_lib.MultiKEHipError, match="gather.*owner"):
        U.make_trainer(0, 1, codes="mine")
    # the native side: own_off on a step without em_coef
    tr = U.make_trainer(0, 1, codes="gather", entity_major=False)
    tr.step(0)
    torch.cuda.synchronize()
    s = tr.backend._steps[0]
    assert not s.em_coef
    off = torch.zeros(int(s.n_pos) + 1, dtype=torch.int32, device="cuda")
    s.own_off, s.own_rec = off.data_ptr(), off.data_ptr()
    a = tr._addr[0]
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mke_oc_score(C.byref(s), C.c_void_p(a[1]), C.c_int64(tr.block), C.c_void_p(a[2]), C.c_void_p(tr.loss_ring.data_ptr()), stream)
    assert rc == -3 and b"own_off" in L.mke_last_error()
    s.own_off = s.own_rec = None

"""Owner-bucketed negative codes (`codes="owner"`) under gloo on the CPU, worlds 2 and 3, with the oracle as the compute backend: the
host side of the plan — this rank's share bucketed by owner (the torch implementation of the bucket launch), the flags' and counts'
all-gathers and the equal-split all-to-all on the step communicator, the owned index, the overflow decision every rank takes from
the same counts table — gives each rank exactly the codes it owns of the `gather` plan's all-gathered codes, in (position, n)
order, and the same slots.

The oracle backend has the atomics form only (no entity-major plan), and `owner` is refused with it at construction — checked
here too — so no epoch is trained on this backend: the PLAN equality is what this file checks; the entity-major epochs of the two
forms are compared bit for bit on the GPU (tests/test_oc_owned_codes_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import ranks

N_REL, DIM, B, NEG, SEED = 12, 20, 64, 5, 7


def _worker(rank, world, n_ent, small_cap):
    os.environ.pop("MKE_OC_CODES", None)
    from oracle import multike_oracle as mo
    from multike_amd import _lib
    from multike_amd.distributed_oc import OwnerComputesTrainer
    from multike_amd.synthetic import SyntheticKGs
    from oracle_backend import OcOracleBackend
    import oc_owned_util as U
    kgs = SyntheticKGs(n_ent=n_ent, n_rel=N_REL, seed=SEED)
    rng = np.random.default_rng(SEED)
    ent0 = mo.xavier_truncated_normal((n_ent, DIM), rng).astype(np.float64)
    rel0 = mo.xavier_truncated_normal((N_REL, DIM), rng).astype(np.float64)
    mk = lambda **kw: OwnerComputesTrainer(kgs, ent0, rel0, B, NEG, rank, world, seed=SEED, lr=0.05, backend=OcOracleBackend(),
                                           device="cpu", dtype=torch.float64, **kw)
    refused = False
    try:
        mk(codes="owner")
    except _lib.MultiKEHipError as e:
        refused = "entity-major" in str(e) and "owner" in str(e)
    tr = mk()
    assert not tr.em and tr.check()["codes"] == "gather" and tr.check()["code_bytes_received_per_epoch"] == 4 * world * -(-tr._n_all // world) * NEG
    b = tr.bat
    pos, n_all, G = (b.pos_h, b.pos_r, b.pos_t), tr._n_all, world
    g = tr._compute_plan(pos, b.rng_stream, 1)                    # the all-gathered codes, in the spare buffer set
    codes = g.codes[:n_all * NEG].numpy().astype(np.int64) & 0xFFFFFFFF
    slots = [s[:n_all].clone() for s in g.slot]
    owns = [o[:n_all].clone() for o in g.own]
    cnt = g.cnt_host.clone()
    # the owner plan of the same epoch order by the same trainer (construction would refuse the form with this backend)
    tr.codes_form = "owner"
    if small_cap:
        tr._own_cap = 9                                           # every pair overflows: bucket + exchange + plan are redone
    o = tr._compute_plan(pos, b.rng_stream, 1)
    n_per = -(-n_all // G)
    table = o.cnt_all.view(G, G).numpy().copy()
    want_table = np.zeros((G, G), dtype=np.int64)
    for src in range(G):
        lo, hi = min(n_all, src * n_per), min(n_all, (src + 1) * n_per)
        _, per_dest = U.np_bucket(codes[lo * NEG:hi * NEG], hi - lo, NEG, lo, G)
        want_table[src] = [len(x) for x in per_dest]
    assert (table == want_table).all(), (table, want_table)
    if small_cap:
        assert table.max() > o.own_cap == 9
    tr._finish_plan(o)                                            # reads the table; redoes the plan when a pair overflowed
    assert tr.owner_replans == (1 if small_cap else 0)
    assert tr._own_cap == (int(want_table.max()) if small_cap else int(1.06 * n_per * NEG / G) + 4096)
    recs, off = U.np_owned(codes, n_all, NEG, G, rank)
    assert int(tr._own_off[n_all]) == len(recs)
    np.testing.assert_array_equal(tr._own_rec[:3 * len(recs)].numpy().reshape(-1, 3), recs)
    np.testing.assert_array_equal(tr._own_off[:n_all + 1].numpy(), off)
    np.testing.assert_array_equal(o.need_all[:n_all].numpy().astype(np.int64) & 0xFFFFFFFF, codes[::NEG] & U.NEED)
    for x in range(2):
        assert torch.equal(tr._slot[x][:n_all], slots[x])
        lo_hi = [(lo, int(tr._own_cnt[x][k])) for k, (_, lo, _) in enumerate(tr._parts)]
        for lo, n in lo_hi:
            assert torch.equal(tr._own[x][lo:lo + n], owns[x][lo:lo + n])
    assert torch.equal(o.cnt_host, cnt)
    info = tr.check()
    assert info["codes"] == "owner" and info["owner_code_capacity_per_pair"] == tr._own_cap
    assert info["code_bytes_received_per_epoch"] == 12 * G * tr._own_cap + 4 * G * n_per + 4 * G * G
    st = tr._build_part_step(len(tr._parts) - 1, 1)               # the step fields of the last part: its offsets into the list
    _, lo, hi = tr._parts[-1]
    assert st.own_rec is tr._own_rec and torch.equal(st.own_off, tr._own_off[lo:hi + 1])
    return refused


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,n_ent,small_cap", [(2, 600, False), (3, 602, False), (3, 80, True), (2, 600, True)])
def test_owner_plan_lists_equal_the_gather_plan(world, n_ent, small_cap):
    """world 3 with 602 entities: ragged shares (the last home rank's is shorter); 80 entities: a sixth of the positives need both
    vectors; small_cap: a pair capacity of 9 records, so the first exchange overflows everywhere and is redone at the exact maximum."""
    got = ranks.run_ranks(world, _worker, (n_ent, small_cap), limit=240)
    assert sorted(got) == list(range(world))
    for rank, out in got.items():
        assert out is True, f"rank {rank}: {out}"


def test_the_new_entry_points_validate_without_a_gpu():
    """mke_oc_bucket_codes / mke_oc_owned_index / the owned-list fields: declared, exported, and every argument error returns its
    code before any launch (fake addresses: a call that launched would not return an argument code)."""
    import ctypes as C
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    L = _lib.lib()
    assert L.mke_version() == 107                                      # additions only: no field moved
    p, F = (lambda a: C.c_void_p(a)), 0x10000
    bc = lambda **k: L.mke_oc_bucket_codes(p(k.get("codes", F)), C.c_int64(k.get("n", 8)), C.c_int(k.get("N", 4)), C.c_int64(k.get("pos0", 0)),
                                           C.c_int(k.get("G", 2)), C.c_int64(k.get("cap", 16)), p(k.get("need", F)), p(k.get("send", F)),
                                           p(k.get("counts", F)), p(k.get("scratch", F)), None)
    assert bc(G=0) == -2 and bc(G=17) == -2 and bc(N=65) == -2 and bc(cap=-1) == -2 and bc(n=-1) == -2
    assert bc(pos0=(1 << 31) - 4) == -4 and bc(n=1 << 29, N=8) == -4   # MKE_E_RANGE: positions / codes of a share below 2^31
    assert bc(counts=None) == -1 and bc(scratch=None) == -1 and bc(need=None) == -1 and bc(codes=None) == -1 and bc(send=None) == -1
    oi = lambda **k: L.mke_oc_owned_index(p(k.get("recv", F)), p(k.get("counts", F)), C.c_int(k.get("G", 2)), C.c_int64(k.get("cap", 16)),
                                          C.c_int64(k.get("n_all", 8)), p(k.get("own_rec", F)), p(k.get("own_off", F)), None)
    assert oi(G=0) == -2 and oi(cap=-1) == -2 and oi(n_all=-1) == -2 and oi(n_all=1 << 31) == -4
    assert oi(recv=None) == -1 and oi(counts=None) == -1 and oi(own_rec=None) == -1 and oi(own_off=None) == -1
    assert b"mke_oc_owned_index" in L.mke_last_error()
    # the plan: an owned list without its records; the step: own_off on the atomics form, own_off without own_rec
    a = _lib.OcEmPlanArgs()
    a.n_ranks, a.rank, a.n_local, a.n_rel, a.chunks, a.capacity, a.neg_per_pos = 2, 0, 10, 3, 1, 100, 4
    for f in ("keys", "keys_alt", "vals_alt", "scratch8", "wave_scratch", "refs", "rows", "off", "flags", "scan", "step_row0", "n_refs", "temp",
              "item_row", "item_off", "item_part", "long_row", "long_part0", "step_item0", "step_long0", "step_part0"):
        setattr(a, f, F)
    a.own_off, a.own_cap = F, 32
    assert L.mke_oc_em_plan(C.byref(a), None) == -2 and b"owned list" in L.mke_last_error()
    import oc_owned_util as U
    _step = U.fake_step
    s = _step(peers=0, em=False, own_off=F, own_rec=F)
    score = lambda s: L.mke_oc_score(C.byref(s), p(F), C.c_int64(2 * 16 * 80), p(F), p(F), None)
    assert score(s) == -3 and b"own_off" in L.mke_last_error()        # MKE_E_UNSUPPORTED: the atomics form reads all-gathered codes
    assert score(_step(peers=0, own_off=F, own_rec=None, codes=None)) == -1 and b"own_rec" in L.mke_last_error()
    # owned lists make the codes optional: with both NULL the check names the codes, with own_off it passes on to the launch's own
    assert score(_step(peers=0, codes=None)) == -1 and b"codes" in L.mke_last_error()
    assert L.mke_oc_score(C.byref(_step(peers=0, own_off=F, own_rec=F, codes=None)), p(F), C.c_int64(2 * 16 * 80), p(F), p(None), None) == -1
    assert b"codes" not in L.mke_last_error()

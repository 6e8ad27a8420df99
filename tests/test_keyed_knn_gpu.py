"""`neighbour_table(keyed=True)` whole: the matrix-free selection of a capped table against the whole-row path on the same
operands in the same (working) order, byte for byte; its slices, its launches, its redo, and the drivers' `truncated_keyed`.

The fixture: n = 6,000, d = 16, k = 1,500, cap = 64, a column sample of 2,048, z = 3.  The thresholds are the 444-th and the
581-st largest of a row's 2,048 sample similarities (s = 512).  tests/keyed_oracle.py on the CPU, on float32 similarities of
exactly these operands and with the key margin included (key_below = 104 / 1,500 of the key range): 0 of the 6,000 rows leave
with a status other than 0 (largest list 603 of the 1,024 slots), so the 5 % bound below is a condition with room, not a
measurement.  At z = 0.25 (ranks 506 and 519) the same run sends 4,372 rows (73 %) to the redo, 2,224 with status 1 and 2,148
with status 3; the bounds of the redo test (30 % in all, 10 % on either side) are well inside that."""
import contextlib
import io
from unittest import mock

import numpy as np
import pytest
import torch

import thin_oracle as to

pytestmark = pytest.mark.gpu

SEED = 2 ** 63 + 31_337
N, D, K, CAP, N_TOTAL = 6000, 16, 1500, 64, 20_000
PARAMS = dict(n_samp=2048, z=3)


def operands():
    """random unit rows, 1 % of them copies of other rows (exact ties), under scattered ids"""
    rng = np.random.default_rng(2024)
    e = rng.standard_normal((N, D)).astype(np.float32)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    dup = rng.choice(N, size=N // 100, replace=False)
    e[dup] = e[rng.choice(N, size=len(dup))]
    ids = rng.choice(N_TOTAL, size=N, replace=False).astype(np.int64)
    return e, ids


class _Fixture:
    """The operands, the keyed table and what it is held against, computed once and only read by the tests."""

    def __init__(self):
        from multike_amd.base.batch import keyed_perm, neighbour_table
        e, self.ids = operands()
        self.e = torch.as_tensor(e, device="cuda")
        self.stats = {}
        self.keyed = neighbour_table(self.e, self.ids, K, N_TOTAL, cap=CAP, seed=SEED, keyed=True, keyed_params=PARAMS, stats=self.stats)
        # the whole-row path on the already-permuted operands: the same columns in the same order
        perm = keyed_perm(N, 0x3C6EF372, "cuda")
        self.perm = perm.cpu().numpy()
        self.e_perm, self.ids_perm = self.e[perm].contiguous(), self.ids[self.perm]
        self.expected = neighbour_table(self.e_perm, self.ids_perm, K, N_TOTAL, cap=CAP, seed=SEED, keyed=False)
        self.uncapped = neighbour_table(self.e_perm, self.ids_perm, K, N_TOTAL)

    def call(self, **kw):
        from multike_amd.base.batch import neighbour_table
        kw.setdefault("keyed_params", PARAMS)
        return neighbour_table(self.e, self.ids, K, N_TOTAL, cap=CAP, seed=SEED, **kw)


@pytest.fixture(scope="module")
def fx():
    return _Fixture()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_keyed_table_is_the_whole_row_table_of_the_working_order(fx):
    assert fx.keyed[0].shape == (N_TOTAL, CAP) and fx.keyed[0].dtype == torch.int32
    assert _same(fx.keyed, fx.expected)
    valid = fx.keyed[1].cpu().numpy()
    assert valid.sum() == N and valid[fx.ids].all()
    rest = np.setdiff1d(np.arange(N_TOTAL), fx.ids)
    assert not fx.keyed[0].cpu().numpy()[rest].any()


def test_keyed_table_is_the_thinned_uncapped_table(fx):
    full = fx.uncapped[0].cpu().numpy()[fx.ids]
    assert full.shape == (N, K)
    want = to.thin(full, fx.ids, CAP, SEED)
    got = fx.keyed[0].cpu().numpy()[fx.ids]
    assert np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1))


def test_the_redo_does_not_hide_the_keyed_path(fx):
    print("keyed stats:", fx.stats)
    assert fx.stats["rows"] == N and fx.stats["redone"] == sum(fx.stats["redone_by_status"].values())
    assert fx.stats["redone"] <= 0.05 * N


def test_slices_launches_and_a_second_call_give_the_same_bytes(fx):
    assert _same(fx.call(keyed=True), fx.keyed)
    small = {}
    assert _same(fx.call(keyed=True, rows_per_launch=700, stats=small), fx.keyed) and small["rows"] == N
    table = torch.zeros_like(fx.keyed[0])
    valid = torch.zeros_like(fx.keyed[1])
    seen = []
    for r in range(3):
        st = {}
        t, v, ids = fx.call(keyed=True, part=(r, 3), stats=st)
        assert st["rows"] == ids.numel() == N * (r + 1) // 3 - N * r // 3
        assert np.array_equal(ids.cpu().numpy(), fx.ids_perm[N * r // 3:N * (r + 1) // 3])      # slices of the working order
        assert int(v.sum()) == ids.numel() and not t[fx.ids_perm[:N * r // 3]].any()
        table[ids], valid[ids] = t[ids], v[ids]
        seen.append(ids)
    assert torch.cat(seen).unique().numel() == N and _same((table, valid), fx.keyed)


def test_off_and_automatic_keep_the_path_and_the_bytes_of_this_shape(fx):
    today = fx.call()                                  # keyed=None: n < 262,144
    stats = {}
    assert _same(fx.call(keyed=False, stats=stats), today) and stats == {}
    from multike_amd.base.batch import neighbour_table
    plain = neighbour_table(fx.e, fx.ids, K, N_TOTAL, cap=CAP, seed=SEED)
    assert _same(today, plain)
    want = to.thin(neighbour_table(fx.e, fx.ids, K, N_TOTAL)[0].cpu().numpy()[fx.ids], fx.ids, CAP, SEED)
    assert np.array_equal(today[0].cpu().numpy()[fx.ids], want)          # the capped table of before: list order of the id order


def test_rows_the_thresholds_miss_are_redone_to_the_same_bytes(fx):
    """z = 0.25: the band is 13 sample ranks wide and the k-th value falls outside it for most rows, on either side."""
    stats = {}
    got = fx.call(keyed=True, keyed_params=dict(n_samp=2048, z=0.25), stats=stats)
    print("keyed stats at z = 0.25:", stats)
    assert _same(got, fx.expected)
    by = stats["redone_by_status"]
    assert stats["redone"] >= 0.3 * N and by[1] >= 0.1 * N and by[3] >= 0.1 * N and stats["redone"] == sum(by.values())


def test_unknown_keyed_params_are_refused(fx):
    from multike_amd._lib import MultiKEHipError
    with pytest.raises(MultiKEHipError, match="keyed_params"):
        fx.call(keyed=True, keyed_params=dict(n_sample=100))


def test_tiny_samples_and_no_lower_threshold():
    """n = 300, a sample of 37: the lower rank lies beyond the sample, every column is band or sure."""
    from multike_amd.base.batch import keyed_perm, keyed_sample_ranks, neighbour_table
    rng = np.random.default_rng(5)
    n, k, cap = 300, 200, 16
    e = rng.standard_normal((n, 8)).astype(np.float32)
    e = torch.as_tensor(e / np.linalg.norm(e, axis=1, keepdims=True), device="cuda")
    ids = rng.permutation(n).astype(np.int64)
    assert keyed_sample_ranks(k, n, n // 8, 3) == (9, 41) and n // 8 == 37
    stats = {}
    got = neighbour_table(e, ids, k, n, cap=cap, seed=SEED, keyed=True, stats=stats)
    perm = keyed_perm(n, 0x3C6EF372, "cuda")
    assert _same(got, neighbour_table(e[perm].contiguous(), ids[perm.cpu().numpy()], k, n, cap=cap, seed=SEED, keyed=False))
    assert stats["rows"] == n


# ------------------------------------------------------ driver -------------------------------------------------------
def _run_driver(tmp_path, tag, truncated_keyed):
    """One short run; at every refresh the installed table is held against the other path ON THE SAME EMBEDDINGS (two runs do
    not train the same bits: tests/test_capped_knn_gpu.py)."""
    from multike_amd import MultiKE_Late as p_late
    from multike_amd.MultiKE_CSL import MultiKE_CV
    from multike_amd.synthetic import SyntheticData, synthetic_args
    data = SyntheticData(n_ent=3000, dim=20)                 # 1,500 entities per KG: k = int((1 - 0.9) * 1500) = 149
    args = synthetic_args(dim=20, batch_size=1500, attribute_batch_size=1500, entity_batch_size=1500, neg_triple_num=5,
                          learning_rate=0.01, max_epoch=2, shared_learning_max_epoch=1, start_valid=100, eval_freq=10,
                          start_predicate_soft_alignment=100, truncated_freq=1, truncated_epsilon=0.9, truncated_cap=32,
                          truncated_keyed=truncated_keyed, output=str(tmp_path / tag) + "/")
    calls, real = [], p_late.neighbour_table

    def recording(emb, useful, k, n_total, **kw):
        stats = {}
        out = real(emb, useful, k, n_total, **kw, stats=stats)
        other = real(emb, useful, k, n_total, **{**kw, "keyed": not kw.get("keyed")})
        calls.append(dict(kw=dict(kw), k=k, useful=np.asarray(useful), stats=stats, table=out[0].cpu().numpy(), valid=out[1].cpu().numpy(),
                          other=tuple(x.cpu().numpy() for x in other)))
        return out

    with mock.patch.object(p_late, "neighbour_table", recording), contextlib.redirect_stdout(io.StringIO()):
        model = MultiKE_CV(data, args, data.predicate_align_model)
        res = model.run()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in res.values()) and len(calls) == 4
    return calls


def test_driver_installs_the_same_tables_with_and_without_the_keyed_path(tmp_path):
    on = _run_driver(tmp_path, "on", 1)
    off = _run_driver(tmp_path, "off", 0)
    for calls, flag in ((on, True), (off, False)):
        for c in calls:
            assert c["kw"]["keyed"] is flag and c["kw"]["cap"] == 32 and c["k"] == 149
            u = c["useful"]
            assert np.array_equal(np.sort(c["table"][u], axis=1), np.sort(c["other"][0][u], axis=1))       # as sets per row
            assert np.array_equal(c["valid"], c["other"][1])
            assert (c["stats"].get("rows") == len(u)) == flag                                              # the path that ran

"""The auction kernels (mke_assign_rounds / mke_assign_finish) against their NumPy definition, bit for bit: on every case the
device's state, price and progress equal the oracle's, the duality certificate is empty, match / counts agree with state, and the
run is identical with and without the tail kernel and for batches of 1 round, 32 rounds and one large call.  The cases are the
smallest shapes at which each mechanism can go wrong: list lengths around the wavefront width, lists ended by a bad column,
values that are not finite, ties in value and in bids, everybody wanting the same columns (the grid form's long run), more rows
than columns, a floor that makes rows give up, the hand-over to the tail kernel at several rounds, and empty inputs."""
import functools

import numpy as np
import pytest

import assign_oracle as AO

f32 = np.float32
ONE_CALL = 4096                       # rounds of "one large call": above every case's round count
FORMS = ((0, 32), (1, 32), (0, 1), (1, 1), (0, ONE_CALL), (1, ONE_CALL))     # (flags, batch)


# ------------------------------------------------------------------------------------------------ cases
def sweep_lists(n_a, n_b, cut, seed):
    """(a): distinct random columns per row, values in eighths (ties in value and in bids), value descending then column
    ascending; lists longer than n_b are padded with column -1; a tenth of the rows end early at a column outside [0, n_b) with
    listed-looking entries behind it; a few values are +inf / -inf."""
    rng = np.random.default_rng(seed)
    val = np.full((n_a, cut), -np.inf, f32)
    col = np.full((n_a, cut), -1, np.int32)
    m = min(cut, n_b)
    for i in range(n_a):
        c = rng.permutation(n_b)[:m]
        v = (rng.integers(0, 9, m) / 8).astype(f32)
        o = np.lexsort((c, -v))
        val[i, :m], col[i, :m] = v[o], c[o]
        if m > 1 and rng.random() < 0.1:
            col[i, rng.integers(1, m)] = -1 if rng.random() < 0.5 else n_b      # ends the list; what follows is never read
        if m > 0 and rng.random() < 0.1:
            val[i, rng.integers(0, m)] = np.inf if rng.random() < 0.5 else -np.inf
    return val, col


def same_columns(n_a, cut):
    """(b): everybody lists columns 0 .. cut - 1 at the values 1 .. 0."""
    return (np.tile(np.linspace(1, 0, cut).astype(f32), (n_a, 1)), np.tile(np.arange(cut, dtype=np.int32), (n_a, 1)))


@functools.lru_cache(maxsize=None)
def quantised_lists(n_a, n_b, cut):
    """(c): similarities of unit Gaussians quantised to quarters."""
    return AO.top_lists(AO.recipe_sim(2, n_a, n_b, np.random.default_rng(77)), cut)


@functools.lru_cache(maxsize=None)
def noisy_lists(n, cut):
    """(d): noisy-copy embeddings; the lists made with NumPy from the float32 similarity matrix."""
    e1, e2 = AO.noisy_copy(n, 32, 0.22, 5)
    return AO.top_lists(e1 @ e2.T, cut)


def _case(name):
    """name -> (val, col, n_b, eps, floor, tail caps to run)."""
    kind, *rest = name.split(":")
    p = [float(x) if "." in x or "e" in x else int(x) for x in rest]
    if kind == "sweep":
        n_a, cut, half = p
        n_b = n_a // 2 if half else n_a + 3
        return (*sweep_lists(n_a, n_b, cut, 100 * n_a + cut + half), n_b, 0.02, -1.0, (0,))
    if kind == "same":
        n_a, cut, floor = p
        return (*same_columns(n_a, cut), cut + 5, 1e-2, floor, (0,))
    if kind == "short":
        floor, = p
        return (*quantised_lists(1100, 900, 12), 900, 1e-2, floor, (0,))
    if kind == "handover":
        cut, = p
        return (*noisy_lists(2000, cut), 2000, 1e-3, -1.0, (1, 64, 0, 300, 2500))
    if kind == "norows":
        return np.zeros((0, 4), f32), np.zeros((0, 4), np.int32), 5, 0.02, -1.0, (0,)
    if kind == "nocolumns":
        return np.ones((70, 3), f32), np.zeros((70, 3), np.int32), 0, 0.02, -1.0, (0,)
    if kind == "emptylists":
        return np.ones((300, 5), f32), np.full((300, 5), -1, np.int32), 40, 0.02, -1.0, (0,)
    if kind == "highfloor":
        val, col = sweep_lists(300, 200, 7, 9)
        return val, col, 200, 0.02, 1.5, (0,)
    raise KeyError(name)


CASES = ([f"sweep:{n_a}:{cut}:{half}" for n_a in (1, 63, 64, 65, 257) for cut in (1, 2, 7, 64, 100, 130) for half in (0, 1)] +
         ["same:300:8:-1.0", "same:300:8:0.5", "same:1100:16:-1.0", "short:0.0", "short:1.0", "handover:20", "handover:100",
          "norows", "nocolumns", "emptylists", "highfloor"])
# the oracle's round counts of the named long cases, re-checked on the CPU: the case is what its name says
ROUNDS = {"same:300:8:-1.0": 1005, "same:300:8:0.5": 68, "same:1100:16:-1.0": 2212}


def case_and_oracle(name):
    val, col, n_b, eps, floor, caps = _case(name)
    if n_b == 0:      # the oracle indexes price[0]: no column is every list ended at once, which one unlisted column says as well
        state, price, progress = AO.auction(val, np.full_like(col, -1), 1, eps, floor)
        return val, col, n_b, eps, floor, caps, (state, price[:0], progress)
    return val, col, n_b, eps, floor, caps, AO.auction(val, col, n_b, eps, floor)


# ------------------------------------------------------------------------------------------------ the device
def device_run(val, col, n_b, eps, floor, flags, batch, tail_cap):
    import torch
    from multike_amd import _lib
    from multike_amd.base import alignment as AL
    v, c = torch.as_tensor(val).cuda().contiguous(), torch.as_tensor(col).cuda().contiguous()
    state, price, progress, _ = AL._auction(v, c, n_b, eps, floor, batch, 1 << 20, tail_cap, flags)
    match = torch.full((col.shape[0],), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    _lib.assign_finish(_lib.assign_args(v, c, n_b, eps, floor, state, None, None, None, None, None, match=match, counts=counts))
    return state.cpu().numpy(), price.cpu().numpy(), progress.cpu().tolist(), match.cpu().numpy(), counts.cpu().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_oracle(name):
    val, col, n_b, eps, floor, caps, (state, price, progress) = case_and_oracle(name)
    n_a = col.shape[0]
    print(f"{name}: oracle progress {progress}")
    assert progress[1] == 0 and progress[0] < ONE_CALL
    if name in ROUNDS:
        assert progress[0] == ROUNDS[name]
    assert AO.certificate(val, col, n_b, eps, floor, state, price) == []
    want_match = np.where(state > 0, state - 1, -1)
    want_counts = [int((want_match >= 0).sum()), int((want_match == np.arange(n_a)).sum()), int((state == -1).sum())]
    for cap in caps:
        for flags, batch in FORMS:
            if flags and cap != caps[0]:
                continue                                    # without the tail kernel tail_cap changes nothing: once
            got = device_run(val, col, n_b, eps, floor, flags, batch, cap)
            what = (name, cap, flags, batch)
            assert np.array_equal(got[0].astype(np.int64), state), what
            assert np.array_equal(got[1].view(np.uint32), price.view(np.uint32)), what          # bit for bit
            assert got[2] == progress, (what, got[2], progress)
            assert np.array_equal(got[3], want_match) and got[4] == want_counts, what
            assert AO.certificate(val, col, n_b, eps, floor, got[0], got[1]) == [], what


@pytest.mark.gpu
def test_matching_surface_and_the_round_limit():
    import torch
    from multike_amd import _lib
    from multike_amd.base.alignment import assignment_matching
    val, col, n_b, eps, floor, _, (state, price, progress) = case_and_oracle("same:300:8:0.5")
    v, c = torch.as_tensor(val).cuda(), torch.as_tensor(col).cuda()
    match, p, prog = assignment_matching(v, c, n_b, eps, floor)
    assert match.dtype == torch.int32 and match.is_cuda and p.is_cuda and prog.is_cuda
    assert np.array_equal(match.cpu().numpy(), np.where(state > 0, state - 1, -1))
    assert np.array_equal(p.cpu().numpy().view(np.uint32), price.view(np.uint32)) and prog.cpu().tolist() == progress
    for flags in (0, _lib.ASSIGN_NO_TAIL):
        with pytest.raises(_lib.MultiKEHipError, match="eps = 0.01"):
            assignment_matching(v, c, n_b, eps, floor, max_rounds=5, flags=flags)
    with pytest.raises(_lib.MultiKEHipError, match="flags"):
        assignment_matching(v, c, n_b, eps, floor, flags=_lib.ASSIGN_TAIL_ONLY)

"""The epoch sampler (k_neg_sample, mke_sampler.hip): group shapes of 16 / 32 / 64 lanes, wave-uniform side with a double pass for
wavefronts of two KGs, 32-bit offsets, the prefilter in front of the known-triple table, a strided grid.  Every case here is
exact equality of integer arrays: against the C restatement of the specification (oracle/mke_oracle.c) for every output word,
and against the Python specification itself (oracle/sampler_oracle.py) for a spread of positives (it is a Python loop per
draw).  Shapes are small and chosen for where the kernel's paths can go wrong: wavefronts of two KGs, sides of different form,
populations that force the duplicate fix-up, dense sets that force later rounds, sets whose filter came late."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from sampler_cases import Side as _Side
from sampler_cases import dev as _dev
from sampler_cases import expected_negatives

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE_HEAD, CODE_FAST = 1 << 26, 1 << 27


def _positions(n, at, offset=11):
    """Stream position of every positive: the epoch positions 3 i + 5 that `at` launches pass, else pos_offset + i."""
    return 3 * np.arange(n) + 5 if at else np.arange(n) + offset


def _sample(pos, kg, sides, N, codes, at, max_try, seed, sid, offset=11):
    """Device output as numpy arrays: (neg_h, neg_r, neg_t), or (code,) in the code-word form.  `at`: mke_neg_sample_at with the
    epoch positions 3 i + 5, else mke_neg_sample with pos_offset."""
    from multike_amd import _lib
    from multike_amd.sampling import side_array
    n = len(pos[0])
    dpos = tuple(_dev(x) for x in pos)
    dkg = None if kg is None else _dev(kg, np.uint8)
    sa = side_array(sides[0].dev, sides[-1].dev)
    index = _dev(_positions(n, True)) if at else None
    if codes:
        out = (torch.full((n * N,), -1, dtype=torch.int32, device="cuda"),)
        _lib.neg_sample_codes(dpos, offset, index, dkg, sa, N, max_try, seed, sid, out[0])
    else:
        out = tuple(torch.full((n * N,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
        if at:
            _lib.neg_sample_at(dpos, index, dkg, sa, N, max_try, seed, sid, out)
        else:
            _lib.neg_sample(dpos, offset, dkg, sa, N, max_try, seed, sid, out)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _spec_rows(pos, kg, sides, N, at, max_try, seed, sid, rows, offset=11):
    """The specification's ids of the positives `rows`: [len(rows), N] per array."""
    out = [np.zeros((len(rows), N), np.int32) for _ in range(3)]
    for j, i in enumerate(int(x) for x in rows):
        k = 0 if kg is None else int(kg[i] != 0)
        gi = 3 * i + 5 if at else i + offset
        got = sides[k if len(sides) > 1 else 0].spec(int(pos[0][i]), int(pos[1][i]), int(pos[2][i]), N, seed, sid + k, gi, max_try)
        for a, g in zip(out, got):
            a[j] = g
    return out


def _codes_of(ids, pos, rows):
    """The code words of header section (1c) (without MKE_CODE_EXCL) of the ids [len(rows), N] of the positives `rows`."""
    nh, _, nt = ids
    h, t = pos[0][rows][:, None], pos[2][rows][:, None]
    return np.where(nh != h, nh | CODE_HEAD | CODE_FAST, np.where(nt != t, nt | CODE_FAST, np.broadcast_to(t, nt.shape))).astype(np.int32)


def _spread(n, count=40):
    """First, last and evenly spread positives: every wavefront position and both ends of the launch."""
    return sorted(set(np.linspace(0, n - 1, min(n, count)).astype(int).tolist()) | set(range(min(n, 6))) | {n - 1})


def _check(pos, kg, sides, N, max_try=10, seed=(123, 456), sid=7, forms=((False, False), (True, False), (False, True), (True, True)),
           spec_count=40):
    """device == the C restatement, every output word; == the Python specification on a spread of positives.  forms: (codes, at)
    pairs."""
    n = len(pos[0])
    rows = np.array(_spread(n, spec_count))
    for at in sorted({a for _, a in forms}):
        spec = _spec_rows(pos, kg, sides, N, at, max_try, seed, sid, rows)
        ids = expected_negatives(pos, kg, sides, N, _positions(n, at), max_try, seed, sid)
        for a, w in zip(ids, spec):
            assert np.array_equal(a[rows], w), f"C restatement != specification: N={N} at={at}"
        for codes in sorted({c for c, a in forms if a == at}):
            got = _sample(pos, kg, sides, N, codes, at, max_try, seed, sid)
            want = (_codes_of(ids, pos, np.arange(n)),) if codes else ids
            for a, w in zip(got, want):
                a = a.reshape(n, N)
                assert np.array_equal(a, w), f"device != C restatement: N={N} codes={codes} at={at}: {int((a != w).sum())} of {a.size} words"
            want = (_codes_of(spec, pos, rows),) if codes else spec
            for a, w in zip(got, want):
                assert np.array_equal(a.reshape(n, N)[rows], w), f"device != specification: N={N} codes={codes} at={at}"


def _triples(rng, ents, n_rel, count):
    return np.stack([rng.choice(ents, count), rng.integers(0, n_rel, count), rng.choice(ents, count)], 1).astype(np.int32)


def _runner_kg(n, b0=20, b1=17):
    """pos_kg of the relation loop: steps of b0 positives of KG 0, then b1 of KG 1 — the boundaries fall inside wavefronts."""
    return (np.arange(n) % (b0 + b1) >= b0).astype(np.uint8)


@pytest.fixture(scope="module")
def two_kgs():
    """Two sides of different form in one launch: a contiguous range and an entity list, each with its known-triple set."""
    rng = np.random.default_rng(25)
    e0, e1 = np.arange(0, 900), rng.permutation(np.arange(1000, 2900, 2))
    k0, k1 = _triples(rng, e0, 7, 5000), _triples(rng, e1, 7, 5000)
    return rng, (e0, e1), (k0, k1), [_Side(e0, k0), _Side(e1, k1)]


def _positives(known, kg, n):
    """Positives drawn from the known triples of their KG (as the loop's are)."""
    pos = np.zeros((n, 3), np.int32)
    for k in (0, 1):
        m = kg == k
        pos[m] = known[k][np.arange(int(m.sum())) % len(known[k])]
    return pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()


@pytest.mark.parametrize("N", [1, 15, 16, 25, 31, 32, 33, 64])
def test_every_group_size_both_forms_both_entry_points(two_kgs, N):
    """neg_per_pos across every group size (16 / 32 / 64 lanes) and the "idle lane for the coin" edge (15 | 16, 31 | 32 | 33, 64),
    ids and code words, mke_neg_sample and mke_neg_sample_at, a runner-like pos_kg, n_pos no multiple of anything."""
    rng, ents, known, sides = two_kgs
    n = 1999
    kg = _runner_kg(n)
    _check(_positives(known, kg, n), kg, sides, N)


@pytest.mark.parametrize("N", [1, 25, 40])
def test_a_launch_larger_than_the_grid_cap(two_kgs, N):
    """The kernel strides by a capped grid (32 workgroups per CU: 8,192 on the MI355X = 131,072 / 65,536 / 32,768 positives
    of the 16- / 32- / 64-lane form).  150,001 positives pass the cap in every form, so wavefronts take a second, partly
    filled, iteration."""
    rng, ents, known, sides = two_kgs
    n = 150_001
    kg = _runner_kg(n)
    co.set_threads(16)                  # N = 40: six million draws of the C restatement; its output does not depend on the threads
    try:
        _check(_positives(known, kg, n), kg, sides, N, forms=((True, False), (False, True)), spec_count=24)
    finally:
        co.set_threads(1)               # its default


@pytest.mark.parametrize("n", [1, 2, 3, 5, 129, 4095])
@pytest.mark.parametrize("layout", ["alternate", "runner", "none"])
def test_mixed_wavefronts_and_ragged_launches(two_kgs, layout, n):
    """Wavefronts whose groups are of different KGs (alternating positives: one group of each KG in every wavefront of the 32-lane
    form; a KG 1 prefix / KG 2 suffix whose boundary falls inside a wavefront), pos_kg == NULL, and n_pos that fills neither a
    wavefront nor a workgroup (n_pos = 1 included)."""
    rng, ents, known, sides = two_kgs
    kg = {"alternate": (np.arange(n) % 2).astype(np.uint8), "runner": _runner_kg(n, 3, 2) if n < 100 else _runner_kg(n), "none": None}[layout]
    pos = _positives(known, kg if kg is not None else np.zeros(n, np.uint8), n)
    for N in (10, 25, 40):            # 16, 32 and 64 lanes per positive
        _check(pos, kg, sides if kg is not None else sides[:1], N, forms=((False, False), (True, True)), spec_count=24)


@pytest.mark.parametrize("forms", ["range+list", "table_valid+range", "table+list", "list+table_valid"])
def test_sides_of_different_form_in_one_launch(forms):
    """ent_lo range, ent_list, cand_table with and without cand_valid — two different ones per launch, so that the wave-uniform
    path takes different branches in different wavefronts (and in the two passes of a mixed wavefront)."""
    rng = np.random.default_rng(3)
    n_tot, K = 1200, 70
    e0, e1 = np.arange(0, 600), rng.permutation(np.arange(600, 1200))
    table = np.stack([rng.choice(n_tot, K, replace=False) for _ in range(n_tot)]).astype(np.int32)
    valid = (np.arange(n_tot) % 3 != 0).astype(np.uint8)
    k0, k1 = _triples(rng, e0, 5, 3000), _triples(rng, e1, 5, 3000)

    def make(kind, ents, known):
        if kind == "range":
            return _Side(np.sort(ents), known)
        if kind == "list":
            return _Side(ents if not np.array_equal(ents, np.sort(ents)) else ents[::-1], known)
        return _Side(ents, known, table, valid if kind == "table_valid" else None)

    a, b = forms.split("+")
    sides = [make(a, e0, k0), make(b, e1, k1)]
    n = 777
    kg = _runner_kg(n)
    pos = _positives((k0, k1), kg, n)
    for N in (10, 25, 40):
        _check(pos, kg, sides, N, forms=((False, False), (True, False)), spec_count=24)


@pytest.mark.parametrize("N,extra", [(15, 1), (16, 2), (25, 1), (31, 3), (32, 1), (33, 2), (64, 1), (64, 3)])
def test_populations_barely_larger_than_the_sample(N, extra):
    """neg_per_pos + 1 .. + 3 candidates: almost every group sees a duplicate first draw, so the LDS table reports it and the
    sequential fix-up runs, in every group shape, in wavefronts of one KG and of two."""
    rng = np.random.default_rng(N * 10 + extra)
    pop = N + extra
    sides = [_Side(np.arange(0, pop)), _Side(rng.permutation(np.arange(100, 100 + pop)))]
    n = 301
    kg = _runner_kg(n, 5, 4)
    pos = (np.where(kg == 0, rng.integers(0, pop, n), rng.integers(100, 100 + pop, n)).astype(np.int32), rng.integers(0, 4, n).astype(np.int32),
           np.where(kg == 0, rng.integers(0, pop, n), rng.integers(100, 100 + pop, n)).astype(np.int32))
    _check(pos, kg, sides, N, forms=((False, False), (True, False)), spec_count=30)


def _dense_kg(lo, n_ent=48, n_rel=3, share=0.8, seed=5):
    """Most (h, r, t) over a small entity range ARE triples: the prefilter says "maybe" nearly always, the table says "known" for
    most candidates, and the rounds after the first do the work."""
    rng = np.random.default_rng(seed)
    h, r, t = np.meshgrid(np.arange(lo, lo + n_ent), np.arange(n_rel), np.arange(lo, lo + n_ent), indexing="ij")
    allt = np.stack([h.ravel(), r.ravel(), t.ravel()], 1).astype(np.int32)
    return allt[rng.random(len(allt)) < share]


@pytest.mark.parametrize("max_try", [1, 2, 4])
@pytest.mark.parametrize("N", [10, 25, 40])
def test_later_rounds_and_the_keep_anyway_rule_on_a_dense_kg(N, max_try):
    k0, k1 = _dense_kg(0, seed=5), _dense_kg(48, seed=6)
    sides = [_Side(np.arange(0, 48), k0), _Side(np.arange(48, 96)[::-1], k1)]
    n = 1501
    kg = _runner_kg(n)
    pos = _positives((k0, k1), kg, n)
    _check(pos, kg, sides, N, max_try=max_try, forms=((False, False), (True, True)), spec_count=30)
    if max_try == 1:                   # the setting is what it claims: most first-round candidates are known triples
        ids = _sample(pos, kg, sides, N, False, False, 1, (123, 456), 7)
        known = {tuple(x) for x in np.concatenate([k0, k1]).tolist()}
        assert np.mean([tuple(x) in known for x in np.stack(ids, 1)[:2000].tolist()]) > 0.5


def test_a_set_built_before_and_after_its_filter_exists():
    """The filter of a set is created late, from a table that already holds keys (k_filter_from_table has only the stored key to
    go by), and then extended by a second build: the sampler must keep answering what the table answers — the C restatement with
    the first half of the triples known, then with both halves."""
    from multike_amd import _lib
    tr = _dense_kg(0, share=0.6, seed=2)
    half = len(tr) // 2
    side = _Side(np.arange(0, 48), tr[:half])
    pos = (tr[:, 0].copy(), tr[:, 1].copy(), tr[:, 2].copy())

    def both(what):
        for N in (10, 25):
            got = _sample(pos, None, [side], N, False, False, 3, (9, 9), 1)
            want = expected_negatives(pos, None, [side], N, _positions(len(tr), False), 3, (9, 9), 1)
            for a, w in zip(got, want):
                assert np.array_equal(a.reshape(len(tr), N), w), what
        return got

    # a copy of the table that the library never built: no filter, the kernel probes it directly
    keys = side.ks.keys.clone()
    _lib.tripleset_forget(keys)
    assert _lib.tripleset_filter_bytes(keys) == 0
    owner, side.dev.known = side.ks, type("K", (), {"keys": keys})()
    first = both("no filter")
    # the second half arrives through mke_tripleset_build: the filter is created now, from the first half + the second
    _lib.tripleset_build(_dev(tr[half:, 0]), _dev(tr[half:, 1]), _dev(tr[half:, 2]), keys)
    assert _lib.tripleset_filter_bytes(keys) > 0
    side.set_host_known(tr)
    second = both("late filter")
    rows = np.array(_spread(len(tr), 30))
    spec = _spec_rows(pos, None, [side], 25, False, 3, (9, 9), 1, rows)
    for a, w in zip(second, spec):
        assert np.array_equal(a.reshape(len(tr), 25)[rows], w)
    assert any(not np.array_equal(a, b) for a, b in zip(first, second))      # the second half did change the answers
    _lib.tripleset_forget(keys)
    del owner


def test_the_launchers_choice_of_32_bit_offsets():
    """Which instantiation a launch takes, on both sides of each limit, from the launcher's own predicate (a host function in a
    header of its own) — not from a multi-GB launch."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    src = r'''
#include <cstdio>
#include "mke_sampler_o32.h"
int main() {
  const long long L = 1ll << 30;
  const long long cases[][4] = {
      {919908, 25, 100000, 100000}, {L, 1, 5, 5}, {L + 1, 1, 5, 5}, {L / 64, 64, 5, 5}, {L / 64 + 1, 64, 5, 5}, {L / 25, 25, 5, 5},
      {L / 25 + 1, 25, 5, 5}, {1, 1, L, 5}, {1, 1, L + 1, 5}, {1, 1, 5, L}, {1, 1, 5, L + 1}, {1ll << 40, 64, 5, 5}, {0, 25, 5, 5}};
  for (const auto& c : cases) std::printf("%d", (int)mke::sampler_o32_fits(c[0], (int)c[1], c[2], c[3]));
  std::printf("\n");
  return 0;
}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "o32.cpp"), "w") as f:
            f.write(src)
        exe = os.path.join(d, "o32")
        subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "multike_amd", "csrc"), os.path.join(d, "o32.cpp"), "-o", exe])
        got = subprocess.check_output([exe]).decode().strip()
    assert got == "1101010101001", got

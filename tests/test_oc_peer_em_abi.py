"""Peer-direct entity-major step, C-ABI without a GPU: the new entry point and phase bit are exported and declared, the
refusals that kept the two forms apart are gone, and every argument error of the new ground returns its code before any
launch (the descriptors below hold fake device addresses: a call that launched would not return an argument code)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


FAKE = 0x10000


def _step(peers=2, em=True, **over):
    """A descriptor that passes every check of the step: 2 ranks, stride 80, 8 positives, fake addresses everywhere."""
    from multike_amd import _lib
    s = _lib.OcStepStruct()
    for f in ("ent", "ent_acc", "ent_grad", "ent_touched", "rel", "rel_acc", "rel_grad", "rel_touched", "pos_h", "pos_r", "pos_t",
              "slot_h", "slot_t", "own_h", "own_t", "codes"):
        setattr(s, f, FAKE)
    s.n_local, s.n_rel, s.rel_grad_copies = 100, 5, 1
    s.stride, s.dim, s.rank, s.n_ranks = 80, 75, 0, 2
    s.n_pos, s.per, s.n_own_h, s.n_own_t, s.neg_per_pos, s.capacity = 8, 4, 3, 2, 4, 16
    s.optimizer, s.lr, s.scale, s.tag = _lib.OPT_ADAGRAD, 0.01, 1.0, 1
    s.n_peers = peers
    for g in range(peers):
        s.peer_v[g], s.peer_g[g] = FAKE, FAKE
    if em:
        s.em_coef, s.em_chunks, s.em_block_floats = FAKE, 1, 2 * 16 * 80
        s.em_refs = s.em_rows = s.em_off = FAKE
        s.em_v[0] = s.em_gv[0] = FAKE
    for k, v in over.items():
        setattr(s, k, v)
    return s


def _run(lib, s, phases, send=FAKE, v_all=FAKE, g_all=FAKE, gv=FAKE, loss=FAKE):
    p = lambda a: C.c_void_p(a)
    return lib.mke_oc_run(C.byref(s), C.c_int(phases), p(send), p(v_all), C.c_int64(2 * 16 * 80), p(g_all), p(gv), p(loss), None)


def test_gv_sum_is_exported_declared_and_listed(lib):
    from multike_amd import _lib
    assert "mke_oc_gv_sum" in _lib.SYMBOLS
    getattr(C.CDLL(_lib.SO_PATH), "mke_oc_gv_sum")
    h = open(os.path.join(ROOT, "include", "multike_hip.h")).read()
    assert int(re.search(r"#define MKE_OC_GVSUM (\d+)", h).group(1)) == 64 == _lib.OC_GVSUM
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()   # no field moved: no new version


def test_score_of_a_peer_direct_entity_major_step_needs_the_mirror(lib):
    p = lambda a: C.c_void_p(a)
    s = _step()
    score = lambda v_all: lib.mke_oc_score(C.byref(s), p(v_all), C.c_int64(2 * 16 * 80), p(None), p(FAKE), None)
    assert score(None) == E_NULL
    assert b"mirror" in lib.mke_last_error()
    assert _run(lib, s, 4, v_all=None) == E_NULL                       # ... through mke_oc_run(MKE_OC_SCORE) as well
    # the check no longer refuses the combination itself: an empty step gets as far as the NULL loss partials
    assert lib.mke_oc_score(C.byref(_step(n_pos=0)), p(FAKE), C.c_int64(2 * 16 * 80), p(None), p(None), None) == E_NULL
    assert b"does not run peer-direct" not in lib.mke_last_error()


def test_pass2_no_longer_refuses_peers(lib):
    from multike_amd import _lib
    assert lib.mke_oc_pass2(C.byref(_step(em_n_rows=0)), None) == 0    # nothing to do: returns before any launch
    assert lib.mke_oc_pass2(C.byref(_step(em_n_rows=0, em_chunks=0)), None) == E_SHAPE      # its other checks still hold
    assert lib.mke_oc_pass2(C.byref(_step(em=False)), None) == E_UNSUPPORTED
    assert _run(lib, _step(em_n_rows=0), _lib.OC_PASS2) == 0


def test_apply_on_an_entity_major_step_is_still_refused(lib):
    from multike_amd import _lib
    for phases in (_lib.OC_APPLY, _lib.OC_SCORE | _lib.OC_APPLY, _lib.OC_GVSUM | _lib.OC_APPLY):
        assert _run(lib, _step(), phases) == E_UNSUPPORTED
    assert lib.mke_oc_apply(C.byref(_step()), C.c_void_p(FAKE), None) == E_UNSUPPORTED


def test_gv_sum_argument_errors(lib):
    from multike_amd import _lib
    p = lambda a: C.c_void_p(a)
    G = _lib.OC_GVSUM
    assert _run(lib, _step(peers=0), G) == E_UNSUPPORTED               # collectives: the reduce-scatter has done the sum
    assert _run(lib, _step(em=False), G) == E_UNSUPPORTED              # atomics form: mke_oc_apply sums the inbox itself
    assert _run(lib, _step(), G, g_all=None) == E_NULL
    assert _run(lib, _step(), G, gv=None) == E_NULL
    assert _run(lib, _step(n_own_h=0, n_own_t=0), G) == 0              # no owned slot: nothing launched
    assert _run(lib, _step(n_own_h=17), G) == E_SHAPE                  # the step's own checks come first
    assert _run(lib, _step(peers=1), G) == E_SHAPE                     # n_peers is 0 or n_ranks
    # the stand-alone entry point: the same answers
    gs = lambda s, inbox, gv: lib.mke_oc_gv_sum(C.byref(s), p(inbox), p(gv), None)
    assert lib.mke_oc_gv_sum(None, p(FAKE), p(FAKE), None) == E_NULL
    assert gs(_step(peers=0), FAKE, FAKE) == E_UNSUPPORTED
    assert gs(_step(em=False), FAKE, FAKE) == E_UNSUPPORTED
    assert gs(_step(), None, FAKE) == E_NULL and gs(_step(), FAKE, None) == E_NULL
    assert gs(_step(n_own_h=0, n_own_t=0), FAKE, FAKE) == 0
    assert lib.mke_last_error()

"""The auction decoder without a GPU: the three symbols are exported and bound (version unchanged), the ctypes structure matches
the header, every argument error returns its code and its message before any launch, mke_assign_temp_bytes, the hyper-parameters'
defaults, and what the sharded driver and the host surface refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as ah
from conftest import ROOT

NEW = ("mke_assign_temp_bytes", "mke_assign_rounds", "mke_assign_finish")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from multike_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        g.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "multike_hip.h")).read()


def test_new_symbols_exported_and_listed(lib):
    from multike_amd import _lib
    raw = C.CDLL(_lib.SO_PATH)
    h = _header()
    for s in NEW:
        assert s in _lib.SYMBOLS
        getattr(raw, s)
        assert re.search(r"^(?:int|int64_t)\s+" + s + r"\s*\(", h, flags=re.M), s
    assert int(re.search(r"#define MKE_VERSION (\d+)", h).group(1)) == 107 == lib.mke_version()   # additions only
    assert lib.mke_assign_temp_bytes.restype is C.c_int64
    for name in ("MKE_ASSIGN_TAIL_CAP", "MKE_ASSIGN_NO_TAIL", "MKE_ASSIGN_TAIL_ONLY"):
        assert int(re.search(r"#define %s (\d+)" % name, h).group(1)) == getattr(_lib, name[4:])
    src = open(os.path.join(ROOT, "multike_amd", "csrc", "mke_assign.hip")).read()
    assert int(re.search(r"#define ASSIGN_TAIL_MAX (\d+)", src).group(1)) == _lib.ASSIGN_TAIL_MAX
    assert "mke_assign.hip" in open(os.path.join(ROOT, "multike_amd", "csrc", "Makefile")).read()


def test_struct_fields_match_header():
    from multike_amd import _lib
    names = ah.members("mke_assign_args")
    assert names == [f for f, _ in _lib.AssignArgs._fields_]
    assert names == ["n_a", "n_b", "cut", "val", "col", "eps", "floor", "state", "price", "owner", "bid", "progress", "tail_cap",
                     "flags", "temp", "temp_bytes", "match", "counts"]                      # the order the issue fixed
    kinds = dict(_lib.AssignArgs._fields_)
    assert kinds["n_a"] is C.c_int64 and kinds["temp_bytes"] is C.c_int64 and kinds["eps"] is C.c_float and kinds["cut"] is C.c_int


def _args(**over):
    from multike_amd import _lib
    fake = C.c_void_p(0x1000)
    base = dict(n_a=100, n_b=60, cut=8, val=fake, col=fake, eps=1e-3, floor=-1.0, state=fake, price=fake, owner=fake, bid=fake,
                progress=fake, tail_cap=0, flags=0, temp=fake, temp_bytes=1 << 20, match=fake, counts=fake)
    base.update(over)
    return _lib.AssignArgs(**base)


def test_rounds_argument_errors(lib):
    def call(want, text, n_rounds=4, **over):
        assert lib.mke_assign_rounds(C.byref(_args(**over)), n_rounds, None) == want, over
        msg = lib.mke_last_error().decode()
        assert msg.startswith("mke_assign_rounds: ") and text in msg, (over, msg)

    assert lib.mke_assign_rounds(None, 1, None) == -1 and "mke_assign_rounds: NULL args" in lib.mke_last_error().decode()
    for name in ("val", "col", "state", "price", "owner", "bid", "progress", "temp"):
        call(-1, "NULL pointer", **{name: None})
    call(-2, "cut < 1", cut=0)
    call(-2, "bad n_a / n_b", n_a=-1)
    call(-2, "bad n_a / n_b", n_a=0x7FFFFF01)
    call(-2, "bad n_a / n_b", n_b=1 << 31)
    for bad in (float("nan"), float("inf")):
        call(-4, "must be finite", eps=bad)
        call(-4, "must be finite", floor=bad)
    call(-4, "must be finite", floor=float("-inf"))
    call(-4, "eps below 2^-14", eps=2.0 ** -15)
    call(-4, "eps below 2^-14", eps=0.0)
    call(-4, "eps below 2^-14", eps=-1.0)
    call(-2, "n_rounds < 0", n_rounds=-1)
    call(-2, "tail_cap < 0", tail_cap=-1)
    call(-3, "unknown flags", flags=4)
    call(-3, "unknown flags", flags=3)
    need = lib.mke_assign_temp_bytes(C.c_int64(100), C.c_int64(60), 0)
    call(-2, "temp below mke_assign_temp_bytes (%d)" % need, temp_bytes=need - 1)
    call(-2, "temp below mke_assign_temp_bytes", temp_bytes=lib.mke_assign_temp_bytes(C.c_int64(100), C.c_int64(60), 64), tail_cap=65)
    # nothing to do: success without a launch, whatever the pointers
    assert lib.mke_assign_rounds(C.byref(_args(n_a=0, val=None, col=None, state=None, temp=None, temp_bytes=0)), 4, None) == 0
    assert lib.mke_assign_rounds(C.byref(_args(eps=2.0 ** -14)), 0, None) == 0          # 2^-14 itself is accepted


def test_finish_argument_errors(lib):
    def call(want, text, **over):
        assert lib.mke_assign_finish(C.byref(_args(**over)), None) == want, over
        msg = lib.mke_last_error().decode()
        assert msg.startswith("mke_assign_finish: ") and text in msg, (over, msg)

    assert lib.mke_assign_finish(None, None) == -1 and "mke_assign_finish: NULL args" in lib.mke_last_error().decode()
    for name in ("state", "match", "counts"):
        call(-1, "NULL pointer", **{name: None})
    call(-2, "cut < 1", cut=0)
    call(-2, "bad n_a / n_b", n_b=-1)


def test_temp_bytes(lib):
    from multike_amd import _lib
    tb = lambda n_a, n_b, cap: lib.mke_assign_temp_bytes(C.c_int64(n_a), C.c_int64(n_b), cap)
    assert tb(100, 60, 0) == 256 + 4 * _lib.ASSIGN_TAIL_CAP == tb(0, 0, 0) == tb(0x7FFFFF00, 0x7FFFFF00, 0)      # independent of the sizes
    assert tb(100, 60, 1) == 260 and tb(100, 60, 64) == 256 + 256
    assert tb(100, 60, 4096) == tb(100, 60, 1 << 30) == 256 + 4 * _lib.ASSIGN_TAIL_MAX      # larger values act as 4096
    assert tb(-1, 60, 0) == -2 and "mke_assign_temp_bytes: bad n_a / n_b" in lib.mke_last_error().decode()
    assert tb(100, 1 << 31, 0) == -2
    assert tb(100, 60, -1) == -2 and "tail_cap < 0" in lib.mke_last_error().decode()
    assert _lib.assign_temp_bytes(100, 60) == tb(100, 60, 0)
    with pytest.raises(_lib.MultiKEHipError, match="bad n_a / n_b"):
        _lib.assign_temp_bytes(-1, 60)


def test_hyper_parameters_and_the_sharded_driver():
    from multike_amd import _lib
    from multike_amd.distributed_run import _ShardedMixin
    from multike_amd.utils import default_args
    d = default_args()
    assert d.assign_cut == 0 and d.assign_eps == 1e-3 and d.assign_floor is None
    with pytest.raises(_lib.MultiKEHipError, match="assign_cut"):
        _ShardedMixin()._init_sharded(None, default_args(assign_cut=100), None, 0, 2)     # refused before any data is touched


def test_host_surface_refuses_before_the_device():
    from multike_amd import _lib
    from multike_amd.base.alignment import assignment_alignment
    e1, e2 = np.ones((5, 8), dtype=np.float32), np.ones((4, 8), dtype=np.float32)
    with pytest.raises(_lib.MultiKEHipError, match="len\\(embed2\\) >= len\\(embed1\\)"):
        assignment_alignment(e1, e2, "inner", True, 0, 4)
    with pytest.raises(_lib.MultiKEHipError, match="choose one re-scoring"):
        assignment_alignment(e2, e1, "inner", True, 10, 4, sinkhorn=(4, 0.1))
    with pytest.raises(_lib.MultiKEHipError, match="a given sim_mat is used as it is"):
        assignment_alignment(e2, e1, "inner", True, 0, 4, sim_mat=np.ones((4, 5), dtype=np.float32), sinkhorn=(4, 0.1))
    with pytest.raises(_lib.MultiKEHipError, match="manhattan"):
        assignment_alignment(e2, e1, "manhattan", True, 0, 4)
    for eps in (0.0, 2.0 ** -15, float("nan"), float("inf")):
        with pytest.raises(_lib.MultiKEHipError, match="2\\^-14"):
            assignment_alignment(e2, e1, "inner", True, 0, 4, eps=eps)

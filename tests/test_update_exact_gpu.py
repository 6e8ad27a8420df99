"""The optimizer kernels -- k_rows_update / k_rows_update_multi (mke_update.hip), k_rows_update_dense / k_dense_update_opt
(mke_dense_opt.hip) and the flat k_dense_update -- against the references of update_cases.py, through the C ABI itself
(mke_update_table, mke_count_job and mke_optimizer filled here), at every row width and ragged dim, every chunk and row shape,
with privatised copies, hub rows, the slot_of owner path, several tables per launch, the count rider and every grid cap.

Tier 1 is compared as bit patterns: SGD without normalisation (table, grad and every copy, hub copies, slot_of, ref_count),
Adagrad's accumulator without normalisation, Adam's m / v and Adadelta's accum at beta = rho = 1/2.  Tier 2 (normalised rows,
Adagrad's w, Adam, Adadelta) is held against float64 within the bound update_cases.py derives by counting roundings; the
bound is not fitted to the device.  test_update_cases.py shows, without a device, that thirteen kinds of subtly wrong kernel
fail these comparisons.  Every test prints the worst error / bound it saw ("RATIO ...") before it asserts.

Worst error / bound observed on the MI355X (gfx950), per kernel and output (w: the table; none above 1, so no finding):

  k_rows_update, k_rows_update_multi    quarter-wave rows                        whole-wave rows
    SGD, normalised                     w 0.4991                                 w 0.4972
    Adagrad                             w 0.4947                                 w 0.3826
    Adagrad, normalised                 w 0.4998  acc 0.4545                     w 0.5000  acc 0.4545
  k_rows_update_dense                   plain                                    normalised
    Adam, beta = 1/2                    w 0.1913                                 w 0.1225  m 0.3131  v 0.3916
    Adam, TF defaults                   w 0.3325  m 0.2857  v 0.2437             w 0.4836  m 0.3488  v 0.3461
    Adadelta, rho = 1/2                 w 0.4354  accum_update 0.1490            w 0.4992  accum 0.3355  accum_update 0.1254
    Adadelta, TF defaults               w 0.4147  accum 0.2243  a._update 0.0709 w 0.4999  accum 0.3470  accum_update 0.1093
  k_dense_update_opt                    Adam 1/2: w 0.1913; TF: w 0.3325 m 0.2857 v 0.2437
                                        Adadelta 1/2: w 0.4354 accum_update 0.1490; TF: w 0.4147 accum 0.2243 accum_update 0.0629
  k_dense_update                        Adagrad: w 0.3826

The figures next to 0.5 are elements whose error is the last rounding alone (half an ulp, charged a whole one); where both
ran the same case the device gave the figure of the float32 NumPy emulation of test_update_cases.py, so the 2 ulp allowed for
rsqrtf, rsq, sqrtf and the division were not needed by these operands.

Bitmap tables (mke_update_table.bits / pos_h / pos_t / n_pos: walk_chunk on pair 11, walk_list on pair 01 named by the step's
positives; update_cases.BIT_CASES and BIT_LAUNCHES) run through the same comparison; SGD without normalisation matched bit for
bit at every row count, list length and pattern, alone and in the production launch with and without the count rider.  Worst
error / bound:

  bitmap tables                         quarter-wave rows                        whole-wave rows          64-bit mask
    SGD, normalised                     w 0.4989
    Adagrad                             w 0.4947                                 w 0.3826                 w 0.3826
    Adagrad, normalised                 w 0.4993  acc 0.4524                     w 0.4978  acc 0.4545

test_update_cases.py shows that nine kinds of kernel that walk the bitmap or the list wrongly fail these comparisons.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import update_cases as uc
from multike_amd._abi import mke_count_job as CountJob     # the generated class: the prototypes accept no other
from rows_cases import TAG

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return None if t is None else t.cpu().numpy()


def addr(t):
    return None if t is None else t.data_ptr()


def opt_code(c):
    from multike_amd import _lib
    return {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "adam": _lib.OPT_ADAM, "adadelta": _lib.OPT_ADADELTA}[c.opt]


def sync():
    """A device error ends the session: nothing more is started on a card that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error: {e}", returncode=3)


class chunk_option:
    """The process-wide "update_chunk" for the duration of a launch."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from multike_amd import _lib
        self.old = _lib.set_option("update_chunk", self.value)

    def __exit__(self, *exc):
        from multike_amd import _lib
        _lib.set_option("update_chunk", self.old)


def report(ratios, kernel, c):
    for name, r in ratios.items():
        print(f"RATIO {kernel}:{c.opt}{'+norm' if c.normalize else ''}{':' + c.hyper if c.hyper else ''}:{name} {r:.4f} {c.id}")


def upload(c):
    o = uc.rows_ops(c)
    return {k: dev(getattr(o, k)) for k in uc.BUFFERS}


def table_struct(c, d):
    from multike_amd import _lib
    t = _lib.UpdateTableStruct()
    t.table, t.acc, t.grad, t.touched = addr(d["table"]), addr(d["acc"]), addr(d["grad"]), addr(d["touched"])
    t.n_rows, t.normalize, t.grad_copies, t.ref_count = c.n, c.normalize, c.copies, addr(d["ref_count"])
    if c.n_ranks:
        t.src_rows, t.slot_of, t.n_ranks, t.capacity = addr(d["src_rows"]), addr(d["slot_of"]), c.n_ranks, uc.rows_ops(c).capacity
    if c.n_hot:
        t.hot = _lib.HotRowsStruct(addr(d["hot_slot"]), c.n_hot, c.hot_copies, c.n)           # row0 = n_rows
    if c.bits:                                                       # the bitmap row and the step's positives in place of the flags
        t.bits, t.pos_h, t.pos_t, t.n_pos = addr(d["bits"]), addr(d["pos_h"]), addr(d["pos_t"]), c.n_pos
    return t


def launch_multi(tables, count=None):
    """One mke_rows_update_multi[_count] launch over fresh operands -> (the buffers of every table, the rider's ref_count)."""
    from multike_amd import _lib
    c0 = tables[0]
    ds = [upload(t) for t in tables]
    arr = (_lib.UpdateTableStruct * len(tables))(*[table_struct(t, d) for t, d in zip(tables, ds)])
    args = (arr, C.c_int(len(tables)), C.c_int32(TAG), C.c_int(c0.stride), C.c_int(c0.dim), C.c_int(opt_code(c0)), C.c_float(c0.lr))
    counted = None
    with chunk_option(c0.chunk):
        if count is None:
            code = _lib.lib().mke_rows_update_multi(*args, _lib._stream())
        else:
            o = uc.count_ops(count)
            cd = [dev(x) for x in (o.pos_h, o.pos_t, o.neg_h, o.neg_t, o.ref_count)]
            n_neg = count.n_pos * count.neg_per_pos
            cj = CountJob(addr(cd[0]), addr(cd[1]), count.n_pos, addr(cd[2]), addr(cd[3]), n_neg, count.neg_per_pos, addr(cd[4]))
            code = _lib.lib().mke_rows_update_multi_count(*args, C.byref(cj), _lib._stream())
            counted = cd[4]
    assert code == 0, _lib.lib().mke_last_error()
    sync()
    return [{k: host(v) for k, v in d.items()} for d in ds], host(counted)


def launch_single(c):
    """mke_rows_update on fresh operands, acc = NULL under SGD."""
    from multike_amd import _lib
    d = upload(c)
    acc = d["acc"] if c.opt == "adagrad" else None
    with chunk_option(c.chunk):
        code = _lib.lib().mke_rows_update(C.c_void_p(addr(d["table"])), C.c_void_p(addr(acc)), C.c_void_p(addr(d["grad"])), C.c_int(c.copies),
                                          C.c_void_p(addr(d["touched"])), C.c_int32(TAG), C.c_int64(c.n), C.c_int(c.stride), C.c_int(c.dim),
                                          C.c_int(c.normalize), C.c_int(opt_code(c)), C.c_float(c.lr), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    torch.cuda.synchronize()
    return {k: host(v) for k, v in d.items()}


def shape_name(c, shard=False):
    return "rows-" + uc.row_shape(c.n, c.stride, c.chunk, shard or bool(c.n_ranks))


def run_rows(c):
    o, want = uc.rows_ops(c), uc.rows_reference(c)
    (got,), _ = launch_multi([c])
    problems, ratios = uc.check_rows(o, got, want)
    report(ratios, shape_name(c), c)
    assert not problems, (c.id, "mke_rows_update_multi", problems)
    if not (c.n_hot or c.n_ranks):                                   # what the single-table entry point can express (it has no ref_count)
        problems, ratios = uc.check_rows(o, launch_single(c), {k: v for k, v in want.items() if k != "ref_count"})
        report(ratios, shape_name(c), c)
        assert not problems, (c.id, "mke_rows_update", problems)


def grouped(cases, key):
    out = {}
    for c in cases:
        out.setdefault(key(c), []).append(c)
    return out


PLAIN = grouped([c for c in uc.cases_of("rows") if not (c.n_hot or c.n_ranks or c.tag)], lambda c: f"s{c.stride}-d{c.dim}")
HUB = grouped([c for c in uc.cases_of("rows") if c.n_hot], lambda c: f"s{c.stride}-n{c.n}")
SHARD = grouped([c for c in uc.cases_of("rows") if c.n_ranks], lambda c: f"s{c.stride}-n{c.n}-ch{c.chunk}")


@pytest.mark.parametrize("key", list(PLAIN))
def test_rows_update(key):
    """Every chunk, flag pattern, copy count and both row shapes of this width; SGD bit for bit, the arithmetic within its bound."""
    for c in PLAIN[key]:
        run_rows(c)


@pytest.mark.parametrize("key", list(HUB))
def test_hub_rows(key):
    for c in HUB[key]:
        run_rows(c)


@pytest.mark.parametrize("key", list(SHARD))
def test_slot_of(key):
    for c in SHARD[key]:
        run_rows(c)


def test_chunk_by_size():
    """500,001 rows: chunk 64 by size alone.  The touched rows against the reference, every other row on the device."""
    from multike_amd import _lib
    (c,) = uc.cases_of("rows", tag="bysize")
    o, want = uc.rows_ops(c), uc.rows_reference(c)
    table, grad, touched = dev(o.table), dev(o.grad), dev(o.touched)
    table0, grad0 = table.clone(), grad.clone()
    with chunk_option(0):
        code = _lib.lib().mke_rows_update(C.c_void_p(addr(table)), None, C.c_void_p(addr(grad)), C.c_int(1), C.c_void_p(addr(touched)),
                                          C.c_int32(TAG), C.c_int64(c.n), C.c_int(c.stride), C.c_int(c.dim), C.c_int(0),
                                          C.c_int(opt_code(c)), C.c_float(c.lr), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    rows = dev(want["rows"])
    assert np.array_equal(uc.bits(host(table[rows])), uc.bits(want["table"][0]))
    assert not host(grad[rows]).any()
    table[rows], grad[rows] = table0[rows], grad0[rows]
    assert torch.equal(table.view(torch.int32), table0.view(torch.int32)) and torch.equal(grad, grad0)
    assert torch.equal(touched, dev(o.touched))


def same_buffers(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(uc.bits(a[k]), uc.bits(b[k])) for k in uc.BUFFERS)


@pytest.mark.parametrize("L", [L for L in uc.LAUNCHES if not L.count], ids=lambda L: L.name)
def test_several_tables(L):
    """Every table of the launch against its reference and, bit for bit, against what it gives alone."""
    gots, _ = launch_multi(L.tables)
    shard = any(t.n_ranks for t in L.tables)
    for t, got, want in zip(L.tables, gots, uc.launch_reference(L)):
        problems, ratios = uc.check_rows(uc.rows_ops(t), got, want)
        report(ratios, shape_name(t, shard), t)
        assert not problems, (L.name, t.id, problems)
        if t.n:
            (alone,), _ = launch_multi([t])
            assert same_buffers(got, alone), (L.name, t.id)
        else:
            assert same_buffers(got, {k: getattr(uc.rows_ops(t), k) for k in uc.BUFFERS})


@pytest.mark.parametrize("L", [L for L in uc.LAUNCHES if L.count], ids=lambda L: L.name)
def test_count_rider(L):
    """mke_rows_update_multi_count: the rider's counts follow the mke_count_entity_refs rule, the tables are those of the
    launch without it."""
    gots, counted = launch_multi(L.tables, L.count)
    assert np.array_equal(counted, uc.count_reference(L.count)), L.name
    plain, _ = launch_multi(L.tables)
    for t, got, alone, want in zip(L.tables, gots, plain, uc.launch_reference(L)):
        problems, _ = uc.check_rows(uc.rows_ops(t), got, want)
        assert not problems and same_buffers(got, alone), (L.name, t.id, problems)


# ----------------------------------------------------------------------------------------------------- bitmap tables
BITMAP = grouped(uc.BIT_CASES, lambda c: f"s{c.stride}" + ("-hub" if c.n_hot else ""))


def shape_name_bits(c):
    return "bits-" + uc.row_shape(c.n, c.stride, c.chunk)


@pytest.mark.parametrize("key", list(BITMAP))
def test_bitmap_rows(key):
    """mke_update_table.bits: the visited rows are pair 11 (walk_chunk) and pair 01 named by an entry of pos_h ++ pos_t
    (walk_list).  Everything else -- pair 01 that no entry names, pair 00 that one names, pair 10, the junk pairs behind the last
    row -- keeps table, accumulator and its SENTINEL gradient row bit for bit."""
    for c in BITMAP[key]:
        o, want = uc.rows_ops(c), uc.rows_reference(c)
        (got,), _ = launch_multi([c])
        problems, ratios = uc.check_rows(o, got, want)
        report(ratios, shape_name_bits(c), c)
        assert not problems, (c.id, problems)


@pytest.mark.parametrize("L", uc.BIT_LAUNCHES, ids=lambda L: L.name)
def test_bitmap_launches(L):
    """The production launch (a flagged relation table with privatised copies, then the bitmap table), with the count rider (list
    blocks, rider blocks, update blocks), the bitmap table alone, first, and without positives: every table against its
    reference and, bit for bit, against what it gives alone; the rider's counts by the mke_count_entity_refs rule."""
    gots, counted = launch_multi(L.tables, L.count)
    if L.count:
        assert np.array_equal(counted, uc.count_reference(L.count)), L.name
    for t, got, want in zip(L.tables, gots, uc.launch_reference(L)):
        problems, ratios = uc.check_rows(uc.rows_ops(t), got, want)
        report(ratios, shape_name_bits(t) if t.bits else shape_name(t), t)
        assert not problems, (L.name, t.id, problems)
        (alone,), _ = launch_multi([t])
        assert same_buffers(got, alone), (L.name, t.id)


def test_bitmap_refusals_launch_nothing():
    """A bitmap beside slot_of or grad_copies > 1, a second bitmap table, NULL lists: refused before any launch."""
    from multike_amd import _lib
    c = next(c for c in uc.BIT_CASES if c.n == 33 and c.stride == 16)
    d = upload(c)
    before = {k: v.clone() for k, v in d.items() if v is not None}

    def call(*structs):
        arr = (_lib.UpdateTableStruct * len(structs))(*structs)
        return _lib.lib().mke_rows_update_multi(arr, C.c_int(len(structs)), C.c_int32(TAG), C.c_int(c.stride), C.c_int(c.dim), C.c_int(opt_code(c)),
                                                C.c_float(c.lr), _lib._stream())

    t = table_struct(c, d)
    t.grad_copies = 2
    assert call(t) == -3
    assert call(table_struct(c, d), table_struct(c, d)) == -3
    t = table_struct(c, d)
    t.pos_t = None
    assert call(t) == -1
    t = table_struct(c, d)
    t.n_pos = -1
    assert call(t) == -2
    sync()
    for k, v in before.items():
        assert torch.equal(d[k].view(torch.int32), v.view(torch.int32)), k


# ----------------------------------------------------------------------------------------------------- the dense rules
def optimizer_struct(c, step):
    from multike_amd import _lib
    h = uc.HYPERS[c.hyper]
    return _lib.OptimizerStruct(opt_code(c), h.lr, h.b1, h.b2, h.eps, h.rho, step)


def run_dense(c):
    from multike_amd import _lib
    o, want = uc.dense_ops(c), uc.dense_reference(c)
    n = c.n
    d = {"table": dev(o.table), "s1": dev(o.s1), "s2": dev(o.s2)}
    for t, (g0, step) in enumerate(zip(o.grads, want), start=1):
        grad = dev(g0)
        p = [C.c_void_p(addr(x)) for x in (d["table"], d["s1"], d["s2"], grad)]
        if c.kernel == "dense_rows":
            opt = optimizer_struct(c, t)
            code = _lib.lib().mke_rows_update_dense(*p, C.c_int64(n), C.c_int(c.stride), C.c_int(c.dim), C.c_int(c.normalize), C.byref(opt),
                                                    _lib._stream())
        elif c.kernel == "dense_opt":
            opt = optimizer_struct(c, t)
            code = _lib.lib().mke_dense_update_opt(*p, C.c_int64(n), C.byref(opt), _lib._stream())
        else:
            code = _lib.lib().mke_dense_update(p[0], p[1], p[3], C.c_int64(n), C.c_int(opt_code(c)), C.c_float(c.lr), _lib._stream())
        assert code == 0, _lib.lib().mke_last_error()
        got = {k: host(v) for k, v in d.items() if v is not None}
        g = host(grad)
        assert not g[:n].any() and (g[n] == uc.SENTINEL).all(), (c.id, t)                       # consumed, and not past the end
        problems, ratios = uc.check_dense(o, got, step, n)
        report(ratios, c.kernel, c)
        assert not problems, (c.id, t, problems)
        if c.kernel == "dense_rows":                                                              # pad columns: 0 and SENTINEL stay
            assert not got["table"][:n, c.dim:].any() and (got["s1"][:n, c.dim:] == uc.SENTINEL).all() and (got["s2"][:n, c.dim:] == uc.SENTINEL).all()


DENSE_ROWS = grouped([c for c in uc.cases_of("dense_rows") if not c.tag], lambda c: f"s{c.stride}-d{c.dim}")


@pytest.mark.parametrize("key", list(DENSE_ROWS))
def test_rows_update_dense(key):
    """Adam and Adadelta over whole tables, three steps, with and without the Jacobian."""
    for c in DENSE_ROWS[key]:
        run_dense(c)


@pytest.mark.parametrize("c", uc.cases_of("dense_rows", tag="pass"), ids=lambda c: c.id)
def test_rows_update_dense_second_grid_pass(c):
    run_dense(c)


@pytest.mark.parametrize("opt", ("adam", "adadelta"))
def test_dense_update_opt(opt):
    for c in uc.cases_of("dense_opt", opt=opt):
        run_dense(c)


@pytest.mark.parametrize("opt", ("sgd", "adagrad"))
def test_dense_update(opt):
    for c in uc.cases_of("dense", opt=opt):
        run_dense(c)

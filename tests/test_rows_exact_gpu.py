"""The kernels of multike_amd/csrc/mke_rows.hip (and the common-space step loop on top of them) against the float64
references of rows_cases.py, at every row width, at the ragged dims, at the row counts around a block and around a grid pass.

Exact tier (torch.equal / ==): the operands are dyadic and every intermediate fits 24 bits (test_rows_cases.py proves it
without a device), so the device must return the float64 result bit for bit: gathered alignment loss, the saturated tier of
the gathered logistic loss, the row gather without normalisation, the placement probe, the fused alignment term with every id
pattern, and three SGD steps of mke_align_steps.  Tolerance tier: the normalised gather, the generic logistic loss, Adagrad on
normalised tables, each against float64 at tolerances derived or taken from the neighbouring tests.

The saturated logistic tier rests on the device's log(1.0f) being exactly 0 and rcp(1.0f) exactly 1, and on exp(-32) falling
below half an ulp of 1: test_saturation_identities_on_the_device prints what the device returns for single rows (the MI355X
returns exactly these values, so the tier is held with ==).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import rows_cases as rc
from oracle import multike_oracle as mo

pytestmark = pytest.mark.gpu
RT = 3e-6                       # loss of the generic logistic tier; its gradient rows: rtol 1e-4, atol 2e-6 (test_losses_gpu.py)
NORM_RTOL = 2e-6                # normalised gather: 24 roundings of the sum of squares halved by rsqrt, ~2 ulp of rsqrtf, one product
f32 = np.float32


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return t.cpu().numpy()


def nan_partials():
    from multike_amd import _lib
    return torch.full((_lib.LOSS_PARTIALS,), float("nan"), dtype=torch.float64, device="cuda")


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def check_partials(lp, loss, n, what):
    """Every partial overwritten (none of the NaNs left), all zero for an empty launch, their sum the float64 loss exactly."""
    p = host(lp)
    assert np.isfinite(p).all(), what
    if n == 0:
        assert not p.any(), what
    assert p.sum() == loss, (what, p.sum(), loss)


def groups(kernel, key):
    """The untagged cases of a kernel by key(case) -> {id: [cases]}; tagged cases (heavy, pass) run one by one."""
    out = {}
    for c in rc.cases_of(kernel):
        if not c.tag:
            out.setdefault(key(c), []).append(c)
    return out


def dense_key(c):
    return f"{c.kernel}-d{c.dim}-ldp{c.width - c.dim}"


def tagged(kernel):
    return [c for c in rc.cases_of(kernel) if c.tag]


# ----------------------------------------------------------------------------------------------------- gathered alignment
def run_galign(c):
    from multike_amd import _lib
    o = rc.galign_ops(c)
    n, dim, ld = c.n, c.dim, c.width
    a, b = dev(rc.poisoned(o.a.astype(f32), ld)), dev(rc.poisoned(o.b.astype(f32), ld))
    grad = c.variant == "grad"
    ga = dev(rc.sentinel_buffer(n, ld)) if grad else None
    gb = dev(rc.sentinel_buffer(n, ld)) if grad else None
    lp = nan_partials()
    if ld == dim:
        _lib.gathered_alignment_fwd_bwd(a[:n], b[:n], None if ga is None else ga[:n], None if gb is None else gb[:n], lp)
    else:       # the wrapper passes ld = dim
        code = _lib.lib().mke_gathered_alignment_fwd_bwd(ptr(a), ptr(b), C.c_int64(n), C.c_int(dim), C.c_int(ld), ptr(ga), ptr(gb),
                                                         ptr(lp), _lib._stream())
        assert code == 0, (c.id, _lib.lib().mke_last_error())
    check_partials(lp, o.loss, n, c.id)
    if grad:
        want = rc.sentinel_buffer(n, ld)
        want[:n, :dim] = o.ga
        assert np.array_equal(host(ga), want), c.id                 # ga == 2 (a - b); pad columns and the tail row untouched
        want[:n, :dim] = -o.ga
        assert np.array_equal(host(gb), want), c.id                 # gb == -ga


@pytest.mark.parametrize("key", list(groups("galign", dense_key)))
def test_gathered_alignment_exact(key):
    for c in groups("galign", dense_key)[key]:
        run_galign(c)


@pytest.mark.parametrize("c", tagged("galign") + [c for c in rc.cases_of("galign") if c.n > 1000], ids=lambda c: c.id)
def test_gathered_alignment_exact_across_a_grid_pass(c):
    run_galign(c)


# ----------------------------------------------------------------------------------------------------- gathered logistic
def launch_logistic(h, r, t, w, n, dim, ld, sign, gh, gr, gt, lp):
    from multike_amd import _lib
    if ld == dim:
        cut = lambda x: None if x is None else x[:n]
        _lib.gathered_logistic_fwd_bwd(cut(h), cut(r), cut(t), w, sign, cut(gh), cut(gr), cut(gt), lp)
    else:
        code = _lib.lib().mke_gathered_logistic_fwd_bwd(ptr(h), ptr(r), ptr(t), ptr(w), C.c_int64(n), C.c_int(dim), C.c_int(ld),
                                                        C.c_int(sign), ptr(gh), ptr(gr), ptr(gt), ptr(lp), _lib._stream())
        assert code == 0, _lib.lib().mke_last_error()


def run_glog(c):
    o = rc.glog_ops(c)
    n, dim, ld = c.n, c.dim, c.width
    h, r, t = (dev(rc.poisoned(m.astype(f32), ld)) for m in (o.h, o.r, o.t))
    w = None if o.w is None else dev(o.w.astype(f32))
    grad = not c.variant.startswith("nograd")
    gh, gr, gt = (dev(rc.sentinel_buffer(n, ld)) if grad else None for _ in range(3))
    lp = nan_partials()
    launch_logistic(h, r, t, w, n, dim, ld, c.sign, gh, gr, gt, lp)
    check_partials(lp, o.loss, n, c.id)
    if grad:
        want = rc.sentinel_buffer(n, ld)
        want[:n, :dim] = o.gh
        got_h, got_r, got_t = host(gh), host(gr), host(gt)
        assert np.array_equal(got_h, want), c.id                    # 2 w (h + r - t), or zero rows (sign -1): == , sign of zero open
        assert np.array_equal(got_r, got_h), c.id                   # gr == gh
        want[:n, :dim] = -o.gh
        assert np.array_equal(got_t, want), c.id                    # gt == -gh


def test_saturation_identities_on_the_device():
    """What the saturated tier rests on, one row at a time: from x = 32 on the term is exactly x and the gradient exactly
    2 (h + r - t) (sign +1); from x = 128 on the term and the gradient are exactly zero (sign -1).  The figures are printed
    before they are asserted.  The MI355X returns exactly these: terms 32, 36, 128, 144, 2880 and gradient factor 2.0 for
    sign +1 (so log(1.0f) is 0 and rcp(1.0f) is 1 on v_log_f32 / v_rcp_f32); term 0.0 and gradient factor -0.0 at
    x = 128, 144, 2880 for sign -1 (exp overflows to infinity, its reciprocal is 0)."""
    rows = ((32, 16, {2: 8}), (36, 16, {3: 4}), (128, 32, {3: 12, 2: 5}), (144, 16, {3: 16}), (2880, 320, {3: 320}))
    bad = []
    for sign in (1, -1):
        for x, dim, parts in rows:
            if x < (rc.SAT_POS if sign > 0 else rc.SAT_NEG):
                continue
            e = np.zeros((1, dim))
            at = 0
            for v, k in parts.items():
                e[0, at:at + k] = v
                at += k
            e[0, ::2] *= -1.0
            assert (e * e).sum() == x
            hh = np.clip(e, -1, 1)
            rr = np.clip(e - hh, -1, 1)
            tt = hh + rr - e
            assert np.abs(tt).max() <= 1
            g = [torch.full((1, dim), float("nan"), device="cuda") for _ in range(3)]
            lp = nan_partials()
            launch_logistic(dev(hh.astype(f32)), dev(rr.astype(f32)), dev(tt.astype(f32)), None, 1, dim, dim, sign, g[0], g[1], g[2], lp)
            loss, gh = host(lp).sum(), host(g[0]).astype(np.float64)
            ratio = gh[e != 0] / e[e != 0]
            print(f"device: x = {x} sign {sign:+d}: term {loss!r}, gradient / (h + r - t) in [{ratio.min()!r}, {ratio.max()!r}]")
            if loss != (x if sign > 0 else 0.0) or not np.array_equal(gh, 2.0 * e if sign > 0 else 0.0 * e):
                bad.append((x, sign, loss, ratio.min(), ratio.max()))
    assert not bad, bad


@pytest.mark.parametrize("key", list(groups("glog", dense_key)))
def test_gathered_logistic_saturated_exact(key):
    for c in groups("glog", dense_key)[key]:
        run_glog(c)


@pytest.mark.parametrize("c", [c for c in rc.cases_of("glog") if c.n > 1000], ids=lambda c: c.id)
def test_gathered_logistic_saturated_exact_across_a_grid_pass(c):
    run_glog(c)


def run_glog_generic(g, dim, sign, extra=0):
    """extra > 0: ld = dim + extra, operands in NaN-poisoned buffers; the gradient buffers are NaN all over either way, so a
    skipped row stays NaN and a write past dim or past the last row would show as a number."""
    n, ld = len(g.terms), dim + extra
    h, r, t, w = dev(rc.poisoned(g.h, ld)), dev(rc.poisoned(g.r, ld)), dev(rc.poisoned(g.t, ld)), dev(g.w)
    grads = [torch.full((n + 1, ld), float("nan"), device="cuda") for _ in range(3)]
    lp = nan_partials()
    launch_logistic(h, r, t, w, n, dim, ld, sign, grads[0], grads[1], grads[2], lp)
    p = host(lp)
    assert np.isfinite(p).all()
    full = [host(x) for x in grads]
    for x in full:
        assert np.isnan(x[n]).all() and np.isnan(x[:, dim:]).all()
    gh, gr, gt = (x[:n, :dim] for x in full)
    print(f"generic d{dim} ld+{extra} sign {sign:+d}: loss rel err {abs(p.sum() - g.loss) / abs(g.loss):.2e}, "
          f"gradient max abs err {np.abs(gh - g.gh).max():.2e}")
    np.testing.assert_allclose(p.sum(), g.loss, rtol=RT, atol=0)
    assert np.isfinite(gh).all() and np.isfinite(gr).all() and np.isfinite(gt).all()
    np.testing.assert_allclose(gh, g.gh, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(gr, g.gh, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(gt, -g.gh, rtol=1e-4, atol=2e-6)
    assert not gh[g.zero].any()                                      # (h + r) - t is exactly zero there


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("extra", rc.LD_EXTRA)
@pytest.mark.parametrize("dim", rc.DENSE_DIMS)
def test_gathered_logistic_generic_tier(dim, extra, sign):
    g = rc.glog_generic(dim, sign)
    assert g.terms.min() > 10 * RT * abs(g.loss)                     # one lost row cannot hide in the loss tolerance
    run_glog_generic(g, dim, sign, extra)


@pytest.mark.parametrize("sign", [1, -1])
def test_gathered_logistic_where_exp_overflows_or_goes_denormal(sign):
    """|z| in [80, 110]: exp(+x) is infinite in float32 (sign -1, inside the sigmoid), exp(-x) denormal (sign +1)."""
    g = rc.glog_generic(75, sign, n=64, n_extreme=8)
    run_glog_generic(g, 75, sign)


# ----------------------------------------------------------------------------------------------------- gather
def run_gather(c):
    from multike_amd import _lib
    o = rc.gather_ops(c)
    n = c.n
    table = dev(o.table)
    idx = None if o.idx is None else dev(o.idx)
    out = torch.full((n + 1, c.dim), rc.SENTINEL, dtype=torch.float32, device="cuda")
    _lib.gather_rows(table, c.variant == "norm", c.dim, idx, out[:n])
    got = host(out)
    assert np.all(got[n] == f32(rc.SENTINEL)), c.id                  # nothing behind the last row
    got = got[:n]
    if c.variant == "copy":
        assert np.array_equal(got.view(np.uint32), o.ref.view(np.uint32)), c.id        # bit for bit
        return
    np.testing.assert_allclose(got, o.ref, rtol=NORM_RTOL, atol=0, err_msg=c.id)
    for name, at in o.special.items():
        if name == "zero":
            assert not got[at].any(), c.id
        elif name == "tiny":                                         # below the epsilon floor: v * rsqrt(1e-12)
            np.testing.assert_allclose(got[at], 2.0 ** -30 * 1e6, rtol=NORM_RTOL, atol=0, err_msg=c.id)
        elif name == "underflow":
            np.testing.assert_allclose(got[at], 1e-25 * 1e6, rtol=NORM_RTOL, atol=0, err_msg=c.id)
        else:                                                        # norm exactly 1: the row itself, to the same rtol (rsqrtf(1) may be 1 ulp off)
            np.testing.assert_allclose(got[at], o.table[3, :c.dim][None, :].repeat(len(at), 0), rtol=NORM_RTOL, atol=0, err_msg=c.id)


@pytest.mark.parametrize("key", list(groups("gather", lambda c: f"gather-{c.variant}-s{c.width}-d{c.dim}")))
def test_gather_rows(key):
    for c in groups("gather", lambda c: f"gather-{c.variant}-s{c.width}-d{c.dim}")[key]:
        run_gather(c)


@pytest.mark.parametrize("c", tagged("gather"), ids=lambda c: c.id)
def test_gather_rows_across_a_grid_pass(c):
    run_gather(c)


def test_embedding_table_reads_go_through_the_gather():
    """EmbeddingTable.lookup / .eval (the product's read path) at a ragged dim: the normalised view, with and without ids."""
    from multike_amd.tables import EmbeddingTable
    rng = np.random.default_rng(3)
    vals = (0.3 * rng.standard_normal((70, 100))).astype(f32)
    ref = mo.l2_normalize_rows(vals.astype(np.float64))
    t = EmbeddingTable(70, 100, "t", normalize=True, values=vals)
    np.testing.assert_allclose(t.eval(), ref, rtol=NORM_RTOL, atol=0)
    idx = rng.integers(0, 70, 33)
    np.testing.assert_allclose(host(t.lookup(dev(idx))), ref[idx], rtol=NORM_RTOL, atol=0)
    raw = EmbeddingTable(70, 100, "raw", normalize=False, trainable=False, values=vals)
    assert np.array_equal(raw.eval(), vals)


# ----------------------------------------------------------------------------------------------------- probe
def run_probe(c):
    from multike_amd import _lib
    o = rc.probe_ops(c)
    n = c.n
    a, b, cc = (None if m is None else dev(m) for m in (o.a, o.b, o.c))
    out = torch.full((n + 1,), rc.SENTINEL, dtype=torch.float32, device="cuda")
    _lib.probe_rows(a, b, cc, dev(o.idx), out[:n])
    got = host(out)
    assert got[n] == f32(rc.SENTINEL), c.id
    assert np.array_equal(got[:n].astype(np.float64), o.ref), c.id


@pytest.mark.parametrize("key", list(groups("probe", lambda c: f"probe-s{c.width}")))
def test_probe_rows_exact(key):
    for c in groups("probe", lambda c: f"probe-s{c.width}")[key]:
        run_probe(c)


@pytest.mark.parametrize("c", tagged("probe"), ids=lambda c: c.id)
def test_probe_rows_exact_across_a_grid_pass(c):
    run_probe(c)


# ----------------------------------------------------------------------------------------------------- fused alignment term
def run_align(c):
    from multike_amd import _lib
    o = rc.align_ops(c)
    one = c.variant == "self"
    ta = dev(o.ta)
    tb = ta if one else dev(o.tb)
    want_a = c.variant not in ("no_ga", "loss_only")
    want_b = c.variant not in ("no_gb", "loss_only")
    flags = lambda: torch.full((c.rows,), rc.OLD_TAG, dtype=torch.int32, device="cuda")
    ga, toa = (torch.zeros_like(ta), flags()) if want_a else (None, None)
    gb, tob = ((ga, toa) if one else (torch.zeros_like(tb), flags())) if want_b else (None, None)
    lp = nan_partials()
    _lib.align_fwd_bwd(ta, False, tb, False, c.dim, dev(o.ia), dev(o.ib), c.weight, ga, toa, gb, tob, rc.TAG, lp)
    check_partials(lp, o.loss, c.n, c.id)
    for g, want, flag, hit in ((ga, o.ga, toa, o.hit_a), (gb, o.gb, tob, o.hit_b)):
        if g is None:
            continue
        got = host(g)
        assert np.array_equal(got.astype(np.float64), want), c.id    # the np.add.at reference, exactly
        assert not got[:, c.dim:].any(), c.id                        # pad columns still zero
        assert np.array_equal(host(flag), np.where(hit, rc.TAG, rc.OLD_TAG)), c.id
    assert np.array_equal(host(ta), o.ta) and np.array_equal(host(tb), o.tb), c.id     # the tables are read only


@pytest.mark.parametrize("key", list(groups("align", lambda c: f"align-s{c.width}-d{c.dim}")))
def test_align_fwd_bwd_exact(key):
    for c in groups("align", lambda c: f"align-s{c.width}-d{c.dim}")[key]:
        run_align(c)


@pytest.mark.parametrize("c", tagged("align"), ids=lambda c: c.id)
def test_align_fwd_bwd_exact_heavy_duplicates_and_grid_passes(c):
    run_align(c)


# ----------------------------------------------------------------------------------------------------- mke_align_steps
@pytest.mark.parametrize("c", rc.cases_of("steps"), ids=lambda c: c.id)
def test_align_steps_sgd_exact(c):
    from multike_amd import _lib
    from multike_amd.runner import run_alignment_steps
    from multike_amd.tables import EmbeddingTable
    o = rc.steps_ops(c)
    tabs = [EmbeddingTable(c.rows, c.dim, f"t{k}", normalize=False, trainable=(k != rc.STEPS_CONSTANT), values=t[:, :c.dim])
            for k, t in enumerate(o.tables)]
    assert all(t.stride == c.width for t in tabs)
    ring = run_alignment_steps(tabs, list(rc.STEPS_TERMS), dev(o.ia), dev(o.ib), o.off, "cs", 5, rc.STEPS_LR, optimizer="SGD")
    assert ring.shape == (4, len(rc.STEPS_TERMS), _lib.LOSS_PARTIALS)
    assert np.array_equal(host(ring).sum(-1), o.losses)             # every [step][term] block of partials
    for k, t in enumerate(tabs):
        assert np.array_equal(host(t.data).astype(np.float64), o.final[k]), k       # pad columns included
        if k == rc.STEPS_CONSTANT:
            assert np.array_equal(host(t.data).view(np.uint32), o.tables[k].view(np.uint32))
        else:
            assert not host(t.grad).any(), k                         # gradient scratch back at zero


# ----------------------------------------------------------------------------------------------------- normalised tables, Adagrad
def _common_space_setup(d, seed):
    rng = np.random.default_rng(seed)
    n_rows, B, lr = 200, 300, 0.01
    vals = [mo.xavier_truncated_normal((n_rows, d), rng).astype(f32) for _ in range(4)]
    # the name vectors: constants, read as they are.  Their norms are spread over [0.5, 1.5]: on unit rows a kernel that
    # normalised this side by the OTHER side's flag would change nothing
    vals[1] = (vals[1] / np.linalg.norm(vals[1], axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (n_rows, 1))).astype(f32)
    ia = rng.integers(0, n_rows, (2, B)).astype(np.int32)            # with replacement
    ib = rng.integers(0, n_rows, (2, B)).astype(np.int32)
    assert not np.array_equal(ia, ib) and len(np.unique(ia[0])) < B
    weights = (0.5, 1.0, 1.0)
    T = [v.astype(np.float64) for v in vals]
    acc = [np.full_like(t, 0.1) for t in T]
    losses = []
    for s in range(2):          # as tests/test_model_gpu.py composes the common-space step: three terms, one Adagrad step per table
        l1, g1a, _ = mo.alignment_step_dense(T[0], T[1], None, None, ia[s], ib[s], lr, weight=weights[0], b_norm=False, update=False)
        l2, g2a, g2b = mo.alignment_step_dense(T[0], T[2], None, None, ia[s], ib[s], lr, weight=weights[1], update=False)
        l3, g3a, g3b = mo.alignment_step_dense(T[0], T[3], None, None, ia[s], ib[s], lr, weight=weights[2], update=False)
        mo.adagrad_dense(T[0], acc[0], mo.l2_normalize_rows_backward(T[0], g1a + g2a + g3a), lr)
        mo.adagrad_dense(T[2], acc[2], mo.l2_normalize_rows_backward(T[2], g2b), lr)
        mo.adagrad_dense(T[3], acc[3], mo.l2_normalize_rows_backward(T[3], g3b), lr)
        losses.append(l1 + l2 + l3)
    return vals, ia, ib, weights, lr, T, losses


def _common_space_tables(vals, d):
    from multike_amd.tables import EmbeddingTable
    n = vals[0].shape[0]
    return [EmbeddingTable(n, d, "ent", True, values=vals[0]), EmbeddingTable(n, d, "name", False, trainable=False, values=vals[1]),
            EmbeddingTable(n, d, "rv", True, values=vals[2]), EmbeddingTable(n, d, "av", True, values=vals[3])]


@pytest.mark.parametrize("d", [75, 100])
def test_normalised_alignment_with_adagrad_matches_oracle(d):
    """Two consecutive common-space steps with ia != ib and ids drawn with replacement, through StepEngine.alignment_step and
    through run_alignment_steps, against alignment_step_dense + adagrad_dense in float64."""
    from multike_amd.runner import run_alignment_steps
    from multike_amd.tables import StepEngine
    vals, ia, ib, weights, lr, T, losses = _common_space_setup(d, 11)
    tabs = _common_space_tables(vals, d)
    eng = StepEngine()
    for s in range(2):
        a, b = dev(ia[s]), dev(ib[s])
        got = float(eng.alignment_step([(tabs[0], a, tabs[k], b, weights[k - 1]) for k in (1, 2, 3)], "cs", lr))
        print(f"engine d{d} step {s}: loss rel err {abs(got - losses[s]) / losses[s]:.2e}")
        np.testing.assert_allclose(got, losses[s], rtol=1e-5)
    for k in range(4):
        np.testing.assert_allclose(host(tabs[k].raw()), T[k], rtol=2e-4, atol=2e-6)
    tabs = _common_space_tables(vals, d)
    ring = run_alignment_steps(tabs, [(0, k, weights[k - 1]) for k in (1, 2, 3)], dev(ia.reshape(-1)), dev(ib.reshape(-1)),
                               np.array([0, 300, 600]), "cs", 1, lr)
    np.testing.assert_allclose(host(ring.sum(dim=(1, 2))), losses, rtol=1e-5)
    for k in range(4):
        np.testing.assert_allclose(host(tabs[k].raw()), T[k], rtol=2e-4, atol=2e-6)
    assert np.array_equal(host(tabs[1].raw()), vals[1])

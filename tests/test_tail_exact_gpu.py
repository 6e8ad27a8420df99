"""The tails of the dense steps on the device against tail_cases.py, kernel by kernel through the C ABI: the space-mapping
step (mke_mapping_step_phases: FWD, TAIL, BWD, UPD one at a time, the scratch read back after each), the attribute step's loss
tail (mke_attr_tail_z, mke_attr_tail_loss, mke_attr_tail_bwd alone; W^T and the backward on planted sums through
mke_attr_step_phases, fused and unfused) and the literal auto-encoder (mke_ae_step_phases: ENC, DEC, BWD; without activation
bit for bit, with tanh / sigmoid and for the plans [20, 12] at ldx 23, [150, 140, 130] and [32, 24, 16, 12, 8] within a bound).

Every phase starts from NaN-poisoned outputs and partials (the auto-encoder's zero-invariant partials excepted); the consuming
phases find the batch-wide sums the way the row-sharded trainer leaves them ([total, 0, ...], or split between slot 0 and slot
2047); a batch on the epsilon floor is reached with a view of 2^-25 entries and with planted totals.  Tier 1 (products of dyadic
operands, k_map_ortho, the scatters, the SGD update, W^T, the auto-encoder step without activation, every "keeps its poison"
check) is compared as bit patterns; tier 2 (everything behind rsqrtf, tanhf, the expf sigmoid and the logistic functions)
against float64 within the bound tail_cases.py derives.  test_tail_cases.py shows without a device that eighteen kinds of
subtly wrong kernel fail these comparisons.  Every test prints "RATIO <kernel>:<output> <error / bound> <case>" before it asserts.

Worst error / bound observed on the MI355X (gfx950), by output (none above 1, so no finding; 347 cases, 4.3 s):

  mapping    F 0.2943  V 0.2943  P 0.1708  ssq 0.0382  G 0.4990  GF 0.4990  loss 0.1690  dot 0.0851  dP 0.3304  gM 0.2554
  tail_z     z 0.1396  ssq 0.3220
  tail_loss  gout 0.1913  grad_ent 0.6236  loss 0.0814  dot 0.0697
  tail_bwd   dz 0.1998  grad_bias 0.0618
  autoenc    act = none, tier 1: the three sums 0.0000 (the device's sums were the exact ones), everything else bit for bit
             none     H 0.0664  D 0.2901  dZ 0.2064  dcn 0.0810  dz 0.2946  dW 0.1996  db 0.1363  scal[0] 0.3612  loss 0.0049
             tanh     H 0.0913  D 0.1977  dZ 0.2124  dcn 0.0695  dz 0.3718  dW 0.2042  db 0.1790  scal[0] 0.3863  loss 0.0106
             sigmoid  H 0.1064  D 0.1939  dZ 0.2177  dcn 0.0634  dz 0.3977  dW 0.1975  db 0.2021  scal[0] 0.3682  loss 0.0098

G / GF next to 0.5 are elements whose error is the last rounding alone (half an ulp, charged a whole one); gM varies from run to
run with the order of the split-K atomics (0.23 to 0.26 seen).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tail_cases as tc
from rows_cases import SENTINEL, TAG

pytestmark = pytest.mark.gpu
f32 = np.float32
S = tc.SLOTS


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return None if t is None else t.cpu().numpy()


def addr(t):
    return None if t is None else t.data_ptr()


def nan_buffer(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


def all_nan(t):
    return bool(torch.isnan(t).all())


def report(kernel, ratios, c):
    for name, r in ratios.items():
        print(f"RATIO {kernel}:{name.rstrip('0123456789')} {r:.4f} {c.id}")


# ----------------------------------------------------------------------------------------------------- A. the space-mapping step
class MapRun:
    """The buffers of one case on the device and the argument struct over them."""

    def __init__(self, c, o):
        from multike_amd import _lib
        self.c, self.o = c, o
        d, n = c.d, c.n
        assert _lib.mapping_scratch_floats(n, d) == tc.mapping_scratch_floats(n, d)
        self.floats = tc.mapping_scratch_floats(n, d)
        self.ent, self.views = dev(o.ent), [dev(v) for v in o.views]
        self.M, self.gM, self.idx = dev(o.M), dev(o.gM0), dev(o.idx)
        self.grad, self.touched = dev(o.grad0), dev(o.touched0)
        self.scratch = nan_buffer(self.floats + 64, torch.float32)
        self.partials = nan_buffer(2 * tc.MAX_VIEWS * S + 16, torch.float64)
        self.loss = nan_buffer((tc.MAX_VIEWS + 1) * S + 16, torch.float64)
        a = _lib.MappingStepArgs()
        a.ent_table, a.n_ent, a.ent_normalize = addr(self.ent), o.n_ent, c.ent_norm
        a.ent_grad, a.ent_touched = addr(self.grad), addr(self.touched)
        for k, nz in enumerate(c.views):
            a.views[k].table, a.views[k].normalize = addr(self.views[k]), nz
        a.n_views, a.stride, a.dim, a.idx, a.n = len(c.views), c.stride, d, addr(self.idx) if n else None, n
        a.M, a.gM, a.orthogonal_weight, a.norm_w = addr(self.M), addr(self.gM), tc.ORTHO_W, tc.NORM_W
        a.scratch, a.partials = addr(self.scratch), addr(self.partials)
        a.optimizer, a.lr, a.tag, a.update = _lib.OPT_SGD, tc.MAP_LR, TAG, 0
        self.args = a

    def phase(self, mask):
        from multike_amd import _lib
        code = _lib.lib().mke_mapping_step_phases(C.byref(self.args), C.c_void_p(addr(self.loss)), C.c_int(mask), _lib._stream())
        torch.cuda.synchronize()
        return code

    def region(self, name):
        o = tc.mapping_layout(self.c.n, self.c.d)[name]
        return self.scratch[o:o + self.c.total]

    def read(self, name):
        return host(self.region(name)).reshape(self.c.n, self.c.d)

    def block(self, buf, i):
        return buf[i * S:(i + 1) * S]

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("scratch", "partials", "loss", "gM", "grad", "touched", "ent", "M")}

    def unchanged(self, snap, *names):
        return [k for k in names if not torch.equal(getattr(self, k).view(torch.uint8), snap[k].view(torch.uint8))]


def plant(run, what, k, own):
    arr, total = tc.map_plant(run.c, own, what)
    if arr is not None:
        run.block(run.partials, 2 * k + (what == "T"))[:] = dev(arr)
    return total


def run_map(c):
    from multike_amd import _lib
    o = tc.map_ops(c)
    r = MapRun(c, o)
    nv, d = len(c.views), c.d
    got = {"V": [], "P": [], "ssq": [], "S": [], "G": [], "lossp": [], "dotp": [], "T": [], "dP": []}

    snap = r.snapshot()
    assert r.phase(tc.MAP_FWD) == 0, _lib.lib().mke_last_error()
    got["F"] = r.read("F")
    for k in range(nv):
        got["V"].append(r.read(f"V{k}")), got["P"].append(r.read(f"P{k}"))
        got["ssq"].append(host(r.block(r.partials, 2 * k)))
        assert all_nan(r.region(f"G{k}")) and all_nan(r.block(r.partials, 2 * k + 1)), c.id
    for k in range(nv, tc.MAX_VIEWS):
        assert all(all_nan(r.region(f"{x}{k}")) for x in "VPG") and all_nan(r.block(r.partials, 2 * k)) and all_nan(r.block(r.partials, 2 * k + 1)), c.id
    assert all_nan(r.region("GF")) and all_nan(r.scratch[r.floats:]) and all_nan(r.partials[6 * S:]), c.id
    assert not r.unchanged(snap, "loss", "gM", "grad", "touched", "ent", "M"), c.id

    for k in range(nv):
        got["S"].append(plant(r, "S", k, float(got["ssq"][k].sum())))
    snap = r.snapshot()
    assert r.phase(tc.MAP_TAIL) == 0, _lib.lib().mke_last_error()
    got["GF"] = r.read("GF")
    for k in range(nv):
        got["G"].append(r.read(f"G{k}"))
        got["lossp"].append(host(r.block(r.loss, k))), got["dotp"].append(host(r.block(r.partials, 2 * k + 1)))
        assert torch.equal(r.region(f"V{k}"), snap["scratch"][tc.mapping_layout(c.n, d)[f"V{k}"]:][:c.total]), c.id
        assert torch.equal(r.block(r.partials, 2 * k).view(torch.int64), r.block(snap["partials"], 2 * k).view(torch.int64)), c.id
    for k in range(nv, tc.MAX_VIEWS):                                # the loss blocks of the views that are not there: zeros
        assert not r.block(r.loss, k).any() and all_nan(r.region(f"G{k}")) and all_nan(r.block(r.partials, 2 * k + 1)), c.id
    assert all_nan(r.block(r.loss, tc.MAX_VIEWS)) and all_nan(r.loss[4 * S:]) and all_nan(r.scratch[r.floats:]), c.id
    assert not r.unchanged(snap, "gM", "grad", "touched", "ent", "M"), c.id

    for k in range(nv):
        got["T"].append(plant(r, "T", k, float(got["dotp"][k].sum())))
    snap = r.snapshot()
    assert r.phase(tc.MAP_BWD) == 0, _lib.lib().mke_last_error()
    for k in range(nv):
        got["dP"].append(r.read(f"G{k}"))
    got["gM"] = host(r.gM)
    assert not r.unchanged(snap, "partials", "loss", "grad", "touched", "ent", "M"), c.id
    assert torch.equal(r.region("GF"), snap["scratch"][c.total:2 * c.total]) and all_nan(r.scratch[r.floats:]), c.id

    r.region("GF")[:] = dev(o.GF.ravel())                          # dyadic operands for the exact phase
    r.gM[:] = dev(o.gM0)
    snap = r.snapshot()
    assert r.phase(tc.MAP_UPD) == 0, _lib.lib().mke_last_error()
    got["gM_upd"], got["ortho"] = host(r.gM), host(r.block(r.loss, tc.MAX_VIEWS))
    got["grad"], got["touched"] = host(r.grad), host(r.touched)
    assert not r.unchanged(snap, "scratch", "partials", "ent", "M"), c.id
    assert torch.equal(r.loss[:3 * S].view(torch.int64), snap["loss"][:3 * S].view(torch.int64)) and all_nan(r.loss[4 * S:]), c.id

    problems, ratios = tc.check_map(c, o, got)
    report("mapping", ratios, c)
    assert not problems, (c.id, problems)

    if c.sgd:                                                        # the same phase with the SGD update behind it
        r.gM[:], r.grad[:], r.touched[:] = dev(o.gM0), dev(o.grad0), dev(o.touched0)
        r.args.update = 1
        assert r.phase(tc.MAP_UPD) == 0, _lib.lib().mke_last_error()
        want = tc.sgd_reference(o, c, got["gM_upd"], got["grad"], got["touched"])
        for name, g, w in zip(("M", "gM", "ent", "grad"), (r.M, r.gM, r.ent, r.grad), want):
            assert tc.same_bits(host(g), w), (c.id, "sgd", name)
        assert np.array_equal(host(r.touched), got["touched"]), c.id


@pytest.mark.parametrize("c", tc.MAP_CASES, ids=lambda c: c.id)
def test_mapping_phases(c):
    run_map(c)


@pytest.mark.parametrize("mask", (tc.MAP_FWD, tc.MAP_TAIL, tc.MAP_BWD, tc.MAP_UPD, tc.MAP_ALL), ids=("fwd", "tail", "bwd", "upd", "all"))
def test_mapping_empty_part(mask):
    """n = 0 (idx NULL): a part contributes zeros to the sums it owns and touches nothing else; UPD still adds the
    orthogonality / norm terms, the whole step in one call moves nothing and reports a zero loss."""
    from multike_amd import _lib
    c = tc.MCase(17, 0, (0, 1))
    o = tc.map_ops(c)
    r = MapRun(c, o)
    snap = r.snapshot()
    assert r.phase(mask) == 0, _lib.lib().mke_last_error()
    nv = len(c.views)
    want_p, want_l = snap["partials"].clone(), snap["loss"].clone()
    if mask == tc.MAP_ALL:
        want_l[:4 * S] = 0
    if mask == tc.MAP_FWD:
        for k in range(nv):
            r.block(want_p, 2 * k)[:] = 0
    if mask == tc.MAP_TAIL:
        for k in range(nv):
            r.block(want_p, 2 * k + 1)[:] = 0
        want_l[:3 * S] = 0
    gM = o.gM0.copy()
    if mask == tc.MAP_UPD:
        M = o.M[:3 * 17 * 17].astype(np.float64).reshape(3, 17, 17)
        tot = np.zeros(S)
        for k in range(nv):
            blk = slice(k * 289, (k + 1) * 289)
            g, tot[k] = tc.ortho_reference(M[k], o.gM0[blk], 17)
            gM[blk] = g.astype(f32).ravel()
        r.block(want_l, 3)[:] = dev(tot)
    assert tc.same_bits(host(r.partials), host(want_p)) and tc.same_bits(host(r.loss), host(want_l))
    assert tc.same_bits(host(r.gM), gM)
    assert not r.unchanged(snap, "scratch", "grad", "touched", "ent", "M")


def test_mapping_refuses_dim_89():
    """One past MKE_MAP_MAX_DIM: MKE_E_SHAPE in every phase mask, nothing written."""
    c = tc.MCase(89, 17, (0,))
    r = MapRun(c, tc.map_ops(c))
    snap = r.snapshot()
    for mask in (tc.MAP_FWD, tc.MAP_TAIL, tc.MAP_BWD, tc.MAP_UPD, tc.MAP_ALL):
        assert r.phase(mask) == tc.E_SHAPE
    assert not r.unchanged(snap, *snap)


# ----------------------------------------------------------------------------------------------------- B. the attribute tail
@pytest.mark.parametrize("c", tc.Z_CASES, ids=lambda c: c.id)
def test_attr_tail_z(c):
    from multike_amd import _lib
    z0, bias = tc.tailz_ops(c)
    z, b, part = dev(z0), dev(bias), nan_buffer(S + 16, torch.float64)
    code = _lib.lib().mke_attr_tail_z(C.c_void_p(addr(z)), C.c_void_p(addr(b)), C.c_int64(c.n), C.c_int(c.dim), C.c_void_p(addr(part)), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    problems, ratios = tc.check_tailz(c, z0, bias, host(z), host(part[:S]))
    report("tail_z", ratios, c)
    assert not problems and all_nan(part[S:]), (c.id, problems)


@pytest.mark.parametrize("c", tc.B_CASES, ids=lambda c: c.id)
def test_attr_tail_bwd(c):
    from multike_amd import _lib
    z0, g0, sp, tp, gb0 = tc.tailbwd_ops(c)
    z, g, s, t, gb = dev(z0), dev(g0), dev(sp), dev(tp), dev(gb0)
    code = _lib.lib().mke_attr_tail_bwd(C.c_void_p(addr(z)), C.c_void_p(addr(g)), C.c_void_p(addr(s)), C.c_void_p(addr(t)), C.c_int64(c.n),
                                        C.c_int(c.dim), C.c_void_p(addr(gb)), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    problems, ratios = tc.check_tailbwd(c, host(g), host(gb))
    report("tail_bwd", ratios, c)
    assert not problems, (c.id, problems)
    assert tc.same_bits(host(z), z0) and tc.same_bits(host(s), sp) and tc.same_bits(host(t), tp), c.id       # read-only operands


def run_tail_loss(c):
    from multike_amd import _lib
    o = tc.tailloss_ops(c)
    n, dim = c.n, c.dim
    z, ent, ih, ws, ssq = dev(o.z), dev(o.ent), dev(o.ih), dev(o.ws), dev(o.sumsq)
    gout = torch.full((n * dim + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    lossp, dotp = nan_buffer(S + 16, torch.float64), nan_buffer(S + 16, torch.float64)
    gent, touched = dev(o.gent0), (dev(o.touched0) if c.grad_ent else None)
    p = C.c_void_p
    code = _lib.lib().mke_attr_tail_loss(p(addr(z)), p(addr(ssq)), p(addr(ent)), C.c_int(c.stride), C.c_int(c.ent_norm), p(addr(ih) if n else None),
                                         p(addr(ws)), C.c_float(c.scale), C.c_int64(n), C.c_int(dim), p(addr(gout)), p(addr(dotp)), p(addr(gent)),
                                         p(addr(touched)), C.c_int32(TAG), p(addr(lossp)), _lib._stream())
    assert code == 0, _lib.lib().mke_last_error()
    got = {"gout": host(gout), "lossp": host(lossp[:S]), "dotp": host(dotp[:S]), "gent": host(gent), "touched": host(touched)}
    problems, ratios = tc.check_tailloss(c, o, got)
    report("tail_loss", ratios, c)
    assert not problems and all_nan(lossp[S:]) and all_nan(dotp[S:]), (c.id, problems)
    assert tc.same_bits(host(z), o.z) and tc.same_bits(host(ent), o.ent) and tc.same_bits(host(ssq), o.sumsq), c.id


@pytest.mark.parametrize("c", tc.L_CASES, ids=lambda c: c.id)
def test_attr_tail_loss(c):
    """Every width, dim and row count; weights, grad_ent, the table's normalisation, scale and the planted form alternate."""
    run_tail_loss(c)


# ----------------------------------------------------------------------------------------------------- B. through mke_attr_step_phases
def _grad_close(got, ref, what):
    """The tolerance of test_attr_conv_widths_gpu.py."""
    np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=what)


@pytest.mark.parametrize("form", ("total", "split"))
@pytest.mark.parametrize("floor", (0, 1), ids=("live", "floor"))
@pytest.mark.parametrize("fused", (1, 0), ids=("fused", "unfused"))
@pytest.mark.parametrize("dim,n", tc.STEP_SHAPES)
def test_attr_step_planted_backward(dim, n, fused, floor, form):
    """FWD | TAIL on NaN-poisoned scratch and partials: with the fused backward on, the first 4 dim^2 floats of the dflat scratch
    are W^T bit for bit (else the tail leaves them alone).  Then the sharded contract: (S, T) planted in the step's two partial
    arrays, as [total, 0, ...] or split between slots 0 and 2047, above the epsilon floor or below it; BWD alone must give the
    parameter and attribute gradients of oracle.conv_backward for dflat = dz W^T, dz formed in float64 from the planted
    scalars and the device's own z and g."""
    from multike_amd import _lib
    from multike_amd.attr_cnn import AttrCNN
    from multike_amd.tables import EmbeddingTable, StepEngine
    from oracle import attr_cnn_oracle as ao
    from oracle import multike_oracle as mo
    rng = np.random.default_rng(1000 * dim + n)
    n_ent, n_attr, n_lit = 23, 9, 50
    P = ao.init_params(dim, rng)
    P["gamma"], P["beta"] = 1.0 + 0.1 * rng.standard_normal(dim), 0.05 * rng.standard_normal(dim)
    P["b1"], P["b2"] = 0.05 * rng.standard_normal(2), 0.5 + 0.05 * rng.standard_normal(2)       # see test_attr_conv_widths_gpu._case
    P["bias"] = 0.1 * rng.standard_normal(dim)
    P = {k: v.astype(f32) for k, v in P.items()}
    e0 = rng.standard_normal((n_ent, dim)).astype(f32)
    a0 = (0.3 * rng.standard_normal((n_attr, dim))).astype(f32)
    l0 = mo.l2_normalize_rows(rng.standard_normal((n_lit, dim))).astype(f32)
    ih, ia, iv = (rng.integers(0, m, n).astype(np.int32) for m in (n_ent, n_attr, n_lit))
    ws = rng.random(n).astype(f32)
    ent = EmbeddingTable(n_ent, dim, "e", values=e0)
    attr = EmbeddingTable(n_attr, dim, "a", normalize=False, values=a0)
    lit = EmbeddingTable(n_lit, dim, "l", normalize=False, trainable=False, values=l0)
    cnn, eng = AttrCNN(dim, params=P), StepEngine()
    ids = [dev(x) for x in (ih, ia, iv, ws)]                      # the argument struct holds raw pointers: these stay alive to the end
    args, part = cnn._args(eng, ent, attr, lit, *ids, n, 0.5, "o", 0.01, "SGD", False, 1)
    assert cnn._scratch.numel() == tc.attr_scratch_floats(n, dim) == _lib.attr_scratch_floats(n, dim)
    cnn._scratch.fill_(float("nan"))
    part.fill_(float("nan"))
    lay = tc.attr_layout(n, dim)

    def region(name):
        off, rows, ld = lay[name]
        return cnn._scratch[off:off + rows * ld].view(rows, ld)

    old = _lib.set_option("attr_fused_bwd", fused)
    try:
        _lib.attr_step_phases(args, _lib.ATTR_FWD | _lib.ATTR_TAIL)
        torch.cuda.synchronize()
        p = host(part).reshape(3, S)
        assert np.isfinite(p).all(), "a partial slot kept its poison"
        wt = region("dflat").reshape(-1)[:4 * dim * dim]
        if tc.fused_tail(n, dim, fused):
            assert not tc.check_wt(host(wt), P["W"]), "W^T in the dflat scratch"
            assert all_nan(region("dflat").reshape(-1)[4 * dim * dim:])
        else:
            assert all_nan(region("dflat"))
        z, g = host(region("z")), host(region("gout"))
        assert np.isfinite(z).all() and np.isfinite(g).all()
        S_own, T_own = float(p[1].sum()), float(p[2].sum())
        np.testing.assert_allclose(S_own, float((z.astype(np.float64) ** 2).sum()), rtol=1e-5)
        S_planted = tc.S_FLOOR_PLANTED if floor else 2.0 * S_own
        T_planted = 0.5 * T_own + 0.25
        part[S:2 * S] = dev(tc.planted(S_planted, form))
        part[2 * S:] = dev(tc.planted(T_planted, form))
        _lib.attr_step_phases(args, _lib.ATTR_BWD)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("attr_fused_bwd", old)
    assert tc.same_bits(host(part[S:]).reshape(2, S), np.stack([tc.planted(S_planted, form), tc.planted(T_planted, form)])), "BWD wrote the partials"
    p64 = {k: v.astype(np.float64) for k, v in P.items()}
    _, c = ao.forward(p64, np.zeros((n, dim)), a0.astype(np.float64)[ia], l0.astype(np.float64)[iv])
    dz = tc.dz_reference(z, g, S_planted, T_planted)
    ref = ao.conv_backward(p64, c, dz @ p64["W"].T)
    ref["W"], ref["bias"] = c["flat"].T @ dz, dz.sum(0)
    g_attr = np.zeros((n_attr, dim))
    np.add.at(g_attr, ia, ref.pop("as"))
    for k in ao.PARAM_NAMES:
        _grad_close(host(cnn.gviews[k]), ref[k], f"{k} dim={dim} n={n}")
    _grad_close(host(attr.grad[:, :dim]), g_attr, f"grad_attr dim={dim} n={n}")
    del ids


# ----------------------------------------------------------------------------------------------------- C. the literal auto-encoder
def run_ae(c):
    """mke_ae_step_phases with update = 0, ENC | DEC | BWD one at a time on a NaN-poisoned scratch; the totals of sum code^2 and
    sum dcn . code are planted between the phases the way the data-parallel trainer leaves them."""
    from multike_amd import _lib
    o = tc.ae_ops(c)
    n, d, M = c.n, c.dims, c.rows
    w_off, b_off, total, _ = tc.ae_offsets(d)
    x, params = dev(o.x), dev(o.params)
    grads = torch.cat([torch.zeros(total, dtype=torch.float32, device="cuda"), torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")])
    partials = torch.zeros(3 * S, dtype=torch.float64, device="cuda")
    scal, loss = nan_buffer(4, torch.float32), nan_buffer(1, torch.float64)
    p = _lib.AEPlanStruct()
    p.n_layers, p.act, p.normalize = n, tc.ACT_CODE[c.act], c.normalize
    assert (_lib.ACT_NONE, _lib.ACT_TANH, _lib.ACT_SIGMOID) == (0, 1, 2)
    for i, w in enumerate(d):
        p.dims[i] = w
    for k in range(2 * n):
        p.w_off[k], p.b_off[k] = w_off[k], b_off[k]
    p.params, p.grads, p.acc, p.n_params = addr(params), addr(grads), None, total
    p.optimizer, p.lr, p.update = _lib.OPT_SGD, 0.25, 0
    floats = _lib.ae_scratch_floats(p, M)
    assert floats == tc.ae_scratch_floats(d, M)
    base = nan_buffer(floats + 8, torch.float32)
    assert base.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and params.data_ptr() % 16 == 0
    scratch = base[c.shift:c.shift + floats]
    p.scratch, p.scratch_floats, p.partials, p.scalars = scratch.data_ptr(), floats, addr(partials), addr(scal)
    lay = tc.ae_layout(d, M)

    def read(name, width):
        off, ld = lay[name]
        return host(scratch[off:off + M * ld].view(M, ld)[:, :width])

    def phase(mask):
        code = _lib.lib().mke_ae_step_phases(C.byref(p), C.c_void_p(addr(x)), C.c_int64(M), C.c_int64(c.ldx), C.c_int64(c.global_rows), C.c_int(mask),
                                             C.c_void_p(addr(loss)), _lib._stream())
        assert code == 0, _lib.lib().mke_last_error()
        torch.cuda.synchronize()

    got = {}
    phase(tc.AE_ENC)
    got["H"] = [read(f"H{i}", d[i]) for i in range(1, n + 1)]
    part = host(partials).reshape(3, S)
    assert np.isfinite(part).all() and not part[1:].any(), c.id
    got["ssq_own"] = float(part[0].sum())
    if c.normalize:
        partials[:S] = dev(tc.planted(o.S, c.form))
    phase(tc.AE_DEC)
    got["D"] = [read(f"D{j}", d[n - j]) for j in range(1, n)]
    got["dZ"], got["dcn"], got["loss"] = read(f"D{n}", d[0]), read("dcn", d[n]), float(host(loss)[0])
    part = host(partials).reshape(3, S).copy()
    got["dot_own"] = float(part[1].sum())
    part[1] = 0
    got["partials_after_dec"] = part
    got["grads_dec"] = host(grads[:total])
    sc = host(scal)
    got["scal_dec"] = (sc[0], sc[1]) if c.normalize else None
    assert np.isnan(sc[2:]).all() and (c.normalize or np.isnan(sc).all()), c.id
    if c.normalize:
        partials[S:2 * S] = dev(tc.planted(o.D, c.form))
    phase(tc.AE_BWD)
    got["dzc"], got["grads"] = read("dz", d[n]), host(grads[:total])
    got["scal_bwd"] = host(scal)[2] if c.normalize else None
    got["partials_after_bwd"] = host(partials).reshape(3, S)
    problems, ratios = (tc.check_ae2 if c.tier2 else tc.check_ae)(c, o, got)
    report("autoenc" + ("-" + c.act if c.tier2 else ""), ratios, c)
    assert not problems, (c.id, problems)
    assert (host(grads[total:]) == f32(SENTINEL)).all() and tc.same_bits(host(params), o.params) and tc.same_bits(host(x), o.x), c.id
    assert all_nan(base[:c.shift]) and all_nan(base[c.shift + lay["end"][0]:]), c.id          # nothing outside the carve-up


@pytest.mark.parametrize("c", tc.A_CASES, ids=lambda c: c.id)
def test_autoencoder_phases(c):
    run_ae(c)

"""The GEMM paths that only internal callers reach, at the sizes where the host dispatchers switch kernels, each against
the float64 oracle of its caller at the tolerances the neighbouring tests use:

  space-mapping step    k_gemm_tall<5, 5> (P = V M, 1024 <= rows <= 32768, dim <= 80) and its fall-back k_gemm_f32 with per-block
                        partials on either side of every limit
  attribute step        k_gemm_tallsplit_plus with 1..16 K splits (unfused backward), and the forward past the fused launch's
                        row limit (k_gemm_f32 with per-block partials)
  dense_layer_fwd       bias + activation epilogue of launch_gemm_f32_ex on padded, NaN-poisoned operands, both kernels
  ae_encode             the same epilogue chained through the scratch, ragged widths
"""
import numpy as np
import pytest
import torch

import gemm_cases as gc
from oracle import attr_cnn_oracle as ao
from oracle import literal_oracle as lo
from oracle import multike_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d,B", [(75, 5000),                          # the production shape
                                 (75, 1023), (75, 1024), (75, 1025),  # the M >= 1024 switch
                                 (80, 1040), (81, 1040),              # widest tall width, first width past it
                                 (16, 2050),                          # one column tile; M not a multiple of 16
                                 (5, 1100),
                                 (75, 32768), (75, 32769)])           # last tall grid; first fall-back to per-block partials
def test_mapping_step_at_the_tall_kernel_limits(d, B):
    """test_mapping_gpu.py's three native steps against mo.space_mapping_step_dense, same tolerances."""
    from test_mapping_gpu import test_native_steps_match_oracle as native_steps_match_oracle
    native_steps_match_oracle(d, B + 300, B, False)


UNFUSED = [(75, 5000, 20000, 300, 8000),   # 16 K splits, the last one ragged (200 of 320)
           (32, 513, 900, 20, 400),        # 2 splits, the second 193 wide
           (80, 1029, 2000, 30, 600),      # widest; 4 splits, the last 69 wide
           (8, 700, 500, 9, 200),          # one column tile; 3 splits
           (40, 640, 900, 13, 300)]        # 2 splits, both full
PAST_SPLIT = [(81, 1029, 2000, 30, 600), (96, 700, 900, 9, 300)]   # N0 > 80: both products on k_gemm_f32_batch, 32 K splits


def _unfused(fn, *a):
    from multike_amd import _lib
    old = _lib.set_option("attr_fused_bwd", 0)
    try:
        assert _lib.get_option("attr_fused_bwd") == 0
        fn(*a)
    finally:
        _lib.set_option("attr_fused_bwd", old)


@pytest.mark.parametrize("d,B,n_ent,n_attr,n_lit", UNFUSED + PAST_SPLIT)
def test_attr_three_steps_unfused_backward(d, B, n_ent, n_attr, n_lit):
    """test_attr_cnn_gpu.py's three full steps against the dense oracle with the fused backward switched off: the weight
    gradient runs on k_gemm_tallsplit_plus (K = B split in slices of 320) and dflat on its 64 x 64 blocks; past dim 80 the
    pair runs on k_gemm_f32_batch."""
    from test_attr_cnn_gpu import test_three_steps_vs_oracle as three_steps_vs_oracle
    _unfused(three_steps_vs_oracle, d, B, n_ent, n_attr, n_lit)


def _one_step_loss_and_gradients(d, B, n_ent, n_attr, n_lit):
    """One step without update: loss in the band of test_three_steps_vs_oracle, every parameter gradient in the band of
    test_golden_loss_and_every_gradient."""
    from multike_amd.attr_cnn import AttrCNN
    from multike_amd.tables import EmbeddingTable, StepEngine
    rng = np.random.default_rng(d + B)
    P = ao.init_params(d, rng)
    P["bias"] = 0.05 * rng.standard_normal(d)
    P["b1"] = 0.05 * rng.standard_normal(2)
    ent = mo.xavier_truncated_normal((n_ent, d), rng)
    attr = mo.xavier_truncated_normal((n_attr, d), rng)
    lit = rng.standard_normal((n_lit, d)).astype(np.float32)
    lit /= np.linalg.norm(lit, axis=1, keepdims=True)
    E = EmbeddingTable(n_ent, d, "av_ent", normalize=True, values=ent)
    A = EmbeddingTable(n_attr, d, "attr", normalize=False, values=attr)
    L = EmbeddingTable(n_lit, d, "lit", normalize=False, trainable=False, values=lit)
    cnn = AttrCNN(d, params=P)
    p64 = {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}
    ih, ia, iv = rng.integers(0, n_ent, B), rng.integers(0, n_attr, B), rng.integers(0, n_lit, B)
    ws = rng.uniform(0.2, 1.0, B).astype(np.float32)
    Lo, g = ao.loss_and_grads(p64, mo.l2_normalize_rows(ent.astype(np.float64))[ih], attr.astype(np.float64)[ia],
                              lit.astype(np.float64)[iv], ws.astype(np.float64), 2.0)
    t = lambda x: torch.as_tensor(x.astype(np.int32), device="cuda")
    lp = cnn.step(StepEngine(), E, A, L, t(ih), t(ia), t(iv), torch.as_tensor(ws, device="cuda"), scale=2.0, update=False)
    np.testing.assert_allclose(float(lp.sum()), Lo, rtol=1e-5)
    for k in ao.PARAM_NAMES:
        np.testing.assert_allclose(cnn.gviews[k].cpu().numpy(), g[k], rtol=2e-3, atol=2e-5 * max(1.0, np.abs(g[k]).max()), err_msg=k)


@pytest.mark.parametrize("d,B,n_ent,n_attr,n_lit", UNFUSED + PAST_SPLIT)
def test_attr_gradients_unfused_backward(d, B, n_ent, n_attr, n_lit):
    """The same launches held at the gradients themselves ([dW; dbias] is what the K-split product writes): three Adagrad
    steps divide a gradient by its own magnitude and forgive a split that drops a few of its rows."""
    _unfused(_one_step_loss_and_gradients, d, B, n_ent, n_attr, n_lit)


def test_attr_step_past_the_fused_forward_limit():
    """B = 32784 rows (> 16 * 2048): the forward leaves the fused conv + dense launch for the separate convolution and
    k_gemm_f32 with per-block partials."""
    _one_step_loss_and_gradients(32, 32784, 40000, 200, 9000)


# --- mke_dense_layer_fwd -------------------------------------------------------------------------------------------------
ACT = {"none": 0, "tanh": 1, "sigmoid": 2}
ACT64 = {"none": lambda p: p, "tanh": np.tanh, "sigmoid": lambda p: 1.0 / (1.0 + np.exp(-p))}
ACT32 = {"tanh": torch.tanh, "sigmoid": torch.sigmoid}
DENSE_SHAPES = [(50, 301, 75), (129, 75, 33), (1, 5, 1), (65, 63, 130), (64, 150, 70)]


def _bias_tensor(b, how):
    """None, a 16-byte aligned device vector, or one that starts 4 bytes past an aligned address (NaN around it)."""
    if how == "none":
        return None
    buf = torch.full((b.size + 8,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    o = 1 if how == "odd" else 4
    buf[o:o + b.size] = torch.as_tensor(b, device="cuda")
    return buf[o:o + b.size]


def _dense_layer(x, w, b, act, vec, bias, extra):
    """mke_dense_layer_fwd on x, w, out embedded in NaN / sentinel buffers (x one float off its aligned base for the dword
    kernel); returns the [M, N] result after checking that nothing else of out's buffer was written."""
    from multike_amd import _lib
    (M, K), N = x.shape, w.shape[1]
    lx, lw, lo_ = gc.Lay("pad", False, extra, 0 if vec else 1), gc.Lay("pad", False, (extra + 4) % 12), gc.Lay("pad", False, (extra + 8) % 12)
    xbuf, px = gc.embed(x, lx)
    wbuf, pw = gc.embed(w, lw)
    obuf, po = gc.embed(np.full((M, N), gc.SENTINEL, np.float32), lo_, gc.SENTINEL)
    assert gc.takes_vec_kernel(M, N, K, px, pw) == vec
    dev = lambda a: torch.as_tensor(a, device="cuda")
    xbuf, wbuf, obuf = dev(xbuf), dev(wbuf), dev(obuf)
    out = gc.view(obuf, M, N, po)
    _lib.dense_layer_fwd(gc.view(xbuf, M, K, px), gc.view(wbuf, K, N, pw), _bias_tensor(b, bias), ACT[act], out)
    res = out.clone()
    out.fill_(gc.SENTINEL)
    assert bool((obuf == gc.SENTINEL).all()), "out was written outside [M, N]"
    assert not bool(torch.isnan(res).any()), "poison reached the result"
    return res


@pytest.mark.parametrize("bias", ["none", "aligned", "odd"])
@pytest.mark.parametrize("vec", [True, False], ids=["vec", "dword"])
def test_dense_layer_fwd_plain_is_exact(vec, bias):
    """act = none on integer operands and an integer bias: the result equals the float64 one."""
    for i, (M, K, N) in enumerate(DENSE_SHAPES):
        c = gc.make_case("dense", M, N, K, gc.Lay(), gc.Lay())
        x, w, c0 = gc.operands(c)
        b = c0[0]                                                          # integers in [-C_MAX, C_MAX]
        ref = gc.reference(x, w) + (b.astype(np.float64) if bias != "none" else 0.0)
        got = _dense_layer(x, w, b, "none", vec, bias, (0, 4, 8)[i % 3])
        assert torch.equal(got, torch.as_tensor(ref.astype(np.float32), device="cuda")), (M, K, N)


@pytest.mark.parametrize("bias", ["none", "aligned", "odd"])
@pytest.mark.parametrize("act", ["tanh", "sigmoid"])
@pytest.mark.parametrize("vec", [True, False], ids=["vec", "dword"])
def test_dense_layer_fwd_activation(vec, act, bias):
    """Dyadic operands (gemm_cases.dyadic_operands): the pre-activation is exact in float32, so the only error left is the
    activation function's own.  Bound: 4 x the max error of torch's CPU float32 tanh / sigmoid against float64 on the same
    pre-activations (computed here; ~3e-8 / ~8.5e-8, i.e. a bound of ~1.2e-7 / ~3.4e-7) — room for a device libm of a few ulp
    against the CPU's <= 1 ulp, while a swapped activation or a dropped bias is off by more than 1e-2."""
    for i, (M, K, N) in enumerate(DENSE_SHAPES):
        x, w, b = gc.dyadic_operands(M, K, N, i)
        p64 = x.astype(np.float64) @ w.astype(np.float64) + (b.astype(np.float64) if bias != "none" else 0.0)
        p32 = p64.astype(np.float32)
        assert np.array_equal(p32.astype(np.float64), p64)
        ref = ACT64[act](p64)
        cpu_err = float(np.abs(ACT32[act](torch.as_tensor(p32)).double().numpy() - ref).max())
        got = _dense_layer(x, w, b, act, vec, bias, (0, 4, 8)[i % 3])
        err = float(np.abs(got.double().cpu().numpy() - ref).max())
        print(f"dense_layer_fwd {act} {'vec' if vec else 'dword'} bias={bias} {M}x{K}x{N}: device max err {err:.3e}, "
              f"cpu float32 max err {cpu_err:.3e}, bound {4 * cpu_err:.3e}")
        assert err <= 4 * cpu_err, (M, K, N, err, cpu_err)


# --- mke_ae_encode -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,L,active,pad_x,pad_out", [([128, 64, 32, 16], 256, "sigmoid", 0, 0),    # every product on the 16-byte path
                                                         ([150, 70, 33, 9], 77, "tanh", 0, 0),         # ragged: dword first layer, then 16-byte loads with K % 4 != 0
                                                         ([150, 70, 33, 9], 130, "tanh", 6, 7),        # padded x / out rows: 16-byte loads throughout
                                                         ([150, 70, 33, 9], 63, "thah", 10, 3)])       # no activation
def test_ae_encode_vs_oracle(dims, L, active, pad_x, pad_out):
    """mke_ae_encode against lo.encode at test_literal_gpu.py's rtol / atol, with NaN in every place the encoder may load
    from but must not use: x's row padding, the pad entries of the packed parameters, the whole scratch (whose row padding
    the inner layers' 16-byte loads straddle)."""
    from multike_amd import _lib
    from multike_amd.literal_encoder import AutoEncoderModel
    from multike_amd.synthetic import synthetic_args
    rng = np.random.default_rng(len(dims) * 1000 + L)
    n = len(dims) - 1
    x = rng.standard_normal((L, dims[0])).astype(np.float32)
    args = synthetic_args(dim=dims[-1], batch_size=L, learning_rate=0.05, encoder_active=active, encoder_normalize=False, encoder_epoch=1)
    m = AutoEncoderModel(x, args, input_dimension=dims[0], hidden_dimensions=dims[1:])
    p = {k: (0.4 * v).astype(np.float32) for k, v in lo.init_params(dims, rng).items()}
    m.params.fill_(float("nan"))
    m.set_params(p)
    m._ensure_scratch(L)
    m._scratch.fill_(float("nan"))
    ldx, ld_out = dims[0] + pad_x, dims[-1] + pad_out
    xbuf = torch.full((L, ldx), float("nan"), device="cuda")
    xbuf[:, :dims[0]] = torch.as_tensor(x, device="cuda")
    obuf = torch.full((L, ld_out), gc.SENTINEL, device="cuda")
    _lib.ae_encode(m._plan, xbuf, obuf)            # contiguous [L, ld] buffers: the logical widths are the plan's
    enc = obuf[:, :dims[-1]].double().cpu().numpy()
    assert bool((obuf[:, dims[-1]:] == gc.SENTINEL).all())
    want = lo.encode({k: v.astype(np.float64) for k, v in p.items()}, x.astype(np.float64), n, active)
    assert np.all(np.isfinite(enc))
    np.testing.assert_allclose(enc, want, rtol=5e-3, atol=5e-4)

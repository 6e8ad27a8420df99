"""tail_cases.py without a device: the kernel-by-kernel references compose to the existing float64 oracles, every bit-for-bit
claim is proved by Bound.check(), the float32 and contracted-fma emulations stay within half of every derived bound, the
scratch layout and grids are the ones the sources state, and every mutant fails the device test's own comparison."""
import numpy as np
import pytest

import tail_cases as tc
from oracle import multike_oracle as mo
from update_cases import L2_EPS32, Arith

f64 = np.float64


def worst(ratios):
    return max(ratios.values(), default=0.0)


# ----------------------------------------------------------------------------------------------------- A. the space-mapping step
def test_case_table_covers_the_issue():
    cs = tc.MAP_CASES
    plain = [c for c in cs if not c.floor and not c.sgd]
    assert {(c.d, c.n) for c in plain} >= {(d, n) for d in tc.MAP_WIDTHS for n in tc.MAP_ROWS}
    assert {(c.d, c.n) for c in plain if c.tall} >= {(d, n) for d in tc.MAP_WIDTHS if d <= 80 for n in tc.MAP_ROWS_TALL}
    assert not any(c.tall for c in cs if c.d > 80) and any(c.d == 88 and c.n == 257 for c in cs)
    assert {len(c.views) for c in cs} == {1, 2, 3} and {v for c in cs for v in c.views} == {0, 1}
    assert {c.idx for c in cs} == {"perm", "rep"} and {c.plant for c in cs} == {"own", "total", "split"}
    assert {c.floor for c in cs} == {"", "view", "planted"} and any(c.sgd for c in cs)
    big = [c for c in cs if (c.d, c.n) == tc.MAP_BIG]
    assert len(big) == 1 and big[0].blocks == tc.SLOTS and big[0].gemm_blocks == 513
    assert big[0].total - tc.SLOTS * 4 * tc.BLOCK == 1088                      # a fifth element for the threads of five blocks only
    assert tc.thread_elems(big[0].total, big[0].blocks) == 5
    assert tc.mapping_scratch_floats(*tc.MAP_BIG[::-1]) * 4 < 93e6


def test_layout_tiles_the_scratch():
    for n, d in ((1, 1), (17, 5), (257, 88)):
        lay = tc.mapping_layout(n, d)
        offs = sorted(lay.values())
        assert offs == [i * n * d for i in range(2 + 3 * tc.MAX_VIEWS)] and offs[-1] + n * d == tc.mapping_scratch_floats(n, d)
        assert list(lay)[:2] == ["F", "GF"] and lay["V1"] < lay["P1"] < lay["G1"] < lay["V2"]


@pytest.mark.parametrize("c", [c for c in tc.MAP_CASES if c.n <= 257 and c.plant == "own" and not c.floor][::3], ids=lambda c: c.id)
def test_mapping_references_compose_to_the_oracle(c):
    """The references chained in float64 (Arith("bound") values) against oracle.space_mapping_grads per view."""
    ar = Arith("bound")
    o = tc.map_ops(c)
    d = c.d
    F = tc.gather_reference(ar, o.ent[:-1], c.stride, d, o.idx, c.ent_norm)[0]
    M = o.M[:3 * d * d].astype(f64).reshape(3, d, d)
    Vs = [tc.gather_reference(ar, o.views[k][:-1], c.stride, d, o.idx, nz)[0] for k, nz in enumerate(c.views)]
    Ps = [v @ M[k] for k, v in enumerate(Vs)]
    Ss = [float((p * p).sum()) for p in Ps]
    t1 = tc.tail1_reference(ar, c, Ps, F, Ss)
    gF = 0.0
    for k, v in enumerate(Vs):
        loss, g_shared, gM = mo.space_mapping_grads(v, F, M[k], tc.ORTHO_W, tc.NORM_W)
        dP = tc.tail2_reference(ar, Ps[k], t1["G"][k][0], Ss[k], t1["dot"][k][0])[0]
        want_gM, want_ortho = tc.ortho_reference(M[k], v.T @ dP, d)
        np.testing.assert_allclose(want_gM, gM, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(t1["loss"][k][0] + want_ortho, loss, rtol=1e-12)
        gF = gF + g_shared
    np.testing.assert_allclose(t1["GF"][0], gF, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", tc.MAP_CASES, ids=lambda c: c.id)
def test_mapping_case(c):
    """Tier 1 is provably exact; both float32 emulations pass the device comparison within half of every bound."""
    tc.map_bound(c).check()
    o = tc.map_ops(c)
    for mode in ("f32", "fma"):
        got = tc.emulate_map(c, mode)
        problems, ratios = tc.check_map(c, o, got)
        assert not problems, (mode, problems)
        assert worst(ratios) <= 0.5, (mode, ratios)
        if c.floor == "view":
            assert 0 < got["S"][0] < 1e-12 and not tc.live32(got["S"][0]) and tc.live32(got["S"][1])
        if c.floor == "planted":
            assert not any(tc.live32(s) for s in got["S"])


# ----------------------------------------------------------------------------------------------------- B. the attribute tail
def test_attr_tables_cover_the_issue():
    assert {(c.n, c.dim) for c in tc.Z_CASES} == {(1, 1), (37, 75), (16, 80), (2049, 256)} and {c.bias for c in tc.Z_CASES} == {True, False}
    assert 2049 * 256 > tc.SLOTS * tc.BLOCK                                   # a partly live second pass of the 2048-block grid
    assert {c.n * c.dim for c in tc.B_CASES} >= {1, 1023, 1024, 1025, 32785 * 33}
    assert 32785 * 33 > 4 * 1024 * tc.BLOCK and any(c.grad_bias for c in tc.B_CASES) and any(c.floor for c in tc.B_CASES)
    plain = [c for c in tc.L_CASES if c.n < 30000]
    assert {(c.stride, c.dim, c.n) for c in plain} == {(s, dm, n) for s in tc.L_STRIDES for dm in (s, s - 1, s - 15) for n in tc.L_ROWS}
    for field in ("weights", "grad_ent", "ent_norm"):
        assert {bool(getattr(c, field)) for c in tc.L_CASES} == {True, False}
    assert any(c.n == 32785 and c.dim == 5 and c.blocks == tc.SLOTS for c in tc.L_CASES)


def test_attr_step_layout():
    for d, n in tc.STEP_SHAPES:
        lay = tc.attr_layout(n, d)
        end = 0
        for name in ("flat", "dflat", "z", "gout"):
            off, rows, ld = lay[name]
            assert off == end and rows == n
            end = off + rows * ld
        assert end == tc.attr_scratch_floats(n, d)
    assert [tc.fused_tail(n, d, 1) for d, n in tc.STEP_SHAPES] == [True, True, True, False] and not tc.fused_tail(80, 75, 0)
    assert all((4 * d * d <= n * 4 * d) == (n >= d) for d, n in tc.STEP_SHAPES)    # W^T fits the dflat scratch from n >= dim on: the gate


def test_attr_tail_composes_to_the_oracle():
    """dz of tailbwd_reference against the closed form of l2_normalize + tanh backward in float64."""
    for c in tc.B_CASES[:8]:
        z, g, sp, tp, _ = tc.tailbwd_ops(c)
        S, T, t = float(sp.sum()), float(tp.sum()), c.n * c.dim
        z64, g64 = z[:t].astype(f64), g[:t].astype(f64)
        inv = 1.0 / np.sqrt(max(S, L2_EPS32))                     # the epsilon as the kernels hold it: float32
        want = inv * (g64 - (z64 * inv * inv * T if S > L2_EPS32 else 0.0)) * (1 - z64 * z64)
        np.testing.assert_allclose(tc.tailbwd_reference(Arith("bound"), c, z, g, S, T)[0], want, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(tc.dz_reference(z[:t], g[:t], S, T), want, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("c", tc.L_CASES[::7] + tc.L_CASES[-2:], ids=lambda c: c.id)
def test_tail_loss_reference_against_plain_numpy(c):
    o = tc.tailloss_ops(c)
    r = tc.tailloss_reference(Arith("bound"), c, o)
    n, dim = c.n, c.dim
    H = o.ent[:-1, :dim].astype(f64)
    if c.ent_norm:
        H = H / np.sqrt(np.maximum((H * H).sum(1, keepdims=True), 1e-12))
    H, Z = H[o.ih], o.z[:n * dim].astype(f64).reshape(n, dim)
    w = o.ws[:n].astype(f64) if c.weights else np.ones(n)
    diff = H - Z / np.sqrt(o.S)
    x = (diff * diff).sum(1)
    np.testing.assert_allclose(r["loss"][0], c.scale * float((w * np.logaddexp(0, x)).sum()), rtol=1e-12)
    gh = (2 * c.scale * w / (1 + np.exp(-x)))[:, None] * diff
    np.testing.assert_allclose(r["gout"][0], -gh, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(r["dot"][0], -float((gh * Z).sum()), rtol=1e-9, atol=1e-12)


def test_attr_emulations_within_half_of_the_bounds():
    for c in tc.Z_CASES:
        z, b = tc.tailz_ops(c)
        problems, ratios = tc.check_tailz(c, z, b, *tc.emulate_tailz(c))
        assert not problems and worst(ratios) <= 0.5, (c.id, problems, ratios)
    for c in tc.B_CASES:
        for mode in ("f32", "fma"):
            problems, ratios = tc.check_tailbwd(c, *tc.emulate_tailbwd(c, mode))
            assert not problems and worst(ratios) <= 0.5, (c.id, mode, problems, ratios)
    for c in tc.L_CASES:
        o = tc.tailloss_ops(c)
        for mode in ("f32", "fma"):
            problems, ratios = tc.check_tailloss(c, o, tc.emulate_tailloss(c, mode))
            assert not problems and worst(ratios) <= 0.5, (c.id, mode, problems, ratios)


# ----------------------------------------------------------------------------------------------------- C. the auto-encoder
@pytest.mark.parametrize("c", tc.A_CASES, ids=lambda c: c.id)
def test_autoencoder_case(c):
    """Every product of the step is exact in float32 in any order, and a device that computes the reference passes."""
    o = tc.ae_ops(c)
    lay = tc.ae_layout(c.dims, c.rows)
    assert lay["end"][0] + c.shift <= tc.ae_scratch_floats(c.dims, c.rows)
    if c.tier2:                                                 # both float32 emulations within half of every counted bound
        for mode in ("f32", "fma"):
            problems, ratios = tc.check_ae2(c, o, tc.ae2_emulate(c, mode))
            assert not problems and worst(ratios) <= 0.5, (mode, problems, ratios)
        return
    b = tc.Bound()
    tc.ae_reference(c, o, bound=b)
    b.check()
    problems, _ = tc.check_ae(c, o, tc.ae_emulate(c))
    assert not problems, problems
    ts = 2.0 / (c.global_rows * c.dims[0])
    assert np.frexp(ts)[0] == 0.5 and tc.live32(o.S) != c.floor


def test_autoencoder_table_covers_the_issue():
    t2 = [c for c in tc.A_CASES if c.tier2]
    assert {c.dims for c in t2} == {(16, 8), (64, 33, 9), (20, 12), (150, 140, 130), (32, 24, 16, 12, 8)}
    for dims, ldx in tc.AE_PLANS:
        mine = [c for c in t2 if c.dims == dims and not c.shift]
        assert {c.rows for c in mine} == set(tc.AE_ROWS) | {37} and {c.ldx for c in mine} == {ldx}
        assert {c.act for c in mine} >= {"tanh", "sigmoid"} and {c.normalize for c in mine} == {0, 1}
        assert any(c.rows == 37 and c.global_rows == 64 for c in mine)
        assert {c.act for c in mine if c.normalize} >= {"tanh", "sigmoid"}
    assert {c.act for c in t2 if c.dims in ((20, 12), (150, 140, 130), (32, 24, 16, 12, 8))} == {"none", "tanh", "sigmoid"}
    t1 = [c for c in tc.A_CASES if not c.tier2 and not c.floor and not c.shift]
    for dims in ((16, 8), (64, 33, 9), (32, 12)):
        assert {c.rows for c in t1 if c.dims == dims} >= set(tc.AE_ROWS)
    assert 130 > 128                                            # the code of [150, 140, 130]: a second column pass of k_ae_norm_bwd


def test_autoencoder_tier2_composes_to_the_oracle():
    """ae2_eval in float64 with the batch's own S and D against oracle.loss_and_grads, activations and normalisation included
    (plans whose target_scale is a power of two: the kernel's float32 target_scale is then the oracle's)."""
    from oracle import literal_oracle as lo
    done = set()
    for c in tc.A_CASES:
        if not c.tier2 or c.rows != c.global_rows or c.dims[0] not in (16, 32, 64) or c.rows not in (1, 8, 16) or c.shift:
            continue
        o = tc.ae_ops(c)
        n = c.n
        ar = tc.Arith("bound")
        first = tc.ae2_eval(ar, c, o._replace(S=1.0, D=0.0))
        o = o._replace(S=first["ssq_own"][0] if c.normalize else 1.0)
        o = o._replace(D=tc.ae2_eval(ar, c, o)["dot_own"][0])
        r = tc.ae2_eval(ar, c, o)
        p = {}
        for i in range(n):
            p[f"encoder_h{i}"], p[f"encoder_b{i}"], p[f"decoder_h{i}"], p[f"decoder_b{i}"] = o.W[i], o.b[i], o.W[n + i], o.b[n + i]
        loss, g = lo.loss_and_grads(p, o.x[:c.rows, :c.dims[0]].astype(f64), n, c.act, bool(c.normalize))
        np.testing.assert_allclose(r["loss"][0], loss, rtol=1e-12)
        for k in range(2 * n):
            name = f"encoder_h{k}" if k < n else f"decoder_h{k - n}"
            np.testing.assert_allclose(r["g"][f"W{k}"][0], g[name], rtol=1e-9, atol=1e-13, err_msg=c.id + name)
            np.testing.assert_allclose(r["g"][f"b{k}"][0], g[name.replace("_h", "_b")], rtol=1e-9, atol=1e-13, err_msg=c.id + name)
        done.add((c.act, c.normalize))
    assert done >= {("tanh", 0), ("tanh", 1), ("sigmoid", 0), ("sigmoid", 1)}, done


def test_autoencoder_reference_against_the_oracle():
    from oracle import literal_oracle as lo
    for c in tc.A_CASES:
        if c.floor or c.rows != c.global_rows or c.tier2:
            continue
        o = tc.ae_ops(c)
        n = c.n
        r = tc.ae_reference(c, o._replace(S=1.0, D=0.0))
        p = {}
        for i in range(n):
            p[f"encoder_h{i}"], p[f"encoder_b{i}"], p[f"decoder_h{i}"], p[f"decoder_b{i}"] = o.W[i], o.b[i], o.W[n + i], o.b[n + i]
        loss, g = lo.loss_and_grads(p, o.x[:c.rows, :c.dims[0]].astype(f64), n, "none", False)
        if not c.normalize:
            np.testing.assert_allclose(r["loss"], loss, rtol=1e-12)
            w_off, b_off, _, shapes = tc.ae_offsets(c.dims)
            for k in range(2 * n):
                name = (f"encoder_h{k}" if k < n else f"decoder_h{k - n}")
                din, dout = shapes[k]
                got = r["grads"][w_off[k]:w_off[k] + din * tc.pad4(dout)].reshape(din, tc.pad4(dout))
                np.testing.assert_allclose(got[:, :dout], g[name], rtol=1e-12, atol=1e-15)
                assert not got[:, dout:].any()
                np.testing.assert_allclose(r["grads"][b_off[k]:b_off[k] + dout], g[name.replace("_h", "_b")], rtol=1e-12, atol=1e-15)


def test_every_epilogue_field_on_both_gemm_kernels():
    seen = {True: set(), False: set()}
    for c in tc.A_CASES:
        if not c.floor:
            for fields, vec in tc.ae_products(c):
                if c.act == "none":                             # act' = 1: a kernel that ignored dact_y would pass these
                    fields = fields - {"dact_y"}
                seen[vec] |= fields
    for act in ("tanh", "sigmoid"):
        for vec in (True, False):
            assert any("dact_y" in f and v == vec for c in tc.A_CASES if c.act == act for f, v in tc.ae_products(c)), (act, vec)
    assert seen[True] >= tc.EPILOGUE_FIELDS and seen[False] >= tc.EPILOGUE_FIELDS, seen
    plain = [v for c in tc.A_CASES if not c.shift and c.ldx % 4 == 0 for _, v in tc.ae_products(c)]
    assert all(plain)                                           # aligned, padded plans never leave the 16-byte kernel


# ----------------------------------------------------------------------------------------------------- mutants
# what the comparison must say: "differs" (tier 1), "error / bound" (tier 2, a ratio above 1) or "not finite" (the NaN poison
# of a partials array or of GF came through)
KIND = {"slots_not_cleared": "not finite", "floor_keeps_projection": "error / bound", "coef_one_inv": "error / bound",
        "first_view_adds": "not finite", "later_view_overwrites": "error / bound", "ortho_keeps_identity": "differs",
        "scatter_last_wins": "differs", "bias_by_stride": "error / bound", "second_pass_row": "error / bound",
        "weights_dropped_in_gradient": "error / bound", "scale_twice": "error / bound", "wt_not_transposed": "differs",
        "colsum_one_half": "differs", "colsum_dead_rows": "differs", "target_ld": "differs", "mean_over_local_rows": "differs",
        "partials_not_rezeroed": "not all zero", "dact_dropped": "error / bound"}
MAP_SAMPLE = [c for c in tc.MAP_CASES if c.n <= 257][::4] + [c for c in tc.MAP_CASES if c.floor]


def broken_cases(mutant):
    out = []
    if mutant in tc.MAP_MUTANTS:
        for c in MAP_SAMPLE:
            problems, _ = tc.check_map(c, tc.map_ops(c), tc.emulate_map(c, "f32", mutant))
            out += [(c.id, p) for p in problems]
    if mutant in ("floor_keeps_projection", "coef_one_inv"):
        for c in tc.B_CASES[:8]:
            out += [(c.id, p) for p in tc.check_tailbwd(c, *tc.emulate_tailbwd(c, "f32", mutant))[0]]
    if mutant == "bias_by_stride":
        for c in tc.Z_CASES:
            z, b = tc.tailz_ops(c)
            out += [(c.id, p) for p in tc.check_tailz(c, z, b, *tc.emulate_tailz(c, mutant))[0]]
    if mutant in tc.AE_MUTANTS or mutant == "floor_keeps_projection":
        for c in tc.A_CASES:
            if not c.tier2:
                out += [(c.id, p) for p in tc.check_ae(c, tc.ae_ops(c), tc.ae_emulate(c, mutant))[0]]
            elif mutant == "dact_dropped":
                out += [(c.id, p) for p in tc.check_ae2(c, tc.ae_ops(c), tc.ae2_emulate(c, "f32", mutant))[0]]
    if mutant == "wt_not_transposed":
        for d, _ in tc.STEP_SHAPES:
            W = tc.quarters(np.random.default_rng(d), (4 * d, d)).astype(np.float32)
            out += [(f"step-d{d}", p) for p in tc.check_wt(tc.wt_reference(W, mutant), W)]
    if mutant in tc.ATTR_MUTANTS and mutant not in ("bias_by_stride", "wt_not_transposed"):
        for c in tc.L_CASES[::5] + tc.L_CASES[-2:]:
            out += [(c.id, p) for p in tc.check_tailloss(c, tc.tailloss_ops(c), tc.emulate_tailloss(c, "f32", mutant))[0]]
    return out


@pytest.mark.parametrize("mutant", tc.MUTANTS)
def test_every_mutant_breaks_a_case(mutant):
    broken = broken_cases(mutant)
    assert broken, mutant
    assert any(KIND[mutant] in p for _, p in broken), (mutant, broken[:5])
    if mutant == "floor_keeps_projection":                     # only batches on the floor tell
        assert all("floor" in cid for cid, _ in broken), broken[:5]
        assert any(cid.startswith("ae-") for cid, _ in broken) and any(cid.startswith("map-") for cid, _ in broken)
    if mutant == "scatter_last_wins":
        assert all("-rep-" in cid for cid, _ in broken), broken[:5]
    if mutant == "dact_dropped":                               # invisible without an activation, and in one-layer plans
        assert all(cid.endswith(("-tanh", "-sigmoid")) for cid, _ in broken) and not any("ae-16x8" in cid or "ae-20x12" in cid for cid, _ in broken)
    if mutant == "second_pass_row":
        assert all("n32785" in cid for cid, _ in broken), broken[:5]


def test_mutant_list():
    assert tc.MUTANTS == ("slots_not_cleared", "floor_keeps_projection", "coef_one_inv", "first_view_adds", "later_view_overwrites",
                          "ortho_keeps_identity", "scatter_last_wins", "bias_by_stride", "second_pass_row",
                          "weights_dropped_in_gradient", "scale_twice", "wt_not_transposed", "colsum_one_half", "colsum_dead_rows",
                          "target_ld", "mean_over_local_rows", "partials_not_rezeroed", "dact_dropped")
    assert set(KIND) == set(tc.MUTANTS)

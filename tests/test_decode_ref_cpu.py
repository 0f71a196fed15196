"""decode_ref.py checks itself, without a GPU: on every case that test_decode_kernels_gpu.py runs, a faithful fp32 op-by-op evaluation of
each decode-step kernel stays inside the counted bound (bad == 0, worst err / bound printed), and every listed defect, planted into the
same evaluation, leaves the bound on the case named for it here — a defect that no case caught would mean a missing case or a bound that is
too wide.  Two host-side checks of the decode engine's weight packing are here as well: BeamDecodeEngine._fold_ln against the fp64
identity it rests on, and fragment_major against the address formula of the fused kernel."""
from importlib import import_module

import pytest
import torch

import decode_ref as R
from conftest import load_pkg

F, B = R.F, R.B


def inside(got, ref, bound, label):
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("RATIO %-60s faithful worst err/bound %.3f" % (label, ratio))
    assert bad == 0 and ratio < 1.0, "%s: %d elements outside the bound, worst err/bound %.3f" % (label, bad, ratio)
    return ratio


def leaves(got, ref, bound, label):
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("DEFECT %-60s worst err/bound %.3g, %d outside" % (label, ratio, bad))
    assert bad > 0, "%s stays inside the bound (worst err/bound %.3f): the bound is blind to it" % (label, ratio)


# ------------------------------------------------------------------------------------------------------------------------------------
# cross attention
# ------------------------------------------------------------------------------------------------------------------------------------
CROSS = [("mc", c) for c in R.MC_CASES] + [("valu", c) for c in R.VALU_CASES]


@pytest.mark.parametrize("route,case", CROSS, ids=[r + "-" + R.cross_id(c) for r, c in CROSS])
def test_cross_faithful(route, case):
    dt, D, H, S, beam = case
    q, kx, vx, scale = R.cross_inputs(S, beam, H, D, dt)
    for mk in R.MASKS:
        kpm = R.cross_mask(S, mk)
        for nw in ((4, 8) if route == "valu" and S == 289 and beam == 5 else (4,)):    # CST_DEC_CROSS_NW=8
            r = R.cross64(q, kx, vx, kpm, scale, beam, route, nw)
            inside(R.cross_emulate32(q, kx, vx, kpm, scale, beam, route, None, nw), r["out"], r["bound"], "%s %s %s nw=%d" % (route, R.cross_id(case), mk, nw))


def test_cross_planted_logits_climb():
    """Sentence 1 at S = 289: for every query row the maximum over a wave's tile climbs by more than FA_THR = 8 log2 units from tile
    w to w + 4 and again to w + 8 (waves 0 and 1 own three tiles), so the matrix-core kernel raises its maximum three times per row; the
    planted key of sentence 2's row 0 leads by ONE_HOT log2 units and sits in tile 7, wave 3's last."""
    q, kx, vx, scale = R.cross_inputs(289, 5, 2, 64, B)
    t = R.cross64(q, kx, vx, None, scale, 5, "mc")["t"]      # [BSZ, H, beam, S], log2 units
    tiles = torch.cat([t, t.new_full(t.shape[:-1] + (31,), R.NINF)], -1).view(3, 2, 5, 10, 32).amax(-1)
    for w in (0, 1):
        assert float((tiles[1, :, :, w + 4] - tiles[1, :, :, w]).min()) > 8.0 and float((tiles[1, :, :, w + 8] - tiles[1, :, :, w + 4]).min()) > 8.0
    jh = R.one_hot_key(289)
    assert jh // 32 == 7
    row = t[2, :, 0]
    rest = torch.cat([row[:, :jh], row[:, jh + 1:]], 1).amax(-1)
    assert float((row[:, jh] - rest).min()) >= R.ONE_HOT


def test_cross_all_masked_sentence_is_plus_zero():
    """Both emulations (as both kernels must) return +0 rows for a sentence whose every key is masked, and leave the others as they were."""
    for route, dt in (("mc", B), ("valu", B), ("valu", F)):
        q, kx, vx, scale = R.cross_inputs(97, 5, 2, 64, dt)
        kpm = R.cross_mask(97, "suffix").clone()
        ref = R.cross_emulate32(q, kx, vx, kpm, scale, 5, route)
        kpm[1] = 1
        got = R.cross_emulate32(q, kx, vx, kpm, scale, 5, route)
        assert bool((got[5:10] == 0).all()) and not bool(torch.signbit(got[5:10]).any())
        assert torch.equal(got[:5], ref[:5]) and torch.equal(got[10:], ref[10:])


S33, S289, S97 = (B, 64, 2, 33, 5), (B, 64, 2, 289, 5), (B, 64, 3, 97, 32)
CROSS_DEFECT_CASE = {
    "last_key_of_ragged_tile_dropped": (S33, "none"), "mask_bit_of_wrong_register": (S33, "suffix"),
    "second_mask_word_of_ballot_lost": (S289, "suffix"), "wave_3_state_not_merged": (S289, "none"),
    "rescale_skipped_on_second_raise": (S289, "none"), "wave_with_masked_first_tile_keeps_minus_inf": (S289, "prefix"),
    "query_row_beam_minus_1_from_row_0": (S33, "none"), "scale_applied_after_rounding": (S97, "prefix")}


# scale_applied_after_rounding is the matrix-core kernel's alone: the VALU kernel does not round the scaled query, and moving its fp32
# product behind the dot product is a reordering that the bound rightly allows
CROSS_DEFECT_RUNS = [(r, d) for r in ("mc", "valu") for d in R.CROSS_DEFECTS if (r, d) != ("valu", "scale_applied_after_rounding")]


@pytest.mark.parametrize("route,defect", CROSS_DEFECT_RUNS, ids=["%s-%s" % rd for rd in CROSS_DEFECT_RUNS])
def test_cross_defect_leaves_bound(route, defect):
    (dt, D, H, S, beam), mk = CROSS_DEFECT_CASE[defect]
    q, kx, vx, scale = R.cross_inputs(S, beam, H, D, dt)
    kpm = R.cross_mask(S, mk)
    r = R.cross64(q, kx, vx, kpm, scale, beam, route)
    label = "%s %s %s %s" % (route, R.cross_id((dt, D, H, S, beam)), mk, defect)
    inside(R.cross_emulate32(q, kx, vx, kpm, scale, beam, route), r["out"], r["bound"], label)
    leaves(R.cross_emulate32(q, kx, vx, kpm, scale, beam, route, defect), r["out"], r["bound"], label)


# ------------------------------------------------------------------------------------------------------------------------------------
# the fused LayerNorm + query projection + cross attention
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.QX_CASES, ids=R.qx_id)
def test_qx_faithful(case):
    H, beam, S = case
    p = R.qx_inputs(H, beam, S)
    for mk in R.MASKS:
        kpm = R.cross_mask(S, mk)
        r = R.qx64(p, kpm, beam)
        inside(R.qx_emulate32(p, kpm, beam), r["out"], r["bound"], "qx %s %s" % (R.qx_id(case), mk))
    t = R.qx64(p, None, beam)["t"] / R.LOG2E            # natural units
    sd = t.std(-1)
    big = sd[sd > 1.0]                                  # (the rows of small elements have q = sb: flat scores)
    assert 2.0 <= float(big.mean()) <= 3.0, float(big.mean())


QX_DEFECT_CASE = {d: ((4, 5, 289), "none") for d in R.LN_DEFECTS}
QX_DEFECT_CASE["fragment_major_halves_swapped"] = ((8, 5, 129), "scattered")


@pytest.mark.parametrize("defect", R.LN_DEFECTS)
def test_qx_defect_leaves_bound(defect):
    (H, beam, S), mk = QX_DEFECT_CASE[defect]
    p = R.qx_inputs(H, beam, S)
    kpm = R.cross_mask(S, mk)
    r = R.qx64(p, kpm, beam)
    leaves(R.qx_emulate32(p, kpm, beam, defect), r["out"], r["bound"], "qx %s %s %s" % (R.qx_id((H, beam, S)), mk, defect))


# ------------------------------------------------------------------------------------------------------------------------------------
# self-attention
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D", R.SELF_CASES, ids=["%s-D%d" % (R.NAME[dt], D) for dt, D in R.SELF_CASES])
def test_self_faithful(dt, D):
    bk, max_len, steps = R.self_geometry(dt, D)
    assert steps == [0, 1, bk - 1, bk, bk + 1, 2 * bk, max_len] and max_len > 2 * bk
    for s in steps:
        qkv, kc, vc, anc, scale = R.self_inputs(dt, D, s)
        r = R.self64(qkv, kc, vc, anc, s, scale)
        inside(R.self_emulate32(qkv, kc, vc, anc, s, scale), r["out"], r["bound"], "self %s D%d s=%d" % (R.NAME[dt], D, s))


SELF_DEFECT_STEP = {"ancestor_of_previous_parity": "bk+1", "position_s_read_from_cache": "0", "batch_boundary_key_dropped": "bk",
                    "slot_reduction_misses_last_slot": "bk-1"}


@pytest.mark.parametrize("dt,D", R.SELF_CASES, ids=["%s-D%d" % (R.NAME[dt], D) for dt, D in R.SELF_CASES])
@pytest.mark.parametrize("defect", R.SELF_DEFECTS)
def test_self_defect_leaves_bound(defect, dt, D):
    bk = R.self_geometry(dt, D)[0]
    s = {"0": 0, "bk-1": bk - 1, "bk": bk, "bk+1": bk + 1}[SELF_DEFECT_STEP[defect]]
    qkv, kc, vc, anc, scale = R.self_inputs(dt, D, s)
    r = R.self64(qkv, kc, vc, anc, s, scale)
    leaves(R.self_emulate32(qkv, kc, vc, anc, s, scale, defect), r["out"], r["bound"], "self %s D%d s=%d %s" % (R.NAME[dt], D, s, defect))


# ------------------------------------------------------------------------------------------------------------------------------------
# Linear, LayerNorm-folded Linear
# ------------------------------------------------------------------------------------------------------------------------------------
LIN_COMBOS = [("none", True, False), ("relu", False, True), ("gelu", True, True)]    # (activation, bias, residual)


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("case", R.LIN_CASES, ids=R.lin_id)
def test_linear_faithful(case, ln):
    name, M, N, K = case
    d = R.lin_dispatch(M, N, K)
    assert d["name"] == name, d
    p = R.lin_inputs(M, N, K, ln)
    for env_nw in ((0, 4, 16) if N <= 520 else (0,)):     # CST_DEC_LINEAR_NW
        d = R.lin_dispatch(M, N, K, env_nw)
        for act, hb, hr in LIN_COMBOS:
            r = R.lin64(p, ln, act, hb, hr, d["nw"])
            inside(R.lin_emulate32(p, ln, act, hb, hr, d["nw"], d["un"]), r["y"], r["bound"],
                   "linear %s ln=%d %s bias=%d resid=%d nw=%d" % (R.lin_id(case), ln, act, hb, hr, d["nw"]))


def test_linear_table_reaches_every_default_instantiation():
    """The table's shapes, through the launcher's dispatch restated in lin_dispatch: every (NT, UN) pair that the default NW = 8
    reaches, a second row tile holding one row, the prefetch loop at one and at several iterations."""
    got = {R.lin_dispatch(M, N, K)["name"] for _, M, N, K in R.LIN_CASES}
    assert got == {"NT1/UN4", "NT1/UN2", "NT2/UN4", "NT2/UN2", "NT4/UN2"}
    d = R.lin_dispatch(81, 2576, 1536)
    assert (d["nt"], d["un"], d["nw"]) == (2, 2, 8) and 320 < d["wg1"] <= 1024 and d["iters"] == 3
    assert R.lin_dispatch(80, 520, 1536)["iters"] == 3 and R.lin_dispatch(161, 5472, 1024)["iters"] == 4
    assert R.lin_dispatch(81, 40, 1024)["iters"] == 1 and R.lin_dispatch(161, 5472, 512)["wg1"] > 1024


LIN_DEFECT_CASE = {"k_quarter_of_last_wave_dropped": (81, 40, 1024), "prefetched_step_used_twice": (80, 520, 1536), "row_80_from_row_79": (81, 40, 1024),
                   "bias_of_column_n_minus_1": (1, 17, 512), "resid_with_ldy": (81, 40, 1024), "activation_after_residual": (1, 17, 512)}
LN_DEFECT_CASE = {"sg_of_wrong_head": (80, 520, 1536), "mean_over_kq": (1, 17, 512), "variance_without_mean_square": (81, 40, 1024),
                  "eps_outside_sqrt": (81, 40, 1024)}


@pytest.mark.parametrize("defect", R.LIN_DEFECTS + R.LN_DEFECTS[:4])
def test_linear_defect_leaves_bound(defect):
    """(fragment_major_halves_swapped belongs to the fused query projection alone: test_qx_defect_leaves_bound.)"""
    ln = defect in R.LN_DEFECTS
    M, N, K = (LN_DEFECT_CASE if ln else LIN_DEFECT_CASE)[defect]
    d = R.lin_dispatch(M, N, K)
    p = R.lin_inputs(M, N, K, ln)
    r = R.lin64(p, ln, "gelu", True, True, d["nw"])
    leaves(R.lin_emulate32(p, ln, "gelu", True, True, d["nw"], d["un"], defect), r["y"], r["bound"], "linear M%d-N%d-K%d ln=%d %s" % (M, N, K, ln, defect))


# ------------------------------------------------------------------------------------------------------------------------------------
# host side: the LayerNorm fold and the fragment-major packing of the decode engine
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    load_pkg()
    return import_module("chimera-st_amd.decode_engine").BeamDecodeEngine


@pytest.mark.parametrize("with_bias", [True, False])
def test_fold_ln_identity(engine, with_bias):
    """LN(x) W^T + b = rstd (x Wg^T - mean sg) + sb in fp64, with the engine's Wg (bf16), sg, sb (fp32).  sg is summed from the ROUNDED
    Wg, so the two sides differ by the one bf16 rounding of Wg = W gamma, rstd sum_k |x_k - mean| |W gamma|_k UBF, and by the fp32
    roundings of the products and of the two K-term sums (counted: K + 1 roundings on the absolute terms)."""
    N, K, M = 72, 512, 6
    g = R._gen(71)
    ln = torch.nn.LayerNorm(K)
    with torch.no_grad():
        ln.weight.copy_(1.0 + 0.3 * torch.randn(K, generator=g))
        ln.bias.copy_(0.2 * torch.randn(K, generator=g))
    ln = ln.to(B)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(B)
    b = torch.randn(N, generator=g).to(B) if with_bias else None
    x = R.ln_rows(M, K, 72).double()
    wg, sg, sb, eps = engine._fold_ln(ln, W, b)
    assert wg.dtype == B and sg.dtype == F and sb.dtype == F and eps == ln.eps
    ga, be, Wd = ln.weight.detach().double(), ln.bias.detach().double(), W.double()
    mean = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    lhs = ((x - mean) * rstd * ga + be) @ Wd.t() + (b.double() if with_bias else 0.0)
    rhs = rstd * (x @ wg.double().t() - mean * sg.double()) + sb.double()
    u = R.U32
    slack = rstd * ((x - mean).abs() @ (Wd * ga).abs().t()) * (R.UBF + u)              # the rounding of Wg (and of the fp32 product before it)
    slack = slack + (rstd * mean).abs() * (K + 1) * u * wg.double().abs().sum(1)        # sg: an fp32 sum of K terms
    slack = slack + (K + 3) * u * ((Wd * be).abs().sum(1) + (b.double().abs() if with_bias else 0.0))   # sb
    inside(rhs, lhs, R.SLACK * slack, "fold_ln bias=%d" % with_bias)
    # and the slack is the rounding's, not room: gamma left out of the fold leaves it at once
    wrong = rstd * (x @ Wd.t() - mean * Wd.sum(1)) + sb.double()
    leaves(wrong, lhs, R.SLACK * slack, "fold_ln without gamma")


@pytest.mark.parametrize("K", [256, 512])
def test_fragment_major_address(engine, K):
    """fragment_major followed by the kernel's address formula returns Wg[h * 64 + n][k] for every (h, n, k): exact."""
    H = 2
    wg = torch.arange(H * 64 * K, dtype=torch.float32).view(H * 64, K)      # every element its own value
    flat = engine.fragment_major(wg, H).reshape(-1)
    assert flat.numel() == wg.numel()
    h, n, k = torch.meshgrid(torch.arange(H), torch.arange(64), torch.arange(K), indexing="ij")
    addr = R.frag_address(h, n, k, K)
    assert torch.equal(flat[addr], wg.view(H, 64, K))
    # lane l of the load of k-group kg of block bl reads 8 contiguous elements: (column 32 bl + l % 32, k = 16 kg + 8 (l / 32) ..)
    assert int(R.frag_address(1, 33, 24, K)) == (((1 * 2 + 1) * (K // 16) + 1) * 64 + 32 + 1) * 8

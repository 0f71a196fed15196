"""The HBM-bound helpers of csrc/elementwise.hip, the embedding kernels of csrc/embed.hip and the contrastive term of csrc/loss_optim.hip
on a real MI355X against the fp64 restatements of helper_ref.py, under ITS per-element bounds (counted from the kernels' operation
sequences; test_helper_ref_cpu.py shows that a faithful fp32 evaluation stays inside them and that every listed defect leaves them).
What is exact is compared with torch.equal.  The shapes are the smallest that reach each path: the second grid-stride iteration of the
capped elementwise grids (8.4 M elements; the fp64 reference of those runs on the device), both sides of every unroll, more than 64 row
chunks in the column sums' reduce kernel, rows = 49 .. 63 (mod 64), all four vector slots and the second round of the owner search of
the embedding gradient, M = 1 and C < 32 in the contrastive kernels.

Every comparison prints `RATIO <kernel> <dtype> <quantity> ... worst err/bound`, and the module prints the worst ratio per kernel,
quantity and dtype at its end (pytest -s)."""
from importlib import import_module

import pytest
import torch

import helper_ref as H
from conftest import load_pkg

pytestmark = pytest.mark.gpu
DTS = [H.F, H.B]
IDS = ["f32", "bf16"]
WORST = {}


@pytest.fixture(scope="module")
def K():
    load_pkg()
    yield import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")
    for key in sorted(WORST):
        print("WORST %-22s %-10s %-5s %.3f" % (key + (WORST[key],)))


def within(got, ref, bound, key, what=""):
    """key = (kernel, quantity, dtype name)."""
    got = got.detach().to(ref.device)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), "%s: the reference is not finite" % (key,)
    assert bool(torch.isfinite(got.float()).all()), "%s %s: non-finite output" % (key, what)
    ratio, bad = H.worst_ratio(got, ref, bound)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("RATIO %-16s %-8s %-5s %-44s worst err/bound %.3f" % (key + (what, ratio)))
    assert bad == 0, "%s %s: %d of %d elements outside the bound, worst err/bound %.3f" % (key, what, bad, got.numel(), ratio)


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _keep(key, n, p):
    rng = import_module("chimera-st_amd.rng")
    return torch.from_numpy(rng.keep_mask_numpy(key, n, p))


def keep_of(key, n, p):
    """The package's numpy statement of the mask; helper_ref.py's restatement of the hash must be the same function."""
    keep = _keep(key, n, p)
    assert torch.equal(keep, H.keep_mask(key, n, p))
    return keep


# ------------------------------------------------------------------------------------------------------------------------------------
# GLU, activations
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("rows,C", H.GLU_SHAPES + [H.GLU_BIG])
def test_glu(K, rows, C, dt):
    k, _ = K
    assert (rows * C // 8 > H.EW_THREADS) == ((rows, C) == H.GLU_BIG)
    z, dy = cu(*H.glu_inputs(rows, C, dt))
    r = H.glu64(z, dy)                       # (on the device: 8.4 M pairs)
    b = H.glu_bounds(r, dt)
    what = "%dx%d" % (rows, C)
    within(k.glu_fwd(z), r["y"], b["y"], ("glu_fwd", "y", H.NAME[dt]), what)
    within(k.glu_bwd(dy, z), torch.cat([r["da"], r["dg"]], 1), b["dz"], ("glu_bwd", "dz", H.NAME[dt]), what)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n", H.ACT_SIZES)
def test_activations(K, n, dt):
    """ReLU and ReLU' are exact, with ReLU'(+0) = ReLU'(-0) = 0 and ReLU'(smallest subnormal) = 1; GELU and GELU' under A_GELU / A_DGELU."""
    k, L = K
    x, dy = cu(*H.act_inputs(n, dt))
    y, dx = H.relu_ref(x, dy)
    assert torch.equal(k.act_fwd(x, L.ACT_RELU), y)
    got = k.act_bwd(dy, x, L.ACT_RELU)
    assert torch.equal(got, dx)
    assert bool((got[:2] == 0).all()) and float(got[2]) == float(dy[2]) and float(got[3]) == 0.0
    r = H.gelu_act64(x, dy)
    b = H.gelu_act_bounds(r, dt)
    within(k.act_fwd(x, L.ACT_GELU), r["y"], b["y"], ("act_fwd", "gelu", H.NAME[dt]), "n=%d" % n)
    within(k.act_bwd(dy, x, L.ACT_GELU), r["dx"], b["dx"], ("act_bwd", "gelu'", H.NAME[dt]), "n=%d" % n)


# ------------------------------------------------------------------------------------------------------------------------------------
# mask_rows, dropout, dropout_scale
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("rows,cols", H.MASK_SHAPES + [H.MASK_BIG])
def test_mask_rows(K, rows, cols, dt):
    """Masked rows hold NaN and Inf and come back as +0: the kernel assigns, it does not multiply."""
    k, _ = K
    x, mask = cu(*H.mask_inputs(rows, cols, dt))
    y = k.mask_rows(x, mask)
    assert torch.equal(y, H.mask_ref(x, mask))
    assert not bool(torch.signbit(y[mask.bool()]).any())


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n", H.DROP_SIZES)
def test_dropout(K, n, dt):
    k, _ = K
    x = H.drop_inputs(n, dt).cuda()
    assert torch.equal(k.dropout(x, 0.0, H.DROP_KEY), x)
    for p in H.DROP_PS:
        keep = keep_of(H.DROP_KEY, n, p).cuda()
        y = k.dropout(x, p, H.DROP_KEY)
        assert torch.equal(y != 0, keep), "the kept set is not the hash's"
        ref, b = H.dropout64(x, keep, p)
        within(y, ref, b, ("dropout", "y", H.NAME[dt]), "n=%d p=%g" % (n, p))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n", H.DROP_SCALE_SIZES)
def test_dropout_scale(K, n, dt):
    k, _ = K
    x = H.drop_inputs(n, dt).cuda()
    for p in [0.0] + H.DROP_PS:
        keep = keep_of(H.DROP_KEY, n, p).cuda()
        y = k.dropout_scale(x, H.ALPHA, p, H.DROP_KEY)
        assert torch.equal(y != 0, keep)
        ref, b = H.dropout64(x, keep, p, H.ALPHA)
        within(y, ref, b, ("dropout_scale", "y", H.NAME[dt]), "n=%d p=%g" % (n, p))


# ------------------------------------------------------------------------------------------------------------------------------------
# col2im
# ------------------------------------------------------------------------------------------------------------------------------------
def _col2im(k, L, Bn, Lin, C, kk, s, pad, dt, what):
    dcol, z = cu(*H.c2i_inputs(Bn, Lin, C, kk, s, pad, dt))
    Lout = H.c2i_lout(Lin, kk, s, pad)
    for dact, code in ((None, 0), ("gelu", L.ACT_GELU), ("relu", L.ACT_RELU)):
        r = H.col2im64(dcol, z, Bn, Lin, C, kk, s, pad, dact)
        got = k.col2im1d(dcol, z if dact else None, Bn, Lin, Lout, C, kk, s, pad, code)
        within(got, r["dx"], H.col2im_bounds(r, dt), ("col2im1d", str(dact), H.NAME[dt]), what)
        if dact is None and (Lin + 2 * pad - kk) % s > pad:
            assert bool((got[:, -1] == 0).all())      # a trailing position no window covers


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("kk,s,pad", H.C2I_TRIPLES)
def test_col2im(K, kk, s, pad, dt):
    k, L = K
    for Lin in H.c2i_lins(kk, s, pad):
        for C in (8, 16):
            _col2im(k, L, H.C2I_B, Lin, C, kk, s, pad, dt, "k%d s%d p%d Lin%d C%d" % (kk, s, pad, Lin, C))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_col2im_grid_stride(K, dt):
    k, L = K
    Bn, Lin, C, kk, s, pad = H.C2I_BIG
    assert Bn * Lin * C // 8 > H.EW_THREADS
    _col2im(k, L, Bn, Lin, C, kk, s, pad, dt, "k%d s%d p%d Lin%d C%d" % (kk, s, pad, Lin, C))


# ------------------------------------------------------------------------------------------------------------------------------------
# packed rows
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("C", H.RP_COLS)
def test_rows_pack_unpack(K, C, dt):
    k, _ = K
    x, off = H.rp_inputs(C, dt)
    Bn, T = x.shape[0], x.shape[1]
    N = int(off[-1])
    xd, offd = x.cuda(), off.cuda()
    plain = k.rows_pack(xd, offd, N, tail_sum=False).cpu()
    for b in range(Bn):
        assert torch.equal(plain[off[b]:off[b + 1]], x[b, :off[b + 1] - off[b]])
    for tail in (True, False):
        assert torch.equal(k.rows_unpack(plain.cuda(), offd, Bn, T, tail_broadcast=tail).cpu(), H.rows_unpack_ref(plain, off, Bn, T, tail))
    ref, b = H.rows_pack64(x, off)
    got = k.rows_pack(xd, offd, N, tail_sum=True)
    within(got, ref, b, ("rows_pack", "tail_sum", H.NAME[dt]), "C%d" % C)       # (a zero bound: the copies, exact)
    assert torch.equal(got, k.rows_pack(xd, offd, N, tail_sum=True))


# ------------------------------------------------------------------------------------------------------------------------------------
# weight normalisation
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("C", H.WN_COLS)
def test_weight_norm(K, C, dt):
    k, _ = K
    for R, C_ in H.WN_CASES:
        if C_ != C:
            continue
        v, g, dw = H.wn_inputs(R, C, dt)
        vd, gd, dwd = cu(v, g, dw)
        r = H.wn_fwd64(v, g)
        b = H.wn_fwd_bounds(r, dt)
        w, norm = k.weight_norm_fwd(vd, gd)
        what = "%dx%d" % (R, C)
        within(w, r["w"], b["w"], ("weight_norm_fwd", "w", H.NAME[dt]), what)
        within(norm, r["norm"], b["norm"], ("weight_norm_fwd", "norm", H.NAME[dt]), what)
        assert bool((w[:, H.WN_G0] == 0).all())
        rb = H.wn_bwd64(v, g, dw, norm.cpu())       # the reference takes the fp32 norm the kernel is handed
        bb = H.wn_bwd_bounds(rb, dt)
        dv, dg = k.weight_norm_bwd(vd, gd, dwd, norm)
        within(dv, rb["dv"], bb["dv"], ("weight_norm_bwd", "dv", H.NAME[dt]), what)
        within(dg, rb["dg"], bb["dg"], ("weight_norm_bwd", "dg", H.NAME[dt]), what)
        dv2, dg2 = k.weight_norm_bwd(vd, gd, dwd, norm)
        assert torch.equal(dv, dv2) and torch.equal(dg, dg2)


# ------------------------------------------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("cols", H.CS_COLS)
def test_colsum(K, cols, dt):
    """cst_colsum (atomics), cst_colsum_typed in both output dtypes from a contiguous and a strided x (ldx = cols + 8),
    cst_colsum_typed_live with every second tile dead, the last (partial) tile dead, the last tile live, and cst_dropout_colsum:
    bit-equal to cst_dropout followed by cst_colsum_typed, xd under the dropout bound, the sums — defined on the STORED xd — under the
    chain's."""
    k, L = K
    nm = H.NAME[dt]
    for rows in H.CS_ROWS:
        x = H.cs_inputs(rows, cols, dt)
        xd = x.cuda()
        wide = torch.full((rows, cols + 8), 7.0, dtype=dt, device="cuda")
        wide[:, :cols] = xd
        strided = wide[:, :cols]
        what = "%dx%d" % (rows, cols)
        ref, b = H.colsum64(x, rows, cols, False)
        within(k.colsum_atomic(xd), ref, b, ("colsum", "atomic", nm), what)
        within(k.colsum_atomic(strided), ref, b, ("colsum", "atomic", nm), what + " ldx")
        for out_dt in DTS:
            ref, b = H.colsum64(x, rows, cols, True, out_dt)
            got = k.colsum(xd, out_dt)
            within(got, ref, b, ("colsum_typed", "->" + H.NAME[out_dt], nm), what)
            assert torch.equal(got, k.colsum(strided, out_dt)) and torch.equal(got, k.colsum(xd, out_dt))
        for which in H.CS_STAMPS[1:]:
            st, dead = H.cs_stamps(rows, which)
            xs = x.clone()
            xs[dead] = 0
            ref, b = H.colsum64(xs, rows, cols, True, H.F)
            within(k.colsum(xs.cuda(), H.F, (st.cuda(), H.CS_EPOCH)), ref, b, ("colsum_live", which, nm), what)
        keep = keep_of(H.CS_KEY, rows * cols, H.CS_P).view(rows, cols)
        for which in (None, "alternate", "last_dead"):
            xs, live = x.clone(), None
            if which:
                st, dead = H.cs_stamps(rows, which)
                xs[dead] = 0
                live = (st.cuda(), H.CS_EPOCH)
            xsd = xs.cuda()
            for out_dt in DTS:
                got_x, got_s = k.dropout_colsum(xsd, H.CS_P, H.CS_KEY, out_dt, live)
                plain = k.dropout(xsd, H.CS_P, H.CS_KEY)
                assert torch.equal(got_x, plain) and torch.equal(got_s, k.colsum(plain, out_dt, live)), "dropout_colsum != dropout + colsum"
                xref, xb = H.dropout64(xs, keep, H.CS_P)
                within(got_x, xref, xb, ("dropout_colsum", "xd", nm), what + " " + str(which))
                ref, b = H.colsum64(got_x.cpu(), rows, cols, True, out_dt)
                within(got_s, ref, b, ("dropout_colsum", "->" + H.NAME[out_dt], nm), what + " " + str(which))


# ------------------------------------------------------------------------------------------------------------------------------------
# embedding
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("T", H.EF_T)
def test_embed_forward(K, T, dt):
    from oracle import chimera_oracle as O
    k, _ = K
    for C in H.EF_COLS:
        tok, E, x, table = H.ef_inputs(T, C, dt)
        assert torch.equal(table, O.sinusoidal_table(H.PAD + 1 + T, C, H.PAD))
        # the position index itself, exactly: a table whose row r holds r, a zero source, scale 1
        count = torch.arange(H.PAD + 1 + T, dtype=torch.float32)[:, None].expand(-1, C).contiguous().cuda()
        zeros = torch.zeros(4, T, C, dtype=dt, device="cuda")
        want = O.make_positions(tok, H.PAD)
        assert torch.equal(want, H.make_positions(tok.ne(H.PAD), H.PAD)) and torch.equal(table[want], O.positional_embedding(tok, C, H.PAD))
        for tk, mk in ((tok, None), (None, tok.eq(H.PAD).to(torch.uint8)), (tok, tok.eq(H.PAD).to(torch.uint8))):
            got = k.embed_pos_fwd(*cu(tk, mk), None, zeros, count, 1.0, H.PAD, 0.0, 0)
            assert torch.equal(got.float().cpu(), want[:, :, None].expand(-1, -1, C).float()), "positions differ from make_positions"
        scale = C ** 0.5
        for form in H.EF_FORMS:
            args = H.ef_args(form, tok, E, x, table)
            for p in H.EF_PS:
                ref, b = H.embed_fwd64(*args, scale, p, H.EF_KEY)
                got = k.embed_pos_fwd(*cu(*args), scale, H.PAD, p, H.EF_KEY)
                within(got, ref, b, ("embed_pos_fwd", form, H.NAME[dt]), "T%d C%d p=%g" % (T, C, p))
                if form == "tokens":
                    assert bool((got.cpu()[tok == H.PAD] == 0).all())
                if p > 0:
                    keep_of(H.EF_KEY, 4 * T * C, p)


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("n,C,V", H.EB_CASES)
def test_embed_backward(K, n, C, V, dt):
    k, _ = K
    dy, tok = H.eb_inputs(n, C, V, dt)
    dyd, tokd = cu(dy, tok)
    scale = C ** 0.5
    unused = torch.ones(V, dtype=torch.bool)
    unused[tok] = False
    unused[H.PAD] = True
    for gdt in sorted({dt, H.F}, key=str):
        for p in H.EB_PS:
            ref, b = H.embed_bwd64(dy, tok, V, scale, p, H.EB_KEY, gdt)
            got = k.embed_bwd(dyd, tokd, V, scale, H.PAD, p, H.EB_KEY, gdt)
            within(got, ref, b, ("embed_bwd", "->" + H.NAME[gdt], H.NAME[dt]), "n%d C%d V%d p=%g" % (n, C, V, p))
            assert bool((got.cpu()[unused] == 0).all()), "the pad row or an unused row is not zero"
            assert torch.equal(got, k.embed_bwd(dyd, tokd, V, scale, H.PAD, p, H.EB_KEY, gdt))


# ------------------------------------------------------------------------------------------------------------------------------------
# contrastive term
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("Bn,M,C", H.CT_SHAPES)
def test_contrastive(K, Bn, M, C, dt):
    """sim, |a|, |t|, the per-utterance terms and the loss each under its own bound; the backward against the fp64 function of the fp32
    sim / |a| / |t| it is handed.  With an all-zero audio and text row: everything finite, sim and loss still the restatement of the
    clamp max(|a||t|, 1e-8)."""
    k, _ = K
    nm = H.NAME[dt]
    for temp in H.CT_TEMPS:
        for zero_row in (False, True):
            a, t = H.ct_inputs(Bn, M, C, dt, zero_row=zero_row)
            ad, td = cu(a, t)
            r = H.ct_fwd64(a, t, temp)
            b = H.ct_fwd_bounds(r)
            loss, sim, na, nt = k.contrastive_fwd(ad, td, temp)
            rows = k.workspace(Bn * 4, ad.device)[:Bn * 4].view(torch.float32).clone()    # loss_rows: the call's scratch
            what = "%dx%dx%d temp=%g%s" % (Bn, M, C, temp, " zero-row" if zero_row else "")
            q = "0 " if zero_row else ""
            for name, got in (("loss", loss.reshape(())), ("rows", rows), ("sim", sim), ("na", na), ("nt", nt)):
                within(got, r[name], b[name], ("contrastive_fwd", q + name, nm), what)
            for gs in H.CT_GSCALES:
                da, dtt = k.contrastive_bwd(ad, td, sim, na, nt, torch.full((1,), gs, device="cuda"), temp)
                assert bool(torch.isfinite(da.float()).all()) and bool(torch.isfinite(dtt.float()).all())
                if zero_row:
                    continue
                rb = H.ct_bwd64(a, t, sim.cpu(), na.cpu(), nt.cpu(), gs, temp)
                bb = H.ct_bwd_bounds(rb, dt)
                within(da, rb["da"], bb["da"], ("contrastive_bwd", "da", nm), what + " g=%g" % gs)
                within(dtt, rb["dt"], bb["dt"], ("contrastive_bwd", "dt", nm), what + " g=%g" % gs)

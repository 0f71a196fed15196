"""The bounds of helper_ref.py are sound and sharp, shown without a GPU.  For every small case of helper_ref.py and both dtypes:
  * the fp64 reference is finite on every element (no element is exempt from a bound);
  * the faithful fp32 emulation of each kernel lies inside the bound against fp64 on EVERY element (an exact output is torch.equal);
  * every listed defect leaves the bound on at least one element in at least one case of its kernel and dtype — asserted at the end of
    each test from what the cases showed, so a bound too loose to see a defect fails here.
The 8.4 M-element cases of test_helper_gpu.py use the same functions; what changes there is the grid-stride iteration, which the
reference does not know about.

Defects that exist in one dtype only (BF16_ONLY): `norm_of_rounded_w` and `sums_of_unrounded_product` are no change in fp32."""
import pytest
import torch

import helper_ref as H

DTS = [H.F, H.B]
IDS = ["f32", "bf16"]
BF16_ONLY = ("norm_of_rounded_w", "sums_of_unrounded_product")


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all()), "the fp64 reference is not finite"


def _in(got, ref, bound, what):
    _finite(ref, bound)
    ratio, bad = H.worst_ratio(got, ref, bound)
    print("clean %-56s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: the faithful emulation leaves the bound on %d elements (worst ratio %.3f)" % (what, bad, ratio)


def _leaves(got, ref, bound):
    return H.worst_ratio(got, ref, bound)[1] > 0


class Seen:
    """Which defects left the bound in some case."""

    def __init__(self, defects, dt):
        self.seen = {d: False for d in defects if dt == H.B or d not in BF16_ONLY}

    def note(self, defect, out, what):
        if defect in self.seen:
            print("defect %-60s %s" % (what + " " + defect, "outside" if out else "inside"))
            self.seen[defect] = self.seen[defect] or bool(out)

    def check(self):
        missed = [d for d, s in self.seen.items() if not s]
        assert not missed, "defects that stay inside the bound in every case: %s" % missed


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_glu(dt):
    seen = Seen(H.GLU_DEFECTS, dt)
    for rows, C in H.GLU_SHAPES:
        z, dy = H.glu_case(rows, C, dt)
        r = H.glu64(z, dy)
        b = H.glu_bounds(r, dt)
        ref_dz = torch.cat([r["da"], r["dg"]], 1)
        tag = "glu %s %dx%d " % (H.NAME[dt], rows, C)
        y, dz = H.glu_emulate32(z, dy)
        _in(y, r["y"], b["y"], tag + "y")
        _in(dz, ref_dz, b["dz"], tag + "dz")
        for d in H.GLU_DEFECTS:
            yd, dzd = H.glu_emulate32(z, dy, defect=d)
            seen.note(d, _leaves(yd, r["y"], b["y"]) or _leaves(dzd, ref_dz, b["dz"]), tag)
    seen.check()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_activations(dt):
    seen = Seen(H.ACT_DEFECTS, dt)
    for n in (8, 4104):
        x, dy = H.act_inputs(n, dt)
        y, dx = H.relu_ref(x, dy)
        ye, dxe = H.relu_emulate(x, dy)
        assert torch.equal(ye, y) and torch.equal(dxe, dx)
        assert bool((dx[:2] == 0).all()) and float(dx[2]) == float(dy[2]) and float(dx[3]) == 0.0   # ReLU'(+-0) = 0, ReLU'(subnormal) = 1
        for d in H.ACT_DEFECTS:
            seen.note(d, not torch.equal(H.relu_emulate(x, dy, defect=d)[1], dx), "relu n=%d" % n)
        r = H.gelu_act64(x, dy)
        b = H.gelu_act_bounds(r, dt)
        ge, dge = H.gelu_act_emulate32(x, dy)
        _in(ge, r["y"], b["y"], "gelu %s n=%d y" % (H.NAME[dt], n))
        _in(dge, r["dx"], b["dx"], "gelu %s n=%d dx" % (H.NAME[dt], n))
    seen.check()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_mask_rows_and_dropout(dt):
    seen = Seen(H.MASK_DEFECTS + H.DROP_DEFECTS, dt)
    for rows, cols in H.MASK_SHAPES:
        x, mask = H.mask_inputs(rows, cols, dt)
        ref = H.mask_ref(x, mask)
        assert bool(torch.isfinite(ref.float()).all()) and torch.equal(H.mask_emulate(x, mask), ref)
        assert not bool(torch.signbit(ref[mask.bool()]).any())          # masked rows are +0
        seen.note("masked_by_product", not torch.equal(H.mask_emulate(x, mask, defect="masked_by_product"), ref), "mask %dx%d" % (rows, cols))
    for n in H.DROP_SIZES[:-1]:
        x = H.drop_inputs(n, dt)
        assert torch.equal(H.dropout_emulate32(x, H.DROP_KEY, 0.0), x)     # p = 0: the identity
        for p in H.DROP_PS:
            keep = H.keep_mask(H.DROP_KEY, n, p)
            ref, b = H.dropout64(x, keep, p)
            y = H.dropout_emulate32(x, H.DROP_KEY, p)
            assert torch.equal(y != 0, keep)
            _in(y, ref, b, "dropout %s n=%d p=%g" % (H.NAME[dt], n, p))
            for d in H.DROP_DEFECTS:
                seen.note(d, _leaves(H.dropout_emulate32(x, H.DROP_KEY, p, defect=d), ref, b), "dropout n=%d p=%g" % (n, p))
    for n in H.DROP_SCALE_SIZES[:-1]:
        x = H.drop_inputs(n, dt)
        for p in [0.0] + H.DROP_PS:
            keep = H.keep_mask(H.DROP_KEY, n, p)
            ref, b = H.dropout64(x, keep, p, H.ALPHA)
            y = H.dropout_emulate32(x, H.DROP_KEY, p, H.ALPHA)
            assert torch.equal(y != 0, keep)
            _in(y, ref, b, "dropout_scale %s n=%d p=%g" % (H.NAME[dt], n, p))
            assert _leaves(H.dropout_emulate32(x, H.DROP_KEY, p), ref, b), "dropout_scale without alpha stays inside the bound"
    seen.check()


def test_keep_rate():
    for p in H.DROP_PS:
        assert abs(float(H.keep_mask(H.DROP_KEY, 1 << 16, p).float().mean()) - (1 - p)) < 0.01


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_col2im(dt):
    seen = Seen(H.C2I_DEFECTS, dt)
    Bn = H.C2I_B
    for k, s, pad, Lin, C in H.C2I_CASES:
        dcol, z = H.c2i_inputs(Bn, Lin, C, k, s, pad, dt)
        for dact in (None, "gelu", "relu"):
            r = H.col2im64(dcol, z, Bn, Lin, C, k, s, pad, dact)
            b = H.col2im_bounds(r, dt)
            tag = "col2im %s k%d s%d p%d Lin%d C%d %s" % (H.NAME[dt], k, s, pad, Lin, C, dact)
            _in(H.col2im_emulate32(dcol, z, Bn, Lin, C, k, s, pad, dact), r["dx"], b, tag)
            for d in H.C2I_DEFECTS:
                if d == "dact_from_row_l_plus_1" and not dact:
                    continue
                seen.note(d, _leaves(H.col2im_emulate32(dcol, z, Bn, Lin, C, k, s, pad, dact, defect=d), r["dx"], b), tag)
        if (Lin + 2 * pad - k) % s > pad:      # trailing input positions (not only padding) receive nothing: exactly 0
            r = H.col2im64(dcol, z, Bn, Lin, C, k, s, pad, None)
            assert int(r["cnt"][-1]) == 0 and bool((r["dx"][:, -1] == 0).all())
    seen.check()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_rows_pack(dt):
    seen = Seen(H.RP_DEFECTS, dt)
    for C in H.RP_COLS:
        x, off = H.rp_inputs(C, dt)
        ref, b = H.rows_pack64(x, off)
        got = H.rows_pack_emulate32(x, off)
        _in(got, ref, b, "rows_pack %s C%d" % (H.NAME[dt], C))
        copies = b.sum(1) == 0
        assert int(copies.sum()) == int(off[-1]) - len(H.RP_LENS) + 1 and torch.equal(got[copies].double(), ref[copies])
        for d in H.RP_DEFECTS:
            seen.note(d, _leaves(H.rows_pack_emulate32(x, off, defect=d), ref, b), "rows_pack C%d" % C)
    seen.check()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_weight_norm(dt):
    fseen, bseen = Seen(H.WN_FWD_DEFECTS, dt), Seen(H.WN_BWD_DEFECTS, dt)
    for R, C in H.WN_CASES:
        v, g, dw = H.wn_case(R, C, dt)
        r = H.wn_fwd64(v, g)
        b = H.wn_fwd_bounds(r, dt)
        w, norm = H.wn_fwd_emulate32(v, g)
        tag = "weight_norm %s %dx%d " % (H.NAME[dt], R, C)
        _in(w, r["w"], b["w"], tag + "w")
        _in(norm, r["norm"], b["norm"], tag + "norm")
        assert bool((w[:, H.WN_G0] == 0).all())
        rb = H.wn_bwd64(v, g, dw, norm)
        bb = H.wn_bwd_bounds(rb, dt)
        dv, dg = H.wn_bwd_emulate32(v, g, dw, norm)
        _in(dv, rb["dv"], bb["dv"], tag + "dv")
        _in(dg, rb["dg"], bb["dg"], tag + "dg")
        assert float(rb["dot"][H.WN_ORTH].abs()) < 0.02 * float(rb["adot"][H.WN_ORTH]) or R == 1   # the orthogonal column: dot ~ 0 (R = 1 has no orthogonal complement)
        if (R, C) == H.WN_MODEL:
            continue
        for d in H.WN_FWD_DEFECTS:
            if d == "last_row_chunk_dropped" and R <= H.WN_CHUNK:
                continue
            wd, nd = H.wn_fwd_emulate32(v, g, defect=d)
            seen_out = _leaves(wd, r["w"], b["w"]) or (d != "norm_per_row" and _leaves(nd, r["norm"], b["norm"]))
            fseen.note(d, seen_out, tag)
        for d in H.WN_BWD_DEFECTS:
            if d == "last_row_chunk_dropped" and R <= H.WN_CHUNK:
                continue
            dvd, dgd = H.wn_bwd_emulate32(v, g, dw, norm, defect=d)
            bseen.note(d, _leaves(dvd, rb["dv"], bb["dv"]) or _leaves(dgd, rb["dg"], bb["dg"]), tag)
    fseen.check()
    bseen.check()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
@pytest.mark.parametrize("cols", H.CS_COLS)
def test_colsum(cols, dt):
    seen = Seen([d for d in H.CS_DEFECTS if d != "last_column_block_dropped" or cols > 128], dt)
    for rows in H.CS_ROWS:
        x = H.cs_case(rows, cols, dt)
        tag = "colsum %s %dx%d " % (H.NAME[dt], rows, cols)
        ref, b = H.colsum64(x, rows, cols, False)
        _in(H.colsum_emulate32(x, False), ref, b, tag + "atomic")
        for out_dt in DTS:
            ref, b = H.colsum64(x, rows, cols, True, out_dt)
            _in(H.colsum_emulate32(x, True, out_dt), ref, b, tag + "typed->" + H.NAME[out_dt])
        ref, b = H.colsum64(x, rows, cols, True, H.F)
        for d in ("tail_rows_dropped", "chunks_from_64_dropped", "last_column_block_dropped"):
            seen.note(d, _leaves(H.colsum_emulate32(x, True, H.F, defect=d), ref, b), tag)
        for which in H.CS_STAMPS[1:]:
            st, dead = H.cs_stamps(rows, which)
            xs = x.clone()
            xs[dead] = 0
            ref, b = H.colsum64(xs, rows, cols, True, H.F)
            _in(H.colsum_emulate32(xs, True, H.F, stamps=st), ref, b, tag + "live " + which)
            seen.note("stamp_off_by_one_tile", _leaves(H.colsum_emulate32(xs, True, H.F, stamps=st, defect="stamp_off_by_one_tile"), ref, b), tag + which)
        keep = H.keep_mask(H.CS_KEY, rows * cols, H.CS_P).view(rows, cols)
        xref, xb = H.dropout64(x, keep, H.CS_P)
        xd, s = H.colsum_emulate32(x, True, H.F, drop=(H.CS_KEY, H.CS_P))
        _in(xd, xref, xb, tag + "dropout_colsum xd")
        assert torch.equal(xd, H.dropout_emulate32(x, H.CS_KEY, H.CS_P))
        ref, b = H.colsum64(xd, rows, cols, True, H.F)          # the sums are DEFINED on the stored xd
        _in(s, ref, b, tag + "dropout_colsum sums")
        assert torch.equal(s, H.colsum_emulate32(xd, True, H.F))
        d = "sums_of_unrounded_product"
        seen.note(d, _leaves(H.colsum_emulate32(x, True, H.F, drop=(H.CS_KEY, H.CS_P), defect=d)[1], ref, b), tag)
    seen.check()


def test_colsum_shapes_reach_the_paths_they_name():
    rows = H.CS_ROWS[-1]
    for cols in H.CS_COLS:
        rows_per, nch = H.cs_grid(rows, cols, True)
        assert rows_per % 64 == 0 and nch > 64, "the reduce kernel's chunk loop needs more than 64 chunks"
    assert H._lane_steps(49, 0) == (1, 0) and H._lane_steps(49, 15) == (0, 3) and H._lane_steps(64, 15) == (1, 0)
    assert all(r % 64 >= 49 for r in (113, 127, rows))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_embed_forward(dt):
    seen = Seen(H.EF_DEFECTS, dt)
    scale_of = {C: C ** 0.5 for C in H.EF_COLS}
    for T in H.EF_T:
        for C in H.EF_COLS:
            tok, E, x, table = H.ef_inputs(T, C, dt)
            for form in H.EF_FORMS:
                args = H.ef_args(form, tok, E, x, table)
                for p in H.EF_PS:
                    ref, b = H.embed_fwd64(*args, scale_of[C], p, H.EF_KEY)
                    tag = "embed fwd %s T%d C%d %s p=%g" % (H.NAME[dt], T, C, form, p)
                    _in(H.embed_fwd_emulate32(*args, scale_of[C], p, H.EF_KEY), ref, b, tag)
                    if form == "tokens":
                        assert bool((ref[tok == H.PAD] == 0).all())
                    if form == "dense_no_table":
                        continue
                    for d in H.EF_DEFECTS:
                        if d == "dropout_index_per_row" and p == 0:
                            continue
                        seen.note(d, _leaves(H.embed_fwd_emulate32(*args, scale_of[C], p, H.EF_KEY, defect=d), ref, b), tag)
    seen.check()


def test_positions_follow_make_positions():
    from oracle import chimera_oracle as O
    for T in H.EF_T:
        tok = H.ef_tokens(T)
        assert torch.equal(H.make_positions(tok.ne(H.PAD), H.PAD), O.make_positions(tok, H.PAD))
        assert torch.equal(H.sinusoidal_table(H.PAD + 1 + T, 8, H.PAD), O.sinusoidal_table(H.PAD + 1 + T, 8, H.PAD))


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_embed_backward(dt):
    seen = Seen(H.EB_DEFECTS, dt)
    for n, C, V in H.EB_CASES:
        dy, tok = H.eb_inputs(n, C, V, dt)
        scale = C ** 0.5
        for gdt in ({dt, H.F}):
            for p in H.EB_PS:
                ref, b = H.embed_bwd64(dy, tok, V, scale, p, H.EB_KEY, gdt)
                tag = "embed bwd %s->%s n%d C%d V%d p=%g" % (H.NAME[dt], H.NAME[gdt], n, C, V, p)
                got = H.embed_bwd_emulate32(dy, tok, V, scale, p, H.EB_KEY, gdt)
                _in(got, ref, b, tag)
                unused = torch.ones(V, dtype=torch.bool)
                unused[tok] = False
                unused[H.PAD] = True
                assert int(unused.sum()) >= 3 and bool((got[unused] == 0).all()) and bool((b[unused] == 0).all())
                for d in H.EB_DEFECTS:
                    if d == "mask_of_wrong_row" and p == 0:
                        continue
                    seen.note(d, _leaves(H.embed_bwd_emulate32(dy, tok, V, scale, p, H.EB_KEY, gdt, defect=d), ref, b), tag)
    seen.check()


@pytest.mark.parametrize("dt", DTS, ids=IDS)
def test_contrastive(dt):
    fseen, bseen = Seen(H.CT_FWD_DEFECTS, dt), Seen(H.CT_BWD_DEFECTS, dt)
    names = ("loss", "rows", "sim", "na", "nt")
    for Bn, M, C in H.CT_SHAPES:
        for temp in H.CT_TEMPS:
            for zero_row in (False, True):
                a, t = H.ct_inputs(Bn, M, C, dt, zero_row=zero_row)
                r = H.ct_fwd64(a, t, temp)
                b = H.ct_fwd_bounds(r)
                out = dict(zip(names, H.ct_fwd_emulate32(a, t, temp)))
                tag = "contrastive %s %dx%dx%d temp=%g%s " % (H.NAME[dt], Bn, M, C, temp, " zero-row" if zero_row else "")
                for n in names:
                    _in(out[n], r[n], b[n], tag + n)
                if zero_row:      # the clamp max(|a||t|, 1e-8): cosine 0 against every slot, everything finite
                    assert bool(r["clamped"].any()) and bool((out["sim"][-1, M - 1] == 0).all()) and bool((out["sim"][-1, :, 0] == 0).all())
                    da, dtt = H.ct_bwd_emulate32(a, t, out["sim"], out["na"], out["nt"], 0.7, temp)
                    assert bool(torch.isfinite(da.float()).all()) and bool(torch.isfinite(dtt.float()).all())
                    continue
                for d in H.CT_FWD_DEFECTS:
                    od = dict(zip(names, H.ct_fwd_emulate32(a, t, temp, defect=d)))
                    fseen.note(d, _leaves(od["loss"], r["loss"], b["loss"]) or _leaves(od["sim"], r["sim"], b["sim"]), tag)
                for gs in H.CT_GSCALES:
                    rb = H.ct_bwd64(a, t, out["sim"], out["na"], out["nt"], gs, temp)
                    bb = H.ct_bwd_bounds(rb, dt)
                    da, dtt = H.ct_bwd_emulate32(a, t, out["sim"], out["na"], out["nt"], gs, temp)
                    _in(da, rb["da"], bb["da"], tag + "da g=%g" % gs)
                    _in(dtt, rb["dt"], bb["dt"], tag + "dt g=%g" % gs)
                    for d in H.CT_BWD_DEFECTS:
                        dad, dtd = H.ct_bwd_emulate32(a, t, out["sim"], out["na"], out["nt"], gs, temp, defect=d)
                        bseen.note(d, _leaves(dad, rb["da"], bb["da"]) or _leaves(dtd, rb["dt"], bb["dt"]), tag + "g=%g" % gs)
    fseen.check()
    bseen.check()


def test_contrastive_inputs_hold_the_pairs_they_name():
    a, t = H.ct_inputs(2, 8, 64, H.F)
    r = H.ct_fwd64(a, t, 0.1)
    assert 0.0 < 1.0 - float(r["sim"][0, 0, 0]) < 3e-6 and 0.0 < 1.0 + float(r["sim"][0, 1, 1]) < 3e-6
    assert float(r["na"][0, 2]) > 1e3 and float(r["nt"][0, 3]) < 3e-2


def test_embed_backward_tokens_reach_the_owner_search():
    tok = H.eb_tokens(700, 40)
    for sym, first in ((35, 300), (36, 260)):
        where = torch.nonzero(tok == sym).reshape(-1).tolist()
        assert where[0] == first >= 256 and len(where) == 2
    gaps = [int(torch.nonzero(tok == s).reshape(-1)[-1] - torch.nonzero(tok == s).reshape(-1)[0]) for s in range(2, 35) if bool((tok == s).any())]
    assert max(gaps) > 256

"""The bounds of posconv_ref.py are sound and sharp, shown without a GPU.
  * the fp64 restatements equal torch's grouped conv1d and its autograd in fp64 to 1e-12 (tail3, full4, k127, nkb5, many_utts: odd
    and even k, more than one frame block, T < k);
  * the table of cases reaches the paths its comments name: nkb, ntb, the stage count and the item counts are derived from the kernel's
    constants and asserted here, so a changed constant fails this test instead of silently moving a case off its path;
  * on every case both fp32 emulation shapes ("seq": a sequential chain in K order; "chunk16": 16 products exact, one rounding per
    chunk) lie inside the bounds on EVERY element.  Every case runs whole, no channel slice; the rows of past_list with zero dz are
    skipped, exactly;
  * every listed defect leaves the bounds on at least one element in the case pinned for it (posconv_ref.FWD_DEFECT_CASE /
    DW_DEFECT_CASE), in which the faithful emulation has just passed;
  * the bounds are below the tolerance test_posconv_window_gpu.py uses (2e-2 max|ref| + 2e-2 |ref|) on every element of k128 and blocks3.
The GELU restatement is checked against its constants in test_norm_ref_cpu.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import posconv_ref as R

_case = R.case


@functools.lru_cache(maxsize=None)
def _refs(name, lens=None):
    c = _case(name, lens)
    z, y = R.fwd64(c["x"], c["w"], c["bias"], c["G"], lens)
    dw, db = R.dw64(c["dz"], c["x"], c["G"], c["k"])
    ref = dict(z=z, y=y, dx=R.dx64(c["dz"], c["w"], c["dy"], c["G"]), dw=dw, db=db)
    b = dict(R.fwd_bounds(c["x"], c["w"], c["bias"], c["G"]))
    b.update(R.dx_bounds(c["dz"], c["w"], c["dy"], c["G"]))
    b.update(R.dw_bounds(c["dz"], c["x"], c["G"], c["k"]))
    return ref, b


@functools.lru_cache(maxsize=None)
def _dw_refs(name, lens=None):
    c = _case(name, lens)
    dw, db = R.dw64(c["dz"], c["x"], c["G"], c["k"])
    return dict(dw=dw, db=db), R.dw_bounds(c["dz"], c["x"], c["G"], c["k"])


def _in(got, ref, bound, what):
    ratio, bad = R.worst_ratio(got, ref, bound)
    print("clean %-40s worst err/bound %.3f" % (what, ratio))
    assert bad == 0, "%s: the faithful emulation leaves the bound on %d elements (worst ratio %.3f)" % (what, bad, ratio)


def _out(got, ref, bound, what):
    err = (got.double() - ref.double()).abs()
    n = int((err > bound.expand_as(err)).sum())
    print("defect %-52s outside on %d of %d" % (what, n, err.numel()))
    return n


def test_inputs_are_bf16_exact_without_subnormals():
    for name in R.CASES:
        c = R.case(name)
        for key in ("x", "w", "bias", "dy", "dz"):
            v = c[key]
            assert v.dtype == torch.bfloat16 and bool(torch.isfinite(v.float()).all())
            nz = v.float().abs()[v != 0]
            assert float(nz.min()) >= 2.0 ** -126, (name, key)
    c = R.case("k127", R.LIMITS["k127"])
    assert not bool(c["x"][1, 100:].any()) and not bool(c["dz"][2].any()) and bool(c["x"][1, 99].any())
    # the edge frames are four times larger: the largest |x| of frames 0 .. 3 is above every interior frame's typical size
    c = R.case("k128")
    assert float(c["x"][0, :4].float().abs().mean()) > 3.0 * float(c["x"][0, 4:-4].float().abs().mean())


def test_case_table_reaches_its_paths():
    g = {n: R.geometry(*R.CASES[n]) for n in R.CASES}
    assert set(R.FWD_CASES) | set(R.DW_ONLY_CASES) == set(R.CASES)
    assert {n: (v["nkb"], v["ntb"]) for n, v in g.items()} == {
        "one": (1, 1), "tail3": (1, 1), "full4": (3, 1), "full4p1": (3, 1), "k126": (16, 16), "k127": (16, 16), "k128": (5, 16),
        "blocks3": (33, 16), "nkb2": (2, 1), "nkb5": (5, 2), "wrap": (7, 2), "remap9": (2, 3), "many_utts": (2, 1), "past_list": (1032, 1)}
    assert all(G * R.CG <= 144 and 1 <= k <= R.KMAX for (_, _, G, k) in R.CASES.values())
    # forward / dX: stage loop
    assert g["one"]["nst"] == 1 and g["one"]["tail"] == 1 and g["one"]["padl"] == 0 and g["one"]["lp"] == 0 and g["one"]["fwd_items"] == 1
    assert g["tail3"]["nst"] == 1 and g["tail3"]["tail"] == 3
    assert R.CASES["many_utts"][1] < R.CASES["many_utts"][3]   # T < k
    assert g["full4"]["nst"] == 1 and g["full4"]["tail"] == 0 and (g["full4"]["padl"], g["full4"]["lp"]) == (2, 1)
    assert g["full4p1"]["nst"] == 2 and g["full4p1"]["tail"] == 1
    assert g["k126"]["tail"] == 2 and g["k127"]["tail"] == 3 and g["k128"]["tail"] == 0
    # frame blocks and the item remap
    assert R.CASES["k126"][1] == R.FBM and g["k126"]["nblk"] == 1
    assert R.CASES["k127"][1] == R.FBM + 1 and g["k127"]["nblk"] == 2 and (g["k127"]["fwd_items"], g["k127"]["fwd_r8"]) == (12, 4)
    assert (g["k128"]["fwd_items"], g["k128"]["fwd_n8"]) == (2, 0)
    assert (g["blocks3"]["nblk"], g["blocks3"]["fwd_items"], g["blocks3"]["fwd_n8"], g["blocks3"]["fwd_r8"]) == (3, 27, 3, 3)
    assert g["blocks3"]["dw_items"] == 48
    # a dead block behind a live one, and an utterance with nothing live
    for name, lens in R.LIMITS.items():
        T, k = R.CASES[name][1], R.CASES[name][3]
        m_len = [min(n + k // 2, T) for n in lens]
        assert lens[0] == T and 0 < m_len[1] <= (g[name]["nblk"] - 1) * R.FBM and lens[2] == 0
    # dW: tap blocks and the store
    assert [g[n]["ntb"] for n in ("one", "tail3", "full4", "nkb2", "nkb5", "wrap", "k126", "k128")] == [1, 1, 1, 1, 2, 2, 16, 16]
    assert R.CASES["nkb2"][3] == R.DTJ and R.CASES["nkb5"][3] == R.DTJ + 1
    assert R.CASES["k126"][3] % 2 == 0 and R.CASES["k126"][3] % 8 == 6
    # dW: the K-block ring
    assert g["one"]["nkb"] == 1 and g["one"]["Tp"] == 1 and g["one"]["magic"] == 0
    assert g["nkb2"]["nkb"] == 2 < R.DNS - 1
    assert g["nkb5"]["nkb"] == R.DNS - 1
    assert g["wrap"]["nkb"] == R.DNS + 1          # iteration 1 issues block 6 into stage 6 % DNS = 0
    assert g["many_utts"]["Tp"] == 3 and 64 // g["many_utts"]["Tp"] == 21
    assert g["past_list"]["nkb"] == 1032 > R.DKLIST
    # dW: the item remap
    assert (g["wrap"]["dw_items"], g["wrap"]["dw_n8"]) == (6, 0) and g["nkb2"]["dw_items"] == 1
    assert g["k127"]["dw_items"] == 32 and g["full4p1"]["dw_items"] % 8 == 3
    assert (g["remap9"]["dw_items"], g["remap9"]["dw_n8"], g["remap9"]["dw_r8"]) == (9, 1, 1)
    # past_list: blocks past the list carry weight, in both runs the stamps would matter if they were read
    T, k = R.CASES["past_list"][1], R.CASES["past_list"][3]
    assert (g["past_list"]["Tp"] + T - R.PAST_LIST_LIVE[1]) // 64 > R.DKLIST
    st = R.k_block_stamps(2, T, k, R.PAST_LIST_ROWS)
    assert st.numel() == 1032 and 0 < int(st.sum()) < 10
    assert int(R.k_block_stamps(2, 190, 16, (0, 0)).sum()) == 0 and R.k_block_stamps(2, 190, 16, (0, 0)).numel() == 7


@pytest.mark.parametrize("name", ["tail3", "full4", "k127", "nkb5", "many_utts"])
def test_restatements_equal_conv1d_autograd(name):
    c = R.case(name)
    G, k = c["G"], c["k"]
    x, w, b = (c[n].double().requires_grad_(True) for n in ("x", "w", "bias"))
    conv = F.conv1d(x.transpose(1, 2), w, b, padding=k // 2, groups=G)
    if k % 2 == 0:
        conv = conv[:, :, :-1]
    conv = conv.transpose(1, 2)
    yt = x + F.gelu(conv)
    (conv * c["dz"].double()).sum().backward()
    z, y = R.fwd64(c["x"], c["w"], c["bias"], G)
    dx = R.dx64(c["dz"], c["w"], c["dy"], G)
    dw, db = R.dw64(c["dz"], c["x"], G, k)

    def close(a, ref, what):
        err = float((a - ref).abs().max())
        assert err <= 1e-12 * max(float(ref.abs().max()), 1e-30), "%s %s: %.3e" % (name, what, err)
    close(z, conv.detach(), "z")
    close(y, yt.detach(), "y")
    close(dx - c["dy"].double(), x.grad, "dx")
    close(dw, w.grad, "dw")
    close(db, b.grad, "db")


def test_gelu_bound_is_the_first_line_of_norm_ref():
    z = torch.linspace(-7.0, 7.0, 57, dtype=torch.float64)
    b_z = torch.full_like(z, 1e-3)
    whole = R._gelu_out_bound(z, b_z, R.BF)
    mine = R._store(R._gelu_bound(z, b_z), R.gelu64(z), R.BF) + R.ETA
    assert float((whole - mine).abs().max()) <= 1e-15


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("name,lens", [(n, None) for n in R.FWD_CASES] + list(R.LIMITS.items()), ids=lambda v: str(v))
def test_forward_and_dx_emulations_stay_inside(name, lens, shape):
    c = _case(name, lens)
    ref, b = _refs(name, lens)
    z, y = R.fwd_emulate32(c["x"], c["w"], c["bias"], c["G"], lens, shape)
    dx = R.dx_emulate32(c["dz"], c["w"], c["dy"], c["G"], lens, shape)
    tag = "%s %s%s " % (shape, name, "" if lens is None else " limited")
    _in(z, ref["z"], b["z"], tag + "z")
    _in(y, ref["y"], b["y"], tag + "y")
    _in(dx, ref["dx"], b["dx"], tag + "dx")
    if lens is not None:   # the limited call is the unlimited call on these inputs, bit for bit
        z0, y0 = R.fwd_emulate32(c["x"], c["w"], c["bias"], c["G"], None, shape)
        assert torch.equal(z0, z) and torch.equal(y0, y)
        assert torch.equal(R.dx_emulate32(c["dz"], c["w"], c["dy"], c["G"], None, shape), dx)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("name,lens", [(n, None) for n in R.FWD_CASES + R.DW_ONLY_CASES] + list(R.LIMITS.items())
                         + [("past_list", R.PAST_LIST_ROWS), ("wrap", (0, 0))], ids=lambda v: str(v))
def test_dw_emulation_stays_inside(name, lens, shape):
    c = _case(name, lens)
    ref, b = _dw_refs(name, lens)
    dw, db = R.dw_emulate32(c["dz"], c["x"], c["G"], c["k"], shape)
    tag = "%s %s%s " % (shape, name, "" if lens is None else " limited")
    _in(dw, ref["dw"], b["dw"], tag + "dw")
    _in(db, ref["db"], b["db"], tag + "db")
    if lens == (0, 0):
        assert not bool(dw.any()) and not bool(db.any()) and float(b["dw"].max()) == 0.0 and float(b["db"].max()) == 0.0


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("defect", R.FWD_DEFECTS)
def test_forward_and_dx_defects_leave_the_bounds(defect, shape):
    name, lens = R.FWD_DEFECT_CASE[defect]
    c = _case(name, lens)
    ref, b = _refs(name, lens)
    z, y = R.fwd_emulate32(c["x"], c["w"], c["bias"], c["G"], lens, shape, defect)
    tag = "%s %s %s " % (shape, name, defect)
    # bias_after_gelu and residual_missing leave z as it is: y is what they are judged on
    out_y = _out(y, ref["y"], b["y"], tag + "y")
    out_z = _out(z, ref["z"], b["z"], tag + "z")
    assert out_y >= 1, tag + "stays inside the bound of y"
    if defect not in ("bias_after_gelu", "residual_missing"):
        assert out_z >= 1, tag + "stays inside the bound of z"
    if defect in R.DX_DEFECTS:
        dx = R.dx_emulate32(c["dz"], c["w"], c["dy"], c["G"], lens, shape, defect)
        assert _out(dx, ref["dx"], b["dx"], tag + "dx") >= 1, tag + "stays inside the bound of dx"


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("defect", R.DW_DEFECTS)
def test_dw_defects_leave_the_bounds(defect, shape):
    name, lens = R.DW_DEFECT_CASE[defect]
    c = _case(name, lens)
    ref, b = _dw_refs(name, lens)
    dw, db = R.dw_emulate32(c["dz"], c["x"], c["G"], c["k"], shape, defect)
    tag = "%s %s %s " % (shape, name, defect)
    out_dw, out_db = _out(dw, ref["dw"], b["dw"], tag + "dw"), _out(db, ref["db"], b["db"], tag + "db")
    if defect.startswith("db_"):
        assert out_db >= 1 and out_dw == 0, tag + "db"
    elif defect in ("last_k_block_dropped", "blocks_past_1024_dropped"):
        assert out_dw >= 1 and out_db >= 1, tag
    else:   # a shifted or leaking window leaves the column sums of dz alone
        assert out_dw >= 1, tag + "dw"


def test_every_defect_has_a_case():
    assert set(R.FWD_DEFECT_CASE) == set(R.FWD_DEFECTS) and set(R.DW_DEFECT_CASE) == set(R.DW_DEFECTS)
    for d, (name, _) in R.FWD_DEFECT_CASE.items():
        B, T, G, k = R.CASES[name]
        assert name in R.FWD_CASES
        assert d != "next_group_channels" or G >= 2
        assert d != "second_block_reads_first_window" or T > R.FBM
        assert d != "tail_stage_dropped" or k % R.TAPS
        assert d not in ("window_one_frame_late", "even_k_keeps_last_frame_drops_first") or (k % 2 == 0 and k - 1 - k // 2 >= 1)
    for d, (name, _) in R.DW_DEFECT_CASE.items():
        B, T, G, k = R.CASES[name]
        assert d not in ("tap_block_offset_ignored", "db_from_every_tap_block") or k > R.DTJ
        assert d != "lp_is_k_half" or k % 2 == 0
        assert d != "frames_leak_across_utterances" or B >= 2


@pytest.mark.parametrize("name", ["k128", "blocks3"])
def test_bounds_are_tighter_than_the_old_tolerance(name):
    """bound / (2e-2 max|ref| + 2e-2 |ref|), the check() of test_posconv_window_gpu.py, per element: median and maximum."""
    c = R.case(name)
    z, y = R.fwd64(c["x"], c["w"], c["bias"], c["G"])
    dw, db = R.dw64(c["dz"], c["x"], c["G"], c["k"])
    ref = dict(z=z, y=y, dx=R.dx64(c["dz"], c["w"], c["dy"], c["G"]), dw=dw, db=db)
    b = dict(R.fwd_bounds(c["x"], c["w"], c["bias"], c["G"]))
    b.update(R.dx_bounds(c["dz"], c["w"], c["dy"], c["G"]))
    b.update(R.dw_bounds(c["dz"], c["x"], c["G"], c["k"]))
    for q in ("z", "y", "dx", "dw", "db"):
        old = 2e-2 * float(ref[q].abs().max()) + 2e-2 * ref[q].abs()
        r = (b[q] / old).reshape(-1)
        print("TIGHT posconv %-8s %-3s bound / old tolerance: median %.4f  max %.4f" % (name, q, float(r.median()), float(r.max())))
        assert float(r.max()) < 1.0, (name, q, float(r.max()))

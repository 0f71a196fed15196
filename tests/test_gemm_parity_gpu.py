"""cst_gemm on a real MI355X against gemm_ref.py, on every launch arm gemm_route returns without the experiment hook: exact cases bit
for bit against the fp64 reference's bits (integer operands: no rounding before the one store), bounded cases (GELU, GELU', a general
alpha, full-mantissa fp32 operands) under counted bounds.  Every launch goes through kernels.gemm with nothing forced; C, aux_out and
the column sums are prefilled with NaN, the gaps of strided outputs with a sentinel that must survive.  Run with -s for the ratios."""
import os
from importlib import import_module

import pytest
import torch

import gemm_ref as G
from conftest import load_pkg
from test_gemm_route_cpu import route_of

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in G.CASES]


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")


def dev(t, dt):
    return None if t is None else t.to(dt).cuda()


def device_operands(o, all_dead=False):
    d = dict(a=dev(o["a"], o["dt"]), b=dev(o["b"], o["dt"]), bias=dev(o["bias"], o["dt"]), resid=dev(o["resid"], o["dt"]),
             aux_in=dev(o["aux_in"], o["dt"]))
    if all_dead:
        d["a"].zero_()
    every = lambda n: range((n + 63) // 64)  # noqa: E731
    d["k_live"] = None if o["dead_k"] is None else (G.stamps(every(o["K"]) if all_dead else o["dead_k"], o["K"]).cuda(), G.EPOCH)
    d["m_live"] = None if o["dead_m"] is None else (G.stamps(every(o["M"]) if all_dead else o["dead_m"], o["M"]).cuda(), G.EPOCH)
    lim = lambda v: None if v is None else torch.tensor([0] * len(v) if all_dead else list(v), dtype=torch.int32).cuda()  # noqa: E731
    d["k_len"], d["m_len"] = lim(o["k_len"]), lim(o["m_len"])
    return d


def outputs(o):
    """The outputs of one launch on the device: NaN where it must write, the sentinel where it must not."""
    out = {"C": G.prefill(o, o["cdt"]).cuda()}
    if o["aux_out"]:
        out["aux_out"] = G.prefill(o, o["dt"]).cuda()
    if o["colsum"]:
        out["colsum"] = torch.full((o["nb"], o["M"]), float("nan"), dtype=o["dt"], device="cuda")
    return out


def launch(K, o, d, skips=True, defer=False, out=None):
    """One launch of the case through kernels.gemm.  skips=False: without the live stamps / row limits.  out: outputs() made earlier
    (nothing but the launch itself then happens here).  -> {C, aux_out, colsum}."""
    k, L = K
    out = out if out is not None else outputs(o)
    ld = o["ldc"]
    k.gemm(d["a"], d["b"], out["C"], o["M"], o["N"], o["K"], a_kmajor=o["ak"], b_kmajor=o["bk"], lda=o["lda"], ldb=o["ldb"], ldc=ld,
           bias=d["bias"], bias_mode=o["bias_mode"], act=o["act"], aux_out=out.get("aux_out"), ld_aux_out=ld if o["aux_out"] else 0,
           dact=o["dact"], aux_in=d["aux_in"], ld_aux_in=ld if o["dact"] else 0, resid=d["resid"], ld_resid=ld if d["resid"] is not None else 0,
           alpha=o["alpha"], batch0=o["b0"], batch1=o["b1"], sa=o["sa"], sb=o["sb"], sc=o["sc"], sbias=o["sbias"], a_seg=o["a_seg"],
           a_seg_stride=o["a_seg_stride"], split_k=o["split_k"], drop_p=o["drop_p"], drop_key=G.DROP_KEY,
           k_live=d["k_live"] if skips else None, m_live=d["m_live"] if skips else None, k_len=d["k_len"] if skips else None,
           m_len=d["m_len"] if skips else None, colsum=out.get("colsum"), defer=defer)
    return out


def same_bits(x, y):
    iv = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
    return torch.equal(x.view(iv), y.view(iv))


def assert_bits(name, got, want, what=""):
    """Every output equals the expected bits; the message carries the mismatch map a diagnosis starts from."""
    o, route = G.operands(name), G.BY_NAME[name]["route"]
    for key in ("C", "aux_out", "colsum"):
        if key not in want:
            continue
        w = want[key].cuda()
        if same_bits(got[key], w):        # (an integer view: the sign of a zero is part of the bits)
            continue
        if key == "colsum":
            bad = (~(got[key] == w)).nonzero()
            msg = "%d of %d differ; first %s" % (len(bad), w.numel(), [(int(z), int(m), float(got[key][z, m]), float(w[z, m])) for z, m in bad[:6]])
        else:
            msg = G.mismatch_report(got[key], want[key], o, route)
        zeros = int(((got[key] == w) & (torch.signbit(got[key]) != torch.signbit(w))).sum())
        pytest.fail("%s %s %s (%s): %s; %d more differ only in the sign of a zero" % (name, what, key, route, msg, zeros))


def check_route(K, name):
    c = G.BY_NAME[name]
    got = route_of(K[1], K[1].load(), c["row"])
    assert got == c["route"], "case %s no longer reaches its arm: %r routes to %r, not %r" % (name, c["row"], got, c["route"])


@pytest.mark.parametrize("name", NAMES)
def test_case(K, name):
    check_route(K, name)
    o, ex = G.operands(name), G.expected(name)
    d = device_operands(o)
    got, again = launch(K, o, d), launch(K, o, d)
    torch.cuda.synchronize()
    if o["kind"] == "exact":
        assert_bits(name, got, ex)
    else:
        bd = G.bounds(name, ex)
        for key, b in bd.items():
            g = got[key].cpu()
            if key != "colsum":
                gaps = G.prefill(o, g.dtype) == G.SENT
                assert torch.equal(g[gaps], torch.full_like(g[gaps], G.SENT)), (name, key, "the launch wrote outside its output")
                g = G.c_stack(o, g)
            r, bad = G.worst_ratio(g, ex["v64"][key], b)
            print("RATIO %s %s worst err/bound %.4f" % (name, key, r))
            assert bad == 0 and r <= 1.0, (name, key, r, bad)
    for key in got:
        assert same_bits(got[key], again[key]), (name, key, "two launches differ")


STATES = [(0, False), (216, False), (248, False), (248, True)]   # (reserved CUs, CST_GEMM8P_NO_HALVES)


@pytest.mark.parametrize("name", ["8p_kk_plain", "8p_km_plain", "8p_kk_resid", "8p_km_resid"])
def test_8p_scheduling_states_on_one_problem(K, name):
    """One round static; 40 CUs: claims without halves; 8 CUs: the remainder tile as two half items, claims; the same without halves.
    Every state gives the expected bits, hence the states give each other's."""
    k, L = K
    lib = L.load()
    check_route(K, name)
    o, ex = G.operands(name), G.expected(name)
    d = device_operands(o)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    prev = lib.cst_gemm_reserve_cus(-1)
    try:
        for reserved, no_halves in STATES:
            st = G.launch8p_state(o["M"], o["N"], 1, 1, False, ncu=ncu, reserved=reserved, no_halves=no_halves)
            print("STATE %s reserved %d no_halves %d: %s" % (name, reserved, no_halves, st))
            if ncu == 256:
                want = {(0, False): (False, None), (216, False): (True, None), (248, False): (True, 224), (248, True): (True, None)}[(reserved, no_halves)]
                assert (st["claims"], st["half_from"]) == want, st
            lib.cst_gemm_reserve_cus(reserved)
            if no_halves:
                os.environ["CST_GEMM8P_NO_HALVES"] = "1"
            try:
                got = launch(K, o, d)
                torch.cuda.synchronize()
            finally:
                os.environ.pop("CST_GEMM8P_NO_HALVES", None)
            assert_bits(name, got, ex, "reserved %d no_halves %d" % (reserved, no_halves))
    finally:
        lib.cst_gemm_reserve_cus(prev)


SKIPS = {"reg_km_mlen": "gemm_m_len", "8p_kk_mlive_resid": "gemm_m_live", "8p_kk_mlive_bias": "gemm_m_live", "narrowm_klive": "gemm_k_live", "large_colsum_klive": "gemm_k_live", "reg_klen_split1": "gemm_k_len", "reg_klen_split2": "gemm_k_len",
         "reg_km_mlive": "gemm_m_live", "glds_mlive": "gemm_m_live", "8p_kk_tail_mlive": "gemm_m_live", "4w_mlive_resid": "gemm_m_live",
         "glds_narrown": "gemm_m_len", "8p_mrot": "gemm_m_len", "8p_gperm": "gemm_m_len"}


@pytest.mark.parametrize("name", sorted(SKIPS))
def test_skips_under_their_contracts(K, name):
    """The launch told what is zero in A and the launch not told give the same expected bits; with everything dead, exactly the
    epilogue of zero; the STATS counters show that the operand went into the descriptor."""
    k, L = K
    check_route(K, name)
    o, ex = G.operands(name), G.expected(name)
    d = device_operands(o)
    n0 = k.STATS.get(SKIPS[name], 0)
    told, untold = launch(K, o, d), launch(K, o, d, skips=False)
    torch.cuda.synchronize()
    assert k.STATS.get(SKIPS[name], 0) == n0 + 1
    assert_bits(name, told, ex, "with the operand")
    assert_bits(name, untold, ex, "without the operand")
    dead = launch(K, o, device_operands(o, all_dead=True))
    torch.cuda.synchronize()
    assert k.STATS.get(SKIPS[name], 0) == n0 + 2
    assert_bits(name, dead, G.expected_all_dead(name), "everything dead")


@pytest.mark.parametrize("name", ["reg_mm_split8", "reg_mm_colsum_split8"])
def test_deferred_reduce_gives_the_expected_bits(K, name):
    k, L = K
    check_route(K, name)
    o, ex = G.operands(name), G.expected(name)
    d = device_operands(o)
    flushes = k.DEFER.flushes
    with k.deferred_reductions(True):
        got = launch(K, o, d, defer=True)
        assert len(k.DEFER.items) == (2 if o["colsum"] else 1)      # the slabs (and the slice sums) wait for the flush
    torch.cuda.synchronize()
    assert k.DEFER.flushes == flushes + 1
    assert_bits(name, got, ex, "deferred")


def test_two_streams_keep_the_bits(K):
    """The 272-tile persistent launch (claimed items, half-height tail) in flight on two streams, four launches each: the eight outputs
    are made and prefilled before the first launch, and the eight launches are queued back to back with no host work between them, so
    that launches of both streams are on the device together and draw their claim counters from the launcher's ring at the same time.
    Every one of the eight outputs has the expected bits."""
    name = "8p_kk_tail"
    check_route(K, name)
    o, ex = G.operands(name), G.expected(name)
    st = G.launch8p_state(o["M"], o["N"], 1, 1, False, ncu=torch.cuda.get_device_properties(0).multi_processor_count)
    assert st["claims"], st
    d = device_operands(o)
    launch(K, o, d)                       # (first use: the launcher allocates its ring of scheduling slots, synchronously)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [outputs(o) for _ in range(8)]
    torch.cuda.synchronize()
    for i in range(4):
        with torch.cuda.stream(s1):
            launch(K, o, d, out=outs[2 * i])
        with torch.cuda.stream(s2):
            launch(K, o, d, out=outs[2 * i + 1])
    torch.cuda.synchronize()
    for i, got in enumerate(outs):
        assert_bits(name, got, ex, "stream %d launch %d" % (1 + i % 2, i // 2))

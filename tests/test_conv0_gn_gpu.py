"""cst_conv0_gn_gelu_fwd / _bwd on a real MI355X against the fp64 restatements of conv0_gn_ref.py, under ITS per-element bounds (counted
from the operation sequences of csrc/conv0.hip; no constant was fitted to an output of a kernel or of an emulation;
test_conv0_gn_ref_cpu.py shows that a faithful fp32 evaluation stays inside them, that every listed defect leaves them and that they
are not vacuous).  y (over the frames below the limit), mean, rstd and gram are outputs in their own right; dW, dgamma and dbeta are
held against a reference that is a function of the DEVICE's mean, rstd and gram.  B = 8, one utterance of each kind, frame limits
none, L, L + 5, 2049, 2048, 700, 7, 0 by utterance; dy is exactly zero from the limit on.

Which case reaches which launch (k s C, dtype, L):
  conv0_gram_kernel<10>             every k = 10 case;  two blocks at L = 2049, one at L <= 2048, the cap of 64 blocks and a ninth, partial
                                    grid-stride iteration at 10 5 8 f32 L = 64 * 2048 + 300 (B = 1)
  conv0_gram_kernel<16>             3 2 32, 16 7 72 (k = KMAX), 1 1 8, 2 2 512, and the LDS-envelope cases
  conv0_stats_kernel<float|bf16>    every case; two blocks over the channels from C = 512, one below
  conv0_fwd_reg_kernel<float, 10>   10 5 {512, 64, 8, 1024} f32: frames in flight 2, 16, 128, 1
  conv0_fwd_reg_kernel<bf16, 10>    10 5 {512, 64, 8, 1024} bf16
  conv0_fwd_kernel<float|bf16>      10 5 24 (k = 10, but C / 4 = 6 does not divide 256: cvecs = 3), 3 2 32, 16 7 72, 1 1 8, 2 2 512, both dtypes
  conv0_bwd_mfma_kernel             10 5 512 bf16: L = 2049 (a second block holding ONE frame), L = 2048 (one full block: the u operand of
                                    the last step reads taps beyond the staged span, into the zero strip), L = 15 with B = 33 (a single,
                                    partial 16-frame step: the buffer descriptor's range check stands in for all tail code); the limits 700
                                    and 7 end in the middle of a step, 0 and 2048 at a step's edge
  conv0_bwd_reg_kernel<float, 10>   10 5 {512, 64, 8, 1024} f32
  conv0_bwd_reg_kernel<bf16, 10>    10 5 {64, 8, 1024} bf16; at C = 512 behind CST_CONV0_NO_MFMA (read once into a static: not flipped here) and at
                                    10 17 512 bf16, where the MFMA kernel's LDS request no longer fits a CU
  conv0_bwd_kernel<float|bf16>      the cases of conv0_fwd_kernel: tpc = 85 (one idle thread), 64, 28, 256, 4 threads per channel vector
  conv0_bwd_reduce_kernel           every case; two blocks per utterance from L = 2049
  conv0_bwd_finish_kernel           every case; its second pass of 32 utterances, with one utterance in it, at B = 33
  the LDS envelope                  test_lds_envelope_*: the generic launches at the largest accepted requests, and the refusals

Dynamic LDS of the generic launches, from the launch code: forward 4 (k C + C + 64 stride + k), backward 4 (k C + 4 C + 2048 stride + k)
bytes, no static LDS.  What the runtime grants a kernel that has not raised hipFuncAttributeMaxDynamicSharedMemorySize is not stated by
HIP beyond 64 KiB; conv0_bwd_mfma_kernel has always been launched with 65952 bytes without it, so this runtime grants more, up to
what the part has — which is why the corner went unnoticed.  Now the entry points raise the attribute whenever a request is above 64 KiB
and refuse, before the Gram pass, whatever is above the 160 KiB of a CU (also a register-path stride so large that its staged span does
not fit): the accepted and the launchable envelope are the same.

Worst err/bound per path, as measured on an MI355X (pytest -s prints one `RATIO` line per output and case; every kernel is inside):
  statistics (all cases)    gram 0.165 (B = 33, L = 15)   mean 0.096   rstd 0.807 (where var << eps the bound is the one rounding of the store)
  forward  register         y 0.440 f32 (10 5 512)   0.969 bf16 (the half-ulp of the bf16 store against UBF |y|)
  forward  generic          y 0.469 f32 (2 2 512)    0.972 bf16 (16 7 72)
  backward register  f32    dW 0.005   dgamma 0.009   dbeta 0.007 (10 5 1024, L = 300: fp = 1, the longest thread chain per frame)
  backward register  bf16   dW 0.036   dgamma 0.081   dbeta 0.060 (10 5 1024)
  backward generic   f32    dW 0.048   dgamma 0.036   dbeta 0.031 (15 5 1616 and 14 1 2048, L = 37)
  backward generic   bf16   dW 0.298   dgamma 0.318   dbeta 0.283 (the same)
  backward MFMA      bf16   dW 0.116   dgamma 0.103   dbeta 0.077 (L = 15, B = 33);  0.081 / 0.025 / 0.014 at L = 2049
(Measured before the 10 17 512 bf16 case was added; that case passed in the run of the whole suite, its figures are not among these.)
(The backward figures are small because the bounds are worst-case sums over up to 16392 frames whose rounding errors add like a random
walk; at L = 37 they reach a third.)"""
from importlib import import_module

import pytest
import torch

import conv0_gn_ref as R
import norm_ref as N
from conftest import load_pkg
from test_norm_gpu import cu, within

pytestmark = pytest.mark.gpu
FWD_OUT = ("y", "mean", "rstd", "gram")
BWD_OUT = ("dW", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def K():
    load_pkg()
    return import_module("chimera-st_amd.kernels"), import_module("chimera-st_amd.lib")


def _run(k, cs, backward=True, alone=(1, 3, 6)):
    c = R.case(*cs)
    kk, st, dt, Bn, L = c["k"], c["stride"], c["dt"], c["Bn"], c["L"]
    tag = "conv0_gn %s " % c["route"]
    wav, w, gamma, beta, dy, lim = cu(c["wav"], c["w"], c["gamma"], c["beta"], c["dy"], c["limit"])
    r = R.fwd64(c["wav"], c["w"], c["gamma"], c["beta"], kk, st)
    b = R.fwd_bounds(r, dt)
    out = k.conv0_fwd(wav, w, gamma, beta, kk, st, R.EPS, frame_limit=lim)
    live = R.live_of(c["limit"], Bn, L)
    host = [o.cpu() for o in out]
    within(host[0][live], r["y"][live], b["y"][live], tag + "y      " + cs[0])
    for n, o in zip(FWD_OUT[1:], host[1:]):
        within(o, r[n], b[n], tag + "%-7s" % n + cs[0])
    again = k.conv0_fwd(wav, w, gamma, beta, kk, st, R.EPS, frame_limit=lim)
    assert torch.equal(again[0].cpu()[live], host[0][live]) and all(torch.equal(a, o) for a, o in zip(again[1:], out[1:])), "the forward is not bit-reproducible"
    for bi in (i for i in alone if i < Bn):    # utterance bi alone gives the bits of its rows in the batch
        one = k.conv0_fwd(wav[bi:bi + 1].contiguous(), w, gamma, beta, kk, st, R.EPS, frame_limit=lim[bi:bi + 1].contiguous())
        assert torch.equal(one[0].cpu()[0][live[bi]], host[0][bi][live[bi]]), "y of utterance %d alone differs from the batch" % bi
        assert all(torch.equal(a[0], o[bi]) for a, o in zip(one[1:], out[1:])), "statistics of utterance %d alone differ from the batch" % bi
    for bi in range(R.ZERO, Bn, 8):            # the zero utterance: mean 0, rstd fl(1 / sqrt(eps)) exactly, y = GELU(beta) to the store rounding
        assert bool((host[1][bi] == 0).all()) and bool((host[2][bi] == torch.tensor(1.0 / N.f32(R.EPS) ** 0.5, dtype=torch.float32)).all())
        zb = c["beta"].double()[None].expand(int(live[bi].sum()), -1)
        within(host[0][bi][live[bi]], N.gelu64(zb), N._gelu_out_bound(zb, torch.zeros_like(zb), dt), tag + "y zero utterance " + cs[0])
    if not backward:
        return
    rb = R.bwd64(c["dy"], c["wav"], c["w"], c["gamma"], c["beta"], host[1], host[2], host[3], kk, st, c["limit"])
    bb = R.bwd_bounds(rb, dt, c["route"])
    g = k.conv0_bwd(dy, wav, w, gamma, beta, out[1], out[2], out[3], kk, st, frame_limit=lim)
    for n, o in zip(BWD_OUT, g):
        within(o, rb[n], bb[n], tag + "%-7s" % n + cs[0])
    g2 = k.conv0_bwd(dy, wav, w, gamma, beta, out[1], out[2], out[3], kk, st, frame_limit=lim)
    assert all(torch.equal(a, o) for a, o in zip(g2, g)), "the backward is not bit-reproducible"


@pytest.mark.parametrize("cs", R.CASES, ids=[c[0] for c in R.CASES])
def test_conv0_gn(K, cs):
    _run(K[0], cs)


def test_conv0_gn_gram_block_cap(K):
    """L = 64 * 2048 + 300: the Gram pass runs its cap of 64 blocks, every lane eight full grid-stride iterations and 300 lanes a ninth."""
    L = R.CAP_CASE[5]
    assert R.ceil_div(L, R.TB) > R.GRAM_CAP and R.ceil_div(L, 256 * R.GRAM_CAP) == 9 and L % (256 * R.GRAM_CAP) == 300
    assert K[1].load().cst_conv0_fwd_workspace(1, R.S_of(10, 5, L), 10, 5) == R.GRAM_CAP * 110 * 4, "the block cap moved: this shape no longer reaches it"
    _run(K[0], R.CAP_CASE, alone=())


@pytest.mark.parametrize("cs", R.LDS_CASES, ids=[c[0] for c in R.LDS_CASES])
def test_lds_envelope_backward_largest_accepted(K, cs):
    """The generic backward (and forward) at the largest dynamic LDS the entry point accepts: 163836 bytes, and 155704 at C = 2048."""
    assert R.bwd_lds(cs[1], cs[2], cs[3], cs[4]) <= R.LDS_MAX
    _run(K[0], cs, alone=())


@pytest.mark.parametrize("cs", R.LDS_FWD_CASES, ids=[c[0] for c in R.LDS_FWD_CASES])
def test_lds_envelope_forward_largest_accepted(K, cs):
    """The generic forward at the largest dynamic LDS it accepts (163840 bytes: all of a CU's; 163648 at C = 2048).  The backward of these
    shapes asks for more than the part has and is refused: the two entry points have envelopes of their own."""
    assert R.fwd_lds(cs[1], cs[2], cs[3]) <= R.LDS_MAX < R.bwd_lds(cs[1], cs[2], cs[3], cs[4])
    _run(K[0], cs, backward=False, alone=())
    k, lib = K
    c = R.case(*cs)
    wav, w, gamma, beta, dy = cu(c["wav"], c["w"], c["gamma"], c["beta"], c["dy"])
    y, mean, rstd, gram = k.conv0_fwd(wav, w, gamma, beta, c["k"], c["stride"], R.EPS)
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        k.conv0_bwd(dy, wav, w, gamma, beta, mean, rstd, gram, c["k"], c["stride"])


@pytest.mark.parametrize("dt", [R.F, R.B], ids=["f32", "bf16"])
def test_lds_envelope_refusals_touch_nothing(K, dt):
    """The smallest refused requests (163844 bytes, forward and backward) are refused before the first launch: every output and the
    workspace keep what they held."""
    k, lib = K
    P, cl = lib.ptr, lib.load()
    L, Bn = 37, 1
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    for (kk, st, C), fwd in ((R.LDS_FWD_REFUSED, True), (R.LDS_BWD_REFUSED, False)):
        S = R.S_of(kk, st, L)
        assert (R.fwd_lds(kk, st, C) if fwd else R.bwd_lds(kk, st, C, dt)) == R.LDS_MAX + 4
        wav, w, gamma, beta = cu(*R.make_inputs(Bn, S, C, kk, st, dt))
        y = f(Bn, L, C).to(dt)
        mean, rstd, gram = f(Bn, C), f(Bn, C), f(Bn, kk * kk + kk)
        dw, dg, db = f(C, kk), f(C), f(C)
        ws = f(max(cl.cst_conv0_fwd_workspace(Bn, S, kk, st), cl.cst_conv0_bwd_workspace(Bn, S, C, kk, st)) // 4)
        if fwd:
            rc = cl.cst_conv0_gn_gelu_fwd(P(wav), P(w), P(gamma), P(beta), P(y), P(mean), P(rstd), P(gram), P(ws), None, Bn, S, C, kk, st, R.EPS,
                                          lib.dtype_code(dt), lib.stream_ptr())
            with pytest.raises(RuntimeError, match="bytes of LDS"):
                k.conv0_fwd(wav, w, gamma, beta, kk, st, R.EPS)
        else:
            rc = cl.cst_conv0_gn_gelu_bwd(P(y), P(wav), P(w), P(gamma), P(beta), P(mean), P(rstd), P(gram), P(dw), P(dg), P(db), P(ws), None, Bn, S,
                                          C, kk, st, lib.dtype_code(dt), lib.stream_ptr())
        assert rc == -1 and b"bytes of LDS" in cl.cst_last_error(), (kk, st, C)
        torch.cuda.synchronize()
        for t in (y, mean, rstd, gram, dw, dg, db, ws):
            assert bool((t.float() == 7.0).all())

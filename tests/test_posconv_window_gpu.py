"""Sliding-window kernels of the positional convolution (csrc/posconv.hip) against the implicit-GEMM route of
functional._PosConvGemmFn (CST_POSCONV_GEMM=1) and against torch's grouped conv1d in fp64.

The window kernels keep the GEMM route's order of summation (one MFMA accumulator chain per output element over the same K
order, the same epilogue code), so every result is compared with torch.equal: y, z, dx, and also dw / db (the weight-gradient chain —
ascending 64-frame blocks of the zero-padded frame axis, live blocks only — and the bias gradient's partial-sum chain are
reproduced as well, so the fp64 comparison the issue allows as a fallback for dw / db is not needed).

Shapes: C = 96 (two groups of 48), B = 3, k = 128 (even: torch pads k / 2 on both sides and SamePad drops the last frame) and one
odd k = 127; T in {1, 64, 129, 300}: every tap in the padding, a partial 64-frame K block, a K block boundary + 1, and more than one
256-frame workgroup block (and the narrow-tile GEMM configurations on the other route)."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg

pytestmark = pytest.mark.gpu

B_, C, G = 3, 96, 2
DT = torch.bfloat16


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DT).to("cuda")


@pytest.fixture(scope="module")
def mods():
    load_pkg()
    return importlib.import_module("chimera-st_amd.functional"), importlib.import_module("chimera-st_amd.kernels")


def inputs(T, k, lens=None, keep=None):
    x = rnd(B_, T, C, seed=160 + T, scale=0.5)
    w = rnd(C, C // G, k, seed=161 + T, scale=0.02)
    b = rnd(C, seed=162 + T, scale=0.1)
    dy = rnd(B_, T, C, seed=163 + T)
    t = torch.arange(T, device="cuda")[None, :, None]
    if lens is not None:
        x = x * (t < lens[:, None, None]).to(DT)
    if keep is not None:
        dy = dy * (t < keep[:, None, None]).to(DT)
    return x, w, b, dy


def run(mods, monkeypatch, gemm_route, x0, w0, b0, dy, lens=None, keep=None, host=False):
    """-> dict of y, z, dx, dw, db and the number of window-kernel launches of the call."""
    CF, Kn = mods
    if gemm_route:
        monkeypatch.setenv("CST_POSCONV_GEMM", "1")
    else:
        monkeypatch.delenv("CST_POSCONV_GEMM", raising=False)
    calls = []
    for name in ("posconv_fwd", "posconv_dx", "posconv_dw"):
        fn = getattr(Kn, name)
        monkeypatch.setattr(Kn, name, (lambda f, n: lambda *a, **kw: (calls.append(n), f(*a, **kw))[1])(fn, name))
    x, w, b = (v.clone().requires_grad_(True) for v in (x0, w0, b0))
    y = CF.pos_conv_gelu_residual(x, w, b, x0.shape[2] // w0.shape[1], lens, keep, keep.tolist() if (host and keep is not None) else None)
    z = y.grad_fn.saved_tensors[2].clone()
    y.backward(dy)
    monkeypatch.undo()
    return {"y": y.detach(), "z": z, "dx": x.grad, "dw": w.grad, "db": b.grad, "calls": calls}


def same_bits(a, b, what):
    for name in ("y", "z", "dx", "dw", "db"):
        assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype, "%s %s" % (what, name)
        assert torch.isfinite(b[name].float()).all(), "%s %s: not finite" % (what, name)
        assert torch.equal(a[name], b[name]), "%s: %s differs on %d of %d elements (max |diff| %.3e)" % (
            what, name, int((a[name] != b[name]).sum()), a[name].numel(), float((a[name].float() - b[name].float()).abs().max()))


@pytest.mark.parametrize("T,k", [(1, 128), (64, 128), (129, 128), (300, 128), (129, 127)])
def test_window_route_has_the_bits_of_the_gemm_route_and_the_values_of_conv1d(mods, monkeypatch, T, k):
    x, w, b, dy = inputs(T, k)
    new = run(mods, monkeypatch, False, x, w, b, dy)
    old = run(mods, monkeypatch, True, x, w, b, dy)
    assert new["calls"] == ["posconv_fwd", "posconv_dx", "posconv_dw"] and old["calls"] == []
    same_bits(old, new, "T=%d k=%d" % (T, k))
    # absolute: torch's grouped conv1d in fp64 (even k: pad k / 2 both sides, drop the last frame), at the tolerance of
    # test_kernels_gpu.test_pos_conv_function_wav2vec_small_shape (bf16: rtol 2e-2, atol 2e-2 * scale)
    xr, wr, br = (v.double().requires_grad_(True) for v in (x, w, b))
    conv = F.conv1d(xr.transpose(1, 2), wr, br, padding=k // 2, groups=G)
    if k % 2 == 0:
        conv = conv[:, :, :-1]
    ref = xr + F.gelu(conv).transpose(1, 2)
    ref.backward(dy.double())

    def check(got, want, what, scale=None):
        got, want = got.double(), want.double()
        s = float(want.abs().max()) if scale is None else scale
        bad = (got - want).abs() > 2e-2 * max(s, 1e-6) + 2e-2 * want.abs()
        assert not bad.any(), "%s: max err %.3e (ref max %.3e), %d/%d out of tolerance" % (
            what, float((got - want).abs().max()), s, int(bad.sum()), bad.numel())

    check(new["y"], ref, "y")
    check(new["z"], conv.transpose(1, 2), "z")
    check(new["dx"], xr.grad, "dx")
    check(new["dw"], wr.grad, "dw", scale=float(wr.grad.abs().max()))
    check(new["db"], br.grad, "db", scale=float(br.grad.abs().max()))


@pytest.mark.parametrize("T,host", [(1, False), (64, False), (129, False), (300, False), (300, True)])
def test_window_route_frame_limits_keep_every_bit(mods, monkeypatch, T, host):
    """lens / grad_rows = (T, T / 2, 0): what test_kernels_gpu.test_pos_conv_frame_limits_keep_every_bit demands of the GEMM route — y, dx,
    dw and db of the limited call equal the unlimited call's — and the limited calls of both routes agree, an utterance with nothing
    live included ("host": the K-block stamps come from the plan's host integers)."""
    k = 128
    lens = torch.tensor([T, T // 2, 0], dtype=torch.int32, device="cuda")
    x, w, b, dy = inputs(T, k, lens, lens)
    free = run(mods, monkeypatch, False, x, w, b, dy)
    lim = run(mods, monkeypatch, False, x, w, b, dy, lens, lens, host)
    old = run(mods, monkeypatch, True, x, w, b, dy, lens, lens, host)
    assert lim["calls"] == ["posconv_fwd", "posconv_dx", "posconv_dw"] and old["calls"] == []
    same_bits(free, lim, "limited vs unlimited")
    same_bits(old, lim, "limited, both routes")


def test_other_group_widths_take_the_gemm_route(mods, monkeypatch):
    """C / groups = 32: the window kernels are not built for it; the call runs the implicit GEMM (and is right)."""
    CF, Kn = mods
    T, k, C2, G2 = 37, 16, 64, 2
    x = rnd(B_, T, C2, seed=170, scale=0.5)
    w = rnd(C2, C2 // G2, k, seed=171, scale=0.1)
    b = rnd(C2, seed=172, scale=0.1)
    dy = rnd(B_, T, C2, seed=173)
    got = run(mods, monkeypatch, False, x, w, b, dy)
    assert got["calls"] == []
    ref = F.conv1d(x.double().transpose(1, 2), w.double(), b.double(), padding=k // 2, groups=G2)[:, :, :-1]
    ref = x.double() + F.gelu(ref).transpose(1, 2)
    err = (got["y"].double() - ref).abs()
    assert not (err > 2e-2 * float(ref.abs().max()) + 2e-2 * ref.abs()).any(), float(err.max())

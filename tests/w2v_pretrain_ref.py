"""fp64 restatement, derived forward-error bounds and an fp32 op-by-op evaluation of the kernels in csrc/w2v_pretrain.hip:
cst_infonce_fwd, cst_infonce_bwd_x, cst_infonce_bwd_y and, in the second half of this file under its own header, cst_gumbel_vq_fwd /
cst_gumbel_vq_bwd (the sampler cst_w2v_negatives is integers only: rng.negatives_numpy restates it bit
for bit).  Plain torch / numpy on the CPU; shared by test_w2v_pretrain_ref_cpu.py (the restatement equals torch's cosine_similarity +
cross_entropy with autograd in fp64; the bounds hold for a faithful fp32 evaluation and reject every listed defect) and
test_w2v_pretrain_gpu.py (the kernels under the same bounds).

How the bounds are built (the conventions of ctc_ref.py / loss_optim_ref.py).  Every fp32 operation returns (x op y)(1 + d), |d| <= u =
2^-24; a division and a square root are counted 2u (correctly rounded in the build's default; 2u leaves room for a libm-accuracy
lowering), expf and logf 2u.  A bf16 store rounds to nearest even, counted 2^-8.  The operands ROUNDED to the storage type are the exact
inputs, and so is the fp32 value of 1 / temp.  Every count of a multiply-add chain allows one more u per term, so that the bound covers a
separately rounded product as well as an fmaf.

    dot = sum_e x_e t_e: a lane's chain of 8 ceil(D / 512) terms, then 6 butterfly adds:  Cd u A,  A = sum_e |x_e t_e|,
          Cd = 8 ceil(D / 512) + 6 + 1
    |x| = sqrt(sum x^2): Cn u relative, Cn = Cd / 2 + 2 (the square root halves the sum's error);  the clamp to eps is exact
    cos = dot / (cx ct):  u (Cd A / (cx ct) + |cos| (2 Cn + 3))                                                  =: dcos   (absolute)
    l = cos / temp:  dcos / temp + u |l|;   a masked negative's -inf is exact (the rows' equality is decided on the stored values)   =: dl
    lse = m + log(sum_j exp(l_j - m)), m = max_j l_j exact on the computed logits; logsumexp is 1-Lipschitz in the sup norm:
          max_j dl_j + u (Cs + 2 + sum_j p_j |l_j - m| + 2 |log se| + |lse|),  Cs = ceil((K' + 1) / 64) + 6 the adds of the strided sum
    nll = lse - l_0:  dlse + dl_0 + u |nll|;   exactly 0 (bound 0) where every negative is masked
    loss = (float) sum in double:  sum_p dnll_p + u |loss|
Backward, position p (g = the upstream gradient, exact):
    p_j = exp(l_j - lse): p_j (expm1(dl_j + dlse + u |l_j - lse|) + 2u) + FLUSH;  gl_j = g (p_j - [j = 0]): |g| dp_j + 2u |gl_j|
    dc_j = gl_j / temp:  dgl_j / temp + u |dc_j|;    w_j = dc_j / ct_j:  ddc_j / ct_j + |w_j| (Cn + 2) u
    acc_e = sum_j w_j t_je (a chain of K' + 1 terms):  sum_j dw_j |t_je| + (K' + 2) u sum_j |w_j t_je|
    S = sum_j dc_j cos_j:  sum_j (ddc_j |cos_j| + |dc_j| dcos_j) + (K' + 2) u sum_j |dc_j cos_j|
    dx_e = acc_e / cx - coef x_e, coef = [|x| >= eps] S / (cx |x|):
          dacc_e / cx + |acc_e / cx| (Cn + 2) u  +  (dS / (cx |x|) + |coef| (2 Cn + 3) u) |x_e| + u |coef x_e|  +  u |dx_e|
    dy_r: the same with the roles exchanged; the chain is the row's list of L_r (position, j) pairs, the weights dc / cx_p.
A bf16 store adds 2^-8 |value|.  SLACK = 1 + 2^-10 covers the second-order products; FLUSH the results below the smallest normal.
No constant here was fitted to an output of the kernels or of the evaluation below."""
import functools
import math
from importlib import import_module

import numpy as np
import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -8
FLUSH = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
EPS = 1e-8

DEFECTS = ("no_eps_clamp", "no_mask", "duplicate_once", "no_temp_in_backward")

# name -> dict(B, M, K, Kx, D, temp, plant)
CASES = {
    "tiny": dict(B=1, M=2, K=1, D=16),
    "duplicates": dict(B=3, M=37, K=100, D=256),       # K > M - 1: every position draws some row more than once
    "recipe": dict(B=2, M=300, K=100, D=256),
    "wide": dict(B=2, M=5, K=3, D=768),                # two 8-element groups per lane
    "cross": dict(B=2, M=16, K=4, Kx=3, D=16),
    "planted": dict(B=2, M=6, K=4, D=16, plant=True),
}
TEMP = 0.1


def _rng():
    import conftest
    conftest.load_pkg()
    return import_module("chimera-st_amd.rng")


def make_case(name, dtype=torch.float32):
    """(x [N, D], y [N, D] in dtype, idx int32 [N, K'], inv_temp: the fp32 value of 1 / temp, (B, M, K, Kx), key) of a named case; the
    indices are the sampler's (rng.negatives_numpy).  `planted`: codebook-like targets —
      rows 1 and 3 of utterance 0 repeat row 0's target (negatives equal to their positive wherever they are drawn), position 2's
      negatives are all pointed at rows that repeat ITS target (rows 4, 5), x row 7 and y row 8 are zero."""
    c = CASES[name]
    B, M, K, Kx, D = c["B"], c["M"], c["K"], c.get("Kx", 0), c["D"]
    seed = 2000 + sorted(CASES).index(name)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    N = B * M
    x = torch.randn(N, D, generator=g).to(dtype)
    y = torch.randn(N, D, generator=g).to(dtype)
    key = (0x5EED0000 + seed) & 0xFFFFFFFF
    idx = torch.from_numpy(_rng().negatives_numpy(key, B, M, K, Kx).reshape(N, K + Kx).copy())
    if c.get("plant"):
        y[1] = y[0]
        y[3] = y[0]
        y[4] = y[2]
        y[5] = y[2]
        idx[2] = torch.tensor([4, 5, 5, 4], dtype=torch.int32)
        idx[0, 0] = 1
        idx[0, 1] = 3
        x[7] = 0.0
        y[8] = 0.0
        idx[9, 0] = 8   # a zero target row among the negatives of a live position
    inv_temp = float(np.float32(1.0) / np.float32(TEMP))
    return x, y, idx, inv_temp, (B, M, K, Kx), key


def dot_chain(D):
    return 8 * math.ceil(D / 512) + 6 + 1


def _xor_butterfly(v):
    """wave_sum: v [..., 64] fp32 -> [...] after the 6 xor steps (every lane ends with equal bits; lane 0 is returned)."""
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def _dot(a, b, dt):
    """sum_e a_e b_e over the last dimension; in fp32 with the kernel's order: lane l owns the 8-element groups l and l + 64, an fmaf
    chain over its elements, then the butterfly.  (The fmaf is evaluated as the fp32 rounding of the exact product plus the sum.)"""
    if dt != torch.float32:
        return (a * b).sum(-1)
    D = a.shape[-1]
    ng = D // 8
    a2 = torch.nn.functional.pad(a, (0, 1024 - D)).reshape(*a.shape[:-1], 2, 64, 8)
    b2 = torch.nn.functional.pad(b, (0, 1024 - D)).reshape(*b.shape[:-1], 2, 64, 8)
    s = torch.zeros(a2.shape[:-3] + (64,), dtype=torch.float32)
    for i in range(2 if ng > 64 else 1):
        for e in range(8):
            s = (a2[..., i, :, e].double() * b2[..., i, :, e].double() + s.double()).float()
    return _xor_butterfly(s)


def _strided_sum(v, dt):
    """sum over the last dimension; in fp32 as the kernel's lanes do: lane l adds elements l, l + 64, ..., then the butterfly."""
    if dt != torch.float32:
        return v.sum(-1)
    n = v.shape[-1]
    pad = (-n) % 64
    v2 = torch.nn.functional.pad(v, (0, pad)).reshape(*v.shape[:-1], -1, 64)
    s = torch.zeros(v.shape[:-1] + (64,), dtype=torch.float32)
    for c in range(v2.shape[-2]):
        s = s + v2[..., c, :]
    return _xor_butterfly(s)


def infonce_eval(x, y, idx, inv_temp, gscale=1.0, dt=torch.float64, defect=None, with_bounds=False, store=None):
    """The operation sequence of cst_infonce_fwd / _bwd_x / _bwd_y in the arithmetic `dt` (fp64: the reference; fp32: a faithful
    evaluation; `defect`: one of DEFECTS).  x, y [N, D] (their values are the exact inputs), idx int32 [N, K'].
    Returns dict(logits [N, K' + 1], nll [N], loss, correct, count, dx, dy) and, under with_bounds (fp64 only), `bounds`: the same keys
    holding per-element absolute bounds for results stored as `store` (torch.float32 / torch.bfloat16)."""
    N, D = x.shape
    KP = idx.shape[1]
    xs, ys = x.to(dt), y.to(dt)
    it = torch.tensor(inv_temp, dtype=dt)
    g = torch.tensor(gscale, dtype=dt)
    rows = torch.cat([torch.arange(N)[:, None], idx.long().clamp(0, N - 1)], 1)
    nx, ny = _dot(xs, xs, dt).sqrt(), _dot(ys, ys, dt).sqrt()
    if defect == "no_eps_clamp":
        cx, cy = nx, ny
    else:
        cx, cy = nx.clamp_min(EPS), ny.clamp_min(EPS)
    cos = torch.empty(N, KP + 1, dtype=dt)
    ahat = torch.empty(N, KP + 1, dtype=dt)
    masked = torch.zeros(N, KP + 1, dtype=torch.bool)
    for j in range(KP + 1):
        t = ys[rows[:, j]]
        cos[:, j] = _dot(xs, t, dt) / (cx * cy[rows[:, j]])
        if with_bounds:
            ahat[:, j] = (xs.abs() * t.abs()).sum(-1) / (cx * cy[rows[:, j]])
        if j > 0:
            masked[:, j] = (y[rows[:, j]] == y).all(-1)
    if defect == "no_mask":
        masked[:] = False
    ninf = torch.tensor(float("-inf"), dtype=dt)
    logits = torch.where(masked, ninf, cos * it)
    live = ~masked
    if defect == "duplicate_once":  # a row drawn twice by one position enters its softmax once
        for j in range(2, KP + 1):
            live[:, j] &= ~(rows[:, 1:j] == rows[:, j:j + 1]).any(-1)
    ll = torch.where(live, logits, ninf)
    m = ll.max(-1).values
    mn = ll.min(-1).values
    e = torch.exp(ll - m[:, None])
    se = _strided_sum(e, dt)
    lse = m + torch.log(se)
    nll = lse - ll[:, 0]
    loss = nll.double().sum().to(dt)
    correct = int(((ll[:, 0] == m) & ~(ll[:, 0] == mn)).sum())
    p = torch.where(live, torch.exp(ll - lse[:, None]), torch.zeros((), dtype=dt))
    onehot = torch.zeros(N, KP + 1, dtype=dt)
    onehot[:, 0] = 1.0
    gl = torch.where(live, g * (p - onehot), torch.zeros((), dtype=dt))
    dc = gl if defect == "no_temp_in_backward" else gl * it
    w = dc / cy[rows]
    acc = torch.zeros(N, D, dtype=dt)
    S = torch.zeros(N, dtype=dt)
    accy = torch.zeros(N, D, dtype=dt)
    Sy = torch.zeros(N, dtype=dt)
    wy = dc / cx[:, None]
    # the inverted index's order: a row's own positive first, then its draws in ascending (position, j)
    for j in range(KP + 1):
        t = ys[rows[:, j]]
        acc = acc + w[:, j:j + 1] * t
        S = S + dc[:, j] * cos[:, j]
    accy.index_add_(0, rows[:, 0], wy[:, 0:1] * xs)
    Sy.index_add_(0, rows[:, 0], dc[:, 0] * cos[:, 0])
    if KP:
        flat = rows[:, 1:].reshape(-1)
        accy.index_add_(0, flat, (wy[:, 1:, None] * xs[:, None, :]).reshape(-1, D))
        Sy.index_add_(0, flat, (dc[:, 1:] * cos[:, 1:]).reshape(-1))
    zero = torch.zeros((), dtype=dt)
    coefx = torch.where(nx >= EPS, S / (cx * nx), zero) if defect != "no_eps_clamp" else S / (cx * nx)
    coefy = torch.where(ny >= EPS, Sy / (cy * ny), zero) if defect != "no_eps_clamp" else Sy / (cy * ny)
    dx = acc / cx[:, None] - coefx[:, None] * xs
    dy = accy / cy[:, None] - coefy[:, None] * ys
    out = dict(logits=logits, nll=nll, loss=loss, correct=correct, count=N, dx=dx, dy=dy, masked=masked)
    if not with_bounds:
        return out
    assert dt == torch.float64 and defect is None
    u = U32
    ub = UBF if store == torch.bfloat16 else 0.0
    Cd = dot_chain(D)
    Cn = Cd / 2 + 2
    Cs = math.ceil((KP + 1) / 64) + 6
    itf = float(it)
    fin = lambda v: torch.where(masked, zero, v)
    d_cos = u * (Cd * ahat + cos.abs() * (2 * Cn + 3))
    d_l = fin(itf * d_cos + u * (cos * it).abs())
    lm = fin((logits - m[:, None]).abs())
    d_lse = d_l.max(-1).values + u * (Cs + 2 + (p * lm).sum(-1) + 2 * torch.log(se).abs() + lse.abs())
    all_masked = masked[:, 1:].all(-1)
    d_nll = torch.where(all_masked, zero, d_lse + d_l[:, 0] + u * nll.abs())
    d_loss = d_nll.sum() + u * loss.abs()
    d_p = fin(p * (torch.expm1(d_l + d_lse[:, None] + u * fin((logits - lse[:, None]).abs())) + 2 * u) + FLUSH)
    d_gl = fin(abs(gscale) * d_p + 2 * u * gl.abs())
    d_dc = itf * d_gl + u * dc.abs()
    d_w = d_dc / cy[rows] + w.abs() * (Cn + 2) * u
    d_wy = d_dc / cx[:, None] + wy.abs() * (Cn + 2) * u
    d_acc = torch.zeros(N, D, dtype=dt)
    m_acc = torch.zeros(N, D, dtype=dt)
    for j in range(KP + 1):
        ta = ys[rows[:, j]].abs()
        d_acc += d_w[:, j:j + 1] * ta
        m_acc += w[:, j:j + 1].abs() * ta
    d_acc += (KP + 2) * u * m_acc
    d_Sterm = d_dc * cos.abs() + dc.abs() * d_cos
    d_S = d_Sterm.sum(-1) + (KP + 2) * u * (dc * cos).abs().sum(-1)
    flat = rows.reshape(-1)
    L_r = torch.bincount(flat, minlength=N).to(dt)
    d_accy = torch.zeros(N, D, dtype=dt).index_add_(0, flat, (d_wy[:, :, None] * xs.abs()[:, None, :]).reshape(-1, D))
    m_accy = torch.zeros(N, D, dtype=dt).index_add_(0, flat, (wy.abs()[:, :, None] * xs.abs()[:, None, :]).reshape(-1, D))
    d_accy += (L_r[:, None] + 1) * u * m_accy
    d_Sy = torch.zeros(N, dtype=dt).index_add_(0, flat, d_Sterm.reshape(-1))
    d_Sy += (L_r + 1) * u * torch.zeros(N, dtype=dt).index_add_(0, flat, (dc * cos).abs().reshape(-1))

    def finish(accv, d_accv, Sv, d_Sv, nv, cv, coef, av, res):
        t1 = accv / cv[:, None]
        d1 = d_accv / cv[:, None] + t1.abs() * (Cn + 2) * u
        d_coef = torch.where(nv >= EPS, d_Sv / (cv * nv.clamp_min(EPS)) + coef.abs() * (2 * Cn + 3) * u, zero)
        d2 = d_coef[:, None] * av.abs() + u * (coef[:, None] * av).abs()
        return (d1 + d2 + (u + ub) * res.abs()) * SLACK + FLUSH

    bounds = dict(
        logits=d_l * SLACK,
        nll=d_nll * SLACK,
        loss=d_loss * SLACK,
        dx=finish(acc, d_acc, S, d_S, nx, cx, coefx, xs, dx),
        dy=finish(accy, d_accy, Sy, d_Sy, ny, cy, coefy, ys, dy),
    )
    out["bounds"] = bounds
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype, gscale=1.0):
    """(case, fp64 reference with bounds) of a named case at a storage type: computed once, shared, left unchanged."""
    case = make_case(name, dtype)
    x, y, idx, inv_temp = case[:4]
    return case, infonce_eval(x, y, idx, inv_temp, gscale=gscale, with_bounds=True, store=dtype)


def judge(ref, got, keys=("logits", "nll", "loss", "dx", "dy")):
    """Worst |got - ref| / bound per quantity and the number of elements outside their bound (a non-finite value where the reference is
    finite counts; where the reference is -inf the value must be -inf)."""
    ratios, bad = {}, 0
    for k in keys:
        if k not in got or got[k] is None:
            continue
        r = ref[k].double().reshape(-1)
        v = torch.as_tensor(got[k]).double().reshape(-1)
        b = torch.as_tensor(ref["bounds"][k]).double().reshape(-1)
        inf = torch.isinf(r)
        bad += int((v[inf] != r[inf]).sum())
        err = (v[~inf] - r[~inf]).abs()
        wrong = ~(err <= b[~inf])  # (NaN compares false)
        bad += int(wrong.sum())
        nz = b[~inf] > 0
        ratios[k] = float((err[nz] / b[~inf][nz]).nan_to_num(nan=float("inf")).max()) if bool(nz.any()) else 0.0
    return ratios, bad


def torch_composition(x, y, idx, temp, gscale=1.0):
    """compute_preds (models/wav2vec/wav2vec2.py:512-525) + the criterion's cross entropy (criterions/wav2vec_criterion.py:64-103) in
    fp64 with autograd, on the gathered [K' + 1, N, D] tensor — what the kernels replace."""
    x = x.double().detach().requires_grad_(True)
    y = y.double().detach().requires_grad_(True)
    N, D = x.shape
    negs = y[idx.long().reshape(-1)].view(N, -1, D).permute(1, 0, 2)  # [K', N, D]
    neg_is_pos = (y.unsqueeze(0) == negs).all(-1)
    targets = torch.cat([y.unsqueeze(0), negs], dim=0)
    logits = torch.cosine_similarity(x.unsqueeze(0), targets, dim=-1)
    logits = logits / temp
    if bool(neg_is_pos.any()):
        logits = logits.clone()
        logits[1:][neg_is_pos] = float("-inf")
    lg = logits.transpose(0, 1)  # [N, K' + 1]
    loss = torch.nn.functional.cross_entropy(lg, torch.zeros(N, dtype=torch.long), reduction="sum")
    (loss * gscale).backward()
    mx = lg.argmax(-1) == 0
    mi = lg.argmin(-1) == 0
    return dict(logits=lg.detach(), loss=loss.detach(), dx=x.grad, dy=y.grad, correct=int(mx.sum()) - int((mx & mi).sum()), count=N)


# ----------------------------------------------------------------------------------------------------------------------------------
# Gumbel vector quantizer: cst_gumbel_vq_fwd / cst_gumbel_vq_bwd (and the two GEMMs of functional.gumbel_vector_quantize's backward).
#
# Bounds, row n, group g (u = 2^-24; NI = the classes a lane holds: 1 up to 64 codes, 5 up to 320, else 16; a wave sum is a chain of
# Cw = NI + 6 adds; expf / logf / a division 2u):
#   noise g = -log(-log u_e) from the exact uniform: the inner logarithm's 2u relative error is 2u absolute after the outer one, which
#       adds 2u |g|:  dg = 2u (1 + |g|)  (0 for injected noise);   sg = l + g: dg + u |sg|;   z = sg / tau: dsg / tau + u |z|
#   a hard choice is DECIDED when the fp64 top-2 margin of sg exceeds the two candidates' dsg; the cases' seeds leave none undecided
#   softmax with perturbed inputs: d log s_v = dz_v - sum_w s_w dz_w, and the evaluation itself (argument rounding |z - m| u, expf, the
#       sum: Cw + 2 + sum_w s_w |z_w - m|, the division):  rho~_v = dz_v + sum_w s~_w dz_w + u (|z_v - m| + Cw + 6 + sum_w s~_w |z_w - m|)
#       relative; rho_v for softmax(l) likewise with dz = 0
#   d1 = sum s~ gy: sum rho~ s~ |gy| + (Cw + 1) u sum s~ |gy|;   t1 = (1 / tau) s~ (gy - d1):
#       (1 / tau) [rho~ s~ |gy - d1| + s~ (dd1 + u |gy - d1|)] + 2u |t1|     (+ the caller's GEMM error of gy where gy is its output)
#   h = -c0 (L + R), c0 = dppl exp(H_g), L = log(a + 1e-7), R = a / (a + 1e-7):  |c0| (2u |L| + u + 3u R + u |L + R|) + 2u |h|
#       (a, exp(H_g) and dppl are the backward's INPUTS: the forward's outputs have their own bounds below)
#   t2 = (1 / N) s (h - d2): (1 / N) [rho s |h - d2| + s (dh + dd2 + u |h - d2|)] + 3u |t2|;   dl = t1 + t2: + u |dl| (+ 2^-8 |dl| in bf16)
# Forward statistics: a_v = (1 / N) sum_n s_nv through 8 rows per wave, 4 waves, then the workgroups in order: the chain is
#   Cr = 8 + 3 + ceil(N / 32) adds:  da = mean_n rho s + (Cr + 2) u a;   t = a log(a + eps): da |L| + a (d(a + eps) / (a + eps) + 2u |L|)
#   + u |t|;   H = -sum_v t: a chain of Ch = ceil(V / 256) + 8 adds;   exp(H): exp(H) (expm1(dH) + 2u);   the sum over groups: G u more.
#   The hard frequencies are exact counts over N: da = 2u a.
# d vars = onehot^T dq: products by 1 are exact, the chain is the rows that chose the code (in any split): (rows + 1) u sum |dq| + the store.
# ----------------------------------------------------------------------------------------------------------------------------------
VQ_DEFECTS = ("no_tau_in_backward", "hard_gradient", "diversity_sign", "no_tiny")
VQ_CASES = {  # name -> (N, G, V, d)
    "tiny": (1, 2, 8, 8),
    "two_groups": (67, 2, 320, 128),
    "one_group": (1000, 1, 320, 256),
    "unused": (130, 2, 8, 8),  # half the codes never chosen
}
VQ_TAU = 1.7
VQ_TINY = float(np.float32(1e-7))


def vq_lanes(V):
    return 1 if V <= 64 else (5 if V <= 320 else 16)


def make_vq_case(name, dtype=torch.float32):
    """dict(l [N, G V], vars [G V, d], dq [N, G d] in dtype, u fp32 [N, G, V] (the kernel's own uniforms at `key`), dppl, inv_tau, G, key)."""
    N, G, V, d = VQ_CASES[name]
    seed = 3000 + sorted(VQ_CASES).index(name)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    l = torch.randn(N, G, V, generator=g) * 2.0
    if name == "unused":
        l[:, :, V // 2:] -= 40.0
    vars_ = torch.rand(G * V, d, generator=g)
    dq = torch.randn(N, G * d, generator=g)
    key = (0x6B0B0000 + seed) & 0xFFFFFFFF
    u = torch.from_numpy(_rng().gumbel_uniform_numpy(key, N * G * V).reshape(N, G, V).copy())
    return dict(l=l.reshape(N, G * V).to(dtype), vars=vars_.to(dtype), dq=dq.to(dtype), u=u, dppl=float(np.float32(-0.37)),
                inv_tau=float(np.float32(1.0 / VQ_TAU)), G=G, key=key)


def gumbel_of(u, dt=torch.float64):
    u = u.to(dt)
    return -torch.log(-torch.log(u))


def vq_eval(c, noise=None, training=True, dt=torch.float64, defect=None, a_in=None, exph_in=None, gy=None, d_gy=None, with_bounds=False,
            store=None):
    """The operation sequence of cst_gumbel_vq_fwd / _bwd in the arithmetic `dt`.  c: a make_vq_case dict.  noise: fp32 [N, G, V] injected
    noise (exact input), else the noise is -log(-log(c["u"])) evaluated in `dt`.  a_in / exph_in: the backward's inputs when they are not
    this evaluation's own (fp32 outputs of a forward kernel); gy [N, G V]: the backward's input when it is not dq vars^T in `dt`."""
    G = c["G"]
    N, GV = c["l"].shape
    V, d = GV // G, c["vars"].shape[1]
    l = c["l"].to(dt).view(N, G, V)
    vr = c["vars"].to(dt).view(G, V, d)
    dq = c["dq"].to(dt).view(N, G, d)
    it = torch.tensor(c["inv_tau"], dtype=dt)
    tiny = torch.tensor(0.0 if defect == "no_tiny" else VQ_TINY, dtype=dt)
    gn = noise.to(dt).view(N, G, V) if noise is not None else gumbel_of(c["u"], dt)
    sg = l + gn if training else l
    k = sg.argmax(-1)
    kh = l.argmax(-1)
    onehot = torch.zeros(N, G, V, dtype=dt).scatter_(-1, k.unsqueeze(-1), 1.0)
    hard = torch.zeros(N, G, V, dtype=dt).scatter_(-1, kh.unsqueeze(-1), 1.0)
    q = torch.stack([vr[g][k[:, g]] for g in range(G)], 1).reshape(N, G * d)
    m2 = l.max(-1, keepdim=True).values
    e2 = torch.exp(l - m2)
    s = e2 / e2.sum(-1, keepdim=True)
    a = s.sum(0) / N
    hp = hard.sum(0) / N
    La = torch.log(a + tiny)
    H = -(a * La).sum(-1)
    Hc = -(hp * torch.log(hp + tiny)).sum(-1)
    exph = torch.exp(H)
    out = dict(idx=k, q=q, onehot=onehot.view(N, GV), avg_probs=a, exph=exph, prob_perplexity=exph.sum(), code_perplexity=torch.exp(Hc).sum())
    if not training:
        return out
    a_b = a if a_in is None else a_in.to(dt)
    e_b = exph if exph_in is None else exph_in.to(dt)
    gyv = torch.einsum("ngd,gvd->ngv", dq, vr) if gy is None else gy.to(dt).view(N, G, V)
    z = sg * it
    m1 = z.max(-1, keepdim=True).values
    e1 = torch.exp(z - m1)
    st = e1 / e1.sum(-1, keepdim=True)
    sx = onehot if defect == "hard_gradient" else st
    d1 = (sx * gyv).sum(-1, keepdim=True)
    t1 = sx * (gyv - d1) * (1.0 if defect == "no_tau_in_backward" else it)
    c0 = (c["dppl"] * e_b).view(1, G, 1)
    Lb, Rb = torch.log(a_b + tiny), a_b / (a_b + tiny)
    h = (-c0 * (Lb + Rb).unsqueeze(0)).expand(N, G, V)
    d2 = (s * h).sum(-1, keepdim=True)
    t2 = s * (h - d2) / N
    dl = t1 - t2 if defect == "diversity_sign" else t1 + t2
    dvars = torch.einsum("ngv,ngd->gvd", onehot, dq).reshape(G * V, d)
    out.update(dl=dl.reshape(N, GV), dvars=dvars, gy=gyv.reshape(N, GV))
    if not with_bounds:
        return out
    assert dt == torch.float64 and defect is None
    u_, ub = U32, (UBF if store == torch.bfloat16 else 0.0)
    Cw = vq_lanes(V) + 6
    itf = float(it)
    d_g = torch.zeros_like(gn) if noise is not None else 2 * u_ * (1 + gn.abs())
    d_sg = d_g + u_ * sg.abs()
    top2 = sg.topk(2, dim=-1) if V > 1 else None
    undecided = int(((top2.values[..., 0] - top2.values[..., 1]) <= d_sg.gather(-1, top2.indices).sum(-1)).sum()) if V > 1 else 0
    d_z = itf * d_sg + u_ * z.abs()
    zm, lm = (z - m1).abs(), (l - m2).abs()
    rho_t = d_z + (st * d_z).sum(-1, keepdim=True) + u_ * (zm + Cw + 6 + (st * zm).sum(-1, keepdim=True))
    rho = u_ * (lm + Cw + 6 + (s * lm).sum(-1, keepdim=True))
    dgy = torch.zeros_like(gyv) if d_gy is None else d_gy.view(N, G, V)
    d_d1 = (rho_t * st * gyv.abs()).sum(-1, keepdim=True) + (Cw + 1) * u_ * (st * gyv.abs()).sum(-1, keepdim=True) + (st * dgy).sum(-1, keepdim=True)
    r1 = (gyv - d1).abs()
    d_t1 = itf * (rho_t * st * r1 + st * (d_d1 + dgy + u_ * r1)) + 2 * u_ * t1.abs()
    d_h = (c0.abs() * (2 * u_ * Lb.abs() + u_ + 3 * u_ * Rb + u_ * (Lb + Rb).abs()).unsqueeze(0) + 2 * u_ * h.abs()).expand(N, G, V)
    d_d2 = (rho * s * h.abs() + s * d_h).sum(-1, keepdim=True) + (Cw + 1) * u_ * (s * h.abs()).sum(-1, keepdim=True)
    r2 = (h - d2).abs()
    d_t2 = (rho * s * r2 + s * (d_h + d_d2 + u_ * r2)) / N + 3 * u_ * t2.abs()
    d_dl = ((d_t1 + d_t2 + (u_ + ub) * dl.abs()) * SLACK + FLUSH).reshape(N, GV)
    Cr = 8 + 3 + math.ceil(N / 32)
    Ch = math.ceil(V / 256) + 8

    def ppl_bound(av, d_av):
        Lv = torch.log(av + tiny)
        d_L = (d_av + u_ * (av + tiny)) / (av + tiny) + 2 * u_ * Lv.abs()
        tv = av * Lv
        d_H = (d_av * Lv.abs() + av * d_L + u_ * tv.abs()).sum(-1) + Ch * u_ * tv.abs().sum(-1)
        ev = torch.exp(-tv.sum(-1))
        d_e = ev * (torch.expm1(d_H) + 2 * u_)
        return d_e, d_e.sum() + G * u_ * ev.sum()

    d_a = (rho * s).sum(0) / N + (Cr + 2) * u_ * a
    d_exph, d_ppl = ppl_bound(a, d_a)
    _, d_cpl = ppl_bound(hp, 2 * u_ * hp)
    rows = onehot.sum(0).view(G * V, 1)
    d_dvars = ((rows + 1) * u_ * torch.einsum("ngv,ngd->gvd", onehot, dq.abs()).reshape(G * V, d) + (u_ + ub) * dvars.abs()) * SLACK + FLUSH
    d_gy_own = ((d + 1) * u_ * torch.einsum("ngd,gvd->ngv", dq.abs(), vr.abs()) + (u_ + ub) * gyv.abs()).reshape(N, GV) * SLACK + FLUSH
    out["undecided"] = undecided
    out["bounds"] = dict(dl=d_dl, avg_probs=d_a * SLACK, exph=d_exph * SLACK, prob_perplexity=d_ppl * SLACK, code_perplexity=d_cpl * SLACK,
                         dvars=d_dvars, gy=d_gy_own)
    return out


@functools.lru_cache(maxsize=None)
def vq_reference(name, dtype, injected=False):
    """(case, injected noise or None, fp64 reference with bounds) of a quantizer case: computed once, shared, left unchanged.  injected:
    the noise is a given fp32 tensor (the harness' recorded F.gumbel_softmax noise) instead of the kernel's own."""
    c = make_vq_case(name, dtype)
    noise = None
    if injected:
        g = torch.Generator(device="cpu")
        g.manual_seed(77)
        noise = -torch.log(torch.empty(c["u"].shape).exponential_(generator=g))  # torch's own formula for gumbel noise
    return c, noise, vq_eval(c, noise=noise, with_bounds=True, store=dtype)


def vq_torch_composition(c, noise):
    """GumbelVectorQuantizer.forward after weight_proj (modules/gumbel_vector_quantizer.py:148-199) with F.gumbel_softmax(hard=True)
    spelt out on the given noise, in fp64 with autograd; the loss is sum(q * dq) + dppl * prob_perplexity."""
    G = c["G"]
    N, GV = c["l"].shape
    V = GV // G
    x = c["l"].double().reshape(N * G, V).detach().requires_grad_(True)
    vars_ = c["vars"].double().detach().requires_grad_(True)
    _, k = x.max(-1)
    hard_x = x.new_zeros(*x.shape).scatter_(-1, k.view(-1, 1), 1.0).view(N, G, -1)
    hard_probs = hard_x.mean(0)
    code_ppl = torch.exp(-torch.sum(hard_probs * torch.log(hard_probs + 1e-7), dim=-1)).sum()
    avg_probs = torch.softmax(x.view(N, G, -1), dim=-1).mean(0)
    prob_ppl = torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-7), dim=-1)).sum()
    y_soft = ((x + noise.double().reshape(N * G, V)) / (1.0 / c["inv_tau"])).softmax(-1)
    index = y_soft.max(-1, keepdim=True)[1]
    y_hard = torch.zeros_like(x).scatter_(-1, index, 1.0)
    ret = y_hard - y_soft.detach() + y_soft
    q = (ret.view(N, GV).unsqueeze(-1) * vars_.unsqueeze(0)).view(N, G, V, -1).sum(-2).view(N, -1)
    ((q * c["dq"].double()).sum() + c["dppl"] * prob_ppl).backward()
    return dict(q=q.detach(), idx=index.view(N, G), prob_perplexity=prob_ppl.detach(), code_perplexity=code_ppl.detach(),
                dl=x.grad.reshape(N, GV), dvars=vars_.grad)

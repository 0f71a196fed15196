"""Inputs and torch evaluations of the N-member log-probability combination, shared by the ensemble kernel test and by the
measurement of its bound (both evaluate the SAME stored inputs)."""
import math

import torch


def member_logits(N, dtype, rows=160, V=10000, seed=0):
    """[N, rows, V] logits in `dtype`: row 5 has -inf in member 1 only at every 7th token, row 9 in every member at every 11th."""
    g = torch.Generator().manual_seed(1000 * N + seed + (1 if dtype == torch.bfloat16 else 0))
    x = (torch.randn(N, rows, V, generator=g) * 3.0).to(dtype)
    x[1, 5, ::7] = -math.inf
    x[:, 9, ::11] = -math.inf
    return x


def combine(x, T, dt):
    """lp[v] = log(sum_n exp(l_n[v] / T - lse_n)) - log N evaluated by torch in `dt` on the stored logits."""
    lp = torch.log_softmax(x.to(dt) / T, dim=-1)
    return torch.logsumexp(lp, dim=0) - math.log(x.size(0))


def fp32_torch_error(x, T):
    """Largest |fp32 torch - fp64 torch| over the finite elements; the -inf sets must coincide."""
    a, b = combine(x, T, torch.float32), combine(x, T, torch.float64)
    fin = torch.isfinite(b)
    assert torch.equal(fin, torch.isfinite(a))
    return float((a.double() - b)[fin].abs().max())

"""The fp64 reference of ``pv_vae_attention`` and the inputs its tests share (``tests/test_vae_flash_cpu.py`` checks the reference and the inputs on the
CPU, ``tests/test_vae_flash_gpu.py`` runs the kernel on the same inputs).  Nothing here is shared with the code under test."""
import math

import torch

#: the kernel bound of the issue: twice 2^-11 - the two fp16 roundings on the path (P and the output), each at its worst case
BOUND = 1e-3
DIMS = (256, 512)
#: one key; less than a fragment; one short of a 64-key tile and exactly one; one past it with two images; a ragged third tile; a ragged fourth tile with
#: three images (12 workgroups: the block remap is not the identity); exact tiles
SHAPES = ((1, 1), (2, 7), (1, 63), (1, 64), (2, 65), (1, 129), (3, 200), (2, 256))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def attention_ref(q, k, v, *, batch, n, scale, round_p=False):
    """``softmax(scale * q k^T) v`` per image in fp64 from fp16-valued rows ``[batch * n][d]``; image ``i`` owns the rows ``i * n ... i * n + n - 1`` and the
    softmax runs over its own ``n`` keys only.  ``round_p``: the kernel's roundings - ``P = exp(s - max)`` rounded to fp16 once, the denominator summed
    from those rounded values, the quotient rounded to fp16 once.  (The kernel's softmax reference may sit up to 8 binary orders below the row maximum:
    that moves P's exponent, not its 11 significant bits.)"""
    q, k, v = (t.detach().double().cpu() for t in (q, k, v))
    d = q.shape[1]
    out = torch.empty(batch * n, d, dtype=torch.float64)
    for i in range(batch):
        r = slice(i * n, (i + 1) * n)
        s = scale * (q[r] @ k[r].T)
        p = torch.exp(s - s.max(dim=1, keepdim=True).values)
        if round_p:
            p = p.to(torch.float16).double()
        o = (p @ v[r]) / p.sum(dim=1, keepdim=True)
        out[r] = o.to(torch.float16).double() if round_p else o
    return out


def randn_case(d, batch, n):
    """fp16 ``randn`` rows: the scaled scores are ~N(0, 1)."""
    g = torch.Generator().manual_seed(1000 * d + 10 * n + batch)
    return tuple(torch.randn(batch * n, d, generator=g).to(torch.float16) for _ in range(3))


def growing_case(d, batch=2, n=200):
    """Key norms grow along the sequence: the scaled score of query i against key j is about ``a_i * 40 * j / n`` with ``a_i`` in [0.75, 1.5] - at least
    13 binary orders more per 64-key tile, so the running maximum moves (and the accumulated output is rescaled) at every tile."""
    g = torch.Generator().manual_seed(7 * d + n)
    u = torch.randn(d, generator=g)
    u = u / u.norm()
    a = 0.75 + 0.75 * torch.rand(batch * n, 1, generator=g)
    j = (torch.arange(batch * n) % n).float()[:, None]
    q = a * u * math.sqrt(d) + 0.1 * torch.randn(batch * n, d, generator=g)
    k = (40.0 * j / n) * u + 0.1 * torch.randn(batch * n, d, generator=g)
    v = torch.randn(batch * n, d, generator=g)
    return q.to(torch.float16), k.to(torch.float16), v.to(torch.float16)


def peaked_case(d, batch=1, n=129):
    """Scaled scores ~N(0, 20^2): up to about +-60, a softmax that is nearly one-hot."""
    g = torch.Generator().manual_seed(11 * d + n)
    q, k, v = (torch.randn(batch * n, d, generator=g) for _ in range(3))
    return (q * math.sqrt(20.0)).to(torch.float16), (k * math.sqrt(20.0)).to(torch.float16), v.to(torch.float16)

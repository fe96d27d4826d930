"""The noise definition of ``pv_cfg_dpm_step_stochastic`` / ``pv_cfg_dpm_step_pag`` (and the draw of ``pv_fusion_draw``) restated in numpy from the
header alone: Philox4x32-10 (Salmon et al. 2011), the Box-Muller transform of one block into four normals, and the (seed, sample_offset, stream,
step, element) counter layout.  Shared by the kernel tests (``tests/test_sampler_cpu.py`` holds the known-answer tests) and the launch references of
``oracle.abi_ref``."""
from __future__ import annotations

import math

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon et al. 2011) over arrays: ``key`` two and ``ctr`` four uint32 values or arrays (broadcast) -> four uint32 arrays."""
    k0, k1 = (np.asarray(k, dtype=np.uint64) & M32 for k in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in ctr))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2           # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def box_muller(words, dtype=np.float64):
    """The four normals of a Philox block (the header's definition), evaluated in ``dtype``: -> array (..., 4) = (z0, z1, z2, z3)."""
    u = [((w >> np.uint32(9)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -23) for w in words]
    r0, r1 = np.sqrt(dtype(-2) * np.log(u[0])), np.sqrt(dtype(-2) * np.log(u[2]))
    a0, a1 = dtype(2 * math.pi) * u[1], dtype(2 * math.pi) * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def noise_ref(shape, seed, sample_offset, stream, step, dtype=np.float64):
    """``z`` of ``pv_cfg_dpm_step_stochastic`` for a (B, C, H, W) launch -> float64 tensor: elements 4q .. 4q+3 of sample ``b`` are the four normals of
    the block at key (seed_lo, seed_hi), counter (q, sample_offset + b, step, stream)."""
    B, chw = shape[0], int(np.prod(shape[1:]))
    assert chw % 4 == 0
    seed %= 1 << 64
    q = np.arange(chw // 4, dtype=np.uint64)
    out = np.empty((B, chw), dtype=np.float64)
    for b in range(B):
        words = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (q, (sample_offset + b) & 0xFFFFFFFF, step, stream))
        out[b] = box_muller(words, dtype).reshape(-1)
    return torch.from_numpy(out.reshape(shape))


def noise_from_words(rng_words, batch, chw, step):
    """``noise_ref`` from the four device words {seed_lo, seed_hi, sample_offset, stream} (any integer type: taken as uint32 bit patterns) -> [batch, chw]."""
    k0, k1, off, stream = (int(w) & 0xFFFFFFFF for w in rng_words)
    return noise_ref((batch, chw), k0 | (k1 << 32), off, stream, int(step))


def fusion_uniform(rng_words, n_layers):
    """The draws of ``pv_fusion_draw``: u[layer] = (first word of the block at key (rng[0], rng[1]), counter (rng[2], layer, 0, 0)) >> 8, times 2^-24 -
    in [0, 1), exact in fp32."""
    k0, k1, call = (int(w) & 0xFFFFFFFF for w in rng_words[:3])
    w0 = philox4x32_10((k0, k1), (call, np.arange(n_layers, dtype=np.uint64), 0, 0))[0]
    return (w0 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24

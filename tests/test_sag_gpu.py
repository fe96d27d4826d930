"""GPU tests of the two launches of self-attention guidance (SAG): ``pv_attn_colmass`` and ``pv_sag_degrade`` against the fp64 references of
``test_sag_cpu``, in every layout a plan would hand them, with their exact properties (bits of a second run and of a graph replay, bits of ``x`` where the
mask is off, inputs unchanged)."""
import math

import pytest
import torch

from test_sag_cpu import sag_degrade_ref, sag_mask_ref, sag_mass_ref

pytestmark = pytest.mark.gpu

ROWS = (0, 3, 5)                 # first-order first row, a second-order middle row, the last row of the 6-step table
TOL_STEP = 1e-5                  # the project's bound for an fp32 pointwise launch on the coefficient rows (test_guidance_gpu, test_pag_gpu)
#: what ``pv_attn_colmass`` may lose against a plain fp32 torch evaluation of the same formula (the hardware exp2 and another summation order): the issue
#: allowed 16 times that evaluation's own error; the kernel measures 0.4 ... 1.24 times it on every shape and layout, so the entries are held to 4 times
#: it and only the row sums - nk entries added up - to the 16
MASS_FACTOR, MASS_SUM_FACTOR = 4.0, 16.0


@pytest.fixture(scope="module")
def rec_cls():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd.ops import Recorder
    return Recorder


def _graph_of(rec):
    """``rec`` captured into a HIP graph; its launches have run eagerly before, so nothing is loaded under capture"""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rec.run()
    return g


# ---------------------------------------------------------------------------------------------------------------- pv_attn_colmass
COLMASS_SHAPES = [(1, 1, 1, 1, 40), (2, 3, 9, 9, 40), (1, 2, 35, 35, 80), (1, 2, 65, 33, 64), (2, 8, 64, 64, 160), (1, 8, 144, 144, 160), (1, 1, 257, 130, 80)]


@pytest.mark.parametrize("shape", COLMASS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attn_colmass_kernel(rec_cls, shape):
    """``pv_attn_colmass`` against ``sag_mass_ref`` (fp64 on the same fp16 q / k) in three layouts - contiguous, column slices of a ``[B n][3 C]`` buffer
    (nq == nk) or of two padded buffers, the second half of a batch-2B buffer through the pointer - and once with q scaled so that the scores reach
    +-60.  Bound: MASS_FACTOR = 4 times the error of a plain fp32 torch evaluation of the same formula against fp64 on the same inputs (hardware exp2,
    another summation order; not P rounded to fp16, which would cost 5e-4 relative).  ``mass.sum(-1) == nq`` within 16 times that error; two runs and a
    graph replay give the same bits; the inputs are unchanged.
    Measured on MI355X (printed with -s), max |got - fp64| / the fp32 evaluation's: 0 / 0 (1 x 1: exactly 1.0), 1.33e-7 / 1.36e-7, 1.36e-7 / 2.93e-7,
    2.29e-7 / 2.09e-7, 1.34e-7 / 1.48e-7, 2.09e-7 / 1.69e-7, 2.68e-7 / 4.36e-7 - the same in every layout; with scores to +-60 2.7e-7 ... 2.1e-6 against
    6.0e-7 ... 5.3e-6.  max |sum - nq| 4.2e-7 ... 1.4e-6, at most 7.8 times the fp32 error."""
    Bq, heads, nq, nk, d = shape
    C = heads * d
    g = torch.Generator().manual_seed(sum(shape))
    q, k = torch.randn(Bq, nq, C, generator=g).half(), torch.randn(Bq, nk, C, generator=g).half()
    scores = (q.double().view(Bq, nq, heads, d).transpose(1, 2) @ k.double().view(Bq, nk, heads, d).transpose(1, 2).transpose(-1, -2)) / math.sqrt(d)
    q_big = (q.float() * (60.0 / scores.abs().max().item())).half()
    rec = rec_cls("cuda")
    runs = []

    def add(label, qv, kv, qh, kh):
        out = rec.attn_colmass(qv, kv, batch=Bq, heads=heads, nq=nq, nk=nk, d=d)
        out.fill_(float("nan"))
        runs.append((label, out, qh, kh))

    for label, qh in (("contiguous", q), ("scores to +-60", q_big)):
        add(label, qh.reshape(Bq * nq, C).cuda(), k.reshape(Bq * nk, C).cuda(), qh, k)
    # column slices: q and k inside wider rows, with junk around them
    wq, wk = torch.randn(Bq * nq, 3 * C + 8, generator=g).half(), torch.randn(Bq * nk, 3 * C + 8, generator=g).half()
    wq[:, :C], wk[:, C:2 * C] = q.reshape(-1, C), k.reshape(-1, C)
    d_wq, d_wk = wq.cuda(), wk.cuda()
    if nq == nk:
        fused = torch.randn(Bq * nq, 3 * C, generator=g).half()
        fused[:, :C], fused[:, C:2 * C] = q.reshape(-1, C), k.reshape(-1, C)
        d_fused = fused.cuda()
        add("slices of [B n][3 C]", d_fused[:, :C], d_fused[:, C:2 * C], q, k)
    add("slices of padded rows", d_wq[:, :C], d_wk[:, C:2 * C], q, k)
    # the second half of a batch-2B buffer
    q2, k2 = torch.cat([torch.randn_like(q.float()).half(), q]), torch.cat([torch.randn_like(k.float()).half(), k])
    d_q2, d_k2 = q2.reshape(-1, C).cuda(), k2.reshape(-1, C).cuda()
    add("second half of batch 2 B", d_q2[Bq * nq:], d_k2[Bq * nk:], q, k)
    rec.run()
    torch.cuda.synchronize()
    first = [out.clone() for _, out, _, _ in runs]
    rec.run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, out) for a, (_, out, _, _) in zip(first, runs)), "a second run gives other bits"
    graph = _graph_of(rec)
    for _, out, _, _ in runs:
        out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, out) for a, (_, out, _, _) in zip(first, runs)), "a graph replay gives other bits"
    for label, out, qh, kh in runs:
        exp = sag_mass_ref(qh, kh, heads)
        f32_err = (sag_mass_ref(qh, kh, heads, dtype=torch.float32).double() - exp).abs().max().item()
        got = out.cpu().double()
        err, sum_err = (got - exp).abs().max().item(), (got.sum(-1) - nq).abs().max().item()
        print(f"attn_colmass {shape} {label}: max |got - fp64| = {err:.3e} (fp32 torch: {f32_err:.3e}, bound {MASS_FACTOR * f32_err:.3e} / {MASS_SUM_FACTOR * f32_err:.3e}), "
              f"max |sum - nq| = {sum_err:.3e}, mass in [{exp.min():.3f}, {exp.max():.3f}]")
        assert torch.isfinite(got).all() and err <= MASS_FACTOR * f32_err
        assert sum_err <= MASS_SUM_FACTOR * f32_err
    assert torch.equal(d_wq.cpu(), wq) and torch.equal(d_wk.cpu(), wk) and torch.equal(d_q2.cpu(), q2.reshape(-1, C)) and torch.equal(d_k2.cpu(), k2.reshape(-1, C))


# ---------------------------------------------------------------------------------------------------------------- pv_sag_degrade
DEGRADE_SHAPES = [(1, 4, 8, 8, 1, 1), (2, 4, 16, 16, 8, 8), (1, 4, 10, 14, 3, 4), (1, 4, 5, 5, 2, 2), (1, 4, 24, 40, 6, 10)]


@pytest.fixture(scope="module")
def table6():
    from photoverse_amd.scheduler import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(6)
    return sch.coefficient_table(0, blend=True)


@pytest.mark.parametrize("shape", DEGRADE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sag_degrade_kernel(rec_cls, table6, shape):
    """``pv_sag_degrade`` on rows 0, 3 and 5 of the 6-step table against ``sag_degrade_ref`` (fp64 on the same fp32 inputs), rtol = atol = TOL_STEP, with the
    masses all below 1, all above 1, exactly 1.0 (not selected: the comparison is strict) and mixed.  Exactly: an all-zero mask gives the bits of ``x``; a
    pixel whose mask is 0 keeps its bits; ``state`` and every input are unchanged.
    Measured on MI355X (printed with -s), worst max |got - fp64| / (1 + |fp64|) per shape: 3.1e-7, 2.8e-7, 2.0e-7, 2.4e-7, 2.7e-7 - a thirtieth of the bound."""
    n, C, h, w, mh, mw = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, eps = torch.randn(n, C, h, w, generator=g), torch.randn(n, C, h, w, generator=g)
    mixed = torch.rand(n, mh * mw, generator=g) * 2
    mixed.view(-1)[0] = 1.5                                                 # at least one selected cell, also on the 1 x 1 map
    if mh * mw > 2:
        mixed.view(-1)[1:3] = torch.tensor([1.0, 0.5])
    masses = {"below": torch.full((n, mh * mw), 0.75), "above": torch.full((n, mh * mw), 1.25), "exactly 1": torch.ones(n, mh * mw), "mixed": mixed}
    d_x, d_eps, d_coef = x.cuda(), eps.cuda(), table6.cuda()
    worst = 0.0
    for row in ROWS:
        d_state = torch.tensor([row, 6, 0, 0], dtype=torch.int32).cuda()
        rec = rec_cls("cuda")
        outs = {}
        for label, mass in masses.items():
            d_mass = mass.cuda()
            outs[label] = (rec.sag_degrade(d_x, d_eps, d_mass, d_coef, d_state, mh=mh, mw=mw), d_mass)
        rec.run()
        torch.cuda.synchronize()
        for label, (out, d_mass) in outs.items():
            got = out.cpu()
            exp = sag_degrade_ref(x, eps, masses[label], table6[row], mh, mw)
            err = ((got.double() - exp).abs() / (1 + exp.abs())).max().item()
            worst = max(worst, err)
            print(f"sag_degrade {shape} row {row} masses {label}: max |d| / (1 + |fp64|) = {err:.3e}")
            torch.testing.assert_close(got.double(), exp, rtol=TOL_STEP, atol=TOL_STEP)
            m = sag_mask_ref(masses[label], mh, mw, h, w).expand(n, C, h, w)
            assert torch.equal(got[m == 0], x[m == 0])                      # a pixel outside the mask keeps its bits
            if label in ("below", "exactly 1"):
                assert torch.equal(got, x)
            else:
                assert not torch.equal(got[m == 1], x[m == 1])
            assert torch.equal(d_mass.cpu(), masses[label])
        assert d_state.cpu().tolist() == [row, 6, 0, 0]
    print(f"sag_degrade {shape}: worst max |d| / (1 + |fp64|) = {worst:.3e}")
    assert torch.equal(d_x.cpu(), x) and torch.equal(d_eps.cpu(), eps) and torch.equal(d_coef.cpu(), table6)

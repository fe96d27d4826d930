"""Every launch of the inference plans, one at a time, against its fp64 reference (``oracle.plan_audit`` / ``oracle.abi_ref``), at the shapes
the product gives it: pointers resolved to held tensors (use-after-free check), outputs poisoned, element-wise and aggregate bounds, the bytes
around every output, column statistics, and a bit-identical second run.  Plus every batch position of the headline plan against the B = 1
plan the oracle pins."""
import time
import zlib

import pytest
import torch

from oracle import fullsize as fs
from oracle.plan_audit import Auditor

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def auditor():
    from photoverse_amd import _lib
    aud = Auditor(_lib.load())
    yield aud
    print("\nplan audit coverage (worst element error / bound, worst rel-L2 / aggregate bound):\n" + aud.table())


def _conditioning(B, S, P, seed):
    g = torch.Generator().manual_seed(seed)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    return cond, uncond, torch.randn(B, 4, S, S, generator=g)


def _recorders(loop):
    out = [loop.tail]
    for e in loop.all_engines:
        out += [r for r in (e.rec, e.rec_head, e.rec_tail, e.rec_cond) if r is not None]
    return out


def _audit_loop(aud, plan, loop, seed):
    """Conditioning, every launch of the first denoising step in a valid serial order (prefix, heads u / c, merged, tails u / c, tail), then the
    second step's tail (the solver's second-order update).  Returns (audited, recorded)."""
    B, S, P = loop.B, loop.S, loop.P
    cond, uncond, noise = _conditioning(B, S, P, seed)
    for (text, ip), (dt, di) in ((cond, (loop.text_c, loop.ip_c)), (uncond, (loop.text_u, loop.ip_u))):
        dt.copy_(text.reshape(dt.shape).to(dt.device))
        di.copy_(ip.reshape(di.shape).to(di.device))
    recs = _recorders(loop)
    n_aud = n_rec = 0

    def run(name, rec):
        nonlocal n_aud, n_rec
        n_rec += len(rec.calls)
        n_aud += aud.audit(f"{plan}", rec, holders=recs)

    for e in loop.all_engines:
        run("cond", e.rec_cond)
    loop.reset(noise)
    step = []
    step += [e.rec for e in loop.engines_p]
    if loop.merge_lowres:
        (eu,), (ec,), (em,) = loop.engines_u, loop.engines_c, loop.engines_m
        step += [eu.rec_head, ec.rec_head, em.rec, eu.rec_tail, ec.rec_tail]
    else:
        step += [e.rec for e in loop.engines_u + loop.engines_c]
    for r in step:
        run("step1", r)
    run("tail1", loop.tail)
    assert loop.state[0].item() == 1
    for r in step:                                    # second step: the UNet plans as the product runs them, then its tail audited
        r.run()
    run("tail2", loop.tail)
    assert loop.state[0].item() == 2 and torch.isfinite(loop.latents).all()
    return n_aud, n_rec


PLANS = {
    "a-headline": dict(batch=16, S=64, P=1, kw=dict(use_graph=True, two_streams=True, batch_splits=1, share_prefix=False)),
    "b-onestream": dict(batch=16, S=64, P=1, kw=dict(use_graph=True, two_streams=False, batch_splits=1, share_prefix=False)),
    "c-cfg4rank": dict(batch=4, S=96, P=6, kw={}),
    "d-bs1": dict(batch=1, S=64, P=1, kw={}),
}


def _want(doc, fn):
    fn.__doc__ = doc
    return fn


conv9 = lambda k: k[1] == "pv_gemm_conv" and "taps=9" in k[4]
#: (plan, launcher, kernel symbol, splitk, flags) rows each plan must contain
REQUIRED = {
    "a-headline": [_want("attn8_kernel<497>", lambda k: k[2] == "attn8_kernel<497>"),
                   _want("a 3x3 conv on big_tile_kernel<true, ...>", lambda k: conv9(k) and k[2].startswith("big_tile_kernel<true")),
                   _want("a 3x3 conv on big_tile_kernel<false, ...>", lambda k: conv9(k) and k[2].startswith("big_tile_kernel<false")),
                   _want("split-K 2 on the 256 x 320 tile (merged plan)", lambda k: conv9(k) and k[2].startswith("big_tile_kernel") and k[3] == 2),
                   _want("fused attn2, C = 320", lambda k: k[2].startswith("xattn_fused_kernel<320")),
                   _want("fused attn2, C = 640", lambda k: k[2].startswith("xattn_fused_kernel<640")),
                   _want("xattn_lnq_kernel", lambda k: k[2] == "xattn_lnq_kernel")],
    "c-cfg4rank": [_want(f"3x3 conv with {n} K-slices on gemm_conv_kernel<5, true", lambda k, n=n: conv9(k) and k[2].startswith("gemm_conv_kernel<5, true")
                         and k[3] == n) for n in (3, 5, 8)] +
                  [_want("attn8_kernel<497>", lambda k: k[2] == "attn8_kernel<497>"),
                   _want("fused attn2, C = 320", lambda k: k[2].startswith("xattn_fused_kernel<320")),
                   _want("fused attn2, C = 640", lambda k: k[2].startswith("xattn_fused_kernel<640")),
                   _want("xattn_lnq_kernel", lambda k: k[2] == "xattn_lnq_kernel")],
}


@pytest.mark.parametrize("plan", list(PLANS))
def test_plan_audit_unet(plan, full_hip_unet, auditor):
    from photoverse_amd.pipeline import DenoiseLoop
    c = PLANS[plan]
    t0 = time.time()
    loop = DenoiseLoop(full_hip_unet, c["batch"], c["S"], c["P"], 50, 7.5, **c["kw"])
    n_aud, n_rec = _audit_loop(auditor, plan, loop, seed=zlib.crc32(plan.encode()) % 10000)
    print(f"\n{plan}: audited {n_aud} of {n_rec} recorded launches in {time.time() - t0:.1f} s (merge_lowres={loop.merge_lowres})")
    assert n_aud == n_rec and n_rec > 0
    # the dispatch decisions the plan is known to reach are in the audit (a dispatch change that drops one shows up here)
    rows = [k for k in auditor.rows if k[0] == plan]
    for want in REQUIRED.get(plan, ()):
        assert any(want(k) for k in rows), f"{plan}: no audited launch matches {want.__doc__}"
    del loop
    torch.cuda.empty_cache()


def test_plan_audit_vae(full_weights, auditor):
    from photoverse_amd.ops import Recorder
    from photoverse_amd.vae import AutoencoderKL
    with fs.no_init():
        vae = AutoencoderKL()
    vae.load_state_dict(full_weights("vae"))
    vae.to("cuda")
    g = torch.Generator().manual_seed(21)
    t0 = time.time()
    dec = vae._plan(1, 64, 64, torch.device("cuda"))
    dec.z.copy_(torch.randn(dec.z.shape, generator=g))
    n_dec = auditor.audit("e-vae-dec", dec.rec)
    enc = vae._plan_encode(1, 512, 512, torch.device("cuda"))
    enc.x.copy_(torch.rand(enc.x.shape, generator=g) * 2 - 1)
    n_enc = auditor.audit("e-vae-enc", enc.rec)
    mom = enc.moments.view(1, enc.h, enc.w, -1)[..., :enc.nm].permute(0, 3, 1, 2).contiguous()
    rec = Recorder(mom.device)
    rec.posterior_sample(mom, torch.randn(1, enc.nm // 2, enc.h, enc.w, generator=g).cuda())
    n_post = auditor.audit("e-vae-enc", rec)
    print(f"\nVAE: audited {n_dec} of {len(dec.rec)} decode, {n_enc} of {len(enc.rec)} encode, {n_post} of {len(rec)} posterior launches "
          f"in {time.time() - t0:.1f} s")
    assert (n_dec, n_enc, n_post) == (len(dec.rec), len(enc.rec), len(rec)) and n_dec and n_enc


def test_headline_plan_every_batch_position_matches_bs1(full_hip_unet):
    """All 16 samples of the bs = 16 headline plan (two streams, merged low-resolution plan, split-K, half-chip tiles) after 10 steps against the
    B = 1 plan - the plan the fp32 oracle pins (test_fullsize_gpu) - run on each sample's own conditioning and noise."""
    from photoverse_amd.pipeline import DenoiseLoop
    B, S = 16, 64
    cond, uncond, noise = _conditioning(B, S, 1, seed=31)
    big = DenoiseLoop(full_hip_unet, B, S, 1, 50, 7.5, use_graph=True, two_streams=True, batch_splits=1, share_prefix=False)
    big.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    big.reset(noise)
    got = big.run(10).clone().cpu()
    assert big.state[0].item() == 10
    del big
    one = DenoiseLoop(full_hip_unet, 1, S, 1, 50, 7.5)
    errs = []
    for i in range(B):
        one.set_conditioning(tuple(t[i:i + 1].cuda() for t in cond), tuple(t[i:i + 1].cuda() for t in uncond))
        one.reset(noise[i:i + 1])
        ref = one.run(10).clone().cpu()
        errs.append(rel_l2(got[i:i + 1], ref))
    print("headline plan vs B = 1 plan after 10 steps, per batch position:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < 1e-3, errs

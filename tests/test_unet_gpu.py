"""GPU parity of the HIP UNet / processors against the CPU oracle (same weights via state_dict, same inputs)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def tiny_pair():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from oracle.unet_ref import TINY_CONFIG, UNet2DConditionModelRef, set_visual_cross_attention_adapter_ref
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    torch.manual_seed(0)
    ref = UNet2DConditionModelRef(**TINY_CONFIG).eval()
    set_visual_cross_attention_adapter_ref(ref, (5,))
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    missing = hip.load_state_dict(ref.state_dict(), strict=True)
    hip.to("cuda")
    return ref, hip


# fp16-storage tolerance for ONE UNet forward vs the fp32 oracle (measured 1.2e-3 .. 2e-3 on random-init weights)
TOL_FWD = 2.5e-3


@pytest.mark.parametrize("B,hw,P,t", [(1, 16, 1, 500), (2, 16, 5, 981), (2, 32, 1, 20)])
def test_tiny_unet_forward_matches_oracle(tiny_pair, B, hw, P, t):
    ref, hip = tiny_pair
    g = torch.Generator().manual_seed(100 + B + P)
    x = torch.randn(B, 4, hw, hw, generator=g)
    text, ip = torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)
    with torch.no_grad():
        exp = ref(x, torch.tensor(t), encoder_hidden_states=(text, ip)).sample
        got = hip(x.cuda(), torch.tensor(t), encoder_hidden_states=(text.cuda(), ip.cuda())).sample
    assert got.shape == exp.shape and got.dtype == torch.float32
    assert rel_l2(got, exp) < TOL_FWD
    # side output of the 4 PhotoVerse processors (models/unet.py:38-47)
    from oracle.unet_ref import get_visual_cross_attention_values_norm_ref
    from photoverse_amd.unet import get_visual_cross_attention_values_norm
    assert rel_l2(get_visual_cross_attention_values_norm(hip), get_visual_cross_attention_values_norm_ref(ref)) < 2e-3


def test_per_sample_timesteps(tiny_pair):
    ref, hip = tiny_pair
    g = torch.Generator().manual_seed(7)
    x, text, ip = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 77, 768, generator=g), torch.randn(2, 5, 768, generator=g)
    t = torch.tensor([10, 900])
    with torch.no_grad():
        exp = ref(x, t, encoder_hidden_states=(text, ip)).sample
        got = hip(x.cuda(), t.cuda(), encoder_hidden_states=(text.cuda(), ip.cuda())).sample
    assert rel_l2(got, exp) < TOL_FWD


def test_processor_protocol_standalone(tiny_pair):
    """attention-processor seam: processor(attn, hidden_states, encoder_hidden_states=(text, ip))."""
    ref, hip = tiny_pair
    name = "mid_block.attentions.0.transformer_blocks.0.attn2"
    ra, ha = dict(ref.named_modules())[name], dict(hip.named_modules())[name]
    g = torch.Generator().manual_seed(8)
    h, text, ip = torch.randn(2, 64, 640, generator=g), torch.randn(2, 77, 768, generator=g), torch.randn(2, 5, 768, generator=g)
    with torch.no_grad():
        exp = ra(h, encoder_hidden_states=(text, ip))
        got = ha(h.cuda(), encoder_hidden_states=(text.cuda(), ip.cuda()))
        assert rel_l2(got, exp) < 2e-3
        assert rel_l2(ha.processor.to_v_ip_norm, ra.processor.to_v_ip_norm) < 1e-3
        got_list = ha(h.cuda(), encoder_hidden_states=(text.cuda(), [ip.cuda()]))
        assert torch.equal(got_list, got)
        got_cat = ha(h.cuda(), encoder_hidden_states=torch.cat([text, ip], 1).cuda())     # deprecated bare-tensor form
        assert torch.equal(got_cat, got)
    # grad-mode fusion rule (attention_processor.py:413-420), forced seeds
    for seed in (0.1, 0.5, 0.9):
        ra.processor.forced_fusion_seed = ha.processor.forced_fusion_seed = seed
        exp = ra(h, encoder_hidden_states=(text, ip)).detach()
        got = ha(h.cuda(), encoder_hidden_states=(text.cuda(), ip.cuda()))
        assert rel_l2(got, exp) < 2e-3
    ra.processor.forced_fusion_seed = ha.processor.forced_fusion_seed = None
    # stock self-attention processor
    name1 = "mid_block.attentions.0.transformer_blocks.0.attn1"
    ra1, ha1 = dict(ref.named_modules())[name1], dict(hip.named_modules())[name1]
    with torch.no_grad():
        assert rel_l2(ha1(h.cuda()), ra1(h)) < 2e-3


def test_training_shaped_forward_with_device_side_fusion(tiny_pair):
    """The forward a training step needs (train.py:495-506): P = 5 image tokens, per-sample timesteps (B,), and the grad-mode branch
    fusion of every cross-attention layer (attention_processor.py:413-420) drawn ON THE DEVICE (pv_fusion_draw) instead of the
    reference's per-layer `torch.rand(1).item()` host sync.  Forced u values per layer -> parity with the oracle in grad mode; free
    draws -> valid, changing, seed-reproducible."""
    ref, hip = tiny_pair
    g = torch.Generator().manual_seed(17)
    B, P = 2, 5
    x, text, ip = torch.randn(B, 4, 16, 16, generator=g), torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)
    t = torch.tensor([37, 911])
    eng = hip.engine(B, 16, 16, P, B, device_fusion="always", fusion_seed=1234)
    assert len(eng.fusion_names) == 4 and eng.fusion_tab.shape == (4, 2)
    eng.x_in.copy_(x); eng.text.copy_(text.reshape(-1, 768)); eng.ip.copy_(ip.reshape(-1, 768)); eng.timesteps.copy_(t.float())
    forced = [0.1, 0.5, 0.9, 0.3]                                   # -> (2,0), (1,1), (0,2), (2,0)
    eng.fusion_forced.copy_(torch.tensor(forced))
    got = eng.run().clone().cpu()
    assert eng.fusion_tab.cpu().tolist() == [[2.0, 0.0], [1.0, 1.0], [0.0, 2.0], [2.0, 0.0]]
    mods = dict(ref.named_modules())
    for name, u in zip(eng.fusion_names, forced):
        mods[name + ".transformer_blocks.0.attn2"].processor.forced_fusion_seed = u
    try:
        with torch.enable_grad():
            exp = ref(x, t, encoder_hidden_states=(text, ip)).sample.detach()
    finally:
        for name in eng.fusion_names:
            mods[name + ".transformer_blocks.0.attn2"].processor.forced_fusion_seed = None
    assert rel_l2(got, exp) < TOL_FWD
    with torch.no_grad():                                           # and it is NOT the no_grad result
        assert rel_l2(got, ref(x, t, encoder_hidden_states=(text, ip)).sample) > 10 * TOL_FWD
    # free draws: every row follows the rule, the pattern changes between launches, and is a function of (seed, launch index)
    eng.fusion_forced.fill_(-1.0)
    valid = {(2.0, 0.0), (0.0, 2.0), (1.0, 1.0)}
    seq = []
    for _ in range(12):
        eng.run()
        rows = [tuple(r) for r in eng.fusion_tab.cpu().tolist()]
        assert set(rows) <= valid
        seq.append(tuple(rows))
    assert len(set(seq)) > 3 and eng.fusion_rng[2].item() == 13
    counts = {v: sum(r == v for rows in seq for r in rows) for v in valid}
    assert all(c >= 4 for c in counts.values()), counts             # 48 draws, three outcomes of probability 1/3 each
    eng2 = hip.engine(B, 16, 16, P, B, device_fusion="always", fusion_seed=1234)
    eng2.x_in.copy_(x); eng2.text.copy_(text.reshape(-1, 768)); eng2.ip.copy_(ip.reshape(-1, 768)); eng2.timesteps.copy_(t.float())
    eng2.run()                                                      # launch 0 was the forced one above
    seq2 = []
    for _ in range(3):
        eng2.run()
        seq2.append(tuple(tuple(r) for r in eng2.fusion_tab.cpu().tolist()))
    assert seq2 == seq[:3]


def test_training_mode_loop_fuses_on_the_last_step_only(tiny_pair):
    """run_inference(training_mode=True) forward semantics (infer.py:99): only the LAST denoising step runs its forwards in grad
    mode.  One captured graph serves all steps; the device-side draw is keyed on the step counter."""
    from photoverse_amd.pipeline import DenoiseLoop
    _, hip = tiny_pair
    g = torch.Generator().manual_seed(23)
    B, P, T = 2, 5, 3
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, 16, 16, generator=g)
    plain = DenoiseLoop(hip, B, 16, P, T, 3.0)
    plain.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    plain.reset(noise)
    train = DenoiseLoop(hip, B, 16, P, T, 3.0, training_mode=True, fusion_seed=5)
    train.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    train.reset(noise)
    ones = [[1.0, 1.0]] * 4
    for step in range(T):
        plain.step(); train.step()
        tabs = [e.fusion_tab.cpu().tolist() for e in train.engines_u + train.engines_c]
        if step < T - 1:
            assert all(tb == ones for tb in tabs)
            assert torch.equal(plain.latents, train.latents)        # identical until the last step
        else:
            assert any(tb != ones for tb in tabs) and tabs[0] != tabs[1]     # 8 draws: uncond / cond forwards draw independently
            assert not torch.equal(plain.latents, train.latents) and torch.isfinite(train.latents).all()


@pytest.mark.parametrize("name,N", [("mid_block.attentions.0.transformer_blocks.0.attn2", 64), ("down_blocks.0.attentions.0.transformer_blocks.0.attn2", 200)])
def test_processor_backward_matches_oracle_autograd(tiny_pair, name, N):
    """BACKWARD of the reference's own processor on HIP: gradients of PhotoVerseAttnProcessor2_0 (grad mode, forced fusion draws)
    with respect to hidden_states, the text / image-token embeddings, to_k_ip / to_v_ip, to_q / to_k / to_v / to_out, and through
    to_v_ip_norm (the regulariser of train.py:512-513) - against torch autograd over the oracle processor."""
    ref, hip = tiny_pair
    ra, ha = dict(ref.named_modules())[name], dict(hip.named_modules())[name]
    C = ra.to_q.in_features
    g = torch.Generator().manual_seed(61)
    B, P = 2, 5
    h0, t0, i0 = torch.randn(B, N, C, generator=g), torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g)
    G = torch.randn(B, N, C, generator=g)
    plist = [("to_q.weight", lambda m: m.to_q.weight), ("to_k.weight", lambda m: m.to_k.weight), ("to_v.weight", lambda m: m.to_v.weight),
             ("to_out.0.weight", lambda m: m.to_out[0].weight), ("to_out.0.bias", lambda m: m.to_out[0].bias),
             ("to_k_ip", lambda m: m.processor.to_k_ip[0].weight), ("to_v_ip", lambda m: m.processor.to_v_ip[0].weight)]
    for seed in (0.5, 0.1, 0.9):
        ra.processor.forced_fusion_seed = ha.processor.forced_fusion_seed = seed
        res = []
        for mod, dev in ((ra, "cpu"), (ha, "cuda")):
            for _, get in plist:
                get(mod).requires_grad_(True)
                get(mod).grad = None
            h, t, i = (x.clone().to(dev).requires_grad_(True) for x in (h0, t0, i0))
            with torch.enable_grad():
                out = mod(h, encoder_hidden_states=(t, i))
                vn = mod.processor.to_v_ip_norm
                loss = (out.float() * G.to(dev)).sum() + 0.3 * vn.sum()
            loss.backward()
            res.append({"h": h.grad, "t": t.grad, "i": i.grad, **{n: get(mod).grad for n, get in plist}})
        for k in res[0]:
            a, b = res[1][k], res[0][k]
            if b is None or b.abs().max() == 0:              # a branch the fusion draw dropped (e.g. to_k_ip under text-only fusion)
                assert a is None or a.abs().max() < 1e-6, k
                continue
            assert a is not None and a.shape == b.shape, k
            assert rel_l2(a, b) < 4e-3, (k, seed, rel_l2(a, b))      # measured 4e-4 .. 1.5e-3 (the reference-code fixture: tests/test_reference_pins_gpu.py)
    ra.processor.forced_fusion_seed = ha.processor.forced_fusion_seed = None
    for _, get in plist:
        get(ha).grad = None
        get(ra).grad = None


def test_cpu_tensor_is_refused(tiny_pair):
    _, hip = tiny_pair
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip(torch.randn(1, 4, 16, 16), torch.tensor(1), encoder_hidden_states=(torch.randn(1, 77, 768), torch.randn(1, 1, 768)))


# fp16-storage tolerance for a short denoise loop on the tiny config (latents, rel-L2 vs fp32 oracle; measured <= 2e-3)
TOL_LOOP = 2.5e-3


@pytest.mark.parametrize("steps,P", [(3, 1), (4, 5)])
def test_denoise_loop_matches_oracle_and_graph_equals_eager(tiny_pair, steps, P):
    from oracle.infer_ref import denoise_ref, draw_noise_ref
    from photoverse_amd.pipeline import DenoiseLoop
    ref, hip = tiny_pair
    g = torch.Generator().manual_seed(21)
    B = 2
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = draw_noise_ref(B, 4, 16, seed=5)
    exp = denoise_ref(ref, noise, cond, uncond, guidance_scale=7.5, timesteps=steps)
    outs = []
    for use_graph, two in ((False, False), (True, False), (True, True)):
        loop = DenoiseLoop(hip, B, 16, P, steps, 7.5, use_graph=use_graph, two_streams=two)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.reset(noise)
        outs.append(loop.run().clone().cpu())
        assert loop.state[0].item() == steps
    assert torch.equal(outs[0], outs[1])                       # graph replay == eager launches, bit for bit
    assert torch.equal(outs[0], outs[2])                       # two overlapping graph branches (uncond || cond) change nothing
    assert rel_l2(outs[2], exp) < TOL_LOOP
    # replay again from the same noise: deterministic
    loop.reset(noise)
    assert torch.equal(loop.run().cpu(), outs[2])
    # a step past the end of the schedule raises on the host (the device tables have exactly `steps` rows) until reset()
    with pytest.raises(RuntimeError, match="reset"):
        loop.step()
    loop.reset(noise)
    loop.step()
    assert loop.state[0].item() == 1 and loop.state[1].item() == steps


def test_fifty_step_loop_latent_tolerance(tiny_pair, golden_dir):
    """The stated fp16 latent tolerance: 50-step CFG loop (guidance 7.5) on the tiny config vs the fp32 oracle (expectation computed in the
    build container by oracle/make_fullsize_golden.py tiny50: same seeds as here; the full-size counterpart is
    tests/test_fullsize_gpu.py::test_headline_schedule_latents_within_north_star_tolerance)."""
    from oracle.infer_ref import draw_noise_ref
    from photoverse_amd.pipeline import DenoiseLoop
    _ref, hip = tiny_pair
    fx = torch.load(os.path.join(golden_dir, "full_tiny50.pt"), weights_only=True)
    g = torch.Generator().manual_seed(fx["cond_seed"])
    B, P = 1, 1
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = draw_noise_ref(B, 4, 16, seed=fx["noise_seed"])
    loop = DenoiseLoop(hip, B, 16, P, 50, 7.5)
    loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
    loop.reset(noise)
    got = loop.run().cpu()
    err = rel_l2(got, fx["latents_50step"])
    print(f"50-step latents rel-L2 vs fp32 oracle: {err:.3e}")
    assert torch.isfinite(got).all()
    assert err < 1.5e-3          # measured 7.9e-4 .. 8.1e-4 on MI355X (north_star target 1e-3); headroom for fp32 summation-order variation


def test_bench_contract_line(tmp_path):
    """bench.py prints ONE JSON line with the driver's contract keys plus, under --full, the roofline object (short run, no CPU baseline);
    a plain run leaves the separately labelled objects null and --dump-outputs writes the latents of its last timed step."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f16" and "workload" in d["config"] and d["finite"] is True
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_stale", "kernel", "avg_launch_us", "runner_up"):
        assert k in rf, k
    # the two symbols with the largest shares of a step's flops: the d = 40 self-attention kernel and the 3x3 conv of the 64 x 64 level (patch form)
    assert {rf["kernel"].split("<")[0], rf["runner_up"]["kernel"].split("<")[0]} == {"attn8_kernel", "big_tile_kernel"}
    assert rf["runner_up"]["kernel"] != rf["kernel"] and 0.02 < rf["runner_up"]["frac"] < 1.0
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert 0.05 < rf["frac"] < 1.0
    # derived label, self-verifying multi-GPU fields, the attn2 branch over ALL layers
    assert d["config"]["workload"].startswith("configs[1] shape timed over 3 steps") and d["rccl_world"] == 1
    assert d["ms_per_step_ranks"]["n"] == 1 and d["ms_per_step_ranks"]["max"] == pytest.approx(d["ms_per_step"], rel=1e-3)
    xa = d["xattn_fused"]
    assert set(xa["levels"]) == {"320", "640", "1280"} and xa["levels"]["320"]["fused"] and xa["levels"]["320"]["launches_per_layer"] == 1
    assert xa["levels"]["640"]["fused"] and xa["levels"]["640"]["launches_per_layer"] == 1
    # C = 1280: norm2 + to_q + both SDPAs head-parallel in one launch, to_out + residual as a GEMM (round 3: four launches)
    assert not xa["levels"]["1280"]["fused"] and xa["levels"]["1280"]["head_parallel"] and xa["levels"]["1280"]["launches_per_layer"] == 2
    assert xa["all_layers"]["layers_per_step"] == 32 and 0.02 < xa["all_layers"]["frac"] < 1.0 and xa["north_star_target_frac"] == 0.40
    # P = 5 (token_index = 'full') next to the P = 1 headline
    assert d["ip_tokens_5"]["finite"] is True and 0.8 * d["value"] < d["ip_tokens_5"]["value"] < 1.1 * d["value"]
    assert d["configs4_per_rank"]["finite"] is True and d["configs4_per_rank"]["value"] > 0 and "96x96" in d["configs4_per_rank"]["workload"]
    # the optional shared-prefix loop: a separately labelled number, never the headline
    sp = d["shared_prefix"]
    assert sp["what"].startswith("NOT the headline") and 0.97 < sp["flops_vs_two_full_forwards"] < 0.98 and sp["launches_per_step"] < d["config"]["launches_per_step"]
    assert sp["value"] > 0.9 * d["value"]
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--batch", "2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                        capture_output=True, text=True, timeout=600, cwd=root)
    assert r2.returncode == 0, r2.stderr[-2000:]
    d2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][0])
    assert d2["config"]["workload"].startswith("custom shape (NOT a BASELINE config)")
    assert d2["full"] is False and d2["steps"] == 2 and d2["ms_per_step"] > 0
    for k in ("roofline", "xattn_fused", "shared_prefix", "ip_tokens_5", "configs4_per_rank", "train_forward", "train_step", "cpu_baseline"):
        assert d2[k] is None, k
    lat = np.load(tmp_path / "latents.npy")
    assert lat.dtype == np.float32 and lat.shape == (2, 4, 64, 64) and np.isfinite(lat).all() and lat.std() > 0


def test_bench_under_torch_distributed_run_uses_rccl_and_agrees_with_the_plain_run():
    """The driver's N > 1 launch form with ONE rank: `python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` initialises RCCL,
    runs the barrier / all_gather path (`force=True`) with `rccl_world` = 1 taken from the process group and every rank's own ms_per_step in
    the line.  Throughput is compared with the plain run only as a sanity bound (two processes on a shared pool: timing is not a correctness
    property), the gathered latents as a finite flag."""
    import json
    import os
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--gpus", "1", "--steps", "20", "--warmup", "4", "--no-cpu-baseline", "--no-roofline", "--no-train-forward"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    plain = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *common], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert plain.returncode == 0, plain.stderr[-2000:]
    dist = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                           "--master-port", "29533", os.path.join(root, "bench.py"), *common], capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert dist.returncode == 0, dist.stderr[-2000:]
    a = json.loads([l for l in plain.stdout.splitlines() if l.startswith("{")][-1])
    b = json.loads([l for l in dist.stdout.splitlines() if l.startswith("{")][-1])
    assert a["collective"].startswith("none") and b["collective"].startswith("all_gather_into_tensor over RCCL") and b["rccl_world"] == 1
    assert b["n_gpus"] == 1 and b["ms_per_step_ranks"]["n"] == 1 and b["finite"] is True
    print(f"plain {a['value']:.2f} steps/s vs under torch.distributed.run (RCCL) {b['value']:.2f} steps/s")
    assert 0.5 * a["value"] < b["value"] < 2.0 * a["value"]


# ---------------------------------------------------------------------------------------------------------------------
# headline-config coverage that needs no oracle time: batch invariance at bs=16, full model size (BASELINE configs[1])
def test_bs16_full_size_samples_match_bs1_runs(monkeypatch, full_hip_unet):
    """configs[1] beyond `finite`: 2 graph-replayed CFG steps at the headline shape (full SD-v1.5 size, bs=16, 64x64 latents,
    guidance 7.5); sample i of the batch must equal the bs=1 run of the same sample.  Samples never interact inside the UNet
    and no kernel's arithmetic depends on the batch, EXCEPT the split-K decision (small-M layers split K, which changes the fp32
    summation order): with split-K disabled the two runs are BIT-IDENTICAL; with the default heuristic they differ by the fp16
    storage noise (a different fp32 rounding flips fp16 roundings downstream - measured 1e-3 per forward, the same size as the
    error against the fp32 oracle), which guidance 7.5 amplifies in a 2-step loop."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from photoverse_amd import ops
    from photoverse_amd.pipeline import DenoiseLoop
    hip = full_hip_unet
    g = torch.Generator().manual_seed(77)
    B, P, T = 16, 1, 2
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, 64, 64, generator=g)

    def run_pair():
        big = DenoiseLoop(hip, B, 64, P, T, 7.5)
        big.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        big.reset(noise)
        full = big.run().clone().cpu()
        del big
        one = DenoiseLoop(hip, 1, 64, P, T, 7.5)
        singles = {}
        for i in (0, 7, 15):
            one.set_conditioning(tuple(t[i:i + 1].cuda() for t in cond), tuple(t[i:i + 1].cuda() for t in uncond))
            one.reset(noise[i:i + 1])
            singles[i] = one.run().clone().cpu()
        return full, singles

    monkeypatch.setattr(ops, "SPLITK_MAX", 1)            # no split-K anywhere: the bs=1 plan runs the same arithmetic as the bs=16 plan
    # ONE self-attention kernel per shape: the d = 40 launches take the 8-wave staggered kernel where they fill the chip (bs = 16) and the
    # 4-wave kernel below that (bs = 1); the two move the softmax reference at different moments (equal to rounding, not to the bit)
    monkeypatch.setenv("PV_ATTN8_MIN", "1")
    # ... and ONE conv tile: the 64 x 64 convs run on the LDS-resident-patch form of the 256-row tile at bs = 16 (32-channel-chunk-major K order) and on
    # the 128-row kernel at bs = 1 (64-channel-chunk major, as the gathered form of the 256-row tile, which is what this half of the test pins)
    monkeypatch.setenv("PV_CONV_PATCH", "0")
    full, singles = run_pair()
    assert torch.isfinite(full).all()
    for i, s1 in singles.items():
        assert torch.equal(full[i:i + 1], s1), f"sample {i} of the bs=16 run differs from its bs=1 run with split-K off"
    monkeypatch.undo()
    full2, singles2 = run_pair()                          # default split-K heuristic (what the bench runs)
    worst = max(rel_l2(full2[i:i + 1], s1) for i, s1 in singles2.items())
    print(f"bs=16 sample vs its bs=1 run (default split-K), 2 CFG steps, full size: worst rel-L2 = {worst:.3e}")
    assert worst < 4e-3


@pytest.mark.parametrize("merge", [True, False])
def test_shared_prefix_of_the_two_cfg_forwards_is_exact(full_hip_unet, merge):
    """``DenoiseLoop(share_prefix=True)`` (verdict item 9, opt-in: the headline counts two full forwards): conv_in, the first ResnetBlock and the first
    transformer block up to attn1 see neither text nor image tokens, so the uncond and cond forwards of a step compute them on identical inputs; recorded
    once, both branches start from the same tensors.  Same kernels, same inputs: the latents are BIT-identical, with fewer launches per step."""
    from photoverse_amd.pipeline import DenoiseLoop
    hip = full_hip_unet
    B, S, P, T = 2, 64, 1, 3
    g = torch.Generator().manual_seed(91)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)

    def run(share):
        loop = DenoiseLoop(hip, B, S, P, T, 7.5, merge_lowres=merge, share_prefix=share)
        assert loop.share_prefix == share and len(loop.engines_p) == (1 if share else 0)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.reset(noise)
        out = loop.run().clone().cpu()
        n, fl = loop.launches_per_step, sum(t[1] for e in loop.all_engines for t in e.rec.tags)
        del loop
        return out, n, fl

    a, na, fa = run(True)
    b, nb, fb = run(False)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert na < nb and 0.97 * fb < fa < 0.98 * fb        # 2.5 % of a step's algorithmic flops are computed once instead of twice
    print(f"shared CFG prefix: launches per step {na} vs {nb}, algorithmic flops {fa / fb:.4f} of two full forwards")


@pytest.mark.parametrize("B,S,P", [(4, 64, 1), (2, 96, 6)])
def test_lowres_merge_of_the_two_cfg_forwards_changes_nothing_per_sample(full_hip_unet, monkeypatch, B, S, P):
    """``DenoiseLoop(merge_lowres=True)`` (default) runs the 16 x 16 / 8 x 8 levels and the mid block of the uncond and cond forwards as ONE plan over
    both branches' samples (three plans per step: heads, merged part, tails).  Samples never interact inside the UNet: with split-K off the
    latents equal the two-plan loop's BIT FOR BIT (every kernel accumulates each output in the same order whatever the tile or batch); with the
    default split-K heuristic (which sees a different M) they agree to rounding.  Second case: BASELINE configs[4]'s per-rank latent size and token count
    (96 x 96: the seams sit at 24 x 24 = 9 statistics blocks per sample and 48 x 48)."""
    from photoverse_amd import ops
    from photoverse_amd.pipeline import DenoiseLoop
    hip = full_hip_unet
    g = torch.Generator().manual_seed(77)
    T = 2
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)

    def run(merge):
        loop = DenoiseLoop(hip, B, S, P, T, 7.5, merge_lowres=merge)
        assert loop.merge_lowres == merge and len(loop.engines_m) == (1 if merge else 0)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.reset(noise)
        out = loop.run().clone().cpu()
        n = loop.launches_per_step
        del loop
        return out, n

    monkeypatch.setattr(ops, "SPLITK_MAX", 1)
    a, na = run(True)
    b, nb = run(False)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    monkeypatch.undo()
    a2, _ = run(True)
    b2, _ = run(False)
    err = rel_l2(a2, b2)
    print(f"low-resolution CFG merge vs two whole forwards (default split-K): rel-L2 {err:.2e}; launches per step {na} vs {nb}")
    assert err < 4e-3 and na < nb           # measured 4e-4 (64 x 64) .. 2.1e-3 (96 x 96): fp32 summation order of different split-K choices through two random-init UNet steps


def test_seam_statistics_are_not_adopted_when_the_gemm_epilogue_does_not_write_them(full_hip_unet, monkeypatch):
    """with the PV_NO_COLSTATS A/B switch ``Recorder.gemm`` leaves the caller-owned seam statistics buffers of the
    low-resolution merge untouched (zeros).  The consuming plans must then run GroupNorm's own statistics pass instead of adopting the
    buffers (mean = var = 0 -> silently wrong latents); the shared prefix must not raise a KeyError either."""
    from photoverse_amd import ops
    from photoverse_amd.pipeline import DenoiseLoop
    hip = full_hip_unet
    B, S, P, T = 2, 64, 1, 2
    g = torch.Generator().manual_seed(78)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)

    def run(**kw):
        loop = DenoiseLoop(hip, B, S, P, T, 7.5, merge_lowres=True, **kw)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.reset(noise)
        out = loop.run().clone().cpu()
        del loop
        return out

    want = run()
    monkeypatch.setattr(ops, "_NO_COLSTATS", True)
    got = run()
    got_prefix = run(share_prefix=True)
    assert torch.isfinite(got).all()
    err, err_p = rel_l2(got, want), rel_l2(got_prefix, want)
    print(f"merged loop with GroupNorm statistics by a pass (PV_NO_COLSTATS) vs epilogue statistics: rel-L2 {err:.2e}, with the shared prefix {err_p:.2e}")
    assert err < 2e-3 and err_p < 2e-3


def test_groupnorm_folds_change_nothing_in_the_loop(full_hip_unet, monkeypatch):
    """Round 5's two GroupNorm folds at full size: Transformer2DModel.norm -> proj_in on the row-owning launch (default ON: compared with the two-launch
    path to rounding - the GEMM behind the norm changes kernel) and ResnetBlock2D.norm1 / norm2 + SiLU -> conv1 / conv2 on the LDS-resident patch
    (``Recorder.GN_FOLD``, default OFF: the conv consumes the same fp16 values either way, so the latents are BIT-IDENTICAL with and without it)."""
    from photoverse_amd import ops, unet as unet_mod
    from photoverse_amd.pipeline import DenoiseLoop
    hip = full_hip_unet
    B, S, P, T = 8, 64, 1, 2                 # 8 samples: the 64 x 64 convs are 128 tiles per branch = on the 256-row tile
    g = torch.Generator().manual_seed(79)
    cond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    uncond = (torch.randn(B, 77, 768, generator=g), torch.randn(B, P, 768, generator=g))
    noise = torch.randn(B, 4, S, S, generator=g)

    def run():
        loop = DenoiseLoop(hip, B, S, P, T, 7.5)
        loop.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        loop.reset(noise)
        out = loop.run().clone().cpu()
        syms = {t[0] for e in loop.all_engines for t in e.rec.tags}
        n = loop.launches_per_step
        del loop
        return out, syms, n

    base, syms0, n0 = run()
    assert any(s_.startswith("big_tile_kernel<true, false, 8, 3") for s_ in syms0) and not any(", 8, 5, false>" in s_ for s_ in syms0)
    monkeypatch.setattr(ops.Recorder, "GN_FOLD", True)
    fold, syms1, n1 = run()
    assert any(", 8, 5, false>" in s_ for s_ in syms1) and n1 < n0
    assert torch.isfinite(base).all() and torch.equal(fold, base)
    monkeypatch.undo()
    monkeypatch.setattr(unet_mod, "GN_PROJ_IN", False)
    plain, _, n2 = run()
    err = rel_l2(base, plain)
    print(f"GroupNorm folds: conv fold bit-identical ({n1} vs {n0} launches per step); proj_in fold vs two launches rel-L2 {err:.2e} ({n0} vs {n2} launches)")
    assert n0 < n2 and err < 2e-3


def _two_rank_loop_worker(rank, world, port, q):
    """One rank of the batch-sharded path on the REAL HIP loop: shard of the CPU-drawn global batch -> DenoiseLoop -> the single
    gather (gloo here: both test ranks share the box's one GPU, where RCCL refuses duplicate devices)."""
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PV_SPLITK_MAX="1")   # no split-K: batch-invariant arithmetic
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle.unet_ref import TINY_CONFIG
    from photoverse_amd.pipeline import DenoiseLoop, gather_latents, shard_batch
    from photoverse_amd.unet import UNet2DConditionModel, set_visual_cross_attention_adapter
    torch.manual_seed(0)
    hip = UNet2DConditionModel(**TINY_CONFIG)
    set_visual_cross_attention_adapter(hip, (5,))
    hip.to("cuda:0")
    g = torch.Generator().manual_seed(55)
    GB, P, T = 4, 1, 3
    cond = (torch.randn(GB, 77, 768, generator=g), torch.randn(GB, P, 768, generator=g))
    uncond = (torch.randn(GB, 77, 768, generator=g), torch.randn(GB, P, 768, generator=g))
    noise = torch.randn(GB, 4, 16, 16, generator=torch.manual_seed(9))        # global draw, infer.py:52-59 semantics
    sl = shard_batch(GB, rank, world)
    loop = DenoiseLoop(hip, GB // world, 16, P, T, 7.5)
    loop.set_conditioning(tuple(t[sl].cuda() for t in cond), tuple(t[sl].cuda() for t in uncond))
    loop.reset(noise[sl])
    full = gather_latents(loop.run(), world, force=True).cpu()
    err = None
    if rank == 0:       # the 1-rank run of the whole batch
        one = DenoiseLoop(hip, GB, 16, P, T, 7.5)
        one.set_conditioning(tuple(t.cuda() for t in cond), tuple(t.cuda() for t in uncond))
        one.reset(noise)
        ref = one.run().cpu()
        err = ((full.double() - ref.double()).norm() / ref.double().norm()).item()
    q.put((rank, tuple(full.shape), err))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_loop_equals_one_rank_run():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_two_rank_loop_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(120)
    assert [r[:2] for r in res] == [(0, (4, 4, 16, 16)), (1, (4, 4, 16, 16))]
    print(f"2-rank sharded loop vs 1-rank run: rel-L2 = {res[0][2]:.3e}")
    assert res[0][2] == 0.0          # split-K off (its decision depends on the per-rank batch): sharded == unsharded, bit for bit

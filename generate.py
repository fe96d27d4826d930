#!/usr/bin/env python3
"""Inference CLI - counterpart of ``/root/reference/generate.py`` for the MI355X build.

Same flags and the same call into ``run_inference`` as the reference (``generate.py:21-34,82-85``); additions forced by
the offline environment: ``--model_path random`` (seeded random-init weights), ``--synthetic_input`` (no image / tokenizer
files needed), ``--seed``, ``--latent_size``.  Images are written as PNG like the reference (``generate.py:86-90``).

Beyond the reference: ``--mask_image_path`` (inpainting: white = regenerate) with ``--target_image_path`` (the photograph to edit; the identity
still comes from ``--input_image_path``), ``--strength`` (img2img: run only the last part of the schedule) and ``--no_paste_back``;
``--hires_latent_size`` (two-pass high-resolution generation: generate at ``--latent_size``, upscale the latents, re-noise them and run the last
``--hires_strength`` of a ``--hires_timesteps`` schedule at the large size; the images are ``8 * hires_latent_size`` pixels);
``--image_guidance_scale`` (a guidance scale of its own for the identity - the image tokens - beside ``--guidance_scale`` for the prompt: a third
forward per step) and ``--guidance_rescale`` (renormalise the guided prediction against the over-saturation of high scales);
``--sampler sde-dpmsolver++`` (the stochastic form of the solver, "DPM++ 2M SDE": fresh noise at every step, keyed on ``--seed``).

``--pag_scale`` (perturbed-attention guidance: one more forward per step with the self-attention map of the ``--pag_layers`` transformers replaced by
the identity, and the prediction pushed away from it - repairs eyes, teeth and symmetry at low ``--guidance_scale`` without raising it) and
``--pag_layers`` (name prefixes of the UNet's transformers such as ``mid_block`` or ``up_blocks.1``, or ``all``; default the mid block).

``--freeu B1 B2 S1 S2`` (FreeU: in the first two decoder blocks the first half of the backbone's channels is scaled by ``B1`` / ``B2`` and the skip
connection's lowest frequencies by ``S1`` / ``S2``; the authors' values for SD-1.5 are ``1.5 1.6 0.9 0.2``; no additional forward).

``--controlnet_path DIR|random`` with ``--control_image_path`` (ControlNet: a pose, edge or depth map, resized to the working resolution and scaled to
[0, 1], steers the layout; ``random`` is a ControlNet copied from the UNet with a seeded non-zero init of its zero convs, or with no image path a
synthetic checkerboard - for smoke runs) and ``--controlnet_conditioning_scale``.

``--kv_downsample F`` (token downsampling, ToDo: in the self-attention of the ``--kv_downsample_layers`` transformers - default those of the
highest-resolution level - every query attends to keys and values pooled ``F`` per side, 2 ... 8: a quarter of that attention work at 2; approximate, no
additional forward), ``--kv_downsample_method avg|nearest`` (block means, the default because it aliases less, or the top-left token) and
``--hires_kv_downsample F`` (the factor of the second pass of a ``--hires_latent_size`` run; default the same as ``--kv_downsample``, 1 = off there.
The intended use: ``--hires_latent_size 96 --hires_kv_downsample 2`` - an exact first pass, a pooled second one).

``--window S`` (windowed denoising, MultiDiffusion: every step denoises the overlapping ``S x S`` windows of the latent canvas as one batch and sets the
canvas to their weighted mean, so the UNet works at its training size whatever the picture's), ``--window_stride`` (default ``S // 2``),
``--window_weights uniform|gaussian``, ``--latent_height`` / ``--latent_width`` (a portrait or panorama canvas; default ``--latent_size``, need
``--window``) and ``--hires_window`` / ``--hires_window_stride`` (the same for the second pass of a ``--hires_latent_size`` run).

``--upscaler_path FILE|random`` (Real-ESRGAN's RRDBNet, ``RealESRGAN_x4plus.pth``: the images ``run_inference`` returns are upscaled 4x before they are saved -
it runs after the call, so it composes with every flag above), ``--upscaler_blocks`` (the size of the ``random`` network; 23 is x4plus), ``--upscale_tile``
and ``--upscale_tile_pad`` (Real-ESRGAN's tiling: input tiles with a margin of real neighbourhood, cropped without blending).
"""
import argparse
import os

import torch

from photoverse_amd.infer import run_inference
from photoverse_amd.modeling_utils import load_models

parser = argparse.ArgumentParser(description="Run PhotoVerse inference on MI355X")
parser.add_argument("--model_path", type=str, default="random", help="Local HF-layout model directory, or 'random'")
parser.add_argument("--extra_num_tokens", type=int, default=4, help="Number of additional tokens")
parser.add_argument("--encoder_layers_idx", nargs="+", type=int, default=[4, 8, 12, 16], help="Indices of image encoder layers")
parser.add_argument("--guidance_scale", type=float, default=1.0, help="Guidance scale")
parser.add_argument("--checkpoint_path", type=str, default=None, help="Path to a photoverse*.pt checkpoint")
parser.add_argument("--input_image_path", type=str, default=None, help="Path to the input image (needs PIL)")
parser.add_argument("--output_image_path", type=str, default="generated_image", help="Prefix for the outputs")
parser.add_argument("--num_timesteps", type=int, default=25, help="Number of timesteps for inference")
parser.add_argument("--results_dir", type=str, default="results", help="Directory to save the outputs")
parser.add_argument("--text", type=str, default="a photo of a {}", help="Prompt template")
parser.add_argument("--negative_prompt", type=str, default=None, help="Negative prompt")
parser.add_argument("--num_of_samples", type=int, default=None, help="Number of samples to generate")
parser.add_argument("--from_noised_image", action="store_true", help="Use noised image as input (needs a VAE)")
parser.add_argument("--synthetic_input", action="store_true", help="Random CLIP pixels instead of an image file")
parser.add_argument("--seed", type=int, default=None)
parser.add_argument("--latent_size", type=int, default=64)
parser.add_argument("--image_encoder_path", type=str, default=None,
                    help="Local directory of openai/clip-vit-large-patch14 (default: <model_path>/image_encoder)")
parser.add_argument("--mask_image_path", type=str, default=None,
                    help="Greyscale mask, white = regenerate (nearest-neighbour resize to the working resolution): inpaint the target image (needs a VAE)")
parser.add_argument("--target_image_path", type=str, default=None, help="The photograph to edit (default: the input image)")
parser.add_argument("--strength", type=float, default=1.0,
                    help="Fraction of the schedule to run, starting from the noised image (with --from_noised_image or --mask_image_path)")
parser.add_argument("--no_paste_back", action="store_true", help="Return the decoded image as it is instead of the target's own pixels outside the mask")
parser.add_argument("--hires_latent_size", type=int, default=None,
                    help="Second pass at this latent size (>= --latent_size): upscale the first pass's latents, re-noise and refine them")
parser.add_argument("--hires_strength", type=float, default=0.5, help="Fraction of the second pass's schedule to run (with --hires_latent_size)")
parser.add_argument("--hires_timesteps", type=int, default=None, help="Steps of the second pass's schedule (default: --num_timesteps)")
parser.add_argument("--image_guidance_scale", type=float, default=None,
                    help="Guidance scale of the image tokens (identity); --guidance_scale then weighs the prompt alone (default: one scale for both)")
parser.add_argument("--guidance_rescale", type=float, default=0.0,
                    help="In [0, 1]: scale the guided noise prediction towards the conditional one's standard deviation (0 = off)")
parser.add_argument("--sampler", choices=["dpmsolver++", "sde-dpmsolver++"], default="dpmsolver++",
                    help="dpmsolver++: deterministic DPM-Solver++(2M); sde-dpmsolver++: its stochastic form (fresh noise per step, drawn on the device)")
parser.add_argument("--pag_scale", type=float, default=None,
                    help="Perturbed-attention guidance scale (one more forward per step with identity self-attention maps in --pag_layers; default off)")
parser.add_argument("--pag_layers", nargs="+", type=str, default=["mid_block"],
                    help="Transformers whose self-attention is perturbed: name prefixes (mid_block, up_blocks.1, down_blocks.0.attentions.0, ...) or all")
parser.add_argument("--freeu", nargs=4, type=float, default=None, metavar=("B1", "B2", "S1", "S2"),
                    help="FreeU: backbone scales B1 B2 and skip low-frequency scales S1 S2 of the first two decoder blocks (SD-1.5: 1.5 1.6 0.9 0.2; default off)")
parser.add_argument("--controlnet_path", type=str, default=None,
                    help="Directory with a ControlNet's diffusion_pytorch_model.safetensors (diffusers layout), or 'random' (copied from the UNet, seeded non-zero zero convs and a seeded re-draw of the embedding's convs)")
parser.add_argument("--control_image_path", type=str, default=None, help="The control image (pose / edges / depth); resized to 8 * latent_size, scaled to [0, 1]")
parser.add_argument("--controlnet_conditioning_scale", type=float, default=1.0, help="Scale of the ControlNet's residuals (0 = off)")
parser.add_argument("--kv_downsample", type=int, default=None,
                    help="Token downsampling: pool the self-attention keys / values of --kv_downsample_layers by this factor per side (2 ... 8; default off)")
parser.add_argument("--kv_downsample_method", choices=["avg", "nearest"], default="avg",
                    help="avg: block means (aliases less); nearest: the top-left token of every block")
parser.add_argument("--kv_downsample_layers", nargs="+", type=str, default=None,
                    help="Transformers whose keys / values are pooled: name prefixes as --pag_layers takes them, or all (default: the highest-resolution level)")
parser.add_argument("--hires_kv_downsample", type=int, default=None,
                    help="The factor in the second pass (with --hires_latent_size; default: --kv_downsample, 1 = off in the second pass)")
parser.add_argument("--window", type=int, default=None,
                    help="Windowed denoising (MultiDiffusion): denoise overlapping windows of this latent size and average them (default off)")
parser.add_argument("--window_stride", type=int, default=None, help="Distance between two windows (default: --window // 2)")
parser.add_argument("--window_weights", choices=["uniform", "gaussian"], default="uniform",
                    help="uniform: the plain mean of the windows (MultiDiffusion); gaussian: windows weigh most at their centre (Mixture of Diffusers)")
parser.add_argument("--hires_window", type=int, default=None, help="Windowed denoising in the second pass (with --hires_latent_size)")
parser.add_argument("--hires_window_stride", type=int, default=None, help="Distance between two windows of the second pass (default: --hires_window // 2)")
parser.add_argument("--latent_height", type=int, default=None, help="Height of the latent canvas (default: --latent_size; needs --window)")
parser.add_argument("--latent_width", type=int, default=None, help="Width of the latent canvas (default: --latent_size; needs --window)")
parser.add_argument("--vae_tiling", action="store_true",
                    help="vae.enable_tiling(): decode / encode images larger than one tile in overlapping tiles with blended seams (large --hires_latent_size)")
parser.add_argument("--vae_tile_size", type=int, default=512, help="tile_sample_min_size of --vae_tiling, in pixels")
parser.add_argument("--vae_tile_overlap", type=float, default=0.25, help="tile_overlap_factor of --vae_tiling")
parser.add_argument("--vae_flash_attention", action="store_true",
                    help="vae.enable_flash_attention(): the VAE mid-block attention as one flash launch with no score matrix (untiled decode of large latents)")
parser.add_argument("--vae_tiny_path", type=str, default=None,
                    help="AutoencoderTiny (TAESD) directory, or 'random' for seeded random weights: the tiny autoencoder replaces the VAE in run_inference")
parser.add_argument("--upscaler_path", type=str, default=None,
                    help="Real-ESRGAN RRDBNet weights (RealESRGAN_x4plus.pth or a .safetensors of the same names), or 'random' for seeded random weights: "
                         "the generated images are upscaled 4x before they are saved")
parser.add_argument("--upscaler_blocks", type=int, default=None, help="RRDB blocks of --upscaler_path random (default 23, the x4plus size; a file brings its own)")
parser.add_argument("--upscale_tile", type=int, default=None,
                    help="Upscale in tiles of this many input pixels per side (Real-ESRGAN's tile; default: the whole image where it fits)")
parser.add_argument("--upscale_tile_pad", type=int, default=10, help="Pixels of real neighbourhood around every tile of --upscale_tile, cropped from its output")
parser.add_argument("--tiny", action="store_true", help="Small random-init model (smoke tests of the CLI; needs --model_path random)")


def prepare_example(args, tokenizer):
    """Output format of ``datasets/utils.py:160-199`` (prepare_prompt) + ``generate.py:53-61``."""
    n = args.num_of_samples or 1
    placeholder = "*"
    text = args.text.format(placeholder)
    ids = tokenizer([text] * n, padding="max_length", max_length=tokenizer.model_max_length, return_tensors="pt").input_ids
    idx = text.split().index(placeholder) + 1                     # + BOS (datasets/utils.py:215-220)
    example = {"text": [text] * n, "text_input_ids": ids, "concept_placeholder_idx": torch.full((n, 1), idx, dtype=torch.int64)}
    if args.negative_prompt is not None:
        example["negative_text_input_ids"] = tokenizer([args.negative_prompt] * n, padding="max_length",
                                                       max_length=tokenizer.model_max_length, return_tensors="pt").input_ids
    if args.synthetic_input or args.input_image_path is None:
        g = torch.Generator().manual_seed(0 if args.seed is None else args.seed)
        example["pixel_values_clip"] = torch.randn(1, 3, 224, 224, generator=g).repeat(n, 1, 1, 1)
        example["pixel_values"] = torch.zeros(n, 3, 8 * args.latent_size, 8 * args.latent_size)
    else:
        from PIL import Image
        from photoverse_amd.image_utils import clip_image_processor, preprocess_image
        raw_image = Image.open(args.input_image_path)
        if raw_image.mode != "RGB":
            raw_image = raw_image.convert("RGB")
        # generate.py:57-58: CLIPImageProcessor (short side 224 bicubic + centre crop) and preprocess_image (short side `size`
        # bicubic + centre crop, [-1, 1]); size = 8 * latent (512 for the reference's fixed latent_size 64)
        example["pixel_values_clip"] = clip_image_processor(raw_image)[None].repeat(n, 1, 1, 1)
        example["pixel_values"] = preprocess_image(raw_image, size=8 * args.latent_size, interpolation="bicubic")[None].repeat(n, 1, 1, 1)
    if getattr(args, "target_image_path", None) is not None:       # the photograph to edit; pixel_values_clip stays the identity image
        from PIL import Image
        from photoverse_amd.image_utils import preprocess_image
        example["pixel_values"] = preprocess_image(Image.open(args.target_image_path), size=8 * args.latent_size,
                                                   interpolation="bicubic")[None].repeat(n, 1, 1, 1)
    return example


def prepare_mask(args):
    """``--mask_image_path`` -> (1, 1, H, W) in {0, 1} at the resolution of ``pixel_values`` (shared by all samples), or None."""
    if getattr(args, "mask_image_path", None) is None:
        return None
    from PIL import Image
    from photoverse_amd.image_utils import preprocess_mask
    return preprocess_mask(Image.open(args.mask_image_path), size=8 * args.latent_size)[None]


def prepare_control(args, unet):
    """``--controlnet_path`` / ``--control_image_path`` -> (ControlNetModel on the UNet's device, control image (1, 3, H, W) in [0, 1]), or (None, None)."""
    if args.controlnet_path is None:
        if args.control_image_path is not None:
            raise SystemExit("--control_image_path needs --controlnet_path")
        return None, None
    from photoverse_amd.controlnet import ControlNetModel
    if args.controlnet_path == "random":
        cn = ControlNetModel.from_unet(unet).randomize_zero_convs_(seed=0 if args.seed is None else args.seed)
    else:
        cn = ControlNetModel.from_pretrained(args.controlnet_path, **{k: v for k, v in vars(unet.config).items()})
    side = 8 * args.latent_size
    if args.control_image_path is not None:
        from PIL import Image
        from photoverse_amd.image_utils import preprocess_image
        image = preprocess_image(Image.open(args.control_image_path).convert("RGB"), size=side, interpolation="bicubic")[None] * 0.5 + 0.5
    elif args.controlnet_path == "random":
        yy, xx = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
        image = (((yy // 32 + xx // 32) % 2).float())[None, None].repeat(1, 3, 1, 1)        # a checkerboard: something with edges for a smoke run
    else:
        raise SystemExit("--controlnet_path needs --control_image_path")
    return cn.to(unet.device), image.clamp(0, 1).contiguous()


def canvas_size(args):
    """The ``latent_size`` of ``run_inference``: ``--latent_size``, or with ``--latent_height`` / ``--latent_width`` the ``(H, W)`` pair of a windowed run."""
    if args.latent_height is None and args.latent_width is None:
        return args.latent_size
    if args.window is None:
        raise SystemExit("--latent_height / --latent_width need --window: without it the denoiser is one square plan of --latent_size")
    return (args.latent_size if args.latent_height is None else args.latent_height, args.latent_size if args.latent_width is None else args.latent_width)


def configure_vae(args, vae):
    """The VAE switches of the command line (--vae_tiling, --vae_flash_attention): the VAE object carries them into run_inference."""
    if args.vae_tiling:
        vae.enable_tiling(args.vae_tile_size, args.vae_tile_overlap)
    if args.vae_flash_attention:
        vae.enable_flash_attention()
    return vae


def prepare_vae_tiny(args, device):
    """``--vae_tiny_path`` -> an ``AutoencoderTiny`` on ``device`` (the ``vae`` of ``run_inference``), or None.  ``--vae_tiling`` and
    ``--vae_flash_attention`` are switches of ``AutoencoderKL``: combining them with it exits."""
    if args.vae_tiny_path is None:
        return None
    for flag in ("vae_tiling", "vae_flash_attention"):
        if getattr(args, flag):
            raise SystemExit(f"--{flag} is a switch of AutoencoderKL: it does not combine with --vae_tiny_path (AutoencoderTiny has no attention and is not tiled)")
    from photoverse_amd.vae_tiny import AutoencoderTiny
    if args.vae_tiny_path == "random":
        with torch.random.fork_rng(devices=[]):                   # the generation's own random stream stays what it is without the flag
            torch.manual_seed(0 if args.seed is None else args.seed)
            vae = AutoencoderTiny()
    else:
        vae = AutoencoderTiny.from_pretrained(args.vae_tiny_path)
    return vae.requires_grad_(False).to(device)


def select_vae(args, vae, device):
    """The object ``run_inference`` gets as its ``vae``: the tiny autoencoder of ``--vae_tiny_path``, else the loaded ``AutoencoderKL`` with its switches."""
    tiny = prepare_vae_tiny(args, device)
    return configure_vae(args, vae) if tiny is None else tiny


def check_upscaler_args(args):
    """The ``--upscaler_path`` / ``--upscale_*`` flags, checked before any model is loaded: a bad value exits with a message."""
    if args.upscaler_path is None:
        for flag in ("upscaler_blocks", "upscale_tile"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} needs --upscaler_path")
        return
    if args.upscaler_path == "random":
        if args.upscaler_blocks is not None and args.upscaler_blocks < 1:
            raise SystemExit(f"--upscaler_blocks must be >= 1, got {args.upscaler_blocks}")
    else:
        if args.upscaler_blocks is not None:
            raise SystemExit("--upscaler_blocks belongs to --upscaler_path random: a weight file brings its own block count")
        if not os.path.isfile(args.upscaler_path):
            raise SystemExit(f"--upscaler_path: no file at {args.upscaler_path}")
    if args.upscale_tile is not None and args.upscale_tile < 1:
        raise SystemExit(f"--upscale_tile must be >= 1, got {args.upscale_tile}")
    if args.upscale_tile_pad < 0:
        raise SystemExit(f"--upscale_tile_pad must be >= 0, got {args.upscale_tile_pad}")


def prepare_upscaler(args, device):
    """``--upscaler_path`` -> an ``RRDBNet`` on ``device``, or None."""
    check_upscaler_args(args)
    if args.upscaler_path is None:
        return None
    from photoverse_amd.upscaler import RRDBNet
    if args.upscaler_path == "random":
        net = RRDBNet(num_block=23 if args.upscaler_blocks is None else args.upscaler_blocks).randomize_(seed=0 if args.seed is None else args.seed)
    else:
        net = RRDBNet.from_pretrained(args.upscaler_path)
    return net.requires_grad_(False).to(device)


def upscale_images(args, upscaler, images):
    """The images ``run_inference`` returned, 4x larger through ``--upscaler_path`` (unchanged without it)."""
    if upscaler is None:
        return images
    return upscaler.upscale(images.float(), tile=args.upscale_tile, tile_pad=args.upscale_tile_pad)


if __name__ == "__main__":
    args = parser.parse_args()
    check_upscaler_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("generate.py needs a HIP device: photoverse_amd has no CPU path")
    device = torch.device("cuda")
    cfg = {}
    if args.tiny:
        if args.model_path != "random":
            raise SystemExit("--tiny builds a small random-init model: use it with --model_path random")
        cfg = dict(unet_config=dict(block_out_channels=(320, 640), layers_per_block=1, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                                    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D")),
                   vision_config=dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=max(args.encoder_layers_idx) + 1),
                   text_config=dict(hidden_size=768, num_attention_heads=12, intermediate_size=512, num_hidden_layers=2),
                   vae_config=dict(block_out_channels=(128, 128, 128, 128), layers_per_block=1))      # 4 levels: x8 like the real VAE
    tokenizer, text_encoder, vae, unet, image_encoder, image_adapter, text_adapter, scheduler, _ = load_models(
        None if args.model_path == "random" else args.model_path, args.extra_num_tokens, args.checkpoint_path,
        image_encoder_path=args.image_encoder_path, **cfg)
    for m in (vae, unet, text_encoder, image_encoder, image_adapter, text_adapter):
        m.to(device)
    vae = select_vae(args, vae, device)
    example = prepare_example(args, tokenizer)
    controlnet, control_image = prepare_control(args, unet)
    with torch.no_grad():
        out = run_inference(example, tokenizer, image_encoder, text_encoder, unet, text_adapter, image_adapter, vae, scheduler, device,
                            args.encoder_layers_idx, latent_size=canvas_size(args), guidance_scale=args.guidance_scale,
                            timesteps=args.num_timesteps, from_noised_image=args.from_noised_image, seed=args.seed,
                            strength=args.strength, inpaint_mask=prepare_mask(args), paste_back=not args.no_paste_back,
                            hires_latent_size=args.hires_latent_size, hires_strength=args.hires_strength, hires_timesteps=args.hires_timesteps,
                            image_guidance_scale=args.image_guidance_scale, guidance_rescale=args.guidance_rescale,
                            sampler=args.sampler, pag_scale=args.pag_scale, pag_layers=tuple(args.pag_layers),
                            freeu=None if args.freeu is None else tuple(args.freeu), controlnet=controlnet, control_image=control_image,
                            controlnet_conditioning_scale=args.controlnet_conditioning_scale, kv_downsample=args.kv_downsample,
                            kv_downsample_method=args.kv_downsample_method,
                            kv_downsample_layers=None if args.kv_downsample_layers is None else tuple(args.kv_downsample_layers),
                            hires_kv_downsample=args.hires_kv_downsample, window=args.window, window_stride=args.window_stride,
                            window_weights=args.window_weights, hires_window=args.hires_window, hires_window_stride=args.hires_window_stride)
        out = upscale_images(args, prepare_upscaler(args, device), out)
    os.makedirs(args.results_dir, exist_ok=True)
    from photoverse_amd.image_utils import denormalize, to_pil
    imgs = [to_pil(denormalize(img)) for img in out.float().cpu()]                            # generate.py:86
    for idx, img in enumerate(imgs):
        img.save(os.path.join(args.results_dir, f"{args.output_image_path}{idx}.png"))
    print(f"saved {len(imgs)} image(s) {tuple(out.shape[1:])} to {args.results_dir}/")

"""The negative-regions fixture shared by tests/test_negative_regions_host.py and tests/test_negative_regions_gpu.py (test infrastructure):
its constants and the fp32 CPU loop built from the oracle's pieces that both files compare against."""
import torch

import pww_cases as cases
from gpu_util import uninstall_all
from oracle import pww_oracle as O

# ---- the fixture: the runner example with its five regions ALSO named in the unconditional prompt (two regions alone move the oracle's
# latent by 0.25 - 0.28 at any strength and qk_gain tried: too close to twice the bf16 cap)
NEG_PROMPT = "blurry photo of a tree next to a dog and a cat, sky, ground, low quality"
NEG_CONTEXT = {(13, 255, 0): "tree,1.5", (255, 255, 255): "dog,1.0", (0, 0, 0): "cat,1.0", (90, 206, 255): "sky,1.0", (74, 18, 1): "ground,1.0"}
NEG_STRENGTH = 2.0
QK_GAIN = 2.0
STEPS = 10
CAP = {torch.float16: 2e-2, torch.bfloat16: 1e-1}       # tests/test_loop_gpu.py::test_tiny_loop_vs_reference
ORACLE_VISIBLE = 0.5623        # CPU-measured rel-L2(with, without) of the oracle (profiles/negative_regions.md; tests/test_negative_regions_host.py re-measures it)


def oracle_loop(neg_context, neg_strength, steps=STEPS, seed=0, wf=cases.weight_fn_runner, config="tiny", qk_gain=QK_GAIN,
                neg_prompt=NEG_PROMPT, extra=None):
    """fp32 CPU: oracle.sample_latents with the unconditional pass's zero lambda replaced by neg_strength * wf, over the dict the oracle's
    builder returns for (neg_context, neg_prompt). neg_context None: the reference's loop."""
    vae, unet, text, tok, sch = cases.build_tools(config, qk_gain=qk_gain)
    rgb = cases.load_example_rgb()
    O.install_oracle_attention(unet)
    try:
        extra_seeds, regions, cond, uncond = O.encode_text_color_inputs(text, tok, rgb, dict(cases.RUNNER_CONTEXT), cases.RUNNER_PROMPT, neg_prompt)
        uwf = lambda w, sigma, qk: 0.0      # noqa: E731
        if neg_context:
            _, _, uncond, _ = O.encode_text_color_inputs(text, tok, rgb, dict(neg_context), neg_prompt, "")
            uwf = lambda w, sigma, qk: neg_strength * wf(w, sigma, qk)      # noqa: E731
        latents = O.initial_latents(seed, 4, rgb.shape[0], rgb.shape[1], regions, extra_seeds)
        sch.set_timesteps(steps)
        latents = latents * sch.init_noise_sigma
        with torch.no_grad():
            for i, t in enumerate(sch.timesteps):
                sigma = sch.sigmas[i]
                x = sch.scale_model_input(latents, t)
                cond.update({"SIGMA": sigma, "WEIGHT_FUNCTION": wf})
                eps_c = unet(x, t, encoder_hidden_states=cond).sample
                uncond.update({"SIGMA": sigma, "WEIGHT_FUNCTION": uwf})
                eps_u = unet(x, t, encoder_hidden_states=uncond).sample
                latents = sch.step(O.cfg_combine(eps_c, eps_u, 7.5), t, latents).prev_sample
        return latents
    finally:
        uninstall_all()

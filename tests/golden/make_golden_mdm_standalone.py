#!/usr/bin/env python3
"""Generate tests/golden/mdm_standalone.npz: the reference's stand-alone MDM sampler (src/models/mdm.py:195-231) -- MDMDenoiser under
ClassifierFreeSampleModel(2.5) in MotionDiffusion(mode="individual") -- at ddim4 and ddim20 (builder container only; never on the GPU box).

Run:  python tests/golden/make_golden_mdm_standalone.py

Weights: reinit(MDMDenoiser(...), 33) at make_golden.DEN's sizes -- asserted EQUAL to mdm.npz's "w:mdm." set and not stored again.  B = 2, T = 12,
x_T = rnd(580) [B, T, 262], cond = rnd(581) [B, D] (what embed_text hands the denoiser).  Per loop the fixture keeps the reference's fp32 output and
the ratio of |fp32 - float64| to the project's loop bounds (mean 2e-3, p99 3e-2); above 0.25 the script refuses the draw.

A second pair of loops, "loop128:*", runs the same at latent 128 / ff 256 / 2 layers / 2 heads (head size 64: the smallest MDM the fp32_split mode covers),
cond = rnd(582) [B, 128].  Its weights are NOT stored (1.4 MB): they are reinit(..., 33)'s, i.e. every parameter N(0, 0.1) from
Generator(crc32(parameter name) + 33), which the test redraws from the names.
"""
import os
import numpy as np

from make_golden import torch, save, sd, reinit, MDMDenoiser, ClassifierFreeSampleModel, DEN, HERE
from make_golden_intergen import make_diffusion, f64_ratio

B, T = 2, 12
SEEDS = dict(x_T=580, cond=581)
CFG = 2.5


DEN128 = dict(DEN, latent_dim=128, ff_size=256)


def net(den=DEN):
    return reinit(MDMDenoiser(None, 262, den["latent_dim"], den["ff_size"], den["num_layers"], den["num_heads"], den["dropout"], "gelu"), 33)


def draw(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def run_loop(strategy, f64=False, den=DEN):
    orig_float = torch.Tensor.float
    m = net(den)
    if f64:
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self: self.double()
        m = m.double()
    try:
        dt = torch.float64 if f64 else torch.float32
        diff = make_diffusion("individual", strategy)
        return diff.ddim_sample_loop(ClassifierFreeSampleModel(m, CFG), (B, T, 262), noise=draw(SEEDS["x_T"], B, T, 262).to(dt), clip_denoised=False,
                                     progress=False, model_kwargs={"mask": None, "cond": draw(SEEDS["cond"] + (den is not DEN), B, den["latent_dim"]).to(dt)}, x_start=None)
    finally:
        torch.Tensor.float = orig_float
        torch.set_default_dtype(torch.float32)


def main():
    have = np.load(os.path.join(HERE, "mdm.npz"))
    for k, v in sd(net(), "mdm.").items():
        assert np.array_equal(have[k], v), k                # the weights are mdm.npz's: not stored twice
    out = dict(B=B, T=T, cfg_scale=CFG, H=DEN["num_heads"], seeds=np.array([SEEDS["x_T"], SEEDS["cond"]]), weights_seed=33,
               weights_std=0.1, dims128=np.array([DEN128[k] for k in ("latent_dim", "ff_size", "num_layers", "num_heads")]))
    for tag, den, strategy in [("loop", DEN, "ddim4"), ("loop", DEN, "ddim20"), ("loop128", DEN128, "ddim4"), ("loop128", DEN128, "ddim20")]:
        o32, o64 = run_loop(strategy, den=den), run_loop(strategy, f64=True, den=den)
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        d, ratio = f64_ratio(o32, o64)
        print(f"{tag} {strategy}: reference fp32 vs float64: mean {d.mean():.2e}, p99 {np.percentile(d, 99):.2e}, max {d.max():.2e} -> "
              f"{ratio[0]:.3f} / {ratio[1]:.3f} of the loop bounds")
        if ratio.max() > 0.25:
            raise RuntimeError(f"{strategy}: the reference's own fp32 run is {ratio.max():.2f} of the loop bound away from its float64 run")
        out[f"{tag}:{strategy}:output"] = o32
        out[f"{tag}:{strategy}:ref_f64_ratio"] = ratio
    save("mdm_standalone", **out)


if __name__ == "__main__":
    main()

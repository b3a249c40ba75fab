#!/usr/bin/env python3
"""Generate tests/golden/intergen_standalone.npz: the reference's stand-alone InterGen sampler -- InterDenoiser under ClassifierFreeSampleModel in
MotionDiffusion(mode="interaction") -- called with and without eta > 0, init_image / skip_timesteps and x_start (builder container only; never on the
GPU box).

Run:  python tests/golden/make_golden_intergen.py

make_golden.py's helpers are imported (importing it sets up the stubs and the temp cwd).  Weights: reinit(InterDenoiser(262, **DEN), 32) -- kept as
"w:ig.*" -- under ClassifierFreeSampleModel(net, 3.5); ddim4, B = 2, T = 20 (two 16-key chunks, the second partial).  Inputs are seeds: x_T = rnd(560),
cond = rnd(561) [B, 768], x_start = rnd(562, B, 30, 524), init_image = 0.5 * rnd(563); the noise of the k-th executed step is rnd(570 + k), fed by
patching th.randn_like (the base ddim_sample draws it once per step, [B, T, 524], also at eta = 0 where it is multiplied by zero).

Per case the fixture keeps the reference's fp32 output and the ratio of |fp32 - float64| (the same loop evaluated in float64) to the project's two
loop bounds (mean <= 2e-3, 99th percentile <= 3e-2); a case whose ratio exceeds 0.25 is refused: such a draw would measure the input's conditioning
(pick another seed).  A second file, intergen_standalone32.npz, holds the same cases at latent 32 / ff 64: the fp32_split mode's GEMMs take no smaller
sizes, so that mode is compared there.  The reference's fp32 sigma, the radicand 1 - ab_prev - sigma^2 and its th.sqrt are kept for every step, for eta = 0.5 and 1.0.
"""
import numpy as np

from make_golden import torch, save, sd, reinit, InterDenoiser, ClassifierFreeSampleModel, DEN, gd

B, T, TX = 2, 20, 30
STRATEGY = "ddim4"
WSEED = 32
SEEDS = dict(x_T=560, cond=561, x_start=562, init=563, noise0=570)
BOUNDS = (2e-3, 3e-2)
#         name    eta  pin    init   skip
CASES = [("plain", 0.0, False, False, 0),
         ("pin", 0.0, True, False, 0),
         ("init", 0.0, False, True, 1),
         ("init0", 0.0, False, True, 0),
         ("skip", 0.0, False, False, 1),
         ("eta", 0.5, False, False, 0),
         ("all", 1.0, True, True, 1)]


def draw(seed, *shape):
    """make_golden.rnd whatever the default dtype is (the float64 run changes it; the draw stays the fp32 one)."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def inputs(dtype):
    return dict(x_T=draw(SEEDS["x_T"], B, T, 524).to(dtype), cond=draw(SEEDS["cond"], B, 768).to(dtype),
                x_start=draw(SEEDS["x_start"], B, TX, 524).to(dtype), init=(0.5 * draw(SEEDS["init"], B, T, 524)).to(dtype))


def make_diffusion(mode="interaction", strategy=STRATEGY):
    return gd.MotionDiffusion(use_timesteps=gd.space_timesteps(1000, strategy), motion_rep="global", mode=mode,
                              betas=gd.get_named_beta_schedule("cosine", 1000), model_mean_type=gd.ModelMeanType.START_X,
                              model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE, rescale_timesteps=False)


def run_loop(eta, pin, init, skip, f64=False, den=DEN):
    """The reference's loop in fp32, or the same code in float64 (Tensor.float mapped to .double() for the duration: the schedule gathers then stay
    in float64)."""
    orig_float, orig_randn_like = torch.Tensor.float, torch.randn_like
    calls = [0]

    def randn_like(x, *a, **k):
        z = draw(SEEDS["noise0"] + calls[0], *x.shape).to(x.dtype)
        calls[0] += 1
        return z

    net = reinit(InterDenoiser(262, **den), WSEED)            # (seeded fp32 weights: drawn before the default dtype changes)
    if f64:
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self: self.double()
    torch.randn_like = randn_like
    try:
        diff = make_diffusion()
        if f64:
            net = net.double()
        cfg = ClassifierFreeSampleModel(net, 3.5)
        v = inputs(torch.float64 if f64 else torch.float32)
        out = diff.ddim_sample_loop(cfg, (B, T, 524), noise=v["x_T"].clone(), clip_denoised=False, progress=False,
                                    model_kwargs={"mask": None, "cond": v["cond"]}, eta=eta, skip_timesteps=skip,
                                    init_image=v["init"] if init else None, x_start=v["x_start"] if pin else None)
        assert calls[0] == diff.num_timesteps - skip, (calls[0], diff.num_timesteps, skip)
        return out
    finally:
        torch.Tensor.float, torch.randn_like = orig_float, orig_randn_like
        torch.set_default_dtype(torch.float32)


def eta_tables(eta):
    """sigma and sqrt(1 - ab_prev - sigma^2) as ddim_sample computes them (gaussian_diffusion.py:832-844), for every respaced step."""
    diff = make_diffusion()
    t = torch.arange(diff.num_timesteps)
    ab = gd._extract_into_tensor(diff.alphas_cumprod, t, (diff.num_timesteps,))
    ab_prev = gd._extract_into_tensor(diff.alphas_cumprod_prev, t, (diff.num_timesteps,))
    sigma = eta * torch.sqrt((1 - ab_prev) / (1 - ab)) * torch.sqrt(1 - ab / ab_prev)
    arg = 1 - ab_prev - sigma ** 2
    return sigma, arg, torch.sqrt(arg)


def f64_ratio(o32, o64):
    d = (o32.double() - o64).abs().numpy()
    return d, np.array([d.mean() / BOUNDS[0], np.percentile(d, 99) / BOUNDS[1]])


DEN32 = dict(DEN, latent_dim=32, ff_size=64)      # the smallest sizes the 16-bit GEMMs of the fp32_split mode take (mixer32.npz's)


def main(fixture="intergen_standalone", den=DEN):
    out = dict(B=B, T=T, x_start_frames=TX, strategy=STRATEGY, cfg_scale=3.5, H=den["num_heads"], latent_dim=den["latent_dim"], ff_size=den["ff_size"],
               num_layers=den["num_layers"], seeds=np.array([SEEDS[k] for k in ("x_T", "cond", "x_start", "init", "noise0")]))
    out.update(sd(reinit(InterDenoiser(262, **den), WSEED), "ig."))
    plain = None
    for name, eta, pin, init, skip in CASES:
        o32 = run_loop(eta, pin, init, skip, den=den)
        o64 = run_loop(eta, pin, init, skip, f64=True, den=den)
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        plain = o32 if plain is None else plain
        d, ratio = f64_ratio(o32, o64)
        print(f"{name}: reference fp32 vs float64: mean {d.mean():.2e}, p99 {np.percentile(d, 99):.2e}, max {d.max():.2e} -> "
              f"{ratio[0]:.3f} / {ratio[1]:.3f} of the loop bounds; |out - plain| mean {float((o32 - plain).abs().mean()):.3f}")
        if ratio.max() > 0.25:
            raise RuntimeError(f"case {name}: the reference's own fp32 run is {ratio.max():.2f} of the loop bound away from its float64 run")
        out[f"case:{name}"] = np.array([eta, float(pin), float(init), float(skip)])
        out[f"{name}:output"] = o32
        out[f"{name}:ref_f64_ratio"] = ratio
    for eta in (0.5, 1.0):
        sigma, arg, c3 = eta_tables(eta)
        out[f"eta{eta}:sigma"], out[f"eta{eta}:c3_arg"], out[f"eta{eta}:c3"] = sigma, arg, c3
    save(fixture, **out)


if __name__ == "__main__":
    main()
    main("intergen_standalone32", DEN32)

#!/usr/bin/env python3
"""Generate tests/golden/sampler_opts.npz: the reference's two-chain loop called with eta > 0, init_image / skip_timesteps and x_start
(builder container only; never on the GPU box).

Run:  python tests/golden/make_golden_sampler_opts.py

make_golden.py's helpers are imported (importing it sets up the stubs, the temp cwd and the synthetic normaliser files).  Weights:
build_mixer(4, True, None) -- mixer.npz's "mix." set -- under ClassifierFreeSampleModelX2(3.5); ddim4, B = 2, T = 20 (two 16-key chunks, the second
partial).  Inputs are seeds: x_T = rnd(460), cond = rnd(461), x_start = rnd(462, B, 30, 524), init_image = 0.5 * rnd(463); the noise of the k-th
executed step is rnd(470 + k), fed by patching th.randn_like (the reference draws it once per step, [B, T, 524], for both chains).

Per case the fixture keeps the reference's fp32 output and the ratio of |fp32 - float64| (the same loop evaluated in float64) to the project's two
loop bounds (mean <= 2e-3, 99th percentile <= 3e-2); a case whose ratio exceeds 0.25 is refused: such a draw would measure the input's conditioning.
The reference's fp32 sigma, the radicand 1 - ab_prev - sigma^2 and its th.sqrt are kept for every step, for eta = 0.5 and 1.0.
"""
import numpy as np

from make_golden import torch, save, build_mixer, reset_hist, make_diffusion, ClassifierFreeSampleModelX2, gd

B, T, TX = 2, 20, 30
STRATEGY = "ddim4"
SEEDS = dict(x_T=460, cond=461, x_start=462, init=463, noise0=470)
BOUNDS = (2e-3, 3e-2)
#         name    eta  pin    init   skip
CASES = [("pin", 0.0, True, False, 0),
         ("init", 0.0, False, True, 1),
         ("init0", 0.0, False, True, 0),
         ("skip", 0.0, False, False, 1),
         ("eta", 0.5, False, False, 0),
         ("all", 1.0, True, True, 1)]


def draw(seed, *shape):
    """make_golden.rnd whatever the default dtype is (the float64 run changes it; the draw stays the fp32 one)."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def inputs(dtype):
    return dict(x_T=draw(SEEDS["x_T"], B, T, 524).to(dtype), cond=draw(SEEDS["cond"], B, 8 * 768).to(dtype),
                x_start=draw(SEEDS["x_start"], B, TX, 524).to(dtype), init=(0.5 * draw(SEEDS["init"], B, T, 524)).to(dtype))


def run_loop(eta, pin, init, skip, f64=False):
    """The reference's loop in fp32, or the same code in float64 (Tensor.float mapped to .double() for the duration: the schedule gathers,
    Mixer.forward's casts and the normalisers then stay in float64)."""
    orig_float, orig_randn_like = torch.Tensor.float, torch.randn_like
    calls = [0]

    def randn_like(x, *a, **k):
        z = draw(SEEDS["noise0"] + calls[0], *x.shape).to(x.dtype)
        calls[0] += 1
        return z

    mix = build_mixer(4, True, None)            # (seeded fp32 weights: drawn before the default dtype changes)
    if f64:
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self: self.double()
    torch.randn_like = randn_like
    try:
        diff = make_diffusion(STRATEGY)
        if f64:
            mix = mix.double()
            for owner in (mix, diff):
                for nm in ("normalizer_model1", "normalizer_model2"):
                    n = getattr(owner, nm, None)
                    for a in ("motion_mean", "motion_std"):
                        if n is not None and hasattr(n, a):
                            setattr(n, a, getattr(n, a).double())
        cfg = ClassifierFreeSampleModelX2(mix, 3.5)
        reset_hist(mix)
        v = inputs(torch.float64 if f64 else torch.float32)
        out = diff.ddim_sample_loop(cfg, (B, T, 524), noise=v["x_T"].clone(), clip_denoised=False, progress=False,
                                    model_kwargs={"mask": None, "cond": v["cond"]}, eta=eta, skip_timesteps=skip,
                                    init_image=v["init"] if init else None, x_start=v["x_start"] if pin else None)
        assert calls[0] == diff.num_timesteps - skip, (calls[0], diff.num_timesteps, skip)
        assert len(mix.history_out1) == diff.num_timesteps - skip
        return out
    finally:
        torch.Tensor.float, torch.randn_like = orig_float, orig_randn_like
        torch.set_default_dtype(torch.float32)


def eta_tables(eta):
    """sigma and sqrt(1 - ab_prev - sigma^2) as ddim_sample computes them (gaussian_diffusion.py:1939-1951), for every respaced step."""
    diff = make_diffusion(STRATEGY)
    t = torch.arange(diff.num_timesteps)
    ab = gd._extract_into_tensor(diff.alphas_cumprod, t, (diff.num_timesteps,))
    ab_prev = gd._extract_into_tensor(diff.alphas_cumprod_prev, t, (diff.num_timesteps,))
    sigma = eta * torch.sqrt((1 - ab_prev) / (1 - ab)) * torch.sqrt(1 - ab / ab_prev)
    arg = 1 - ab_prev - sigma ** 2
    return sigma, arg, torch.sqrt(arg)


def main():
    out = dict(B=B, T=T, x_start_frames=TX, strategy=STRATEGY, cfg_scale=3.5, seeds=np.array([SEEDS[k] for k in ("x_T", "cond", "x_start", "init", "noise0")]))
    plain = run_loop(0.0, False, False, 0)
    out["plain:output"] = plain
    for name, eta, pin, init, skip in CASES:
        o32 = run_loop(eta, pin, init, skip)
        o64 = run_loop(eta, pin, init, skip, f64=True)
        assert o32.dtype == torch.float32 and o64.dtype == torch.float64
        d = (o32.double() - o64).abs().numpy()
        ratio = np.array([d.mean() / BOUNDS[0], np.percentile(d, 99) / BOUNDS[1]])
        print(f"{name}: reference fp32 vs float64: mean {d.mean():.2e}, p99 {np.percentile(d, 99):.2e}, max {d.max():.2e} -> "
              f"{ratio[0]:.3f} / {ratio[1]:.3f} of the loop bounds; |out - plain| mean {float((o32 - plain).abs().mean()):.3f}")
        if ratio.max() > 0.25:
            raise RuntimeError(f"case {name}: the reference's own fp32 run is {ratio.max():.2f} of the loop bound away from its float64 run")
        out[f"case:{name}"] = np.array([eta, float(pin), float(init), float(skip)])
        out[f"{name}:output"] = o32
        out[f"{name}:ref_f64_ratio"] = ratio
    for eta in (0.5, 1.0):
        # c3_arg: the radicand, so that a reader can take the square root correctly rounded -- this torch build's CPU fp32 sqrt is not (it is one
        # ulp below numpy's, which equals the float64 root rounded once, in a few table entries; every other operation here is exact IEEE)
        sigma, arg, c3 = eta_tables(eta)
        out[f"eta{eta}:sigma"], out[f"eta{eta}:c3_arg"], out[f"eta{eta}:c3"] = sigma, arg, c3
        ulp = np.abs(c3.numpy().view(np.int32).astype(np.int64) - np.sqrt(arg.numpy()).view(np.int32).astype(np.int64))
        print(f"eta {eta}: th.sqrt vs the correctly rounded root: {int((ulp != 0).sum())} of {len(ulp)} entries differ, by at most {int(ulp.max())} ulp")
    save("sampler_opts", **out)


if __name__ == "__main__":
    main()

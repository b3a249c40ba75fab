#!/usr/bin/env python3
"""Generate tests/golden/inversion_*.npz: the reference's DDIM reverse ODE -- MotionDiffusion.ddim_reverse_sample (GaussianDiffusion's, gaussian_diffusion.py:
908-944) driven `for i in range(k)` with t = [i] * B and clip_denoised=False -- under the five guidance set-ups of the one-chain samplers (builder container
only; never on the GPU box).

Run:  python tests/golden/make_golden_inversion.py

Set-ups (helpers, seeds and weights are the existing scripts': make_golden.py, make_golden_intergen.py, make_golden_in2in_opts.py,
make_golden_mdm_standalone.py):
  intergen     ClassifierFreeSampleModel(InterDenoiser, 3.5)                              cond draw(561) [B, 768]       x [B, 20, 524]   weights reinit(.., 32)
  4way         ClassifierFreeSampleModelMultiple(in2IN "interaction", 3, 3, 1)            cond draw(561) [B, 3 * 768]   x [B, 20, 524]   wseed int = 31
  dual         ClassifierFreeSampleDualMDM(dual_individual, dual_interaction, 2, 3, "exp", 0.004)   cond [B, 5 * 768]   x [B, 20, 524]   wseed ind = 30, int = 31
  individual   ClassifierFreeSampleModel(in2INDenoiser "individual", 3.5)                 cond draw(561) [B, 768]       x [B, 20, 262]   weights reinit(.., 30)
  mdm          ClassifierFreeSampleModel(MDMDenoiser, 2.5)                                cond draw(581 / 582) [B, D]   x [B, 12, 262]   weights reinit(.., 33)
ddim4, B = 2; T = 20 is two 16-key chunks, the second partial.  The motion is 0.5 * draw(563, B, T, W).  Sizes: latent 16 (files inversion_<setup>.npz) and
latent 32 / ff 64 (inversion_<setup>32.npz: the fp32_split mode's smallest); MDM: latent 16 and latent 128 / 2 heads (inversion_mdm128.npz).  No weights are
stored: every parameter is make_golden.reinit's draw from its name and the seed above.

Cases: "full" (k = 4 = S: the ab_next = 0 level) and "partial" (k = 2).  Per case a file keeps the reference's fp32 latent and last pred_xstart, the latent of
the same code run in float64, and for latent and pred_xstart the mean / 99th percentile of |fp32 - float64| together with their ratio to the project's loop
bounds (mean 2e-3, p99 3e-2).  A case whose ratio exceeds 0.25 is refused: such a draw would measure the input's conditioning (pick another seed).

inversion_schedule.npz holds, for ddim4 and ddim50, the reference's fp32 expressions of the reverse update (:936-942): the gathered alphas_cumprod_next and
1 - alphas_cumprod_next (the two radicands, exact fp32 operations) and th.sqrt of both.  As with the eta tables of make_golden_intergen.py, the radicands are
what a test can hold bitwise: the CPU th.sqrt of the builder's torch is not correctly rounded (1 ulp off IEEE sqrt for ~0.6 % of fp32 inputs, two of ddim4's
four entries among them), while numpy's and the GPU's fp32 sqrt are.
"""
import numpy as np

from make_golden import torch, save, reinit, gd, in2INDenoiser, InterDenoiser, ClassifierFreeSampleModel, ClassifierFreeSampleModelMultiple, \
    ClassifierFreeSampleDualMDM, DEN
from make_golden_intergen import B, STRATEGY, SEEDS, DEN32, draw, make_diffusion, f64_ratio, BOUNDS
from make_golden_intergen import WSEED as WSEED_IG
from make_golden_in2in_opts import WSEED, SCALES, DUAL, nets
from make_golden_mdm_standalone import net as mdm_net, DEN128, CFG as CFG_MDM, SEEDS as SEEDS_MDM

T, T_MDM = 20, 12
CASES = [("full", 4), ("partial", 2)]
DUAL_FUNC, DUAL_VALUE = "exp", 0.004
#          set-up        width  frames  diffusion mode
SETUPS = {"intergen": (524, T, "interaction"), "4way": (524, T, "interaction"), "dual": (524, T, "interaction"), "individual": (262, T, "individual"),
          "mdm": (262, T_MDM, "individual")}


def build(setup, den):
    """The guidance wrapper over seeded fp32 weights and the condition of the set-up (fp32 draws)."""
    if setup == "intergen":
        return [reinit(InterDenoiser(262, **den), WSEED_IG)], draw(SEEDS["cond"], B, 768)
    if setup == "4way":
        return nets("4way", den), draw(SEEDS["cond"], B, 3 * 768)
    if setup == "dual":
        return nets("dual", den), draw(SEEDS["cond"], B, 5 * 768)
    if setup == "individual":
        return [reinit(in2INDenoiser(262, mode="individual", **den), WSEED["ind"])], draw(SEEDS["cond"], B, 768)
    return [mdm_net(den)], draw(SEEDS_MDM["cond"] + (den is not DEN), B, den["latent_dim"])


def wrap(setup, ms):
    if setup == "intergen" or setup == "individual":
        return ClassifierFreeSampleModel(ms[0], 3.5)
    if setup == "4way":
        return ClassifierFreeSampleModelMultiple(ms[0], SCALES["s"], SCALES["s_int"], SCALES["s_ind"])
    if setup == "dual":
        return ClassifierFreeSampleDualMDM(ms[0], ms[1], DUAL["s_ind"], DUAL["s_int"], DUAL_FUNC, DUAL_VALUE)
    return ClassifierFreeSampleModel(ms[0], CFG_MDM)


def run_reverse(setup, den, k, f64=False):
    """k reverse steps of the reference in fp32, or the same code in float64 (Tensor.float mapped to .double(): the schedule gathers stay in float64)."""
    W, frames, mode = SETUPS[setup]
    orig_float = torch.Tensor.float
    ms, cond = build(setup, den)                             # (seeded fp32 weights: drawn before the default dtype changes)
    if f64:
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self: self.double()
        ms = [m.double() for m in ms]
    try:
        dt = torch.float64 if f64 else torch.float32
        diff = make_diffusion(mode)
        cfg = wrap(setup, ms)
        x = (0.5 * draw(SEEDS["init"], B, frames, W)).to(dt)
        out = None
        for i in range(k):
            out = diff.ddim_reverse_sample(cfg, x, torch.tensor([i] * B), clip_denoised=False, model_kwargs={"mask": None, "cond": cond.to(dt)})
            x = out["sample"]
        return x, out["pred_xstart"]
    finally:
        torch.Tensor.float = orig_float
        torch.set_default_dtype(torch.float32)


def main(fixture, setup, den):
    W, frames, _ = SETUPS[setup]
    out = dict(B=B, T=frames, W=W, strategy=STRATEGY, H=den["num_heads"], latent_dim=den["latent_dim"], ff_size=den["ff_size"], num_layers=den["num_layers"],
               seeds=np.array([SEEDS["init"], SEEDS_MDM["cond"] + (den is not DEN) if setup == "mdm" else SEEDS["cond"]]), motion_scale=0.5, wstd=0.1,
               bounds=np.array(BOUNDS))
    if setup == "dual":
        out.update(w_func=DUAL_FUNC, w_value=DUAL_VALUE)
    for name, k in CASES:
        (x32, p32), (x64, p64) = run_reverse(setup, den, k), run_reverse(setup, den, k, f64=True)
        assert x32.dtype == torch.float32 and x64.dtype == torch.float64
        out[f"case:{name}"] = k
        out[f"{name}:latent"], out[f"{name}:pred_xstart"], out[f"{name}:latent_f64"] = x32, p32, x64
        for tag, a, b in (("latent", x32, x64), ("pred_xstart", p32, p64)):
            d, ratio = f64_ratio(a, b)
            print(f"{fixture} {name} {tag}: reference fp32 vs float64: mean {d.mean():.2e}, p99 {np.percentile(d, 99):.2e}, max {d.max():.2e} -> "
                  f"{ratio[0]:.3f} / {ratio[1]:.3f} of the loop bounds; rms {float(a.double().pow(2).mean().sqrt()):.1f}, |max| {float(a.abs().max()):.1f}")
            if ratio.max() > 0.25:
                raise RuntimeError(f"{fixture} {name} {tag}: the reference's own fp32 run is {ratio.max():.2f} of the loop bound away from its float64 run")
            out[f"{name}:{tag}:ref_f64_err"] = np.array([d.mean(), np.percentile(d, 99)])
            out[f"{name}:{tag}:ref_f64_ratio"] = ratio
    save(fixture, **out)


def schedule_rows():
    out = {}
    for strat in ("ddim4", "ddim50"):
        diff = make_diffusion("interaction", strat)
        t = torch.arange(diff.num_timesteps)
        ab_next = gd._extract_into_tensor(diff.alphas_cumprod_next, t, (diff.num_timesteps,))
        out[f"{strat}:ab_next"], out[f"{strat}:one_minus_ab_next"] = ab_next, 1 - ab_next
        out[f"{strat}:sqrt_ab_next"], out[f"{strat}:sqrt_one_minus_ab_next"] = torch.sqrt(ab_next), torch.sqrt(1 - ab_next)
        assert ab_next.dtype == torch.float32 and float(out[f"{strat}:sqrt_ab_next"][-1]) == 0.0 and float(out[f"{strat}:sqrt_one_minus_ab_next"][-1]) == 1.0
    save("inversion_schedule", **out)


if __name__ == "__main__":
    schedule_rows()
    for setup in ("intergen", "4way", "dual", "individual"):
        main(f"inversion_{setup}", setup, DEN)
        main(f"inversion_{setup}32", setup, DEN32)
    main("inversion_mdm", "mdm", DEN)
    main("inversion_mdm128", "mdm", DEN128)

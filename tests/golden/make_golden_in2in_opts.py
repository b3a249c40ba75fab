#!/usr/bin/env python3
"""Generate tests/golden/in2in_opts{,32}.npz and in2in_dual_opts{,32}.npz: the reference's stand-alone in2IN samplers called with and without eta > 0,
init_image / skip_timesteps and x_start (builder container only; never on the GPU box).

Run:  python tests/golden/make_golden_in2in_opts.py

Two set-ups, each MotionDiffusion(mode="interaction" / "dual").ddim_sample_loop:
  in2in_opts       ClassifierFreeSampleModelMultiple(in2INDenoiser "interaction", 3, 3, 1)                       cond [B, 3 * 768]
  in2in_dual_opts  ClassifierFreeSampleDualMDM(in2INDenoiser "dual_individual", "dual_interaction", 2, 3, ...)    cond [B, 5 * 768]
                   with the time-varying weight ("exp", 0.004) for every case and the constant one ("const", 0.3) for "plain" and "all"
Shape, cases, input seeds, the patched randn_like and the refusal rule are make_golden_intergen.py's (its helpers are imported): B = 2, T = 20, x_start
of 30 frames, ddim4, the seven cases; per case the reference's fp32 output and the ratio of |fp32 - float64| to the project's loop bound (mean 2e-3,
99th percentile 3e-2) -- a case above 0.25 is refused (pick another seed).  The *32 files hold the same at latent 32 / ff 64, the smallest sizes the
fp32_split mode's GEMMs take.

The files hold no weights: every parameter is make_golden.reinit's draw -- randn(shape, Generator(crc32(name) + seed)) * 0.1 -- and a test re-draws it
from "wseed:*" (checked here against the modules' state dicts), which keeps each file below the size limit for a committed file; the DualMDM set-up is
its own pair of files for the same reason.
"""
import zlib
import numpy as np

from make_golden import torch, save, reinit, in2INDenoiser, ClassifierFreeSampleModelMultiple, ClassifierFreeSampleDualMDM, DEN
from make_golden_intergen import B, T, TX, STRATEGY, SEEDS, CASES, DEN32, draw, make_diffusion, f64_ratio

WSEED = dict(ind=30, int=31)
SCALES = dict(s=3.0, s_int=3.0, s_ind=1.0)                 # configs/models/in2IN.yaml CFG_WEIGHT{,_INTERACTION,_INDIVIDUAL}
DUAL = dict(s_ind=2.0, s_int=3.0)
DUAL_W = {"exp": 0.004, "const": 0.3}
DUAL_CASES = {"exp": [c[0] for c in CASES], "const": ["plain", "all"]}


def redraw(mod, seed, std=0.1):
    """What a test does with "wseed:*": the parameters from their names and shapes alone."""
    return {k: torch.randn(p.shape, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()) + seed)) * std for k, p in mod.named_parameters()}


def nets(setup, den):
    if setup == "4way":
        return [reinit(in2INDenoiser(262, mode="interaction", **den), WSEED["int"])]
    return [reinit(in2INDenoiser(262, mode="dual_individual", **den), WSEED["ind"]), reinit(in2INDenoiser(262, mode="dual_interaction", **den), WSEED["int"])]


def run_loop(setup, func, den, eta, pin, init, skip, f64=False):
    """make_golden_intergen.run_loop over the set-up's guidance wrapper: fp32, or the same code in float64."""
    orig_float, orig_randn_like = torch.Tensor.float, torch.randn_like
    calls = [0]

    def randn_like(x, *a, **k):
        z = draw(SEEDS["noise0"] + calls[0], *x.shape).to(x.dtype)
        calls[0] += 1
        return z

    ms = nets(setup, den)                                    # (seeded fp32 weights: drawn before the default dtype changes)
    if f64:
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self: self.double()
    torch.randn_like = randn_like
    try:
        diff = make_diffusion("interaction" if setup == "4way" else "dual")
        if f64:
            ms = [m.double() for m in ms]
        dt = torch.float64 if f64 else torch.float32
        if setup == "4way":
            cfg = ClassifierFreeSampleModelMultiple(ms[0], SCALES["s"], SCALES["s_int"], SCALES["s_ind"])
        else:
            cfg = ClassifierFreeSampleDualMDM(ms[0], ms[1], DUAL["s_ind"], DUAL["s_int"], func, DUAL_W[func])
        cond = draw(SEEDS["cond"], B, (3 if setup == "4way" else 5) * 768).to(dt)
        x_T, x_start, ini = draw(SEEDS["x_T"], B, T, 524).to(dt), draw(SEEDS["x_start"], B, TX, 524).to(dt), (0.5 * draw(SEEDS["init"], B, T, 524)).to(dt)
        out = diff.ddim_sample_loop(cfg, (B, T, 524), noise=x_T.clone(), clip_denoised=False, progress=False, model_kwargs={"mask": None, "cond": cond},
                                    eta=eta, skip_timesteps=skip, init_image=ini if init else None, x_start=x_start if pin else None)
        assert calls[0] == diff.num_timesteps - skip, (calls[0], diff.num_timesteps, skip)
        return out
    finally:
        torch.Tensor.float, torch.randn_like = orig_float, orig_randn_like
        torch.set_default_dtype(torch.float32)


def main(fixture, setup, den):
    out = dict(B=B, T=T, x_start_frames=TX, strategy=STRATEGY, H=den["num_heads"], latent_dim=den["latent_dim"], ff_size=den["ff_size"],
               num_layers=den["num_layers"], seeds=np.array([SEEDS[k] for k in ("x_T", "cond", "x_start", "init", "noise0")]), wstd=0.1)
    out.update(SCALES if setup == "4way" else DUAL)
    for m, name in zip(nets(setup, den), ("int",) if setup == "4way" else ("ind", "int")):
        out[f"wseed:{name}"] = WSEED[name]
        again = redraw(m, WSEED[name])
        assert all(torch.equal(p, again[k]) for k, p in m.named_parameters())
        assert set(again) == {k for k in m.state_dict() if not k.endswith("sequence_pos_encoder.pe")}
    for func in (("",) if setup == "4way" else DUAL_W):
        pre = f"{func}:" if func else ""
        if func:
            out[f"w:{func}"] = DUAL_W[func]
        plain = None
        for name, eta, pin, init, skip in CASES:
            if func and name not in DUAL_CASES[func]:
                continue
            o32 = run_loop(setup, func, den, eta, pin, init, skip)
            o64 = run_loop(setup, func, den, eta, pin, init, skip, f64=True)
            assert o32.dtype == torch.float32 and o64.dtype == torch.float64
            plain = o32 if plain is None else plain
            d, ratio = f64_ratio(o32, o64)
            print(f"{fixture} {pre}{name}: reference fp32 vs float64: mean {d.mean():.2e}, p99 {np.percentile(d, 99):.2e}, max {d.max():.2e} -> "
                  f"{ratio[0]:.3f} / {ratio[1]:.3f} of the loop bounds; |out - plain| mean {float((o32 - plain).abs().mean()):.3f}")
            if ratio.max() > 0.25:
                raise RuntimeError(f"case {pre}{name}: the reference's own fp32 run is {ratio.max():.2f} of the loop bound away from its float64 run")
            out[f"case:{name}"] = np.array([eta, float(pin), float(init), float(skip)])
            out[f"{pre}{name}:output"] = o32
            out[f"{pre}{name}:ref_f64_ratio"] = ratio
    save(fixture, **out)


if __name__ == "__main__":
    main("in2in_opts", "4way", DEN)
    main("in2in_opts32", "4way", DEN32)
    main("in2in_dual_opts", "dual", DEN)
    main("in2in_dual_opts32", "dual", DEN32)

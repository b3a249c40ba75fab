#!/usr/bin/env python3
"""Generate tests/golden/mask.npz: the reference's modules called WITH a key-padding mask (builder container only; never on the GPU box).

Run:  python tests/golden/make_golden_mask.py

Builds the reference's own modules the way make_golden.py does (its helpers are imported; importing it sets up the stubs, the temp cwd and
the synthetic normaliser files).  Per-parameter seeding (make_golden.reinit) gives the weights of the existing fixtures -- layers.npz
(sa. / ca.), denoisers.npz (ind. / int. / ig.), influence.npz (m1. .. m4.), mixer.npz (mix. / mix_out1.) -- and every input is rnd(seed, *shape) of a seed and
shape recorded under "in:<name>" (the same deterministic CPU generator on every box, as fulldims.npz does), so this fixture stores masks,
seeds and the reference's outputs only.

Masks are float [n, T, 1] as the reference's callers pass them (only mask[..., 0] is used):
  trail  item 0 all valid, item 1 with its last 7 frames invalid
  holes  item 0 with frames 3-5 invalid and the last frame valid (count - 1 differs from the last valid index: pins align_trajectories'
         actual indexing, frame lengths - 1), item 1 with its last 7 frames invalid
T = 20 (two 16-key chunks, the second partial) and T = 33 (crosses two chunk boundaries).
"""
import numpy as np

from make_golden import (torch, reinit, rnd, save, DEN, build_mixer, reset_hist, make_diffusion, in2INDenoiser, InterDenoiser, Influence,
                         VanillaSelfAttention, VanillaCrossAttention, ClassifierFreeSampleModelX2, al)


def mask_of(kind, n, T):
    m = torch.ones(n, T, 1)
    if kind == "holes":
        m[0, 3:6] = 0
    for b in range(1, n):
        m[b, T - 7:] = 0
    return m


def kpm(mask):
    return ~(mask[..., 0] > 0.5)


def forward_f64(mix, x1, x2, cond, mask, t):
    """The reference's Mixer.forward evaluated in float64 on the same weights and inputs (Mixer.forward casts with .float(): mapped to
    .double() for the duration of the call)."""
    mix = mix.double()
    for nm in ("normalizer_model1", "normalizer_model2"):
        n = getattr(mix, nm)
        for a in ("motion_mean", "motion_std"):
            if hasattr(n, a):
                setattr(n, a, getattr(n, a).double())
    orig = torch.Tensor.float
    torch.set_default_dtype(torch.float64)
    torch.Tensor.float = lambda self: self.double()
    try:
        return mix(x1.double(), t, cond=cond.double(), mask=mask.double(), x2=x2.double())
    finally:
        torch.Tensor.float = orig
        torch.set_default_dtype(torch.float32)


OUT = {}


def inp(name, seed, *shape):
    """A seeded N(0, 1) input; the fixture keeps [seed, *shape] only (tests/mask_cases.py re-draws it)."""
    OUT["in:" + name] = np.array([seed, *shape])
    return rnd(seed, *shape)


def main():
    out = OUT
    B = 2
    cases = [("trail", 20), ("holes", 33), ("holes", 20)]
    for kind, T in cases:
        out[f"mask:{kind}:T{T}"] = mask_of(kind, B, T)
    # --- layers (weights: layers.npz sa. / ca.; D = 32, H = 4)
    D, H = 32, 4
    sa = reinit(VanillaSelfAttention(D, H, 0.1), 11)
    ca = reinit(VanillaCrossAttention(D, D, H, 0.1, D), 12)
    for kind, T in cases[:2]:
        tag = f"{kind}:T{T}"
        x, y, e = inp(f"layers:{tag}:x", 401, B, T, D), inp(f"layers:{tag}:y", 402, B, T, D), inp(f"layers:{tag}:emb", 403, B, D)
        m = mask_of(kind, B, T)
        out[f"sa:{tag}"] = sa(x, e, kpm(m))
        out[f"ca:{tag}"] = ca(x, y, e, kpm(m))
    # --- denoisers (weights: denoisers.npz ind. / int. / ig.; one timestep for all rows: the handle's module forward shares it)
    tt = 500
    out["den:t"] = tt
    nets = {"ind": reinit(in2INDenoiser(262, mode="individual", **DEN), 30), "int": reinit(in2INDenoiser(262, mode="interaction", **DEN), 31),
            "ig": reinit(InterDenoiser(262, **DEN), 32)}
    for net, kind, T in [("ind", "holes", 33), ("int", "trail", 20), ("ig", "holes", 20)]:
        tag = f"{net}:{kind}:T{T}"
        x = inp(f"{tag}:x", 410, B, T, 262 if net == "ind" else 524)
        c = inp(f"{tag}:cond", 412, B, 768 if net == "ind" else 3 * 768)
        out[tag] = nets[net](x, torch.full((B,), tt, dtype=torch.long), mask=mask_of(kind, B, T), cond=c)
    # --- Influence, modes 1 and 2 (weights: influence.npz m4. + m{1,2}.out; D = 32, 2 blocks, 4 heads, ff 64)
    for kind, T in cases[:2]:
        tag = f"{kind}:T{T}"
        mi, mI = inp(f"infl:{tag}:m_i", 420, B, T, 32), inp(f"infl:{tag}:m_I", 421, B, T, 32)
        ci, cI = inp(f"infl:{tag}:cond_i", 422, B, 32), inp(f"infl:{tag}:cond_I", 423, B, 32)
        for mode in (1, 2):
            out[f"infl:m{mode}:{tag}"] = reinit(Influence(32, 2, 4, 64, mode), 50)(mi, mI, ci, cI, mask_of(kind, B, T))
    # --- align_motions with a mask (N(0, 1) motions in the 262-d representation, as geometry.npz's "rand" pair)
    for kind, T in [("holes", 20), ("trail", 33)]:
        tag = f"{kind}:T{T}"
        c, d = inp(f"geo:{tag}:target", 430, B, T, 262), inp(f"geo:{tag}:moved", 431, B, T, 262)
        m = mask_of(kind, B, T)
        r1, r2 = al.align_motions(al.ih_to_smpl(c), al.ih_to_smpl(d), m)
        out[f"geo:{tag}:align_m2_ih"] = al.smpl_to_ih(r2)
        out[f"geo:{tag}:last"] = (m.squeeze().sum(dim=1).int() - 1).numpy()
    out["mask:trail:T33"] = mask_of("trail", B, 33)
    # --- Mixer.forward with a mask, align on, mixing modes 2 and 3 (3: the time mean runs over all T frames) (weights: mixer.npz mix. /
    #     mix_out1.); CFG-doubled batch, the mask repeated with it
    B2 = 2 * B
    out["mix:t"] = 640
    for mode, kind, T in [(2, "trail", 20), (3, "holes", 20)]:
        tag = f"m{mode}:{kind}:T{T}"
        m2 = torch.cat([mask_of(kind, B, T)] * 2, 0)
        t = torch.full((B2,), 640, dtype=torch.long)
        # N(0, 1) "denoiser outputs" make some alignments ill-conditioned (a displacement of near-zero length, or the two displacements nearly
        # anti-parallel): the reference's OWN fp32 run then misses its float64 run by more than the step tolerance of the unmasked tests
        # (2e-4 + 2e-4 |ref|), in rows no mask touches.  Such a draw measures the input, not the mask: take the first seed triple at which the
        # reference's fp32 result is within that tolerance of its float64 result in every element.
        for base in range(440, 1440, 100):
            x1, x2, cond = rnd(base, B2, T, 524), rnd(base + 1, B2, T, 524), rnd(base + 2, B2, 8 * 768)
            cond[B:] = 0                                 # (the uncond half: tests zero it the same way)
            mix = build_mixer(mode, True, None)
            reset_hist(mix)
            o32 = mix(x1, t, cond=cond, mask=m2, x2=x2)
            o64 = forward_f64(build_mixer(mode, True, None), x1, x2, cond, m2, t)
            err = (o32.double() - o64).abs()
            worst = float((err / (2e-4 + 2e-4 * o64.abs())).max())
            print(f"mix {tag}: seeds {base}..{base + 2}: reference fp32 vs float64 max err {float(err.max()):.2e}, {worst:.2f} x the step tolerance")
            if worst <= 1.0:
                break
        else:
            raise RuntimeError("no well-conditioned draw found")
        inp(f"mix:{tag}:x1", base, B2, T, 524), inp(f"mix:{tag}:x2", base + 1, B2, T, 524), inp(f"mix:{tag}:cond", base + 2, B2, 8 * 768)
        out[f"mix:{tag}"] = o32
        out[f"mix:{tag}:ref_f64_ratio"] = worst
    # --- the CFG wrapper and a 4-step loop of the two-chain sampler (mode 4, align)
    mix = build_mixer(4, True, None)
    cfg = ClassifierFreeSampleModelX2(mix, 3.5)
    kind, T = "holes", 20
    tag = f"{kind}:T{T}"
    xb, xb2, cb = inp(f"cfg:{tag}:x", 450, B, T, 524), inp(f"cfg:{tag}:x2", 451, B, T, 524), inp(f"cfg:{tag}:cond", 452, B, 8 * 768)
    reset_hist(mix)
    out[f"cfg:{tag}"] = cfg(xb, xb2, torch.full((B,), 640, dtype=torch.long), cond=cb, mask=mask_of(kind, B, T))
    diff = make_diffusion("ddim4")
    out["loop:strategy"] = "ddim4"
    kind, T = "holes", 33
    tag = f"{kind}:T{T}"
    xT, cb = inp(f"loop:{tag}:x_T", 460, B, T, 524), inp(f"loop:{tag}:cond", 461, B, 8 * 768)
    reset_hist(mix)
    out[f"loop:{tag}"] = diff.ddim_sample_loop(cfg, (B, T, 524), noise=xT.clone(), clip_denoised=False, progress=False,
                                               model_kwargs={"mask": mask_of(kind, B, T), "cond": cb})
    save("mask", **out)


if __name__ == "__main__":
    main()

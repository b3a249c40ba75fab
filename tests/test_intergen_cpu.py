"""CPU: the stand-alone InterGen sampler's contract without a GPU -- the single-chain loop with its options (eta > 0, init_image / skip_timesteps,
x_start) restated over the oracle's InterDenoiser and schedule and held to the reference's runs (tests/golden/intergen_standalone{,32}.npz,
tests/golden/make_golden_intergen.py), and the host logic of the InterGen / InterDiffusion / MDM facades: constructor, state_dict names, checkpoint
unwrapping and sample_many's argument rules."""
import os
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("plain", "pin", "init", "init0", "skip", "eta", "all")
BOUNDS = (2e-3, 3e-2)            # the project's loop bound (mean, 99th percentile): the unit of the fixture's ref_f64_ratio


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def fixture_inputs(g):
    """x_T, cond, x_start, init_image, step noises: re-drawn from the fixture's seeds (make_golden_intergen.py: inputs / randn_like)."""
    B, T, S = int(g["B"]), int(g["T"]), 4
    sx, sc, ss, si, sn = [int(v) for v in g["seeds"]]
    return dict(x_T=rnd(sx, B, T, 524), cond=rnd(sc, B, 768), x_start=rnd(ss, B, int(g["x_start_frames"]), 524), init=0.5 * rnd(si, B, T, 524),
                noise=torch.stack([rnd(sn + k, B, T, 524) for k in range(S)]))


def case_kwargs(g, v, name):
    eta, pin, init, skip = [float(x) for x in g[f"case:{name}"]]
    return dict(eta=eta, skip=int(skip), x_start=v["x_start"] if pin else None, init=v["init"] if init else None)


def oracle_loop(W, H, s, sched, x_T, cond, noise, eta=0.0, skip=0, x_start=None, init=None):
    """GaussianDiffusion.ddim_sample_loop over ClassifierFreeSampleModel(InterDenoiser, s) in float64 (gaussian_diffusion.py:799-849, 999-1069;
    cfg_sampler.py:12-28): -> the last pred_xstart."""
    from oracle.denoiser import inter_denoiser
    f = lambda a: torch.as_tensor(a, dtype=torch.float64)
    B, T, _ = x_T.shape
    S = sched.num_timesteps
    img = f(x_T).clone()
    idx = list(range(S - skip))[::-1]
    if skip and init is None:
        init = torch.zeros_like(img)
    if init is not None:
        ab = sched.alphas_cumprod[idx[0]]
        img = np.sqrt(ab) * f(init) + np.sqrt(1.0 - ab) * img
    cond2 = torch.cat([f(cond), torch.zeros_like(f(cond))], 0)
    x0 = None
    for k, i in enumerate(idx):
        if x_start is not None:
            for c in (0, 2, 262, 264):
                img[:, :, c] = f(x_start)[:, :T, c]
        t = torch.full((2 * B,), sched.timestep_map[i], dtype=torch.long)
        out = inter_denoiser(W, "", torch.cat([img, img], 0), t, cond2, H)
        x0 = s * out[:B] + (1.0 - s) * out[B:]
        eps = (sched.sqrt_recip_alphas_cumprod[i] * img - x0) / sched.sqrt_recipm1_alphas_cumprod[i]
        ab, abp = sched.alphas_cumprod[i], sched.alphas_cumprod_prev[i]
        sigma = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
        img = x0 * np.sqrt(abp) + np.sqrt(1 - abp - sigma ** 2) * eps
        if i != 0:
            img = img + sigma * f(noise[k])
    return x0


@pytest.mark.parametrize("fixture", ["intergen_standalone", "intergen_standalone32"])
def test_restated_loop_matches_every_golden_case(golden, fixture):
    """The float64 restatement against the reference's fp32 output: their distance is the reference's own fp32 rounding, which the fixture recorded
    against ITS float64 run (ref_f64_ratio, in units of the loop bound).  Two float64 evaluations of one loop differ by ~1e-13, so mean and p99 must come
    out as recorded: held within 5 % of the recorded figures (percentile interpolation and float64 summation order), i.e. ~1e-6 absolute."""
    from oracle.schedule import make_schedule
    g, w, _ = golden(fixture)
    D = int(g["latent_dim"])
    W = {k: v.double() for k, v in w("ig.", [("sequence_pos_encoder.pe", D)]).items()}
    sched = make_schedule("cosine", 1000, str(g["strategy"]))
    assert sched.num_timesteps == 4
    v = fixture_inputs(g)
    for name in CASES:
        kw = case_kwargs(g, v, name)
        got = oracle_loop(W, int(g["H"]), float(g["cfg_scale"]), sched, v["x_T"], v["cond"], v["noise"], **kw)
        d = (got - torch.from_numpy(g[f"{name}:output"]).double()).abs().numpy()
        want = g[f"{name}:ref_f64_ratio"] * np.array(BOUNDS)
        print(f"{fixture} {name}: |oracle f64 - reference fp32| mean {d.mean():.3e} (recorded {want[0]:.3e}), p99 {np.percentile(d, 99):.3e} (recorded {want[1]:.3e})")
        assert g[f"{name}:ref_f64_ratio"].max() <= 0.25
        assert d.mean() <= 1.05 * want[0] and np.percentile(d, 99) <= 1.05 * want[1], name


def test_eta_tables_are_the_references(golden):
    """sigma and the radicand of the single-chain update are the reference's fp32 tensors bit for bit (the tables of the two-chain sampler: one
    schedule.eta_coefficients serves both)."""
    from mixermdm_amd.schedule import make_schedule
    g, _, _ = golden("intergen_standalone")
    sch = make_schedule("cosine", 1000, str(g["strategy"]))
    for eta in (0.5, 1.0):
        tab = sch.eta_coefficients(eta)
        np.testing.assert_array_equal(tab[1], g[f"eta{eta}:sigma"])
        np.testing.assert_array_equal(tab[0], np.sqrt(g[f"eta{eta}:c3_arg"]))


def tiny_cfg(**over):
    from mixermdm_amd.configs import CfgNode
    c = dict(NAME="InterGen", LATENT_DIM=16, FF_SIZE=32, NUM_LAYERS=2, NUM_HEADS=2, INPUT_DIM=262, CFG_WEIGHT=3.5, STRATEGY="ddim4", DIFFUSION_STEPS=1000,
             BETA_SCHEDULER="cosine")
    c.update(over)
    return CfgNode(c)


def test_config_files_hold_what_the_classes_read():
    from mixermdm_amd.configs import get_config
    from mixermdm_amd.models import InterGen, MDM
    ig = get_config(os.path.join(ROOT, "configs", "models", "InterGen.yaml"))
    md = get_config(os.path.join(ROOT, "configs", "models", "MDM.yaml"))
    m = InterGen(ig)
    assert (m.decoder.latent_dim, m.decoder.ff_size, m.decoder.num_layers, m.decoder.num_heads, m.decoder.cfg_weight) == (1024, 2048, 8, 8, 3.5)
    assert m.decoder.sampling_strategy == "ddim50"
    assert m.state_dict()["decoder.net.blocks.7.ca_block.attention.in_proj_weight"].shape == (3072, 1024)
    d = MDM(md)
    assert (d.latent_dim, d.ff_size, d.num_layers, d.num_heads, d.cfg_weight, d.sampling_strategy, d.num_frames) == (256, 1024, 8, 4, 2.5, "ddim50", 300)
    assert d.state_dict()["model.seqTransEncoder.layers.7.linear1.weight"].shape == (1024, 256)
    assert d.state_dict()["embed_text.weight"].shape == (256, 512)


def test_intergen_state_dict_names_and_checkpoint_forms(golden):
    """The reference's names: decoder.net.* are InterDenoiser.state_dict()'s keys (the fixture's weight set); a Lightning checkpoint with a model. prefix
    is unwrapped; text modules are accepted, anything else is refused by name."""
    from mixermdm_amd.models import InterGen
    g, w, _ = golden("intergen_standalone")
    W = w("ig.")
    m = InterGen(tiny_cfg())
    assert {k[len("decoder.net."):] for k in m.state_dict()} == set(W)
    m.load_state_dict({"state_dict": {"model.decoder.net." + k: v for k, v in W.items()}})
    assert torch.equal(m.state_dict()["decoder.net.out.linear.weight"], W["out.linear.weight"])
    m.load_state_dict({**{"decoder.net." + k: v for k, v in W.items()}, "decoder.net.sequence_pos_encoder.pe": torch.zeros(5000, 16),
                       "clip_ln.weight": torch.ones(4), "positional_embedding": torch.zeros(3, 4)})
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict({**{"decoder.net." + k: v for k, v in W.items()}, "discriminator.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({"decoder.net." + k: v for k, v in W.items() if k != "out.linear.bias"})
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict({"decoder.net." + k: (torch.zeros(3, 3) if k == "out.linear.weight" else v) for k, v in W.items()})
    with pytest.raises(NotImplementedError, match="text encoding"):
        m.text_process({"text": ["a"]})
    with pytest.raises(ValueError, match="Mode not recognized"):
        m.text_process({"text": ["a"]}, mode="dual")
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.forward_test({"cond": torch.zeros(1, 768), "motion_lens": torch.tensor([8])})
    with pytest.raises(NotImplementedError, match="INPUT_DIM"):
        InterGen(tiny_cfg(INPUT_DIM=263))


def test_mdm_state_dict_names(golden):
    from mixermdm_amd.models import MDM
    _, w, _ = golden("mdm")
    W = w("mdm.")
    m = MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=2.5))
    assert {k[len("model."):] for k in m.state_dict() if k.startswith("model.")} == set(W)
    sd = {"model.model." + k: v for k, v in W.items()}
    sd.update({"model.embed_text.weight": torch.ones(16, 512), "model.embed_text.bias": torch.ones(16)})
    m.load_state_dict({"state_dict": sd})
    assert torch.equal(m.state_dict()["model.output_process.poseFinal.weight"], W["output_process.poseFinal.weight"])
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict({**{k[len("model."):]: v for k, v in sd.items()}, "decoder.x": torch.zeros(1)})
    with pytest.raises(NotImplementedError, match="text encoding"):
        m.forward({"text": ["a"], "motion_lens": torch.tensor([8])})


def test_sample_many_argument_rules():
    """Checked before any device is touched (the model is on the CPU: a call that got past validation would raise "MI355X only")."""
    from mixermdm_amd.models import InterGen
    m = InterGen(tiny_cfg())
    b = lambda **kw: dict(cond=torch.zeros(1, 768), motion_lens=torch.tensor([8]), **kw)
    with pytest.raises(ValueError, match="batching 'inflight' not recognized"):
        m.sample_many([b()], batching="inflight")
    with pytest.raises(ValueError, match="eta=-1.0 must be >= 0"):
        m.sample_many([b()], eta=-1)
    with pytest.raises(ValueError, match="batch 1 differs from batch 0 in whether it gives 'x_start'"):
        m.sample_many([b(x_start=torch.zeros(1, 8, 524)), b()])
    with pytest.raises(ValueError, match="batch 0 gives both 'seed' and 'step_noise'"):
        m.sample_many([b(seed=1, step_noise=torch.zeros(4, 1, 8, 524))], eta=1.0)
    with pytest.raises(ValueError, match="one noise form per call"):
        m.sample_many([b(seed=1), b(step_noise=torch.zeros(4, 1, 8, 524))], eta=1.0)
    with pytest.raises(ValueError, match=r"x_T \[1, 8, 524\] expected"):
        m.sample_many([b(x_T=torch.zeros(1, 9, 524))])
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.sample_many([b()], mode="eval_intermediate", inflight=2, keep_history=False)

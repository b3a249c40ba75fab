"""GPU: the stand-alone MDM facade (mixermdm_amd.models.MDM over Sampler(single_only=1, model1_kind=1)) against the reference's loops
(tests/golden/mdm_standalone.npz, tests/golden/make_golden_mdm_standalone.py; the weights are mdm.npz's "mdm." set), its ragged sample_many against the
sequential calls, and the loop options it refuses."""
import numpy as np
import pytest
import torch

from test_intergen_cpu import tiny_cfg

pytestmark = pytest.mark.gpu

LOOP_BOUND = dict(mean=2e-3, p99=3e-2)       # the project's loop bound


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def mdm_model(golden, strategy, precision="fp32", **cfg):
    from mixermdm_amd.models import MDM
    g = golden("mdm_standalone")[0]
    _, w, _ = golden("mdm")
    m = MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=float(g["cfg_scale"]), **cfg), num_frames=64, sampling_strategy=strategy)
    sd = {"model.model." + k: v for k, v in w("mdm.").items()}
    sd.update({"model.embed_text.weight": torch.zeros(16, 512), "model.embed_text.bias": torch.zeros(16)})
    m.load_state_dict({"state_dict": sd})
    m.precision = precision
    return m.to("cuda"), g


@pytest.mark.parametrize("strategy", ["ddim4", "ddim20"])
def test_forward_test_vs_reference_golden_fp32(golden, strategy):
    m, g = mdm_model(golden, strategy)
    B, T = int(g["B"]), int(g["T"])
    sx, sc = [int(v) for v in g["seeds"]]
    out = m.forward_test({"cond": rnd(sc, B, 16), "x_T": rnd(sx, B, T, 262), "motion_lens": torch.tensor([T] * B)})["output"]
    assert out.shape == (B, T, 262)
    d = np.abs(out.cpu().numpy() - g[f"loop:{strategy}:output"])
    print("MDM %s fp32: mean err %.3e, p99 %.3e, max %.3e" % (strategy, d.mean(), np.percentile(d, 99), d.max()))
    assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (d.mean(), np.percentile(d, 99), d.max())


def test_fp32_split_needs_head_size_64_or_128_at_the_fixture_sizes(golden):
    """The fixture's denoiser (latent 16, 2 heads: head size 8) is below what the fp32_split mode of MDM covers (head sizes 64 / 128): the handle refuses
    it by name, and the facade hands the refusal on.  The mode is held to the reference below, at the smallest sizes it covers."""
    from mixermdm_amd._lib import MMDMError
    m, g = mdm_model(golden, "ddim4", precision="fp32_split")
    B, T = int(g["B"]), int(g["T"])
    with pytest.raises(MMDMError, match="multiples of 32|head size"):
        m.forward_test({"cond": rnd(1, B, 16), "x_T": rnd(2, B, T, 262), "motion_lens": torch.tensor([T] * B)})


def mdm_model128(golden, strategy, prec):
    """The fixture's second model: latent 128 / 2 heads (head size 64: the smallest MDM that the fp32_split mode and ragged batches cover).  The fixture
    keeps the outputs only; the weights are make_golden.reinit's -- every parameter N(0, 0.1) from Generator(crc32(name) + seed) -- redrawn here."""
    import zlib
    from mixermdm_amd.models import MDM
    from mixermdm_amd.synthetic import mdm_denoiser_shapes
    g = golden("mdm_standalone")[0]
    D, F, L, H = [int(v) for v in g["dims128"]]
    seed, std = int(g["weights_seed"]), float(g["weights_std"])
    sd = {"model." + k: torch.randn(shp, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()) + seed)) * std
          for k, shp in mdm_denoiser_shapes("", D, F, L).items()}
    sd.update({"embed_text.weight": torch.zeros(D, 512), "embed_text.bias": torch.zeros(D)})
    m = MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=float(g["cfg_scale"]), LATENT_DIM=D, FF_SIZE=F, NUM_LAYERS=L, NUM_HEADS=H), num_frames=64, sampling_strategy=strategy)
    m.load_state_dict(sd)
    m.precision = prec
    return m, g, D


@pytest.mark.parametrize("prec", ["fp32", "fp32_split"])
@pytest.mark.parametrize("strategy", ["ddim4", "ddim20"])
def test_forward_test_vs_reference_golden_at_head_size_64(golden, strategy, prec):
    """The reference's loops at latent 128 / 2 heads, in fp32 and fp32_split."""
    m, g, D = mdm_model128(golden, strategy, prec)
    B, T = int(g["B"]), int(g["T"])
    sx, sc = [int(v) for v in g["seeds"]]
    out = m.to("cuda").forward_test({"cond": rnd(sc + 1, B, D), "x_T": rnd(sx, B, T, 262), "motion_lens": torch.tensor([T] * B)})["output"]
    m._sampler.close()
    d = np.abs(out.cpu().numpy() - g[f"loop128:{strategy}:output"])
    print("MDM(128) %s %s: mean err %.3e, p99 %.3e, max %.3e" % (strategy, prec, d.mean(), np.percentile(d, 99), d.max()))
    assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (d.mean(), np.percentile(d, 99), d.max())


@pytest.mark.parametrize("prec", ["fp32", "fp32_split"])
def test_sample_many_ragged_equals_sequential_bitwise(golden, prec):
    m, g, D = mdm_model128(golden, "ddim4", prec)
    m = m.to("cuda")
    batches = [dict(cond=rnd(50 + i, nb, D), motion_lens=torch.tensor([T] * nb), x_T=rnd(60 + i, nb, T, 262)) for i, (nb, T) in enumerate([(2, 12), (1, 33), (3, 20), (1, 64)])]
    seq = m.sample_many(batches, batching="sequential")
    rag = m.sample_many(batches, batching="ragged")
    small = m.sample_many(batches, batching="ragged", max_rows=64, max_items=2)
    for a, b, c, bt in zip(seq, rag, small, batches):
        assert a["output"].shape == bt["x_T"].shape
        assert torch.equal(a["output"], b["output"]) and torch.equal(a["output"], c["output"])
        assert torch.equal(a["output"], m.forward_test(dict(bt))["output"])


def test_loop_options_are_refused_with_the_librarys_message(golden):
    m, g = mdm_model(golden, "ddim4")
    B, T = 2, 12
    batch = {"cond": rnd(1, B, 16), "x_T": rnd(2, B, T, 262), "motion_lens": torch.tensor([T] * B)}
    with pytest.raises(NotImplementedError, match="eta > 0 covers the two-chain MixerMDM sampler"):
        m.forward(dict(batch), eta=0.5, seed=1)
    with pytest.raises(NotImplementedError, match="step noise, x_start, init_image and skip_timesteps cover the two-chain MixerMDM sampler"):
        m.forward(dict(batch), skip_timesteps=1)
    with pytest.raises(NotImplementedError, match="cover the two-chain MixerMDM sampler"):
        m.forward(dict(batch), x_start=rnd(3, B, T, 524))
    with pytest.raises(NotImplementedError, match="cover"):
        m.sample_many([dict(batch)], eta=1.0)
    with pytest.raises(NotImplementedError, match="cover"):
        m.sample_many([dict(batch, init_image=rnd(4, B, T, 524))])
    out = m.forward_test(dict(batch))["output"]                       # and the plain call still runs
    assert out.shape == (B, T, 262) and bool(torch.isfinite(out).all())

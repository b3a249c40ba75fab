"""CPU: the fixtures of the in2IN samplers with the loop's options (tests/golden/in2in_opts{,32}.npz, in2in_dual_opts{,32}.npz;
tests/golden/make_golden_in2in_opts.py) -- recorded ratios, cases, inputs and weights re-drawn from their seeds -- and the host logic of
in2INDiffusion / in2IN.sample_many over a fake sampler: which handle a call builds, grouping, the argument rules and their texts."""
import types
import zlib
import numpy as np
import pytest
import torch

from test_intergen_cpu import CASES

FIXTURES = ("in2in_opts", "in2in_opts32", "in2in_dual_opts", "in2in_dual_opts32")
DUAL_CASES = {"exp": CASES, "const": ("plain", "all")}


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def fixture_sets(g):
    """[(key prefix, dual weight function or None, its cases)] of a fixture."""
    if "w:exp" not in g:
        return [("", None, CASES)]
    return [(f"{f}:", f, DUAL_CASES[f]) for f in ("exp", "const")]


def fixture_inputs(g):
    """x_T, cond (3 or 5 text slices), x_start, init_image, step noises: re-drawn from the fixture's seeds."""
    B, T, S = int(g["B"]), int(g["T"]), 4
    sx, sc, ss, si, sn = [int(v) for v in g["seeds"]]
    k = 5 if "w:exp" in g else 3
    return dict(x_T=rnd(sx, B, T, 524), cond=rnd(sc, B, k * 768), x_start=rnd(ss, B, int(g["x_start_frames"]), 524), init=0.5 * rnd(si, B, T, 524),
                noise=torch.stack([rnd(sn + k, B, T, 524) for k in range(S)]))


def fixture_weights(g, net, prefix):
    """The denoiser `net` ("ind" / "int") of a fixture under `prefix`: every parameter is randn(shape, Generator(crc32(name) + seed)) * std."""
    from mixermdm_amd.synthetic import denoiser_shapes
    seed, std = int(g[f"wseed:{net}"]), float(g["wstd"])
    shapes = denoiser_shapes("", int(g["latent_dim"]), int(g["ff_size"]), int(g["num_layers"]))
    return {prefix + k: torch.randn(shp, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()) + seed)) * std for k, shp in shapes.items()}


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fixture_ratios_cases_and_redraws(golden, fixture):
    g, _, _ = golden(fixture)
    v = fixture_inputs(g)
    B, T = int(g["B"]), int(g["T"])
    assert (B, T, int(g["x_start_frames"]), str(g["strategy"])) == (2, 20, 30, "ddim4") and v["cond"].shape[1] in (3 * 768, 5 * 768)
    want = dict(plain=(0, 0, 0, 0), pin=(0, 1, 0, 0), init=(0, 0, 1, 1), init0=(0, 0, 1, 0), skip=(0, 0, 0, 1), eta=(0.5, 0, 0, 0), all=(1, 1, 1, 1))
    for name in CASES:
        assert tuple(float(x) for x in g[f"case:{name}"]) == tuple(float(x) for x in want[name])
    for pre, func, cases in fixture_sets(g):
        for name in cases:
            out, ratio = g[f"{pre}{name}:output"], g[f"{pre}{name}:ref_f64_ratio"]
            assert out.shape == (B, T, 524) and out.dtype == np.float32 and ratio.shape == (2,) and ratio.max() <= 0.25, (pre, name, ratio)
            if name != "plain":      # the case is not the plain loop
                assert np.abs(out - g[f"{pre}plain:output"]).mean() > 0.03, (pre, name)
    # the weights are the names and shapes of the facade's parameters
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import in2INDiffusion
    dual = "w:exp" in g
    cfg = CfgNode(dict(NAME="in2IN", LATENT_DIM=int(g["latent_dim"]), FF_SIZE=int(g["ff_size"]), NUM_LAYERS=int(g["num_layers"]), NUM_HEADS=int(g["H"]),
                       INPUT_DIM=262, DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine", W_FUNC="exp", W_VALUE=0.004))
    m = in2INDiffusion(cfg, "dual" if dual else "interaction", sampling_strategy="ddim4")
    W = fixture_weights(g, "int", "net_interaction.")
    if dual:
        W.update(fixture_weights(g, "ind", "net_individual."))
    m.load_state_dict(W)                          # strict: names and shapes
    assert abs(float(W["net_interaction.out.linear.weight"].std()) - 0.1) < 0.01


# ---------------------------------------------------------------------------------------------------
# host logic over a fake sampler
# ---------------------------------------------------------------------------------------------------
class FakeSampler:
    made = []

    def __init__(self, **kw):
        self.kw = kw
        self.cfg = types.SimpleNamespace(max_batch=kw["max_batch"], max_frames=kw["max_frames"])
        self.device = kw["device"]
        self.schedule = types.SimpleNamespace(num_timesteps=4)
        self.stream = object()
        self.calls, self.etas, self.closed = [], [], False
        FakeSampler.made.append(self)

    def close(self):
        self.closed = True

    def load_state_dict(self, sd):
        self.loaded = sorted(sd)

    def prepare(self):
        pass

    def set_schedule(self, *a):
        self.sched = a

    def set_dual_weights(self, func, value):
        self.dual = (func, value)

    def set_eta(self, eta):
        self.etas.append(float(eta))

    def sample_ragged_async(self, cond, x_T, lens, **kw):
        self.calls.append(dict(cond=cond, lens=list(lens), kw=kw))
        return [torch.full((t, 524), float(len(self.calls))) for t in lens], None, types.SimpleNamespace(synchronize=lambda: None)


@pytest.fixture
def fake(monkeypatch):
    from mixermdm_amd import models
    FakeSampler.made = []
    monkeypatch.setattr(models, "Sampler", FakeSampler)
    monkeypatch.setattr(models.in2INDiffusion, "device", property(lambda self: torch.device("cuda:0")))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(wait_stream=lambda s: None))
    return FakeSampler


def tiny(mode, **over):
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import in2IN
    c = dict(NAME="in2IN", LATENT_DIM=16, FF_SIZE=32, NUM_LAYERS=2, NUM_HEADS=2, INPUT_DIM=262, CFG_WEIGHT=3.0, CFG_WEIGHT_INTERACTION=3.0,
             CFG_WEIGHT_INDIVIDUAL=1.0, STRATEGY="ddim4", DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine", W_FUNC="exp", W_VALUE=0.004)
    c.update(over)
    return in2IN(CfgNode(c), mode)


def ibatch(nb, T, **kw):
    z = lambda: torch.zeros(nb, 768)
    return {**dict(cond_interaction=z(), cond_interaction_individual1=z(), cond_interaction_individual2=z(), cond_individual_individual1=z(),
                   cond_individual_individual2=z(), motion_lens=torch.tensor([T] * nb), x_T=torch.zeros(nb, T, 524)), **kw}


def test_cfg_form_reaches_the_config_and_the_handle_policy(fake):
    from mixermdm_amd._lib import Config
    assert Config._fields_[-1] == ("cfg_form", __import__("ctypes").c_int)
    c = Config()
    c.cfg_form = 2
    assert c.cfg_form == 2 and c.single_only == 0
    for mode, new, legacy in (("interaction", dict(single_only=4, cfg_form=1), dict(single_only=2)), ("dual", dict(single_only=4, cfg_form=2), dict(single_only=3))):
        d = tiny(mode).decoder
        d.precision = "fp32_split"
        s = d._get_sampler(2, 20)
        assert {k: s.kw.get(k) for k in ("single_only", "cfg_form")} == {"cfg_form": new["cfg_form"], "single_only": 4}
        assert s.kw["precision"] == "fp32_split" and s.kw["max_frames"] == 300 and s.sched[0] == "ddim4"
        assert (mode == "dual") == hasattr(s, "dual") and (mode != "dual" or s.dual == ("exp", 0.004))
        assert d._get_sampler(1, 10) is s                               # fits: the same handle
        s2 = d._get_sampler(2, 20, legacy=True)                         # an explicit mask: the single_only 2 / 3 handle, one handle at a time
        assert s.closed and s2.kw["single_only"] == legacy["single_only"] and "cfg_form" not in s2.kw
        s3 = d._get_sampler(3, 20)
        assert s2.closed and s3.kw["single_only"] == 4 and s3.kw["max_batch"] == 3
    s = tiny("individual").decoder._get_sampler(1, 8)
    assert s.kw["single_only"] == 1 and "cfg_form" not in s.kw


def test_sample_many_groups_and_argument_rules(fake):
    m = tiny("interaction")
    batches = [ibatch(2, 12), ibatch(1, 33), ibatch(3, 20)]
    out = m.sample_many(batches, mode="eval_intermediate", batching="ragged", inflight=2, keep_history=False, max_rows=60, max_items=64)
    s = fake.made[-1]
    assert [c["lens"] for c in s.calls] == [[12, 12, 33], [20, 20, 20]] and all(c["kw"] == {} for c in s.calls)      # <= 60 rows a group
    assert [tuple(o["output"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)] and s.calls[0]["cond"].shape == (3, 3 * 768)
    assert float(out[1]["output"][0, 0, 0]) == 1.0 and float(out[2]["output"][0, 0, 0]) == 2.0
    s.calls.clear()
    m.sample_many(batches, max_items=2)
    assert [c["lens"] for c in s.calls] == [[12, 12], [33, 20], [20, 20]]
    # options: seeds and the generator's rows per motion, per-item x_start; eta belongs to the call
    s.calls.clear()
    bo = [ibatch(2, 12, seed=5, x_start=torch.zeros(2, 14, 524)), ibatch(1, 33, seed=6, x_start=torch.zeros(1, 33, 524))]
    m.sample_many(bo, eta=1.0, skip_timesteps=1)
    kw = s.calls[0]["kw"]
    assert kw["seeds"] == [5, 5, 6] and kw["noise_rows"] == [0, 1, 0] and kw["skip_timesteps"] == 1 and len(kw["x_start"]) == 3 and s.etas == [1.0, 0.0]
    dual = tiny("dual")
    dual.sample_many([ibatch(1, 8)])
    assert fake.made[-1].calls[0]["cond"].shape == (1, 5 * 768)
    b = lambda **k: ibatch(1, 8, **k)
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
    with pytest.raises(ValueError, match=r"step_noise \[>= 3, 1, 8, 524\] expected"):
        m.sample_many([b(step_noise=torch.zeros(2, 1, 8, 524))], eta=1.0, skip_timesteps=1)
    with pytest.raises(ValueError, match=r"skip_timesteps=4 outside \[0, 4\)"):
        m.sample_many([b()], skip_timesteps=4)
    with pytest.raises(ValueError, match=r"x_T \[1, 8, 524\] expected"):
        m.sample_many([b(x_T=torch.zeros(1, 9, 524))])


def test_without_a_device_the_call_is_refused_by_name():
    with pytest.raises(RuntimeError, match="MI355X only"):
        tiny("interaction").sample_many([ibatch(1, 8)])

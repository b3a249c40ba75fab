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


# ---------------------------------------------------------------------------------------------------
# the other many-call drivers over the same kind of fake: InterDiffusion, MDM, the inversions, MixerMDM
# ---------------------------------------------------------------------------------------------------
class FakeOneChain(FakeSampler):
    """FakeSampler plus the uniform calls the one-chain facades make: sample (the refusable call) and the inversions."""

    fail_at = None

    def sample_ragged_async(self, cond, x_T, lens, **kw):
        if self.fail_at == len(self.calls):
            raise RuntimeError("boom")
        return super().sample_ragged_async(cond, x_T, lens, **kw)

    def sample(self, cond, x_T, **kw):
        self.calls.append(dict(sample=kw))
        return torch.zeros_like(x_T)

    def invert(self, cond, x_0, k):
        self.calls.append(dict(invert=k, cond=cond))
        return torch.full_like(x_0, float(len(self.calls)))

    def invert_ragged(self, cond, x_0, lens, k):
        self.calls.append(dict(invert=k, cond=cond, lens=list(lens), x_0=x_0))
        return [torch.full((t, x.shape[-1]), float(len(self.calls))) for t, x in zip(lens, x_0)]


@pytest.fixture
def fake1(monkeypatch, fake):
    from mixermdm_amd import models
    monkeypatch.setattr(models, "Sampler", FakeOneChain)
    monkeypatch.setattr(models._StandaloneDiffusion, "device", property(lambda self: torch.device("cuda:0")))
    return FakeOneChain


def gbatch(nb, T, W=524, cw=768, **kw):
    return {**dict(cond=torch.zeros(nb, cw), motion_lens=torch.tensor([T] * nb), x_T=torch.zeros(nb, T, W)), **kw}


THREE = ((2, 12), (1, 33), (3, 20))


def drawn(seed, n):
    """The n un-named seeds a many-call draws after torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    return [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(n)]


def test_interdiffusion_sample_many_transcript(fake1):
    from test_intergen_cpu import tiny_cfg
    from mixermdm_amd.models import InterGen
    m = InterGen(tiny_cfg())
    batches = [gbatch(b, T) for b, T in THREE]
    out = m.sample_many(batches, mode="eval_intermediate", inflight=2, keep_history=False, max_rows=60)
    s = fake1.made[-1]
    assert (s.kw["single_only"], s.kw["model2_kind"], s.kw["max_batch"], s.kw["max_frames"], s.sched[0]) == (4, 1, 3, 300, "ddim4")
    assert [c["lens"] for c in s.calls] == [[12, 12, 33], [20, 20, 20]] and all(c["kw"] == {} for c in s.calls) and s.etas == []
    assert [tuple(o["output"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)] and all(set(o) == {"output"} for o in out)
    assert [float(o["output"][0, 0, 0]) for o in out] == [1.0, 1.0, 2.0]
    s.calls.clear()
    m.sample_many(batches, max_items=2)
    assert [c["lens"] for c in s.calls] == [[12, 12], [33, 20], [20, 20]] and fake1.made[-1] is s
    s.calls.clear()
    m.sample_many([gbatch(1, 70), gbatch(2, 10)], max_rows=60)                # a motion longer than max_rows: a group of its own
    assert [c["lens"] for c in s.calls] == [[70], [10, 10]] and fake1.made[-1] is s
    # eta > 0: named seeds, and un-named ones drawn in batch order from torch's default generator
    s.calls.clear()
    d = drawn(11, 2)
    torch.manual_seed(11)
    m.sample_many([gbatch(2, 12), gbatch(1, 33, seed=6), gbatch(3, 20)], eta=1.0, skip_timesteps=1, max_rows=60)
    assert [c["kw"] for c in s.calls] == [dict(skip_timesteps=1, seeds=[d[0], d[0], 6], noise_rows=[0, 1, 0]), dict(skip_timesteps=1, seeds=[d[1]] * 3, noise_rows=[0, 1, 2])]
    assert s.etas == [1.0, 0.0]
    # the step_noise form: every motion its slice of the batch's buffer, cut to the executed steps
    s.calls.clear()
    sn = [torch.arange(4 * b * T * 524, dtype=torch.float32).reshape(4, b, T, 524) for b, T in THREE]
    m.sample_many([gbatch(b, T, step_noise=n) for (b, T), n in zip(THREE, sn)], eta=0.5, skip_timesteps=1, max_rows=60)
    kw = s.calls[0]["kw"]
    assert sorted(kw) == ["noise", "skip_timesteps"] and [tuple(t.shape) for t in kw["noise"]] == [(3, 12, 524), (3, 12, 524), (3, 33, 524)]
    assert torch.equal(kw["noise"][1], sn[0][:3, 1]) and torch.equal(s.calls[1]["kw"]["noise"][2], sn[2][:3, 2]) and s.etas[-2:] == [0.5, 0.0]
    # x_start / init_image for every batch, eta = 0: no eta is set, no noise is named
    s.calls.clear()
    s.etas.clear()
    m.sample_many([gbatch(b, T, x_start=torch.zeros(b, T + 2, 524), init_image=torch.full((b, T, 524), float(i))) for i, (b, T) in enumerate(THREE)], max_rows=60)
    kw = s.calls[0]["kw"]
    assert sorted(kw) == ["init_image", "skip_timesteps", "x_start"] and kw["skip_timesteps"] == 0 and s.etas == []
    assert [t.shape[0] for t in kw["x_start"]] == [14, 14, 35] and [float(t[0, 0]) for t in kw["init_image"]] == [0.0, 0.0, 1.0]
    # eta is the call's, also when the second group fails
    s.calls.clear()
    s.fail_at = 1
    with pytest.raises(RuntimeError, match="boom"):
        m.sample_many(batches, eta=1.0, max_rows=60)
    assert s.etas == [1.0, 0.0] and len(s.calls) == 1
    s.fail_at = None
    b = lambda **k: gbatch(1, 8, **k)
    for text, bs, kw in (("InterDiffusion.sample_many: batching 'inflight' not recognized \\(\"ragged\" or \"sequential\"\\)", [b()], dict(batching="inflight")),
                         ("eta=-1.0 must be >= 0", [b()], dict(eta=-1)),
                         ("InterDiffusion.sample_many: batch 1 differs from batch 0 in whether it gives 'init_image': give it for every batch or for none",
                          [b(init_image=torch.zeros(1, 8, 524)), b()], {}),
                         ("InterDiffusion.sample_many: batch 0 gives both 'seed' and 'step_noise'", [b(seed=1, step_noise=torch.zeros(4, 1, 8, 524))], dict(eta=1.0)),
                         ("InterDiffusion.sample_many: batch 1 names its step noise as a 'noise', batch 0 as a 'seed': one noise form per call",
                          [b(seed=1), b(step_noise=torch.zeros(4, 1, 8, 524))], dict(eta=1.0)),
                         (r"InterDiffusion.sample_many: batch 0: step_noise \[>= 3, 1, 8, 524\] expected, got \(2, 1, 8, 524\)",
                          [b(step_noise=torch.zeros(2, 1, 8, 524))], dict(eta=1.0, skip_timesteps=1)),
                         (r"InterDiffusion.sample_many: batch 1: x_start \[1, T, 524\] expected, got \(2, 8, 524\)",
                          [b(x_start=torch.zeros(1, 8, 524)), b(x_start=torch.zeros(2, 8, 524))], {}),
                         (r"InterDiffusion.sample_many: batch 0: init_image \[1, T, 524\] expected, got \(8, 524\)", [b(init_image=torch.zeros(8, 524))], {}),
                         (r"skip_timesteps=4 outside \[0, 4\)", [b()], dict(skip_timesteps=4)),
                         (r"InterDiffusion: x_T \[1, 8, 524\] expected, got \(1, 9, 524\)", [b(x_T=torch.zeros(1, 9, 524))], {})):
        with pytest.raises(ValueError, match=text):
            m.sample_many(bs, **kw)


def test_mdm_sample_many_without_options_transcript(fake1):
    from test_intergen_cpu import tiny_cfg
    from mixermdm_amd.models import MDM
    m = MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=2.5))
    seen = []
    m.text_encoder = lambda batch: seen.append(torch.is_grad_enabled()) or torch.full((len(batch["text"]), 16), 2.0)
    batches = [dict(text=["a"] * b, motion_lens=torch.tensor([T] * b), x_T=torch.zeros(b, T, 262)) for b, T in THREE]
    out = m.sample_many(batches, mode="eval", inflight=4, keep_history=None, max_rows=60)
    s = fake1.made[-1]
    assert (s.kw["single_only"], s.kw["model1_kind"], s.kw["max_batch"]) == (1, 1, 3) and seen == [False] * 3 and all("cond" not in b for b in batches)
    assert [c["lens"] for c in s.calls] == [[12, 12, 33], [20, 20, 20]] and all(c["kw"] == {} for c in s.calls) and float(s.calls[0]["cond"][2, 0]) == 2.0
    assert [tuple(o["output"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)]        # (the fake's rows are 524 wide)
    # the loop's options: the library decides (its call is made, on batch 0), then the facade refuses by name
    s.calls.clear()
    with pytest.raises(NotImplementedError, match="MDM.sample_many: the loop options are not covered by this sampler"):
        m.sample_many([gbatch(1, 8, W=262, cw=16, seed=3, x_start=torch.zeros(1, 8, 262))], eta=1.0, skip_timesteps=2)
    kw = s.calls[0]["sample"]
    assert len(s.calls) == 1 and (kw["eta"], kw["skip_timesteps"], kw["seed"], kw["init_image"]) == (1.0, 2, 3, None) and kw["x_start"].shape == (1, 8, 262)
    with pytest.raises(ValueError, match="MDM.sample_many: batch 0 gives both 'seed' and 'step_noise'"):
        m.sample_many([gbatch(1, 8, W=262, cw=16, seed=1, step_noise=torch.zeros(4, 1, 8, 262))], eta=1.0)
    with pytest.raises(ValueError, match=r"MDM: x_T \[1, 8, 262\] expected"):
        m.sample_many([gbatch(1, 8, W=524, cw=16)])


def test_invert_many_transcript(fake1):
    from test_intergen_cpu import tiny_cfg
    from mixermdm_amd.models import InterGen, MDM
    ig = InterGen(tiny_cfg())
    batches = [dict(cond=torch.full((b, 768), float(i)), motions=torch.zeros(b, T, 524)) for i, (b, T) in enumerate(THREE)]
    out = ig.invert_many(batches, steps=3, max_rows=60)
    s = fake1.made[-1]
    assert [(c["lens"], c["invert"]) for c in s.calls] == [([12, 12, 33], 3), ([20, 20, 20], 3)] and s.kw["max_batch"] == 3 and s.kw["max_frames"] == 300
    assert [float(v) for v in s.calls[0]["cond"][:, 0]] == [0.0, 0.0, 1.0] and [tuple(x.shape) for x in s.calls[0]["x_0"]] == [(12, 524), (12, 524), (33, 524)]
    assert [(tuple(o["latent"].shape), o["steps"], float(o["latent"][0, 0, 0])) for o in out] == [((2, 12, 524), 3, 1.0), ((1, 33, 524), 3, 1.0), ((3, 20, 524), 3, 2.0)]
    s.calls.clear()
    out = ig.invert_many(batches, max_items=2, batching="ragged")
    assert [(c["lens"], c["invert"]) for c in s.calls] == [([12, 12], 4), ([33, 20], 4), ([20, 20], 4)] and out[0]["steps"] == 4
    s.calls.clear()
    out = ig.invert_many(batches, batching="sequential", steps=1)
    assert [c["invert"] for c in s.calls] == [1, 1, 1] and all("lens" not in c for c in s.calls) and [tuple(o["latent"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)]
    with pytest.raises(ValueError, match=r"invert: steps=9 outside \[1, 4\]"):
        ig.invert_many(batches, steps=9)
    with pytest.raises(ValueError, match="InterDiffusion.invert_many: batching 'inflight' not recognized \\(\"ragged\" or \"sequential\"\\)"):
        ig.invert_many(batches, batching="inflight")
    # the text stage of the facades runs first, on a copy of every batch, without autograd
    md = MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=2.5))
    seen = []
    md.text_encoder = lambda batch: seen.append(torch.is_grad_enabled()) or torch.full((len(batch["text"]), 16), 2.0)
    mb = [dict(text=["a"] * b, motions=torch.zeros(b, T, 262)) for b, T in THREE]
    out = md.invert_many(mb, max_rows=60)
    s = fake1.made[-1]
    assert [c["lens"] for c in s.calls] == [[12, 12, 33], [20, 20, 20]] and float(s.calls[1]["cond"][0, 0]) == 2.0 and seen == [False] * 3 and all("cond" not in b for b in mb)
    assert [tuple(o["latent"].shape) for o in out] == [(2, 12, 262), (1, 33, 262), (3, 20, 262)]
    assert md.invert(mb[1], steps=2)["steps"] == 2 and s.calls[-1]["invert"] == 2 and seen == [False] * 4
    m = tiny("interaction")
    m.text_encoder = lambda batch, mode, text_name, out_name: seen.append((mode, text_name, out_name, torch.is_grad_enabled())) or {**batch, out_name: torch.zeros(1, 768)}
    del seen[:]
    raw = dict(motions=torch.zeros(1, 8, 524))
    assert m.invert_many([raw])[0]["latent"].shape == (1, 8, 524) and list(raw) == ["motions"]
    assert seen == [("interaction", "text", "cond_interaction", False), ("interaction", "text_individual1", "cond_interaction_individual1", False),
                    ("interaction", "text_individual2", "cond_interaction_individual2", False)]
    assert m.invert(raw, steps=1)["steps"] == 1 and len(seen) == 6 and list(raw) == ["motions"]


class Dev(str):
    """A device name torch takes for the CPU and the facade takes for a GPU."""
    type = "cuda"


def _fake_mixer_sampler():
    from mixermdm_amd.sampler import Sampler

    class FakeMixerSampler(Sampler):
        """The real Sampler's host logic (schedule upload, item_slices) over a handle that records: no library, no device."""
        made = []

        def __init__(self, **kw):
            self.kw, self.device, self.single_only = kw, kw["device"], 0
            self.cfg = types.SimpleNamespace(max_batch=kw["max_batch"], max_frames=kw["max_frames"], mixing_mode=kw.get("mixing_mode", 4))
            self.uploads = []
            self.lib = types.SimpleNamespace(mmdm_set_schedule=lambda h, tmap, coef, n, s: self.uploads.append(n) or 0)
            self.h, self.schedule, self._strategy = None, None, None
            self.stream = types.SimpleNamespace(wait_stream=lambda s: None, synchronize=lambda: None)
            self.calls, self.etas, self.closed, self.fail_at, self.kids = [], [], False, None, []
            type(self).made.append(self)

        def _s(self):
            return None

        def close(self):
            self.closed = True

        def share(self, max_batch=None, max_frames=None):
            self.kids.append(type(self)(**{**self.kw, "max_batch": max_batch, "max_frames": max_frames}))
            return self.kids[-1]

        def load_state_dict(self, sd):
            self.loaded = sorted(sd)

        def set_norm_stats(self, *a):
            pass

        def prepare(self):
            pass

        def set_eta(self, eta):
            self.etas.append(float(eta))
            self.eta = float(eta)

        def _hist(self, names, every, rows_shape):
            slots = (self._steps + every - 1) // every
            w = lambda n: (262 if self.cfg.mixing_mode >= 3 else 1) if n.startswith("influence") else 524
            base = torch.arange(slots * rows_shape[0] * rows_shape[1], dtype=torch.float32).reshape(slots, *rows_shape, 1) + 1e5 * len(self.calls)
            return {n: base.expand(slots, *rows_shape, w(n)) for n in names}

        def begin(self, cond, x_T, **kw):
            self.calls.append(dict(begin=kw, cond=cond, x_T=x_T))
            self.B, self.T = x_T.shape[:2]
            self.lens, self.rows = None, self.B * self.T
            self._steps = self.schedule.num_timesteps - kw.get("skip_timesteps", 0)

        def set_history(self, names, every=1):
            self.calls[-1]["history"] = (list(names), every)
            return self._hist(names, every, (2 * self.B, self.T))

        def run(self, nsteps=None, use_graph=True):
            self.calls[-1]["run"] = (nsteps, use_graph)

        def state(self, sync=True):
            return {"pred_xstart2": torch.full((self.B, self.T, 524), float(len(self.calls)))}

        def enqueue(self, cond, x_T, out, hist=None, history_every=1, use_graph=True):
            self.calls.append(dict(enqueue=tuple(x_T.shape), history=(sorted(hist or {}), history_every)))
            out.fill_(float(len(self.calls)))

        def sample_ragged_async(self, cond, x_T, lens, history=None, history_every=1, **kw):
            if self.fail_at == len(self.calls):
                raise RuntimeError("boom")
            self.calls.append(dict(cond=cond, lens=list(lens), history=(history, history_every), kw=kw))
            self.lens, self.rows = list(lens), sum(lens) + 5
            self._steps = self.schedule.num_timesteps - kw.get("skip_timesteps", 0)
            items = [torch.full((t, 524), 100.0 * len(self.calls) + k) for k, t in enumerate(lens)]
            return items, (self._hist(history, history_every, (2, self.rows)) if history else None), types.SimpleNamespace(synchronize=lambda: None)

    return FakeMixerSampler


@pytest.fixture
def mixer(monkeypatch, tmp_path):
    """A tiny MixerMDM (mixing mode 4, ddim4, store_influence) over FakeMixerSampler."""
    import contextlib
    import yaml
    from mixermdm_amd import models
    from mixermdm_amd.configs import CfgNode
    sub = dict(NUM_LAYERS=1, NUM_HEADS=2, DROPOUT=0.1, INPUT_DIM=262, LATENT_DIM=16, FF_SIZE=32)
    yaml.safe_dump(dict(NAME="in2INind", **sub), open(tmp_path / "individual.yaml", "w"))
    yaml.safe_dump(dict(NAME="InterGen", **sub), open(tmp_path / "intergen.yaml", "w"))
    cfg = CfgNode(dict(NAME="MixerMDM", GENERATOR=dict(sub), DISCRIMINATOR=dict(sub), ACTIVATION="gelu", DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine", SAMPLER="uniform",
                       MOTION_REP="global", CFG_WEIGHT=3.5, MIXING_MODE=4, FORCE_INFLUENCE_VAL="None", MODEL1="individual.yaml", MODEL2="intergen.yaml"))
    Fake = _fake_mixer_sampler()
    monkeypatch.setattr(models, "Sampler", Fake)
    monkeypatch.setattr(models.MixerMDM, "device", property(lambda self: Dev("cpu")))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(wait_stream=lambda s: None))
    monkeypatch.setattr(torch.cuda, "device", lambda dev=None: contextlib.nullcontext())
    m = models.MixerMDM(cfg, num_frames=16, sampling_strategy="ddim4", config_root=str(tmp_path))
    m.set_norm_stats(*[np.zeros(262)] * 4)
    return m, Fake


def mbatch(nb, T, **kw):
    return {**dict(cond=torch.zeros(nb, 8 * 768), motion_lens=torch.tensor([T] * nb), x_T=torch.zeros(nb, T, 524)), **kw}


def hist_value(call, rows, slot, half, row):
    """FakeMixerSampler's history entry: [slots, 2, rows] counted up from 1e5 * the call's number."""
    return 1e5 * call + (slot * 2 + half) * rows + row


def test_mixermdm_sample_many_ragged_transcript(mixer, monkeypatch):
    from mixermdm_amd import models
    m, Fake = mixer
    batches = [mbatch(b, T) for b, T in THREE]
    out = m.sample_many(batches, mode="eval", max_rows=60)
    s = Fake.made[-1]
    names = ["influence_i1", "influence_i2", "out1", "out2", "out_influenced"]
    assert len(Fake.made) == 1 and (s.kw["max_batch"], s.kw["max_frames"]) == (3, 33) and s.uploads == [4] and m.mixing.mode == "eval"
    assert [c["lens"] for c in s.calls] == [[12, 12, 33], [20, 20, 20]] and all(c["kw"] == {} and c["history"] == (names, 1) for c in s.calls) and s.etas == []
    assert [tuple(o["output"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)] and all(sorted(o) == sorted(names + ["output"]) for o in out)
    assert [float(v) for o in out for v in o["output"][:, 0, 0]] == [100.0, 101.0, 102.0, 200.0, 201.0, 202.0]
    # the reference's [2b, T, C] history rows: the batch's cond rows, then its uncond rows, each motion from its slice of its group
    for i, (b, T) in enumerate(THREE):
        for n in names:
            assert len(out[i][n]) == 4 and all(tuple(h.shape) == (2 * b, T, 262 if n.startswith("influence") else 524) for h in out[i][n])
    assert float(out[0]["out1"][2][1, 3, 0]) == hist_value(1, 62, 2, 0, 12 + 3) and float(out[0]["out1"][2][3, 3, 5]) == hist_value(1, 62, 2, 1, 12 + 3)
    assert float(out[1]["influence_i2"][0][1, 32, 0]) == hist_value(1, 62, 0, 1, 24 + 32) and float(out[2]["out2"][3][2, 0, 0]) == hist_value(2, 65, 3, 0, 40)
    # what is kept: the mode's names, or none; history_every is handed down; the schedule is uploaded once
    s.calls.clear()
    m.history_every = 2
    out = m.sample_many(batches, mode="eval_intermediate", max_items=2)
    assert [c["lens"] for c in s.calls] == [[12, 12], [33, 20], [20, 20]] and all(c["history"] == (names[:2], 2) for c in s.calls)
    assert sorted(out[0]) == ["influence_i1", "influence_i2", "output"] and len(out[0]["influence_i1"]) == 2 and out[0]["influence_i1"][0].shape == (4, 12, 262)
    m.history_every = 1
    for mode, keys in (("eval", names), ("eval_intermediate", names[:2])):
        s.calls.clear()
        out = m.sample_many(batches, mode=mode, keep_history=False, max_rows=60)
        assert all(c["history"] == (None, 1) for c in s.calls) and all(o[k] == [] for o in out for k in keys) and sorted(out[0]) == sorted(keys + ["output"])
    m.mixing.store_influence = False
    s.calls.clear()
    assert m.sample_many(batches, max_rows=60)[0]["influence_i1"] == [] and s.calls[0]["history"] == (None, 1)
    m.mixing.store_influence = True
    s.calls.clear()
    m.sample_many([mbatch(1, 70), mbatch(2, 10)], max_rows=60)
    assert len(Fake.made) == 2 and s.closed and Fake.made[-1].kw["max_frames"] == 70     # T grew: a new handle, as wide as the last
    s = Fake.made[-1]
    assert [c["lens"] for c in s.calls] == [[70], [10, 10]] and s.kw["max_batch"] == 3 and s.uploads == [4] and Fake.made[0].uploads == [4]
    # eta > 0 and skip_timesteps: named and drawn seeds, the generator's rows, S - skip history entries
    s.calls.clear()
    d = drawn(11, 2)
    torch.manual_seed(11)
    out = m.sample_many([mbatch(2, 12), mbatch(1, 33, seed=6), mbatch(3, 20)], eta=1.0, skip_timesteps=1, max_rows=60)
    assert [c["kw"] for c in s.calls] == [dict(skip_timesteps=1, seeds=[d[0], d[0], 6], noise_rows=[0, 1, 0]), dict(skip_timesteps=1, seeds=[d[1]] * 3, noise_rows=[0, 1, 2])]
    assert s.etas == [1.0, 0.0] and len(out[2]["influence_i1"]) == 3 and s.uploads == [4]
    s.calls.clear()
    sn = [torch.arange(4 * b * T * 524, dtype=torch.float32).reshape(4, b, T, 524) for b, T in THREE]
    m.sample_many([mbatch(b, T, step_noise=n) for (b, T), n in zip(THREE, sn)], eta=0.5, skip_timesteps=1, max_rows=60)
    kw = s.calls[0]["kw"]
    assert sorted(kw) == ["noise", "skip_timesteps"] and [tuple(t.shape) for t in kw["noise"]] == [(3, 12, 524), (3, 12, 524), (3, 33, 524)]
    assert torch.equal(kw["noise"][1], sn[0][:3, 1]) and torch.equal(s.calls[1]["kw"]["noise"][2], sn[2][:3, 2]) and s.etas[-2:] == [0.5, 0.0]
    s.calls.clear()
    s.etas.clear()
    m.sample_many([mbatch(b, T, x_start=torch.zeros(b, T + 2, 524), init_image=torch.full((b, T, 524), float(i))) for i, (b, T) in enumerate(THREE)], max_rows=60)
    kw = s.calls[0]["kw"]
    assert sorted(kw) == ["init_image", "skip_timesteps", "x_start"] and kw["skip_timesteps"] == 0 and s.etas == []
    assert [t.shape[0] for t in kw["x_start"]] == [14, 14, 35] and [float(t[0, 0]) for t in kw["init_image"]] == [0.0, 0.0, 1.0]
    # eta is the call's, also when the second group fails
    s.calls.clear()
    s.fail_at = 1
    with pytest.raises(RuntimeError, match="boom"):
        m.sample_many(batches, eta=1.0, max_rows=60)
    assert s.etas == [1.0, 0.0] and len(s.calls) == 1
    s.fail_at = None
    b = lambda **k: mbatch(1, 8, **k)
    for text, bs, kw in (("batching 'threads' not recognized", [b()], dict(batching="threads")),
                         ("eta=-1.0 must be >= 0", [b()], dict(eta=-1)),
                         ("^sample_many: batch 1 differs from batch 0 in whether it gives 'x_start': give it for every batch or for none", [b(x_start=torch.zeros(1, 8, 524)), b()], {}),
                         ("^sample_many: batch 0 gives both 'seed' and 'step_noise'", [b(seed=1, step_noise=torch.zeros(4, 1, 8, 524))], dict(eta=1.0)),
                         ("^sample_many: batch 1 names its step noise as a 'noise', batch 0 as a 'seed': one noise form per call",
                          [b(seed=1), b(step_noise=torch.zeros(4, 1, 8, 524))], dict(eta=1.0)),
                         ('^sample_many: batching="inflight" takes no eta / skip_timesteps / x_start / init_image; use "ragged" or "sequential"', [b()],
                          dict(batching="inflight", skip_timesteps=1)),
                         (r"^sample_many: batch 0: step_noise \[>= 3, 1, 8, 524\] expected, got \(2, 1, 8, 524\)", [b(step_noise=torch.zeros(2, 1, 8, 524))], dict(eta=1.0, skip_timesteps=1)),
                         (r"^sample_many: batch 1: x_start \[1, T, 524\] expected, got \(2, 8, 524\)", [b(x_start=torch.zeros(1, 8, 524)), b(x_start=torch.zeros(2, 8, 524))], {}),
                         (r"^sample_many: batch 0: init_image \[1, T, 524\] expected, got \(8, 524\)", [b(init_image=torch.zeros(8, 524))], {}),
                         (r"skip_timesteps=4 outside \[0, 4\)", [b()], dict(skip_timesteps=4))):
        with pytest.raises(ValueError, match=text):
            m.sample_many(bs, **kw)
    # the history budget, per ragged group: (frames + 128) rows of 2 * 262 + 3 * 524 floats, cond and uncond, 4 steps
    per_row = 4 * 2 * 4 * (2 * 262 + 3 * 524)
    monkeypatch.setattr(models, "HISTORY_BUDGET_BYTES", per_row * (57 + 128))
    s.calls.clear()
    with pytest.raises(MemoryError, match=r"history side outputs of a ragged batch of 60 frames need 0\.0 GiB; lower max_rows, set model.history_every, or pass keep_history=False"):
        m.sample_many(batches, mode="eval", max_rows=60)
    assert len(s.calls) == 1                                               # the first group of 57 frames fits and was queued
    m.sample_many(batches, mode="eval", max_rows=60, keep_history=False)


def test_mixermdm_sample_many_sequential_and_inflight_transcript(mixer, monkeypatch):
    from mixermdm_amd import models
    m, Fake = mixer
    m.num_frames = 40
    batches = [mbatch(b, T) for b, T in THREE]
    names = ["influence_i1", "influence_i2", "out1", "out2", "out_influenced"]
    plain = dict(noise=None, seed=None, x_start=None, init_image=None, skip_timesteps=0)
    out = m.sample_many(batches, mode="eval", batching="sequential")
    s = Fake.made[-1]
    assert len(Fake.made) == 2 and s.kw["max_batch"] == 3 and s.kw["max_frames"] == 40      # one call after the other: the handle grows with them
    assert [f.uploads for f in Fake.made] == [[4], [4]] and s.etas == []
    calls = [c for f in Fake.made for c in f.calls]
    assert [tuple(c["x_T"].shape) for c in calls] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)]
    assert all(c["begin"] == plain and c["history"] == (names, 1) and c["run"] == (None, True) for c in calls)
    assert [tuple(o["output"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)] and sorted(out[0]) == sorted(names + ["output"])
    assert [len(o["out1"]) for o in out] == [4, 4, 4] and out[2]["influence_i1"][3].shape == (6, 20, 262) and out[2]["out_influenced"][0].shape == (6, 20, 524)
    # keep_history=False: the influences are switched off for the calls and on again; mode "eval" still keeps its three outputs
    s.calls.clear()
    out = m.sample_many(batches, mode="eval_intermediate", batching="sequential", keep_history=False)
    assert all("history" not in c for c in s.calls) and all(o["influence_i1"] == [] and sorted(o) == ["influence_i1", "influence_i2", "output"] for o in out)
    assert m.mixing.store_influence is True and len(Fake.made) == 2 and s.uploads == [4]
    s.calls.clear()
    out = m.sample_many(batches, mode="eval", batching="sequential", keep_history=False)
    assert all(c["history"] == (names[2:], 1) for c in s.calls) and out[0]["influence_i1"] == [] and len(out[0]["out2"]) == 4 and m.mixing.store_influence is True
    s.calls.clear()
    assert len(m.sample_many(batches, batching="sequential")[1]["influence_i2"]) == 4 and all(c["history"] == (names[:2], 1) for c in s.calls)
    # the loop's options go through ddim_sample_loop: every call sets its eta and clears it
    s.calls.clear()
    d = drawn(11, 2)
    torch.manual_seed(11)
    xs = torch.zeros(1, 40, 524)
    out = m.sample_many([mbatch(2, 12), mbatch(1, 33, seed=6, x_start=xs), mbatch(3, 20)][1:2] + [mbatch(2, 12, x_start=xs[:, :12].repeat(2, 1, 1))], batching="sequential",
                        eta=1.0, skip_timesteps=1)
    assert [c["begin"]["seed"] for c in s.calls] == [6, d[0]] and all(c["begin"]["skip_timesteps"] == 1 and c["begin"]["noise"] is None for c in s.calls)
    assert s.calls[0]["begin"]["x_start"] is xs and s.etas == [1.0, 0.0, 1.0, 0.0] and [len(o["influence_i1"]) for o in out] == [3, 3] and s.uploads == [4]
    s.calls.clear()
    sn = torch.ones(4, 1, 8, 524)
    m.sample_many([mbatch(1, 8, step_noise=sn)], batching="sequential", eta=0.5)
    assert s.calls[0]["begin"]["noise"] is sn and s.calls[0]["begin"]["seed"] is None and s.etas[-2:] == [0.5, 0.0]
    with pytest.raises(ValueError, match=r"skip_timesteps=4 outside \[0, 4\)"):
        m.sample_many([mbatch(1, 8)], batching="sequential", skip_timesteps=4)
    # in flight: `inflight` handles over one weight set, every one on the call's schedule, calls dealt round-robin
    s.calls.clear()
    out = m.sample_many(batches, mode="eval", batching="inflight", inflight=2, keep_history=False)
    pool = [s] + s.kids
    assert len(pool) == 2 and [p.uploads for p in pool] == [[4], [4]] and (s.kids[0].kw["max_batch"], s.kids[0].kw["max_frames"]) == (3, 40)
    assert [c["enqueue"] for c in s.calls] == [(2, 12, 524), (3, 20, 524)] and [c["enqueue"] for c in s.kids[0].calls] == [(1, 33, 524)]
    assert all(c["history"] == ([], 1) for p in pool for c in p.calls) and [tuple(o["output"].shape) for o in out] == [(2, 12, 524), (1, 33, 524), (3, 20, 524)]
    out = m.sample_many(batches, mode="eval", batching="inflight", inflight=2)
    assert s.calls[-1]["history"] == (sorted(names), 1) and out[2]["out1"][3].shape == (6, 20, 524) and out[1]["influence_i1"][0].shape == (2, 33, 262) and len(out[0]["out2"]) == 4
    # the history budgets of the two paths: bytes per (motion, frame) = slots * 2 rows * 4 bytes * the widths kept
    per_row = 4 * 2 * 4 * (2 * 262 + 3 * 524)
    monkeypatch.setattr(models, "HISTORY_BUDGET_BYTES", per_row * 117 - 1)
    with pytest.raises(MemoryError, match=r"history side outputs of 3 in-flight calls need 0\.0 GiB; pass fewer batches per call, set model.history_every, or pass keep_history=False"):
        m.sample_many(batches, mode="eval", batching="inflight", inflight=2)
    m.sample_many(batches, mode="eval_intermediate", batching="inflight", inflight=2)
    monkeypatch.setattr(models, "HISTORY_BUDGET_BYTES", per_row * 60 - 1)
    with pytest.raises(MemoryError, match=r"history side outputs need 0\.0 GiB for 4 steps \(the reference keeps every step: mixermdm.py:794-808\); set model.history_every = k to keep "
                                          "every k-th step, or store_influence=False / forward_test"):
        m.sample_many(batches, mode="eval", batching="sequential")
    m.history_every = 2
    assert len(m.sample_many(batches, mode="eval", batching="sequential")[2]["out1"]) == 2

"""GPU: the stand-alone InterGen sampler (single_only = 4: InterDenoiser alone under the 2-way CFG) with the loop's options -- against the reference
(tests/golden/intergen_standalone.npz at latent 16 for fp32; intergen_standalone32.npz at latent 32, the smallest sizes the 16-bit GEMMs take, for fp32 and
fp32_split; tests/golden/make_golden_intergen.py) and against identities that rest on no tolerance -- and the InterGen / InterDiffusion facades.
B = 2, T = 20, ddim4."""
import ctypes as C
import numpy as np
import pytest
import torch

from test_intergen_cpu import CASES, fixture_inputs, tiny_cfg

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
LOOP_BOUND = dict(mean=2e-3, p99=3e-2)       # the project's loop bound (tests/test_gpu_sampler_opts.py, tests/test_gpu_facade.py)
COLS = [0, 2, 262, 264]
PRECISIONS = ("fp32", "fp32_split", "bf16", "bf16_fp8")


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


class Case:
    """A fixture's inputs (re-drawn from its seeds) and a tiny sampler in one precision mode."""

    def __init__(self, golden, fixture, prec):
        from mixermdm_amd.sampler import Sampler
        self.g, w, _ = golden(fixture)
        g = self.g
        self.B, self.T, self.S = int(g["B"]), int(g["T"]), 4
        v = {k: t.cuda() for k, t in fixture_inputs(g).items()}
        self.x_T, self.cond, self.x_start, self.init, self.noise = v["x_T"], v["cond"], v["x_start"], v["init"], v["noise"]
        self.W = {"denoiser2." + k: t for k, t in w("ig.").items()}
        self.s = Sampler(d_latent=int(g["latent_dim"]), d_ff=int(g["ff_size"]), d_layers=int(g["num_layers"]), d_heads=int(g["H"]), single_only=4, model2_kind=1,
                         cfg_scale=float(g["cfg_scale"]), max_batch=3, max_frames=40, precision=prec)
        self.s.load_state_dict(self.W)
        self.s.prepare()
        self.s.set_schedule(str(g["strategy"]))
        assert self.s.schedule.num_timesteps == self.S

    def kwargs(self, name, noise=None):
        eta, pin, init, skip = [float(v) for v in self.g[f"case:{name}"]]
        skip = int(skip)
        kw = dict(eta=eta, skip_timesteps=skip)
        if eta:
            kw["noise"] = (self.noise if noise is None else noise)[:self.S - skip]
        if pin:
            kw["x_start"] = self.x_start
        if init:
            kw["init_image"] = self.init
        return kw


@pytest.fixture(scope="module")
def case(golden):
    c = Case(golden, "intergen_standalone", "fp32")
    c.plain = c.s.sample(c.cond, c.x_T, use_graph=False)
    yield c
    c.s.close()


# ---------------------------------------------------------------------------------------------------
# 1. every fixture case against the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture, prec", [("intergen_standalone", "fp32"), ("intergen_standalone32", "fp32"), ("intergen_standalone32", "fp32_split")])
def test_cases_vs_reference_golden(golden, fixture, prec):
    c = Case(golden, fixture, prec)
    try:
        outs = {}
        for name in CASES:
            out = outs[name] = c.s.sample(c.cond, c.x_T, use_graph=False, **c.kwargs(name))
            d = np.abs(out.cpu().numpy() - c.g[f"{name}:output"])
            print("%s %s %s: mean err %.3e, p99 %.3e, max %.3e" % (fixture, prec, name, d.mean(), np.percentile(d, 99), d.max()))
            assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (name, d.mean(), np.percentile(d, 99), d.max())
        for name in CASES[1:]:
            assert float((outs[name] - outs["plain"]).abs().mean()) > 0.03, name       # and it is not the plain loop
    finally:
        c.s.close()


# ---------------------------------------------------------------------------------------------------
# 2. identities
# ---------------------------------------------------------------------------------------------------
def test_pinned_loop_is_the_manual_loop_bitwise(case):
    s = case.s
    s.set_eta(0.0)
    out = s.sample(case.cond, case.x_T, use_graph=False, x_start=case.x_start)
    left = {k: v.clone() for k, v in s.state().items() if k in ("x", "pred_xstart")}
    s.begin(case.cond, case.x_T)
    for _ in range(case.S):
        s.state()["x"][:, :, COLS] = case.x_start[:, :case.T, COLS]
        torch.cuda.synchronize()
        s.run(1, use_graph=False)
    st = s.state()
    assert torch.equal(st["pred_xstart"], out) and not torch.equal(out, case.plain)
    for k in left:
        assert torch.equal(st[k], left[k]), k
    assert st["x2"] is None and st["pred_xstart2"] is None
    assert not torch.equal(st["x"][:, :, COLS], case.x_start[:, :case.T, COLS])          # the sample the last step leaves is not pinned


@pytest.mark.parametrize("skip, with_init", [(1, True), (0, True), (2, False)])
def test_init_image_start_and_the_loop_from_there(case, skip, with_init):
    s, S = case.s, case.S
    s.set_eta(0.0)
    s.begin(case.cond, case.x_T, init_image=case.init if with_init else None, skip_timesteps=skip)
    x0 = s.state()["x"].clone()
    i0 = S - 1 - skip
    a, b = np.sqrt(s.schedule.alphas_cumprod[i0]), np.sqrt(1.0 - s.schedule.alphas_cumprod[i0])
    want = a * (case.init.double() if with_init else 0.0) + b * case.x_T.double()
    assert torch.allclose(x0.double(), want, rtol=1e-6, atol=1e-6), float((x0.double() - want).abs().max())
    s.run(None, use_graph=False)
    out = s.state()["pred_xstart"].clone()
    s.begin(case.cond, x0)
    s.seek(i0)
    s.run(None, use_graph=False)
    assert torch.equal(s.state()["pred_xstart"], out)


def test_seed_is_the_noise_buffer_filled_by_randn(case):
    from mixermdm_amd import ops
    s = case.s
    a = s.sample(case.cond, case.x_T, use_graph=False, eta=0.5, seed=SEED)
    xa = s.state()["x"].clone()
    buf = torch.stack([ops.randn(SEED, k, case.B, case.T) for k in range(case.S)])
    b = s.sample(case.cond, case.x_T, use_graph=False, eta=0.5, noise=buf)
    assert torch.equal(a, b) and torch.equal(s.state()["x"], xa)
    c = s.sample(case.cond, case.x_T, use_graph=False, eta=0.5, seed=SEED + 1)
    assert not torch.equal(a, c)
    s.set_eta(0.0)


def test_no_noise_at_the_last_step(case):
    """Two noise buffers that differ in the last slot only leave bitwise equal chains; differing in the slot before does not."""
    s, S = case.s, case.S
    other, other2 = case.noise.clone(), case.noise.clone()
    other[S - 1] = rnd(999, case.B, case.T, 524).cuda()
    other2[S - 2] = rnd(998, case.B, case.T, 524).cuda()
    fin = []
    for buf in (case.noise, other, other2):
        s.sample(case.cond, case.x_T, use_graph=False, eta=1.0, noise=buf)
        fin.append(s.state()["x"].clone())
    s.set_eta(0.0)
    assert torch.equal(fin[0], fin[1]) and not torch.equal(fin[0], fin[2])


def test_graph_replay_equals_eager_for_every_call_form(case):
    """Each call form replayed == eager, bitwise; new option VALUES replay the same graph, another form never does; the plain call is unchanged before and
    after; a zeroed mmdm_begin_options is mmdm_begin."""
    from mixermdm_amd._lib import BeginOptions, check
    s = case.s
    s.set_eta(0.0)
    assert torch.equal(s.sample(case.cond, case.x_T, use_graph=True), case.plain)
    cap = s.graph_stats()[0]
    forms = [case.kwargs("all"), case.kwargs("pin"), case.kwargs("eta"), dict(eta=1.0, seed=SEED), dict(eta=1.0, seed=SEED, x_start=case.x_start), case.kwargs("init")]
    new = [1, 1, 1, 1, 1, 0]               # (init_image / skip change values only: the plain graph)
    for kw, n in zip(forms, new):
        eager = s.sample(case.cond, case.x_T, use_graph=False, **kw)
        graph = s.sample(case.cond, case.x_T, use_graph=True, **kw)
        assert torch.equal(eager, graph), sorted(kw)
        cap += n
        assert s.graph_stats()[0] == cap, sorted(kw)
    kw = case.kwargs("all")
    kw2 = dict(kw, noise=torch.stack([rnd(700 + k, case.B, case.T, 524) for k in range(case.S - 1)]).cuda(), x_start=rnd(710, case.B, case.T, 524).cuda(),
               init_image=rnd(711, case.B, case.T, 524).cuda())
    g2 = s.sample(case.cond, case.x_T, use_graph=True, **kw2)
    assert s.graph_stats()[0] == cap                                   # new values, same graph
    assert torch.equal(g2, s.sample(case.cond, case.x_T, use_graph=False, **kw2))
    s.set_eta(0.0)
    assert torch.equal(s.sample(case.cond, case.x_T, use_graph=True), case.plain) and s.graph_stats()[0] == cap
    o = BeginOptions()
    with torch.cuda.device(s.device):
        check(s.lib.mmdm_begin_opts(s.h, C.c_void_p(case.cond.data_ptr()), C.c_void_p(case.x_T.data_ptr()), case.B, case.T, C.byref(o), s._s()), s.h)
        check(s.lib.mmdm_run(s.h, case.S, 0, s._s()), s.h)
    assert torch.equal(s.state()["pred_xstart"], case.plain)
    out = torch.empty_like(case.plain)
    check(s.lib.mmdm_copy_result(s.h, C.c_void_p(out.data_ptr()), s._s()), s.h)
    s.synchronize()
    assert torch.equal(out, case.plain)


# ---------------------------------------------------------------------------------------------------
# 3. ragged batches: every item is its stand-alone call, with and without the options, in every precision mode
# ---------------------------------------------------------------------------------------------------
LENS = (8, 20, 17, 64, 33)
RAG_DIMS = dict(d_latent=128, d_ff=256, d_layers=2)


def ragged_sampler(prec):
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import denoiser_shapes
    g = torch.Generator().manual_seed(7)
    sd = {k: torch.randn(shp, generator=g) * (0.05 if len(shp) == 2 else 0.02) for k, shp in denoiser_shapes("denoiser2.", 128, 256, 2).items()}
    s = Sampler(d_heads=2, single_only=4, model2_kind=1, cfg_scale=3.5, max_batch=len(LENS), max_frames=64, precision=prec, **RAG_DIMS)
    s.load_state_dict(sd)
    s.prepare()
    s.set_schedule("ddim4")
    return s


_FP32_RAGGED = {}


@pytest.mark.parametrize("prec", PRECISIONS)
def test_ragged_items_equal_their_own_calls_bitwise(prec):
    s = ragged_sampler(prec)
    try:
        B, S = len(LENS), 4
        cond = rnd(800, B, 768).cuda()
        xs = [rnd(810 + b, T, 524).cuda() for b, T in enumerate(LENS)]
        xst = [rnd(820 + b, T + 3, 524).cuda() for b, T in enumerate(LENS)]
        ini = [0.5 * rnd(830 + b, T, 524).cuda() for b, T in enumerate(LENS)]
        seeds = [SEED + 17 * b for b in range(B)]
        for tag, rk, ik in (("plain", {}, lambda b: {}),
                            ("options", dict(eta=1.0, seeds=seeds, x_start=xst, init_image=ini, skip_timesteps=1),
                             lambda b: dict(eta=1.0, seed=seeds[b], x_start=xst[b][None], init_image=ini[b][None], skip_timesteps=1))):
            items = s.sample_ragged(cond, xs, list(LENS), **rk)
            again = s.sample_ragged(cond, xs, list(LENS), use_graph=False, **rk)
            for b, T in enumerate(LENS):
                alone = s.sample(cond[b:b + 1], xs[b][None], **ik(b))[0]
                assert items[b].shape == (T, 524)
                assert torch.equal(items[b], alone), (prec, tag, b)
                assert torch.equal(again[b], alone), (prec, tag, b, "eager")
            s.set_eta(0.0)
            full = torch.cat(items, 0)
            if prec == "fp32":
                _FP32_RAGGED[tag] = full
            elif tag in _FP32_RAGGED:           # a figure for DESIGN.md, no tolerance: the low-precision modes against the fp32 loop
                d = (full - _FP32_RAGGED[tag]).abs()
                print("%s %s: distance to the fp32 loop: mean %.3e, p99 %.3e, max %.3e" % (prec, tag, d.mean(), d.flatten().kthvalue(int(0.99 * d.numel())).values, d.max()))
        # one seed for the batch: a uniform batch's rows
        T = 20
        xu = rnd(840, 3, T, 524).cuda()
        u = s.sample(cond[:3], xu, eta=0.5, seed=SEED)
        r = s.sample_ragged(cond[:3], [xu[b] for b in range(3)], [T] * 3, eta=0.5, seeds=SEED)
        s.set_eta(0.0)
        assert all(torch.equal(r[b], u[b]) for b in range(3))
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 4. refusals of the new mode, each by its message
# ---------------------------------------------------------------------------------------------------
def test_refusals(case):
    from mixermdm_amd._lib import MMDMError
    from mixermdm_amd.sampler import Sampler
    s, S = case.s, case.S
    ARG, STATE, UNSUPPORTED = 1, 2, 4

    def refused(match, fn, status):
        with pytest.raises(MMDMError, match=match) as e:
            fn()
        assert e.value.status == status

    refused("single_only = 4 is the stand-alone InterGen sampler and needs model2_kind = 1",
            lambda: Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=2, single_only=4, model2_kind=0), ARG)
    refused("single_only must be 0, 1, 2, 3 or 4", lambda: Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=2, single_only=5), ARG)
    refused("single_only = 4 -- the stand-alone InterGen sampler takes no key mask", lambda: s.set_key_mask(torch.ones(case.B, case.T)), UNSUPPORTED)
    s.set_eta(0.0)
    s.begin(case.cond, case.x_T)
    refused("only the two-chain MixerMDM sampler has history side outputs", lambda: s.set_history(("out1",)), STATE)
    refused(r"x_start has 10 frames, the call has T=20", lambda: s.begin(case.cond, case.x_T, x_start=case.x_start[:, :10]), ARG)
    refused(r"skip_timesteps=4 outside \[0, 4\)", lambda: s.begin(case.cond, case.x_T, skip_timesteps=S), ARG)
    refused("a noise source is given and no eta table is set", lambda: s.begin(case.cond, case.x_T, seed=1), STATE)
    s.set_eta(0.5)
    refused("names no noise source", lambda: s.begin(case.cond, case.x_T), STATE)
    refused("the noise buffer holds 3 steps, 4 are left", lambda: s.begin(case.cond, case.x_T, noise=case.noise[:3]), ARG)
    s.begin(case.cond, case.x_T, noise=case.noise[:3], skip_timesteps=1)
    s.seek(1)
    refused("run past the call's noise buffer", lambda: s.run(2), ARG)
    s.set_eta(0.0)
    assert torch.equal(s.sample(case.cond, case.x_T, use_graph=False), case.plain)      # the handle is as it was


# ---------------------------------------------------------------------------------------------------
# 5. the facades
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(golden):
    from mixermdm_amd.models import InterGen
    g, w, _ = golden("intergen_standalone")
    m = InterGen(tiny_cfg())
    m.load_state_dict({"state_dict": {"model.decoder.net." + k: v for k, v in w("ig.").items()}})
    m.decoder.num_frames = 64
    return m.to("cuda")


def test_facade_forward_test_and_forward_with_options(model, case):
    batch = {"cond": case.cond, "motion_lens": torch.tensor([case.T, case.T]), "x_T": case.x_T}
    out = model.forward_test(dict(batch))
    assert set(out) >= {"cond", "output"} and out["output"].shape == (case.B, case.T, 524)
    for name, o in (("plain", out["output"]),
                    ("all", model.forward(dict(batch), eta=1.0, step_noise=case.noise, x_start=case.x_start, init_image=case.init, skip_timesteps=1)["output"]),
                    ("plain", model.forward_test(dict(batch))["output"])):                 # and eta does not stay behind
        d = np.abs(o.cpu().numpy() - case.g[f"{name}:output"])
        print("facade %s: mean err %.3e, p99 %.3e" % (name, d.mean(), np.percentile(d, 99)))
        assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (name, d.mean(), d.max())
    assert torch.equal(out["output"], case.plain)
    torch.manual_seed(5)
    a = model.decoder(dict(batch), eta=0.5)["output"]
    torch.manual_seed(5)
    b = model.decoder(dict(batch), eta=0.5)["output"]
    assert torch.equal(a, b) and not torch.equal(a, model.decoder(dict(batch), eta=0.5)["output"])
    with pytest.raises(ValueError, match="not both"):
        model.decoder(dict(batch), eta=0.5, seed=1, step_noise=case.noise)


def test_facade_text_process_vs_reference_golden(golden):
    from mixermdm_amd.models import InterGen
    g, w, t = golden("text")
    m = InterGen(tiny_cfg()).to("cuda")
    m.text_num_heads = int(g["H"])
    m.load_state_dict({"decoder.net." + k[len("net."):]: v for k, v in m.decoder.state_dict().items()} | dict(w("txt.")), strict=False)
    batch = m.text_process({"tokens_text": t("tokens").long()})
    got, want = batch["cond"].cpu(), t("intergen:cond")
    assert got.shape == want.shape
    assert torch.allclose(got, want, atol=2e-5, rtol=1e-4), float((got - want).abs().max())


def test_sample_many_and_generate_for_evaluation():
    """Ragged == sequential, bitwise: the plain call through generate_for_evaluation (seed= names every item's x_T), and sample_many with the options.
    Synthetic weights at latent 128, 2 heads: ragged batches need head size 64 / 128."""
    from mixermdm_amd.generation import generate_for_evaluation
    from mixermdm_amd.models import InterGen
    from mixermdm_amd.synthetic import denoiser_shapes
    gen = torch.Generator().manual_seed(7)
    model = InterGen(tiny_cfg(LATENT_DIM=128, FF_SIZE=256))
    model.load_state_dict({k: torch.randn(shp, generator=gen) * (0.05 if len(shp) == 2 else 0.02) for k, shp in denoiser_shapes("decoder.net.", 128, 256, 2).items()})
    model.decoder.num_frames = 64
    model = model.to("cuda")
    lens = (8, 20, 17, 33)
    items = [{"text": ("a",), "motion_lens": torch.tensor([T]), "cond": rnd(900 + i, 1, 768).cuda()} for i, T in enumerate(lens)]
    kw = dict(max_length=40, mm_idxs=(1,), mm_num_repeats=2, extended=False, seed=11)
    seq, mm_seq = generate_for_evaluation(model, items, batching="sequential", **kw)
    rag, mm_rag = generate_for_evaluation(model, items, batching="ragged", **kw)
    assert len(seq) == len(rag) == 4 and len(mm_seq) == len(mm_rag) == 1
    for a, b in zip(seq, rag):
        assert np.array_equal(a["motion1"], b["motion1"]) and np.array_equal(a["motion2"], b["motion2"]) and np.abs(a["motion1"]).sum() > 0
    assert np.array_equal(mm_seq[0]["mm_motions"], mm_rag[0]["mm_motions"]) and mm_seq[0]["mm_motions"].shape[0] == 2
    batches = [dict(cond=rnd(910 + i, nb, 768).cuda(), motion_lens=torch.tensor([T] * nb), x_T=rnd(920 + i, nb, T, 524).cuda(), seed=30 + i,
                    x_start=rnd(930 + i, nb, T + 2, 524).cuda(), init_image=rnd(940 + i, nb, T, 524).cuda()) for i, (nb, T) in enumerate([(2, 12), (1, 33), (3, 20)])]
    a = model.sample_many(batches, batching="sequential", eta=1.0, skip_timesteps=1)
    b = model.sample_many(batches, batching="ragged", eta=1.0, skip_timesteps=1)
    c = model.sample_many(batches, batching="ragged")
    for x, y, z, bt in zip(a, b, c, batches):
        assert x["output"].shape == bt["x_T"].shape and torch.equal(x["output"], y["output"]) and not torch.equal(y["output"], z["output"])


# ---------------------------------------------------------------------------------------------------
# 6. the teacher-forced denoiser forward of the mode
# ---------------------------------------------------------------------------------------------------
def test_module_forward_is_the_inter_denoiser_and_the_step_is_its_cfg_combine(case, golden):
    """mmdm_module_forward(which = 1) on the mode-4 handle against the oracle's InterDenoiser (tolerance of the same comparison in
    tests/test_gpu_sampler.py), the other modules refused, the schedule kept; and one step's pred_xstart is the 2-way CFG combine of that forward on the
    doubled batch -- the step's single row group of conditioning against the forward's three (1e-5: the same arithmetic, other GEMM row counts)."""
    from mixermdm_amd._lib import MMDMError
    from oracle.denoiser import inter_denoiser
    s, B, T = case.s, case.B, case.T
    _, w, _ = golden("intergen_standalone")
    W = w("ig.", [("sequence_pos_encoder.pe", 16)])
    x2 = torch.cat([case.x_T, case.x_T], 0)
    c3 = torch.cat([case.cond.repeat(1, 3), torch.zeros(B, 3 * 768, device="cuda")], 0)
    i = case.S - 1
    t = int(s.schedule.timestep_map[i])
    out = s.module_forward(1, x2, c3, t)
    ref = inter_denoiser(W, "", x2.cpu(), torch.full((2 * B,), t, dtype=torch.long), c3.cpu(), int(case.g["H"]))
    assert torch.allclose(out.cpu(), ref, atol=1e-4, rtol=1e-3), float((out.cpu() - ref).abs().max())
    for which in (0, 2, 3, 4):
        with pytest.raises(MMDMError, match="bad module|needs the two-chain handle"):
            s.module_forward(which, x2, c3, t, x2=x2)
    s.set_eta(0.0)
    s.begin(case.cond, case.x_T)
    s.run(1, use_graph=False)
    px = s.state()["pred_xstart"]
    cs = float(case.g["cfg_scale"])
    want = cs * out[:B] + (1.0 - cs) * out[B:]
    assert torch.allclose(px, want, atol=1e-5, rtol=1e-5), float((px - want).abs().max())
    assert torch.equal(s.sample(case.cond, case.x_T, use_graph=False), case.plain)       # the schedule survived the forward

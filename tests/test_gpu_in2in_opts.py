"""GPU: the one-chain sampler under the 4-way CFG (single_only = 4, cfg_form = 1) and DualMDM (cfg_form = 2) -- the stand-alone in2IN samplers with the
loop's options and ragged batches.  The new forms are the old samplers (single_only 2 / 3) bit for bit on a plain call; the options are checked against
identities that rest on no tolerance, in all four precision modes; ragged items equal their own calls bitwise; the refusals are named."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
COLS = [0, 2, 262, 264]
PRECISIONS = ("fp32", "fp32_split", "bf16", "bf16_fp8")
FORMS = (1, 2)
DUAL_WEIGHTS = (("const", 0.3), ("exp", 0.005))          # one constant and one time-varying composition weight
SCALES = dict(cfg_scale=3.5, cfg_scale_interaction=1.5, cfg_scale_individual=0.75)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


# ---------------------------------------------------------------------------------------------------
# 1. the new forms are the old samplers, bit for bit
# ---------------------------------------------------------------------------------------------------
def golden_sampler(golden, form, legacy):
    """The sampler of tests/golden/interaction.npz (form 1) or dual.npz (form 2): as single_only = 2 / 3 (legacy) or as single_only = 4 with cfg_form."""
    from mixermdm_amd.sampler import Sampler
    g, w, t = golden("interaction" if form == 1 else "dual")
    kw = dict(d_latent=16, d_ff=32, d_layers=2, d_heads=int(g["H"]), cfg_scale_interaction=float(g["s_int"]), cfg_scale_individual=float(g["s_ind"]),
              max_batch=2, max_frames=16)
    if form == 1:
        kw["cfg_scale"] = float(g["s"])
    kw.update(dict(single_only=form + 1) if legacy else dict(single_only=4, cfg_form=form))
    s = Sampler(**kw)
    W = {"denoiser2." + k: v for k, v in w("int.").items()}
    if form == 2:
        W.update({"denoiser1." + k: v for k, v in w("ind.").items()})
    s.load_state_dict(W)
    s.prepare()
    return s, g, t


@pytest.mark.parametrize("form", FORMS)
def test_new_form_is_the_old_sampler_bitwise(golden, form):
    old, g, t = golden_sampler(golden, form, True)
    new, _, _ = golden_sampler(golden, form, False)
    try:
        cond, x_T = t("cond").cuda(), t("x_T").cuda()
        for s in (old, new):
            s.set_schedule("ddim20")
        for func, value in (DUAL_WEIGHTS if form == 2 else ((None, None),)):
            if form == 2:
                for s in (old, new):
                    s.set_dual_weights(func, value)
            for graph in (False, True):
                a = old.sample(cond, x_T, use_graph=graph)
                b = new.sample(cond, x_T, use_graph=graph)
                assert a.shape == (2, 12, 524) and torch.equal(a, b), (form, func, graph)
                sa, sb = old.state(), new.state()
                assert torch.equal(sa["x"], sb["x"]) and torch.equal(sa["pred_xstart"], sb["pred_xstart"]) and sb["x2"] is None
        # and it still is the reference's loop (the bound of tests/test_gpu_sampler.py / test_gpu_extensions.py for these fixtures)
        key = "loop:ddim20:output" if form == 1 else "loop:exp:ddim20:output"
        if form == 2:
            new.set_dual_weights("exp", float(g["cfg:exp:value"]))
        d = np.abs(new.sample(cond, x_T).cpu().numpy() - g[key])
        assert d.mean() <= 1e-4 and d.max() <= 1e-2, (d.mean(), d.max())
    finally:
        old.close()
        new.close()


# ---------------------------------------------------------------------------------------------------
# synthetic samplers at latent 128 / 2 heads: head size 64, the smallest the ragged attention covers and a size every precision mode takes
# ---------------------------------------------------------------------------------------------------
LENS = (8, 20, 17, 64, 33, 1)          # one frame, half a 16-key chunk, a chunk + 1 and + 4, exactly four chunks, two chunks + 1: 143 frames, 113 padding rows
LENS2 = (5, 31, 16, 60, 30, 2)         # other lengths, the same row bucket (144 -> 256) and the same query tiles


def synthetic_sampler(form, prec, max_batch, max_frames, heads=2, latent=128):
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import denoiser_shapes
    g = torch.Generator().manual_seed(7)
    shapes = dict(denoiser_shapes("denoiser2.", latent, 2 * latent, 2))
    if form == 2:
        shapes.update(denoiser_shapes("denoiser1.", latent, 2 * latent, 2))
    sd = {k: torch.randn(shp, generator=g) * (0.05 if len(shp) == 2 else 0.02) for k, shp in shapes.items()}
    s = Sampler(d_latent=latent, d_ff=2 * latent, d_layers=2, d_heads=heads, single_only=4, cfg_form=form, max_batch=max_batch, max_frames=max_frames,
                precision=prec, **SCALES)
    s.load_state_dict(sd)
    s.prepare()
    s.set_schedule("ddim4")
    if form == 2:
        s.set_dual_weights("exp", 0.005)
    return s


def cond_of(form, seed, B):
    return rnd(seed, B, (3 if form == 1 else 5) * 768).cuda()


# ---------------------------------------------------------------------------------------------------
# 3. identities that rest on no tolerance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("form", FORMS)
def test_option_identities(form, prec):
    B, T, S = 2, 20, 4
    s = synthetic_sampler(form, prec, B, 24)
    try:
        cond, x_T = cond_of(form, 100, B), rnd(101, B, T, 524).cuda()
        x_start, init = rnd(102, B, 30, 524).cuda(), 0.5 * rnd(103, B, T, 524).cuda()
        noise = torch.stack([rnd(110 + k, B, T, 524) for k in range(S)]).cuda()
        plain = s.sample(cond, x_T, use_graph=False)

        # the pinned loop is the manual loop that overwrites the four root columns before each eager step
        out = s.sample(cond, x_T, use_graph=False, x_start=x_start)
        left = {k: v.clone() for k, v in s.state().items() if k in ("x", "pred_xstart")}
        s.begin(cond, x_T)
        for _ in range(S):
            s.state()["x"][:, :, COLS] = x_start[:, :T, COLS]
            torch.cuda.synchronize()
            s.run(1, use_graph=False)
        st = s.state()
        assert torch.equal(st["pred_xstart"], out) and not torch.equal(out, plain)
        assert all(torch.equal(st[k], left[k]) for k in left) and st["x2"] is None

        # init_image / skip_timesteps: the start is q_sample, the loop from there is begin(x0); seek(i0); run
        for skip, with_init in ((1, True), (0, True), (2, False)):
            s.begin(cond, x_T, init_image=init if with_init else None, skip_timesteps=skip)
            x0 = s.state()["x"].clone()
            i0 = S - 1 - skip
            a, b = np.sqrt(s.schedule.alphas_cumprod[i0]), np.sqrt(1.0 - s.schedule.alphas_cumprod[i0])
            want = a * (init.double() if with_init else 0.0) + b * x_T.double()
            assert torch.allclose(x0.double(), want, rtol=1e-6, atol=1e-6), float((x0.double() - want).abs().max())
            s.run(None, use_graph=False)
            o = s.state()["pred_xstart"].clone()
            s.begin(cond, x0)
            s.seek(i0)
            s.run(None, use_graph=False)
            assert torch.equal(s.state()["pred_xstart"], o), (skip, with_init)

        # seed= is noise= filled by ops.randn
        from mixermdm_amd import ops
        a = s.sample(cond, x_T, use_graph=False, eta=0.5, seed=SEED)
        xa = s.state()["x"].clone()
        buf = torch.stack([ops.randn(SEED, k, B, T) for k in range(S)])
        assert torch.equal(a, s.sample(cond, x_T, use_graph=False, eta=0.5, noise=buf)) and torch.equal(s.state()["x"], xa)
        assert not torch.equal(a, s.sample(cond, x_T, use_graph=False, eta=0.5, seed=SEED + 1)) and not torch.equal(a, plain)

        # no noise at the last step: buffers that differ in the last slot only leave equal chains, differing in the slot before does not
        other, other2 = noise.clone(), noise.clone()
        other[S - 1] = rnd(999, B, T, 524).cuda()
        other2[S - 2] = rnd(998, B, T, 524).cuda()
        fin = []
        for nb in (noise, other, other2):
            s.sample(cond, x_T, use_graph=False, eta=1.0, noise=nb)
            fin.append(s.state()["x"].clone())
        assert torch.equal(fin[0], fin[1]) and not torch.equal(fin[0], fin[2])

        # graph replay equals eager for every call form; another form never replays a form's graph, new values do
        s.set_eta(0.0)
        assert torch.equal(s.sample(cond, x_T, use_graph=True), plain)
        cap = s.graph_stats()[0]
        every = dict(eta=1.0, noise=noise[:S - 1], x_start=x_start, init_image=init, skip_timesteps=1)
        forms = [(every, 1), (dict(eta=0.0, x_start=x_start), 1), (dict(eta=0.5, noise=noise), 1), (dict(eta=1.0, seed=SEED), 1),
                 (dict(eta=1.0, seed=SEED, x_start=x_start), 1), (dict(eta=0.0, init_image=init, skip_timesteps=1), 0)]
        for kw, n in forms:
            eager = s.sample(cond, x_T, use_graph=False, **kw)
            assert torch.equal(eager, s.sample(cond, x_T, use_graph=True, **kw)), sorted(kw)
            cap += n
            assert s.graph_stats()[0] == cap, sorted(kw)
        kw2 = dict(every, noise=torch.stack([rnd(700 + k, B, T, 524) for k in range(S - 1)]).cuda(), x_start=rnd(710, B, T, 524).cuda())
        g2 = s.sample(cond, x_T, use_graph=True, **kw2)
        assert s.graph_stats()[0] == cap and torch.equal(g2, s.sample(cond, x_T, use_graph=False, **kw2))
        s.set_eta(0.0)
        assert torch.equal(s.sample(cond, x_T, use_graph=True), plain) and s.graph_stats()[0] == cap
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 4. ragged items equal their own calls, bitwise
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("form", FORMS)
def test_ragged_items_equal_their_own_calls_bitwise(form, prec):
    s = synthetic_sampler(form, prec, len(LENS), 64)
    try:
        B, S = len(LENS), 4
        cond = cond_of(form, 800, B)
        xs = [rnd(810 + b, T, 524).cuda() for b, T in enumerate(LENS)]
        xst = [rnd(820 + b, T + 3, 524).cuda() for b, T in enumerate(LENS)]
        ini = [0.5 * rnd(830 + b, T, 524).cuda() for b, T in enumerate(LENS)]
        nz = [rnd(840 + b, S, T, 524).cuda() for b, T in enumerate(LENS)]
        seeds = [SEED + 17 * b for b in range(B)]
        rows = [3, 0, 5, 1, 0, 2]
        calls = (("plain", {}, lambda b: {}),
                 ("seeds + noise_rows", dict(eta=0.5, seeds=seeds, noise_rows=rows), None),
                 ("packed noise", dict(eta=0.5, noise=torch.cat(nz, 1)), lambda b: dict(eta=0.5, noise=nz[b][:, None])),
                 ("x_start + init_image + skip", dict(eta=1.0, seeds=seeds, x_start=xst, init_image=ini, skip_timesteps=1),
                  lambda b: dict(eta=1.0, seed=seeds[b], x_start=xst[b][None], init_image=ini[b][None], skip_timesteps=1)))
        for tag, rk, ik in calls:
            items = s.sample_ragged(cond, xs, list(LENS), **rk)
            again = s.sample_ragged(cond, xs, list(LENS), use_graph=False, **rk)
            for b, T in enumerate(LENS):
                if ik is None:      # item b draws row rows[b] of its generator: the last row of a uniform call of rows[b] + 1 copies of the item
                    k = rows[b] + 1
                    alone = s.sample(cond[b:b + 1].repeat(k, 1), xs[b][None].repeat(k, 1, 1), eta=0.5, seed=seeds[b])[k - 1]
                else:
                    alone = s.sample(cond[b:b + 1], xs[b][None], **ik(b))[0]
                assert items[b].shape == (T, 524)
                assert torch.equal(items[b], alone), (form, prec, tag, b)
                assert torch.equal(again[b], alone), (form, prec, tag, b, "eager")
            s.set_eta(0.0)
        # padding rows stay zero; a second batch of other lengths in the same row bucket replays the captured graph
        s.sample_ragged(cond, xs, list(LENS))
        st = s.state()
        assert st["x"].shape[0] > sum(LENS) and not st["x"][sum(LENS):].any()
        cap = s.graph_stats()[0]
        xs2 = [rnd(850 + b, T, 524).cuda() for b, T in enumerate(LENS2)]
        items = s.sample_ragged(cond, xs2, list(LENS2))
        assert s.graph_stats()[0] == cap
        for b in (1, 3, 5):
            assert torch.equal(items[b], s.sample(cond[b:b + 1], xs2[b][None])[0]), (form, prec, "second batch", b)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 5. refusals by name and status
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_refusals(form):
    from mixermdm_amd._lib import MMDMError
    from mixermdm_amd.sampler import Sampler
    ARG, STATE, UNSUPPORTED = 1, 2, 4
    B, T = 2, 12

    def refused(match, fn, status):
        with pytest.raises(MMDMError, match=match) as e:
            fn()
        assert e.value.status == status

    tiny = dict(d_latent=16, d_ff=32, d_layers=2, d_heads=2)
    refused(r"cfg_form must be 0 \(2-way CFG\), 1 \(4-way CFG\) or 2 \(DualMDM\), got cfg_form = 3", lambda: Sampler(single_only=4, cfg_form=3, **tiny), ARG)
    refused("cfg_form = 1 selects the guidance wrapper of the one-chain sampler and needs single_only = 4, got single_only = 2",
            lambda: Sampler(single_only=2, cfg_form=1, **tiny), ARG)
    s = synthetic_sampler(form, "fp32", B, 16, heads=16)          # head size 8
    try:
        cond, x_T = cond_of(form, 300, B), rnd(301, B, T, 524).cuda()
        noise = torch.stack([rnd(310 + k, B, T, 524) for k in range(4)]).cuda()
        plain = s.sample(cond, x_T, use_graph=False)
        if form == 2:
            s.set_schedule("ddim4")              # a new schedule drops the weights
            refused("call mmdm_set_dual_weights after mmdm_set_schedule", lambda: s.begin(cond, x_T), STATE)
            s.set_dual_weights("exp", 0.005)
        with pytest.raises(ValueError, match=f"cfg_form={form} takes cond"):
            s.begin(cond[:, :768], x_T)
        refused("single_only = 4 -- the stand-alone InterGen sampler takes no key mask", lambda: s.set_key_mask(torch.ones(B, T)), UNSUPPORTED)
        s.begin(cond, x_T)
        refused("only the two-chain MixerMDM sampler has history side outputs", lambda: s.set_history(("out1",)), STATE)
        refused(r"head size 8 \(the ragged attention kernels cover 64 and 128\)", lambda: s.begin_ragged(cond, [x_T[0], x_T[1, :7]], [T, 7]), UNSUPPORTED)
        refused("a noise source is given and no eta table is set", lambda: s.begin(cond, x_T, seed=1), STATE)
        s.set_eta(0.5)
        refused("names no noise source", lambda: s.begin(cond, x_T), STATE)
        refused("the noise buffer holds 3 steps, 4 are left", lambda: s.begin(cond, x_T, noise=noise[:3]), ARG)
        s.set_eta(0.0)
        refused(r"x_start has 10 frames, the call has T=12", lambda: s.begin(cond, x_T, x_start=noise[0][:, :10]), ARG)
        assert torch.equal(s.sample(cond, x_T, use_graph=False), plain)      # the handle is as it was
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 2. every fixture case against the reference
# ---------------------------------------------------------------------------------------------------
LOOP_BOUND = dict(mean=2e-3, p99=3e-2)       # the project's loop bound (tests/test_gpu_intergen.py)


def fixture_sampler(g, prec, legacy=False):
    """The sampler of an in2in_opts / in2in_dual_opts fixture, its weights re-drawn from the fixture's seeds."""
    from mixermdm_amd.sampler import Sampler
    from test_in2in_opts_cpu import fixture_weights
    dual = "w:exp" in g
    kw = dict(cfg_scale_interaction=float(g["s_int"]), cfg_scale_individual=float(g["s_ind"]))
    if not dual:
        kw["cfg_scale"] = float(g["s"])
    kw.update(dict(single_only=3 if dual else 2) if legacy else dict(single_only=4, cfg_form=2 if dual else 1))
    s = Sampler(d_latent=int(g["latent_dim"]), d_ff=int(g["ff_size"]), d_layers=int(g["num_layers"]), d_heads=int(g["H"]), max_batch=3, max_frames=40,
                precision=prec, **kw)
    W = fixture_weights(g, "int", "denoiser2.")
    if dual:
        W.update(fixture_weights(g, "ind", "denoiser1."))
    s.load_state_dict(W)
    s.prepare()
    s.set_schedule(str(g["strategy"]))
    return s


def case_kwargs(g, v, name, S=4):
    eta, pin, init, skip = [float(x) for x in g[f"case:{name}"]]
    skip = int(skip)
    kw = dict(eta=eta, skip_timesteps=skip)
    if eta:
        kw["noise"] = v["noise"][:S - skip]
    if pin:
        kw["x_start"] = v["x_start"]
    if init:
        kw["init_image"] = v["init"]
    return kw


@pytest.mark.parametrize("fixture, prec", [("in2in_opts", "fp32"), ("in2in_opts32", "fp32"), ("in2in_opts32", "fp32_split"),
                                           ("in2in_dual_opts", "fp32"), ("in2in_dual_opts32", "fp32"), ("in2in_dual_opts32", "fp32_split")])
def test_cases_vs_reference_golden(golden, fixture, prec):
    from test_in2in_opts_cpu import fixture_inputs, fixture_sets
    g, _, _ = golden(fixture)
    s = fixture_sampler(g, prec)
    try:
        v = {k: t.cuda() for k, t in fixture_inputs(g).items()}
        for pre, func, cases in fixture_sets(g):
            if func:
                s.set_dual_weights(func, float(g[f"w:{func}"]))
            outs = {}
            for name in cases:
                out = outs[name] = s.sample(v["cond"], v["x_T"], use_graph=False, **case_kwargs(g, v, name))
                d = np.abs(out.cpu().numpy() - g[f"{pre}{name}:output"])
                print("%s %s %s%s: mean err %.3e, p99 %.3e, max %.3e" % (fixture, prec, pre, name, d.mean(), np.percentile(d, 99), d.max()))
                assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (pre, name, d.mean(), np.percentile(d, 99), d.max())
            for name in cases[1:]:
                assert float((outs[name] - outs["plain"]).abs().mean()) > 0.03, (pre, name)       # and it is not the plain loop
            s.set_eta(0.0)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 6. the facades
# ---------------------------------------------------------------------------------------------------
def facade(mode, latent=16, heads=2, strategy="ddim4", **over):
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import in2IN
    c = dict(NAME="in2IN", LATENT_DIM=latent, FF_SIZE=2 * latent, NUM_LAYERS=2, NUM_HEADS=heads, INPUT_DIM=262, CFG_WEIGHT=3.0, CFG_WEIGHT_INTERACTION=3.0,
             CFG_WEIGHT_INDIVIDUAL=1.0, STRATEGY=strategy, DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine", W_FUNC="exp", W_VALUE=0.004)
    c.update(over)
    return in2IN(CfgNode(c), mode)


def cond_batch(cond, **kw):
    """A cond [B, 3 or 5 text slices] as the cond_* entries in2INDiffusion.forward concatenates."""
    names = ("cond_interaction", "cond_interaction_individual1", "cond_interaction_individual2", "cond_individual_individual1", "cond_individual_individual2")
    return {**{n: cond[:, 768 * i:768 * (i + 1)] for i, n in enumerate(names[:cond.shape[1] // 768])}, **kw}


@pytest.mark.parametrize("fixture", ["in2in_opts", "in2in_dual_opts"])
def test_facade_forward_is_the_sampler_call(golden, fixture):
    from test_in2in_opts_cpu import fixture_inputs, fixture_weights
    g, _, _ = golden(fixture)
    dual = "w:exp" in g
    v = {k: t.cuda() for k, t in fixture_inputs(g).items()}
    m = facade("dual" if dual else "interaction", CFG_WEIGHT_INTERACTION=float(g["s_int"]), CFG_WEIGHT_INDIVIDUAL=float(g["s_ind"]))
    W = fixture_weights(g, "int", "net_interaction.")
    if dual:
        W.update(fixture_weights(g, "ind", "net_individual."))
    m.decoder.load_state_dict(W)
    m = m.to("cuda")
    new, old = fixture_sampler(g, "fp32"), fixture_sampler(g, "fp32", legacy=True)
    try:
        if dual:
            for s in (new, old):
                s.set_dual_weights("exp", 0.004)
        pre = "exp:" if dual else ""
        batch = cond_batch(v["cond"], x_T=v["x_T"], motion_lens=torch.tensor([20, 20]))
        plain = m.forward_test(dict(batch))["output"]
        assert torch.equal(plain, old.sample(v["cond"], v["x_T"])) and torch.equal(plain, new.sample(v["cond"], v["x_T"]))
        d = np.abs(plain.cpu().numpy() - g[f"{pre}plain:output"])
        assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"]
        got = m.decoder(dict(batch), eta=1.0, step_noise=v["noise"], x_start=v["x_start"], init_image=v["init"], skip_timesteps=1)["output"]
        assert torch.equal(got, new.sample(v["cond"], v["x_T"], **case_kwargs(g, v, "all"))) and not torch.equal(got, plain)
        assert torch.equal(m.decoder(dict(batch))["output"], plain)                          # eta does not stay behind
        torch.manual_seed(5)
        a = m.decoder(dict(batch), eta=0.5)["output"]
        torch.manual_seed(5)
        assert torch.equal(a, m.decoder(dict(batch), eta=0.5)["output"]) and not torch.equal(a, m.decoder(dict(batch), eta=0.5)["output"])
        with pytest.raises(ValueError, match="not both"):
            m.decoder(dict(batch), eta=0.5, seed=1, step_noise=v["noise"])
        # an explicit mask builds the stand-alone sampler of the mode and gets its refusal by name; the next call is the one-chain handle again
        with pytest.raises(NotImplementedError, match="single_only = 3" if dual else "single_only = 2"):
            m.decoder(dict(batch), mask=torch.ones(2, 20, 1).cuda())
        assert torch.equal(m.decoder(dict(batch))["output"], plain)
    finally:
        new.close()
        old.close()


def synthetic_facade(mode):
    from mixermdm_amd.synthetic import denoiser_shapes
    gen = torch.Generator().manual_seed(7)
    m = facade(mode, latent=128, CFG_WEIGHT=3.5, CFG_WEIGHT_INTERACTION=1.5, CFG_WEIGHT_INDIVIDUAL=0.75)
    nets = {"individual": ["net_individual."], "interaction": ["net_interaction."], "dual": ["net_individual.", "net_interaction."]}[mode]
    sd = {}
    for n in nets:
        sd.update({k: torch.randn(shp, generator=gen) * (0.05 if len(shp) == 2 else 0.02) for k, shp in denoiser_shapes(n, 128, 256, 2).items()})
    m.decoder.load_state_dict(sd)
    m.decoder.num_frames = 64
    return m.to("cuda")


@pytest.mark.parametrize("mode", ["interaction", "dual"])
def test_sample_many_and_generate_for_evaluation(mode):
    """Ragged == sequential, bitwise: the plain call through generate_for_evaluation (seed= names every item's x_T; a stand-in text encoder maps a text to
    its cond), and sample_many with the options.  Synthetic weights at latent 128, 2 heads: ragged batches need head size 64 / 128."""
    import zlib
    from mixermdm_amd.generation import generate_for_evaluation
    model = synthetic_facade(mode)

    def text_encoder(batch, tmode, text_name, out_name):
        batch[out_name] = torch.cat([rnd(zlib.crc32((t + "|" + tmode + "|" + out_name).encode()), 1, 768) for t in batch[text_name]], 0).cuda()
        return batch

    model.text_encoder = text_encoder
    lens = (8, 20, 17, 33)
    items = [{"text": (f"two people {i}",), "text_individual1": (f"one {i}",), "text_individual2": (f"other {i}",), "motion_lens": torch.tensor([T])}
             for i, T in enumerate(lens)]
    kw = dict(max_length=40, mm_idxs=(1,), mm_num_repeats=2, extended=True, seed=11)
    seq, mm_seq = generate_for_evaluation(model, items, batching="sequential", **kw)
    rag, mm_rag = generate_for_evaluation(model, items, batching="ragged", **kw)
    assert len(seq) == len(rag) == 4 and len(mm_seq) == len(mm_rag) == 1
    for a, b in zip(seq, rag):
        assert np.array_equal(a["motion1"], b["motion1"]) and np.array_equal(a["motion2"], b["motion2"]) and np.abs(a["motion1"]).sum() > 0
    assert np.array_equal(mm_seq[0]["mm_motions"], mm_rag[0]["mm_motions"]) and mm_seq[0]["mm_motions"].shape[0] == 2
    k = 3 if mode == "interaction" else 5
    batches = [cond_batch(rnd(910 + i, nb, k * 768).cuda(), motion_lens=torch.tensor([T] * nb), x_T=rnd(920 + i, nb, T, 524).cuda(), seed=30 + i,
                          x_start=rnd(930 + i, nb, T + 2, 524).cuda(), init_image=rnd(940 + i, nb, T, 524).cuda()) for i, (nb, T) in enumerate([(2, 12), (1, 33), (3, 20)])]
    a = model.sample_many(batches, batching="sequential", eta=1.0, skip_timesteps=1)
    b = model.sample_many(batches, batching="ragged", eta=1.0, skip_timesteps=1)
    c = model.sample_many(batches, batching="ragged")
    d = model.sample_many(batches, batching="sequential")
    for x, y, z, w, bt in zip(a, b, c, d, batches):
        assert x["output"].shape == bt["x_T"].shape and torch.equal(x["output"], y["output"]) and torch.equal(z["output"], w["output"])
        assert not torch.equal(y["output"], z["output"])
    with pytest.raises(ValueError, match="batching 'inflight' not recognized"):
        model.sample_many(batches, batching="inflight")


def test_individual_mode_keeps_its_refusals_and_runs_ragged():
    model = synthetic_facade("individual")
    batches = [dict(cond_individual_individual1=rnd(950 + i, nb, 768).cuda(), motion_lens=torch.tensor([T] * nb), x_T=rnd(960 + i, nb, T, 262).cuda())
               for i, (nb, T) in enumerate([(2, 12), (1, 33), (3, 20)])]
    a = model.decoder.sample_many(batches, batching="sequential")
    b = model.decoder.sample_many(batches, batching="ragged")
    for x, y, bt in zip(a, b, batches):
        assert x["output"].shape == bt["x_T"].shape and torch.equal(x["output"], y["output"])
    for kw in (dict(eta=0.5), dict(skip_timesteps=1), dict(x_start=rnd(970, 2, 14, 524).cuda())):
        with pytest.raises(NotImplementedError, match="single_only = 1"):
            model.decoder(dict(batches[0]), **kw)
    with pytest.raises(NotImplementedError, match="single_only = 1"):
        model.decoder.sample_many(batches, batching="ragged", eta=0.5)
    assert torch.equal(model.decoder(dict(batches[0]))["output"], a[0]["output"])

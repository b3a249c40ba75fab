"""GPU: DDIM inversion on the one-chain samplers (Sampler.begin_reverse / run_reverse / invert over mmdm_ddim_reverse_f32, the facades' invert / invert_many).

  1. reference parity: every set-up x case of tests/golden/inversion_*.npz within the project's loop bounds, and within 3 x the reference's own fp32 rounding
     of its float64 run (DESIGN section 3's yardstick);
  2. the reverse update kernel against its float64 formula on constructed rows: first, middle and last step, both widths, a ragged group with padding rows;
  3. the off-by-one identity: with a constant model, k reverse steps and the forward steps k .. 1 return the motion;
  4. bitwise: graph == eager, invert(2) + run_reverse(2) == invert(4), a reverse call between two forward calls, ragged items == their own calls in every
     precision mode, invert_many ragged == sequential, start_step = S - 1 == the plain loop;
  5. the refusals, each by its message."""
import ctypes as C
import numpy as np
import pytest
import torch

import inversion_cases as IC

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "fp32_split", "bf16", "bf16_fp8")
ARG, STATE, UNSUPPORTED = 1, 2, 4


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def err(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return d.mean(), np.percentile(d, 99), d.max()


# ---------------------------------------------------------------------------------------------------
# 1. reference parity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,setup,prec", IC.PARITY, ids=[f"{fx}-{prec}" for fx, _, prec in IC.PARITY])
def test_latents_vs_reference_golden(golden, fixture, setup, prec):
    """|GPU - reference fp32| within the loop bounds for the latent and for pred_xstart, and |GPU - reference float64| of the latent within 3 x the
    reference's own |fp32 - float64| (mean and 99th percentile).  Measured figures: DESIGN.md section 9f."""
    g, _, _ = golden(fixture)
    s = IC.make_sampler(g, setup, prec)
    try:
        x_0, cond = IC.inputs(g, setup)
        for name in IC.CASES:
            k = int(g[f"case:{name}"])
            lat = s.invert(cond.cuda(), x_0.cuda(), steps=k).cpu().numpy()
            px = s.state()["pred_xstart"].cpu().numpy()
            (lm, lp, lx), (pm, pp, _) = err(lat, g[f"{name}:latent"]), err(px, g[f"{name}:pred_xstart"])
            fm, fp, _ = err(lat, g[f"{name}:latent_f64"])
            rm, rp = g[f"{name}:latent:ref_f64_err"]
            print(f"PARITY {fixture} {prec} {name}: latent vs fp32 mean {lm:.3e} p99 {lp:.3e} max {lx:.3e}; pred_xstart mean {pm:.3e} p99 {pp:.3e}; "
                  f"latent vs f64 mean {fm:.3e} ({fm / rm:.2f} x ref) p99 {fp:.3e} ({fp / rp:.2f} x ref)")
            assert lm <= IC.BOUNDS[0] and lp <= IC.BOUNDS[1], (name, "latent", lm, lp)
            assert pm <= IC.BOUNDS[0] and pp <= IC.BOUNDS[1], (name, "pred_xstart", pm, pp)
            assert fm <= 3 * rm and fp <= 3 * rp, (name, "float64 yardstick", fm / rm, fp / rp)
            assert torch.equal(s.state()["x"].cpu(), torch.from_numpy(lat))
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 2. kernel level
# ---------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("Cw", [262, 524])
@pytest.mark.parametrize("i", [0, 25, 49])
def test_reverse_update_kernel_vs_float64_formula(i, Cw, ragged):
    """mmdm_ddim_reverse_f32 on constructed rows at ddim50: i = 0 (the smallest c_recipm1: eps is ~150 x the inputs), a middle step, i = S - 1 (rev =
    (0, 1): x becomes eps).  Bound: 3 x the error of the same formula evaluated in numpy fp32, maximum and mean.  Ragged: rows marked -1 keep their bits."""
    from mixermdm_amd._lib import load_library, check
    from mixermdm_amd.schedule import make_schedule
    lib = load_library()
    sch = make_schedule("cosine", 1000, "ddim50")
    coef, rev = sch.device_coefficients(), sch.reverse_coefficients()
    S, rows = 50, 21                                 # 21 rows x 262 / 524: more than one block of 256, the last one partial
    x0, x = rnd(10 + i, rows, Cw), 0.5 * rnd(20 + i, rows, Cw)
    item = np.repeat(np.arange(3), 7).astype(np.int32)
    if ragged:
        item[[4, 5, 13, 20]] = -1                    # padding rows inside and at the end of the group
    d_x0, d_x = x0.cuda(), x.clone().cuda()
    d_coef, d_rev, d_step = torch.from_numpy(coef).cuda(), torch.from_numpy(rev).cuda(), torch.tensor([i], dtype=torch.int32).cuda()
    d_item = torch.from_numpy(item).cuda()
    check(lib.mmdm_ddim_reverse_f32(_p(d_x0), _p(d_coef), _p(d_rev), S, _p(d_step), _p(d_x), rows, Cw, _p(d_item) if ragged else None, None))
    torch.cuda.synchronize()
    got = d_x.cpu().numpy()
    want = IC.reverse_update(x.numpy(), x0.numpy(), coef, rev, i, np.float64)
    np32 = IC.reverse_update(x.numpy(), x0.numpy(), coef, rev, i, np.float32)
    real = item >= 0
    e_gpu, e_np = np.abs(got[real] - want[real]), np.abs(np32[real].astype(np.float64) - want[real])
    print(f"KERNEL i={i} C={Cw} ragged={ragged}: |gpu - f64| max {e_gpu.max():.3e} mean {e_gpu.mean():.3e}; numpy fp32: max {e_np.max():.3e} mean {e_np.mean():.3e}")
    assert e_gpu.max() <= 3 * e_np.max() and e_gpu.mean() <= 3 * e_np.mean()
    if i == S - 1:                                   # x becomes eps
        eps = (coef[0, i].astype(np.float64) * x.numpy() - x0.numpy()) / coef[1, i].astype(np.float64)
        assert np.abs(got[real] - eps[real]).max() <= 3 * e_np.max()
    if ragged:
        assert np.array_equal(got[~real].view(np.uint32), x.numpy()[~real].view(np.uint32))
    assert np.isfinite(got).all() and torch.equal(d_x0.cpu(), x0)


# ---------------------------------------------------------------------------------------------------
# 3. the off-by-one identity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", list(IC.SETUPS))
def test_reverse_then_forward_returns_the_motion(golden, setup):
    """A constant model (the final layer's weight zeroed: every prediction is the layer's bias): invert(k), then begin + seek(k) + run(k), walks the levels
    ab[0] -> ab[k] -> ab[0].  state().x is held to the float64 restatement of the 2k updates on the fp32 tables within 3 x the deviation of the numpy fp32
    restatement from it (maximum and mean) -- ~5e-7; the float64 restatement itself returns the motion to the tables' rounding (5.3e-4: test_inversion_cpu.py).
    A wrong ab_next row or an index shift misses by 0.1 and more."""
    from mixermdm_amd.sampler import Sampler
    g, _, _ = golden(IC.SETUPS[setup][0][0])
    D, F, L, H = IC.dims(g)
    W = IC.weights(g, setup)
    final = "output_process.poseFinal." if setup == "mdm" else "out.linear."
    for k in [k for k in W if k.endswith(final + "weight")]:
        W[k] = torch.zeros_like(W[k])
    if setup == "dual":                              # one bias for both models: the composition weight then has nothing to blend
        W["denoiser1." + final + "bias"] = W["denoiser2." + final + "bias"].clone()
    kind = {"intergen": dict(single_only=4, model2_kind=1), "4way": dict(single_only=4, cfg_form=1), "dual": dict(single_only=4, cfg_form=2),
            "individual": dict(single_only=1), "mdm": dict(single_only=1, model1_kind=1)}[setup]
    B, T, Wd = 2, int(g["T"]), int(g["W"])
    s = Sampler(d_latent=D, d_ff=F, d_layers=L, d_heads=H, max_batch=B, max_frames=T, **kind, **IC.SCALES[setup])
    try:
        s.load_state_dict(W)
        s.prepare()
        x_0, cond = IC.inputs(g, setup)
        worst = 0.0
        for strat, ks in (("ddim4", (1, 2, 3)), ("ddim20", (7,))):
            s.set_schedule(strat)
            if setup == "dual":
                s.set_dual_weights("exp", 0.004)
            coef, rev = s.schedule.device_coefficients(), s.schedule.reverse_coefficients()
            for k in ks:
                lat = s.invert(cond.cuda(), x_0.cuda(), steps=k)
                x0 = s.state()["pred_xstart"].cpu().numpy()
                assert (x0 == x0[0, 0]).all() and np.abs(x0).max() > 0           # the model is constant
                s.begin(cond.cuda(), lat)
                s.seek(k)
                s.run(k)
                got = s.state()["x"].cpu().numpy()
                assert np.array_equal(s.state()["pred_xstart"].cpu().numpy(), x0)
                res = {}
                for dt in (np.float64, np.float32):
                    x = x_0.numpy().astype(dt)
                    for i in range(k):
                        x = IC.reverse_update(x, x0, coef, rev, i, dt)
                    res[dt, "latent"] = x
                    for i in range(k, 0, -1):
                        x = IC.forward_update(x, x0, coef, i, dt)
                    res[dt, "back"] = x
                for what, gpu in (("latent", lat.cpu().numpy()), ("back", got)):
                    e_gpu = np.abs(gpu - res[np.float64, what])
                    e_np = np.abs(res[np.float32, what].astype(np.float64) - res[np.float64, what])
                    ratio = max(e_gpu.max() / e_np.max(), e_gpu.mean() / e_np.mean())
                    worst = max(worst, ratio)
                    print(f"IDENTITY {setup} {strat} k={k} {what}: |gpu - f64| max {e_gpu.max():.3e} mean {e_gpu.mean():.3e}; numpy fp32 max {e_np.max():.3e} "
                          f"mean {e_np.mean():.3e}; ratio {ratio:.2f}; |gpu - motion| max {np.abs(got - x_0.numpy()).max():.3e}")
                    assert e_gpu.max() <= 3 * e_np.max() and e_gpu.mean() <= 3 * e_np.mean(), (strat, k, what, ratio)
                assert np.abs(got - x_0.numpy()).max() <= 2e-3
        print(f"IDENTITY {setup}: worst ratio {worst:.2f}")
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# 4. bitwise
# ---------------------------------------------------------------------------------------------------
LENS = (8, 20, 17, 64, 33)                     # half a 16-key chunk, a chunk + 4, + 1, exactly four chunks, two + 1: 142 frames -> 256 rows
LENS_MDM = (12, 63, 64, 33)                    # 64 frames are one tile of frames and two of tokens
MODES = {"intergen": PRECISIONS, "4way": PRECISIONS, "dual": PRECISIONS, "individual": PRECISIONS, "mdm": ("fp32", "fp32_split")}


def synth(setup, prec, max_batch, max_frames=64, strategy="ddim4"):
    """Synthetic weights at latent 128 / 2 heads: head size 64, the smallest the ragged attention covers and a size every precision mode takes."""
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import denoiser_shapes, mdm_denoiser_shapes
    gen = torch.Generator().manual_seed(7)
    if setup == "mdm":
        shapes = mdm_denoiser_shapes("denoiser1.", 128, 256, 2)
    else:
        shapes = {}
        if setup in ("dual", "individual"):
            shapes.update(denoiser_shapes("denoiser1.", 128, 256, 2))
        if setup != "individual":
            shapes.update(denoiser_shapes("denoiser2.", 128, 256, 2))
    sd = {k: torch.randn(shp, generator=gen) * (0.05 if len(shp) == 2 else 0.02) for k, shp in shapes.items()}
    for k in sd:
        if k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            sd[k] = sd[k] + 1.0                      # LayerNorm gamma
    kind = {"intergen": dict(single_only=4, model2_kind=1), "4way": dict(single_only=4, cfg_form=1), "dual": dict(single_only=4, cfg_form=2),
            "individual": dict(single_only=1), "mdm": dict(single_only=1, model1_kind=1)}[setup]
    s = Sampler(d_latent=128, d_ff=256, d_layers=2, d_heads=2, max_batch=max_batch, max_frames=max_frames, precision=prec, **kind, **IC.SCALES[setup])
    s.load_state_dict(sd)
    s.prepare()
    s.set_schedule(strategy)
    if setup == "dual":
        s.set_dual_weights("exp", 0.005)
    return s


def synth_inputs(setup, lens, seed=800):
    cw = 128 if setup == "mdm" else IC.COND_SLICES[setup] * 768
    Wd = 262 if setup in ("individual", "mdm") else 524
    return rnd(seed, len(lens), cw).cuda(), [0.5 * rnd(seed + 10 + b, T, Wd).cuda() for b, T in enumerate(lens)]


@pytest.mark.parametrize("setup,prec", [(su, p) for su, ps in MODES.items() for p in ps])
def test_ragged_items_equal_their_own_inversions_bitwise(setup, prec):
    """Every item of a ragged inversion is its stand-alone call, graph and eager, full (k = 4) and partial (k = 3); the group's padding rows stay zero; and
    invert(2) followed by run_reverse(2) is invert(4)."""
    lens = LENS_MDM if setup == "mdm" else LENS
    s = synth(setup, prec, len(lens))
    try:
        cond, xs = synth_inputs(setup, lens)
        for k in (4, 3):
            items = s.invert_ragged(cond, xs, list(lens), steps=k)
            st = s.state()
            assert s.rows % 128 == 0 and s.rows > sum(lens) and not st["x"][sum(lens):].any()
            eager = s.invert_ragged(cond, xs, list(lens), steps=k, use_graph=False)
            for b, T in enumerate(lens):
                alone = s.invert(cond[b:b + 1], xs[b][None], steps=k)[0]
                assert items[b].shape == alone.shape == xs[b].shape and torch.isfinite(alone).all()
                assert torch.equal(items[b], alone), (setup, prec, k, b, float((items[b] - alone).abs().max()))
                assert torch.equal(eager[b], alone), (setup, prec, k, b, "eager")
                if b == 1:
                    assert torch.equal(s.invert(cond[b:b + 1], xs[b][None], steps=k, use_graph=False)[0], alone)
            assert not torch.equal(items[1], xs[1])
        b = 1
        full = s.invert(cond[b:b + 1], xs[b][None], steps=4)
        px = s.state()["pred_xstart"].clone()
        part = s.invert(cond[b:b + 1], xs[b][None], steps=2)
        assert not torch.equal(part, full)
        s.run_reverse(2)
        assert torch.equal(s.state()["x"], full) and torch.equal(s.state()["pred_xstart"], px)
    finally:
        s.close()


@pytest.mark.parametrize("setup", ["intergen", "dual", "mdm"])
def test_reverse_call_between_forward_calls(setup):
    """A reverse step's model evaluation is the forward step's: an inversion between two forward calls replays their captured graph (nothing new is
    captured for the same B, T, S) and leaves the forward results' bits alone; eager and graph agree for both."""
    lens = LENS_MDM if setup == "mdm" else LENS
    s = synth(setup, "fp32", len(lens))
    try:
        cond, xs = synth_inputs(setup, lens)
        c1, x1 = cond[:1], xs[1][None]
        eager_f, eager_r = s.sample(c1, x1, use_graph=False), s.invert(c1, x1, use_graph=False)
        assert s.graph_stats() == (0, 0, 0)
        for what, want_cap in (("f", 1), ("r", 0), ("f", 0), ("r", 0)):
            cap, rep, _ = s.graph_stats()
            out = s.sample(c1, x1) if what == "f" else s.invert(c1, x1)
            assert torch.equal(out, eager_f if what == "f" else eager_r), what
            cap2, rep2, cached = s.graph_stats()
            assert cap2 - cap == want_cap and rep2 - rep == 4 and cached == 1, (what, cap, cap2, rep, rep2)
    finally:
        s.close()


@pytest.mark.parametrize("setup", list(IC.SETUPS))
def test_start_step_hands_a_partial_inversion_back_to_the_loop(setup):
    """sample_from(start_step=S - 1) is the plain sample; start_step=k is begin + seek(k) + run; ragged likewise."""
    lens = (12, 33)
    s = synth(setup, "fp32", 2)
    try:
        S = 4
        cond, xs = synth_inputs(setup, lens)
        c1, x1 = cond[:1], xs[0][None]
        plain = s.sample(c1, x1)
        assert torch.equal(s.sample_from(c1, x1, S - 1), plain)
        lat = s.invert(c1, x1, steps=2)
        a = s.sample_from(c1, lat, 2)
        s.begin(c1, lat)
        s.seek(2)
        s.run(3)
        assert torch.equal(s.state()["pred_xstart"], a) and not torch.equal(a, plain)
        rag = s.sample_ragged_from(cond, xs, list(lens), 2)
        for b in range(2):
            assert torch.equal(rag[b], s.sample_from(cond[b:b + 1], xs[b][None], 2)[0])
        with pytest.raises(ValueError, match="exclusive with init_image / skip_timesteps"):
            s.sample_from(c1, x1, 2, skip_timesteps=1)
        with pytest.raises(ValueError, match=r"start_step=4 outside \[0, 4\)"):
            s.sample_from(c1, x1, 4)
    finally:
        s.close()


def tiny_cfg(**over):
    from mixermdm_amd.configs import CfgNode
    c = dict(NAME="InterGen", LATENT_DIM=128, FF_SIZE=256, NUM_LAYERS=2, NUM_HEADS=2, INPUT_DIM=262, CFG_WEIGHT=3.5, CFG_WEIGHT_INTERACTION=3.0,
             CFG_WEIGHT_INDIVIDUAL=1.0, STRATEGY="ddim4", DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine", W_FUNC="exp", W_VALUE=0.004)
    c.update(over)
    return CfgNode(c)


def facade(name):
    """(model on the GPU, batch maker) of a facade with synthetic weights at latent 128."""
    from mixermdm_amd.models import InterGen, in2IN, MDM
    gen = torch.Generator().manual_seed(7)
    if name == "InterGen":
        m = InterGen(tiny_cfg())
    elif name == "MDM":
        m = MDM(tiny_cfg(NAME="MDM", CFG_WEIGHT=2.5), num_frames=64, sampling_strategy="ddim4")
    else:
        m = in2IN(tiny_cfg(NAME="in2IN"), name)
    sd = {}
    for k, p in m.state_dict().items():
        sd[k] = torch.randn(p.shape, generator=gen) * (0.05 if p.dim() == 2 else 0.02) + (1.0 if k.endswith(("norm1.weight", "norm2.weight")) else 0.0)
    m.load_state_dict(sd)
    dec = m if name == "MDM" else m.decoder
    dec.num_frames = 64
    m = m.to("cuda")
    Wd = 262 if name in ("MDM", "individual") else 524
    conds = {"InterGen": ("cond",), "MDM": ("cond",), "individual": ("cond_individual_individual1",),
             "interaction": ("cond_interaction", "cond_interaction_individual1", "cond_interaction_individual2"),
             "dual": ("cond_interaction", "cond_interaction_individual1", "cond_interaction_individual2", "cond_individual_individual1",
                      "cond_individual_individual2")}[name]
    cw = 128 if name == "MDM" else 768

    def batch(i, nb, T):
        b = {k: rnd(1000 + 10 * i + j, nb, cw).cuda() for j, k in enumerate(conds)}
        b["motions"] = 0.5 * rnd(1100 + i, nb, T, Wd).cuda()
        return b
    return m, batch


@pytest.mark.parametrize("name", ["InterGen", "interaction", "dual", "individual", "MDM"])
def test_facades_invert_many_ragged_equals_sequential(name):
    m, batch = facade(name)
    batches = [batch(i, nb, T) for i, (nb, T) in enumerate([(2, 12), (1, 33), (3, 20)])]
    one = m.invert(dict(batches[0]))
    assert set(one) == {"latent", "steps"} and one["steps"] == 4 and one["latent"].shape == batches[0]["motions"].shape
    for steps in (None, 3):
        a = m.invert_many([dict(b) for b in batches], batching="sequential", steps=steps)
        r = m.invert_many([dict(b) for b in batches], batching="ragged", steps=steps)
        for x, y, bt in zip(a, r, batches):
            assert x["steps"] == y["steps"] == (steps or 4) and x["latent"].shape == bt["motions"].shape
            assert torch.equal(x["latent"], y["latent"]) and torch.isfinite(x["latent"]).all() and not torch.equal(x["latent"], bt["motions"])
        if steps is None:
            assert torch.equal(a[0]["latent"], one["latent"])
    # forward(start_step=) reaches the sampler: the last step index is the plain loop, an earlier one is not
    b0 = dict(batches[0], motion_lens=torch.tensor([12, 12]), x_T=batches[0]["motions"])
    fw = m.forward if name in ("InterGen", "MDM") else m.decoder.forward
    plain = fw(dict(b0))["output"]
    assert torch.equal(fw(dict(b0), start_step=3)["output"], plain) and not torch.equal(fw(dict(b0), start_step=1)["output"], plain)
    with pytest.raises(ValueError, match=r"steps=5 outside \[1, 4\]"):
        m.invert(dict(batches[0]), steps=5)


# ---------------------------------------------------------------------------------------------------
# 5. refusals, each by its message
# ---------------------------------------------------------------------------------------------------
def refused(match, fn, status):
    from mixermdm_amd._lib import MMDMError
    with pytest.raises(MMDMError, match=match) as e:
        fn()
    assert e.value.status == status


def test_refusals(golden):
    from test_gpu_ragged import small
    from test_gpu_in2in_opts import golden_sampler
    two = small(max_batch=2, max_frames=16)
    try:
        two.set_schedule("ddim4")
        refused(r"begin_reverse: the two-chain MixerMDM sampler \(single_only = 0\) has no reverse step",
                lambda: two.begin_reverse(rnd(1, 1, 8 * 768).cuda(), rnd(2, 1, 8, 524).cuda()), UNSUPPORTED)
    finally:
        two.close()
    for form in (1, 2):
        old, g, t = golden_sampler(golden, form, True)
        try:
            old.set_schedule("ddim4")
            if form == 2:
                old.set_dual_weights("const", 0.3)
            refused(rf"begin_reverse: single_only = {form + 1} is superseded by single_only = 4 with cfg_form = {form}",
                    lambda: old.begin_reverse(t("cond").cuda(), t("x_T").cuda()), UNSUPPORTED)
            refused(rf"begin_reverse_ragged: single_only = {form + 1} is superseded",
                    lambda: old.begin_reverse_ragged(t("cond").cuda(), [t("x_T")[0].cuda(), t("x_T")[1].cuda()], [12, 12]), UNSUPPORTED)
            assert old.sample(t("cond").cuda(), t("x_T").cuda()).shape == (2, 12, 524)          # the handle is as it was
        finally:
            old.close()
    s = synth("individual", "fp32", 2)
    try:
        cond, xs = synth_inputs("individual", (12, 12))
        x = torch.stack(xs)
        refused("run_reverse: call begin_reverse / begin_reverse_ragged first", lambda: s.run_reverse(1), STATE)
        s.set_key_mask(torch.ones(2, 12))
        refused("begin_reverse: a key mask is set on the handle", lambda: s.begin_reverse(cond, x), UNSUPPORTED)
        refused("begin_reverse_ragged: a key mask is set on the handle", lambda: s.begin_reverse_ragged(cond, xs, [12, 12]), UNSUPPORTED)
        s.set_key_mask(None)
        want = s.invert(cond, x, steps=2)
        s.set_schedule("ddim4")
        assert torch.equal(s.invert(cond, x, steps=2), want)
        refused(r"run_reverse: 3 reverse steps requested, 2 left in the schedule", lambda: s.run_reverse(3), ARG)
        s.run_reverse(2)
        refused(r"run_reverse: 1 reverse steps requested, 0 left in the schedule", lambda: s.run_reverse(1), ARG)
        for bad in (0, 5):
            with pytest.raises(ValueError, match=rf"steps={bad} outside \[1, 4\]"):
                s.invert(cond, x, steps=bad)
        with pytest.raises(ValueError, match="exclusive with init_image / skip_timesteps"):
            s.sample_from(cond, x, 1, skip_timesteps=1)
        # a forward call after all of it is the forward call
        assert torch.equal(s.sample(cond, x), s.sample(cond, x, use_graph=False))
    finally:
        s.close()
    s = synth("intergen", "fp32", 1)
    try:
        cond, xs = synth_inputs("intergen", (12,))
        s.set_eta(0.5)
        refused("begin_reverse: eta is set on the handle; the reverse ODE is the deterministic path only", lambda: s.begin_reverse(cond, xs[0][None]), STATE)
        s.set_eta(0.0)
        assert torch.isfinite(s.invert(cond, xs[0][None])).all()
    finally:
        s.close()

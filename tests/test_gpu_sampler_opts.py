"""GPU: the two-chain sampler's loop options -- eta > 0 (noise from a caller buffer or from the device generator), init_image / skip_timesteps,
x_start -- against the reference (tests/golden/sampler_opts.npz, captured by tests/golden/make_golden_sampler_opts.py) and against identities
that rest on no tolerance.  Tiny handles built from the existing fixtures' weights (mixer.npz; mixer32.npz for fp32_split); B = 2, T = 20, ddim4."""
import ctypes as C
import numpy as np
import pytest
import torch

from test_sampler_opts_cpu import step_normal_f64

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1          # both key words non-zero
LOOP_BOUND = dict(mean=2e-3, p99=3e-2)  # the project's loop bound (tests/test_gpu_mask.py, tests/test_gpu_facade.py)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


class Case:
    """Inputs of the fixture (seeds) and a tiny fp32 sampler, built once for the module."""

    def __init__(self, golden):
        from mixermdm_amd.sampler import Sampler
        self.g = g = golden("sampler_opts")[0]
        gm, w, _ = golden("mixer")
        self.B, self.T, self.S = int(g["B"]), int(g["T"]), 4
        sx, sc, ss, si, sn = [int(v) for v in g["seeds"]]
        B, T = self.B, self.T
        self.x_T, self.cond = rnd(sx, B, T, 524).cuda(), rnd(sc, B, 8 * 768).cuda()
        self.x_start, self.init = rnd(ss, B, int(g["x_start_frames"]), 524).cuda(), (0.5 * rnd(si, B, T, 524)).cuda()
        self.noise = torch.stack([rnd(sn + k, B, T, 524) for k in range(self.S)]).cuda()
        s = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=int(gm["d_heads"]), m_latent=16, m_ff=32, m_layers=2, m_heads=int(gm["m_heads"]), mixing_mode=4,
                    align=True, cfg_scale=float(g["cfg_scale"]), max_batch=3, max_frames=40)
        s.load_state_dict(w("mix."))
        s.set_norm_stats(gm["mean_hml"], gm["std_hml"], gm["mean_ih"], gm["std_ih"])
        s.prepare()
        s.set_schedule(str(g["strategy"]))
        assert s.schedule.num_timesteps == self.S
        self.s = s
        self.plain = s.sample(self.cond, self.x_T, use_graph=False)

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
    c = Case(golden)
    yield c
    c.s.close()


def sampler_of(golden, prec):
    """(sampler, cond, x_T) of a precision mode: the fixture's tiny model in fp32, mixer32.npz's sizes (the smallest the 16-bit GEMMs take) otherwise."""
    from mixermdm_amd.sampler import Sampler
    g, w, t = golden("mixer32")
    s = Sampler(d_latent=32, d_ff=64, d_layers=2, d_heads=2, m_latent=32, m_ff=64, m_layers=2, m_heads=2, cfg_scale=3.5, max_batch=2, max_frames=16, precision=prec)
    s.load_state_dict(w("mix."))
    s.set_norm_stats(g["mean_hml"], g["std_hml"], g["mean_ih"], g["std_ih"])
    s.prepare()
    s.set_schedule("ddim4")
    return s, t("cfg_cond").cuda(), t("x_T").cuda()


# ---------------------------------------------------------------------------------------------------
# 1. the generator
# ---------------------------------------------------------------------------------------------------
def test_generator_matches_its_definition_and_is_independent_of_batch_and_length():
    """ops.randn against a float64 numpy evaluation of the same formula from the same integer draws, atol 1e-5: the fp32 argument 2 pi u2 is off by
    <= 4e-7 (+ 2e-7 from rounding k + 0.5 at k >= 2^23) and the radius is <= 5.9 (u1 = 2^-25), so the cosine factor contributes <= 3.6e-6; the
    radius itself is computed from an exactly represented u1 (or 1 - u1) with the accurate logf / log1pf, a few 1e-7 relative."""
    from mixermdm_amd import ops
    z33 = ops.randn(SEED, 2, 3, 33)
    ref = step_normal_f64(SEED, 2, 3, 33)
    err = np.abs(z33.cpu().numpy().astype(np.float64) - ref)
    print("generator: max |fp32 - float64| = %.3e (mean %.3e, std %.3f)" % (err.max(), ref.mean(), ref.std()))
    assert torch.isfinite(z33).all() and err.max() <= 1e-5
    z2 = ops.randn(SEED, 2, 2, 33)
    assert torch.equal(z33[:2], z2)                                  # item b of a B = 3 call == item b of a B = 2 call
    assert torch.equal(ops.randn(SEED, 2, 3, 20), z33[:, :20])       # T = 20 == the first 20 frames of T = 33
    assert not torch.equal(ops.randn(SEED + 1, 2, 3, 33), z33)
    assert not torch.equal(ops.randn(SEED, 3, 3, 33), z33)
    assert not torch.equal(ops.randn(SEED ^ (1 << 40), 2, 3, 33), z33)   # the high key word counts


# ---------------------------------------------------------------------------------------------------
# 2. every fixture case against the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pin", "init", "init0", "skip", "eta", "all"])
def test_case_vs_reference_golden(case, name):
    out = case.s.sample(case.cond, case.x_T, use_graph=False, **case.kwargs(name))
    d = np.abs(out.cpu().numpy() - case.g[f"{name}:output"])
    print("%s: mean err %.3e, p99 %.3e, max %.3e" % (name, d.mean(), np.percentile(d, 99), d.max()))
    assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (d.mean(), np.percentile(d, 99), d.max())
    assert float((out - case.plain).abs().mean()) > 0.05             # and it is not the plain loop
    dp = np.abs(case.plain.cpu().numpy() - case.g["plain:output"])
    assert dp.mean() <= LOOP_BOUND["mean"] and np.percentile(dp, 99) <= LOOP_BOUND["p99"]


# ---------------------------------------------------------------------------------------------------
# 3. identities
# ---------------------------------------------------------------------------------------------------
COLS = [0, 2, 262, 264]


def test_pinned_loop_is_the_manual_loop_bitwise(case):
    s = case.s
    s.set_eta(0.0)
    out = s.sample(case.cond, case.x_T, use_graph=False, x_start=case.x_start)
    left = {k: v.clone() for k, v in s.state().items() if k in ("x", "x2", "pred_xstart")}
    s.begin(case.cond, case.x_T)
    for _ in range(case.S):
        st = s.state()
        for k in ("x", "x2"):
            st[k][:, :, COLS] = case.x_start[:, :case.T, COLS]
        torch.cuda.synchronize()
        s.run(1, use_graph=False)
    st = s.state()
    assert torch.equal(st["pred_xstart2"], out)
    for k in left:
        assert torch.equal(st[k], left[k]), k
    assert not torch.equal(st["x"][:, :, COLS], case.x_start[:, :case.T, COLS])          # the sample the last step leaves is not pinned
    assert not torch.equal(st["pred_xstart2"][:, :, COLS], case.x_start[:, :case.T, COLS])


@pytest.mark.parametrize("skip, with_init", [(1, True), (0, True), (2, False)])
def test_init_image_start_and_the_loop_from_there(case, skip, with_init):
    s, S = case.s, case.S
    s.set_eta(0.0)
    init = case.init if with_init else None
    s.begin(case.cond, case.x_T, init_image=init, skip_timesteps=skip)
    st = s.state()
    x0, x20 = st["x"].clone(), st["x2"].clone()
    i0 = S - 1 - skip
    a, b = np.sqrt(s.schedule.alphas_cumprod[i0]), np.sqrt(1.0 - s.schedule.alphas_cumprod[i0])
    want = a * (case.init.double() if with_init else 0.0) + b * case.x_T.double()
    assert torch.equal(x0, x20)
    assert torch.allclose(x0.double(), want, rtol=1e-6, atol=1e-6), float((x0.double() - want).abs().max())
    hist = s.set_history(("out1",))
    assert hist["out1"].shape[0] == S - skip                          # one entry per executed step
    s.run(None, use_graph=False)
    out = s.state()["pred_xstart2"].clone()
    s.begin(case.cond, x0)
    s.seek(i0)
    s.run(None, use_graph=False)
    assert torch.equal(s.state()["pred_xstart2"], out)


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


@pytest.mark.parametrize("prec", ["fp32", "fp32_split"])
def test_no_noise_at_the_last_step_and_one_eta_step_vs_float64(case, golden, prec):
    """(a) Two noise buffers that differ in the last slot only leave bitwise equal chains.  (b) One eta = 1 step at i = S - 1 against the float64
    formula from that step's own x and pred_xstart: within 3 x the error the eta = 0 update shows against float64 on the same step (floor 1e-6;
    the margin: one added term and two roundings)."""
    if prec == "fp32":
        s, cond, x_T = case.s, case.cond, case.x_T
    else:
        s, cond, x_T = sampler_of(golden, prec)
    B, T = x_T.shape[:2]
    S = s.schedule.num_timesteps
    noise = torch.stack([rnd(900 + k, B, T, 524) for k in range(S)]).cuda()
    other = noise.clone()
    other[S - 1] = rnd(999, B, T, 524).cuda()
    fin = []
    for buf in (noise, other):
        s.sample(cond, x_T, use_graph=False, eta=1.0, noise=buf)
        st = s.state()
        fin.append((st["x"].clone(), st["x2"].clone()))
    assert torch.equal(fin[0][0], fin[1][0]) and torch.equal(fin[0][1], fin[1][1])
    # (b)
    i = S - 1
    co = s.schedule.device_coefficients().astype(np.float64)
    et = s.schedule.eta_coefficients(1.0).astype(np.float64)
    assert et[1][i] > 0.1

    def f64(x, x0, c3, sigma):
        eps = (co[0][i] * x.double() - x0.double()) / co[1][i]
        return x0.double() * co[2][i] + c3 * eps + sigma * noise[0].double()

    s.set_eta(0.0)
    s.begin(cond, x_T)
    s.run(1, use_graph=False)
    st = {k: v.clone() for k, v in s.state().items() if v is not None}
    err0 = max(float((st["x"].double() - f64(x_T, st["pred_xstart"], co[3][i], 0.0)).abs().max()),
               float((st["x2"].double() - f64(x_T, st["pred_xstart2"], co[3][i], 0.0)).abs().max()))
    s.set_eta(1.0)
    s.begin(cond, x_T, noise=noise)
    s.run(1, use_graph=False)
    se = s.state()
    assert torch.equal(se["pred_xstart"], st["pred_xstart"]) and torch.equal(se["pred_xstart2"], st["pred_xstart2"])
    err1 = max(float((se["x"].double() - f64(x_T, se["pred_xstart"], et[0][i], et[1][i])).abs().max()),
               float((se["x2"].double() - f64(x_T, se["pred_xstart2"], et[0][i], et[1][i])).abs().max()))
    print("%s: eta = 0 update vs float64 %.3e, eta = 1 update %.3e" % (prec, err0, err1))
    assert err1 <= max(3 * err0, 1e-6), (err0, err1)
    assert float((se["x"] - st["x"]).abs().mean()) > 0.05
    s.set_eta(0.0)
    if prec != "fp32":
        s.close()


# ---------------------------------------------------------------------------------------------------
# 4. graphs
# ---------------------------------------------------------------------------------------------------
def test_graph_replay_of_option_calls(case):
    """`all` replayed == eager bitwise; other option VALUES replay the same graph; the plain call before and after is unchanged; a zeroed
    mmdm_begin_options is mmdm_begin."""
    from mixermdm_amd._lib import BeginOptions, check
    s = case.s
    cap0 = s.graph_stats()[0]
    s.set_eta(0.0)
    plain_g = s.sample(case.cond, case.x_T, use_graph=True)
    assert torch.equal(plain_g, case.plain)
    cap1 = s.graph_stats()[0]
    kw = case.kwargs("all")
    eager = s.sample(case.cond, case.x_T, use_graph=False, **kw)
    graph = s.sample(case.cond, case.x_T, use_graph=True, **kw)
    assert torch.equal(eager, graph)
    cap2 = s.graph_stats()[0]
    assert cap2 == cap1 + 1 and cap1 <= cap0 + 1
    kw2 = dict(kw, noise=torch.stack([rnd(700 + k, case.B, case.T, 524) for k in range(case.S - 1)]).cuda(),
               x_start=rnd(710, case.B, case.T, 524).cuda(), init_image=rnd(711, case.B, case.T, 524).cuda())
    graph2 = s.sample(case.cond, case.x_T, use_graph=True, **kw2)
    assert s.graph_stats()[0] == cap2                                  # new values, same graph
    assert torch.equal(graph2, s.sample(case.cond, case.x_T, use_graph=False, **kw2)) and not torch.equal(graph2, graph)
    # seed form and the un-pinned form are other entries, never the buffer form's replay
    sg = s.sample(case.cond, case.x_T, use_graph=True, eta=1.0, seed=SEED)
    assert s.graph_stats()[0] == cap2 + 1
    assert torch.equal(sg, s.sample(case.cond, case.x_T, use_graph=False, eta=1.0, seed=SEED))
    s.set_eta(0.0)
    assert torch.equal(s.sample(case.cond, case.x_T, use_graph=True), case.plain) and s.graph_stats()[0] == cap2 + 1
    # defaults
    o = BeginOptions()
    with torch.cuda.device(s.device):
        check(s.lib.mmdm_begin_opts(s.h, C.c_void_p(case.cond.data_ptr()), C.c_void_p(case.x_T.data_ptr()), case.B, case.T, C.byref(o), s._s()), s.h)
        check(s.lib.mmdm_run(s.h, case.S, 1, s._s()), s.h)
    assert torch.equal(s.state()["pred_xstart2"], case.plain) and s.graph_stats()[0] == cap2 + 1


def test_options_compose_with_a_key_mask(case):
    """A key mask changes the attention only: the masked `all` call differs from the unmasked one, replays bitwise, and a mask of all-valid frames
    is the unmasked call."""
    s = case.s
    kw = case.kwargs("all")
    base = s.sample(case.cond, case.x_T, use_graph=False, **kw)
    valid = torch.ones(case.B, case.T, dtype=torch.bool)
    valid[1, case.T - 7:] = False
    s.set_key_mask(valid)
    m_e = s.sample(case.cond, case.x_T, use_graph=False, **kw)
    m_g = s.sample(case.cond, case.x_T, use_graph=True, **kw)
    s.set_key_mask(torch.ones(case.B, case.T, dtype=torch.bool))
    full = s.sample(case.cond, case.x_T, use_graph=False, **kw)
    s.set_key_mask(None)
    s.set_eta(0.0)
    assert torch.equal(m_e, m_g) and not torch.equal(m_e, base) and torch.equal(full, base)


# ---------------------------------------------------------------------------------------------------
# 5. refusals, each by its message
# ---------------------------------------------------------------------------------------------------
def test_refusals(case, golden):
    from mixermdm_amd._lib import MMDMError, check
    from mixermdm_amd.sampler import Sampler
    s, S = case.s, case.S
    ARG, STATE, UNSUPPORTED = 1, 2, 4            # mmdm_status (include/mmdm.h)

    def refused(match, fn, status=None):
        with pytest.raises(MMDMError, match=match) as e:
            fn()
        if status is not None:
            assert e.value.status == status
        return e.value.status

    s.set_eta(0.5)
    refused("names no noise source", lambda: s.begin(case.cond, case.x_T), STATE)
    refused("names no noise source", lambda: s.begin(case.cond, case.x_T, x_start=case.x_start), STATE)
    refused("eta is set on the handle; the stochastic update covers uniform batches",
            lambda: s.begin_ragged(case.cond, case.x_T.reshape(-1, 524), [case.T] * case.B), UNSUPPORTED)
    refused("the noise buffer holds 3 steps, 4 are left", lambda: s.begin(case.cond, case.x_T, noise=case.noise[:3]), ARG)
    s.begin(case.cond, case.x_T, noise=case.noise[:3], skip_timesteps=1)           # 3 slots are enough for 3 steps ...
    s.seek(1)
    refused("run past the call's noise buffer", lambda: s.run(2), ARG)           # ... and loop positions 2, 3 are not among them
    s.set_eta(0.0)
    refused("a noise source is given and no eta table is set", lambda: s.begin(case.cond, case.x_T, seed=1), STATE)
    refused(r"x_start has 10 frames, the call has T=20", lambda: s.begin(case.cond, case.x_T, x_start=case.x_start[:, :10]), ARG)
    refused(r"skip_timesteps=4 outside \[0, 4\)", lambda: s.begin(case.cond, case.x_T, skip_timesteps=S), ARG)
    assert torch.equal(s.sample(case.cond, case.x_T, use_graph=False), case.plain)   # the handle is as it was
    # single-chain samplers
    for so in (1, 2, 3):
        k = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=2, single_only=so, max_batch=1, max_frames=16)
        refused("eta > 0 covers the two-chain MixerMDM sampler", lambda: check(k.lib.mmdm_set_eta(k.h, None, 0), k.h), UNSUPPORTED)
        k.close()
    g, w, t = golden("single")
    k = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=int(g["H"]), single_only=True, cfg_scale=float(g["cfg_scale"]), max_batch=2, max_frames=16)
    k.load_state_dict({"denoiser1." + n: v for n, v in w("ind.").items()})
    k.prepare()
    k.set_schedule("ddim4")
    refused("cover the two-chain MixerMDM sampler", lambda: k.begin(t("cond"), t("x_T"), skip_timesteps=1), UNSUPPORTED)
    k.close()


# ---------------------------------------------------------------------------------------------------
# 6. the facade
# ---------------------------------------------------------------------------------------------------
def test_facade_loop_takes_the_options(tmp_path, golden, case):
    from test_gpu_facade import tiny_model
    from mixermdm_amd.models import MixerDiffusion, ClassifierFreeSampleModelX2
    from mixermdm_amd.schedule import space_timesteps
    m, _, _ = tiny_model(tmp_path, golden, strategy="ddim4")
    diff = MixerDiffusion(use_timesteps=space_timesteps(1000, "ddim4"), betas=m.betas)
    cfg = ClassifierFreeSampleModelX2(m.mixing, 3.5)
    m.mixing.store_influence, m.mixing.mode = True, "eval_intermediate"
    shape = (case.B, case.T, 524)
    mk = {"mask": None, "cond": case.cond}
    out = diff.ddim_sample_loop(cfg, shape, noise=case.x_T, clip_denoised=False, model_kwargs=mk, eta=1.0, step_noise=case.noise[:3],
                                x_start=case.x_start, init_image=case.init, skip_timesteps=1)
    d = np.abs(out.cpu().numpy() - case.g["all:output"])
    print("facade all: mean err %.3e, p99 %.3e" % (d.mean(), np.percentile(d, 99)))
    assert d.mean() <= LOOP_BOUND["mean"] and np.percentile(d, 99) <= LOOP_BOUND["p99"], (d.mean(), d.max())
    assert len(m.mixing.history_influence_i1) == 3                     # S - skip entries
    # eta > 0 with no noise named: the seed comes from torch's default generator
    torch.manual_seed(5)
    a = diff.ddim_sample_loop(cfg, shape, noise=case.x_T, clip_denoised=False, model_kwargs=mk, eta=0.5)
    torch.manual_seed(5)
    b = diff.ddim_sample_loop(cfg, shape, noise=case.x_T, clip_denoised=False, model_kwargs=mk, eta=0.5)
    c = diff.ddim_sample_loop(cfg, shape, noise=case.x_T, clip_denoised=False, model_kwargs=mk, eta=0.5)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # and the plain call afterwards is the plain loop
    p = diff.ddim_sample_loop(cfg, shape, noise=case.x_T, clip_denoised=False, model_kwargs=mk)
    dp = np.abs(p.cpu().numpy() - case.g["plain:output"])
    assert dp.mean() <= LOOP_BOUND["mean"] and np.percentile(dp, 99) <= LOOP_BOUND["p99"]
    with pytest.raises(NotImplementedError):
        diff.ddim_sample_loop(cfg, shape, noise=case.x_T, clip_denoised=True, model_kwargs=mk, eta=0.5)

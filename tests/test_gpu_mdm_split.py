"""GPU: MDMDenoiser as MODEL1 (model1_kind = 1) in the fp32_split precision mode -- the post-norm encoder on split operands.

fp32_split is the mode that keeps the fp32 tolerances, so everything here is held either to the oracle at the tolerances of the fp32 tests it twins
(tests/test_gpu_extensions.py, tests/test_gpu_sampler.py::STEP_TOL) or bitwise: the new row kernels against the kernels they extend, ragged batches
against the stand-alone calls of the same handle, graph replay against the eager run."""
import ctypes as C
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from oracle import mixer as MX            # noqa: E402  (checker only)
from oracle import encoder as EN          # noqa: E402
from oracle import schedule as OS         # noqa: E402
from oracle.layers import pe_table        # noqa: E402
from parity_tol import STEP_TOL           # noqa: E402
from test_gpu_kernels import assert_close, rnd   # noqa: E402
from test_gpu_extensions import enc_weights      # noqa: E402

NO_ZERO_KEY, CAUSAL = 1, 2
# denoiser 2 and Influence as in tests/test_gpu_ragged_mdm.py (head size 64 everywhere); denoiser 1 = MDM, 128 / 2 heads, two layers
DIMS = dict(d_latent=128, d_ff=256, d_layers=2, m_latent=128, m_ff=256, m_layers=2)
CW = 6 * 768 + 2 * 128


# ---------------------------------------------------------------------------------------------------
# 1. creation
# ---------------------------------------------------------------------------------------------------
def chain_weights(D, Fd, L):
    """The stand-alone MDMDenoiser of tests/test_gpu_extensions.py::test_standalone_mdm_chain_vs_oracle (same seeds)."""
    W = {"input_process.poseEmbedding.weight": rnd(1, D, 262) * 0.05, "input_process.poseEmbedding.bias": rnd(2, D) * 0.05,
         "output_process.poseFinal.weight": rnd(3, 262, D) * 0.05, "output_process.poseFinal.bias": rnd(4, 262) * 0.05}
    for k in ("0", "2"):
        W[f"embed_timestep.time_embed.{k}.weight"], W[f"embed_timestep.time_embed.{k}.bias"] = rnd(5 + int(k), D, D) * 0.05, rnd(8 + int(k), D) * 0.05
    for i in range(L):
        for k, v in enc_weights(50 + 20 * i, D, Fd).items():
            W[f"seqTransEncoder.layers.{i}.{k}"] = v
    return W


def chain_sampler(W, precision, D, Fd, L, H, B, T):
    from mixermdm_amd.sampler import Sampler
    s = Sampler(d_latent=D, d_ff=Fd, d_layers=L, d_heads=H, single_only=1, model1_kind=1, cfg_scale=2.5, max_batch=B, max_frames=T, precision=precision)
    s.load_state_dict({"denoiser1." + k: v for k, v in W.items()})
    s.prepare()
    return s


def test_split_mdm_handle_is_created_and_the_other_modes_are_refused_by_name():
    from mixermdm_amd._lib import MMDMError
    from mixermdm_amd.sampler import Sampler
    D, Fd, L, H = 128, 256, 2, 2
    s = chain_sampler(chain_weights(D, Fd, L), "fp32_split", D, Fd, L, H, 2, 40)
    s.set_schedule("ddim20")
    s.close()
    for prec in ("bf16", "bf16_fp8"):
        with pytest.raises(MMDMError, match=prec + r".*fp32_split \(2\) and fp32 \(0\) are the modes that cover MDM") as e:
            Sampler(d_latent=D, d_ff=Fd, d_layers=L, d_heads=H, single_only=1, model1_kind=1, max_batch=2, max_frames=40, precision=prec)
        assert e.value.status == 4
    # the two-chain sampler refuses them the same way
    with pytest.raises(MMDMError, match="modes that cover MDM"):
        Sampler(d_heads=2, m_heads=2, model1_kind=1, d1_latent=128, d1_ff=256, d1_layers=2, d1_heads=2, max_batch=2, max_frames=20, precision="bf16", **DIMS)
    # head size 8 (d1 = 16 / 2 heads): the two-plane attention covers 64 and 128
    with pytest.raises(MMDMError, match="head size 8") as e:
        Sampler(d_heads=2, m_heads=2, model1_kind=1, d1_latent=16, d1_ff=32, d1_layers=2, d1_heads=2, max_batch=2, max_frames=20, precision="fp32_split", **DIMS)
    assert e.value.status == 4
    with pytest.raises(MMDMError, match="head size 8"):
        Sampler(d_latent=32, d_ff=64, d_layers=2, d_heads=4, single_only=1, model1_kind=1, max_batch=2, max_frames=20, precision="fp32_split")


# ---------------------------------------------------------------------------------------------------
# 2. the row kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 256, 1024])
@pytest.mark.parametrize("rows", [1, 41, 2 * 41 + 3])
def test_layernorm_split_is_the_layernorm_and_its_split_bitwise(rows, D):
    """mmdm_layernorm_split in both builds of the row kernels: fp32 rows bitwise the plain LayerNorm of the same build (build 0: mmdm_layernorm_f32),
    planes bitwise ops.split_f32 of them.  Rows: random, all zeros, inputs near 6e4, and a one-hot row whose OUTPUT is near 6e4 (gamma[3] sized for
    it; the split format covers |y| < 65504); 85 rows leave a partial last workgroup of four wave slots."""
    from mixermdm_amd import ops
    x = rnd(1, rows, D) * 3 + 0.5
    g, b = rnd(2, D), rnd(3, D)
    g[3], b[3] = 6.0e4 / float(np.sqrt(D - 1)), 0.0
    if rows >= 41:
        x[5] = 0.0
        x[6] = (5.9e4 + 1.0e3 * torch.rand(D, generator=torch.Generator().manual_seed(4))) * torch.sign(rnd(5, D))
        x[7] = 0.0
        x[7, 3] = 1.0
    else:
        x[0] = 0.0
        x[0, 3] = 1.0
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    for build in (0, 1):
        ref, none = ops.layernorm_split(xd, gd, bd, 1e-5, build=build, planes=False)
        assert none is None
        out, pl = ops.layernorm_split(xd, gd, bd, 1e-5, build=build)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.isfinite(pl.float()).all()
        assert torch.equal(out, ref), (build, (out - ref).abs().max().item())
        assert torch.equal(pl, ops.split_f32(ref)), build
        if build == 0:
            assert torch.equal(ref, ops.layernorm(xd, gd, bd, 1e-5))
        # the planes carry the row to 2^-22 relative
        back = pl[0].double() + pl[1].double() / 2048.0
        assert ((back - out.double()).abs() <= 2.0 ** -21 * out.double().abs() + 2.0 ** -35).all()
    assert out.abs().max().item() > 5.0e4          # the large output is really there
    # in place
    y = xd.clone()
    pl2 = torch.empty(2, rows, D, device="cuda", dtype=torch.float16)
    from mixermdm_amd._lib import load_library, check
    p = lambda t: C.c_void_p(t.data_ptr())
    check(load_library().mmdm_layernorm_split(p(y), p(gd), p(bd), p(y), p(pl2), rows * D, rows, D, 1e-5, 1, None))
    torch.cuda.synchronize()
    assert torch.equal(y, out) and torch.equal(pl2, pl)


# ---------------------------------------------------------------------------------------------------
# 3. the stand-alone chain against the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,T", [(128, 2, 40), (128, 2, 15), (128, 2, 16), (128, 2, 17), (256, 2, 40)])
def test_standalone_mdm_chain_split_vs_oracle(D, H, T):
    """The split twin of test_standalone_mdm_chain_vs_oracle: same construction, seeds and tolerances (atol = rtol = 1e-4 against the fp32 oracle).
    T = 15 / 16 / 17 put 16 / 17 / 18 keys around the 16-key chunk; (256, 2) is head size 128.  The fp32 handle runs the same inputs and both modes'
    maximum error against a float64 run of the oracle is printed (DESIGN section 7 records the figures; the ratio is reported, not gated)."""
    Fd, L, B = 256, 2, 2
    W = chain_weights(D, Fd, L)
    cond, xT = rnd(70, B, D), rnd(71, B, T, 262)
    Wo = dict(W)
    Wo["sequence_pos_encoder.pe"] = pe_table(D)
    osch = OS.make_schedule("cosine", 1000, "ddim20")
    ts = torch.full((2 * B,), osch.timestep_map[19], dtype=torch.long)

    def oracle(dt):
        Wd = {k: v.to(dt) for k, v in Wo.items()}
        o = EN.mdm_denoiser(Wd, "", torch.cat([xT, xT]).to(dt), ts, torch.cat([cond, torch.zeros_like(cond)]).to(dt), H)
        x0 = 2.5 * o[:B] + (1 - 2.5) * o[B:]
        return x0, MX.ddim_update(osch, 19, xT.to(dt), x0)
    x0, x1 = oracle(torch.float32)
    x0_64, x1_64 = oracle(torch.float64)
    err = {}
    for prec in ("fp32_split", "fp32"):
        s = chain_sampler(W, prec, D, Fd, L, H, B, T)
        s.set_schedule("ddim20")
        s.begin(cond, xT)
        s.run(1, use_graph=True)
        st = {k: v.cpu().clone() for k, v in s.state().items() if v is not None}
        s.begin(cond, xT)
        s.run(1, use_graph=False)
        eager = s.state()
        assert torch.equal(eager["x"].cpu(), st["x"]) and torch.equal(eager["pred_xstart"].cpu(), st["pred_xstart"]), prec
        s.close()
        err[prec] = max((st["pred_xstart"].double() - x0_64).abs().max().item(), (st["x"].double() - x1_64).abs().max().item())
        if prec == "fp32_split":
            assert_close(st["pred_xstart"], x0, atol=1e-4, rtol=1e-4, what="MDM cfg x0 [fp32_split]")
            assert_close(st["x"], x1, atol=1e-4, rtol=1e-4, what="MDM ddim x [fp32_split]")
    e_or = max((x0.double() - x0_64).abs().max().item(), (x1.double() - x1_64).abs().max().item())
    print(f"\nMDM chain D={D} H={H} T={T}: max |err| vs the float64 oracle: fp32_split {err['fp32_split']:.3e}, fp32 {err['fp32']:.3e} "
          f"(ratio {err['fp32_split'] / err['fp32']:.2f}); the fp32 CPU oracle itself {e_or:.3e}")


# ---------------------------------------------------------------------------------------------------
# 4. the Mixer with MDM as MODEL1
# ---------------------------------------------------------------------------------------------------
def mixer_sd(single_only=False):
    from mixermdm_amd.synthetic import synthetic_state_dict
    return synthetic_state_dict(seed=7, std=0.05, bias_std=0.02, mixing_mode=4, model1="MDM", single_only=bool(single_only), d1_latent=128, d1_ff=256, d1_layers=2, **DIMS)


def small(max_batch=4, max_frames=40, single_only=False, precision="fp32_split"):
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_stats
    s = Sampler(d_heads=2, m_heads=2, max_batch=max_batch, max_frames=max_frames, mixing_mode=4, single_only=single_only, model1_kind=1,
                d1_latent=128, d1_ff=256, d1_layers=2, d1_heads=2, precision=precision, **DIMS)
    s.load_state_dict(mixer_sd(single_only))
    if not single_only:
        st = synthetic_stats()
        s.set_norm_stats(st["mean_hml"], st["std_hml"], st["mean_ih"], st["std_ih"])
    s.prepare()
    s.set_schedule("ddim20")
    return s


def test_mixer_with_mdm_split_vs_oracle():
    """Both denoisers at head size 64, Influence at 128 / 2 heads, B = 2, T = 20: Mixer.forward on a CFG-doubled batch against the CPU oracle at STEP_TOL,
    a 4-step ddim20 loop at the loop bounds of test_mixer_with_mdm_vs_reference_golden, graph replay == eager bitwise."""
    from mixermdm_amd.synthetic import synthetic_stats
    B, T = 2, 20
    s = small(max_batch=B, max_frames=T)
    sd, st = mixer_sd(), synthetic_stats()
    W = dict(sd)
    for k in ("sequence_pos_encoder.pe", "denoiser1.sequence_pos_encoder.pe", "denoiser2.sequence_pos_encoder.pe"):
        W[k] = pe_table(128)
    ostats = tuple(torch.as_tensor(np.asarray(st[k]), dtype=torch.float32) for k in ("mean_hml", "std_hml", "mean_ih", "std_ih"))
    spec = MX.MixerSpec(d_heads=2, m_heads=2, mixing_mode=4, d1_text_dim=128, model1="MDM")
    osch = OS.make_schedule("cosine", 1000, "ddim20")
    g = torch.Generator().manual_seed(31)
    cond = torch.randn(B, CW, generator=g)
    x1, x2 = torch.randn(2 * B, T, 524, generator=g), torch.randn(2 * B, T, 524, generator=g)
    cc = torch.cat([cond, torch.zeros_like(cond)])
    t = int(osch.timestep_map[12])
    out = s.module_forward(2, x1, cc, t, x2=x2)
    ref = MX.mixer_forward(W, spec, ostats, x1, torch.full((2 * B,), t, dtype=torch.long), cc, x2)
    assert_close(out, ref, what="Mixer.forward (MDM as model1) [fp32_split]", **STEP_TOL)
    # 4 steps of the loop
    s.set_schedule("ddim20")
    xT = torch.randn(B, T, 524, generator=g)
    p2, rx, rx2 = MX.mixer_ddim_loop(W, spec, ostats, osch, 3.5, xT, cond, first_steps=4)
    runs = {}
    for graph in (False, True):
        s.begin(cond, xT)
        s.run(4, use_graph=graph)
        runs[graph] = {k: v.cpu().clone() for k, v in s.state().items() if v is not None}
        for name, r in (("pred_xstart2", p2), ("x", rx), ("x2", rx2)):
            d = np.abs(runs[graph][name].numpy() - r.numpy())
            assert np.isfinite(runs[graph][name].numpy()).all()
            assert d.mean() <= 2e-3 and np.percentile(d, 99) <= 3e-2, (name, graph, d.mean(), d.max())
    for k in runs[False]:
        assert torch.equal(runs[False][k], runs[True][k]), k
    s.close()


# ---------------------------------------------------------------------------------------------------
# 5. ragged batches
# ---------------------------------------------------------------------------------------------------
def inputs(lens, width=524, cw=CW, seed=0):
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(len(lens), cw, generator=g)
    xs = [torch.randn(t, width, generator=g) for t in lens]
    return cond, xs


LENS_SETS = ((8, 20), (1, 16, 33), (17, 17))


@pytest.mark.parametrize("single_only", [1, 0])
def test_ragged_split_mdm_items_equal_their_stand_alone_calls(single_only):
    """Every item of a ragged batch is bitwise its stand-alone uniform call on the same handle: (8, 20), (1, 16, 33) -- 2 / 17 / 34 tokens around the
    16-key chunk and the 16-query wave -- and (17, 17); every group here has padding rows (28 .. 50 frames and 30 .. 53 tokens in a 128-row bucket).
    Graph replay against the eager run, and a handle that shares the weights (mmdm_create_shared)."""
    s = small(max_batch=4, max_frames=40, single_only=single_only)
    width, cw = (262, 128) if single_only else (524, CW)
    sh = s.share()
    sh.set_schedule("ddim20")
    for i, lens in enumerate(LENS_SETS):
        cond, xs = inputs(lens, width=width, cw=cw, seed=40 + i)
        ref = [s.sample(cond[b:b + 1], x[None])[0] for b, x in enumerate(xs)]
        for smp, graph in ((s, True), (s, False), (sh, True)):
            items = smp.sample_ragged(cond, xs, lens, use_graph=graph)
            assert smp.rows == 128 and smp.rows > sum(lens) + len(lens)           # padding frame rows and padding token rows
            for b, (it, r) in enumerate(zip(items, ref)):
                assert it.shape == r.shape and torch.isfinite(it).all(), (lens, b)
                assert torch.equal(it, r), (lens, b, graph, smp is sh, (it - r).abs().max().item())
    sh.close()
    s.close()


@pytest.mark.parametrize("dh", [64, 128])
def test_ragged_two_plane_attention_without_zero_key_is_the_uniform_kernel_per_sequence(dh):
    """mmdm_attention_split_ragged with MMDM_ATTN_NO_ZERO_KEY: the empty initial state (m = -inf, l = 0) through the ragged walk of attn_qkp_kernel --
    sequences of one key, a partial last chunk (5, 17, 70, 129), query tiles and waves past a sequence's end (1, 2, 5, 16 in a grid sized for 129).
    fp32 and plane outputs, bitwise the uniform launch on each sequence alone; a causal ragged launch stays refused."""
    from mixermdm_amd import ops
    from mixermdm_amd._lib import MMDMError
    H, D = 2, 2 * dh
    lens = [70, 5, 64, 129, 16, 2, 1, 17]
    nseq, total = len(lens), sum(lens)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    qkv = ops.split_f32(rnd(dh, total + 7, 3 * D).cuda())          # rows behind the last sequence exist and hold data
    d_off, d_len = torch.from_numpy(off).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    for split_out in (False, True):
        out = torch.full((2, total + 7, D), float("nan"), device="cuda", dtype=torch.float16) if split_out else torch.full((total + 7, D), float("nan"), device="cuda")
        ops.attention_split_ragged(q, k, v, H, d_off, d_len, max(lens), zero_key=False, split_out=split_out, out=out)
        torch.cuda.synchronize()
        body = out[:, :total] if split_out else out[:total]
        tail = out[:, total:] if split_out else out[total:]
        assert torch.isfinite(body.float()).all() and torch.isnan(tail.float()).all()          # rows outside every sequence are not written
        for s, (o, t) in enumerate(zip(off, lens)):
            one = qkv[:, o:o + t].contiguous()[:, None]                                       # [2, 1, t, 3D]
            ref = ops.attention_split(one[..., :D], one[..., D:2 * D], one[..., 2 * D:], H, zero_key=False, split_out=split_out)
            torch.cuda.synchronize()
            got = out[:, o:o + t] if split_out else out[o:o + t]
            assert torch.equal(got, ref[:, 0] if split_out else ref[0]), (s, t, split_out)
    # the zero-key form of the same launch still runs, a causal mask on a ragged launch stays refused
    ops.attention_split_ragged(q, k, v, H, d_off, d_len, max(lens))
    with pytest.raises(MMDMError, match="ragged"):
        ops.attention_split_ragged(q, k, v, H, d_off, d_len, max(lens), zero_key=False, causal=True)


# ---------------------------------------------------------------------------------------------------
# 6. the facade
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import MixerMDM
    root = tmp_path_factory.mktemp("cfg")
    sub = dict(NUM_LAYERS=2, NUM_HEADS=2, DROPOUT=0.1, INPUT_DIM=262, LATENT_DIM=128, FF_SIZE=256)
    for name, nm in [("mdm.yaml", "MDM"), ("in2IN.yaml", "in2IN")]:
        yaml.safe_dump(dict(NAME=nm, **sub), open(root / name, "w"))
    cfg = CfgNode(dict(NAME="MixerMDM", GENERATOR=dict(sub), DISCRIMINATOR=dict(sub), ACTIVATION="gelu", DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine",
                       SAMPLER="uniform", MOTION_REP="global", CFG_WEIGHT=3.5, MIXING_MODE=4, FORCE_INFLUENCE_VAL="None", MODEL1="mdm.yaml", MODEL2="in2IN.yaml"))
    m = MixerMDM(cfg, num_frames=40, sampling_strategy="ddim20", config_root=str(root))
    m.precision = "fp32_split"
    m.init_synthetic(seed=0, std=0.05, bias_std=0.02)
    m = m.to("cuda:0").eval()
    assert m.model1_kind == 1
    return m


FACADE_LENS = (12, 20, 33, 40)


def test_facade_split_mdm_ragged_equals_the_per_item_loop(model):
    """MixerMDM with MODEL1.NAME == "MDM" in fp32_split: forward / forward_test run, sample_many(batching="ragged") and
    generate_for_evaluation(batching="ragged") equal the per-item loop bitwise on 4 items with T = 12, 20, 33, 40."""
    from mixermdm_amd.generation import generate_for_evaluation
    batches = []
    for i, t in enumerate(FACADE_LENS):
        g = torch.Generator().manual_seed(i)
        batches.append({"cond": torch.randn(1, CW, generator=g).cuda(), "x_T": torch.randn(1, t, 524, generator=g).cuda(), "motion_lens": torch.tensor([t]), "text": ["x"]})
    ref = [model.forward_test(dict(b)) for b in batches]
    ref = [{k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in r.items()} for r in ref]
    assert model._sampler.cfg.precision == 2 and model._sampler.cfg.model1_kind == 1
    fw = model.forward(dict(batches[1]))
    assert fw["output"].shape == (1, 20, 524) and torch.isfinite(fw["output"]).all()
    got = model.sample_many([dict(b) for b in batches], batching="ragged")
    for r, g_, t in zip(ref, got, FACADE_LENS):
        assert g_["output"].shape == (1, t, 524) and torch.isfinite(g_["output"]).all() and torch.equal(g_["output"], r["output"]), t
        for k in ("influence_i1", "influence_i2"):
            assert len(g_[k]) == len(r[k]) == 20
            for a, b in zip(g_[k], r[k]):
                assert torch.equal(a, b), (k, t)
    items = [{"text": ("a",), "text_individual1": ("b",), "text_individual2": ("c",), "motion_lens": torch.tensor([t]),
              "cond": torch.randn(1, CW, generator=torch.Generator().manual_seed(i))} for i, t in enumerate(FACADE_LENS)]
    runs = {}
    for batching in ("sequential", "ragged"):
        gen, mm = generate_for_evaluation(model, items, max_length=40, mm_idxs=(1,), mm_num_repeats=2, batching=batching, seed=11)
        assert len(gen) == len(items) and len(mm) == 1
        runs[batching] = (gen, mm)
    for a, b in zip(runs["sequential"][0], runs["ragged"][0]):
        assert np.isfinite(a["motion1"]).all() and np.array_equal(a["motion1"], b["motion1"]) and np.array_equal(a["motion2"], b["motion2"])
    for a, b in zip(runs["sequential"][1], runs["ragged"][1]):
        assert np.array_equal(a["mm_motions"], b["mm_motions"])

"""GPU: key-padding masks, from the attention kernels up to Mixer.forward(mask=) and the masked DDIM loop.

Kernel level: mmdm_attention_masked_f32 against the float64 yardstick tests/mask_cases.py::ref_attention_masked_f64 (tests/test_mask_cpu.py
shows that it is nn.MultiheadAttention with key_padding_mask) over EVERY output element, outputs in NaN-filled buffers with a guard band, at
the project's fp32 attention tolerance TOL["f32"] of tests/test_gpu_attention_edges.py (3e-6 + 1e-5 |ref|: masking removes terms from the
sums and adds none).  Module and loop level: tests/golden/mask.npz, captured from the reference with a mask (tests/golden/make_golden_mask.py),
each held to the tolerance of the unmasked test of the same module (named at the comparison).
"""
import ctypes as C
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mask_cases as MC                                              # noqa: E402
from test_gpu_attention_edges import TOL, GUARD                      # noqa: E402
from test_gpu_kernels import assert_close, GEO                       # noqa: E402
from test_gpu_sampler import STEP_TOL                                # noqa: E402

ATOL, RTOL = TOL["f32"][1], TOL["f32"][2]
ERR_ARG, ERR_UNSUPPORTED = 1, 4


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def masked(q, k, v, dh, valid, shift=0, flags=0):
    """mmdm_attention_masked_f32 on CPU operands; valid: bool [rows, Tk] or None.  Returns (status, out [nseq, Tq, HD] on the CPU); the
    guard band behind the output must still be NaN and every output element must have been written."""
    from mixermdm_amd._lib import load_library
    lib, d = load_library(), dev()
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    qd, kd, vd = [t.reshape(-1, HD).to(d).contiguous() for t in (q, k, v)]
    vb = valid.to(torch.uint8).to(d).contiguous() if valid is not None else None
    out = torch.full((nseq * Tq + GUARD, HD), float("nan"), device=d)
    rc = lib.mmdm_attention_masked_f32(_p(qd), HD, _p(kd), HD, _p(vd), HD, _p(out), HD, 0, flags, nseq, Tq, Tk, HD // dh, dh, shift,
                                       _p(vb), vb.shape[0] if vb is not None else 0, None)
    torch.cuda.synchronize()
    if rc:
        return rc, None
    assert torch.isnan(out[nseq * Tq:]).all(), "guard band written"
    res = out[:nseq * Tq].cpu().reshape(nseq, Tq, HD)
    assert torch.isfinite(res).all(), "an output element was not written (or is not finite)"
    return 0, res


def unmasked(q, k, v, dh, shift=0):
    from mixermdm_amd import ops
    d = dev()
    out = ops.attention(q.to(d), k.to(d), v.to(d), q.shape[2] // dh, kv_seq_shift=shift)
    torch.cuda.synchronize()
    return out.cpu()


def check_elem(got, ref, what):
    err = (got.double() - ref).abs()
    lim = ATOL + RTOL * ref.abs()
    print(f"{what}: max err {err.max().item():.3e} (limit at that element {lim.flatten()[err.argmax()].item():.3e})")
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())}/{err.numel()} elements outside {ATOL} + {RTOL} |ref|; max err {err.max().item():.3e}"


# ---------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", MC.HEAD_SIZES)
@pytest.mark.parametrize("Tq,Tk", [(T, T) for T in MC.SELF_T] + list(MC.CROSS))
def test_masked_attention_vs_float64(dh, Tq, Tk):
    q, k, v = MC.operands(dh, Tq, Tk)
    shift = 0 if Tq == Tk else 1
    for name, valid in MC.masks(Tk).items():
        rc, got = masked(q, k, v, dh, valid, shift)
        assert rc == 0, name
        check_elem(got, MC.ref_attention_masked_f64(q, k, v, MC.H, valid, shift=shift), f"dh={dh} {Tq}x{Tk} {name}")
        if name == "none":
            assert torch.count_nonzero(got).item() == 0, "every key invalid: the output is exactly 0"


@pytest.mark.parametrize("dh", MC.HEAD_SIZES)
def test_one_mask_row_shared_by_all_sequences(dh):
    q, k, v = MC.operands(dh, 33, 33)
    one = MC.masks(33, rows=1)["holes"]
    rc, got = masked(q, k, v, dh, one)
    assert rc == 0
    check_elem(got, MC.ref_attention_masked_f64(q, k, v, MC.H, one), f"dh={dh} mask_rows=1")
    rc, rep = masked(q, k, v, dh, one.expand(MC.NSEQ, -1))
    assert torch.equal(got, rep)


@pytest.mark.parametrize("dh", (64, 128, 16))
def test_null_and_all_valid_masks_are_bitwise_the_unmasked_call(dh):
    for Tq, Tk, shift in [(33, 33, 0), (65, 65, 0), (16, 65, 1)]:
        q, k, v = MC.operands(dh, Tq, Tk)
        ref = unmasked(q, k, v, dh, shift)
        assert torch.equal(masked(q, k, v, dh, None, shift)[1], ref)
        assert torch.equal(masked(q, k, v, dh, torch.ones(MC.NSEQ, Tk, dtype=torch.bool), shift)[1], ref)


@pytest.mark.parametrize("dh", (64, 128))
def test_trailing_mask_is_bitwise_the_shorter_unmasked_call(dh):
    """L valid keys over finite K / V == the unmasked self-attention call at T = L in the first L query rows (the masked chunks add 2^-inf = 0
    and leave the running maximum alone)."""
    T = 65
    q, k, v = MC.operands(dh, T, T)
    for L in (1, 15, 16, 17, 33, 64):
        valid = torch.zeros(MC.NSEQ, T, dtype=torch.bool)
        valid[:, :L] = True
        got = masked(q, k, v, dh, valid)[1]
        short = unmasked(q[:, :L].contiguous(), k[:, :L].contiguous(), v[:, :L].contiguous(), dh)
        assert torch.equal(got[:, :L], short), L


def test_refusals_name_the_case():
    from mixermdm_amd._lib import load_library
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_state_dict
    lib = load_library()
    q, k, v = MC.operands(64, 17, 17)
    valid = torch.ones(MC.NSEQ, 17, dtype=torch.bool)
    for flags in (1, 3):
        assert masked(q, k, v, 64, valid, flags=flags)[0] == ERR_UNSUPPORTED and b"zero key" in lib.mmdm_last_error()
    one = np.ones((2, 16), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    dims = dict(d_latent=64, d_ff=64, d_layers=1, m_latent=64, m_ff=64, m_layers=1)
    s = Sampler(d_heads=1, m_heads=1, max_batch=2, max_frames=16, precision="bf16", **dims)
    assert lib.mmdm_set_key_mask(s.h, ptr(one), 2, 16) == ERR_UNSUPPORTED and b"precision 1" in lib.mmdm_handle_error(s.h)
    s.close()
    s = Sampler(d_latent=16, d_ff=32, d_layers=1, d_heads=2, m_latent=16, m_ff=32, m_layers=1, m_heads=2, model1_kind=1, max_batch=2, max_frames=16)
    assert lib.mmdm_set_key_mask(s.h, ptr(one), 2, 16) == ERR_UNSUPPORTED and b"MDM" in lib.mmdm_handle_error(s.h)
    s.close()
    s = Sampler(d_latent=16, d_ff=32, d_layers=1, d_heads=2, single_only=2, max_batch=2, max_frames=16)
    assert lib.mmdm_set_key_mask(s.h, ptr(one), 2, 16) == ERR_UNSUPPORTED and b"single_only = 2" in lib.mmdm_handle_error(s.h)
    from mixermdm_amd.models import _KeyMask
    with pytest.raises(NotImplementedError, match="single_only = 2"):       # the Python callables turn the library's refusal into NotImplementedError
        with _KeyMask(s, torch.ones(2, 16, 1)):
            pass
    s.close()
    dims = dict(d_latent=64, d_ff=64, d_layers=1, m_latent=64, m_ff=64, m_layers=1)
    s = Sampler(d_heads=1, m_heads=1, max_batch=2, max_frames=16, **dims)
    s.load_state_dict(synthetic_state_dict(**dims))
    s.set_norm_stats(*[np.ones(262, np.float32)] * 4)
    s.prepare()
    s.set_schedule("ddim20")
    empty = one.copy()
    empty[1] = 0
    assert lib.mmdm_set_key_mask(s.h, ptr(empty), 2, 16) == ERR_ARG and b"row 1 has no valid frame" in lib.mmdm_handle_error(s.h)
    assert lib.mmdm_set_key_mask(s.h, ptr(one), 5, 16) == ERR_ARG
    s.set_key_mask(one)
    x, cond = MC.rnd(1, 2, 12, 524), MC.rnd(2, 2, 8 * 768)
    assert lib.mmdm_begin(s.h, _p(cond.to(dev())), _p(x.to(dev())), 2, 12, s._s()) == ERR_ARG and b"key mask" in lib.mmdm_handle_error(s.h)      # T mismatch
    xd = MC.rnd(1, 4, 16, 524).to(dev())
    out = torch.empty_like(xd)
    assert lib.mmdm_module_forward(s.h, 2, _p(xd), _p(xd), _p(MC.rnd(2, 4, 8 * 768).to(dev())), 5, _p(out), 4, 16, s._s()) == ERR_ARG      # rows 2 != n 4
    assert b"key mask" in lib.mmdm_handle_error(s.h)
    lens = (C.c_int * 2)(16, 9)
    xr = MC.rnd(3, 25, 524).to(dev())
    assert lib.mmdm_begin_ragged(s.h, _p(cond.to(dev())), _p(xr), 2, lens, s._s()) == ERR_UNSUPPORTED and b"ragged" in lib.mmdm_handle_error(s.h)
    s.set_key_mask(None)
    assert lib.mmdm_begin_ragged(s.h, _p(cond.to(dev())), _p(xr), 2, lens, s._s()) == 0
    s.close()


def test_align_with_per_sequence_last_frame_vs_reference_golden():
    """Recipe and tolerance of tests/test_gpu_kernels.py::test_mixer_pre_golden_fixture (GEO), with the reference's masked align_motions."""
    from mixermdm_amd import ops
    g, inp, t = MC.load_mask_golden()
    ident = torch.cat([torch.zeros(262), torch.ones(262), torch.zeros(262), torch.ones(262)]).to(dev())
    for tag in ("holes:T20", "trail:T33"):
        tgt, mov = inp(f"geo:{tag}:target"), inp(f"geo:{tag}:moved")
        last = t(f"geo:{tag}:last").to(torch.int32)
        valid = t(f"mask:{tag}")[..., 0] > 0.5
        assert torch.equal(valid.sum(1).to(torch.int32) - 1, last)
        o1, o2 = torch.cat([mov, mov], -1).to(dev()), torch.cat([tgt, tgt], -1).to(dev())
        g1, _ = ops.mixer_pre(o1, o2, ident, True, last_frame=last.to(dev()))
        assert_close(g1[..., :262], t(f"geo:{tag}:align_m2_ih"), what=tag + " moved", **GEO)
        full, _ = ops.mixer_pre(o1, o2, ident, True, last_frame=torch.full((1,), o1.shape[1] - 1, dtype=torch.int32, device=dev()))
        assert torch.equal(full, ops.mixer_pre(o1, o2, ident, True)[0])


# ---------------------------------------------------------------------------------------------------
# module and loop level (tiny handles built from the existing fixtures' weights)
# ---------------------------------------------------------------------------------------------------
def valid_of(t, tag):
    return t(f"mask:{tag}")[..., 0] > 0.5


def mixer_sampler(golden, mode=4, model2_kind=0, max_batch=2):
    from mixermdm_amd.sampler import Sampler
    g, w, _ = golden("mixer")
    W = w("mix.")
    if mode in (1, 2):
        W.update(w("mix_out1."))
    s = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=int(g["d_heads"]), m_latent=16, m_ff=32, m_layers=2, m_heads=int(g["m_heads"]), mixing_mode=mode,
                align=True, model2_kind=model2_kind, cfg_scale=float(g["cfg_scale"]), max_batch=max_batch, max_frames=40)
    s.load_state_dict(W)
    s.set_norm_stats(g["mean_hml"], g["std_hml"], g["mean_ih"], g["std_ih"])
    s.prepare()
    return s


def test_masked_denoisers_vs_reference_golden(golden):
    """Tolerance of tests/test_gpu_sampler.py::test_denoisers_vs_reference_golden (atol 2e-5, rtol 1e-4)."""
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_state_dict
    g, inp, t = MC.load_mask_golden()
    _, w, _ = golden("denoisers")
    for net, tag, which, kind in [("ind", "holes:T33", 0, 0), ("int", "trail:T20", 1, 0), ("ig", "holes:T20", 1, 1)]:
        if which == 0:
            s = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=2, single_only=True, max_batch=1, max_frames=40)
            W = {"denoiser1." + k: v for k, v in w("ind.").items()}
        else:
            s = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=2, m_latent=16, m_ff=32, m_layers=2, m_heads=2, model2_kind=kind, max_batch=1, max_frames=40)
            W = synthetic_state_dict(d_latent=16, d_ff=32, d_layers=2, m_latent=16, m_ff=32, m_layers=2)
            W.update({"denoiser2." + k: v for k, v in w(net + ".").items()})
            s.set_norm_stats(*[np.ones(262, np.float32)] * 4)
        s.load_state_dict(W)
        s.prepare()
        x, c = inp(f"{net}:{tag}:x"), inp(f"{net}:{tag}:cond")
        plain = s.module_forward(which, x, c, int(g["den:t"]))
        s.set_key_mask(valid_of(t, tag))                 # rows == n: the two fixture items are the call's batch
        out = s.module_forward(which, x, c, int(g["den:t"]))
        assert_close(out, t(f"{net}:{tag}"), atol=2e-5, rtol=1e-4, what=f"{net} {tag}")
        # mask=None is bit-identical before and after a mask was set and cleared
        s.set_key_mask(None)
        assert torch.equal(s.module_forward(which, x, c, int(g["den:t"])), plain) and not torch.equal(plain, out)
        s.close()


@pytest.mark.parametrize("mode,tag", [(2, "trail:T20"), (3, "holes:T20")])
def test_masked_mixer_forward_vs_reference_golden(golden, mode, tag):
    """Tolerance of tests/test_gpu_sampler.py::test_mixer_forward_vs_reference_golden (STEP_TOL).  The inputs are the first seeded draw at which
    the reference's own fp32 run is within 2e-4 + 2e-4 |ref| of its float64 run in every element (make_golden_mask.py; the ratio is stored):
    N(0, 1) denoiser outputs can make an alignment ill-conditioned in rows no mask touches, and such a draw measures the input, not the mask."""
    g, inp, t = MC.load_mask_golden()
    assert float(g[f"mix:m{mode}:{tag}:ref_f64_ratio"]) <= 1.0
    s = mixer_sampler(golden, mode)
    x1, x2, cond = inp(f"mix:m{mode}:{tag}:x1"), inp(f"mix:m{mode}:{tag}:x2"), inp(f"mix:m{mode}:{tag}:cond")
    cond[2:] = 0
    s.set_key_mask(torch.cat([valid_of(t, tag)] * 2, 0))            # the caller repeats the mask for the CFG-doubled batch
    out = s.module_forward(2, x1, cond, int(g["mix:t"]), x2=x2)
    assert_close(out, t(f"mix:m{mode}:{tag}"), what=f"Mixer.forward(mask) mode {mode}", **STEP_TOL)
    s.close()


def test_masked_cfg_wrapper_and_python_callables_vs_reference_golden(tmp_path, golden):
    """Tolerance of tests/test_gpu_callers.py::test_cfg_x2_forward_vs_reference_golden (STEP_TOL), through mmdm_module_forward(which = 4) and
    through the callables of mixermdm_amd.models with the reference's float [n, T, k] mask."""
    from test_gpu_facade import tiny_model
    g, inp, t = MC.load_mask_golden()
    tag = "holes:T20"
    x, x2, cond, ref = inp(f"cfg:{tag}:x"), inp(f"cfg:{tag}:x2"), inp(f"cfg:{tag}:cond"), t(f"cfg:{tag}")
    s = mixer_sampler(golden)
    s.set_key_mask(valid_of(t, tag))                                 # B rows: the library repeats them for its own doubling
    assert_close(s.module_forward(4, x, cond, 640, x2=x2), ref, what="which = 4 with a mask", **STEP_TOL)
    s.close()
    m, _, _ = tiny_model(tmp_path, golden, strategy="ddim20")
    from mixermdm_amd.models import ClassifierFreeSampleModelX2
    cfg = ClassifierFreeSampleModelX2(m.mixing, 3.5)
    mask = t(f"mask:{tag}").cuda()
    ts = torch.full((2,), 640)
    out = cfg(x.cuda(), x2.cuda(), ts, cond=cond.cuda(), mask=mask)
    assert_close(out, ref, what="ClassifierFreeSampleModelX2.forward(mask=)", **STEP_TOL)
    plain = cfg(x.cuda(), x2.cuda(), ts, cond=cond.cuda(), mask=None)
    assert not torch.equal(plain, out) and torch.equal(plain, cfg(x.cuda(), x2.cuda(), ts, cond=cond.cuda()))
    # Mixer.forward(mask=) with the doubled mask vs the mode-3 golden (modes 3 and 4 share their weights: influence.out is 23 wide in both)
    m.mixing.mixing_mode = 3
    xm1, xm2, cm = inp(f"mix:m3:{tag}:x1"), inp(f"mix:m3:{tag}:x2"), inp(f"mix:m3:{tag}:cond")
    cm[2:] = 0
    mask4, t4 = torch.cat([mask, mask]), torch.full((4,), 640)
    mf = m.mixing(xm1.cuda(), t4, cond=cm.cuda(), mask=mask4, x2=xm2.cuda())
    assert_close(mf, t(f"mix:m3:{tag}"), what="Mixer.forward(mask=)", **STEP_TOL)
    plain = m.mixing(xm1.cuda(), t4, cond=cm.cuda(), mask=None, x2=xm2.cuda())          # the mask was cleared behind the masked call
    assert not torch.equal(plain, mf) and torch.equal(plain, m.mixing(xm1.cuda(), t4, cond=cm.cuda(), x2=xm2.cuda()))
    # the denoiser callables with the doubled mask == mmdm_module_forward on a stand-alone Sampler with the same weights and mask (bitwise),
    # which tests/test_gpu_mask.py::test_masked_denoisers_vs_reference_golden ties to the reference
    s = mixer_sampler(golden, 3)
    s.set_key_mask(mask4[..., 0] > 0.5)
    for which, den, x, c in [(0, m.mixing.denoiser1, MC.rnd(470, 4, 20, 262), MC.rnd(471, 4, 768)),
                             (1, m.mixing.denoiser2, MC.rnd(472, 4, 20, 524), MC.rnd(473, 4, 3 * 768))]:
        got = den(x.cuda(), torch.full((4,), 500), mask=mask4, cond=c.cuda())
        ref = s.module_forward(which, x, c, 500)
        assert torch.equal(got, ref), which
        assert not torch.equal(den(x.cuda(), torch.full((4,), 500), mask=None, cond=c.cuda()), ref)
    s.close()


def test_masked_loop_vs_reference_golden_and_graph_cache(golden):
    """The 4-step masked two-chain loop vs mask.npz at the bound of tests/test_gpu_sampler.py::test_ddim_step_and_loop_vs_reference_golden
    (mean <= 2e-3, 99th percentile <= 3e-2); graph replay == eager bitwise; masked -> unmasked -> masked with other values on ONE handle
    gives the stand-alone results each time, with two captures in all."""
    g, inp, t = MC.load_mask_golden()
    tag = "holes:T33"
    xT, cond = inp(f"loop:{tag}:x_T"), inp(f"loop:{tag}:cond")
    va, vb = valid_of(t, tag), valid_of(t, "trail:T33")
    s = mixer_sampler(golden)
    s.set_schedule(str(g["loop:strategy"]))
    s.set_key_mask(va)
    eager_a = s.sample(cond, xT, use_graph=False)
    d = np.abs(eager_a.cpu().numpy() - g[f"loop:{tag}"])
    print("masked loop: mean err %.3e, p99 %.3e, max %.3e" % (d.mean(), np.percentile(d, 99), d.max()))
    assert d.mean() <= 2e-3 and np.percentile(d, 99) <= 3e-2, (d.mean(), d.max())
    s.set_key_mask(vb)
    eager_b = s.sample(cond, xT, use_graph=False)
    s.set_key_mask(None)
    eager_0 = s.sample(cond, xT, use_graph=False)
    assert not torch.equal(eager_a, eager_b) and not torch.equal(eager_a, eager_0)
    assert s.graph_stats()[0] == 0
    s.set_key_mask(va)
    assert torch.equal(s.sample(cond, xT, use_graph=True), eager_a) and s.graph_stats()[0] == 1
    s.set_key_mask(None)
    assert torch.equal(s.sample(cond, xT, use_graph=True), eager_0) and s.graph_stats()[0] == 2
    s.set_key_mask(vb)
    assert torch.equal(s.sample(cond, xT, use_graph=True), eager_b) and s.graph_stats()[0] == 2      # other VALUES: no re-capture
    s.close()


def test_masked_loop_through_the_python_diffusion(tmp_path, golden):
    """model_kwargs = {"mask": m, "cond": c} through MixerDiffusion.ddim_sample_loop (the two-chain loop)."""
    from test_gpu_facade import tiny_model
    from mixermdm_amd.models import MixerDiffusion, ClassifierFreeSampleModelX2
    from mixermdm_amd.schedule import space_timesteps
    g, inp, t = MC.load_mask_golden()
    tag = "holes:T33"
    xT, cond, mask = inp(f"loop:{tag}:x_T").cuda(), inp(f"loop:{tag}:cond").cuda(), t(f"mask:{tag}").cuda()
    m, _, _ = tiny_model(tmp_path, golden, strategy="ddim4")
    diff = MixerDiffusion(use_timesteps=space_timesteps(1000, "ddim4"), betas=m.betas)
    cfg = ClassifierFreeSampleModelX2(m.mixing, 3.5)
    m.mixing.store_influence = False
    out = diff.ddim_sample_loop(cfg, (2, 33, 524), noise=xT, clip_denoised=False, model_kwargs={"mask": mask, "cond": cond})
    d = np.abs(out.cpu().numpy() - g[f"loop:{tag}"])
    assert d.mean() <= 2e-3 and np.percentile(d, 99) <= 3e-2, (d.mean(), d.max())
    plain = diff.ddim_sample_loop(cfg, (2, 33, 524), noise=xT, clip_denoised=False, model_kwargs={"mask": None, "cond": cond})
    assert not torch.equal(plain, out)


def test_in2in_individual_loop_takes_a_mask_only_as_an_explicit_argument(golden):
    """in2INDiffusion.forward keeps the reference's mask=None whatever the batch carries (in2in.py:326-350: batch["mask"] is never read); the
    masked individual loop is forward(batch, mask=) and equals, bitwise, a stand-alone Sampler run with the same key mask.  The interaction
    sampler refuses an explicit mask by name and ignores a batch entry."""
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import in2IN
    from mixermdm_amd.sampler import Sampler
    base = dict(NUM_LAYERS=2, DROPOUT=0.1, INPUT_DIM=262, LATENT_DIM=16, FF_SIZE=32, DIFFUSION_STEPS=1000, BETA_SCHEDULER="cosine", STRATEGY="ddim20")
    g, w, t = golden("single")
    m = in2IN(CfgNode(dict(base, NAME="in2INind", NUM_HEADS=int(g["H"]), CFG_WEIGHT=float(g["cfg_scale"]))), "individual")
    m.decoder.load_state_dict({"net_individual." + k: v for k, v in w("ind.").items()})
    m = m.to("cuda:0")
    mask = torch.ones(2, 12, 1)
    mask[0, 3:6] = 0
    mask[1, 7:] = 0
    batch = {"cond_individual_individual1": t("cond").cuda(), "x_T": t("x_T").cuda(), "motion_lens": torch.tensor([12, 12])}
    plain = m.decoder(dict(batch))["output"]
    assert torch.equal(m.decoder(dict(batch, mask=mask.cuda()))["output"], plain)            # a batch entry changes nothing
    masked_out = m.decoder(dict(batch), mask=mask.cuda())["output"]
    assert not torch.equal(masked_out, plain) and torch.equal(m.decoder(dict(batch))["output"], plain)
    s = Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=int(g["H"]), single_only=True, cfg_scale=float(g["cfg_scale"]), max_batch=2, max_frames=16)
    s.load_state_dict({"denoiser1." + k: v for k, v in w("ind.").items()})
    s.prepare()
    s.set_schedule("ddim20")
    assert torch.equal(s.sample(t("cond"), t("x_T")), plain)
    s.set_key_mask(mask[..., 0] > 0.5)
    assert torch.equal(s.sample(t("cond"), t("x_T")), masked_out)
    s.close()
    g, w, t = golden("interaction")
    mi = in2IN(CfgNode(dict(base, NAME="in2IN", NUM_HEADS=int(g["H"]), CFG_WEIGHT=float(g["s"]), CFG_WEIGHT_INTERACTION=float(g["s_int"]),
                            CFG_WEIGHT_INDIVIDUAL=float(g["s_ind"]))), "interaction")
    mi.decoder.load_state_dict({"net_interaction." + k: v for k, v in w("int.").items()})
    mi = mi.to("cuda:0")
    c = t("cond").cuda()
    bi = {"cond_interaction": c[:, :768], "cond_interaction_individual1": c[:, 768:1536], "cond_interaction_individual2": c[:, 1536:],
          "x_T": t("x_T").cuda(), "motion_lens": torch.tensor([12, 12])}
    ref = mi.decoder(dict(bi))["output"]
    assert torch.equal(mi.decoder(dict(bi, mask=mask.cuda()))["output"], ref)
    with pytest.raises(NotImplementedError, match="single_only = 2"):
        mi.decoder(dict(bi), mask=mask.cuda())


# ---------------------------------------------------------------------------------------------------
# the reference's attention layers and Influence with a mask, composed from the stateless kernels (dh = 8: attn_small_kernel)
# ---------------------------------------------------------------------------------------------------
# A denoiser is a stack of these layers and is held to atol 2e-5 / rtol 1e-4 (test_masked_denoisers_vs_reference_golden); one layer, and the
# two-block Influence stack on unit-variance inputs, are held to the same.
LAYER_TOL = dict(atol=2e-5, rtol=1e-4)


class _Layers:
    """VanillaSelfAttention / VanillaCrossAttention / FFN / InfluenceBlockCross (layers.py:28-106, influence.py:34-48) from mixermdm_amd.ops."""

    def __init__(self, W, H):
        self.W, self.H = {k: v.to(dev()) for k, v in W.items()}, H

    def lin(self, p, x, epilogue="bias"):
        from mixermdm_amd import ops
        return ops.linear(x, self.W[p + ".weight"], self.W[p + ".bias"], epilogue=epilogue)

    def norm(self, p, x, emb):
        from mixermdm_amd import ops
        return ops.adaln(x, self.lin(p + ".emb_layers.1", torch.nn.functional.silu(emb)))

    def mha(self, p, q_in, kv_in, kpm):
        from mixermdm_amd import ops
        D = q_in.shape[-1]
        w, b = self.W[p + ".in_proj_weight"], self.W[p + ".in_proj_bias"]
        q = ops.linear(q_in, w[:D], b[:D])
        kv = ops.linear(kv_in, w[D:], b[D:])
        return self.lin(p + ".out_proj", ops.attention(q, kv[..., :D], kv[..., D:], self.H, key_padding_mask=kpm))

    def sa(self, p, x, emb, kpm):
        xn = self.norm(p + ".norm", x, emb)
        return self.mha(p + ".attention", xn, xn, kpm)

    def ca(self, p, x, xf, emb, kpm):
        return self.mha(p + ".attention", self.norm(p + ".norm", x, emb), self.norm(p + ".xf_norm", xf, emb), kpm)

    def ffn(self, p, x, emb):
        return self.lin(p + ".linear2", self.lin(p + ".linear1", self.norm(p + ".norm", x, emb), "gelu"))

    def influence_block(self, p, m_i, m_I, e_i, e_I, kpm):
        h1 = self.sa(p + ".sa_block", m_i, e_i, kpm) + m_i
        h2 = self.ca(p + ".ca_block", h1, m_I, e_I, kpm) + h1
        return self.ffn(p + ".ffn", h2, e_I) + h2


@pytest.mark.parametrize("tag", ["trail:T20", "holes:T33"])
def test_masked_attention_layers_and_influence_vs_reference_golden(golden, tag):
    from mixermdm_amd import ops
    g, inp, t = MC.load_mask_golden()
    kpm = ~valid_of(t, tag).to(dev())
    _, w, _ = golden("layers")
    W = {"sa." + k: v for k, v in w("sa.").items()}
    W.update({"ca." + k: v for k, v in w("ca.").items()})
    L = _Layers(W, 4)
    x, y, e = [inp(f"layers:{tag}:{n}").to(dev()) for n in ("x", "y", "emb")]
    assert_close(L.sa("sa", x, e, kpm), t(f"sa:{tag}"), what="VanillaSelfAttention " + tag, **LAYER_TOL)
    assert_close(L.ca("ca", x, y, e, kpm), t(f"ca:{tag}"), what="VanillaCrossAttention " + tag, **LAYER_TOL)
    assert not torch.allclose(L.sa("sa", x, e, None).cpu(), t(f"sa:{tag}"), atol=1e-3)
    # Influence, modes 1 (time mean over ALL T frames, masked ones included: influence.py:120-121) and 2
    _, w, _ = golden("influence")
    I = _Layers(w("m4."), 4)
    m_i, m_I, c_i, c_I = [inp(f"infl:{tag}:{n}").to(dev()) for n in ("m_i", "m_I", "cond_i", "cond_I")]
    h = m_i
    for i in range(2):
        h = I.influence_block(f"blocks.{i}", h, m_I, c_i, c_I, kpm)
    for mode in (1, 2):
        o = {k: v.to(dev()) for k, v in w(f"m{mode}.").items()}
        hh = ops.mean_time(h) if mode == 1 else h
        assert_close(ops.influence_head(hh, o["out.weight"], o["out.bias"]), t(f"infl:m{mode}:{tag}"), what=f"Influence mode {mode} " + tag, **LAYER_TOL)

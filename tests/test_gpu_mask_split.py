"""GPU: key-padding masks in the fp32_split precision mode -- mmdm_attention_split_masked (attn_qkp_kernel<DH, 2, true, true, false, MASK = true>)
and mmdm_set_key_mask on precision-2 handles.

Kernel level: against the float64 yardstick tests/mask_cases.py::ref_attention_masked_f64 over EVERY output element, outputs in NaN-filled
buffers with a guard band, at the project's own bound for the two-plane kernel, TOL["split"] of tests/test_gpu_attention_edges.py
(2e-5 + 1e-4 |ref|: masking removes terms from the sums and adds none); the bitwise identities the fp32 form has (tests/test_gpu_mask.py):
NULL / all-valid mask == the unmasked call, one shared mask row == the row repeated, a trailing mask == the shorter unmasked call.
Handle level, at the real head sizes 64 and 128 (DESIGN 9a has the measured distances):
  (a) a trailing mask keeping L frames gives, in the first L frames, the bits of the unmasked call at T = L (denoisers; AdaLN, FFN and PE are
      row-wise, the split GEMMs' bits do not depend on M, masked keys add exact zeros; the mixer's time mean runs over all T frames);
  (b) masked fp32_split against the masked fp32 handle (existing code, pinned by tests/test_gpu_mask.py), with the UNMASKED distance between
      the two handles on the same inputs as the yardstick: masked <= 3 x unmasked + 1e-6 in relative RMS and in maximum error (factor and form
      of tests/test_gpu_packed_modes.py::test_conditioning_projections_on_the_split_kernel_match_the_fp32_kernel);
  (c) the mask <-> no mask <-> other values graph-cache sequence of tests/test_gpu_mask.py::test_masked_loop_vs_reference_golden_and_graph_cache.
The reference goldens of tests/golden/mask.npz (D = 16) cannot run here: mmdm_create refuses latent sizes that are no multiple of 32 for every
precision >= 1 (pinned below), so no fp32_split handle exists at that size.
mmdm_attention_split_ragged gained no mask argument: a mask on a ragged launch is refused inside the library (mmdm_begin_ragged, pinned below).
"""
import ctypes as C
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mask_cases as MC                                              # noqa: E402
from test_gpu_attention_edges import TOL, GUARD                      # noqa: E402
from test_gpu_ragged import DIMS                                     # noqa: E402   (D 128, 2 heads: head size 64 in every stack)

ATOL, RTOL = TOL["split"][1], TOL["split"][2]
ERR_ARG, ERR_UNSUPPORTED = 1, 4
HEAD_SIZES = tuple(dh for dh in MC.HEAD_SIZES if dh in (64, 128))
DIMS128 = dict(d_latent=256, d_ff=512, d_layers=2, m_latent=256, m_ff=512, m_layers=2)      # 2 heads: head size 128 in every stack
HANDLE_DIMS = {64: DIMS, 128: DIMS128}
B, T, L_TRAIL = 2, 33, 17
STEP_ATOL, STEP_RTOL = 2e-4, 2e-4            # the project's step tolerance (tests/test_gpu_sampler.py::STEP_TOL): the conditioning rule of (b), which = 2


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def split_call(q, k, v, dh, valid=None, shift=0, flags=0, out_mode=0, plain=False):
    """mmdm_attention_split_masked (plain: mmdm_attention_split) on CPU fp32 operands, split into their two fp16 planes on the device; valid: bool
    [rows, Tk] or None.  Returns (status, out): fp32 [nseq, Tq, HD], or the fp16 planes [2, nseq, Tq, HD] for out_mode 2, on the CPU; the guard band
    behind the output must still be NaN and every output element must have been written."""
    from mixermdm_amd import ops
    from mixermdm_amd._lib import load_library
    lib, d = load_library(), dev()
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    qs, ks, vs = [ops.split_f32(t.reshape(-1, HD).to(d).contiguous()) for t in (q, k, v)]          # [2, rows, HD]
    vb = valid.to(torch.uint8).to(d).contiguous() if valid is not None else None
    planes, rows = (2 if out_mode == 2 else 1), nseq * Tq
    out = torch.full((planes * rows + GUARD, HD), float("nan"), device=d, dtype=torch.float16 if out_mode == 2 else torch.float32)
    args = (_p(qs), HD, qs.shape[1] * HD, _p(ks), HD, ks.shape[1] * HD, _p(vs), HD, vs.shape[1] * HD, _p(out), HD, out_mode, flags,
            nseq, Tq, Tk, HD // dh, dh, shift)
    if plain:
        assert valid is None
        rc = lib.mmdm_attention_split(*args, None)
    else:
        rc = lib.mmdm_attention_split_masked(*args, _p(vb), vb.shape[0] if vb is not None else 0, None)
    torch.cuda.synchronize()
    if rc:
        return rc, None
    assert torch.isnan(out[planes * rows:]).all(), "guard band written"
    res = out[:planes * rows].cpu()
    assert torch.isfinite(res).all(), "an output element was not written (or is not finite)"
    return 0, (res.reshape(2, nseq, Tq, HD) if out_mode == 2 else res.reshape(nseq, Tq, HD))


def check_elem(got, ref, what):
    err = (got.double() - ref).abs()
    lim = ATOL + RTOL * ref.abs()
    print(f"{what}: max err {err.max().item():.3e} (limit at that element {lim.flatten()[err.argmax()].item():.3e})")
    assert (err <= lim).all(), f"{what}: {int((err > lim).sum())}/{err.numel()} elements outside {ATOL} + {RTOL} |ref|; max err {err.max().item():.3e}"


# ---------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", HEAD_SIZES)
@pytest.mark.parametrize("Tq,Tk", [(t, t) for t in MC.SELF_T] + list(MC.CROSS))
def test_masked_split_attention_vs_float64(dh, Tq, Tk):
    """A partial, a full and a just-over 16-key stage, a whole middle chunk masked, key 0 masked, every key masked (exactly 0).  out_mode 2 is
    ops.split_f32 of the out_mode 0 result, bit for bit -- the property tests/test_gpu_attention_edges.py::test_output_modes_at_the_edges pins
    for the unmasked kernel."""
    from mixermdm_amd import ops
    q, k, v = MC.operands(dh, Tq, Tk)
    shift = 0 if Tq == Tk else 1
    for name, valid in MC.masks(Tk).items():
        rc, got = split_call(q, k, v, dh, valid, shift)
        assert rc == 0, name
        check_elem(got, MC.ref_attention_masked_f64(q, k, v, MC.H, valid, shift=shift), f"split dh={dh} {Tq}x{Tk} {name}")
        if name == "none":
            assert torch.count_nonzero(got).item() == 0, "every key invalid: the output is exactly 0"
        rc, planes = split_call(q, k, v, dh, valid, shift, out_mode=2)
        assert rc == 0, name
        assert torch.equal(planes, ops.split_f32(got.to(dev())).cpu()), (name, "out_mode 2 is not the split of the fp32 output")


@pytest.mark.parametrize("dh", HEAD_SIZES)
def test_one_mask_row_shared_by_all_sequences(dh):
    from mixermdm_amd import ops
    q, k, v = MC.operands(dh, 33, 33)
    one = MC.masks(33, rows=1)["holes"]
    rc, got = split_call(q, k, v, dh, one)
    assert rc == 0
    check_elem(got, MC.ref_attention_masked_f64(q, k, v, MC.H, one), f"split dh={dh} mask_rows=1")
    rc, rep = split_call(q, k, v, dh, one.expand(MC.NSEQ, -1))
    assert rc == 0 and torch.equal(got, rep)
    # the Python entry point: ops.attention_split(key_padding_mask=) is this call (PyTorch's sense: True = ignore the key)
    qs, ks, vs = [ops.split_f32(t.to(dev())) for t in (q, k, v)]
    py = ops.attention_split(qs, ks, vs, MC.H, key_padding_mask=~one.to(dev()))
    torch.cuda.synchronize()
    assert torch.equal(py.cpu(), got)
    with pytest.raises(TypeError, match="key_padding_mask"):
        ops.attention_split(qs, ks, vs, MC.H, key_padding_mask=one)          # a CPU tensor


@pytest.mark.parametrize("dh", HEAD_SIZES)
def test_null_and_all_valid_masks_are_bitwise_the_unmasked_call(dh):
    for Tq, Tk, shift in [(33, 33, 0), (65, 65, 0), (16, 65, 1)]:
        q, k, v = MC.operands(dh, Tq, Tk)
        for out_mode in (0, 2):
            rc, ref = split_call(q, k, v, dh, None, shift, out_mode=out_mode, plain=True)
            assert rc == 0
            assert torch.equal(split_call(q, k, v, dh, None, shift, out_mode=out_mode)[1], ref)
            assert torch.equal(split_call(q, k, v, dh, torch.ones(MC.NSEQ, Tk, dtype=torch.bool), shift, out_mode=out_mode)[1], ref)


@pytest.mark.parametrize("dh", HEAD_SIZES)
def test_trailing_mask_is_bitwise_the_shorter_unmasked_call(dh):
    """L valid keys over finite K / V == mmdm_attention_split at T = L in the first L query rows: the masked probabilities split into exact zero
    planes, and a wholly masked chunk leaves the deferred maximum, the row sums and the accumulators alone."""
    Tfull = 65
    q, k, v = MC.operands(dh, Tfull, Tfull)
    for L in (1, 15, 16, 17, 33, 64):
        valid = torch.zeros(MC.NSEQ, Tfull, dtype=torch.bool)
        valid[:, :L] = True
        got = split_call(q, k, v, dh, valid)[1]
        short = split_call(q[:, :L].contiguous(), k[:, :L].contiguous(), v[:, :L].contiguous(), dh, plain=True)[1]
        assert torch.equal(got[:, :L], short), L


def test_kernel_refusals_name_the_case():
    from mixermdm_amd._lib import load_library
    lib = load_library()
    q, k, v = MC.operands(64, 17, 17)
    valid = torch.ones(MC.NSEQ, 17, dtype=torch.bool)
    for flags in (1, 3):
        assert split_call(q, k, v, 64, valid, flags=flags)[0] == ERR_UNSUPPORTED and b"zero key" in lib.mmdm_last_error()
    assert split_call(q, k, v, 64, valid, out_mode=1)[0] == ERR_ARG and b"out_mode" in lib.mmdm_last_error()
    # head size 96: refused as the unmasked call refuses it
    q, k, v = MC.operands(96, 17, 17)
    assert split_call(q, k, v, 96, plain=True)[0] == ERR_UNSUPPORTED
    plain_msg = lib.mmdm_last_error()
    assert split_call(q, k, v, 96, valid)[0] == ERR_UNSUPPORTED and lib.mmdm_last_error() == plain_msg and b"head dim 96" in plain_msg


# ---------------------------------------------------------------------------------------------------
# handle level, head sizes 64 and 128
# ---------------------------------------------------------------------------------------------------
def make(precision, dims, **kw):
    from mixermdm_amd.sampler import Sampler
    from mixermdm_amd.synthetic import synthetic_state_dict, synthetic_stats
    s = Sampler(d_heads=2, m_heads=2, max_batch=B, max_frames=40, precision=precision, **dims, **kw)
    s.load_state_dict(synthetic_state_dict(seed=7, std=0.05, bias_std=0.02, **dims))
    st = synthetic_stats()
    s.set_norm_stats(st["mean_hml"], st["std_hml"], st["mean_ih"], st["std_ih"])
    s.prepare()
    return s


@pytest.fixture(scope="module", params=[64, 128], ids=["dh64", "dh128"])
def pair(request):
    """(fp32 handle, fp32_split handle) with the same weights; every test leaves them without a mask."""
    dims = HANDLE_DIMS[request.param]
    a, b = make("fp32", dims), make("fp32_split", dims)
    yield a, b
    a.close()
    b.close()


def handle_masks():
    holes = torch.ones(B, T, dtype=torch.bool)
    holes[0, 3:6] = False
    holes[1, T - 7:] = False
    trail = torch.zeros(B, T, dtype=torch.bool)
    trail[:, :L_TRAIL] = True                   # the trailing mask of (a): L = 17 frames of every row
    return {"holes": holes, "trail": trail}


def module_inputs(which, seed):
    """(x, cond, x2, rows of the mask per item) of mmdm_module_forward: the denoisers on n = B rows, Mixer.forward on the CFG-doubled 2 B."""
    if which == 0:
        return MC.rnd(seed, B, T, 262), MC.rnd(seed + 1, B, 768), None, 1
    if which == 1:
        return MC.rnd(seed, B, T, 524), MC.rnd(seed + 1, B, 3 * 768), None, 1
    cond = MC.rnd(seed + 1, 2 * B, 8 * 768)
    cond[B:] = 0
    return MC.rnd(seed, 2 * B, T, 524), cond, MC.rnd(seed + 2, 2 * B, T, 524), 2


def forward(s, which, x, cond, x2, valid, reps):
    s.set_key_mask(None if valid is None else torch.cat([valid] * reps, 0))
    try:
        return s.module_forward(which, x, cond, 500, x2=x2).cpu()
    finally:
        s.set_key_mask(None)


@pytest.mark.parametrize("which", [0, 1])
def test_handle_trailing_mask_is_bitwise_the_shorter_call(pair, which):
    _, s = pair
    x, cond, _, _ = module_inputs(which, 40 + which)
    valid = torch.zeros(B, T, dtype=torch.bool)
    valid[:, :L_TRAIL] = True
    got = forward(s, which, x, cond, None, valid, 1)
    short = forward(s, which, x[:, :L_TRAIL].contiguous(), cond, None, None, 1)
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, :L_TRAIL], short)
    assert not torch.equal(got, forward(s, which, x, cond, None, None, 1)), "the mask changed nothing"


def _dist(got, ref):
    d = (got.double() - ref.double())
    return float(d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()), float(d.abs().max())


@pytest.mark.parametrize("which", [0, 1, 2])
def test_handle_masked_split_vs_masked_fp32(pair, which):
    """Measured on an MI355X (relative RMS / max error, fp32_split against fp32): see DESIGN 9a.  which = 2 takes the first input seed (56, 59, ...)
    at which the unmasked outputs of the two handles agree within the step tolerance 2e-4 + 2e-4 |ref| in every element -- the conditioning rule of
    tests/golden/make_golden_mask.py: N(0, 1) denoiser outputs can make an alignment ill-conditioned, and such a draw measures the input.  The seed
    found is printed: 56 at head size 64 (unmasked 2.96e-6 / 1.29e-4; holes 3.43e-6 / 1.45e-4; trail 3.68e-6 / 1.82e-4) and 59 at 128 (1.77e-6 / 8.49e-5;
    1.82e-6 / 1.76e-4; 3.01e-6 / 2.46e-4 against the 2.56e-4 allowed).  The masks are "holes" and the trailing mask of (a), 17 frames of every row."""
    f32, spl = pair
    seed = 50 + 3 * which
    for _ in range(16):
        x, cond, x2, reps = module_inputs(which, seed)
        ref0, got0 = forward(f32, which, x, cond, x2, None, reps), forward(spl, which, x, cond, x2, None, reps)
        if which != 2 or bool(((got0 - ref0).abs() <= STEP_ATOL + STEP_RTOL * ref0.abs()).all()):
            break
        seed += 3
    else:
        pytest.fail("no well-conditioned Mixer.forward input among 16 seeds")
    rms0, max0 = _dist(got0, ref0)
    print(f"which={which} seed={seed} unmasked: rel rms {rms0:.3e} max {max0:.3e}")
    for name, valid in handle_masks().items():
        ref, got = forward(f32, which, x, cond, x2, valid, reps), forward(spl, which, x, cond, x2, valid, reps)
        assert not torch.equal(got, got0), "the mask changed nothing"
        rms, mx = _dist(got, ref)
        print(f"which={which} seed={seed} {name}: rel rms {rms:.3e} max {mx:.3e}")
        assert rms <= 3.0 * rms0 + 1e-6 and mx <= 3.0 * max0 + 1e-6, (which, name, (rms, mx), (rms0, max0))


def test_split_masked_loop_graph_cache():
    """ddim4 on an fp32_split handle: graph replay == eager bitwise; masked -> unmasked -> masked with other values on ONE handle gives the
    stand-alone results each time, with two captures in all; set_key_mask(None) gives the never-masked bits."""
    s = make("fp32_split", DIMS)
    s.set_schedule("ddim4")
    cond, xT = MC.rnd(70, B, 8 * 768), MC.rnd(71, B, T, 524)
    m = handle_masks()
    va, vb = m["holes"], m["trail"]
    never = s.sample(cond, xT, use_graph=False)
    s.set_key_mask(va)
    eager_a = s.sample(cond, xT, use_graph=False)
    s.set_key_mask(vb)
    eager_b = s.sample(cond, xT, use_graph=False)
    s.set_key_mask(None)
    eager_0 = s.sample(cond, xT, use_graph=False)
    assert torch.isfinite(eager_a).all() and torch.isfinite(eager_b).all()
    assert torch.equal(eager_0, never)
    assert not torch.equal(eager_a, eager_b) and not torch.equal(eager_a, eager_0)
    assert s.graph_stats()[0] == 0
    s.set_key_mask(va)
    assert torch.equal(s.sample(cond, xT, use_graph=True), eager_a) and s.graph_stats()[0] == 1
    s.set_key_mask(None)
    assert torch.equal(s.sample(cond, xT, use_graph=True), eager_0) and s.graph_stats()[0] == 2
    s.set_key_mask(vb)
    assert torch.equal(s.sample(cond, xT, use_graph=True), eager_b) and s.graph_stats()[0] == 2      # other VALUES: no re-capture
    s.close()


def test_what_stays_refused():
    from mixermdm_amd._lib import load_library, MMDMError
    from mixermdm_amd.sampler import Sampler
    lib = load_library()
    one = np.ones((2, 16), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    small = dict(d_latent=64, d_ff=64, d_layers=1, m_latent=64, m_ff=64, m_layers=1)
    for prec, code in (("bf16", b"precision 1"), ("bf16_fp8", b"precision 3")):
        s = Sampler(d_heads=1, m_heads=1, max_batch=2, max_frames=16, precision=prec, **small)
        assert lib.mmdm_set_key_mask(s.h, ptr(one), 2, 16) == ERR_UNSUPPORTED and code in lib.mmdm_handle_error(s.h)
        s.close()
    s = Sampler(d_heads=2, m_heads=2, model1_kind=1, d1_latent=128, d1_ff=256, d1_layers=2, d1_heads=2, max_batch=2, max_frames=16, precision="fp32_split", **DIMS)
    assert lib.mmdm_set_key_mask(s.h, ptr(one), 2, 16) == ERR_UNSUPPORTED and b"MDM" in lib.mmdm_handle_error(s.h)
    s.close()
    s = Sampler(d_latent=64, d_ff=64, d_layers=1, d_heads=1, single_only=2, max_batch=2, max_frames=16, precision="fp32_split")
    assert lib.mmdm_set_key_mask(s.h, ptr(one), 2, 16) == ERR_UNSUPPORTED and b"single_only = 2" in lib.mmdm_handle_error(s.h)
    s.close()
    # the sizes of tests/golden/mask.npz (D = 16) have no fp32_split handle: why the reference goldens are not repeated in this mode
    with pytest.raises(MMDMError, match="multiples of 32"):
        Sampler(d_latent=16, d_ff=32, d_layers=2, d_heads=2, m_latent=16, m_ff=32, m_layers=2, m_heads=2, max_batch=2, max_frames=40, precision="fp32_split")
    # an fp32_split handle takes the mask -- and then refuses a ragged batch, as the fp32 handle does
    s = make("fp32_split", DIMS)
    s.set_schedule("ddim20")
    s.set_key_mask(one)
    cond = MC.rnd(2, 2, 8 * 768).to(dev())
    lens = (C.c_int * 2)(16, 9)
    xr = MC.rnd(3, 25, 524).to(dev())
    assert lib.mmdm_begin_ragged(s.h, _p(cond), _p(xr), 2, lens, s._s()) == ERR_UNSUPPORTED and b"ragged" in lib.mmdm_handle_error(s.h)
    s.set_key_mask(None)
    assert lib.mmdm_begin_ragged(s.h, _p(cond), _p(xr), 2, lens, s._s()) == 0
    s.close()

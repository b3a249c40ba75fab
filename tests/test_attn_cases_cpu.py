"""CPU: the reference and the input builders of the attention edge tests (tests/attn_cases.py) are what they claim to be -- checked
without the library, so that a GPU failure there points at a kernel and not at the yardstick."""
import math
import pytest
import torch
import torch.nn.functional as F

import attn_cases as AC

SHAPES = [(3, 49, 49, 3, 64), (3, 130, 130, 3, 128), (3, 17, 17, 3, 48)]


def _sdpa64(q, k, v, H, zero_key, causal, shift):
    nseq, Tq, HD = q.shape
    dh = HD // H
    idx = (torch.arange(nseq) + shift) % nseq
    sp = lambda t: t.double().reshape(nseq, -1, H, dh).transpose(1, 2)
    qh, kh, vh = sp(q), sp(k[idx]), sp(v[idx])
    if zero_key:
        z = torch.zeros(nseq, H, 1, dh, dtype=torch.float64)
        kh, vh = torch.cat([kh, z], 2), torch.cat([vh, z], 2)
    return F.scaled_dot_product_attention(qh, kh, vh, is_causal=causal).transpose(1, 2).reshape(nseq, Tq, HD)


@pytest.mark.parametrize("nseq,Tq,Tk,H,dh,zero_key,causal,shift", [(3, 17, 17, 3, 64, True, False, 0), (3, 17, 17, 3, 64, False, True, 0), (3, 33, 33, 2, 128, False, False, 1),
                                                                    (3, 16, 65, 3, 64, True, False, 1), (2, 65, 16, 3, 128, False, False, 0), (1, 1, 1, 1, 64, True, False, 0),
                                                                    (3, 17, 1, 3, 48, True, False, 2), (4, 1, 33, 2, 96, False, False, 3)])
def test_reference_is_torch_sdpa_in_float64(nseq, Tq, Tk, H, dh, zero_key, causal, shift):
    q, k, v = AC.normal(nseq, Tq, Tk, H, dh, seed=Tq + Tk)
    got = AC.ref_attention_f64(q, k, v, H, zero_key=zero_key, causal=causal, shift=shift)
    want = _sdpa64(q, k, v, H, zero_key, causal, shift)
    assert got.dtype == torch.float64 and got.shape == (nseq, Tq, H * dh)
    assert (got - want).abs().max().item() <= 1e-13
    # the plain fp32 evaluation is the same formula: fp32-close on N(0, 1) data
    f32 = AC.attention_f32_cpu(q, k, v, H, zero_key=zero_key, causal=causal, shift=shift)
    assert f32.dtype == torch.float32 and (f32.double() - got).abs().max().item() <= 5e-6


def test_reference_shift_and_zero_key_by_hand():
    """One head, two keys: the numbers written out."""
    q = torch.tensor([[[1.0, 0.0, 0.0, 0.0]], [[0.0, 2.0, 0.0, 0.0]]])
    k = torch.tensor([[[2.0, 0, 0, 0], [0, 0, 0, 0]], [[0, 4.0, 0, 0], [0, 1.0, 0, 0]]])
    v = torch.tensor([[[1.0, 2, 3, 4], [5, 6, 7, 8]], [[-1.0, 0, 1, 0], [0, 0, 0, 2]]])
    out = AC.ref_attention_f64(q, k, v, 1, zero_key=True, shift=1)
    w = torch.tensor([math.exp(0.0), math.exp(0.0), 1.0], dtype=torch.float64)          # sequence 0 against the keys of sequence 1: logits 0, 0; zero key 0
    want0 = (w[0] * v[1, 0].double() + w[1] * v[1, 1].double()) / w.sum()
    assert torch.allclose(out[0, 0], want0, atol=1e-15)
    w = torch.tensor([math.exp(0.0), math.exp(0.0)], dtype=torch.float64)               # sequence 1 against sequence 0: q . k = 0 for both keys
    out = AC.ref_attention_f64(q, k, v, 1, zero_key=False, shift=1)
    assert torch.allclose(out[1, 0], (v[0, 0].double() + v[0, 1].double()) / 2, atol=1e-15)


@pytest.mark.parametrize("nseq,Tq,Tk,H,dh", SHAPES)
@pytest.mark.parametrize("name", sorted(AC.EXTREMES))
def test_every_builder_respects_the_operand_bound_and_is_seeded(name, nseq, Tq, Tk, H, dh):
    a = AC.EXTREMES[name](nseq, Tq, Tk, H, dh, seed=3)
    b = AC.EXTREMES[name](nseq, Tq, Tk, H, dh, seed=3)
    for x, y, T in zip(a, b, (Tq, Tk, Tk)):
        assert x.dtype == torch.float32 and x.shape == (nseq, T, H * dh) and x.is_contiguous() and torch.equal(x, y)
        assert x.abs().max().item() <= AC.OPERAND_BOUND
        h = x.half()                                        # the split planes of the operand are finite fp16 numbers
        assert torch.isfinite(h).all() and torch.isfinite(((x - h.float()) * 2048).half()).all()


@pytest.mark.parametrize("nseq,Tq,Tk,H,dh", SHAPES + [(3, 300, 31, 3, 64)])
@pytest.mark.parametrize("step,per_stage", [(s, False) for s in AC.RAMP_KEY_STEPS] + [(s, True) for s in AC.RAMP_STAGE_STEPS])
def test_ramp_rises_by_the_stated_step(step, per_stage, nseq, Tq, Tk, H, dh):
    q, k, v = AC.ramp(nseq, Tq, Tk, H, dh, step, per_stage)
    lg = AC.logits_f64(q, k, H)
    for h in range(H):
        row = lg[:, h, AC.ramp_row(Tq, H, h), :]                                     # [nseq, Tk]
        d = row[:, 1:] - row[:, :-1]
        j = torch.arange(1, Tk)
        want = torch.where(j % AC.STAGE_KEYS == 0, step, 0.0) if per_stage else torch.full((Tk - 1,), step)
        # fp32 keys: the logit carries the rounding of c_j q (relative 2^-24 per element of a sum of dh terms of one sign)
        assert (d - want.double()).abs().max().item() <= 1e-6 * max(1.0, row.abs().max().item()), (h, (d - want).abs().max().item())
        assert abs(row[:, 0] + row[:, -1]).max().item() <= 1e-5 * max(1.0, row.abs().max().item()) + (step if per_stage else 0)      # centred on 0
    # every other row is a ramp too (keys are multiples of one vector): monotone in j
    d = lg[..., 1:] - lg[..., :-1]
    assert bool(((d >= -1e-9).all(-1) | (d <= 1e-9).all(-1)).all())


@pytest.mark.parametrize("nseq,Tq,Tk,H,dh", SHAPES + [(3, 300, 31, 3, 64), (3, 1, 33, 3, 128)])
def test_last_key_dominates_every_row(nseq, Tq, Tk, H, dh):
    q, k, v = AC.last_key_dominates(nseq, Tq, Tk, H, dh)
    for shift in range(nseq):
        lg = AC.logits_f64(q, k, H, shift)
        assert bool((lg.argmax(-1) == Tk - 1).all())
        assert abs(lg[..., -1] - AC.LAST_KEY_LOGIT).max().item() <= 0.3 * AC.LAST_KEY_LOGIT
        if Tk > 1:
            assert (lg[..., -1] - lg[..., :-1].max(-1).values).min().item() >= 5.0        # the rest is 150 x lighter at least
            assert lg[..., :-1].abs().max().item() <= 3.0


@pytest.mark.parametrize("nseq,Tq,Tk,H,dh", SHAPES)
@pytest.mark.parametrize("mag", AC.NEG_MAGS)
def test_all_negative_logits_are_below_minus_mag(mag, nseq, Tq, Tk, H, dh):
    q, k, v = AC.all_negative(nseq, Tq, Tk, H, dh, mag)
    for shift in range(nseq):
        lg = AC.logits_f64(q, k, H, shift)
        assert lg.max().item() <= -mag and lg.min().item() >= -2.0 * mag - 10
    out = AC.ref_attention_f64(q, k, v, H, zero_key=True)
    if mag >= 40:
        assert out.abs().max().item() <= Tk * math.exp(-mag) * v.abs().max().item()      # the zero key takes everything
    else:
        assert out.abs().max().item() >= 1e-3                                            # mag = 5: real keys still count
    assert AC.ref_attention_f64(q, k, v, H, zero_key=False).abs().max().item() >= 1e-2   # a normal softmax without it


@pytest.mark.parametrize("nseq,Tq,Tk,H,dh", SHAPES)
def test_peaked_rows_reach_the_stated_logit(nseq, Tq, Tk, H, dh):
    q, k, v = AC.peaked_rows(nseq, Tq, Tk, H, dh)
    lg = AC.logits_f64(q, k, H)
    assert abs(lg[1].abs().max().item() - AC.PEAK_LOGIT) <= 1e-3
    assert lg[0].abs().max().item() <= 8.0 and lg[2].abs().max().item() <= 8.0
    p = torch.softmax(lg[1], -1)
    assert p.max().item() >= 0.99                                                       # near one-hot rows exist


def test_fp32_yardstick_is_small_for_every_builder():
    """The softmax-extreme GPU tests allow a kernel a small multiple of the error of a plain fp32 CPU evaluation (attention_f32_cpu) on the
    same input; a builder whose yardstick is itself loose (> 1e-4) would make that test powerless and may not be in EXTREMES."""
    for name, build in sorted(AC.EXTREMES.items()):
        for dh in (64, 128):
            for T in (49, 130):
                q, k, v = build(3, T, T, 3, dh, seed=T + dh)
                for zk in (True, False):
                    y = (AC.attention_f32_cpu(q, k, v, 3, zero_key=zk).double() - AC.ref_attention_f64(q, k, v, 3, zero_key=zk)).abs().max().item()
                    assert y <= 1e-4, (name, dh, T, zk, y)

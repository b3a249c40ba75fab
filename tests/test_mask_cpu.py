"""CPU: the float64 masked-attention yardstick of the GPU tests (tests/mask_cases.py) IS the reference's function -- it agrees with
torch.nn.MultiheadAttention(add_zero_attn=True, batch_first=True) given key_padding_mask, in float64, to 1e-12 on the kernel test's inputs
(identity projections, so that the module computes the bare attention core)."""
import pytest
import torch

import mask_cases as MC


def _mha(E, H):
    m = torch.nn.MultiheadAttention(E, H, batch_first=True, add_zero_attn=True, dtype=torch.float64)
    with torch.no_grad():
        m.in_proj_weight.copy_(torch.cat([torch.eye(E, dtype=torch.float64)] * 3))
        m.in_proj_bias.zero_()
        m.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
        m.out_proj.bias.zero_()
    return m.eval()


@pytest.mark.parametrize("dh", MC.HEAD_SIZES)
@pytest.mark.parametrize("Tq,Tk", [(T, T) for T in MC.SELF_T] + list(MC.CROSS))
def test_masked_yardstick_is_multihead_attention_with_key_padding_mask(dh, Tq, Tk):
    q, k, v = MC.operands(dh, Tq, Tk)
    shift = 0 if Tq == Tk else 1
    mha = _mha(MC.H * dh, MC.H)
    idx = (torch.arange(MC.NSEQ) + shift) % MC.NSEQ
    for name, valid in MC.masks(Tk).items():
        ref = MC.ref_attention_masked_f64(q, k, v, MC.H, valid, shift=shift)
        with torch.no_grad():
            got = mha(q.double(), k.double()[idx], v.double()[idx], key_padding_mask=~valid[idx], need_weights=False)[0]
        assert torch.isfinite(got).all(), name
        assert (got - ref).abs().max().item() <= 1e-12, (name, (got - ref).abs().max().item())
        if name == "none":
            assert torch.count_nonzero(ref).item() == 0


def test_shared_mask_row_and_golden_inputs_are_reproducible():
    q, k, v = MC.operands(16, 17, 17)
    one = MC.masks(17, rows=1)["holes"]
    a = MC.ref_attention_masked_f64(q, k, v, MC.H, one)
    b = MC.ref_attention_masked_f64(q, k, v, MC.H, one.expand(MC.NSEQ, -1))
    assert torch.equal(a, b)
    g, inp, t = MC.load_mask_golden()
    assert inp("loop:holes:T33:x_T").shape == (2, 33, 524)
    m = t("mask:holes:T33")[..., 0] > 0.5
    assert int(m[0].sum()) - 1 == 29 and bool(m[0, 32]) and not bool(m[0, 29 - 26])      # count - 1 = 29 differs from the last valid frame 32

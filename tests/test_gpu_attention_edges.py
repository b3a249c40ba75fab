"""GPU: the attention forms at the tile edges of their kernels and on the logit patterns where an online softmax goes wrong.

Forms (entry point -> kernel, csrc/attn_f32.hip):
  f32        mmdm_attention_opts                      attn_mfma_kernel (16 keys per LDS stage, two stages in flight)
  planes3    mmdm_attention_planes, 3 bf16 planes     attn_qkp_kernel<DH, 3>       fp32-accurate scores, fp32 V
  planes1    mmdm_attention_planes, 1 bf16 plane      attn_qkp_kernel<DH, 1>       bf16 Q / K, fp32 V
  bf16       mmdm_attention_bf16                      attn_b32_kernel              32 keys per stage
  bf16_kc16  mmdm_attention_bf16 under attn_kc32 = 0  attn_qkp_kernel<DH, 1, true> the 16-key all-bf16 form
  split      mmdm_attention_split                     attn_qkp_kernel<DH, 2, true, true>   two fp16 planes per operand
Every comparison is against tests/attn_cases.py::ref_attention_f64 of the operands AS THE KERNEL RECEIVES THEM (bf16-rounded on the
device for the bf16 operands; the fp32 values for the fp32, 3-plane and split forms, whose planes hold them exactly / to 2^-22), over
EVERY output element.  Outputs are written into NaN-filled buffers with a guard band of rows behind them.

Tolerances on N(0, 1) inputs are the project's own (tests/test_gpu_kernels.py, tests/test_gpu_fp8.py), see TOL.  On the softmax-extreme
inputs the fp32-accurate forms are held to  max error <= MULT x yardstick + the same absolute floor, where the yardstick is the max
error of a plain fp32 CPU evaluation of the formula (attn_cases.attention_f32_cpu) on the same input: MULT = 4 covers the kernels'
log2-domain v_exp_f32 and their summation order.  The all-bf16 forms are held to 2^-9 max|V| x 1.05 + 1e-5, the bound of
test_attention_bf16_vs_float64_of_the_rounded_operands, on every input.
"""
import ctypes as C
import math
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_cases as AC            # noqa: E402

FORMS = ("f32", "planes3", "planes1", "bf16", "bf16_kc16", "split")
NSEQ, H = 3, 3                     # 9 (sequence, head) pairs: not a multiple of the 8 XCD ranges
GUARD = 8                          # NaN rows behind the output
PAD_ROWS = 7                       # rows of finite garbage behind the last sequence of a packed input
SELF_T = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129)
CROSS = ((1, 33), (17, 1), (16, 65), (65, 16), (64, 300), (300, 31))
REDUCED_T = (1, 16, 17, 33, 64, 65)
NO_ZERO_KEY, CAUSAL = 1, 2
MULT = 4.0
# form -> ("elem", atol, rtol): every element within atol + rtol |ref|; ("max", bound): max error; ("bf16",): 2^-9 max|V| x 1.05 + 1e-5
TOL = {"f32": ("elem", 3e-6, 1e-5), "planes3": ("elem", 2e-5, 1e-4), "split": ("elem", 2e-5, 1e-4), "planes1": ("max", 4e-6), "bf16": ("bf16",), "bf16_kc16": ("bf16",)}
FLOOR = {"f32": 3e-6, "planes3": 2e-5, "split": 2e-5, "planes1": 4e-6}          # the absolute part of the above, for the yardstick rule


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _p(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


class _Operand:
    """One of Q / K / V on the device: columns [col0, col0 + width) of the fp32 buffer `buf` ([rows, ld])."""
    def __init__(self, buf, col0, width):
        self.buf, self.col0, self.width, self.ld, self.rows = buf, col0, width, buf.shape[1], buf.shape[0]


def _place(q, k, v, packed):
    """CPU [nseq, T, HD] operands -> device buffers: one packed [nseq T + PAD_ROWS, 3 HD] projection (column slices, garbage rows behind
    the last sequence) or three exactly sized ones."""
    d = _dev()
    nseq, Tq, HD = q.shape
    if packed:
        assert k.shape[1] == Tq
        buf = torch.cat([torch.cat([q, k, v], -1).reshape(nseq * Tq, 3 * HD), 50.0 * torch.randn(PAD_ROWS, 3 * HD, generator=torch.Generator().manual_seed(1))]).to(d)
        return [_Operand(buf, i * HD, HD) for i in range(3)]
    return [_Operand(t.reshape(-1, HD).to(d).contiguous(), 0, HD) for t in (q, k, v)]


def run_form(form, q, k, v, dh, shift=0, flags=0, packed=False, out_mode=0):
    """Runs one attention form on CPU fp32 operands q [nseq, Tq, H dh], k / v [nseq, Tk, H dh].  Returns (out, (qr, kr, vr)): the
    [nseq, Tq, HD] result (fp32 / bf16; out_mode 2: the [2, nseq, Tq, HD] fp16 planes) after the guard band was checked, and the CPU
    fp32 values of the operands as the kernel received them."""
    from mixermdm_amd import ops
    from mixermdm_amd._lib import load_library, check, diag
    lib, d = load_library(), _dev()
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    heads = HD // dh
    oq, ok, ov = _place(q, k, v, packed)
    rows_o = nseq * Tq
    odt = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}[out_mode]
    out = torch.full(((2 if out_mode == 2 else 1) * rows_o + GUARD, HD), float("nan"), device=d, dtype=odt)
    tail = (flags, nseq, Tq, Tk, heads, dh, shift, None)
    win = lambda o, t: t[:nseq * (Tq if o is oq else Tk), o.col0:o.col0 + HD].float().cpu().reshape(nseq, -1, HD)      # the operand's values, from a tensor shaped like o.buf
    if form == "f32":
        check(lib.mmdm_attention_opts(_p(oq.buf, oq.col0), oq.ld, _p(ok.buf, ok.col0), ok.ld, _p(ov.buf, ov.col0), ov.ld, _p(out), HD, out_mode, *tail))
        recv = (win(oq, oq.buf), win(ok, ok.buf), win(ov, ov.buf))
    elif form in ("planes3", "planes1"):
        if form == "planes3":
            qp, kp = ops.bf16_split3(oq.buf), (ops.bf16_split3(ok.buf) if ok.buf is not oq.buf else None)
            kp = qp if kp is None else kp
            assert torch.equal(qp.float().sum(0), oq.buf) and torch.equal(kp.float().sum(0), ok.buf)          # the three planes hold the fp32 values exactly
            recv = (win(oq, oq.buf), win(ok, ok.buf), win(ov, ov.buf))
        else:
            qp = oq.buf.bfloat16()[None]
            kp = qp if ok.buf is oq.buf else ok.buf.bfloat16()[None]
            recv = (win(oq, qp[0]), win(ok, kp[0]), win(ov, ov.buf))
        check(lib.mmdm_attention_planes(_p(qp, oq.col0), oq.ld, oq.rows * oq.ld, _p(kp, ok.col0), ok.ld, ok.rows * ok.ld, qp.shape[0],
                                        _p(ov.buf, ov.col0), ov.ld, _p(out), HD, out_mode, *tail))
    elif form in ("bf16", "bf16_kc16"):
        qb = oq.buf.bfloat16()
        kb = qb if ok.buf is oq.buf else ok.buf.bfloat16()
        vb = qb if ov.buf is oq.buf else ov.buf.bfloat16()
        recv = (win(oq, qb), win(ok, kb), win(ov, vb))
        try:
            diag("attn_kc32", 0 if form == "bf16_kc16" else 1)
            check(lib.mmdm_attention_bf16(_p(qb, oq.col0), oq.ld, _p(kb, ok.col0), ok.ld, _p(vb, ov.col0), ov.ld, _p(out), HD, out_mode, *tail))
        finally:
            diag("attn_kc32", 1)
    elif form == "split":
        qs = ops.split_f32(oq.buf)
        ks = qs if ok.buf is oq.buf else ops.split_f32(ok.buf)
        vs = qs if ov.buf is oq.buf else ops.split_f32(ov.buf)
        recv = (win(oq, oq.buf), win(ok, ok.buf), win(ov, ov.buf))          # h + l / 2048 holds x to 2^-22 relative: the fp32 values are the operands
        check(lib.mmdm_attention_split(_p(qs, oq.col0), oq.ld, oq.rows * oq.ld, _p(ks, ok.col0), ok.ld, ok.rows * ok.ld, _p(vs, ov.col0), ov.ld, ov.rows * ov.ld,
                                       _p(out), HD, out_mode, *tail))
    else:
        raise KeyError(form)
    torch.cuda.synchronize()
    n_out = (2 if out_mode == 2 else 1) * rows_o
    assert bool(torch.isnan(out[n_out:]).all()), f"{form}: wrote behind row Tq of the last sequence"
    res = out[:n_out]
    return (res.reshape(2, nseq, Tq, HD) if out_mode == 2 else res.reshape(nseq, Tq, HD)), recv


def _errors(form, got, ref, vr):
    """(max error, message or None) of one fp32 result under the form's N(0, 1) tolerance."""
    g = got.detach().cpu().double()
    if not bool(torch.isfinite(g).all()):
        return float("nan"), f"{int((~torch.isfinite(g)).sum())} non-finite outputs"
    d = (g - ref).abs()
    err = d.max().item()
    tol = TOL[form]
    if tol[0] == "elem":
        bad = d > tol[1] + tol[2] * ref.abs()
        return err, (f"{int(bad.sum())}/{bad.numel()} elements outside atol={tol[1]} rtol={tol[2]}, max err {err:.3e}" if bool(bad.any()) else None)
    bound = tol[1] if tol[0] == "max" else 2.0 ** -9 * vr.abs().max().item() * 1.05 + 1e-5
    return err, (f"max err {err:.3e} > {bound:.3e}" if err > bound else None)


def _sweep_cases():
    for shift in (0, 1):
        for T in SELF_T:
            yield T, T, shift, 0
        for Tq, Tk in CROSS:
            yield Tq, Tk, shift, 0
        for fl in (NO_ZERO_KEY, NO_ZERO_KEY | CAUSAL):
            for T in REDUCED_T:
                yield T, T, shift, fl


SWEEP = list(_sweep_cases())


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", range(len(SWEEP)), ids=["Tq%d-Tk%d-shift%d-flags%d" % c for c in SWEEP])
def test_length_sweep(n, form, dh):
    """A partial, an exactly full and a just-over LDS stage; one, two, three stages (pipeline prologue / epilogue with fewer chunks than
    stages); the wave (16) and workgroup (64) edges of Tq; Tq != Tk as every cross attention of a ragged batch has it -- with the zero
    key for both kv_seq_shift values, and a reduced set without it and with the causal mask.

    The all-bf16 forms at Tq17-Tk1 and Tq2-Tk2 are the cases that showed that their kernels must take the row sum over the bf16-ROUNDED
    probabilities (RNE to bf16 errs by up to 2^-8, and with an unrounded sum a row that one key dominates carried all of it: 8.0e-3
    against the 7.3e-3 allowed at Tk = 1); with the rounded sum the weights of a row sum to one and these rows are exact."""
    Tq, Tk, shift, flags = SWEEP[n]
    q, k, v = AC.normal(NSEQ, Tq, Tk, H, dh, seed=1000 * n + Tq)
    got, (qr, kr, vr) = run_form(form, q, k, v, dh, shift=shift, flags=flags, packed=(Tq == Tk))
    ref = AC.ref_attention_f64(qr, kr, vr, H, zero_key=not flags & NO_ZERO_KEY, causal=bool(flags & CAUSAL), shift=shift)
    err, msg = _errors(form, got, ref, vr)
    print(f"attention length sweep {form} dh={dh} Tq={Tq} Tk={Tk} shift={shift} flags={flags}: max error {err:.3e}")
    assert msg is None, f"{form} dh={dh} Tq={Tq} Tk={Tk} shift={shift} flags={flags}: {msg}"


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("form", [f for f in FORMS if f != "f32"])
def test_output_modes_at_the_edges(form, dh):
    """out_mode 1 is .bfloat16() of the fp32 output and out_mode 2 its fp16 split planes, bit for bit, at a wave edge, a workgroup edge
    and a just-over stage."""
    from mixermdm_amd import ops
    for T in (17, 64, 129):
        q, k, v = AC.normal(NSEQ, T, T, H, dh, seed=T)
        f32, _ = run_form(form, q, k, v, dh, shift=1, packed=True)
        b16, _ = run_form(form, q, k, v, dh, shift=1, packed=True, out_mode=1)
        assert torch.equal(b16, f32.bfloat16()), (form, dh, T, "bf16 output")
        pl, _ = run_form(form, q, k, v, dh, shift=1, packed=True, out_mode=2)
        assert torch.equal(pl, ops.split_f32(f32.contiguous())), (form, dh, T, "split-plane output")


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(AC.EXTREMES))
def test_softmax_extremes(name, form, dh):
    """Every builder of attn_cases.EXTREMES at T = 49 and 130 (a partial last stage in the 16- and the 32-key kernels), zero key on and
    off.  Measured on an MI355X (LAB_NOTES.md, "attention edge tests"): (kernel error - floor) / yardstick stays below 4 for every
    builder and every fp32-accurate form (worst: 1.38, the fp32 kernel at dh 128 on ramp_key_1).

    peaked_rows (near one-hot rows) is the builder that needs the all-bf16 kernels' row sum over the rounded probabilities: 2.5e-2
    against the 2.2e-2 allowed before, see test_length_sweep."""
    failures, build = [], AC.EXTREMES[name]
    shift = 0 if name.startswith(("ramp", "peaked")) else 1             # ramp / peaked_rows are built per sequence; the others hold for every sequence pair
    wy, we, wr = 0.0, 0.0, 0.0
    for T in (49, 130):
        q, k, v = build(NSEQ, T, T, H, dh, seed=T + dh)
        for zk in (True, False):
            got, (qr, kr, vr) = run_form(form, q, k, v, dh, shift=shift, flags=0 if zk else NO_ZERO_KEY, packed=True)
            ref = AC.ref_attention_f64(qr, kr, vr, H, zero_key=zk, shift=shift)
            g = got.cpu().double()
            case = f"{name} T={T} zero_key={zk}"
            if not bool(torch.isfinite(g).all()):
                failures.append(f"{case}: non-finite output")
                continue
            err = (g - ref).abs().max().item()
            if form in FLOOR:
                yard = (AC.attention_f32_cpu(qr, kr, vr, H, zero_key=zk, shift=shift).double() - ref).abs().max().item()
                bound = MULT * yard + FLOOR[form]
                wr = max(wr, (err - FLOOR[form]) / max(yard, 1e-30))
            else:
                yard = float("nan")
                bound = 2.0 ** -9 * vr.abs().max().item() * 1.05 + 1e-5
            wy, we = max(wy, yard) if yard == yard else wy, max(we, err)
            if err > bound:
                failures.append(f"{case}: max err {err:.3e} > {bound:.3e} (fp32 CPU yardstick {yard:.3e})")
            if zk and name == "all_negative_40" and g.abs().max().item() > 1e-12:      # the real keys weigh <= T e^-40 = 6e-16 together
                failures.append(f"{case}: |out| = {g.abs().max().item():.3e}, the zero key should take everything")
    line = (f"{name:20s} fp32-CPU yardstick {wy:.2e}  kernel {we:.2e}  (err - floor) / yardstick {wr:.2f}" if form in FLOOR else
            f"{name:20s} kernel {we:.2e}  (bound 2^-9 max|V| x 1.05 + 1e-5 = {bound:.2e})")
    print(f"attention softmax extremes {form} dh={dh}: {line}")
    assert not failures, f"{form} dh={dh}: " + "; ".join(failures)


@pytest.mark.parametrize("dh", [48, 96])
def test_padded_head_sizes_with_the_zero_key(dh):
    """Head widths between the two template sizes run zero-padded on the fp32 MFMA kernel: with the zero key, at a full / just-over stage and
    a just-over workgroup, on inputs where any leak of a padded column into the scores shows (all_negative: the logits decide between the
    zero key and the real ones)."""
    failures = []
    for T in (16, 17, 65):
        for name, build in (("normal", AC.normal), ("all_negative_5", AC.EXTREMES["all_negative_5"]), ("all_negative_40", AC.EXTREMES["all_negative_40"])):
            q, k, v = build(NSEQ, T, T, H, dh, seed=T)
            for shift in (0, 1):
                got, (qr, kr, vr) = run_form("f32", q, k, v, dh, shift=shift, packed=True)
                ref = AC.ref_attention_f64(qr, kr, vr, H, zero_key=True, shift=shift)
                case = f"{name} T={T} shift={shift}"
                if name == "normal":
                    err, msg = _errors("f32", got, ref, vr)
                else:
                    err = (got.cpu().double() - ref).abs().max().item()
                    yard = (AC.attention_f32_cpu(qr, kr, vr, H, zero_key=True, shift=shift).double() - ref).abs().max().item()
                    msg = None if err <= MULT * yard + FLOOR["f32"] else f"max err {err:.3e} > {MULT} x {yard:.3e} + {FLOOR['f32']}"
                    if name == "all_negative_40" and not got.abs().max().item() <= 1e-12:
                        msg = f"|out| = {got.abs().max().item():.3e}, the zero key should take everything"
                if msg:
                    failures.append(f"{case}: {msg}")
    assert not failures, f"dh={dh}: " + "; ".join(failures)


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("shift", [0, 6])
def test_ragged_f32_kernel_at_the_edges(dh, shift):
    """mmdm_attention_ragged_f32 on sequences at every stage / wave / workgroup edge in ONE launch: bitwise the uniform kernel on each
    sequence alone, and within the fp32 tolerance of the float64 reference.  (shift 6: sequence s attends to sequence s + 6, of the
    same length.)"""
    from mixermdm_amd._lib import load_library, check
    lib, d = load_library(), _dev()
    HD = H * dh
    lens = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2, 129] if shift == 0 else [1, 16, 17, 33, 65, 129] * 2
    nseq, total = len(lens), sum(lens)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    g = torch.Generator().manual_seed(dh + shift)
    qkv = torch.randn(total + PAD_ROWS, 3 * HD, generator=g)
    qkv[total:] *= 50.0
    qd = qkv.to(d)
    out = torch.full((total + GUARD, HD), float("nan"), device=d)
    d_off, d_len = torch.from_numpy(off).to(d), torch.tensor(lens, dtype=torch.int32, device=d)
    check(lib.mmdm_attention_ragged_f32(_p(qd), 3 * HD, _p(qd, HD), 3 * HD, _p(qd, 2 * HD), 3 * HD, _p(out), HD, nseq, _p(d_off), _p(d_len), max(lens), total, H, dh, shift, None))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:total]).all()) and bool(torch.isnan(out[total:]).all())
    for s, (o, t) in enumerate(zip(off.tolist(), lens)):
        ks = (s + shift) % nseq
        ko = int(off[ks])
        assert lens[ks] == t
        alone = torch.full((t + GUARD, HD), float("nan"), device=d)
        qs, kvs = qd[o:o + t].contiguous(), qd[ko:ko + t].contiguous()
        check(lib.mmdm_attention_f32(_p(qs), 3 * HD, _p(kvs, HD), 3 * HD, _p(kvs, 2 * HD), 3 * HD, _p(alone), HD, 1, t, t, H, dh, 0, None))
        torch.cuda.synchronize()
        assert bool(torch.isnan(alone[t:]).all())
        assert torch.equal(out[o:o + t], alone[:t]), (s, t)
        ref = AC.ref_attention_f64(qkv[None, o:o + t, :HD], qkv[None, ko:ko + t, HD:2 * HD], qkv[None, ko:ko + t, 2 * HD:], H)
        err, msg = _errors("f32", out[None, o:o + t], ref, None)
        assert msg is None, (s, t, msg)

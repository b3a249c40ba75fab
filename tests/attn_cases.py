"""Inputs and the reference of the attention edge tests (tests/test_gpu_attention_edges.py, tests/test_attn_cases_cpu.py).

ref_attention_f64 is the one float64 statement of what every attention entry point computes; the builders make seeded fp32 CPU operands
q [nseq, Tq, H*dh], k / v [nseq, Tk, H*dh] whose LOGITS (q . k / sqrt(dh), natural-log units) have a stated pattern -- the patterns on
which an online softmax goes wrong: a running maximum that moves in every 16-key stage by less and by more than the kernels' deferral
thresholds, a single dominant key in the last, partial stage, rows on which only the zero key counts.

Every operand a builder returns satisfies |x| <= OPERAND_BOUND = 256 (asserted in the builder).  The fp16 split planes hold x as
h = fp16(x), l = fp16((x - h) * 2048): h needs |x| < 65504, and |l| <= 2048 * ulp_fp16(x) / 2 <= |x|, so 256 is 2^-8 of the range of
either plane; bf16 has fp32's range.  Pure torch on the CPU: nothing here touches the library under test.
"""
import math
import torch

OPERAND_BOUND = 256.0
RAMP_KEY_STEPS = (0.25, 1.0, 3.0)        # logit rise per key
RAMP_STAGE_STEPS = (4.0, 12.0, 30.0)     # logit rise per 16-key stage (log 16 = 2.77: the split kernel defers its maximum by 4 bits, the others by 8 = 5.5)
STAGE_KEYS = 16
NEG_MAGS = (5.0, 40.0)
PEAK_LOGIT = 40.0
LAST_KEY_LOGIT = 12.0


def ref_attention_f64(q, k, v, H, *, zero_key=True, causal=False, shift=0):
    """float64 softmax attention.  q [nseq, Tq, H*dh], k / v [nseq, Tk, H*dh] (any float dtype; used at their values); query sequence s
    attends to the keys / values of sequence (s + shift) % nseq; zero_key appends nn.MultiheadAttention's add_zero_attn key (logit 0,
    value 0); causal (Tq == Tk, no zero key) masks key > query.  Returns float64 [nseq, Tq, H*dh]."""
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    dh = HD // H
    assert HD == H * dh and k.shape == (nseq, Tk, HD) and v.shape == (nseq, Tk, HD)
    assert not causal or (Tq == Tk and not zero_key)
    idx = (torch.arange(nseq) + shift) % nseq
    qh = q.detach().cpu().double().reshape(nseq, Tq, H, dh).transpose(1, 2)
    kh = k.detach().cpu().double()[idx].reshape(nseq, Tk, H, dh).transpose(1, 2)
    vh = v.detach().cpu().double()[idx].reshape(nseq, Tk, H, dh).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    if causal:
        s = s.masked_fill(torch.ones(Tq, Tk, dtype=torch.bool).triu(1), float("-inf"))
    if zero_key:
        s = torch.cat([s, torch.zeros(nseq, H, Tq, 1, dtype=torch.float64)], -1)
        vh = torch.cat([vh, torch.zeros(nseq, H, 1, dh, dtype=torch.float64)], 2)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(nseq, Tq, HD)


def attention_f32_cpu(q, k, v, H, *, zero_key=True, causal=False, shift=0):
    """The same formula evaluated plainly in fp32 (torch matmul / softmax on the CPU): its distance to ref_attention_f64 is the yardstick
    of what fp32 arithmetic can deliver on an input, independent of any kernel."""
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    dh = HD // H
    idx = (torch.arange(nseq) + shift) % nseq
    qh = q.float().reshape(nseq, Tq, H, dh).transpose(1, 2)
    kh = k.float()[idx].reshape(nseq, Tk, H, dh).transpose(1, 2)
    vh = v.float()[idx].reshape(nseq, Tk, H, dh).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * torch.tensor(1.0 / math.sqrt(dh), dtype=torch.float32)
    if causal:
        s = s.masked_fill(torch.ones(Tq, Tk, dtype=torch.bool).triu(1), float("-inf"))
    if zero_key:
        s = torch.cat([s, torch.zeros(nseq, H, Tq, 1)], -1)
        vh = torch.cat([vh, torch.zeros(nseq, H, 1, dh)], 2)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(nseq, Tq, HD)


def logits_f64(q, k, H, shift=0):
    """[nseq, H, Tq, Tk] float64 logits of the real keys."""
    nseq, Tq, HD = q.shape
    dh = HD // H
    idx = (torch.arange(nseq) + shift) % nseq
    qh = q.double().reshape(nseq, Tq, H, dh).transpose(1, 2)
    kh = k.double()[idx].reshape(nseq, -1, H, dh).transpose(1, 2)
    return qh @ kh.transpose(-1, -2) / math.sqrt(dh)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bounded(q, k, v):
    m = max(q.abs().max().item(), k.abs().max().item(), v.abs().max().item())
    assert m <= OPERAND_BOUND and all(torch.isfinite(t).all() for t in (q, k, v)), f"operand magnitude {m} beyond the stated bound {OPERAND_BOUND}"
    return q.contiguous(), k.contiguous(), v.contiguous()


def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, -1)        # a view: writes go through


def normal(nseq, Tq, Tk, H, dh, seed=0):
    g = _gen(seed)
    return _bounded(torch.randn(nseq, Tq, H * dh, generator=g), torch.randn(nseq, Tk, H * dh, generator=g), torch.randn(nseq, Tk, H * dh, generator=g))


def ramp_row(Tq, H, h=0):
    """The query row of head h whose logits are the promised ramp (a different wave / lane position per head)."""
    return (5 + 7 * h) % Tq


def ramp(nseq, Tq, Tk, H, dh, step, per_stage=False, seed=0):
    """Key j of head h is c_j * (query ramp_row(Tq, H, h) of head h of the SAME sequence), with c_j such that this row's logit against
    key j is step * (j - (Tk - 1) / 2) (per key) or step * (j // 16 - (nstages - 1) / 2) (per 16-key stage): a running maximum that
    moves in every stage.  The other query rows see c_j * (q' . q) / sqrt(dh): ramps of about 1 / sqrt(dh) of the step with either
    sign (a falling ramp never moves the maximum after the first stage).  Meant for shift = 0 (the keys of sequence s are built from
    the queries of sequence s)."""
    g = _gen(seed)
    q = torch.randn(nseq, Tq, H * dh, generator=g)
    v = torch.randn(nseq, Tk, H * dh, generator=g)
    k = torch.empty(nseq, Tk, H * dh)
    j = torch.arange(Tk, dtype=torch.float64)
    pos = (j // STAGE_KEYS - ((Tk - 1) // STAGE_KEYS) / 2) if per_stage else (j - (Tk - 1) / 2)
    for h in range(H):
        qv = _heads(q, H)[:, ramp_row(Tq, H, h), h, :].double()                       # [nseq, dh]
        c = step * pos[None, :] * math.sqrt(dh) / (qv * qv).sum(-1, keepdim=True)    # [nseq, Tk]
        _heads(k, H)[:, :, h, :] = (c[:, :, None] * qv[:, None, :]).float()
    return _bounded(q, k, v)


def last_key_dominates(nseq, Tq, Tk, H, dh, seed=0):
    """Every query is u + 0.3 N(0, 1) with a fixed sign vector u per head; keys 0 .. Tk - 2 are 0.3 N(0, 1) (logits of order 0.3), key
    Tk - 1 is (LAST_KEY_LOGIT / sqrt(dh)) u: logit about LAST_KEY_LOGIT for every query of every sequence -- the only large logit sits in
    the last, possibly partial stage."""
    g = _gen(seed)
    u = torch.where(torch.rand(1, 1, H * dh, generator=g) < 0.5, -1.0, 1.0)
    q = u + 0.3 * torch.randn(nseq, Tq, H * dh, generator=g)
    k = 0.3 * torch.randn(nseq, Tk, H * dh, generator=g)
    k[:, Tk - 1, :] = u[0, 0] * (LAST_KEY_LOGIT / math.sqrt(dh))
    v = torch.randn(nseq, Tk, H * dh, generator=g)
    return _bounded(q, k, v)


def all_negative(nseq, Tq, Tk, H, dh, mag, seed=0):
    """Queries u + 0.2 N(0, 1), keys -b u + 0.2 N(0, 1) with the smallest b of a fixed geometric sequence for which EVERY real logit of
    every (query sequence, key sequence) pair is <= -mag.  With the zero key the real keys together weigh <= Tk e^-mag against its 1
    (mag = 40: the output is 0 to 1e-15; mag = 5: a genuine mixture); without it a plain softmax of logits near -mag."""
    g = _gen(seed)
    u = torch.where(torch.rand(1, 1, H * dh, generator=g) < 0.5, -1.0, 1.0)
    q = u + 0.2 * torch.randn(nseq, Tq, H * dh, generator=g)
    kn = 0.2 * torch.randn(nseq, Tk, H * dh, generator=g)
    v = torch.randn(nseq, Tk, H * dh, generator=g)
    b = (mag + 1.0) / math.sqrt(dh)
    for _ in range(200):
        k = kn - b * u
        if max(logits_f64(q, k, H, s).max().item() for s in range(nseq)) <= -mag:
            return _bounded(q, k, v)
        b *= 1.03
    raise AssertionError("all_negative: no scale found")


def peaked_rows(nseq, Tq, Tk, H, dh, seed=0):
    """N(0, 1) operands with sequence 1 (queries and keys alike, values x 2.5) scaled so that the largest |logit| of sequence 1 against
    itself is PEAK_LOGIT: near one-hot softmax rows next to ordinary ones."""
    q, k, v = normal(nseq, Tq, Tk, H, dh, seed)
    s = 1 % nseq
    f = math.sqrt(PEAK_LOGIT / logits_f64(q[s:s + 1], k[s:s + 1], H).abs().max().item())
    q[s] *= f
    k[s] *= f
    v[s] *= 2.5
    return _bounded(q, k, v)


# name -> builder(nseq, Tq, Tk, H, dh, seed): the softmax-extreme cases of tests/test_gpu_attention_edges.py
EXTREMES = {}
for _s in RAMP_KEY_STEPS:
    EXTREMES[f"ramp_key_{_s:g}"] = (lambda st: lambda nseq, Tq, Tk, H, dh, seed=0: ramp(nseq, Tq, Tk, H, dh, st, False, seed))(_s)
for _s in RAMP_STAGE_STEPS:
    EXTREMES[f"ramp_stage_{_s:g}"] = (lambda st: lambda nseq, Tq, Tk, H, dh, seed=0: ramp(nseq, Tq, Tk, H, dh, st, True, seed))(_s)
EXTREMES["last_key_dominates"] = last_key_dominates
for _m in NEG_MAGS:
    EXTREMES[f"all_negative_{_m:g}"] = (lambda mg: lambda nseq, Tq, Tk, H, dh, seed=0: all_negative(nseq, Tq, Tk, H, dh, mg, seed))(_m)
EXTREMES["peaked_rows"] = peaked_rows

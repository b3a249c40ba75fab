"""Key-padding-mask test helpers (tests/test_mask_cpu.py, tests/test_gpu_mask.py): the float64 yardstick, the masks of the kernel grid and
the seeded inputs of tests/golden/mask.npz.  Pure torch on the CPU: nothing here touches the library under test."""
import math
import os
import numpy as np
import torch

NSEQ, H = 3, 3
HEAD_SIZES = (64, 128, 96, 16)
SELF_T = (1, 16, 17, 33, 65)
CROSS = ((17, 1), (16, 65), (65, 16))            # (Tq, Tk), kv_seq_shift = 1


def ref_attention_masked_f64(q, k, v, H, key_valid, *, shift=0):
    """tests/attn_cases.py::ref_attention_f64 (zero key) plus a key mask: key_valid bool [rows, Tk], True = the key exists; key sequence
    kvseq = (s + shift) % nseq reads row kvseq % rows; a masked key gets the logit -inf, the zero key never does."""
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    dh = HD // H
    idx = (torch.arange(nseq) + shift) % nseq
    qh = q.detach().cpu().double().reshape(nseq, Tq, H, dh).transpose(1, 2)
    kh = k.detach().cpu().double()[idx].reshape(nseq, Tk, H, dh).transpose(1, 2)
    vh = v.detach().cpu().double()[idx].reshape(nseq, Tk, H, dh).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh)
    kv = key_valid[idx % key_valid.shape[0]]                                   # [nseq, Tk]
    s = s.masked_fill(~kv[:, None, None, :], float("-inf"))
    s = torch.cat([s, torch.zeros(nseq, H, Tq, 1, dtype=torch.float64)], -1)
    vh = torch.cat([vh, torch.zeros(nseq, H, 1, dh, dtype=torch.float64)], 2)
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(nseq, Tq, HD)


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def operands(dh, Tq, Tk, seed=7):
    HD = H * dh
    return rnd(seed, NSEQ, Tq, HD), rnd(seed + 1, NSEQ, Tk, HD), rnd(seed + 2, NSEQ, Tk, HD)


def masks(Tk, rows=NSEQ):
    """name -> bool [rows, Tk] (True = valid) of the kernel grid: all valid; trailing with 1, 15, 16, 17 and Tk - 1 valid keys where they fit
    (one count per row, cycling); random holes with key 0 invalid; the whole middle chunk (keys 16-31) invalid at Tk = 65; every key invalid."""
    out = {"all": torch.ones(rows, Tk, dtype=torch.bool)}
    counts = [c for c in (1, 15, 16, 17, Tk - 1) if 1 <= c <= Tk]
    for i in range(0, len(counts), rows):
        m = torch.zeros(rows, Tk, dtype=torch.bool)
        for r in range(rows):
            m[r, :counts[(i + r) % len(counts)]] = True
        out["trail%d" % (i // rows)] = m
    g = torch.Generator().manual_seed(100 + Tk)
    m = torch.rand(rows, Tk, generator=g) < 0.6
    m[:, 0] = False
    out["holes"] = m
    if Tk == 65:
        m = torch.ones(rows, Tk, dtype=torch.bool)
        m[:, 16:32] = False
        out["chunk"] = m
    out["none"] = torch.zeros(rows, Tk, dtype=torch.bool)
    return out


# ---- tests/golden/mask.npz -------------------------------------------------------------------------
def load_mask_golden():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask.npz"))
    g = {k: d[k] for k in d.files}

    def inp(name):
        """The seeded input the generator drew: rnd(seed, *shape) of the recorded [seed, *shape]."""
        spec = [int(v) for v in g["in:" + name]]
        return rnd(spec[0], *spec[1:])

    def t(key):
        return torch.from_numpy(np.asarray(g[key]))

    return g, inp, t

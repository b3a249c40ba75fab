"""Cases of the InterCLIP evaluator tests (tests/golden/evaluator.npz): redraw helpers and a plain torch restatement of the evaluator
(src/evaluation/models.py), runnable in fp32 and float64 (test infrastructure, shared by test_evaluator_cpu.py and test_gpu_evaluator.py).

The fixture stores no weights and no inputs: weights are re-drawn by the rule of tests/golden/make_golden.py::reinit (crc32 of the parameter
name + seed), inputs are rnd(seed, *shape) -- the same seeded CPU generators on every box."""
import json
import os
import zlib
import numpy as np
import torch
import torch.nn.functional as F

from parity_tol import YARD_FACTOR, YARD_FLOOR, _quant, record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator.npz")
QS, QN = (0.5, 0.99, 1.0), ("p50", "p99", "max")
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        d = np.load(GOLDEN)
        _CACHE["g"] = {k: d[k] for k in d.files}
    return _CACHE["g"]


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def case_cfg(g, case):
    """The cfg mapping of a case (the keys of configs/eval.yaml that the evaluator reads)."""
    c = json.loads(str(g[f"{case}:cfg"]))
    return {"INPUT_DIM": 258, "ACTIVATION": "gelu", "DROPOUT": 0.1, "EXTENDED": False, **c}


def redraw(names_shapes, seed, std):
    """state_dict by the rule of make_golden.reinit: parameter `name` = randn(shape, Generator(crc32(name) + seed)) * std.  The pe buffer is left out."""
    sd = {}
    for name, shape in names_shapes:
        if name.endswith("sequence_pos_encoder.pe"):
            continue
        gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) + int(seed))
        sd[name] = torch.randn(tuple(shape), generator=gen) * std
    return sd


def case_names_shapes(g, case):
    return [(n, tuple(s)) for n, s in json.loads(str(g[f"{case}:state_dict"]))]


def case_weights(g, case):
    """Redrawn weights of a case; cached per distinct (name, shape) list, since several cases share it."""
    key = str(g[f"{case}:state_dict"])
    if key not in _CACHE:
        _CACHE[key] = redraw(case_names_shapes(g, case), int(g["seed"]), float(g["std"]))
    return _CACHE[key]


def case_motions(g, case):
    """(motions [B, Tpad, C] fp32, lens list)"""
    seed, *shape = [int(v) for v in g[f"{case}:motions"]]
    return rnd(seed, *shape), [int(v) for v in g[f"{case}:lens"]]


def pe_table(D, max_len):
    pe = torch.zeros(max_len, D)
    pos = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div = torch.exp(torch.arange(0, D, 2).float() * (-np.log(10000.0) / D))
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _encoder_layer(W, p, x, H, key_pad):
    """Post-norm nn.TransformerEncoderLayer(batch_first=True), eval mode, exact GELU; key_pad [B, T] bool (True = ignore) or None."""
    B, T, D = x.shape
    dh = D // H
    q, k, v = F.linear(x, W[p + "self_attn.in_proj_weight"], W[p + "self_attn.in_proj_bias"]).chunk(3, dim=-1)
    heads = lambda t: t.reshape(B, T, H, dh).transpose(1, 2)
    s = heads(q) @ heads(k).transpose(-1, -2) / (dh ** 0.5)
    if key_pad is not None:
        s = s.masked_fill(key_pad[:, None, None, :], float("-inf"))
    a = (torch.softmax(s, dim=-1) @ heads(v)).transpose(1, 2).reshape(B, T, D)
    x = F.layer_norm(x + F.linear(a, W[p + "self_attn.out_proj.weight"], W[p + "self_attn.out_proj.bias"]), (D,), W[p + "norm1.weight"], W[p + "norm1.bias"], 1e-5)
    f = F.linear(F.gelu(F.linear(x, W[p + "linear1.weight"], W[p + "linear1.bias"])), W[p + "linear2.weight"], W[p + "linear2.bias"])
    return F.layer_norm(x + f, (D,), W[p + "norm2.weight"], W[p + "norm2.bias"], 1e-5)


def _normalize(W, e):
    return e / e.norm(dim=-1, keepdim=True) * W["latent_scale"]


def encode_motion(W, cfg, motions, lens, dtype=torch.float32):
    """InterCLIP.encode_motion in its padded form: motions [B, T, C], lens [B] -> [B, 512]."""
    W = {k: v.to(dtype) for k, v in W.items()}
    x = motions.to(dtype)
    B, T, _ = x.shape
    if cfg["MODE"] == "interaction":
        x = x.reshape(B, T, 2, -1)[..., :-4].reshape(B, T, -1)
    else:
        x = x[..., :-4]
    D, H = int(cfg["LATENT_DIM"]), int(cfg["NUM_HEADS"])
    emb = F.linear(x, W["motion_encoder.embed_motion.weight"], W["motion_encoder.embed_motion.bias"])
    h = torch.cat([W["motion_encoder.query_token"][None].expand(B, 1, D), emb], dim=1)
    h = h + pe_table(D, T + 1).to(dtype)[None]
    valid = torch.arange(T)[None, :] < torch.as_tensor(lens)[:, None]
    key_pad = ~torch.cat([torch.ones(B, 1, dtype=torch.bool), valid], dim=1)
    for i in range(int(cfg["NUM_LAYERS"])):
        h = _encoder_layer(W, f"motion_encoder.transformer.layers.{i}.", h, H, key_pad)
    h = F.layer_norm(h[:, 0], (D,), W["motion_encoder.out_ln.weight"], W["motion_encoder.out_ln.bias"], 1e-5)
    return _normalize(W, F.linear(h, W["motion_encoder.out.weight"], W["motion_encoder.out.bias"]))


def encode_text(W, tokens, dtype=torch.float32):
    """InterCLIP.encode_text from token ids [B, L] -> [B, 512]."""
    W = {k: v.to(dtype) for k, v in W.items()}
    tokens = torch.as_tensor(tokens).long()
    x = W["token_embedding.weight"][tokens] + W["positional_embedding"][:tokens.shape[1]]
    for i in range(8):
        x = _encoder_layer(W, f"textTransEncoder.layers.{i}.", x, 8, None)
    x = F.layer_norm(x, (768,), W["text_ln.weight"], W["text_ln.bias"], 1e-5)
    x = x[torch.arange(x.shape[0]), tokens.argmax(dim=-1)]
    return _normalize(W, F.linear(x, W["out.weight"], W["out.bias"]))


# ---- the yardstick on embeddings -----------------------------------------------------------------------------------------------------------
def yardstick(got, ref32, ref64, what, report=True):
    """p50 / p99 / max of |got - ref64| <= YARD_FACTOR x the same quantile of |ref32 - ref64| + YARD_FLOOR.  Prints and records the figures, then asserts."""
    got = torch.as_tensor(np.asarray(got.detach().cpu()) if torch.is_tensor(got) else got).double()
    ref32, ref64 = torch.as_tensor(ref32).double(), torch.as_tensor(ref64).double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    qg, qr = _quant((got - ref64).abs(), QS), _quant((ref32 - ref64).abs(), QS)
    print(f"{what}: |got - f64| {dict(zip(QN, qg))}  |ref32 - f64| {dict(zip(QN, qr))}")
    if report:
        record(what, kind="evaluator_yardstick", got_vs_f64=dict(zip(QN, qg)), ref32_vs_f64=dict(zip(QN, qr)), factor=YARD_FACTOR, floor=YARD_FLOOR)
    fails = [f"{n}: {a:.3e} vs {b:.3e}" for n, a, b in zip(QN, qg, qr) if a > YARD_FACTOR * b + YARD_FLOOR]
    assert not fails, f"{what}: further from float64 than {YARD_FACTOR} x the reference's fp32 run: " + "; ".join(fails)
    return qg, qr

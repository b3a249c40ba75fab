#!/usr/bin/env python3
"""Generate tests/golden/evaluator.npz: the reference's InterCLIP evaluator and metric functions (builder container only; never on the GPU box).

Run:  python tests/golden/make_golden_evaluator.py

Imports make_golden for its stubs and helpers (as make_golden_mask.py does) and adds three stubs of its own, none of which touches arithmetic:
``clip.load`` returns an object with token_embedding = nn.Embedding(V, 768), positional_embedding [77, 768] and dtype float32; ``clip.tokenize``
returns the recorded token ids; an empty ``pykeops.torch`` lets utils.metrics import.

No weights are stored (the text tower alone is 22 M floats): the fixture keeps the (name, shape) list of state_dict(), the seed and the std, and the
tests re-draw the weights by the rule of make_golden.reinit.  Inputs are rnd(seed, *shape), recorded as seed and shape.  Reference outputs are stored
from the fp32 model and from model.double() on the same weights.
"""
import json
import sys
import types
import numpy as np

from make_golden import torch, reinit, rnd, save

import clip  # noqa: E402  (make_golden's stub package)

SEED, STD, VOCAB = 700, 0.1, 64
TOKENS = {}


class _ClipStub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.token_embedding = torch.nn.Embedding(VOCAB, 768)
        self.positional_embedding = torch.nn.Parameter(torch.zeros(77, 768))
        self.dtype = torch.float32


clip.load = lambda *a, **k: (_ClipStub(), None)
clip.tokenize = lambda texts, truncate=True: TOKENS["now"]
for name in ("pykeops", "pykeops.torch"):
    sys.modules[name] = types.ModuleType(name)

from evaluation.models import InterCLIP  # noqa: E402
from utils import metrics as M  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


def cfg_of(mode, D, H, F, L):
    return Cfg(INPUT_DIM=258, LATENT_DIM=D, FF_SIZE=F, NUM_LAYERS=L, NUM_HEADS=H, DROPOUT=0.1, ACTIVATION="gelu", MODE=mode)


CASES = {          # name: (cfg, lengths in the order given, buffer shape, motions seed)
    "int128": (cfg_of("interaction", 128, 2, 256, 2), [17, 1, 33, 16, 32], (5, 40, 524), 711),
    "int256": (cfg_of("interaction", 256, 2, 512, 2), [17, 1, 33, 16, 32], (5, 40, 524), 712),
    "ind128": (cfg_of("individual", 128, 2, 256, 2), [17, 1, 33, 16, 32], (5, 40, 262), 713),
    "full": (cfg_of("interaction", 1024, 8, 2048, 8), [150, 300, 61], (3, 300, 524), 714),
}


def tokens_of(seed, n):
    """n rows of 77 ids below VOCAB - 1 with the EOT = VOCAB - 1 (the largest id) at a different position in every row."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, VOCAB - 1, (n, 77), generator=g)
    for i, pos in enumerate(torch.randperm(70, generator=g)[:n].tolist()):
        t[i, pos + 3] = VOCAB - 1
        t[i, pos + 4:] = 0
    return t


def build(cfg):
    return reinit(InterCLIP(cfg), SEED, STD)


def in64(model):
    m = model.double()
    m.dtype = torch.float64
    return m


def motion_emb(model, motions, lens):
    return model.encode_motion({"motions": motions, "motion_lens": torch.tensor(lens)})["motion_emb"]


def text_emb(model, tokens):
    TOKENS["now"] = tokens
    return model.encode_text({"text": [""] * tokens.shape[0]})["text_emb"]


def main():
    out = {"seed": SEED, "std": STD, "vocab": VOCAB, "cases": np.array(list(CASES))}
    models = {}
    for name, (cfg, lens, shape, mseed) in CASES.items():
        model = build(cfg)
        out[f"{name}:cfg"] = json.dumps({k: cfg[k] for k in ("MODE", "LATENT_DIM", "NUM_HEADS", "FF_SIZE", "NUM_LAYERS")})
        out[f"{name}:state_dict"] = json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()])
        out[f"{name}:lens"] = np.array(lens)
        out[f"{name}:motions"] = np.array([mseed, *shape])
        motions = rnd(mseed, *shape)
        r32 = motion_emb(model, motions, lens)
        if name == "int128":
            models["int128"] = build(cfg)          # kept in fp32 for the text and the wrapper case (model.double() converts in place)
        r64 = motion_emb(in64(model), motions.double(), lens)
        out[f"{name}:ref32"], out[f"{name}:ref64"] = r32, r64
        alone = motion_emb(build(cfg), motions[:1], lens[:1]) if name == "int128" else None
        print(f"{name}: max |ref32 - ref64| = {float((r32.double() - r64).abs().max()):.2e}, |emb| = {float(r64.norm(dim=-1).mean()):.3f}" +
              (f", alone vs in batch {float((alone[0] - r32[0]).abs().max()):.1e}" if alone is not None else ""))
        del model
    # --- text (the int128 weights: FF_SIZE = 256 sets the width of the 8 text layers)
    cfg = CASES["int128"][0]
    tok = tokens_of(720, 3)
    out["text:tokens"] = tok.numpy()
    t32 = text_emb(models["int128"], tok)
    m64 = in64(build(cfg))
    t64 = text_emb(m64, tok)
    out["text:ref32"], out["text:ref64"] = t32, t64
    print(f"text: max |ref32 - ref64| = {float((t32.double() - t64).abs().max()):.2e}")
    # --- wrapper case: the int128 motions with 5 prompts; both embeddings in the order np.argsort(lens)[::-1] (utils.py:164, 190)
    _, lens, shape, mseed = CASES["int128"]
    wtok = tokens_of(721, 5)
    out["wrap:tokens"] = wtok.numpy()
    order = np.argsort(torch.tensor(lens).data.tolist())[::-1].copy()
    out["wrap:order"] = order
    motions = rnd(mseed, *shape)
    res = {}
    for tag, model, mo in (("32", models["int128"], motions), ("64", m64, motions.double())):
        me = motion_emb(model, mo[order], [lens[i] for i in order])
        te = text_emb(model, wtok)[order]
        res[tag] = (te, me)
        out[f"wrap:text_ref{tag}"], out[f"wrap:motion_ref{tag}"] = te, me
    err = max(float((res["32"][k].double() - res["64"][k]).abs().max()) for k in (0, 1))
    dist64 = M.euclidean_distance_matrix(res["64"][0].numpy(), res["64"][1].numpy())
    rank_gap = float(np.diff(np.sort(dist64, axis=1), axis=1).min())
    assert rank_gap > 100 * err, f"rank_gap {rank_gap:.2e} <= 100 x {err:.2e}: change the seed, not the factor"
    out["wrap:rank_gap"], out["wrap:max_err"] = rank_gap, err
    d32 = M.euclidean_distance_matrix(res["32"][0].numpy(), res["32"][1].numpy())
    out["wrap:top_k"] = M.calculate_top_k(np.argsort(d32, axis=1), top_k=3).sum(axis=0)
    out["wrap:mm_dist32"], out["wrap:mm_dist64"] = d32.trace() / 5, dist64.trace() / 5
    print(f"wrapper: rank_gap {rank_gap:.2e}, max |ref32 - ref64| {err:.2e}, top-k counts {out['wrap:top_k']}")
    # --- metrics: seeded embeddings, every reference function after np.random.seed(k)
    out["met:in"] = np.array([[731, 64, 16], [732, 64, 16], [733, 48, 16]])          # generated, ground truth, mm (reshaped to [6, 8, 16])
    a, b, mm = rnd(731, 64, 16).double().numpy(), rnd(732, 64, 16).double().numpy(), rnd(733, 48, 16).double().numpy().reshape(6, 8, 16)
    out["met:dist"] = M.euclidean_distance_matrix(a[:32], b[:32])
    out["met:top_k"] = M.calculate_top_k(np.argsort(out["met:dist"], axis=1), 3)
    out["met:r_precision"] = M.calculate_R_precision(a[:32], b[:32], 3, sum_all=True)
    out["met:matching"] = M.calculate_matching_score(a, b)
    mu_a, cov_a = M.calculate_activation_statistics(a)
    mu_b, cov_b = M.calculate_activation_statistics(b)
    out["met:mu"], out["met:cov"] = mu_a, cov_a
    fid = M.calculate_frechet_distance(mu_b, cov_b, mu_a, cov_a)
    perm = np.random.RandomState(5).permutation(64)
    fid_p = M.calculate_frechet_distance(*M.calculate_activation_statistics(b[perm]), *M.calculate_activation_statistics(a[perm]))
    out["met:fid"] = fid
    out["met:fid_rtol"] = max(100 * abs(fid - fid_p) / abs(fid), 1e-10)
    np.random.seed(41)
    out["met:diversity"] = M.calculate_diversity(a, 20)
    np.random.seed(42)
    out["met:multimodality"] = M.calculate_multimodality(mm, 5)
    out["met:seeds"] = np.array([41, 42])
    print(f"metrics: fid {fid:.6f} (rows permuted: {fid_p:.6f}, fid_rtol {float(out['met:fid_rtol']):.1e})")
    save("evaluator", **out)


if __name__ == "__main__":
    main()

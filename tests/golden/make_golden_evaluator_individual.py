#!/usr/bin/env python3
"""Generate tests/golden/evaluator_individual.npz: the reference's own EvaluatorModelWrapperIndividual (src/evaluation/utils.py:237-383) on seeded
batches (builder container only; never on the GPU box).

Run:  python tests/golden/make_golden_evaluator_individual.py

Imports make_golden_evaluator for its stubs and helpers (the ``clip`` stub that returns the recorded token ids, the empty ``pykeops.torch``, cfg_of,
build, tokens_of).  ``evaluation.utils`` imports the reference's dataset and model packages at module level; any of their third-party
imports that this machine lacks gets an empty stand-in module -- none of them touches the arithmetic recorded here.  The wrapper object is made
without a checkpoint file: ``object.__new__`` and the four attributes its methods read, the model built and re-drawn as in make_golden_evaluator.

The fixture holds seeds, names, shapes, token ids and results only (no weights).  A person is drawn by ``person(seed, B, T)`` below -- unit-scale
positions, small velocities, noisy rotations of random unit quaternions, feet in [0, 1) -- and the frames beyond each length are zeroed, as the
datasets pad.  The reference's centring casts to fp32 internally, so there is no float64 run of it: the tests form the float64 side themselves.
"""
import importlib
import json
import sys
import types
import numpy as np

from make_golden_evaluator import torch, clip, cfg_of, build, tokens_of, SEED, STD, VOCAB
from make_golden import save, rc


class _AnyClass(type):
    """Metaclass of the stand-in classes: their attributes are stand-in classes too (``pl.LightningDataModule``, ``a.b.C``)."""
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _AnyClass(name, (), {})


class _Anything(types.ModuleType):
    """A stand-in for a third-party module the dataset code imports at module level: every attribute is its stand-in submodule or a class nobody
    instantiates here."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return sys.modules.get(f"{self.__name__}.{name}") or _AnyClass(name, (), {})


def import_evaluation_utils():
    for _ in range(64):
        try:
            return importlib.import_module("evaluation.utils")
        except ModuleNotFoundError as e:
            print("stand-in for", e.name)
            sys.modules[e.name] = _Anything(e.name)
    raise RuntimeError("evaluation.utils does not import")


EU = import_evaluation_utils()

B, T, LENS = 4, 24, (24, 17, 1, 9)          # per-call batch 4, never 3 (torch.cross without dim)
CASES = {          # name: (cfg, seed of person 1, seed of person 2)
    "ind128": (cfg_of("individual", 128, 2, 256, 2), 7, 14),
    "ind256": (cfg_of("individual", 256, 2, 512, 2), 15, 20),
}


def person(seed, b, t):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randn(b, t, 66, generator=g)
    vel = 0.1 * torch.randn(b, t, 66, generator=g)
    q = torch.nn.functional.normalize(torch.randn(b, t, 21, 4, generator=g), dim=-1)
    rot = rc.matrix_to_rotation_6d(rc.quaternion_to_matrix(q)).reshape(b, t, 126) + 0.05 * torch.randn(b, t, 126, generator=g)
    feet = torch.rand(b, t, 4, generator=g)
    return torch.cat([pos, vel, rot, feet], dim=-1)


def zero_tails(m, lens):
    m = m.clone()
    for i, n in enumerate(lens):
        m[i, n:] = 0
    return m


def wrapper_of(cfg):
    w = object.__new__(EU.EvaluatorModelWrapperIndividual)
    w.model, w.cfg, w.device, w.extended = build(cfg), cfg, torch.device("cpu"), True
    return w


def main():
    out = {"seed": SEED, "std": STD, "vocab": VOCAB, "cases": np.array(list(CASES)), "lens": np.array(LENS), "shape": np.array([B, T])}
    for k, (name, (cfg, s1, s2)) in enumerate(CASES.items()):
        w = wrapper_of(cfg)
        out[f"{name}:cfg"] = json.dumps({k_: cfg[k_] for k_ in ("MODE", "LATENT_DIM", "NUM_HEADS", "FF_SIZE", "NUM_LAYERS")})
        out[f"{name}:state_dict"] = json.dumps([[k_, list(v.shape)] for k_, v in w.model.state_dict().items()])
        out[f"{name}:person_seeds"] = np.array([s1, s2])
        m1, m2 = zero_tails(person(s1, B, T), LENS), zero_tails(person(s2, B, T), LENS)
        tok1, tok2 = tokens_of(740 + 2 * k, B), tokens_of(741 + 2 * k, B)
        out[f"{name}:tokens1"], out[f"{name}:tokens2"] = tok1.numpy(), tok2.numpy()
        # the prompts are stand-ins that name their own token row: the clip stub hands the rows back in the order the wrapper lists the prompts
        names1, names2 = [f"1:{i}" for i in range(B)], [f"2:{i}" for i in range(B)]
        rows = {**{n: tok1[i] for i, n in enumerate(names1)}, **{n: tok2[i] for i, n in enumerate(names2)}}
        seen = []
        clip.tokenize = lambda texts, truncate=True: (seen.append(list(texts)), torch.stack([rows[t] for t in texts]))[1]
        batch = (["n%d" % i for i in range(B)], [""] * B, m1, m2, torch.tensor(LENS), names1, names2)
        te, me = w.get_co_embeddings(batch)
        me2 = w.get_motion_embeddings(batch)
        assert torch.equal(me, me2) and te.shape == (2 * B, 512) and me.shape == (2 * B, 512)
        out[f"{name}:text_order"] = np.array(seen[0])
        out[f"{name}:text_ref32"], out[f"{name}:motion_ref32"] = te, me
        print(f"{name}: text order {seen[0]}, |emb| = {float(me.norm(dim=-1).mean()):.3f}")
    save("evaluator_individual", **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Items/s of the stand-alone InterGen, MDM and in2IN samplers: the per-item forward_test loop against ragged batches (DESIGN sections 9d, 9e).

The reference samples these models one item at a time (src/scripts/infer/mdm.py; InterDiffusion.forward, src/models/intergen.py:184-213).  This script
measures that -- N items (default 16), T uniform in [60, 300], B = 1 per call -- and then the same items through ``sample_many(batching="ragged")`` on the
SAME model / handle, at the sizes of configs/models/InterGen.yaml / MDM.yaml / in2IN.yaml with synthetic weights (in2in-dual: both denoisers at in2IN.yaml's
sizes, W_FUNC "exp" / W_VALUE 0.004 as the dual configuration of the reference's inference script passes them).  The motions are asserted bitwise equal; items/s of
both and their ratio are printed as one JSON line per model.

--invert measures DDIM inversion the same way: every item carries a motion instead of x_T, the per-item ``invert`` loop is compared with
``invert_many(batching="ragged")``, the latents are asserted bitwise equal.

    python tools/standalone_eval.py [--model intergen|mdm|both|in2in-interaction|in2in-dual] [--items 16] [--sampler ddim50] [--precision fp32|fp32_split|bf16|bf16_fp8]
                                    [--invert]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(name, sampler, precision):
    import torch
    from mixermdm_amd.configs import CfgNode, get_config
    from mixermdm_amd import models
    from mixermdm_amd.synthetic import denoiser_shapes, mdm_denoiser_shapes
    g = torch.Generator().manual_seed(0)
    draw = lambda shapes: {k: (1.0 if k.endswith(("norm1.weight", "norm2.weight")) else 0.0) + torch.randn(shp, generator=g) * 0.02 for k, shp in shapes.items()}
    if name == "intergen":
        cfg = CfgNode(dict(get_config(os.path.join(ROOT, "configs", "models", "InterGen.yaml")), STRATEGY=sampler))
        m = models.InterGen(cfg)
        m.load_state_dict(draw(denoiser_shapes("decoder.net.", cfg.LATENT_DIM, cfg.FF_SIZE, cfg.NUM_LAYERS)))
        m.decoder.precision = precision
        return m, 768, 524
    if name.startswith("in2in-"):
        mode = name[len("in2in-"):]
        cfg = CfgNode(dict(get_config(os.path.join(ROOT, "configs", "models", "in2IN.yaml")), STRATEGY=sampler, W_FUNC="exp", W_VALUE=0.004))
        m = models.in2IN(cfg, mode)
        sd = {}
        for net in (("net_interaction.",) if mode == "interaction" else ("net_individual.", "net_interaction.")):
            sd.update(draw(denoiser_shapes("decoder." + net, cfg.LATENT_DIM, cfg.FF_SIZE, cfg.NUM_LAYERS)))
        m.load_state_dict(sd)
        m.decoder.precision = precision
        return m, (3 if mode == "interaction" else 5) * 768, 524
    cfg = get_config(os.path.join(ROOT, "configs", "models", "MDM.yaml"))
    m = models.MDM(cfg, num_frames=300, sampling_strategy=sampler)
    sd = draw(mdm_denoiser_shapes("model.", cfg.LATENT_DIM, cfg.FF_SIZE, cfg.NUM_LAYERS))
    sd.update({"embed_text.weight": torch.zeros(cfg.LATENT_DIM, 512), "embed_text.bias": torch.zeros(cfg.LATENT_DIM)})
    m.load_state_dict(sd)
    m.precision = precision
    return m, cfg.LATENT_DIM, 262


def measure(name, args):
    import numpy as np
    import torch
    model, cw, width = build(name, args.sampler, args.precision)
    model = model.to("cuda:0").eval()
    N = args.items
    lens = [int(v) for v in np.random.RandomState(0).randint(60, 301, size=N)]
    batches = []
    for i, T in enumerate(lens):
        g = torch.Generator().manual_seed(100 + i)
        cond = torch.randn(1, cw, generator=g).cuda()
        b = {"x_T": torch.randn(1, T, width, generator=g).cuda(), "motion_lens": torch.tensor([T])}
        if args.invert:                         # a motion in the models' normalised space instead of the start noise
            b = {"motions": 0.5 * b["x_T"]}
        if name.startswith("in2in-"):           # the text slices under the names in2INDiffusion.forward concatenates
            keys = ("cond_interaction", "cond_interaction_individual1", "cond_interaction_individual2", "cond_individual_individual1", "cond_individual_individual2")
            b.update({k: cond[:, 768 * j:768 * (j + 1)] for j, k in enumerate(keys[:cw // 768])})
        else:
            b["cond"] = cond
        batches.append(b)

    def run(fn, warm):
        with torch.no_grad():
            fn(batches[:warm])                       # untimed: allocator warm-up, the first graph captures
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(batches)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return [r["latent" if args.invert else "output"] for r in res], dt

    if args.invert:
        ref, t_seq = run(lambda b: [model.invert(dict(x)) for x in b], 3)
        got, t_rag = run(lambda b: model.invert_many([dict(x) for x in b], batching="ragged", max_rows=args.max_rows), N)
    else:
        ref, t_seq = run(lambda b: [model.forward_test(dict(x)) for x in b], 3)
        got, t_rag = run(lambda b: model.sample_many([dict(x) for x in b], batching="ragged", max_rows=args.max_rows), N)
    same = all(torch.equal(a, b) for a, b in zip(ref, got))
    assert same, "ragged batches and the per-item loop differ"
    assert all(torch.isfinite(o).all().item() for o in got)
    what = "one invert per item" if args.invert else "one forward_test per item"
    print(json.dumps({"metric": "items/s, stand-alone %s (%s, B = 1, %s, T uniform in [60, 300])" % (name, what, args.sampler), "items": N,
                      "frames": sum(lens), "precision": args.precision, "sequential_invert" if args.invert else "sequential_forward_test": {"wall_s": round(t_seq, 3), "items_per_s": round(N / t_seq, 4)},
                      "ragged": {"wall_s": round(t_rag, 3), "items_per_s": round(N / t_rag, 4)}, "ratio": round(t_seq / t_rag, 3), "bit_identical": bool(same)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both", choices=("intergen", "mdm", "both", "in2in-interaction", "in2in-dual"))
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--sampler", default="ddim50")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "fp32_split", "bf16", "bf16_fp8"), help="MDM: fp32 or fp32_split")
    ap.add_argument("--max-rows", type=int, default=4800, help="frames per ragged batch (16 x 300)")
    ap.add_argument("--invert", action="store_true", help="DDIM inversion: the per-item invert loop against invert_many(batching=\"ragged\")")
    args = ap.parse_args()
    for name in (("intergen", "mdm") if args.model == "both" else (args.model,)):
        measure(name, args)


if __name__ == "__main__":
    main()

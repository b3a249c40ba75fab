#!/usr/bin/env python3
"""Evaluation items/s with MDMDenoiser as MODEL1: the per-item forward_test loop against ragged batches (the MDM row).

The reference's evaluation caller samples one item at a time with that item's own length (src/evaluation/datasets.py:100-116).  bench.py --eval-items
measures that for the in2IN MODEL1 of configs/models/MixerMDM.yaml; this script is the same measurement with MODEL1.NAME == "MDM": N items (default 16),
T uniform in [60, 300], ddim50, fp32 or fp32_split (--precision), on ONE model / handle: first the per-item `forward_test` loop, then `sample_many(batching="ragged")`, results
asserted bitwise equal, items/s of both and their ratio printed as one JSON line.

MDM's sizes: no MDM YAML ships with the reference.  MDMDenoiser.text_dim is hard-coded to 256 and the cond slice is added to the latent-sized timestep
embedding (src/models/mdm.py:238, 279), which fixes LATENT_DIM = 256; the rest are MDM's published defaults (FF_SIZE 1024, 8 layers, 4 heads: head size
64).  The other stacks are the reference's (synthetic.FULL_DIMS).

    python tools/ragged_mdm_eval.py [--items 16] [--sampler ddim50] [--precision fp32|fp32_split] [--profile-steps 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MDM = dict(NAME="MDM", LATENT_DIM=256, FF_SIZE=1024, NUM_LAYERS=8, NUM_HEADS=4, INPUT_DIM=262, DROPOUT=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--sampler", default="ddim50")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "fp32_split"), help="the precision modes that cover MDM as MODEL1")
    ap.add_argument("--max-rows", type=int, default=4800, help="frames per ragged batch (16 x 300)")
    ap.add_argument("--profile-steps", type=int, default=2, help="eager steps of the first ragged batch timed per kernel class (0 = none)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import yaml
    from mixermdm_amd.configs import CfgNode
    from mixermdm_amd.models import MixerMDM
    N = args.items
    lens = [int(v) for v in np.random.RandomState(0).randint(60, 301, size=N)]
    base = yaml.safe_load(open(os.path.join(ROOT, "configs", "models", "MixerMDM.yaml")))
    with tempfile.TemporaryDirectory() as tmp:
        yaml.safe_dump(MDM, open(os.path.join(tmp, "mdm.yaml"), "w"))
        base["MODEL1"] = os.path.join(tmp, "mdm.yaml")
        base["MODEL2"] = os.path.join(ROOT, base["MODEL2"])
        model = MixerMDM(CfgNode(base), num_frames=300, sampling_strategy=args.sampler, config_root=ROOT)
    model.precision = args.precision
    model.init_synthetic(seed=0)
    model = model.to("cuda:0").eval()
    cw = 6 * 768 + 2 * MDM["LATENT_DIM"]
    batches = []
    for i, T in enumerate(lens):
        g = torch.Generator().manual_seed(100 + i)
        batches.append({"cond": torch.randn(1, cw, generator=g).cuda(), "x_T": torch.randn(1, T, 524, generator=g).cuda(), "motion_lens": torch.tensor([T])})

    def run(fn, warm):
        with torch.no_grad():
            fn(batches[:warm])                       # untimed: allocator warm-up, the first graph captures
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(batches)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        return [r["output"] for r in res], dt

    ref, t_seq = run(lambda b: [model.forward_test(dict(x)) for x in b], 3)
    got, t_rag = run(lambda b: model.sample_many([dict(x) for x in b], mode="eval_intermediate", batching="ragged", keep_history=False, max_rows=args.max_rows), 6)
    same = all(torch.equal(a, b) for a, b in zip(ref, got))
    assert same, "ragged batches and the per-item loop differ"
    assert all(torch.isfinite(o).all().item() for o in got)
    line = {"metric": "evaluation items/s, MDM as MODEL1 (one forward_test per item, B = 1, %s, T uniform in [60, 300])" % args.sampler, "items": N, "frames": sum(lens),
            "precision": args.precision,
            "model1": MDM, "sequential_forward_test": {"wall_s": round(t_seq, 3), "items_per_s": round(N / t_seq, 4)},
            "ragged": {"wall_s": round(t_rag, 3), "items_per_s": round(N / t_rag, 4)}, "ratio": round(t_seq / t_rag, 3), "bit_identical": bool(same)}
    if args.profile_steps > 0:
        # where a ragged step's time goes: live event pairs around every GEMM / attention launch of a few eager steps of the first ragged batch
        rows, grp = 0, []
        for i, T in enumerate(lens):
            if grp and rows + T > args.max_rows:
                break
            grp.append(i)
            rows += T
        smp = model._sampler_for(len(grp), 300)
        smp.begin_ragged(torch.cat([batches[i]["cond"] for i in grp], 0), [batches[i]["x_T"][0] for i in grp], [lens[i] for i in grp])
        smp.run(1, use_graph=False)
        smp.synchronize()
        t0 = time.perf_counter()
        smp.run(args.profile_steps, use_graph=False)
        smp.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / args.profile_steps
        smp.profile(True)
        smp.run(args.profile_steps, use_graph=False)
        g_ms, g_n, g_fl, _ = smp.profile_read(0)
        a_ms, a_n, a_fl, _ = smp.profile_read(1)
        smp.profile(False)
        line["first_ragged_batch"] = {"items": len(grp), "frames": rows, "frame_rows": smp.rows, "token_rows_real": rows + len(grp),
                                      "eager_step_ms": round(step_ms, 3), "gemm_ms_per_step": round(g_ms / args.profile_steps, 3),
                                      "gemm_tflops": round(g_fl / (g_ms * 1e-3) / 1e12, 2), "gemm_launches_per_step": g_n // args.profile_steps,
                                      "attention_ms_per_step": round(a_ms / args.profile_steps, 3), "attention_launches_per_step": a_n // args.profile_steps}
    print(json.dumps(line))


if __name__ == "__main__":
    main()

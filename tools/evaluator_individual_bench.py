#!/usr/bin/env python3
"""Throughput of the InterCLIP INDIVIDUAL evaluator (InterCLIP.encode_motion_individual, mixermdm_amd/evaluation.py) at full size on an MI355X.

    python tools/evaluator_individual_bench.py [--items 64] [--batch 32] [--repeats 20] [--warmup 3] [--precision fp32] [--out profiles/evaluator_individual_bench.json]

The workload of tools/evaluator_bench.py -- `--items` interactions with T uniform in [60, 300] (seeded), batches of `--batch` -- through
configs/eval_individual.yaml (D = 1024, 8 heads, F = 2048, 8 layers, one person per sequence) with synthetic weights: every item gives two embeddings.
After the warm-up every repeat encodes all items and ends in a device synchronise; the line reports

  embeddings/s and ms per batch             median over the repeats (and their spread)
  centring                                  ops.center_pack alone (the floor launch + the fused centre-and-pack launch), timed between device events over
                                            the same batches: ms per batch and its share of the encode
  unfused                                   context, no gate: the same batches with ops.center_motion + the batch-level interleave + ops.motion_pack(npers=1)
                                            in front of the same encoder -- ms per batch of that front end alone and of the whole encode

--precision fp32_split measures InterCLIP(cfg, precision="fp32_split"): the fused front end is ops.center_pack_split, the unfused one ends in
ops.motion_pack_split, both in front of the split encoder (default output then: profiles/evaluator_individual_bench_split.json).

One JSON line on stdout; also written to --out.  There is no CPU fall-back: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=("fp32", "fp32_split"), default="fp32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    split = args.precision == "fp32_split"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "evaluator_individual_bench_split.json" if split else "evaluator_individual_bench.json")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evaluator_individual_bench needs an MI355X: not measured")
    from mixermdm_amd import ops
    from mixermdm_amd.configs import get_config
    from mixermdm_amd.evaluation import InterCLIP, interclip_shapes
    from mixermdm_amd.build import sources_sha
    cfg = get_config(os.path.join(ROOT, "configs", "eval_individual.yaml"))
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(args.seed)
    sd = {k: torch.randn(s, generator=gen) * 0.02 for k, s in interclip_shapes(cfg, vocab=64, context=77).items()}
    sd["latent_scale"] = torch.ones(1)
    model = InterCLIP(cfg, device=dev, precision=args.precision).load_state_dict(sd)
    rng = np.random.RandomState(args.seed)
    lens = rng.randint(60, 301, size=args.items).tolist()
    batches = []
    for i in range(0, args.items, args.batch):
        ln = lens[i:i + args.batch]
        motions = torch.randn(len(ln), max(ln), 524, generator=gen).to(dev)
        seq_len = np.repeat(np.array([1 + n for n in ln], dtype=np.int32), 2)
        seq_off = np.concatenate([[0], np.cumsum(seq_len)[:-1]]).astype(np.int32)
        batches.append((motions, ln, torch.from_numpy(seq_off).to(dev), torch.from_numpy(seq_len).to(dev), int(seq_len.sum()), int(seq_len.max())))

    def front_fused(b):
        motions, _, so, sl, total, longest = b
        if split:
            return ops.center_pack_split(motions, so, sl, longest, total, k_pad=model.k_pad)
        return ops.center_pack(motions, so, sl, longest, total, k_pad=model.k_pad)

    def front_unfused(b):
        motions, _, so, sl, total, longest = b
        B, T, _ = motions.shape
        centred = ops.center_motion(motions).reshape(B, T, 2, 262).transpose(1, 2).reshape(2 * B, T, 262)
        if split:
            return ops.motion_pack_split(centred, so, sl, longest, total, npers=1, k_pad=model.k_pad, build=1)
        return ops.motion_pack(centred, so, sl, longest, total, npers=1, k_pad=model.k_pad)

    def run(fused):
        out = None
        for b in batches:
            if fused:
                out = model.encode_motion_individual({"motions": b[0], "motion_lens": b[1]})["motion_emb"]
            else:
                out = (model._encode_packed_split if split else model._encode_packed)(front_unfused(b), b[2], b[3], b[4], b[5])
        torch.cuda.synchronize()
        return out

    def measure(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    def measure_front(front):
        """Device time of the front end over all batches of a pass (events around the launches), seconds per pass."""
        ts = []
        for r in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for b in batches:
                front(b)
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                ts.append(e0.elapsed_time(e1) / 1e3)
        return ts

    t_fused, t_unfused = measure(lambda: run(True)), measure(lambda: run(False))
    c_fused, c_unfused = measure_front(front_fused), measure_front(front_unfused)
    assert torch.isfinite(run(True)).all()
    same = bool(torch.equal(run(True), run(False)))
    med = lambda v: float(np.median(v))
    nb = len(batches)
    line = {"metric": "evaluator_individual_embeddings_per_s", "value": round(2 * args.items / med(t_fused), 1), "unit": "embeddings/s", "precision": args.precision,
            "items": args.items, "embeddings": 2 * args.items, "batch": args.batch, "frames": [min(lens), max(lens)], "repeats": len(t_fused),
            "warmup": args.warmup, "ms_per_batch": round(1e3 * med(t_fused) / nb, 3),
            "ms_per_pass_min_max": [round(1e3 * min(t_fused), 3), round(1e3 * max(t_fused), 3)],
            "packed_rows": sum(2 * (1 + n) for n in lens), "fused_bitwise_equals_unfused": same,
            "centring": {"ms_per_batch": round(1e3 * med(c_fused) / nb, 4), "share_of_encode": round(med(c_fused) / med(t_fused), 5),
                         "what": "ops.center_pack alone (floor + fused centre-and-pack launches) between device events, over the encode's wall time"},
            "unfused": {"front_ms_per_batch": round(1e3 * med(c_unfused) / nb, 4), "ms_per_batch": round(1e3 * med(t_unfused) / nb, 3),
                        "embeddings_per_s": round(2 * args.items / med(t_unfused), 1),
                        "what": "center_motion + batch-level interleave + motion_pack(npers=1) in front of the same encoder: context, not a gate"},
            "device": torch.cuda.get_device_name(0), "kernel_sources_sha": sources_sha(args.precision)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

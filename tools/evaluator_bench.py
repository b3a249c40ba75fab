#!/usr/bin/env python3
"""Throughput of the InterCLIP motion encoder (mixermdm_amd/evaluation.py) at full size on an MI355X.

    python tools/evaluator_bench.py [--items 64] [--batch 32] [--repeats 5] [--warmup 2] [--precision fp32] [--out profiles/evaluator_bench.json]
    python tools/evaluator_bench.py --precision both --warmup 3 --repeats 20          # -> profiles/evaluator_bench_split.json

configs/eval.yaml (D = 1024, 8 heads, F = 2048, 8 layers), synthetic weights, `--items` motions with T uniform in [60, 300] (seeded), encoded in
batches of `--batch`.  After the warm-up every repeat encodes all items and ends in a device synchronise; the line reports

  embeddings/s and ms per batch             median over the repeats (and their spread)
  packed rows vs padded rows                sum(1 + T) against B x (1 + max T) per batch: what the ragged form does not compute
  frac_of_f32_mfma_peak                     the algorithmic FLOPs of the GEMMs and the attention of the PACKED rows (counted from shapes, below) over the
                                            whole encode time, against the fp32 MFMA peak bench.py uses -- an end-to-end rate over peak, not a kernel's share
  padded                                    the same items with every length set to the batch's maximum (what a padded evaluator computes): context, no gate

--precision fp32 / fp32_split measures that mode of InterCLIP; `both` builds the two models over the same weights and ALTERNATES their timed passes in
one process (fp32, split, fp32, split, ...: whatever the box's clocks do, both modes see it), reports embeddings/s of each, their ratio, and the
full-size distance between the two modes' embeddings (relative RMS and max |split - fp32| / max |fp32| over all items).

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

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X fp32 matrix peak: the figure of bench.py's roofline


def encoder_flops(seq_lens, D, F, L, K, emb=512):
    """Algorithmic FLOPs of encode_motion on token sequences of `seq_lens` rows: 2 M N K per GEMM on the packed rows, 4 dh n^2 per (sequence, head)."""
    rows = sum(seq_lens)
    per_layer = 2.0 * rows * D * (3 * D + D + 2 * F) + 4.0 * D * sum(n * n for n in seq_lens)
    return 2.0 * rows * D * K + L * per_layer + 2.0 * len(seq_lens) * D * emb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", choices=("fp32", "fp32_split", "both"), default="fp32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "evaluator_bench_split.json" if args.precision == "both" else "evaluator_bench.json")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("evaluator_bench needs an MI355X: not measured")
    from mixermdm_amd.configs import get_config
    from mixermdm_amd.evaluation import InterCLIP, interclip_shapes
    from mixermdm_amd.build import sources_sha
    cfg = get_config(os.path.join(ROOT, "configs", "eval.yaml"))
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(args.seed)
    sd = {k: torch.randn(s, generator=gen) * 0.02 for k, s in interclip_shapes(cfg, vocab=64, context=77).items()}
    sd["latent_scale"] = torch.ones(1)
    modes = ("fp32", "fp32_split") if args.precision == "both" else (args.precision,)
    models = {p: InterCLIP(cfg, device=dev, precision=p).load_state_dict(sd) for p in modes}
    model = models[modes[0]]
    rng = np.random.RandomState(args.seed)
    lens = rng.randint(60, 301, size=args.items).tolist()
    batches = []
    for i in range(0, args.items, args.batch):
        ln = lens[i:i + args.batch]
        batches.append((torch.randn(len(ln), max(ln), 524, generator=gen).to(dev), ln))

    def run(padded, m=None, keep=False):
        m = m or model
        outs = [m.encode_motion({"motions": motions, "motion_lens": [max(ln)] * len(ln) if padded else ln})["motion_emb"] for motions, ln in batches]
        torch.cuda.synchronize()
        return torch.cat(outs) if keep else outs[-1]

    def measure(padded):
        for _ in range(args.warmup):
            run(padded)
        ts = []
        for _ in range(max(5, args.repeats)):
            t0 = time.perf_counter()
            run(padded)
            ts.append(time.perf_counter() - t0)
        return ts

    med = lambda v: float(np.median(v))
    if args.precision == "both":
        for _ in range(args.warmup):
            for p in modes:
                run(False, models[p])
        ts = {p: [] for p in modes}
        for _ in range(max(5, args.repeats)):
            for p in modes:
                t0 = time.perf_counter()
                run(False, models[p])
                ts[p].append(time.perf_counter() - t0)
        e32, es = run(False, models["fp32"], keep=True).double(), run(False, models["fp32_split"], keep=True).double()
        assert torch.isfinite(es).all() and torch.isfinite(e32).all()
        d = es - e32
        packed = sum(1 + n for n in lens)
        line = {"metric": "evaluator_split_over_fp32", "value": round(med(ts["fp32"]) / med(ts["fp32_split"]), 3), "unit": "x (embeddings/s, fp32_split over fp32)",
                "items": args.items, "batch": args.batch, "frames": [min(lens), max(lens)], "repeats": len(ts["fp32"]), "warmup": args.warmup,
                "order": "alternating passes fp32, fp32_split in one process", "packed_rows": packed,
                "modes": {p: {"embeddings_per_s": round(args.items / med(ts[p]), 1), "ms_per_batch": round(1e3 * med(ts[p]) / len(batches), 3),
                              "ms_per_pass_min_max": [round(1e3 * min(ts[p]), 3), round(1e3 * max(ts[p]), 3)], "k_pad": models[p].k_pad} for p in modes},
                "split_vs_fp32_embeddings": {"rel_rms": float(d.pow(2).mean().sqrt() / e32.pow(2).mean().sqrt()), "max_over_max": float(d.abs().max() / e32.abs().max()),
                                             "max_abs": float(d.abs().max()), "shape": list(es.shape)},
                "device": torch.cuda.get_device_name(0), "kernel_sources_sha": {p: sources_sha(p) for p in modes}}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
        print(json.dumps(line))
        return
    t_rag, t_pad = measure(False), measure(True)
    assert torch.isfinite(run(False)).all()
    D, F, L = int(cfg.LATENT_DIM), int(cfg.FF_SIZE), int(cfg.NUM_LAYERS)
    packed = sum(1 + n for n in lens)
    padded_rows = sum(len(ln) * (1 + max(ln)) for _, ln in batches)
    flops = sum(encoder_flops([1 + n for n in ln], D, F, L, model.k_pad) for _, ln in batches)
    line = {"metric": "evaluator_embeddings_per_s", "value": round(args.items / med(t_rag), 1), "unit": "embeddings/s", "precision": args.precision,
            "items": args.items, "batch": args.batch, "frames": [min(lens), max(lens)], "repeats": len(t_rag), "warmup": args.warmup,
            "ms_per_batch": round(1e3 * med(t_rag) / len(batches), 3),
            "ms_per_pass_min_max": [round(1e3 * min(t_rag), 3), round(1e3 * max(t_rag), 3)],
            "packed_rows": packed, "padded_rows": padded_rows, "packed_over_padded": round(packed / padded_rows, 4),
            "algorithmic_tflop_per_pass": round(flops / 1e12, 4),
            "frac_of_f32_mfma_peak": round(flops / med(t_rag) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4), "peak_tflops": PEAK_F32_MFMA_TFLOPS,
            "frac_is": "algorithmic FLOPs of the packed rows over the whole encode time (host calls included): an end-to-end rate over peak",
            "padded": {"embeddings_per_s": round(args.items / med(t_pad), 1), "ms_per_batch": round(1e3 * med(t_pad) / len(batches), 3),
                       "what": "the same items with every length set to the batch's maximum: context, not a gate"},
            "device": torch.cuda.get_device_name(0), "kernel_sources_sha": sources_sha(args.precision)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

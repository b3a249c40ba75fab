"""What a key-padding mask costs the two masked attention kernels (GPU box): the fp32 form (attn_mfma_kernel<..., MASK>, mmdm_attention_masked_f32) and the
two-plane form of the fp32-split mode (attn_qkp_kernel<DH, 2, true, true, false, MASK>, mmdm_attention_split_masked) at the step's self-attention shape
64 x 8 x 300 x 128.  Three launches per form: unmasked (key_valid = NULL: the unmasked instantiation, the yardstick), masked with an all-valid mask, masked
with trailing masks of lengths uniform in [60, 300] (seeded; the kernels visit every chunk whatever the mask says, so the three do the same work).
HIP event pairs around REPS back-to-back launches, ROUNDS rounds with the three variants alternating inside a round, after a clock warm-up (tools/attn_bench.py);
per variant the median over the rounds and the min .. max spread, then masked / unmasked ratios of the medians.  The last line is one JSON object.
DESIGN 9a quotes the numbers."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C, json, statistics
import torch
from mixermdm_amd import ops, load_library
from mixermdm_amd._lib import check

NSEQ, H, T, DH = 64, 8, 300, 128
REPS, ROUNDS = int(os.environ.get("REPS", "20")), int(os.environ.get("ROUNDS", "11"))
lib = load_library()
d = torch.device("cuda:0")
D = H * DH
p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
g = torch.Generator().manual_seed(0)
qkv = torch.randn(NSEQ, T, 3 * D, generator=g).to(d)
planes = ops.split_f32(qkv.reshape(NSEQ * T, 3 * D))                   # [2, rows, 3D] fp16
out = torch.empty(NSEQ * T, D, device=d)
lens = torch.randint(60, T + 1, (NSEQ,), generator=g)
masks = {"unmasked": None, "all_valid": torch.ones(NSEQ, T, dtype=torch.uint8, device=d),
         "trailing": (torch.arange(T)[None, :] < lens[:, None]).to(torch.uint8).to(d).contiguous()}


def launch(form, valid):
    rows = NSEQ if valid is not None else 0
    if form == "fp32":
        check(lib.mmdm_attention_masked_f32(p(qkv), 3 * D, C.c_void_p(qkv.data_ptr() + 4 * D), 3 * D, C.c_void_p(qkv.data_ptr() + 8 * D), 3 * D, p(out), D, 0, 0,
                                            NSEQ, T, T, H, DH, 0, p(valid), rows, None))
    else:
        ps = NSEQ * T * 3 * D
        check(lib.mmdm_attention_split_masked(p(planes), 3 * D, ps, C.c_void_p(planes.data_ptr() + 2 * D), 3 * D, ps, C.c_void_p(planes.data_ptr() + 4 * D), 3 * D, ps,
                                              p(out), D, 0, 0, NSEQ, T, T, H, DH, 0, p(valid), rows, None))


_w = torch.randn(4096, 4096, device=d)
for _ in range(40): ops.linear(_w, _w)          # clock ramp
result = {"shape": [NSEQ, H, T, DH], "reps": REPS, "rounds": ROUNDS, "trailing_mean_len": float(lens.float().mean())}
with torch.cuda.stream(torch.cuda.default_stream(d)):
    for form in ("fp32", "split"):
        times = {k: [] for k in masks}
        for k, v in masks.items():
            for _ in range(REPS): launch(form, v)       # warm every variant
        torch.cuda.synchronize()
        for r in range(ROUNDS):
            for k, v in masks.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS): launch(form, v)
                e1.record(); torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / REPS * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            print(f"{form:5s} {k:9s}: median {med[k]:7.2f} us   min {min(v):7.2f}   max {max(v):7.2f}   ratio to unmasked {med[k] / med['unmasked']:.4f}", flush=True)
        result[form] = {k: {"median_us": round(med[k], 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in times.items()}
        result[form]["ratio_all_valid"] = round(med["all_valid"] / med["unmasked"], 4)
        result[form]["ratio_trailing"] = round(med["trailing"] / med["unmasked"], 4)
print(json.dumps(result))

"""Torch-tensor front ends of the stateless HIP kernels (include/mmdm.h section 1).

Every function takes contiguous fp32 CUDA(=HIP) tensors, launches on torch's current stream and returns a new
tensor.  No function here computes anything in Python: a non-CUDA tensor raises.
"""
import ctypes as C
import torch

from ._lib import load_library, check, EncoderLayerWeights, EncoderLayerSplitWeights

EPI = {"bias": 0, "gelu": 1, "resid": 2, "pe": 3, "silu": 4, "quickgelu": 5, "sigmoid": 6}
ATTN_NO_ZERO_KEY, ATTN_CAUSAL = 1, 2


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("mixermdm_amd ops run on the GPU only (no CPU fallback): got a CPU tensor")
        if t.dtype != torch.float32 and t.dtype != torch.int32:
            raise TypeError(f"fp32 tensors expected, got {t.dtype}")


def linear(x, weight, bias=None, epilogue="bias", extra=None, period=0, out=None):
    """y = x @ weight.T + bias with a fused epilogue; x [..., K] (last-dim stride 1, uniform row stride)."""
    _chk(x, weight, bias, extra)
    K = x.shape[-1]
    N = weight.shape[0]
    x2 = x.reshape(-1, K) if x.is_contiguous() else x
    assert x2.dim() == 2 and x2.stride(1) == 1 and weight.stride(1) == 1
    M = x2.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    ld_extra = extra.stride(0) if extra is not None else 0
    check(load_library().mmdm_linear_f32(_p(x2), x2.stride(0), _p(weight), weight.stride(0), _p(bias), _p(out), out.stride(0),
                                         M, N, K, EPI[epilogue], _p(extra), ld_extra, period, _stream()))
    return out.reshape(*x.shape[:-1], N) if x.is_contiguous() else out


_ADALN_OUT = {"f32": 0, "bf16": 1, "planes": 2, "fp8": 3}


def adaln(h, ss, ss_rows=None, build=0, out="f32", row_seq=None):
    """h [nseq, T, D]; ss [rows, 2D] (scale | shift); row(s) = s % ss_rows.
    build: 0 = the row kernels of fp32 handles and of the stateless entry points, 1 = the build without packed-fp32 instructions that fp32_split / bf16 /
    bf16_fp8 handles run (mmdm_rowop_adaln).  out: "f32", "bf16", "planes" (float16 [2, *h.shape], the split of the fp32 row) or "fp8" (returns
    (float8_e4m3fn like h, row_scale fp32 [rows])).  row_seq: int32 device tensor [rows] -- the ragged form on h [rows, D], row r takes ss row
    row_seq[r] % ss_rows."""
    _chk(h, ss, row_seq)
    mode = _ADALN_OUT[out]
    h = h.contiguous()
    D = h.shape[-1]
    if mode == 0 and build == 0 and row_seq is None:
        nseq, T, _ = h.shape
        o = torch.empty_like(h)
        check(load_library().mmdm_adaln_f32(_p(h), _p(ss), ss.stride(0), ss_rows or ss.shape[0], _p(o), nseq, T, D, _stream()))
        return o
    if row_seq is not None:
        assert h.dim() == 2 and row_seq.dtype == torch.int32 and row_seq.is_contiguous() and row_seq.numel() == h.shape[0]
        nseq, T, rows = 0, 0, h.shape[0]
    else:
        nseq, T, _ = h.shape
        rows = nseq * T
    shape = (2, *h.shape) if mode == 2 else h.shape
    o = torch.empty(shape, device=h.device, dtype=(torch.float32, torch.bfloat16, torch.float16, torch.uint8)[mode])
    scale = torch.empty(rows, device=h.device, dtype=torch.float32) if mode == 3 else None
    check(load_library().mmdm_rowop_adaln(_p(h), _p(ss), ss.stride(0), ss_rows or ss.shape[0], C.c_void_p(o.data_ptr()), mode, _p(scale), nseq, T, D,
                                          _p(row_seq), rows if row_seq is not None else 0, int(build), _stream()))
    return (o.view(torch.float8_e4m3fn), scale) if mode == 3 else o


def attention(q, k, v, num_heads, kv_seq_shift=0, zero_key=True, causal=False, key_padding_mask=None):
    """q [nseq, Tq, H*dh], k/v [nseq, Tk, H*dh] (may be column slices of a packed projection); add_zero_attn semantics by default,
    plain softmax with zero_key=False (optionally causal).
    key_padding_mask: bool [rows, Tk] in PyTorch's sense (True = ignore the key); key sequence s reads row s % rows (mmdm_attention_masked_f32)."""
    _chk(q, k, v)
    valid, mask_rows = None, 0
    if key_padding_mask is not None:
        if not key_padding_mask.is_cuda or key_padding_mask.dtype != torch.bool or key_padding_mask.dim() != 2 or key_padding_mask.shape[1] != k.shape[1]:
            raise TypeError("key_padding_mask: a CUDA bool tensor [rows, Tk] is expected (True = ignore)")
        valid = (~key_padding_mask).to(torch.uint8).contiguous()
        mask_rows = valid.shape[0]
    nseq, Tq, HD = q.shape
    Tk = k.shape[1]
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1), "rows must be uniformly strided"
    out = torch.empty(nseq, Tq, HD, device=q.device, dtype=torch.float32)
    flags = (0 if zero_key else ATTN_NO_ZERO_KEY) | (ATTN_CAUSAL if causal else 0)
    if valid is not None:
        check(load_library().mmdm_attention_masked_f32(_p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(out), HD, 0, flags,
                                                       nseq, Tq, Tk, num_heads, HD // num_heads, kv_seq_shift, C.c_void_p(valid.data_ptr()), mask_rows, _stream()))
        return out
    check(load_library().mmdm_attention_opts(_p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(out), HD, 0, flags,
                                             nseq, Tq, Tk, num_heads, HD // num_heads, kv_seq_shift, _stream()))
    return out


def attention_ragged(q, k, v, num_heads, seq_off, seq_len, max_len, kv_seq_shift=0, zero_key=True, causal=False, out=None):
    """Attention over a ragged batch (mmdm_attention_ragged_opts_f32): q / k / v [rows, H*dh] (may be column slices of a packed projection), sequence
    s = rows [seq_off[s], seq_off[s] + seq_len[s]) with seq_off / seq_len int32 device tensors; max_len >= every length.  Rows outside every
    sequence are left as they are in `out` (a new tensor: uninitialised)."""
    _chk(q, k, v, seq_off, seq_len)
    assert seq_off.dtype == torch.int32 and seq_len.dtype == torch.int32 and seq_off.numel() == seq_len.numel()
    rows, HD = q.shape
    for t in (q, k, v):
        assert t.dim() == 2 and t.stride(1) == 1
    if out is None:
        out = torch.empty(rows, HD, device=q.device, dtype=torch.float32)
    flags = (0 if zero_key else ATTN_NO_ZERO_KEY) | (ATTN_CAUSAL if causal else 0)
    check(load_library().mmdm_attention_ragged_opts_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0), flags,
                                                        seq_off.numel(), _p(seq_off), _p(seq_len), int(max_len), rows, num_heads, HD // num_heads, kv_seq_shift,
                                                        _stream()))
    return out


def layernorm(x, weight, bias, eps=1e-5):
    """nn.LayerNorm over the last dimension with affine parameters."""
    _chk(x, weight, bias)
    x = x.contiguous()
    out = torch.empty_like(x)
    D = x.shape[-1]
    check(load_library().mmdm_layernorm_f32(_p(x), _p(weight), _p(bias), _p(out), x.numel() // D, D, float(eps), _stream()))
    return out


def layernorm_split(x, weight, bias, eps=1e-5, build=0, planes=True):
    """nn.LayerNorm with affine parameters written as fp32 rows AND as their two fp16 planes (split_f32 of the rows) in one pass
    (mmdm_layernorm_split): returns (out fp32 like x, planes float16 [2, *x.shape]).  build: 0 = the row kernels behind `layernorm`, 1 = the build
    without packed-fp32 instructions that fp32_split / bf16 handles run.  planes=False: the plain LayerNorm of that build, returns (out, None)."""
    _chk(x, weight, bias)
    x = x.contiguous()
    out = torch.empty_like(x)
    D = x.shape[-1]
    n = x.numel()
    stride = (n + 7) // 8 * 8                # the plane stride is a multiple of 8 elements (a 4-element tensor gets a padded buffer and a view of it)
    buf = torch.empty(2, stride, device=x.device, dtype=torch.float16) if planes else None
    check(load_library().mmdm_layernorm_split(_p(x), _p(weight), _p(bias), _p(out), _p(buf), stride, n // D, D, float(eps), int(build), _stream()))
    return out, (buf[:, :n].reshape(2, *x.shape) if planes else None)


def token_embed(table, tokens, pos, build=0):
    """table[tokens] + pos[:L]; tokens int32 [n, L] on the device.  build as in `adaln`."""
    _chk(table, tokens, pos)
    assert tokens.dtype == torch.int32 and tokens.is_contiguous() and table.is_contiguous() and pos.is_contiguous()
    n, L = tokens.shape
    D = table.shape[1]
    assert pos.shape[0] >= L and pos.shape[1] == D
    out = torch.empty(n, L, D, device=table.device, dtype=torch.float32)
    if build == 0:
        check(load_library().mmdm_token_embed_f32(_p(table), table.shape[0], _p(tokens), _p(pos), _p(out), n, L, D, _stream()))
    else:
        check(load_library().mmdm_rowop_token_embed(_p(table), table.shape[0], _p(tokens), _p(pos), _p(out), n, L, D, int(build), _stream()))
    return out


def gather_rows(src, idx):
    """src [R, D][idx] with idx int32 [n] on the device."""
    _chk(src, idx)
    assert idx.dtype == torch.int32 and src.is_contiguous() and src.dim() == 2
    out = torch.empty(idx.shape[0], src.shape[1], device=src.device, dtype=torch.float32)
    check(load_library().mmdm_gather_rows_f32(_p(src), _p(idx), _p(out), idx.shape[0], src.shape[1], _stream()))
    return out


def encoder_layer_(x, w, num_heads, norm_first=False, activation="gelu", causal=False, eps=1e-5, workspace=None):
    """One nn.TransformerEncoderLayer on x [nseq, T, D] IN PLACE.  w: dict with in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias,
    linear1.weight/bias, linear2.weight/bias, norm1.weight/bias, norm2.weight/bias (contiguous fp32 device tensors)."""
    names = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "linear1.weight", "linear1.bias",
             "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
    ts = [w[k] for k in names]
    _chk(x, *ts)
    assert x.is_contiguous() and all(t.is_contiguous() for t in ts)
    nseq, T, D = x.shape
    F = w["linear1.weight"].shape[0]
    lib = load_library()
    need = lib.mmdm_encoder_layer_workspace(nseq, T, D, F)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    cw = EncoderLayerWeights(*[t.data_ptr() for t in ts])
    check(lib.mmdm_encoder_layer_f32(_p(x), C.byref(cw), nseq, T, D, num_heads, F, int(norm_first), EPI[activation], int(causal), float(eps),
                                     _p(workspace), workspace.numel(), _stream()))
    return x


def _seq_args(seq_off, seq_len):
    _chk(seq_off, seq_len)
    assert seq_off.dtype == torch.int32 and seq_len.dtype == torch.int32 and seq_off.is_contiguous() and seq_len.is_contiguous()
    assert seq_off.dim() == 1 and seq_off.numel() == seq_len.numel()
    return seq_off.numel(), _p(seq_off), _p(seq_len)


def encoder_layer_ragged_(x, w, num_heads, seq_off, seq_len, max_len, norm_first=False, activation="gelu", eps=1e-5, workspace=None):
    """One post-norm nn.TransformerEncoderLayer on a ragged batch, x [total_rows, D] IN PLACE (mmdm_encoder_layer_ragged_f32): sequence s = rows
    [seq_off[s], seq_off[s] + seq_len[s]) (int32 device tensors), plain softmax over its own keys; max_len >= every length.  Every sequence's rows are
    bitwise those of encoder_layer_ on that sequence alone.  w as in encoder_layer_.  Head sizes 64 / 128; norm_first is refused by the library."""
    names = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "linear1.weight", "linear1.bias",
             "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
    ts = [w[k] for k in names]
    _chk(x, *ts)
    assert x.dim() == 2 and x.is_contiguous() and all(t.is_contiguous() for t in ts)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    rows, D = x.shape
    F = w["linear1.weight"].shape[0]
    lib = load_library()
    need = lib.mmdm_encoder_layer_workspace(1, rows, D, F)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    cw = EncoderLayerWeights(*[t.data_ptr() for t in ts])
    check(lib.mmdm_encoder_layer_ragged_f32(_p(x), C.byref(cw), nseq, po, pl, int(max_len), rows, D, num_heads, F, int(norm_first), EPI[activation], float(eps),
                                            _p(workspace), workspace.numel(), _stream()))
    return x


def motion_pack(motions, seq_off, seq_len, max_len, total_rows, npers=2, k_pad=None, build=0, out=None):
    """The InterCLIP motion encoder's embedding operand (mmdm_rowop_motion_pack): motions [B, Tpad, npers * 262] (last-dim stride 1) -> A [total_rows, k_pad]
    with frame t of item s at row seq_off[s] + 1 + t, the last 4 features of every person dropped, the columns from npers * 258 on and the token rows
    (seq_off[s]) zeros.  Item s is seq_len[s] rows: its token and its first seq_len[s] - 1 frames; frames beyond are never read.  k_pad: npers * 258
    rounded up to a multiple of 16 unless given.  Rows outside every sequence are left as they are in `out` (a new tensor: uninitialised).  build as in
    `adaln`."""
    _chk(motions)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    assert motions.dim() == 3 and motions.stride(2) == 1 and motions.shape[0] == nseq and motions.shape[2] == npers * 262
    K = npers * 258
    k_pad = (K + 15) // 16 * 16 if k_pad is None else int(k_pad)
    if out is None:
        out = torch.empty(total_rows, k_pad, device=motions.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= total_rows and out.shape[1] == k_pad
    check(load_library().mmdm_rowop_motion_pack(_p(motions), motions.stride(0), motions.stride(1), motions.shape[1], int(npers), _p(out), out.stride(0), k_pad,
                                                nseq, po, pl, int(max_len), int(total_rows), int(build), _stream()))
    return out


def motion_tokens_(h, query_token, pe, seq_off, seq_len, max_len, build=0):
    """IN PLACE on the embedding GEMM's output h [total_rows, D] (mmdm_rowop_motion_tokens): row seq_off[s] = query_token + pe[0], row seq_off[s] + 1 + t
    += pe[1 + t].  query_token [D] or [1, D], pe [rows, D] contiguous.  build as in `adaln`."""
    _chk(h, query_token, pe)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    assert h.dim() == 2 and h.is_contiguous() and pe.dim() == 2 and pe.is_contiguous() and query_token.is_contiguous()
    rows, D = h.shape
    assert pe.shape[1] == D and query_token.numel() == D
    check(load_library().mmdm_rowop_motion_tokens(_p(h), _p(query_token), _p(pe), pe.shape[0], D, nseq, po, pl, int(max_len), rows, int(build), _stream()))
    return h


def center_motion(motions, npers=2, out=None):
    """smpl_to_ih(center_motion(ih_to_smpl(.))) of every person of every item on its own (mmdm_center_motion_f32): motions [B, Tpad, npers * 262]
    (last-dim stride 1) -> a new tensor of that shape, all Tpad frames; channels 258..261 of every person are 0.  The floor is the minimum of position Y
    over ALL Tpad frames of the buffer, not over an item's length (the reference centres the padded buffer); frame 0 supplies the root XZ and the facing.
    The cross product runs along the last dimension for every B: the reference's torch.cross without dim goes wrong at a per-call batch of exactly 3,
    which is not reproduced.  `out` must not overlap `motions`."""
    _chk(motions, out)
    assert motions.dim() == 3 and motions.stride(2) == 1 and motions.shape[2] == npers * 262
    B, T, _ = motions.shape
    if out is None:
        out = torch.empty(B, T, npers * 262, device=motions.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == motions.shape and out.stride(2) == 1
    floor_ws = torch.empty(max(B * npers, 1), device=motions.device, dtype=torch.float32)
    check(load_library().mmdm_center_motion_f32(_p(motions), motions.stride(0), motions.stride(1), T, B, int(npers), _p(out), out.stride(0), out.stride(1),
                                                _p(floor_ws), _stream()))
    return out


def center_pack(motions, seq_off, seq_len, max_len, total_rows, k_pad=None, out=None):
    """The embedding operand of the InterCLIP INDIVIDUAL evaluator in one pass (mmdm_center_pack_f32): motions [B, Tpad, 524] -> A [total_rows, k_pad], bitwise
    motion_pack(center_motion(motions).view(2B, Tpad, 262), ..., npers=1).  Sequence 2 * i + p is person p of item i (seq_off / seq_len int32 device tensors
    [2B]): token row and columns from 258 on zeros, frame t at row seq_off[s] + 1 + t.  Frames at and beyond a length are neither transformed nor written,
    but their position Y enters the floor (see center_motion).  k_pad: 272 unless given.  Rows outside every sequence are left as they are in `out` (a new
    tensor: uninitialised)."""
    _chk(motions)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    assert motions.dim() == 3 and motions.stride(2) == 1 and motions.shape[2] == 524 and nseq == 2 * motions.shape[0]
    k_pad = (258 + 15) // 16 * 16 if k_pad is None else int(k_pad)
    if out is None:
        out = torch.empty(total_rows, k_pad, device=motions.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= total_rows and out.shape[1] == k_pad
    floor_ws = torch.empty(max(nseq, 1), device=motions.device, dtype=torch.float32)
    check(load_library().mmdm_center_pack_f32(_p(motions), motions.stride(0), motions.stride(1), motions.shape[1], motions.shape[0], _p(out), out.stride(0), k_pad,
                                              po, pl, int(max_len), int(total_rows), _p(floor_ws), _stream()))
    return out


def _planes_out(out, rows, ld, device):
    """A contiguous float16 [2, n] buffer whose row length n is the plane stride (n >= rows * ld, a multiple of 8); created unless given."""
    if out is None:
        out = torch.empty(2, (rows * ld + 7) // 8 * 8, device=device, dtype=torch.float16)
    assert out.is_cuda and out.dtype == torch.float16 and out.dim() == 2 and out.shape[0] == 2 and out.is_contiguous() and out.shape[1] >= rows * ld
    return out


def split_k_pad(npers):
    """Columns of the evaluator's embedding operand in the fp32_split mode: npers * 258 rounded up to a multiple of 32 (the split GEMM needs K % 32 == 0):
    544 for two persons, 288 for one."""
    return (int(npers) * 258 + 31) // 32 * 32


def motion_pack_split(motions, seq_off, seq_len, max_len, total_rows, npers=2, k_pad=None, build=1, out=None):
    """motion_pack written directly as the two fp16 planes of the split embedding GEMM's A operand (mmdm_rowop_motion_pack_split): returns float16
    [2, total_rows, k_pad], bitwise split_f32 of motion_pack's result in the rows of the sequences (pad columns and token rows +0 in both planes); other
    rows are left as they are in `out` (a contiguous float16 [2, n >= total_rows * k_pad] buffer; new: uninitialised).  k_pad: split_k_pad(npers) unless given."""
    _chk(motions)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    assert motions.dim() == 3 and motions.stride(2) == 1 and motions.shape[0] == nseq and motions.shape[2] == npers * 262
    k_pad = split_k_pad(npers) if k_pad is None else int(k_pad)
    out = _planes_out(out, total_rows, k_pad, motions.device)
    check(load_library().mmdm_rowop_motion_pack_split(_p(motions), motions.stride(0), motions.stride(1), motions.shape[1], int(npers), _p(out), k_pad, out.shape[1],
                                                      k_pad, nseq, po, pl, int(max_len), int(total_rows), int(build), _stream()))
    return out[:, :total_rows * k_pad].unflatten(1, (total_rows, k_pad))


def center_pack_split(motions, seq_off, seq_len, max_len, total_rows, k_pad=None, out=None):
    """center_pack written directly as the two fp16 planes of the split embedding GEMM's A operand (mmdm_center_pack_split): float16 [2, total_rows, k_pad],
    bitwise split_f32 of center_pack's result in the rows of the sequences.  k_pad: 288 unless given; `out` as in motion_pack_split."""
    _chk(motions)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    assert motions.dim() == 3 and motions.stride(2) == 1 and motions.shape[2] == 524 and nseq == 2 * motions.shape[0]
    k_pad = split_k_pad(1) if k_pad is None else int(k_pad)
    out = _planes_out(out, total_rows, k_pad, motions.device)
    floor_ws = torch.empty(max(nseq, 1), device=motions.device, dtype=torch.float32)
    check(load_library().mmdm_center_pack_split(_p(motions), motions.stride(0), motions.stride(1), motions.shape[1], motions.shape[0], _p(out), k_pad, out.shape[1], k_pad,
                                                po, pl, int(max_len), int(total_rows), _p(floor_ws), _stream()))
    return out[:, :total_rows * k_pad].unflatten(1, (total_rows, k_pad))


def motion_tokens_split_(h, query_token, pe, seq_off, seq_len, max_len, build=1, planes=None):
    """motion_tokens_ that also writes the rows' two fp16 planes in the same pass (mmdm_rowop_motion_tokens_split): IN PLACE on h [total_rows, D], returns
    (h, planes float16 [2, total_rows, D]) with planes == split_f32(h) in the rows of the sequences.  planes: a contiguous float16 [2, n >= total_rows * D]
    buffer (n = the plane stride), created unless given."""
    _chk(h, query_token, pe)
    nseq, po, pl = _seq_args(seq_off, seq_len)
    assert h.dim() == 2 and h.is_contiguous() and pe.dim() == 2 and pe.is_contiguous() and query_token.is_contiguous()
    rows, D = h.shape
    assert pe.shape[1] == D and query_token.numel() == D
    planes = _planes_out(planes, rows, D, h.device)
    check(load_library().mmdm_rowop_motion_tokens_split(_p(h), _p(planes), planes.shape[1], _p(query_token), _p(pe), pe.shape[0], D, nseq, po, pl, int(max_len), rows,
                                                        int(build), _stream()))
    return h, planes[:, :rows * D].unflatten(1, (rows, D))


_SPLIT_LAYER_NAMES = ("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight", "in_proj_bias", "out_proj.bias", "linear1.bias", "linear2.bias",
                      "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def split_weight(w, pack=None):
    """The fp16-plane twin of an fp32 weight [N, K] for linear_split: (float16 [2, N, K], packed) -- split_f32 of it, in fragment order (split_pack_weight)
    when `pack` (default: whenever the packed kernel covers the shape, N % 64 == 0 and K % 64 == 0; results are bit-identical either way)."""
    _chk(w)
    assert w.dim() == 2
    N, K = w.shape
    if pack is None:
        pack = N % 64 == 0 and K % 64 == 0
    ws = split_f32(w)
    return (split_pack_weight(ws), True) if pack else (ws, False)


def encoder_layer_split_weights(w, pack=None):
    """The weights of encoder_layer_split_ / encoder_layer_ragged_split_ from the fp32 dict of encoder_layer_: the four GEMM matrices as fp16 planes -- all in
    fragment order when `pack` (default: D % 64 == 0 and F % 64 == 0), all plain otherwise -- the biases and norms as they are.  Returns a dict with the
    names of encoder_layer_ plus "packed"."""
    F, D = w["linear1.weight"].shape
    if pack is None:
        pack = D % 64 == 0 and F % 64 == 0
    out = {k: w[k].contiguous() for k in _SPLIT_LAYER_NAMES[4:]}
    for k in _SPLIT_LAYER_NAMES[:4]:
        out[k] = split_weight(w[k].contiguous(), pack)[0]
    out["packed"] = bool(pack)
    return out


def _split_layer_args(x, xs, w):
    ts = [w[k] for k in _SPLIT_LAYER_NAMES]
    _chk(x, *ts[4:])
    for t in ts[:4]:
        if not t.is_cuda or t.dtype != torch.float16 or t.dim() != 3 or t.shape[0] != 2 or not t.is_contiguous():
            raise TypeError("encoder_layer_split_: the GEMM weights are contiguous CUDA float16 [2, N, K] planes (ops.encoder_layer_split_weights)")
    if not xs.is_cuda or xs.dtype != torch.float16 or xs.shape[0] != 2 or xs.stride(-1) != 1 or tuple(xs.shape[1:]) != tuple(x.shape):
        raise TypeError("encoder_layer_split_: xs is the float16 planes [2, *x.shape] of x (ops.split_f32)")
    assert x.is_contiguous() and xs[0].is_contiguous() and xs[1].is_contiguous() and all(t.is_contiguous() for t in ts)
    return EncoderLayerSplitWeights(*[t.data_ptr() for t in ts], int(bool(w["packed"]))), w["linear1.weight"].shape[1]


def encoder_layer_split_(x, xs, w, num_heads, norm_first=False, eps=1e-5, last=False, workspace=None):
    """One post-norm nn.TransformerEncoderLayer (gelu) on SPLIT operands, x [nseq, T, D] fp32 IN PLACE and xs, its float16 planes [2, nseq, T, D], rewritten
    for the next layer (mmdm_encoder_layer_split; last=True skips the final plane write).  w: ops.encoder_layer_split_weights.  Head sizes 64 / 128 run the
    two-plane attention, any other <= 256 the fp32 attention.  Returns x."""
    cw, F = _split_layer_args(x, xs, w)
    nseq, T, D = x.shape
    lib = load_library()
    need = lib.mmdm_encoder_layer_split_workspace(nseq, T, D, F)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    check(lib.mmdm_encoder_layer_split(_p(x), _p(xs), xs.stride(0), C.byref(cw), nseq, T, D, num_heads, F, int(norm_first), float(eps), int(last),
                                       _p(workspace), workspace.numel(), _stream()))
    return x


def encoder_layer_ragged_split_(x, xs, w, num_heads, seq_off, seq_len, max_len, norm_first=False, eps=1e-5, last=False, workspace=None):
    """encoder_layer_split_ on a ragged batch, x [total_rows, D] and xs [2, total_rows, D] IN PLACE (mmdm_encoder_layer_ragged_split): sequences as in
    encoder_layer_ragged_; every sequence's rows are bitwise those of encoder_layer_split_ on that sequence alone.  Head sizes 64 / 128."""
    cw, F = _split_layer_args(x, xs, w)
    assert x.dim() == 2
    nseq, po, pl = _seq_args(seq_off, seq_len)
    rows, D = x.shape
    lib = load_library()
    need = lib.mmdm_encoder_layer_split_workspace(1, rows, D, F)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.float32)
    check(lib.mmdm_encoder_layer_ragged_split(_p(x), _p(xs), xs.stride(0), C.byref(cw), nseq, po, pl, int(max_len), rows, D, num_heads, F, int(norm_first),
                                              float(eps), int(last), _p(workspace), workspace.numel(), _stream()))
    return x


def l2_normalize(x, scale, build=0):
    """x / ||x||_2 * scale over the last dimension (mmdm_l2_normalize_rows_f32); scale: a one-element fp32 DEVICE tensor (InterCLIP's latent_scale).
    build as in `adaln`."""
    _chk(x, scale)
    assert scale.numel() == 1
    x = x.contiguous()
    out = torch.empty_like(x)
    D = x.shape[-1]
    if build == 0:
        check(load_library().mmdm_l2_normalize_rows_f32(_p(x), _p(scale), _p(out), x.numel() // D, D, _stream()))
    else:
        check(load_library().mmdm_rowop_l2_normalize(_p(x), _p(scale), _p(out), x.numel() // D, D, int(build), _stream()))
    return out


def cond_silu(time_tab, step_idx, txt, build=0, planes=False, out=None):
    """silu(time_tab[*step_idx] + txt) for txt [rows, D].  build as in `adaln`.  planes: the values as their two fp16 planes instead (float16; `out`, if
    given, is a contiguous float16 tensor [2, n >= rows * D] whose row length n is the plane stride)."""
    _chk(time_tab, step_idx, txt)
    rows, D = txt.shape
    if not planes:
        out = torch.empty_like(txt)
        if build == 0:
            check(load_library().mmdm_cond_silu_f32(_p(time_tab), _p(step_idx), _p(txt), _p(out), rows, D, _stream()))
        else:
            check(load_library().mmdm_rowop_cond_silu(_p(time_tab), _p(step_idx), _p(txt), _p(out), 0, 0, rows, D, int(build), _stream()))
        return out
    if out is None:
        out = torch.empty(2, rows * D, device=txt.device, dtype=torch.float16)
    assert out.is_cuda and out.dtype == torch.float16 and out.dim() == 2 and out.shape[0] == 2 and out.is_contiguous()
    check(load_library().mmdm_rowop_cond_silu(_p(time_tab), _p(step_idx), _p(txt), C.c_void_p(out.data_ptr()), 1, out.shape[1], rows, D, int(build), _stream()))
    return out


def mixer_pre(o1, o2, stats, align=True, last_frame=None):
    """last_frame: int32 [rows] on the device -- the frame the alignment's displacement of batch row b ends at (row b % rows); None = T - 1."""
    _chk(o1, o2, stats, last_frame)
    n, T, _ = o1.shape
    out1, out2 = torch.empty_like(o1), torch.empty_like(o2)
    if last_frame is not None:
        assert last_frame.dtype == torch.int32 and last_frame.is_contiguous() and last_frame.dim() == 1
        check(load_library().mmdm_mixer_pre_masked_f32(_p(o1.contiguous()), _p(o2.contiguous()), _p(stats), _p(out1), _p(out2), n, T, int(align),
                                                       _p(last_frame), last_frame.shape[0], _stream()))
        return out1, out2
    check(load_library().mmdm_mixer_pre_f32(_p(o1.contiguous()), _p(o2.contiguous()), _p(stats), _p(out1), _p(out2), n, T, int(align), _stream()))
    return out1, out2


def influence_head(h, weight, bias):
    _chk(h, weight, bias)
    D = h.shape[-1]
    rows = h.numel() // D
    nw = weight.shape[0]
    w = torch.empty(*h.shape[:-1], nw, device=h.device, dtype=torch.float32)
    check(load_library().mmdm_influence_head_f32(_p(h.contiguous()), _p(weight.contiguous()), _p(bias), _p(w), rows, D, nw, _stream()))
    return w


def mean_time(h, build=0, seq_off=None, seq_len=None):
    """Mean over time of h [nseq, T, D]; with seq_off / seq_len (int32 device tensors [nseq]) the ragged form on h [rows, D]: sequence s = rows
    [seq_off[s], seq_off[s] + seq_len[s]).  build as in `adaln`."""
    _chk(h, seq_off, seq_len)
    h = h.contiguous()
    if seq_off is not None or seq_len is not None:
        assert h.dim() == 2 and seq_off.dtype == torch.int32 and seq_len.dtype == torch.int32 and seq_off.numel() == seq_len.numel()
        nseq, D = seq_off.numel(), h.shape[1]
        out = torch.empty(nseq, D, device=h.device, dtype=torch.float32)
        check(load_library().mmdm_rowop_mean_time(_p(h), _p(out), nseq, 0, _p(seq_off), _p(seq_len), D, int(build), _stream()))
        return out
    nseq, T, D = h.shape
    out = torch.empty(nseq, D, device=h.device, dtype=torch.float32)
    if build == 0:
        check(load_library().mmdm_mean_time_f32(_p(h), _p(out), nseq, T, D, _stream()))
    else:
        check(load_library().mmdm_rowop_mean_time(_p(h), _p(out), nseq, T, None, None, D, int(build), _stream()))
    return out


def mdm_pack(src, cond, time_tab, step_idx, pe, build=0, planes=False):
    """MDMDenoiser's sequence assembly: src [nseq, T, D], cond [nseq, D] (may be a column slice of a wider tensor) -> dst [nseq, T + 1, D] with the
    conditioning token (cond + time_tab[*step_idx]) + pe[0] in front of every sequence.  planes: returns (dst, float16 [2, nseq, T + 1, D]).
    build as in `adaln`."""
    _chk(src, cond, time_tab, step_idx, pe)
    src = src.contiguous()
    nseq, T, D = src.shape
    assert cond.shape == (nseq, D) and cond.stride(1) == 1 and time_tab.is_contiguous() and pe.is_contiguous()
    dst = torch.empty(nseq, T + 1, D, device=src.device, dtype=torch.float32)
    n = dst.numel()
    stride = (n + 7) // 8 * 8                # the plane stride is a multiple of 8 elements
    buf = torch.empty(2, stride, device=src.device, dtype=torch.float16) if planes else None
    check(load_library().mmdm_rowop_mdm_pack(_p(src), _p(cond), cond.stride(0), _p(time_tab), _p(step_idx), _p(pe), _p(dst), _p(buf), stride,
                                             nseq, T, D, int(build), _stream()))
    return (dst, buf[:, :n].reshape(2, nseq, T + 1, D)) if planes else dst


def mdm_unpack(src, build=0):
    """src [nseq, T + 1, D] -> [nseq, T, D] without the conditioning token."""
    _chk(src)
    src = src.contiguous()
    nseq, T1, D = src.shape
    dst = torch.empty(nseq, T1 - 1, D, device=src.device, dtype=torch.float32)
    check(load_library().mmdm_rowop_mdm_unpack(_p(src), _p(dst), nseq, T1 - 1, D, int(build), _stream()))
    return dst


def _rag_args(maps, rows):
    row_item, row_pos, item_off, item_len = maps
    _chk(*maps)
    for t in maps:
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert row_item.numel() == rows and row_pos.numel() == rows and item_off.numel() == item_len.numel()
    return [rows, _p(row_item), _p(row_pos), _p(item_off), _p(item_len)]


def mdm_pack_rag(src, cond, time_tab, step_idx, pe, fr, tk, tk_rows, gpp, build=0, dst=None, planes=None):
    """mdm_pack on a ragged batch (mmdm_rowop_mdm_pack_rag): src [groups, fr_rows, D]; fr / tk = (row_item, row_pos, item_off, item_len) int32 device
    tensors of the frame and the token row space; cond [gpp * B, >= persons * D].  dst [groups, tk_rows, D] (or more rows: what lies behind the
    last group is not written) is created unless given; planes: a contiguous float16 [2, n] tensor (n >= groups * tk_rows * D = the plane stride).
    Returns dst."""
    _chk(src, cond, time_tab, step_idx, pe)
    src = src.contiguous()
    groups, fr_rows, D = src.shape
    B = fr[2].numel()
    assert cond.stride(1) == 1 and cond.shape[0] >= gpp * B
    if dst is None:
        dst = torch.empty(groups, tk_rows, D, device=src.device, dtype=torch.float32)
    assert dst.is_contiguous() and dst.numel() >= groups * tk_rows * D
    stride = 0
    if planes is not None:
        assert planes.is_cuda and planes.dtype == torch.float16 and planes.dim() == 2 and planes.shape[0] == 2 and planes.is_contiguous()
        stride = planes.shape[1]
    check(load_library().mmdm_rowop_mdm_pack_rag(_p(src), _p(cond), cond.stride(0), _p(time_tab), _p(step_idx), _p(pe), _p(dst), _p(planes), stride,
                                                 groups, int(gpp), D, B, *_rag_args(fr, fr_rows), *_rag_args(tk, tk_rows), int(build), _stream()))
    return dst


def mdm_unpack_rag(src, fr, tk, fr_rows, build=0, dst=None):
    """mdm_unpack on a ragged batch: src [groups, tk_rows, D] -> dst [groups, fr_rows, D] (created unless given), padding frame rows zeros."""
    _chk(src)
    src = src.contiguous()
    groups, tk_rows, D = src.shape
    if dst is None:
        dst = torch.empty(groups, fr_rows, D, device=src.device, dtype=torch.float32)
    assert dst.is_contiguous() and dst.numel() >= groups * fr_rows * D
    check(load_library().mmdm_rowop_mdm_unpack_rag(_p(src), _p(dst), groups, D, fr[2].numel(), *_rag_args(fr, fr_rows), *_rag_args(tk, tk_rows),
                                                   int(build), _stream()))
    return dst


def blend_cfg(out1, out2, w, mode, cfg_scale, force=None, want_hist=False):
    """out1/out2 [2B,T,524]; w [2, 2B, Tw, nw].  Returns model_out [B,T,524] (+ influence_i1, influence_i2, out_influenced)."""
    _chk(out1, out2, w)
    n, T, _ = out1.shape
    B = n // 2
    mo = torch.empty(B, T, 524, device=out1.device, dtype=torch.float32)
    h1 = h2 = hm = None
    if want_hist:
        h1 = torch.empty(n, T, 262, device=out1.device, dtype=torch.float32)
        h2 = torch.empty_like(h1)
        hm = torch.empty_like(out1)
    check(load_library().mmdm_blend_cfg_f32(_p(out1.contiguous()), _p(out2.contiguous()), _p(w.contiguous()), mode, int(force is not None),
                                            float(force or 0.0), float(cfg_scale), _p(mo), _p(h1), _p(h2), _p(hm), B, T, _stream()))
    return (mo, h1, h2, hm) if want_hist else mo


def xstart_ddim(model_out, stats, coef, step_idx, x, x2, align=True):
    """In place on x, x2.  Returns (pred_xstart, pred_xstart2)."""
    _chk(model_out, stats, coef, step_idx, x, x2)
    B, T, _ = model_out.shape
    S = coef.shape[1]
    p1, p2 = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(2 * B, device=x.device, dtype=torch.float32)
    check(load_library().mmdm_xstart_ddim_f32(_p(model_out.contiguous()), _p(stats), _p(coef), S, _p(step_idx), _p(x), _p(x2), _p(p1), _p(p2),
                                              _p(ws), B, T, int(align), _stream()))
    return p1, p2


def randn(seed, loop_pos, B, T, device=None):
    """mmdm_randn_f32: [B, T, 524] = exactly the N(0, 1) values the eta > 0 sampler adds at loop position `loop_pos` of a call begun with
    seed=`seed` (Philox4x32-10 counted by the element's own (t, column, b): independent of B and T)."""
    if not torch.cuda.is_available():
        raise RuntimeError("mixermdm_amd ops run on the GPU only (no CPU fallback)")
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    out = torch.empty(B, T, 524, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(load_library().mmdm_randn_f32(int(seed) & 0xFFFFFFFFFFFFFFFF, int(loop_pos), B, T, _p(out), _stream()))
    return out


def cfg_ddim(m, coef, step_idx, cfg_scale, x):
    _chk(m, coef, step_idx, x)
    B, T, Cc = x.shape
    p = torch.empty_like(x)
    check(load_library().mmdm_cfg_ddim_f32(_p(m.contiguous()), _p(coef), coef.shape[1], _p(step_idx), float(cfg_scale), _p(x), _p(p), B, T, Cc, _stream()))
    return p


def _pred_out(pred_xstart, x):
    """pred_xstart of a single-chain update: True -> a new tensor, False / None -> not written, a tensor -> written in place."""
    if pred_xstart is True:
        return torch.empty_like(x)
    if pred_xstart is False or pred_xstart is None:
        return None
    _chk(pred_xstart)
    assert pred_xstart.shape == x.shape and pred_xstart.is_contiguous()
    return pred_xstart


def cfg4_ddim(m, coef, step_idx, s, s_int, s_ind, x, pred_xstart=True):
    """mmdm_cfg4_ddim_f32: m [4B, T, C] = full | interaction-only | individuals-only | uncond rows; x [B, T, C] in place.  Returns pred_xstart (or None)."""
    _chk(m, coef, step_idx, x)
    B, T, Cc = x.shape
    assert m.shape == (4 * B, T, Cc) and x.is_contiguous()
    p = _pred_out(pred_xstart, x)
    check(load_library().mmdm_cfg4_ddim_f32(_p(m.contiguous()), _p(coef), coef.shape[1], _p(step_idx), float(s), float(s_int), float(s_ind), _p(x), _p(p), B, T, Cc,
                                            _stream()))
    return p


def dual_ddim(m_ind, m_int, coef, step_idx, w_table, s_ind, s_int, x, pred_xstart=True):
    """mmdm_dual_ddim_f32: m_ind / m_int [2B, T, C] = cond | uncond rows of the two models, w_table [S] fp32 on the device; x [B, T, C] in place.  Returns
    pred_xstart (or None)."""
    _chk(m_ind, m_int, coef, step_idx, w_table, x)
    B, T, Cc = x.shape
    assert m_ind.shape == m_int.shape == (2 * B, T, Cc) and x.is_contiguous() and w_table.dtype == torch.float32 and w_table.numel() == coef.shape[1]
    p = _pred_out(pred_xstart, x)
    check(load_library().mmdm_dual_ddim_f32(_p(m_ind.contiguous()), _p(m_int.contiguous()), _p(coef), coef.shape[1], _p(step_idx), _p(w_table.contiguous()),
                                            float(s_ind), float(s_int), _p(x), _p(p), B, T, Cc, _stream()))
    return p


def gaussian_filter1d(x, sigma=1.0, truncate=4.0):
    """scipy.ndimage.gaussian_filter1d(x, sigma, axis=-2, mode="nearest") for x [..., T, C] on the GPU."""
    import numpy as np
    _chk(x)
    x = x.contiguous()
    T, Cc = x.shape[-2], x.shape[-1]
    n = x.numel() // (T * Cc) if x.numel() else 0
    radius = int(truncate * float(sigma) + 0.5)            # scipy: lw = int(truncate * sd + 0.5)
    k = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)            # scipy.ndimage._filters._gaussian_kernel1d, order 0
    w = w / w.sum()
    wd = torch.from_numpy(w).to(x.device)
    out = torch.empty_like(x)
    check(load_library().mmdm_gaussian_filter1d_f32(_p(x), _p(out), C.c_void_p(wd.data_ptr()), radius, n, T, Cc, _stream()))
    return out


def to_bf16(x):
    """fp32 -> bf16 (RNE) on the GPU; returns a torch.bfloat16 tensor of the same shape."""
    _chk(x)
    x = x.contiguous()
    out = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(load_library().mmdm_f32_to_bf16(_p(x), C.c_void_p(out.data_ptr()), x.numel(), _stream()))
    return out


def pack_weight_frag(w):
    """A static bf16 or fp8 weight [N, K] -> the same bytes in MFMA fragment order (blocks of 32 rows x 32 bytes), for linear_bf16 /
    linear_fp8 (..., packed=True).  N % 32 == 0 and 32 | bytes per row; the result keeps shape and dtype so N and K can be read back."""
    if not w.is_cuda or w.dtype not in (torch.bfloat16, torch.float8_e4m3fn) or w.dim() != 2 or not w.is_contiguous():
        raise TypeError("pack_weight_frag expects a contiguous CUDA bfloat16 / float8_e4m3fn [N, K] tensor")
    N, K = w.shape
    rb = K * w.element_size()
    out = torch.empty_like(w)
    check(load_library().mmdm_pack_weight_frag(C.c_void_p(w.data_ptr()), rb, C.c_void_p(out.data_ptr()), N, rb, _stream()))
    return out


def linear_bf16(x, weight, bias=None, epilogue="bias", extra=None, period=0, out_dtype=torch.float32, packed=False):
    """y = x @ weight.T + bias with bf16 operands (x, weight torch.bfloat16), fp32 accumulation; fp32 or bf16 result.
    packed: weight comes from pack_weight_frag (W straight from global memory; bit-identical results)."""
    for t in (x, weight):
        if not t.is_cuda or t.dtype != torch.bfloat16:
            raise TypeError("linear_bf16 expects CUDA torch.bfloat16 operands")
    _chk(bias, extra)
    K, N = x.shape[-1], weight.shape[0]
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    out = torch.empty(M, N, device=x.device, dtype=out_dtype)
    if packed:
        check(load_library().mmdm_linear_bf16_packed(C.c_void_p(x2.data_ptr()), x2.stride(0), C.c_void_p(weight.data_ptr()), _p(bias),
                                                     C.c_void_p(out.data_ptr()), out.stride(0), int(out_dtype == torch.bfloat16), M, N, K, EPI[epilogue],
                                                     _p(extra), extra.stride(0) if extra is not None else 0, period, _stream()))
        return out.reshape(*x.shape[:-1], N)
    check(load_library().mmdm_linear_bf16(C.c_void_p(x2.data_ptr()), x2.stride(0), C.c_void_p(weight.data_ptr()), weight.stride(0), _p(bias),
                                          C.c_void_p(out.data_ptr()), out.stride(0), int(out_dtype == torch.bfloat16), M, N, K, EPI[epilogue],
                                          _p(extra), extra.stride(0) if extra is not None else 0, period, _stream()))
    return out.reshape(*x.shape[:-1], N)


SPLIT_SCALE = 2048.0


def split_f32(x):
    """Operand format of the fp32-split mode: [2, *x.shape] torch.float16 with x ~= out[0] + out[1] / 2048 (relative error <= 2^-22;
    out[0] = fp16(x), out[1] = fp16((x - out[0]) * 2048))."""
    _chk(x)
    x = x.contiguous()
    out = torch.empty(2, *x.shape, device=x.device, dtype=torch.float16)
    n = x.numel()
    check(load_library().mmdm_f32_split(_p(x), C.c_void_p(out.data_ptr()), n, n, _stream()))
    return out


def split_pack_weight(ws):
    """Split weights ws [2, N, K] (split_f32) -> the same elements in MFMA fragment order, for linear_split(..., packed=True).
    N % 32 == 0, K % 16 == 0; the result keeps the shape so that N and K can be read back from it."""
    if not ws.is_cuda or ws.dtype != torch.float16 or ws.dim() != 3 or ws.shape[0] != 2 or not ws.is_contiguous():
        raise TypeError("split_pack_weight expects a contiguous CUDA float16 [2, N, K] tensor (ops.split_f32)")
    _, N, K = ws.shape
    out = torch.empty_like(ws)
    check(load_library().mmdm_split_pack_weight(C.c_void_p(ws.data_ptr()), K, N * K, C.c_void_p(out.data_ptr()), N * K, N, K, _stream()))
    return out


def linear_split(xs, ws, bias=None, epilogue="bias", extra=None, period=0, split_out=False, packed=False):
    """fp32 y = x @ w.T + bias computed on the 16-bit matrix cores from two-way fp16 splits xs [2, M, K], ws [2, N, K] (split_f32).
    Returns fp32 [M, N], or its split [2, M, N] when split_out.  packed: ws comes from split_pack_weight (W straight from global memory
    in fragment order; bit-identical results)."""
    for t in (xs, ws):
        if not t.is_cuda or t.dtype != torch.float16 or t.shape[0] != 2 or not t.is_contiguous():
            raise TypeError("linear_split expects contiguous CUDA float16 [2, rows, K] operands (ops.split_f32)")
    _chk(bias, extra)
    _, M, K = xs.shape
    N = ws.shape[1]
    out = torch.empty((2, M, N) if split_out else (M, N), device=xs.device, dtype=torch.float16 if split_out else torch.float32)
    if packed:
        check(load_library().mmdm_linear_split_packed(C.c_void_p(xs.data_ptr()), K, M * K, C.c_void_p(ws.data_ptr()), N * K, _p(bias), C.c_void_p(out.data_ptr()), N,
                                                      M * N, int(split_out), M, N, K, EPI[epilogue], _p(extra), extra.stride(0) if extra is not None else 0, period, _stream()))
        return out
    check(load_library().mmdm_linear_split(C.c_void_p(xs.data_ptr()), K, M * K, C.c_void_p(ws.data_ptr()), K, N * K, _p(bias), C.c_void_p(out.data_ptr()), N,
                                           M * N, int(split_out), M, N, K, EPI[epilogue], _p(extra), extra.stride(0) if extra is not None else 0, period, _stream()))
    return out


def bf16_split3(x):
    """Exact 3-way bf16 split of an fp32 tensor (torch arithmetic): [3, *x.shape] torch.bfloat16 with x == out[0] + out[1] + out[2]; the
    operand format of attention_planes(NP = 3) (the split-mode GEMMs write it as their optional second output)."""
    x1 = x.bfloat16()
    r1 = x - x1.float()
    x2 = r1.bfloat16()
    return torch.stack([x1, x2, (r1 - x2.float()).bfloat16()])


def attention_planes(qp, kp, v, num_heads, kv_seq_shift=0, zero_key=True, causal=False):
    """Attention with Q K^T on the bf16 matrix cores.  qp [NP, nseq, Tq, H*dh], kp [NP, nseq, Tk, H*dh] torch.bfloat16 (NP = 3: exact three-way
    bf16 splits x = x1 + x2 + x3, see bf16_split3 -> fp32-accurate scores; NP = 1: bf16), v [nseq, Tk, H*dh] fp32 (may be a column slice).  Returns fp32 [nseq, Tq, H*dh]."""
    _chk(v)
    NP, nseq, Tq, HD = qp.shape
    Tk = kp.shape[2]
    assert qp.dtype == torch.bfloat16 and kp.dtype == torch.bfloat16 and qp.is_cuda and kp.is_cuda and kp.shape[0] == NP
    assert qp.stride(3) == 1 and kp.stride(3) == 1 and v.stride(2) == 1
    out = torch.empty(nseq, Tq, HD, device=v.device, dtype=torch.float32)
    flags = (0 if zero_key else ATTN_NO_ZERO_KEY) | (ATTN_CAUSAL if causal else 0)
    check(load_library().mmdm_attention_planes(C.c_void_p(qp.data_ptr()), qp.stride(2), qp.stride(0), C.c_void_p(kp.data_ptr()), kp.stride(2), kp.stride(0), NP,
                                               _p(v), v.stride(1), _p(out), HD, 0, flags, nseq, Tq, Tk, num_heads, HD // num_heads, kv_seq_shift, _stream()))
    return out


def attention_bf16(qb, kb, vb, num_heads, kv_seq_shift=0, zero_key=True, causal=False, out_dtype=torch.float32):
    """All-bf16 attention (BASELINE configs[4] path): qb [nseq, Tq, H*dh], kb / vb [nseq, Tk, H*dh] torch.bfloat16 (may be column slices of a
    packed projection copy); Q K^T and P.V on the bf16 matrix cores, fp32 softmax and accumulation.  Returns fp32 or bf16 [nseq, Tq, H*dh]."""
    for t in (qb, kb, vb):
        assert t.is_cuda and t.dtype == torch.bfloat16 and t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1)
    nseq, Tq, HD = qb.shape
    Tk = kb.shape[1]
    out = torch.empty(nseq, Tq, HD, device=qb.device, dtype=out_dtype)
    flags = (0 if zero_key else ATTN_NO_ZERO_KEY) | (ATTN_CAUSAL if causal else 0)
    check(load_library().mmdm_attention_bf16(C.c_void_p(qb.data_ptr()), qb.stride(1), C.c_void_p(kb.data_ptr()), kb.stride(1), C.c_void_p(vb.data_ptr()), vb.stride(1),
                                             C.c_void_p(out.data_ptr()), HD, int(out_dtype == torch.bfloat16), flags, nseq, Tq, Tk, num_heads, HD // num_heads,
                                             kv_seq_shift, _stream()))
    return out


def attention_split(qs, ks, vs, num_heads, kv_seq_shift=0, zero_key=True, causal=False, split_out=False, key_padding_mask=None):
    """Attention of the fp32-split mode: qs [2, nseq, Tq, H*dh], ks / vs [2, nseq, Tk, H*dh] torch.float16 planes (split_f32; may be column
    slices of a packed projection written with split_out); scores and P.V from three fp16 MFMAs per block with hi / lo accumulators, fp32 softmax.
    Returns fp32 [nseq, Tq, H*dh] or its two planes.
    key_padding_mask: bool [rows, Tk] in PyTorch's sense (True = ignore the key), as for attention(); key sequence s reads row s % rows
    (mmdm_attention_split_masked)."""
    for t in (qs, ks, vs):
        assert t.is_cuda and t.dtype == torch.float16 and t.shape[0] == 2 and t.stride(3) == 1 and t.stride(1) == t.shape[2] * t.stride(2)
    _, nseq, Tq, HD = qs.shape
    Tk = ks.shape[2]
    out = torch.empty((2, nseq, Tq, HD) if split_out else (nseq, Tq, HD), device=qs.device, dtype=torch.float16 if split_out else torch.float32)
    flags = (0 if zero_key else ATTN_NO_ZERO_KEY) | (ATTN_CAUSAL if causal else 0)
    if key_padding_mask is not None:
        if not key_padding_mask.is_cuda or key_padding_mask.dtype != torch.bool or key_padding_mask.dim() != 2 or key_padding_mask.shape[1] != Tk:
            raise TypeError("key_padding_mask: a CUDA bool tensor [rows, Tk] is expected (True = ignore)")
        valid = (~key_padding_mask).to(torch.uint8).contiguous()
        check(load_library().mmdm_attention_split_masked(C.c_void_p(qs.data_ptr()), qs.stride(2), qs.stride(0), C.c_void_p(ks.data_ptr()), ks.stride(2), ks.stride(0),
                                                         C.c_void_p(vs.data_ptr()), vs.stride(2), vs.stride(0), C.c_void_p(out.data_ptr()), HD, 2 if split_out else 0, flags,
                                                         nseq, Tq, Tk, num_heads, HD // num_heads, kv_seq_shift, C.c_void_p(valid.data_ptr()), valid.shape[0], _stream()))
        return out
    check(load_library().mmdm_attention_split(C.c_void_p(qs.data_ptr()), qs.stride(2), qs.stride(0), C.c_void_p(ks.data_ptr()), ks.stride(2), ks.stride(0),
                                              C.c_void_p(vs.data_ptr()), vs.stride(2), vs.stride(0), C.c_void_p(out.data_ptr()), HD, 2 if split_out else 0, flags,
                                              nseq, Tq, Tk, num_heads, HD // num_heads, kv_seq_shift, _stream()))
    return out


def attention_split_ragged(qs, ks, vs, num_heads, seq_off, seq_len, max_len, kv_seq_shift=0, zero_key=True, causal=False, split_out=False, out=None):
    """attention_split over a ragged batch (mmdm_attention_split_ragged): qs / ks / vs [2, rows, H*dh] torch.float16 planes (may be column slices of a
    packed projection), sequence s = rows [seq_off[s], seq_off[s] + seq_len[s]) (int32 device tensors).  Returns fp32 [rows, H*dh] or its planes
    [2, rows, H*dh]; rows outside every sequence are left as they are in `out` (a new tensor: uninitialised)."""
    _chk(seq_off, seq_len)
    for t in (qs, ks, vs):
        assert t.is_cuda and t.dtype == torch.float16 and t.dim() == 3 and t.shape[0] == 2 and t.stride(2) == 1
    assert seq_off.dtype == torch.int32 and seq_len.dtype == torch.int32 and seq_off.numel() == seq_len.numel()
    _, rows, HD = qs.shape
    if out is None:
        out = torch.empty((2, rows, HD) if split_out else (rows, HD), device=qs.device, dtype=torch.float16 if split_out else torch.float32)
    flags = (0 if zero_key else ATTN_NO_ZERO_KEY) | (ATTN_CAUSAL if causal else 0)
    check(load_library().mmdm_attention_split_ragged(C.c_void_p(qs.data_ptr()), qs.stride(1), qs.stride(0), C.c_void_p(ks.data_ptr()), ks.stride(1), ks.stride(0),
                                                     C.c_void_p(vs.data_ptr()), vs.stride(1), vs.stride(0), C.c_void_p(out.data_ptr()), HD, 2 if split_out else 0, flags,
                                                     seq_off.numel(), _p(seq_off), _p(seq_len), int(max_len), rows, num_heads, HD // num_heads, kv_seq_shift, _stream()))
    return out


def quantize_rows_fp8(x):
    """Row-wise OCP e4m3 quantisation of an fp32 [rows, K] tensor: returns (q uint8-viewed-as torch.float8_e4m3fn [rows, K], scale fp32 [rows])
    with x ~= q.float() * scale[:, None].  Per-output-channel weight quantisation is this on W [N, K]."""
    _chk(x)
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    rows, K = x2.shape
    q = torch.empty(rows, K, device=x.device, dtype=torch.uint8)
    scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(load_library().mmdm_quantize_rows_fp8(_p(x2), x2.stride(0), C.c_void_p(q.data_ptr()), q.stride(0), _p(scale), rows, K, _stream()))
    return q.view(torch.float8_e4m3fn), scale


def linear_fp8(xq, x_scale, wq, w_scale, bias=None, epilogue="bias", extra=None, period=0, out_dtype=torch.float32, packed=False):
    """y = (xq * x_scale[:, None]) @ (wq * w_scale[:, None]).T + bias on the fp8 matrix instructions (fp32 accumulation, de-quantised in the
    epilogue).  xq [M, K], wq [N, K] torch.float8_e4m3fn; x_scale [M] / w_scale [N] fp32 or None; out fp32, bf16 or float8_e4m3fn (unit scale)."""
    for t in (xq, wq):
        if not t.is_cuda or t.dtype != torch.float8_e4m3fn:
            raise TypeError("linear_fp8 expects CUDA torch.float8_e4m3fn operands")
    _chk(bias, extra, x_scale, w_scale)
    K, N = xq.shape[-1], wq.shape[0]
    x2 = xq.reshape(-1, K)
    M = x2.shape[0]
    out = torch.empty(M, N, device=xq.device, dtype=out_dtype)
    mode = {torch.float32: 0, torch.bfloat16: 1, torch.float8_e4m3fn: 2}[out_dtype]
    if packed:          # wq from pack_weight_frag
        check(load_library().mmdm_linear_fp8_packed(C.c_void_p(x2.data_ptr()), x2.stride(0), _p(x_scale), C.c_void_p(wq.data_ptr()), _p(w_scale), _p(bias),
                                                    C.c_void_p(out.data_ptr()), out.stride(0), mode, M, N, K, EPI[epilogue],
                                                    _p(extra), extra.stride(0) if extra is not None else 0, period, _stream()))
        return out.reshape(*xq.shape[:-1], N)
    check(load_library().mmdm_linear_fp8(C.c_void_p(x2.data_ptr()), x2.stride(0), _p(x_scale), C.c_void_p(wq.data_ptr()), wq.stride(0), _p(w_scale), _p(bias),
                                         C.c_void_p(out.data_ptr()), out.stride(0), mode, M, N, K, EPI[epilogue],
                                         _p(extra), extra.stride(0) if extra is not None else 0, period, _stream()))
    return out.reshape(*xq.shape[:-1], N)


def adaln_fp8(h, ss, ss_rows=None, build=0):
    """AdaLN apply with an fp8 result: (q float8_e4m3fn [nseq, T, D], row_scale fp32 [nseq*T]).  build as in `adaln`."""
    if build:
        return adaln(h, ss, ss_rows, build=build, out="fp8")
    _chk(h, ss)
    nseq, T, D = h.shape
    h = h.contiguous()
    q = torch.empty(nseq, T, D, device=h.device, dtype=torch.uint8)
    scale = torch.empty(nseq * T, device=h.device, dtype=torch.float32)
    check(load_library().mmdm_adaln_fp8(_p(h), _p(ss), ss.stride(0), ss_rows or ss.shape[0], C.c_void_p(q.data_ptr()), _p(scale), nseq, T, D, _stream()))
    return q.view(torch.float8_e4m3fn), scale

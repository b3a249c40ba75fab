"""Inputs, float64 references and tolerance rules of the row-kernel tests (tests/test_gpu_rowops.py, tests/test_rowop_cases_cpu.py).

The row kernels (mixermdm_amd/csrc/rowops.hip: AdaLN, LayerNorm, cond SiLU, time mean, MDM pack / unpack, Influence head) exist in two builds; both are
held to the references below.  Everything here is plain torch on the CPU -- nothing touches the library under test -- and the CPU test proves the
references, the tolerance and the inputs before a GPU is involved: fp32 emulations of the kernels' two-pass algorithm stay inside the bound, and a list
of deliberately wrong float64 variants (MUTANTS_*) falls outside it.

Lane geometry of the normalising kernels: one 64-lane wave per row, lane L loads the float4 slots L, L + 64, ..., so element 4 j + e belongs to lane
j % 64.  A wave reduction that loses lanes loses those elements.
"""
import math
import torch

F64 = torch.float64
U23 = 2.0 ** -23
ADALN_EPS = 1e-6
# every |x| of a normalising case stays below this (the fp16 planes need |y| < 65504; LN_BIG_ROW comes closest)
INPUT_BOUND = 6.0e4

# shapes of tests/test_gpu_rowops.py: the MAXV = 1 / 2 / 4 / 8 instantiations end at D = 256 / 512 / 1024 / 2048; 252, 260, 516, 1028 leave the last
# 64-slot round partly empty; D = 4 is one active lane
NORM_DIMS = (4, 16, 252, 256, 260, 512, 516, 1024, 1028, 2048)
# (nseq, T): 1 row, 5 rows (one workgroup of four wave slots and a partial one), 85 rows, and the AdaLN shape of the issue
NORM_ROWS = ((1, 1), (5, 1), (5, 7), (5, 17))
SS_ROWS = 3
# the persistent row walk: the grid is capped at 2048 blocks of four wave slots, so from row 8192 on a wave slot takes a second row
WALK_CASE = dict(nseq=7, T=1171, D=64)            # 8197 rows: wave slots 0 .. 4 walk on
RAG_LENS = (3, 1, 7, 2)
RAG_PAD = 3
FP8_LANES = (0, 1, 2, 4, 8, 15, 16, 31, 32, 47, 48, 63)       # every quad, half row, 16-lane row and 32-lane half


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rnd(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed))


# ---------------------------------------------------------------------------------------------------
# inputs of the normalising kernels
# ---------------------------------------------------------------------------------------------------
def lane_element(lane, D, k=0):
    """An element of a D-wide row that lane `lane` owns (the k-th choice cycles through the lane's float4 slots and the four elements of a slot);
    for D < 256 the lanes beyond D / 4 own nothing and the lane is folded onto the active ones."""
    nv = D // 4
    slots = [j for j in range(lane % min(nv, 64), nv, 64)]
    j = slots[(k // 4 + 1) % len(slots)]
    return 4 * j + k % 4


def lane_of(element):
    return (element // 4) % 64


def norm_rows(rows, D, seed=0):
    """[rows, D] fp32: N(0.5, 3) rows, and from 5 rows on the edge rows -- 0: all zeros, 1: the constant 3.25 (13 / 4: every partial
    sum of up to 2048 copies is exact in fp32, so in ANY summation order the mean is exact and the output is exactly the shift; with an inexact constant
    the row measures the bias of the summation order -- 142 units of the bound below for a sequential sum at D = 2048 -- and not the kernel), 2: 1000 + N(0, 1), 3: 1e-3 N(0, 1) (variance
    comparable to both eps), 4: |x| near 6e4 with random signs; from 35 rows on one-hot rows whose hot element belongs to each lane of FP8_LANES, from
    85 rows on to each of the 64 lanes in turn.  Returns (x, hot) with hot = {row: element}."""
    x = rnd(seed, rows, D) * 3 + 0.5
    hot = {}
    if rows >= 5:
        x[0] = 0.0
        x[1] = 3.25
        x[2] = 1000.0 + rnd(seed + 1, D)
        x[3] = 1e-3 * rnd(seed + 2, D)
        x[4] = (5.9e4 + 1.0e3 * torch.rand(D, generator=_gen(seed + 3))) * torch.sign(rnd(seed + 4, D))
    lanes = tuple(range(64)) if rows >= 85 else (FP8_LANES if rows >= 35 else ())
    for i, lane in enumerate(lanes):
        r = 5 + i
        x[r] = 0.0
        hot[r] = lane_element(lane, D, i)
        x[r, hot[r]] = 1.0
    assert x.abs().max().item() <= INPUT_BOUND
    return x.contiguous(), hot


def adaln_case(nseq, T, D, seed=0, wide=False):
    """h [nseq, T, D], ss: nseq rows of (scale | shift) although only SS_ROWS are addressed (sequence s reads row s % SS_ROWS: a lookup without the
    modulo reads rows that exist and differ).  With more than one sequence ss row 0 is all zeros, and row 0 of h -- a row of sequence 0 -- is the
    all-zero row where there is one: y = 0 there, the fp8 form has amax = 0.  wide: ss is a column slice of a wider tensor (ss_ld > 2 D)."""
    h, hot = norm_rows(nseq * T, D, seed)
    store = rnd(seed + 10, nseq, 4 * D + 8)
    ss = store[:, D + 4:3 * D + 4] if wide else store[:, :2 * D].contiguous()
    if nseq > 1:
        ss[0] = 0.0
    return h.view(nseq, T, D), ss, hot


def on_device(t, device):
    """t on `device` with its strides kept (a column slice stays a column slice of a wider allocation)."""
    if t.is_contiguous():
        return t.to(device)
    out = torch.empty_strided(t.shape, t.stride(), device=device, dtype=t.dtype)
    out.copy_(t)
    return out


def fp8_lane_case(D, seed=0):
    """AdaLN input whose |y| maximum of sequence j sits in lane FP8_LANES[j]: nseq = ss_rows = 12, T = 2, and the shift of sequence j is 50 at one
    element of that lane (|LN(h) (1 + scale)| stays below ~25 for N(0, 1) rows at these D)."""
    n = len(FP8_LANES)
    h = rnd(seed, n, 2, D)
    ss = rnd(seed + 1, n, 2 * D) * 0.3
    where = []
    for j, lane in enumerate(FP8_LANES):
        e = lane_element(lane, D, j)
        ss[j, D + e] = 50.0 if j % 2 else -50.0
        where.append(e)
    return h, ss, where


def rag_row_seq(lens=RAG_LENS, pad=RAG_PAD):
    """row_seq of a ragged group: every row's sequence, the trailing padding rows mapped to sequence 0 (as the handle's maps do)."""
    return torch.tensor([s for s, n in enumerate(lens) for _ in range(n)] + [0] * pad, dtype=torch.int32)


def ln_case(rows, D, seed=0):
    """LayerNorm input with affine parameters; gamma[3] is sized so that the one-hot row with its hot element at 3 (LN_BIG_ROW, from 5 rows on) comes
    out near 6e4 -- the rows tests/test_gpu_mdm_split.py defines."""
    x, hot = norm_rows(rows, D, seed)
    g, b = rnd(seed + 20, D), rnd(seed + 21, D)
    if rows >= 5 and D >= 16:
        g[3], b[3] = 6.0e4 / math.sqrt(D - 1), 0.0
        x[1] = 0.0
        x[1, 3] = 1.0           # (replaces the constant row; AdaLN keeps it)
    return x, g, b


# ---------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------
def ref_normalise(x, eps):
    """(x - mean) / sqrt(var + eps) with the BIASED variance, float64.  Returns (n, rstd [rows, 1])."""
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd, rstd


def ref_layernorm(x, gamma, beta, eps):
    """nn.LayerNorm with affine (float64)."""
    n, _ = ref_normalise(x, eps)
    return n * gamma.to(F64) + beta.to(F64)


def adaln_rows(rows, T, ss_rows, row_seq=None):
    """ss row of every h row: sequence = row // T (or row_seq[row]), ss row = sequence % ss_rows."""
    seq = torch.arange(rows) // T if row_seq is None else row_seq.long()
    return seq % ss_rows


def ref_adaln(h, ss, T, ss_rows, row_seq=None, eps=ADALN_EPS):
    """AdaLN.forward: LN_{eps, no affine}(h) * (1 + scale) + shift on h [rows, D], ss [., >= 2 D] = (scale | shift); float64 [rows, D]."""
    rows, D = h.shape
    n, _ = ref_normalise(h, eps)
    r = adaln_rows(rows, T, ss_rows, row_seq)
    s = ss.to(F64)
    return n * (1.0 + s[r, :D]) + s[r, D:2 * D]


def ref_silu(x):
    x = x.to(F64)
    return x / (1.0 + torch.exp(-x))


def ref_mean_time(h):
    return h.to(F64).mean(dim=-2)


def split_f16(x):
    """The two fp16 planes of an fp32 tensor: h = fp16(x), l = fp16((x - h) * 2048), both round to nearest even (x - h and the product are exact in
    fp32).  [2, *x.shape] float16."""
    x = x.float()
    h = x.to(torch.float16)
    l = ((x - h.float()) * 2048.0).to(torch.float16)
    return torch.stack([h, l])


def e4m3_rne(v):
    """OCP e4m3 (fn) round to nearest even of float64 values, saturating at +-448; returns the quantised VALUES (float64).  Steps: 2^-9 below 2^-6
    (subnormals), 2^(e - 3) in [2^e, 2^(e + 1))."""
    v = v.to(F64).clamp(-448.0, 448.0)
    a = v.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=-6.0, max=8.0)
    step = torch.pow(torch.full_like(a, 2.0), e - 3.0)
    q = torch.round(a / step) * step           # torch.round: half to even
    return torch.sign(v) * q.clamp(max=448.0)


def e4m3_index(values):
    """Position of an e4m3 value on the format's ladder (..., -2^-9 -> -1, 0 -> 0, 2^-9 -> 1, ...): two values one step apart differ by 1."""
    a = values.to(F64).abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=-6.0)
    idx = torch.where(a < 2.0 ** -6, a * 2.0 ** 9, (e + 7.0) * 8.0 + (a / torch.pow(torch.full_like(a, 2.0), e) - 1.0) * 8.0)
    return (torch.sign(values.to(F64)) * idx).round().long()


def byte_index(b):
    """The same ladder position from e4m3 BYTES (uint8 tensor): sign-magnitude, magnitudes in value order."""
    b = b.long()
    return torch.where(b >= 128, -(b - 128), b)


def ref_quant_rows(y):
    """Row-wise e4m3 quantisation in float64: scale = max|y| / 448 (1 for an all-zero row), q = e4m3(y / scale).  Returns (values, scale)."""
    y = y.to(F64)
    amax = y.abs().amax(-1, keepdim=True)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return e4m3_rne(y / scale), scale[:, 0]


def fp8_scale_f32(y32, lanes=None):
    """The row scale in the kernels' fp32 form, bit for bit: max|y| * fp32(1 / 448), 1 for a zero row (max and a single fp32 product: no rounding
    freedom).  lanes: the maximum taken over those lanes' elements only (the mutation check)."""
    a = y32.float().abs()
    if lanes is not None:
        keep = torch.tensor([lane_of(e) in lanes for e in range(a.shape[-1])])
        a = a[:, keep]
    amax = a.amax(-1)
    return torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))


def quant_rows_f32(y32):
    """The kernels' quantiser emulated in fp32: scl as fp8_scale_f32, inv = 1 / scl, e4m3(y * inv).  Returns (values float64, scale fp32)."""
    y32 = y32.float()
    scl = fp8_scale_f32(y32)
    inv = torch.tensor(1.0, dtype=torch.float32) / scl
    return e4m3_rne((y32 * inv[:, None]).to(F64)), scl


# ---------------------------------------------------------------------------------------------------
# tolerance of the fp32 outputs of the normalising kernels
# ---------------------------------------------------------------------------------------------------
NORM_A, NORM_R = 2e-5, 2e-5            # tests/test_gpu_kernels.py::test_adaln
# C: |LN_fp32(x) - LN_f64(x)| <= NORM_A + C 2^-23 max|x_row| rstd_ref.  The fp32 mean carries roundings of size 2^-24 max|x| and every x - mean
# inherits that absolute error times rstd -- invisible on N(0, 1) rows, 6e-5 rstd on a row with mean 1000; on a one-hot row the sum of squares adds
# ~D terms of 1 / D^2 to a partial sum near 1.  Measured by tests/test_rowop_cases_cpu.py::test_emulations_stay_inside_the_bound (the two-pass
# algorithm in torch fp32, summed sequentially and as 64 lane partials + a butterfly, over every case of NORM_DIMS x NORM_ROWS, AdaLN and LayerNorm):
# the worst ratio (|error| - NORM_A gain - NORM_R |ref|) / (2^-23 max|x| rstd_ref gain) is 6.6 (LayerNorm, sequential order, a one-hot row at
# D = 1028; the row with mean 1000 needs 4.0 in sequential order; the lane-partial order never needs more than 0.6); x 4 for another reduction order
# and fma contraction, rounded up.
NORM_C_MEASURED = 6.6
NORM_C = 27.0


def norm_bound(x, ref, gain, eps):
    """Per-element bound of an fp32 normalising kernel against its float64 reference `ref`: (a + c 2^-23 max|x_row| rstd_ref) gain + r |ref|, with
    gain = 1 + |scale| (AdaLN) or |gamma| (LayerNorm: the factor the normalised value is multiplied by)."""
    _, rstd = ref_normalise(x, eps)
    xmax = x.to(F64).abs().amax(-1, keepdim=True)
    return (NORM_A + NORM_C * U23 * xmax * rstd) * gain.to(F64) + NORM_R * ref.abs()


def adaln_gain(ss, rows, D, T, ss_rows, row_seq=None):
    return 1.0 + ss.to(F64)[adaln_rows(rows, T, ss_rows, row_seq), :D].abs()


def bf16_half_ulp(ref, bound):
    """Half a bf16 ulp (8 significant bits) at the largest magnitude the fp32 value may have: 2^(floor(log2(|ref| + bound)) - 8)."""
    m = (ref.abs() + bound).clamp(min=2.0 ** -126)
    return torch.pow(torch.full_like(m, 2.0), torch.floor(torch.log2(m)) - 8.0)


def planes_bound(y):
    """|h + l / 2048 - y| for the split of an fp32 value (tests/test_gpu_mdm_split.py)."""
    return 2.0 ** -21 * y.to(F64).abs() + 2.0 ** -35


def mean_time_bound(h, ref):
    """Sequential fp32 summation of T terms: (T - 1) roundings of at most 2^-24 sum|x|, divided by T, plus the division's own rounding."""
    T = h.shape[-2]
    return T * 2.0 ** -24 * h.to(F64).abs().mean(dim=-2) + 1e-7 * ref.abs()


# ---------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' two-pass algorithm (what fp32 arithmetic delivers, independent of any kernel)
# ---------------------------------------------------------------------------------------------------
def _sum_sequential(v):
    s = torch.zeros(v.shape[0], dtype=torch.float32)
    for j in range(v.shape[1]):
        s = s + v[:, j]
    return s


def _sum_lanes(v):
    """64 lane partials (lane L adds the four elements of its slots L, L + 64, ... in order), then a butterfly over the lanes."""
    rows, D = v.shape
    nv = D // 4
    part = torch.zeros(rows, 64, dtype=torch.float32)
    for i in range((nv + 63) // 64):
        blk = torch.zeros(rows, 64, 4, dtype=torch.float32)
        n = min(64, nv - 64 * i)
        blk[:, :n] = v[:, 256 * i:256 * i + 4 * n].reshape(rows, n, 4)
        part = part + (((blk[..., 0] + blk[..., 1]) + blk[..., 2]) + blk[..., 3])
    o = 32
    while o:
        part = part + part[:, torch.arange(64) ^ o]
        o >>= 1
    return part[:, 0]


SUM_ORDERS = {"sequential": _sum_sequential, "lanes": _sum_lanes}


def emulate_normalise_f32(x, eps, order):
    """mean = sum / D; q = sum (x - mean)^2; rstd = 1 / sqrt(q / D + eps); (x - mean) * rstd -- every operation rounded to fp32."""
    x = x.float()
    D = x.shape[1]
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    mean = SUM_ORDERS[order](x) / f(float(D))
    d = x - mean[:, None]
    var = SUM_ORDERS[order](d * d) / f(float(D))
    rstd = f(1.0) / torch.sqrt(var + f(eps))
    return d * rstd[:, None]


def emulate_adaln_f32(h, ss, T, ss_rows, order, row_seq=None):
    rows, D = h.shape
    r = adaln_rows(rows, T, ss_rows, row_seq)
    s = ss.float()
    return emulate_normalise_f32(h, ADALN_EPS, order) * (1.0 + s[r, :D]) + s[r, D:2 * D]


def emulate_layernorm_f32(x, g, b, eps, order):
    return emulate_normalise_f32(x, eps, order) * g.float() + b.float()


# ---------------------------------------------------------------------------------------------------
# deliberately wrong float64 variants: each must leave the tolerance on at least one case
# ---------------------------------------------------------------------------------------------------
def _drop_mask(D, lanes):
    return torch.tensor([lane_of(e) not in lanes for e in range(D)])


def _normalise_dropping(x, eps, lanes, unbiased=False):
    """Both wave sums (mean and variance) lose the elements of `lanes`."""
    x = x.to(F64)
    D = x.shape[1]
    keep = _drop_mask(D, lanes).to(F64)
    mean = (x * keep).sum(-1, keepdim=True) / D
    var = (((x - mean) ** 2) * keep).sum(-1, keepdim=True) / (D - 1 if unbiased else D)
    return (x - mean) / torch.sqrt(var + eps)


DROPS = {"lane_5": {5}, "lane_21": {21}, "lane_38": {38}, "lane_63": {63},                         # a lane in each 16-lane row
         "row16_0": set(range(0, 16)), "row16_2": set(range(32, 48)), "half32_0": set(range(0, 32)), "half32_1": set(range(32, 64))}


def adaln_mutants():
    """name -> f(h [rows, D], ss, T, ss_rows, row_seq, nseq) -> float64 [rows, D]."""
    def with_norm(norm):
        def f(h, ss, T, ss_rows, row_seq, nseq):
            D = h.shape[1]
            r = adaln_rows(h.shape[0], T, ss_rows, row_seq)
            s = ss.to(F64)
            return norm(h) * (1.0 + s[r, :D]) + s[r, D:2 * D]
        return f

    def with_affine(aff, rows_of=None):
        def f(h, ss, T, ss_rows, row_seq, nseq):
            D = h.shape[1]
            r = adaln_rows(h.shape[0], T, ss_rows, row_seq) if rows_of is None else rows_of(h.shape[0], T, ss_rows, row_seq, nseq)
            n, _ = ref_normalise(h, ADALN_EPS)
            return aff(n, ss.to(F64)[r], D)
        return f
    M = {"drop_" + k: with_norm(lambda h, L=L: _normalise_dropping(h, ADALN_EPS, L)) for k, L in DROPS.items()}
    M["unbiased_variance"] = with_norm(lambda h: _normalise_dropping(h, ADALN_EPS, set(), unbiased=True))
    M["eps_1e-5"] = with_norm(lambda h: ref_normalise(h, 1e-5)[0])
    M["scale_without_one"] = with_affine(lambda n, s, D: n * s[:, :D] + s[:, D:2 * D])
    M["halves_swapped"] = with_affine(lambda n, s, D: n * (1.0 + s[:, D:2 * D]) + s[:, :D])
    M["seq_is_row_mod_nseq"] = with_affine(lambda n, s, D: n * (1.0 + s[:, :D]) + s[:, D:2 * D],
                                           lambda rows, T, ss_rows, row_seq, nseq: (torch.arange(rows) % nseq) % ss_rows)
    M["ss_row_without_modulo"] = with_affine(lambda n, s, D: n * (1.0 + s[:, :D]) + s[:, D:2 * D],
                                             lambda rows, T, ss_rows, row_seq, nseq: torch.arange(rows) // T if row_seq is None else row_seq.long())
    return M


def layernorm_mutants():
    """name -> f(x, gamma, beta, eps) -> float64."""
    M = {"drop_" + k: (lambda x, g, b, eps, L=L: _normalise_dropping(x, eps, L) * g.to(F64) + b.to(F64)) for k, L in DROPS.items()}
    M["unbiased_variance"] = lambda x, g, b, eps: _normalise_dropping(x, eps, set(), unbiased=True) * g.to(F64) + b.to(F64)
    M["eps_1e-6"] = lambda x, g, b, eps: ref_layernorm(x, g, b, 1e-6)
    return M


# ---------------------------------------------------------------------------------------------------
# MDM pack / unpack: the index maps, written from the definitions in kernels.h / rowops.hip
# ---------------------------------------------------------------------------------------------------
def rag_maps(lens, rows):
    """One row space of a ragged batch (kernels.h mmdm_rag): the items back to back in `rows` rows.  row_item [rows] (-1 = padding), row_pos [rows]
    (index inside the item, 0 on padding rows), item_off [B], item_len [B]; int32."""
    assert sum(lens) <= rows
    row_item = torch.full((rows,), -1, dtype=torch.int32)
    row_pos = torch.zeros(rows, dtype=torch.int32)
    item_off = torch.zeros(len(lens), dtype=torch.int32)
    a = 0
    for b, n in enumerate(lens):
        item_off[b] = a
        row_item[a:a + n] = b
        row_pos[a:a + n] = torch.arange(n, dtype=torch.int32)
        a += n
    return row_item, row_pos, item_off, torch.tensor(lens, dtype=torch.int32)


def token_maps(lens, rows):
    """The token space: every item's conditioning token in front of its frames (lengths + 1; row_pos 0 = the token, k >= 1 = frame k - 1)."""
    return rag_maps([n + 1 for n in lens], rows)


def ref_mdm_pack(src, cond_store, ldc, col0, time_tab, step, pe, cond_ld=None, use_col0=True):
    """dst [nseq, T + 1, D] fp32: dst[s, 0] = (cond[s] + time_tab[step]) + pe[0] with cond[s] = cond_store.flatten()[s * ldc + col0 : + D],
    dst[s, 1 + t] = src[s, t].  fp32 additions in the documented order: exact equality is expected of the kernel.
    cond_ld / use_col0: the mutation check (another stride; no column offset)."""
    nseq, T, D = src.shape
    flat = cond_store.float().reshape(-1)
    ld = ldc if cond_ld is None else cond_ld
    c0 = col0 if use_col0 else 0
    dst = torch.empty(nseq, T + 1, D, dtype=torch.float32)
    for s in range(nseq):
        dst[s, 0] = (flat[s * ld + c0:s * ld + c0 + D] + time_tab[step].float()) + pe[0].float()
    dst[:, 1:] = src.float()
    return dst


def ref_mdm_unpack(src):
    return src[:, 1:].clone()


def ref_mdm_pack_rag(src, cond_store, ldc, time_tab, step, pe, gpp, fr, tk, tk_rows, cond_ld=None, use_col0=True):
    """dst [groups, tk_rows, D]: padding token rows 0; the token of item i in group g = (cond[(g % gpp) B + i, (g // gpp) D : + D] + time_tab[step]) +
    pe[0]; token row (i, pos >= 1) = src[g, fr.item_off[i] + pos - 1]."""
    groups, fr_rows, D = src.shape
    tk_item, tk_pos, _, _ = tk
    fr_off = fr[2]
    B = fr_off.numel()
    flat = cond_store.float().reshape(-1)
    ld = ldc if cond_ld is None else cond_ld
    dst = torch.zeros(groups, tk_rows, D, dtype=torch.float32)
    for g in range(groups):
        for r in range(tk_rows):
            i, pos = int(tk_item[r]), int(tk_pos[r])
            if i < 0:
                continue
            if pos == 0:
                o = ((g % gpp) * B + i) * ld + ((g // gpp) * D if use_col0 else 0)
                dst[g, r] = (flat[o:o + D] + time_tab[step].float()) + pe[0].float()
            else:
                dst[g, r] = src[g, int(fr_off[i]) + pos - 1]
    return dst


def ref_mdm_unpack_rag(src, fr, tk, fr_rows, skip=1):
    """dst [groups, fr_rows, D]: frame row (i, pos) = src[g, tk.item_off[i] + skip + pos] (skip = 1: past the item's token); padding rows 0."""
    groups, _, D = src.shape
    fr_item, fr_pos, _, _ = fr
    tk_off = tk[2]
    dst = torch.zeros(groups, fr_rows, D, dtype=torch.float32)
    for r in range(fr_rows):
        i = int(fr_item[r])
        if i >= 0:
            dst[:, r] = src[:, int(tk_off[i]) + skip + int(fr_pos[r])]
    return dst


PACK_RAG = dict(lens=(1, 16, 5), fr_rows=32, tk_rows=40, groups=4, gpp=2)


def pack_case(nseq, T, D, seed=0):
    """Uniform pack inputs: cond is the SECOND person's D columns of a [nseq, 2 D + 4] store (ldc > D, column offset D), step index 2 of 4."""
    return dict(src=rnd(seed, nseq, T, D), cond_store=rnd(seed + 1, nseq, 2 * D + 4), ldc=2 * D + 4, col0=D, time_tab=rnd(seed + 2, 4, D), step=2,
                pe=rnd(seed + 3, 3, D))


def pack_rag_case(D, seed=0):
    c = dict(PACK_RAG)
    B = len(c["lens"])
    c.update(src=rnd(seed, c["groups"], c["fr_rows"], D), cond_store=rnd(seed + 1, c["gpp"] * B, 2 * D + 4), ldc=2 * D + 4, time_tab=rnd(seed + 2, 4, D),
             step=3, pe=rnd(seed + 3, 3, D), fr=rag_maps(c["lens"], c["fr_rows"]), tk=token_maps(c["lens"], c["tk_rows"]))
    return c


# ---------------------------------------------------------------------------------------------------
# Influence head: weight rows with one dominant element per lane (element c of a row belongs to lane c % 64 in this kernel)
# ---------------------------------------------------------------------------------------------------
def head_case(rows, D, nw, seed=0):
    h, w, b = rnd(seed, rows, D), rnd(seed + 1, nw, D) * 0.05, rnd(seed + 2, nw)
    lanes = (FP8_LANES + tuple(l for l in range(64) if l not in FP8_LANES))[:nw]
    for o, lane in enumerate(lanes):
        c = lane + 64 * (o % (D // 64))
        w[o, c] += 3.0
    return h, w, b, lanes

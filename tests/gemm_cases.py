"""Inputs, layouts and the reference of the low-precision GEMM edge tests (tests/test_gpu_gemm_edges.py, tests/test_gemm_cases_cpu.py).

ref_linear_f64 is the one float64 statement of what mmdm_linear_split / _bf16 / _fp8 (and their _packed entry points) compute.

LATTICE OPERANDS.  x and w entries are k / 4, bias / residual / PE entries k / 8, integer |k| <= 8 (seeded, uniform: one entry in 17 is 0).
Every such value is exact in bf16, in fp16 (the lo plane of the split format is exactly 0) and in e4m3 (four significant bits at most), every
product is a multiple of 1/16 with |product| <= 4, and so every partial sum of a row's K products, IN ANY ORDER, is an integer number of
1/16 units of magnitude <= 64 K.  The fp8 kernels de-quantise with a_scale[m] * w_scale[n]; the scales used here are powers of two 2^-s,
s >= 0, so the de-quantised sum is an integer number of 2^-(4 + s) units, and bias + residual / PE (|.| <= 2, multiples of 1/8) add at most
32 * 2^s of those.  lattice_units(K, s) = 64 K + 32 * 2^s is therefore a bound on |every intermediate| / unit, and while it stays below
2^24 every intermediate is exact in fp32 whatever the order of the additions: the bias, resid and pe results of a correct kernel equal the
float64 reference BIT FOR BIT.  K <= 2048, s <= 8 gives 2^17 + 2^13.  LatticeCase asserts the bound for itself.

Pure torch on the CPU: nothing here touches the library under test.
"""
import functools
import math
import torch

EPI = {"bias": 0, "gelu": 1, "resid": 2, "pe": 3, "silu": 4}
LATTICE_MAX_K = 8                      # |k| of a lattice entry
EXACT_LIMIT = 1 << 24                  # integers below this magnitude are exact in fp32
FORMS = ("split", "split_packed", "bf16", "bf16_packed", "fp8", "fp8_packed")
GUARD = 4                              # NaN rows above and below the output window: the buffer is [M + 8, ldc]


def lattice(shape, denom, seed):
    """Seeded fp32 tensor of k / denom, integer k uniform in [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-LATTICE_MAX_K, LATTICE_MAX_K + 1, shape, generator=g).float() / denom


def pow2_scales(n, seed, exps):
    """Seeded fp32 [n] of 2^-e, e drawn from `exps`."""
    g = torch.Generator().manual_seed(seed)
    e = torch.tensor(exps)[torch.randint(0, len(exps), (n,), generator=g)]
    return torch.ldexp(torch.ones(n), -e)


def lattice_units(K, s=0):
    """Bound on |any intermediate of a lattice case| in units of 2^-(4 + s) (module docstring)."""
    return 64 * K + 32 * (1 << s)


# ---------------------------------------------------------------------------------------------------------------------------------------
# reference and output encoders
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref_linear_f64(x, w, bias, epi, extra=None, period=0, row0=0):
    """float64 epi(x w^T + bias [+ extra]).  x [M, K], w [N, K], bias [N] or None (any float dtype, used at their values).
    resid: + extra[m]; pe: + extra[(row0 + m) % period] (row0: global index of x's row 0, for a row slice of a larger call)."""
    y = x.double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if epi == "resid":
        y = y + extra.double()
    elif epi == "pe":
        assert period > 0
        y = y + extra.double()[(row0 + torch.arange(x.shape[0])) % period]
    elif epi == "gelu":
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    elif epi == "silu":
        y = y / (1.0 + torch.exp(-y))
    else:
        assert epi == "bias", epi
    return y


def enc_bf16(t):
    """fp32 -> bf16, round to nearest even."""
    return t.float().bfloat16()


def enc_e4m3(t):
    """fp32 -> OCP e4m3 at unit scale, saturating at +-448, round to nearest even."""
    return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def enc_split(t):
    """fp32 -> the two fp16 planes of the split format: h = fp16(x), l = fp16((x - h) * 2048).  Returns [2, *t.shape] float16."""
    t = t.float()
    h = t.half()
    return torch.stack([h, ((t - h.float()) * 2048.0).half()])


def received(form, t):
    """float64 values of an fp32 CPU operand as the kernels of `form` receive it."""
    if form.startswith("split"):
        p = enc_split(t)
        return p[0].double() + p[1].double() / 2048.0
    if form.startswith("bf16"):
        return enc_bf16(t).double()
    return t.float().to(torch.float8_e4m3fn).double()            # operands never exceed 448 here: no clamp involved


def bits(t):
    """Integer view of a tensor's bytes, for bit-exact comparison (NaN-safe)."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One GEMM problem on the CPU: x [M, K], w [N, K], bias [N] or None, extra ([M, N] residual or [period, N] PE table) or None,
    a_scale [M] / w_scale [N] or None (fp8 forms only; None = 1).  `split_at`: row at which the split plane kernel's hybrid launch cuts."""
    def __init__(self, kind, M, N, K, epi, period=0, scales=(False, False), has_bias=True, split_at=0):
        self.kind, self.M, self.N, self.K, self.epi, self.period, self.split_at = kind, M, N, K, epi, period, split_at
        seed = ((M * 1315423911) ^ (N * 2654435761) ^ (K * 97) ^ (EPI[epi] * 7919) ^ (period * 31)) & 0x7fffffff
        if kind == "lattice":
            self.x, self.w = lattice((M, K), 4.0, seed), lattice((N, K), 4.0, seed + 1)
            self.bias = lattice((N,), 8.0, seed + 2) if has_bias else None
        else:
            g = torch.Generator().manual_seed(seed)
            self.x, self.w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
            self.bias = torch.randn(N, generator=g) if has_bias else None
        rows = {"resid": M, "pe": period}.get(epi, 0)
        self.extra = None
        if rows:
            self.extra = lattice((rows, N), 8.0, seed + 3) if kind == "lattice" else torch.randn(rows, N, generator=torch.Generator().manual_seed(seed + 3))
        self.a_exps, self.w_exps = (1, 2, 3), (0, 1, 2)
        self.a_scale = pow2_scales(M, seed + 4, self.a_exps) if scales[0] else None
        self.w_scale = pow2_scales(N, seed + 5, self.w_exps) if scales[1] else None
        self.s_max = (max(self.a_exps) if scales[0] else 0) + (max(self.w_exps) if scales[1] else 0)
        if kind == "lattice":
            assert lattice_units(K, self.s_max) < EXACT_LIMIT, (K, self.s_max)
        self._ref = {}

    def scaled(self, form="lattice"):
        """float64 (x, w) as the kernels of `form` see them, de-quantisation scales applied ("lattice": the values themselves)."""
        x = self.x.double() if form == "lattice" else received(form, self.x)
        w = self.w.double() if form == "lattice" else received(form, self.w)
        if self.a_scale is not None:
            x = x * self.a_scale.double()[:, None]
        if self.w_scale is not None:
            w = w * self.w_scale.double()[:, None]
        return x, w

    def ref(self, form="lattice"):
        """float64 reference (computed once per operand form, shared, never modified by the tests)."""
        key = "lattice" if self.kind == "lattice" else form.split("_")[0]
        if key not in self._ref:
            x, w = self.scaled(key)
            self._ref[key] = ref_linear_f64(x, w, self.bias, self.epi, self.extra, self.period)
        return self._ref[key]


@functools.lru_cache(maxsize=None)
def case(kind, M, N, K, epi, period=0, scales=(False, False), has_bias=True, split_at=0):
    return Case(kind, M, N, K, epi, period, scales, has_bias, split_at)


def saturating_case(N=128, M=33, K=256):
    """fp8 output saturation: row 1 of x and row 2 of w are all +2 (product sum 4 K = 1024 -> +448), row 3 of x is all -2 (-> -448 in column 2)."""
    c = Case("lattice", M, N, K, "bias", has_bias=False)
    c.x[1], c.x[3], c.w[2] = 2.0, -2.0, 2.0
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------
# operand layouts (shared by the CPU mutation tests and the GPU runner)
# ---------------------------------------------------------------------------------------------------------------------------------------
A_GARBAGE, EXTRA_GARBAGE = 5.0, 77.0          # finite, exact in every operand format


def layout(form, M, N, K, strided):
    """Element strides and offsets of one run.  q = elements per 16 bytes of an operand row (every operand row / plane must be 16-byte aligned)."""
    q = 16 if form.startswith("fp8") else 8
    if not strided:
        return dict(lda=K, a_c0=0, a_rows=M, ldw=K, w_c0=0, gap=0, ld_extra=N, e_c0=0, ldc=N, c_c0=0, c_gap=0)
    return dict(lda=K + 5 * q, a_c0=2 * q, a_rows=M + 3, ldw=K + 3 * q, w_c0=q, gap=64, ld_extra=N + 12, e_c0=4, ldc=N + 36, c_c0=16, c_gap=20)


def place(t, ld, c0, rows, fill):
    """[r, c] values -> a [rows, ld] buffer of `fill` with the values at columns [c0, c0 + c) of its first r rows."""
    buf = torch.full((rows, ld), fill, dtype=t.dtype)
    buf[:t.shape[0], c0:c0 + t.shape[1]] = t
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------------
# shape tables: every M at one (N, K), every N at one (M, K), every K at one (M, N), plus the corner (largest odd M, tail N, three K steps)
# ---------------------------------------------------------------------------------------------------------------------------------------
PLANE_N = (4, 60, 64, 68, 124, 128, 132, 260)      # 260 = two full 64-column tiles of <22,21> plus a 4-column tail; one 128-column tile + 4 for <42,22>
TABLE = {
    # form: BM of the tile it takes at these shapes, its M / N / K lists and the fixed pair of each sweep
    "split":        dict(BM=128, Ms=(1, 33, 127, 128, 129, 300), Ns=PLANE_N, Ks=(32, 64, 96, 2048), m_at=(132, 64), n_at=(129, 64), k_at=(129, 132), corner=(129, 260, 96)),
    "bf16":         dict(BM=256, Ms=(1, 33, 255, 256, 257, 300), Ns=PLANE_N, Ks=(32, 64, 96, 2048), m_at=(132, 64), n_at=(257, 64), k_at=(257, 132), corner=(257, 260, 96)),
    "fp8":          dict(BM=256, Ms=(1, 33, 255, 256, 257, 300), Ns=PLANE_N, Ks=(64, 128, 192, 2048), m_at=(132, 128), n_at=(257, 128), k_at=(257, 132), corner=(257, 260, 192)),
    # packed split: N = 128 takes gemm_splitw<12,41> (BM = 64), N & 127 takes gemm_splitw<22,21> (BM = 128: `Ms2` at N = 192)
    "split_packed": dict(BM=64, Ms=(1, 33, 63, 64, 65, 300), Ns=(64, 128, 192, 320), Ks=(64, 128, 192, 2048), m_at=(128, 64), n_at=(65, 64), k_at=(65, 128), corner=(65, 128, 192),
                         Ms2=(127, 128, 129), m2_at=(192, 64), corner2=(129, 320, 192)),
    "bf16_packed":  dict(BM=128, Ms=(1, 33, 127, 128, 129, 300), Ns=(128, 256, 384, 512), Ks=(128, 256, 384, 2048), m_at=(384, 128), n_at=(129, 128), k_at=(129, 384), corner=(129, 384, 384)),
    "fp8_packed":   dict(BM=128, Ms=(1, 33, 127, 128, 129, 300), Ns=(128, 256, 384, 512), Ks=(256, 512, 768, 2048), m_at=(384, 256), n_at=(129, 256), k_at=(129, 384), corner=(129, 384, 768)),
}
# shapes under a forced tile: (diag key, value, shapes)
FORCED = {
    "split_packed": ("split_cfg", 6, ((1, 128, 64), (129, 128, 128), (129, 256, 192))),          # gemm_splitw<14,41> (128 x 128)
    "bf16_packed":  ("bf16_cfg", 12, ((1, 256, 128), (129, 256, 256), (129, 512, 384))),         # gemm_bf16w<14,42>  (128 x 256)
    "fp8_packed":   ("bf16_cfg", 12, ((1, 256, 256), (129, 256, 512), (129, 512, 768))),         # gemm_fp8w<14,42>
}
SPLIT_BIG_TILE = ((1, 516, 32), (257, 516, 96))           # N > 512: gemm_split<42,22>, four full 128-column tiles and a 4-column tail
HYBRID = (8449, 1024, 64, 8192)                           # M, N, K, M1: mt = 34, nt = 8 -> 32 row tiles fill a round, 257 rows go to gemm_split<22,21>
HYBRID_PERIOD = 299                                       # 8192 % 299 = 119: the second launch's PE rows do not start at row 0 of the table
FEW_THRESHOLD = ((3968, 1024, 64), (3969, 1024, 64))      # ceil(M / 128) * (N / 128) = 248 | 256: gemm_splitw<12,41> | <14,41>
FP8P = ((8192, 1024, 1024), (8320, 1024, 1024))           # 512 tiles (one per workgroup) | 520 (not a multiple of the grid)
ACT_SHAPES = {"split": ((129, 320, 192), (33, 128, 2048)), "bf16": ((129, 384, 384), (33, 128, 2048)), "fp8": ((129, 384, 768), (33, 128, 2048))}


def sweeps(form):
    """[(sweep, M, N, K)]: sweep in "M", "N", "K", "corner"; no duplicates."""
    t, out, seen = TABLE[form], [], set()

    def add(sw, M, N, K):
        if (M, N, K) not in seen:
            seen.add((M, N, K))
            out.append((sw, M, N, K))
    add("corner", *t["corner"])
    if "corner2" in t:
        add("corner", *t["corner2"])
    for M in t["Ms"]:
        add("M", M, *t["m_at"])
    for M in t.get("Ms2", ()):
        add("M", M, *t["m2_at"])
    for N in t["Ns"]:
        add("N", t["n_at"][0], N, t["n_at"][1])
    for K in t["Ks"]:
        add("K", t["k_at"][0], t["k_at"][1], K)
    return out


# which exact epilogues a sweep's shapes run (resid and pe include the bias; "resid_inplace" is resid with R aliasing C)
SWEEP_EPIS = {"corner": ("bias", "resid", "resid_inplace", "pe"), "M": ("resid", "pe"), "N": ("resid_inplace", "pe"), "K": ("bias",)}
DEFAULT_PERIOD = 7


def pe_periods(M):
    return (5, 299, M + 3)            # below a 32-row tile, between, above M


def exact_cases(form):
    """[(M, N, K, epi_name, period, strided)] of the exact sweep of a form: strided layout everywhere, the contiguous one at the corner too."""
    out = []
    for sw, M, N, K in sweeps(form):
        for e in SWEEP_EPIS[sw]:
            for strided in ((True, False) if sw == "corner" else (True,)):
                out.append((M, N, K, e, DEFAULT_PERIOD if e == "pe" else 0, strided))
    return out


def lattice_case_of(form, M, N, K, epi_name, period=0, split_at=0):
    """The lattice Case behind an exact run (fp8 forms: with power-of-two scales on both sides)."""
    sc = (True, True) if form.startswith("fp8") else (False, False)
    return case("lattice", M, N, K, "resid" if epi_name == "resid_inplace" else epi_name, period, sc, True, split_at)


def all_lattice_cases():
    """Every lattice Case the GPU suite runs (for the CPU exactness and discrimination tests), without duplicates."""
    seen, out = set(), []

    def add(c):
        if id(c) not in seen:
            seen.add(id(c))
            out.append(c)
    for form in FORMS:
        for M, N, K, e, period, _ in exact_cases(form):
            add(lattice_case_of(form, M, N, K, e, period))
        bm = TABLE[form]["BM"]
        N, K = TABLE[form]["m_at"]
        for period in pe_periods(bm + 1):
            add(lattice_case_of(form, bm + 1, N, K, "pe", period))
        if form in FORCED:
            for M, N, K in FORCED[form][2]:
                for e in ("resid", "pe"):
                    add(lattice_case_of(form, M, N, K, e, DEFAULT_PERIOD if e == "pe" else 0))
    for M, N, K in SPLIT_BIG_TILE:
        for e in ("resid", "pe"):
            add(lattice_case_of("split", M, N, K, e, DEFAULT_PERIOD if e == "pe" else 0))
    M, N, K, M1 = HYBRID
    for e in ("bias", "resid", "pe"):
        add(lattice_case_of("split", M, N, K, e, HYBRID_PERIOD if e == "pe" else 0, M1))
    for M, N, K in FEW_THRESHOLD:
        add(lattice_case_of("split_packed", M, N, K, "resid"))
    for M, N, K in FP8P:
        add(lattice_case_of("fp8_packed", M, N, K, "bias"))
    return out

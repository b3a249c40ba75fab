"""GPU: the low-precision linear layers at their tile edges, through strided operands, on every epilogue path.

Forms (entry point -> kernels; csrc/gemm_split.hip, gemm_bf16.hip, gemm_fp8p.hip):
  split         mmdm_linear_split          gemm_split<22,21> (N <= 512), gemm_split<42,22>, and the hybrid <42,22>+<22,21> launch with row0
  split_packed  mmdm_linear_split_packed   gemm_splitw<22,21> (N & 127), gemm_splitw<12,41>, gemm_splitw<14,41>
  bf16 / fp8    mmdm_linear_bf16 / _fp8    gemm_bf16<42,22> / gemm_fp8<42,22>
  bf16_packed   mmdm_linear_bf16_packed    gemm_bf16w<14,41> (narrow), gemm_bf16w<14,42> (wide, forced at small shapes)
  fp8_packed    mmdm_linear_fp8_packed     gemm_fp8w<14,41>, gemm_fp8w<14,42>, and the persistent gemm_fp8p under "fp8p" = 2
Every run asserts the instantiation through mmdm_last_gemm_kernel().

The library is called through ctypes, so strides and pointers are the test's own (tests/gemm_cases.py::layout): A is a column slice of a
wider buffer of finite garbage, W has ldw > K, operand planes have a gap between them, `extra` has ld_extra > N, and C is a window [M, N]
inside a NaN-filled [M + 8, ldc] buffer; after the call every byte outside the window must be what it was.  One contiguous layout is kept.

Lattice operands (tests/gemm_cases.py, proven exact on the CPU by tests/test_gemm_cases_cpu.py) make bias / resid / pe results equal to the
float64 reference BIT FOR BIT: there is no tolerance in any of those comparisons, and the 16-bit / fp8 / plane outputs must equal the CPU
encoders of that reference.  Each of them runs under both epilogue forms ("split_tst" / "bf16_tst" = 0: direct, 1: transposed through LDS).
Shapes are gemm_cases.TABLE's sweeps (every M at one (N, K), every N at one (M, K), every K at one (M, N), the corner); the M sweep runs resid
and pe, the N sweep in-place resid and pe, the K sweep bias, the corner all four in both layouts (gemm_cases.SWEEP_EPIS: resid and pe carry the bias).
gelu / silu run on Gaussian operands against float64 of the operands as received, under the project's own tolerances (tests/test_gpu_headline.py,
tests/test_gpu_configs.py: atol 2e-5 sqrt(K / 1024) with a floor of 2e-5, rtol 1e-5; tests/test_gpu_fp8.py: atol 2e-4, rtol 1e-4).
"""
import contextlib
import ctypes as C
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as GC            # noqa: E402

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 4
OUTS = {"split": ("f32", "planes"), "bf16": ("f32", "bf16"), "fp8": ("f32", "bf16", "fp8")}
TST_KEY = {"split": None, "split_packed": "split_tst", "bf16": "bf16_tst", "bf16_packed": "bf16_tst", "fp8": "bf16_tst", "fp8_packed": "bf16_tst"}
ODT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp8": torch.uint8, "planes": torch.float16}
ENC = {"f32": lambda t: t.float(), "bf16": GC.enc_bf16, "fp8": GC.enc_e4m3, "planes": GC.enc_split}


def _tst_default(name):
    """The build's default of a *_tst switch: -DMMDM_<name>_TST_DEFAULT=<v> among build.py's flags, else the sources' 1."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mixermdm_amd", "build.py")) as f:
        src = f.read()
    m = re.search(rf"-DMMDM_{name}_TST_DEFAULT=(\d+)", src)
    return int(m.group(1)) if m else 1


RESTORE = {"split_cfg": -1, "bf16_cfg": -1, "fp8p": 0, "split_tst": _tst_default("SPLIT"), "bf16_tst": _tst_default("BF16")}


@contextlib.contextmanager
def diags(**kv):
    from mixermdm_amd._lib import diag
    try:
        for k, v in kv.items():
            diag(k, v)
        yield
    finally:
        for k in kv:
            diag(k, RESTORE[k])


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _vp(ptr):
    return C.c_void_p(ptr)


def _base(form):
    return form.split("_")[0]


def expected_kernel(form, M, N, K, forced=False):
    if form == "split":
        if N <= 512:
            return "gemm_split<22,21>"
        return "gemm_split<42,22>+gemm_split<22,21>" if (M, N) == GC.HYBRID[:2] else "gemm_split<42,22>"
    if form == "split_packed":
        if N & 127:
            return "gemm_splitw<22,21>"
        few = -(-M // 128) * (N // 128) < 256
        return "gemm_splitw<12,41>" if not forced and (N <= 512 or few or M <= 64) else "gemm_splitw<14,41>"
    if form in ("bf16", "fp8"):
        return f"gemm_{form}<42,22>"
    return f"gemm_{_base(form)}w<14,4{2 if forced and N % 256 == 0 else 1}>"      # every un-forced shape here is below the wide form's thresholds


class Placed:
    """A Case on the device in one layout of one form: operands are uploaded (and packed) once, run() makes a fresh output buffer per call."""
    def __init__(self, form, c, strided=True):
        from mixermdm_amd._lib import load_library, check
        self.form, self.c, self.base, self.packed = form, c, _base(form), form.endswith("_packed")
        self.lib, d = load_library(), _dev()
        L = self.L = GC.layout(form, c.M, c.N, c.K, strided)
        self.es = 1 if self.base == "fp8" else 2
        self.a_buf, self.a_plane = self._operand(c.x, L["lda"], L["a_c0"], L["a_rows"])
        self.A = self.a_buf.data_ptr() + L["a_c0"] * self.es
        w_buf, self.w_plane = self._operand(c.w, L["ldw"], L["w_c0"], c.N)
        W = w_buf.data_ptr() + L["w_c0"] * self.es
        self.ldw = L["ldw"]
        if self.packed:
            self.ldw = 0
            if self.base == "split":
                plane = c.N * c.K + L["gap"]
                self.w_buf = torch.full((2, plane), GC.A_GARBAGE, dtype=torch.float16, device=d)
                check(self.lib.mmdm_split_pack_weight(_vp(W), L["ldw"], self.w_plane, _vp(self.w_buf.data_ptr()), plane, c.N, c.K, None))
                self.w_plane = plane
            else:
                self.w_buf = torch.zeros(c.N * c.K * self.es, dtype=torch.uint8, device=d)
                check(self.lib.mmdm_pack_weight_frag(_vp(W), L["ldw"] * self.es, _vp(self.w_buf.data_ptr()), c.N, c.K * self.es, None))
            torch.cuda.synchronize()
            self.W = self.w_buf.data_ptr()
        else:
            self.w_buf, self.W = w_buf, W
        self.bias = c.bias.to(d) if c.bias is not None else None
        self.a_scale = c.a_scale.to(d) if c.a_scale is not None else None
        self.w_scale = c.w_scale.to(d) if c.w_scale is not None else None
        assert self.base == "fp8" or (self.a_scale is None and self.w_scale is None)
        self.extra = None
        if c.extra is not None:
            self.extra = GC.place(c.extra, L["ld_extra"], L["e_c0"], c.extra.shape[0] + 1, GC.EXTRA_GARBAGE).to(d)

    def _operand(self, t, ld, c0, rows):
        """fp32 CPU [r, K] -> (device buffer in the form's operand format, plane stride in elements): garbage beside, below and between the planes."""
        p = GC.place(t, ld, c0, rows, GC.A_GARBAGE)
        if self.base == "split":
            pl = GC.enc_split(p).reshape(2, -1)
            buf = torch.cat([pl, torch.full((2, self.L["gap"]), GC.A_GARBAGE, dtype=torch.float16)], 1).contiguous()
            return buf.to(_dev()), rows * ld + self.L["gap"]
        enc = GC.enc_bf16(p) if self.base == "bf16" else p.to(torch.float8_e4m3fn).view(torch.uint8)
        return enc.contiguous().to(_dev()), 0

    def run(self, out="f32", inplace=False):
        """One call.  Returns (window on the CPU -- [M, N], planes: [2, M, N] --, mmdm_last_gemm_kernel()) after the bytes outside it were checked."""
        from mixermdm_amd._lib import check
        c, L, d, G = self.c, self.L, _dev(), GC.GUARD
        M, N, K, ldc, c0 = c.M, c.N, c.K, L["ldc"], L["c_c0"]
        rows, dt = M + 2 * G, ODT[out]
        es = torch.empty(0, dtype=dt).element_size()
        npl = 2 if out == "planes" else 1
        c_plane = rows * ldc + L["c_gap"] if out == "planes" else 0
        buf = torch.full((npl, max(c_plane, rows * ldc)), 0x7F if out == "fp8" else float("nan"), dtype=dt, device=d)      # 0x7f: e4m3's NaN
        win = lambda t: t[:, :rows * ldc].view(npl, rows, ldc)[:, G:G + M, c0:c0 + N]
        extra, ld_extra = (self.extra.data_ptr() + L["e_c0"] * 4, L["ld_extra"]) if self.extra is not None else (0, 0)
        Cp = buf.data_ptr() + (G * ldc + c0) * es
        if inplace:
            assert out == "f32" and c.epi == "resid"
            win(buf)[0].copy_(c.extra.to(d))
            extra, ld_extra = Cp, ldc
        init = buf.clone()
        tail = (M, N, K, GC.EPI[c.epi], _vp(extra), ld_extra, c.period, None)
        bias = _vp(self.bias.data_ptr() if self.bias is not None else 0)
        lib, f = self.lib, self.form
        if f == "split":
            rc = lib.mmdm_linear_split(_vp(self.A), L["lda"], self.a_plane, _vp(self.W), self.ldw, self.w_plane, bias, _vp(Cp), ldc, c_plane, int(out == "planes"), *tail)
        elif f == "split_packed":
            rc = lib.mmdm_linear_split_packed(_vp(self.A), L["lda"], self.a_plane, _vp(self.W), self.w_plane, bias, _vp(Cp), ldc, c_plane, int(out == "planes"), *tail)
        elif f == "bf16":
            rc = lib.mmdm_linear_bf16(_vp(self.A), L["lda"], _vp(self.W), self.ldw, bias, _vp(Cp), ldc, int(out == "bf16"), *tail)
        elif f == "bf16_packed":
            rc = lib.mmdm_linear_bf16_packed(_vp(self.A), L["lda"], _vp(self.W), bias, _vp(Cp), ldc, int(out == "bf16"), *tail)
        else:
            sa = _vp(self.a_scale.data_ptr() if self.a_scale is not None else 0)
            sw = _vp(self.w_scale.data_ptr() if self.w_scale is not None else 0)
            mode = ("f32", "bf16", "fp8").index(out)
            if f == "fp8":
                rc = lib.mmdm_linear_fp8(_vp(self.A), L["lda"], sa, _vp(self.W), self.ldw, sw, bias, _vp(Cp), ldc, mode, *tail)
            else:
                rc = lib.mmdm_linear_fp8_packed(_vp(self.A), L["lda"], sa, _vp(self.W), sw, bias, _vp(Cp), ldc, mode, *tail)
        check(rc)
        name = lib.mmdm_last_gemm_kernel().decode()
        torch.cuda.synchronize()
        got, was = buf.cpu(), init.cpu()
        res = win(got).clone()
        win(got).zero_()
        win(was).zero_()
        assert torch.equal(GC.bits(got), GC.bits(was)), f"{f} {out}: bytes outside the [{M}, {N}] window changed"
        return (res if out == "planes" else res[0]), name


def _assert_bits(got, want, what):
    g, w = GC.bits(got), GC.bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {i}: got {got[i].float().item()!r}, want {want[i].float().item()!r}")


def _exact(form, c, strided=True, inplace=False, forced=None, outs=None, expect=None):
    """Runs a lattice case under both epilogue forms, in every output form: bit-equal to the (encoded) float64 reference."""
    P = Placed(form, c, strided)
    ref32 = c.ref().float()
    assert torch.equal(ref32.double(), c.ref())
    expect = expect or expected_kernel(form, c.M, c.N, c.K, forced is not None)
    key = TST_KEY[form]
    for tst in ((0, 1) if key else (None,)):
        kv = {key: tst} if key else {}
        if forced:
            kv[forced[0]] = forced[1]
        with diags(**kv):
            for out in outs or OUTS[_base(form)]:
                if inplace and out != "f32":
                    continue
                got, name = P.run(out, inplace)
                assert name == expect, (name, expect)
                _assert_bits(got, ENC[out](ref32), f"{form} {c.M}x{c.N}x{c.K} {c.epi} out={out} tst={tst} {'strided' if strided else 'contiguous'}{' in place' if inplace else ''}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1 + 2: exact, under both epilogue forms
# ---------------------------------------------------------------------------------------------------------------------------------------
EXACT = [(f,) + e for f in GC.FORMS for e in GC.exact_cases(f)]


@pytest.mark.parametrize("form,M,N,K,epi,period,strided", EXACT, ids=[f"{f}-{M}x{N}x{K}-{e}-{'strided' if s else 'contig'}" for f, M, N, K, e, p, s in EXACT])
def test_lattice_results_are_bit_exact(form, M, N, K, epi, period, strided):
    _exact(form, GC.lattice_case_of(form, M, N, K, epi, period), strided, inplace=epi == "resid_inplace")


@pytest.mark.parametrize("which", (0, 1, 2), ids=("period5", "period299", "periodM+3"))
@pytest.mark.parametrize("form", GC.FORMS)
def test_pe_periods_at_one_row_past_a_tile(form, which):
    """M = BM + 1: the last tile holds one valid row and 31+ clamped ones, whose PE rows must not reach row M - 1; periods below a 32-row
    tile, between, and above M (the table is then never wrapped)."""
    M = GC.TABLE[form]["BM"] + 1
    N, K = GC.TABLE[form]["m_at"]
    _exact(form, GC.lattice_case_of(form, M, N, K, "pe", GC.pe_periods(M)[which]))


FORCED = [(f, s, e) for f in GC.FORCED for s in GC.FORCED[f][2] for e in ("resid", "pe")]


@pytest.mark.parametrize("form,shape,epi", FORCED, ids=[f"{f}-{'x'.join(map(str, s))}-{e}" for f, s, e in FORCED])
def test_forced_wide_tiles(form, shape, epi):
    """gemm_splitw<14,41>, gemm_bf16w<14,42>, gemm_fp8w<14,42>: the tiles the large shards take, forced at one, two and three K steps."""
    key, val, _ = GC.FORCED[form]
    _exact(form, GC.lattice_case_of(form, *shape, epi, GC.DEFAULT_PERIOD if epi == "pe" else 0), forced=(key, val))


@pytest.mark.parametrize("epi", ("resid", "pe"))
@pytest.mark.parametrize("shape", GC.SPLIT_BIG_TILE, ids=lambda s: "x".join(map(str, s)))
def test_split_plane_kernel_256x128_tile(shape, epi):
    _exact("split", GC.lattice_case_of("split", *shape, epi, GC.DEFAULT_PERIOD if epi == "pe" else 0))


@pytest.mark.parametrize("epi", ("bias", "resid", "resid_inplace", "pe"))
def test_split_hybrid_launch(epi):
    """Rows [0, 8192) on gemm_split<42,22>, the last 257 on gemm_split<22,21> with offset A / C / residual pointers and row0 = 8192 for PE
    (8192 % 299 != 0), fp32 and plane output."""
    M, N, K, M1 = GC.HYBRID
    c = GC.lattice_case_of("split", M, N, K, epi, GC.HYBRID_PERIOD if epi == "pe" else 0, M1)
    _exact("split", c, inplace=epi == "resid_inplace", expect="gemm_split<42,22>+gemm_split<22,21>")


@pytest.mark.parametrize("shape", GC.FEW_THRESHOLD, ids=lambda s: "x".join(map(str, s)))
def test_split_packed_tile_choice_at_the_few_tiles_threshold(shape):
    M, N, K = shape
    want = "gemm_splitw<12,41>" if -(-M // 128) * (N // 128) < 256 else "gemm_splitw<14,41>"
    _exact("split_packed", GC.lattice_case_of("split_packed", M, N, K, "resid"), outs=("f32",), expect=want)


@pytest.mark.parametrize("has_bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("w_s", (True, False), ids=("wscale", "wnull"))
@pytest.mark.parametrize("a_s", (True, False), ids=("ascale", "anull"))
@pytest.mark.parametrize("form,shape", (("fp8", (129, 132, 128)), ("fp8_packed", (129, 128, 256))), ids=("plane", "packed"))
def test_fp8_scale_pointer_combinations(form, shape, a_s, w_s, has_bias):
    """a_scale / w_scale / bias null or not: the global reads of the direct epilogue and of the plane kernel, the LDS copy of the packed one."""
    _exact(form, GC.case("lattice", *shape, "bias", 0, (a_s, w_s), has_bias))


@pytest.mark.parametrize("form", ("fp8", "fp8_packed"))
def test_fp8_output_saturates(form):
    c = GC.saturating_case()
    P = Placed(form, c)
    want = GC.enc_e4m3(c.ref().float())
    for tst in (0, 1):
        with diags(bf16_tst=tst):
            got, _ = P.run("fp8")
        assert got[1, 2] == 0x7E and got[3, 2] == 0xFE and not ((got & 0x7F) == 0x7F).any(), (got[1, 2], got[3, 2])      # +448, -448, no NaN
        _assert_bits(got, want, f"{form} saturating tst={tst}")
        assert (got.view(torch.float8_e4m3fn).float()[1] == -got.view(torch.float8_e4m3fn).float()[3]).all()             # sign symmetry of the negated row


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3: activations on Gaussian operands
# ---------------------------------------------------------------------------------------------------------------------------------------
ACT = [(b, s, e, o) for b in ("split", "bf16", "fp8") for s in GC.ACT_SHAPES[b] for e in ("gelu", "silu") for o in OUTS[b]]
_F32 = {}


def _act_f32(form, c):
    """The fp32 output of a Gaussian case under the build's default epilogue form (one launch per form and case, shared)."""
    if (form, id(c)) not in _F32:
        _F32[(form, id(c))] = Placed(form, c).run("f32")[0]
    return _F32[(form, id(c))]


@pytest.mark.parametrize("base,shape,epi,out", ACT, ids=[f"{b}-{'x'.join(map(str, s))}-{e}-{o}" for b, s, e, o in ACT])
def test_activations_against_float64(base, shape, epi, out):
    M, N, K = shape
    c = GC.case("gauss", M, N, K, epi, 0, (True, True) if base == "fp8" else (False, False))
    ref = c.ref(base)
    atol, rtol = (2e-4, 1e-4) if base == "fp8" else (max(2e-5, 2e-5 * math.sqrt(K / 1024)), 1e-5)
    seen = []
    for form in (base, base + "_packed"):
        f32 = _act_f32(form, c)
        if out == "f32":
            err = (f32.double() - ref).abs()
            print(f"{form} {shape} {epi}: max err {err.max().item():.3e} (atol {atol:.1e}), worst excess {(err - atol - rtol * ref.abs()).max().item():.3e}")
            assert (err <= atol + rtol * ref.abs()).all()
        P, key = Placed(form, c), TST_KEY[form]
        for tst in ((0, 1) if key else (None,)):
            with diags(**({key: tst} if key else {})):
                got, name = P.run(out)
            assert name == expected_kernel(form, M, N, K)
            _assert_bits(got, ENC[out](f32), f"{form} {epi} out={out} tst={tst} against the encoding of the call's fp32 output")
            seen.append(GC.bits(got))
    assert all(torch.equal(s, seen[0]) for s in seen), "plane and packed kernels (one definition for every kernel) must give the same bits"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the persistent fp8 kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ("bf16", "fp8"))
@pytest.mark.parametrize("epi", ("bias", "gelu"))
@pytest.mark.parametrize("shape", GC.FP8P, ids=lambda s: "x".join(map(str, s)))
def test_persistent_fp8_kernel(shape, epi, out):
    """512 tiles (one per workgroup) and 520 (no multiple of the grid).  bias: exact against float64; gelu: within the fp8 tolerance of float64
    through the packed kernel's fp32 output, whose encoding both kernels must produce."""
    M, N, K = shape
    c = GC.lattice_case_of("fp8_packed", M, N, K, epi)
    P = Placed("fp8_packed", c)
    with diags(fp8p=2):
        got, name = P.run(out)
    assert name == f"gemm_fp8p<{2 if out == 'fp8' else 1},{GC.EPI[epi]},0,1>", name
    if epi == "bias":
        _assert_bits(got, ENC[out](c.ref().float()), f"gemm_fp8p {shape} bias out={out}")
        return
    f32, name = P.run("f32")
    assert name == "gemm_fp8w<14,41>"
    ref = c.ref()
    err = (f32.double() - ref).abs()
    print(f"fp8w {shape} gelu: max err {err.max().item():.3e}")
    assert (err <= 2e-4 + 1e-4 * ref.abs()).all()
    _assert_bits(got, ENC[out](f32), f"gemm_fp8p {shape} gelu out={out} against the encoding of the packed kernel's fp32 output")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4: refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
RM, RN, RK = 8, 128, 256          # a shape every entry point accepts


def _refusal_args(form):
    """Valid arguments of a small call, as a dict of ints (pointers as addresses), over amply sized zero-filled buffers."""
    d = _dev()
    q = 16 if _base(form) == "fp8" else 8
    bufs = dict(A=torch.zeros(1 << 16, dtype=torch.float16, device=d), W=torch.zeros(1 << 18, dtype=torch.float16, device=d),
                C=torch.full((1 << 14,), float("nan"), device=d), bias=torch.zeros(1024, device=d), extra=torch.zeros(1 << 14, device=d),
                a_scale=torch.ones(1024, device=d), w_scale=torch.ones(1024, device=d))
    a = {k: v.data_ptr() for k, v in bufs.items()}
    a.update(lda=RK + q, ldw=0 if form.endswith("_packed") else RK + q, a_plane=4096, w_plane=RN * RK + 64, ldc=RN + 4, c_plane=4096, out=0,
             M=RM, N=RN, K=RK, epi=0, ld_extra=RN + 4, period=0)
    return a, bufs


def _invoke(lib, form, a):
    tail = (a["M"], a["N"], a["K"], a["epi"], _vp(a["extra"]), a["ld_extra"], a["period"], None)
    if form == "split":
        return lib.mmdm_linear_split(_vp(a["A"]), a["lda"], a["a_plane"], _vp(a["W"]), a["ldw"], a["w_plane"], _vp(a["bias"]), _vp(a["C"]), a["ldc"], a["c_plane"], a["out"], *tail)
    if form == "split_packed":
        return lib.mmdm_linear_split_packed(_vp(a["A"]), a["lda"], a["a_plane"], _vp(a["W"]), a["w_plane"], _vp(a["bias"]), _vp(a["C"]), a["ldc"], a["c_plane"], a["out"], *tail)
    if form == "bf16":
        return lib.mmdm_linear_bf16(_vp(a["A"]), a["lda"], _vp(a["W"]), a["ldw"], _vp(a["bias"]), _vp(a["C"]), a["ldc"], a["out"], *tail)
    if form == "bf16_packed":
        return lib.mmdm_linear_bf16_packed(_vp(a["A"]), a["lda"], _vp(a["W"]), _vp(a["bias"]), _vp(a["C"]), a["ldc"], a["out"], *tail)
    if form == "fp8":
        return lib.mmdm_linear_fp8(_vp(a["A"]), a["lda"], _vp(a["a_scale"]), _vp(a["W"]), a["ldw"], _vp(a["w_scale"]), _vp(a["bias"]), _vp(a["C"]), a["ldc"], a["out"], *tail)
    return lib.mmdm_linear_fp8_packed(_vp(a["A"]), a["lda"], _vp(a["a_scale"]), _vp(a["W"]), _vp(a["w_scale"]), _vp(a["bias"]), _vp(a["C"]), a["ldc"], a["out"], *tail)


def _refusals(form, a):
    """[(what, changed arguments, status, fragment of mmdm_last_error())].  Read against the three _ex functions: every check below
    precedes the launch, the 4 GB reach of the plane strides included (a number, no allocation behind it)."""
    b, packed = _base(form), form.endswith("_packed")
    name = {"split": "mmdm_linear_split", "bf16": "mmdm_linear_bf16", "fp8": "mmdm_linear_fp8"}[b]
    kq = 64 if b == "fp8" else 32
    half = 8 if b == "fp8" else 4             # elements that break the 16-byte alignment of an operand row
    al_op = f"K % {kq} == 0 and 16-byte aligned"
    al_out = "N % 4 == 0 and 16-byte aligned"
    R = [("unknown epilogue", dict(epi=5), ERR_ARG, "unknown epilogue 5"), ("negative epilogue", dict(epi=-1), ERR_ARG, "unknown epilogue"),
         ("resid without extra", dict(epi=2, extra=0), ERR_ARG, "needs `extra` with ld >= N"), ("ld_extra < N", dict(epi=2, ld_extra=RN - 4), ERR_ARG, "needs `extra` with ld >= N"),
         ("pe ld_extra < N", dict(epi=3, period=5, ld_extra=RN - 4), ERR_ARG, "needs `extra` with ld >= N"),
         ("pe period 0", dict(epi=3, period=0), ERR_ARG, "PE epilogue needs period > 0"), ("pe period < 0", dict(epi=3, period=-3), ERR_ARG, "PE epilogue needs period > 0"),
         ("lda < K", dict(lda=RK - 16), ERR_ARG, "bad shape"), ("ldc < N", dict(ldc=RN - 4), ERR_ARG, "bad shape"), ("M < 0", dict(M=-1), ERR_ARG, "bad shape"),
         ("null A", dict(A=0), ERR_ARG, "bad shape"), ("null W", dict(W=0), ERR_ARG, "bad shape"), ("null C", dict(C=0), ERR_ARG, "bad shape"),
         ("lda misaligned", dict(lda=a["lda"] + half), ERR_UNSUPPORTED, al_op), ("A misaligned", dict(A=a["A"] + 8), ERR_UNSUPPORTED, al_op),
         ("W misaligned", dict(W=a["W"] + 8), ERR_UNSUPPORTED, al_op),
         ("ldc % 4", dict(ldc=RN + 2), ERR_UNSUPPORTED, al_out), ("C misaligned", dict(C=a["C"] + 4), ERR_UNSUPPORTED, al_out), ("bias misaligned", dict(bias=a["bias"] + 4), ERR_UNSUPPORTED, al_out),
         ("ld_extra % 4", dict(epi=2, ld_extra=RN + 2), ERR_UNSUPPORTED, al_out), ("extra misaligned", dict(epi=2, extra=a["extra"] + 8), ERR_UNSUPPORTED, al_out)]
    if packed:
        tn, tk = {"split": (64, 64), "bf16": (128, 128), "fp8": (128, 256)}[b]
        frag = f"{name}_packed: needs N % {tn} == 0 and K % {tk} == 0"
        R += [("packed N", dict(N=RN - tn // 2), ERR_UNSUPPORTED, frag), ("packed K", dict(K=RK + tk // 2), ERR_UNSUPPORTED, frag)]
    else:
        R += [("K step", dict(K=RK - kq // 2), ERR_UNSUPPORTED, al_op), ("N % 4", dict(N=RN - 2), ERR_UNSUPPORTED, al_out), ("K = 0", dict(K=0), ERR_ARG, "bad shape"),
              ("ldw < K", dict(ldw=RK - 16), ERR_ARG, "bad shape"), ("ldw misaligned", dict(ldw=a["ldw"] + half), ERR_UNSUPPORTED, al_op)]
    if b == "split":
        R += [("a_plane 0", dict(a_plane=0), ERR_ARG, "bad shape"), ("w_plane 0", dict(w_plane=0), ERR_ARG, "bad shape"), ("a_plane < 0", dict(a_plane=-8), ERR_ARG, "bad shape"),
              ("c_plane 0 with plane output", dict(out=1, c_plane=0), ERR_ARG, "bad shape"),
              ("a_plane misaligned", dict(a_plane=a["a_plane"] + 4), ERR_UNSUPPORTED, al_op), ("w_plane misaligned", dict(w_plane=a["w_plane"] + 4), ERR_UNSUPPORTED, al_op),
              ("c_plane % 4", dict(out=1, c_plane=a["c_plane"] + 2), ERR_UNSUPPORTED, al_out),
              ("a_plane beyond 4 GB", dict(a_plane=1 << 30), ERR_UNSUPPORTED, "operand planes beyond the 4 GB reach"),
              ("w_plane beyond 4 GB", dict(w_plane=1 << 30), ERR_UNSUPPORTED, "operand planes beyond the 4 GB reach"),
              ("c_plane beyond 4 GB", dict(out=1, c_plane=1 << 31), ERR_UNSUPPORTED, "output planes beyond the 4 GB reach")]
    if b == "fp8":
        R += [("out_mode 3", dict(out=3), ERR_ARG, "out_mode must be 0"), ("out_mode -1", dict(out=-1), ERR_ARG, "out_mode must be 0"),
              ("w_scale misaligned", dict(w_scale=a["w_scale"] + 4), ERR_UNSUPPORTED, al_out)]
    return R


@pytest.mark.parametrize("form", GC.FORMS)
def test_argument_refusals(form):
    """Every mmdm_set_error branch of the entry point: its documented status, its message, and an untouched NaN-filled output."""
    from mixermdm_amd._lib import load_library
    lib = load_library()
    a, bufs = _refusal_args(form)
    R = _refusals(form, a)
    for what, change, code, frag in R:
        rc = _invoke(lib, form, {**a, **change})
        msg = (lib.mmdm_last_error() or b"").decode()
        assert rc == code, (form, what, rc, msg)
        assert frag in msg, (form, what, msg)
        assert lib.mmdm_last_gemm_kernel().decode() == "", (form, what)          # nothing was launched
    for what, change in (("M = 0", dict(M=0)), ("N = 0", dict(N=0))):
        assert _invoke(lib, form, {**a, **change}) == OK, (form, what)
        assert lib.mmdm_last_gemm_kernel().decode() == "", (form, what)
    torch.cuda.synchronize()
    assert torch.isnan(bufs["C"]).all()

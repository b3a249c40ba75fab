"""GPU: mmdm_linear_f32 at its tile edges, on every branch of its dispatch, exact on a lattice.

Kernels (csrc/gemm_f32.hip; the automatic dispatch picks one from the call's shape, alignment and epilogue):
  gemm_f32<22,22,16>                     register-staged fallback (K % 16, a misaligned A or W), four load variants
  gemm_glds<22,21|22,22,16,2,...>        2-stage LDS-DMA kernels, K < 96
  gemm_pipe<21,21,16,4|22,21,16,4|22,22,16,5,vepi|scalar>   the pipelined kernels, 16-byte or scalar epilogue
  gemm_s16<1,4,late|plain>               16 x 16 chains for launches of few tiles
  gemm_mix<vepi|scalar,a+b>              whole rounds on 64 x 64 tiles + the remaining rows on 16 x 16 chains, one launch
Every run asserts the instantiation through mmdm_last_gemm_kernel() against tests/gemm_f32_cases.py::expected_kernel_f32, the suite's
statement of the dispatch rule (held to the tables' hand-written names on the CPU by tests/test_gemm_f32_cases_cpu.py, and csrc/gemm_f32_plan.h
to it by tests/test_gemm_f32_plan_cpu.py).  The forced kernels (gemm_cfg) run once each on one shape.

The library is called through ctypes, so strides and pointers are the test's own (gemm_f32_cases.layout_f32): A, W and `extra` are windows of
wider buffers of finite garbage, C is a window [M, N] of a NaN-filled [M + 8, ldc] buffer, and the alignment kinds move one pointer or
stride off its 16-byte grid.  After a call every byte outside the window must be what it was.

Lattice operands (proven exact on the CPU) make bias / resid / pe results equal to the float64 reference BIT FOR BIT: no tolerance in any of
those comparisons, whatever the tile, the chain length or the order in which an epilogue adds bias and residual.  The activations run on
Gaussian operands against float64 under the project's own tolerance (tests/test_gpu_headline.py, tests/test_gpu_configs.py: atol
2e-5 sqrt(K / 1024) with a floor of 2e-5, rtol 1e-5), every element.
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
import gemm_f32_cases as F         # noqa: E402

OK, ERR_ARG = 0, 1


def _s16_default():
    """The build's default of the gemm_s16 switch: -DMMDM_S16_DEFAULT=<v> among build.py's flags, else the sources' -1."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mixermdm_amd", "build.py")) as f:
        m = re.search(r"-DMMDM_S16_DEFAULT=(-?\d+)", f.read())
    return int(m.group(1)) if m else -1


RESTORE = {"gemm_cfg": -1, "gemm_tail": -1, "gemm_s16": _s16_default()}


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


@pytest.fixture(scope="module", autouse=True)
def _switches_are_at_automatic():
    """gemm_cfg, gemm_tail and gemm_s16 as the build leaves them: M = 8320, N = 1024 is 65 x 8 = 520 tiles of 128 x 128, which the row split (any
    gemm_tail > 0) would cut after 64 row tiles into two launches, a forced gemm_cfg would give to its own tile, and (129, 260, 96) goes to the
    16 x 16 chains only under the automatic gemm_s16."""
    from mixermdm_amd._lib import load_library, check
    lib, d = load_library(), _dev()
    assert RESTORE["gemm_s16"] == -1, "expected_kernel_f32 mirrors the automatic small-launch rule"
    for (M, N, K), want in (((8320, 1024, 528), "gemm_pipe<22,22,16,5,scalar>"), ((129, 260, 96), "gemm_s16<1,4,plain>")):
        assert want == F.expected_kernel_f32(M, N, K, "bias")
        a, w, c = torch.zeros(M, K, device=d), torch.zeros(N, K, device=d), torch.empty(M, N, device=d)
        check(lib.mmdm_linear_f32(_vp(a.data_ptr()), K, _vp(w.data_ptr()), K, None, _vp(c.data_ptr()), N, M, N, K, 0, None, 0, 0, None))
        name = lib.mmdm_last_gemm_kernel().decode()
        torch.cuda.synchronize()
        assert name == want, f"a diagnostic switch is not at automatic: {name}"
    yield


class Placed:
    """A Case on the device in one layout: operands are uploaded once, run() makes a fresh output buffer per call."""
    def __init__(self, c, kind="strided"):
        from mixermdm_amd._lib import load_library
        self.c, self.kind, self.lib, d = c, kind, load_library(), _dev()
        L = self.L = F.layout_f32(kind, c.M, c.N, c.K)
        self.a_buf = GC.place(c.x, L["lda"], L["a_c0"], L["a_rows"], F.A_GARBAGE).to(d)
        self.w_buf = GC.place(c.w, L["ldw"], L["w_c0"], c.N + 1, F.A_GARBAGE).to(d)
        self.A, self.W = self.a_buf.data_ptr() + 4 * L["a_c0"], self.w_buf.data_ptr() + 4 * L["w_c0"]
        assert self.a_buf.data_ptr() % 256 == 0 and self.w_buf.data_ptr() % 256 == 0
        self.b_buf, self.bias = None, 0
        if c.bias is not None:
            b = torch.full((c.N + 4,), F.EXTRA_GARBAGE)
            b[L["b_off"]:L["b_off"] + c.N] = c.bias
            self.b_buf = b.to(d)
            self.bias = self.b_buf.data_ptr() + 4 * L["b_off"]
        self.e_buf = None
        if c.extra is not None:
            self.e_buf = GC.place(c.extra, L["ld_extra"], L["e_c0"], c.extra.shape[0] + 1, F.EXTRA_GARBAGE).to(d)
        for what, (end, alloc) in F.extents(L, c.M, c.N, c.K, 0 if c.extra is None else c.extra.shape[0]).items():
            assert 0 <= end <= alloc, (what, end, alloc)

    def expected(self, epi=None, inplace=False):
        c = self.c
        return F.expected_kernel_f32(c.M, c.N, c.K, epi or c.epi, **F.alignment(self.L, c.bias is not None, inplace))

    def run(self, inplace=False, epi=None):
        """One call (`epi`: an activation in place of the case's "bias").  Returns (window on the CPU, mmdm_last_gemm_kernel()) after every
        byte outside the window was compared with what it was."""
        from mixermdm_amd._lib import check
        c, L, d, G = self.c, self.L, _dev(), F.GUARD
        M, N, K, ldc, c0 = c.M, c.N, c.K, L["ldc"], L["c_c0"]
        buf = torch.full((M + 2 * G, ldc), float("nan"), device=d)
        assert buf.data_ptr() % 256 == 0
        win = lambda t: t[G:G + M, c0:c0 + N]
        Cp = buf.data_ptr() + 4 * (G * ldc + c0)
        extra, ld_extra = (self.e_buf.data_ptr() + 4 * L["e_c0"], L["ld_extra"]) if self.e_buf is not None else (0, 0)
        if inplace:
            assert c.epi == "resid"
            win(buf).copy_(c.extra.to(d))
            extra, ld_extra = Cp, ldc
        was = buf.clone()
        check(self.lib.mmdm_linear_f32(_vp(self.A), L["lda"], _vp(self.W), L["ldw"], _vp(self.bias), _vp(Cp), ldc, M, N, K, F.EPI[epi or c.epi],
                                       _vp(extra), ld_extra, c.period, None))
        name = self.lib.mmdm_last_gemm_kernel().decode()
        torch.cuda.synchronize()
        res = win(buf).cpu()
        win(buf).zero_()
        win(was).zero_()
        assert torch.equal(GC.bits(buf), GC.bits(was)), f"{name}: bytes outside the [{M}, {N}] window changed"
        return res, name


def _assert_bits(got, want, what):
    g, w = GC.bits(got), GC.bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {i}: got {got[i].item()!r}, want {want[i].item()!r}; "
                             f"rows {bad[:, 0].min().item()}..{bad[:, 0].max().item()}, columns {bad[:, 1].min().item()}..{bad[:, 1].max().item()}")


def _exact(c, kind="strided", inplace=False, expect=None, placed=None):
    """Runs a lattice case: the kernel the mirror names, bit-equal to the float64 reference."""
    P = placed or Placed(c, kind)
    ref32 = c.ref().float()
    assert torch.equal(ref32.double(), c.ref())
    got, name = P.run(inplace)
    want = P.expected(inplace=inplace)
    assert name == want and (expect is None or name == expect), (name, want, expect)
    _assert_bits(got, ref32, f"{name} {c.M}x{c.N}x{c.K} {c.epi}{c.period or ''} {kind}{' in place' if inplace else ''}")
    return name


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact: every table entry x its epilogues x its layouts
# ---------------------------------------------------------------------------------------------------------------------------------------
RUNS = F.exact_runs()


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[f"{en.family}-{en.M}x{en.N}x{en.K}-{e}{p or ''}-{k}" for en, e, p, k in RUNS])
def test_lattice_results_are_bit_exact(i):
    en, e, p, kind = RUNS[i]
    _exact(F.lattice_case_f32(en.M, en.N, en.K, e, p), kind, inplace=e == "resid_inplace", expect=F.named_kernel(en, e, kind))


@pytest.mark.parametrize("epi", ("bias", "resid"))
@pytest.mark.parametrize("family", tuple(F.FAMILY_SHAPE))
def test_lattice_results_without_a_bias_pointer(family, epi):
    en = F.family_entry(family)
    _exact(F.lattice_case_f32(en.M, en.N, en.K, epi, 0, has_bias=False), expect=F.named_kernel(en, epi, has_bias=False))
    if family in ("s16", "mix", "pipe64") and epi == "bias":
        # a bias pointer that is not there cannot be misaligned: the layout that moves it changes nothing
        c = F.lattice_case_f32(en.M, en.N, en.K, epi, 0, has_bias=False)
        assert _exact(c, "bias_off1") == F.named_kernel(en, epi, "bias_off1", has_bias=False)


PAIRS = F.threshold_pairs()


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a.M}x{a.N}x{a.K}-{b.M}x{b.N}x{b.K}" for a, b in PAIRS])
def test_dispatch_thresholds(a, b):
    """Neighbouring shapes on the two sides of one dispatch condition land on their two kernels, and both are exact (every other epilogue of a
    pair runs in test_lattice_results_are_bit_exact)."""
    for epi in ("bias", "resid"):
        ka = _exact(F.lattice_case_f32(a.M, a.N, a.K, epi), expect=F.named_kernel(a, epi))
        kb = _exact(F.lattice_case_f32(b.M, b.N, b.K, epi), expect=F.named_kernel(b, epi))
        assert ka != kb, (epi, ka, kb)


@pytest.mark.parametrize("which", (0, 1, 2), ids=("period5", "period299", "periodM+3"))
@pytest.mark.parametrize("family", tuple(F.PE_SHAPE))
def test_pe_periods_across_tiles(family, which):
    """One row past a tile of each family: the last tile holds one valid row, whose PE row must be (M - 1) % period -- periods below a 32-row
    tile, between, and above M (the table is then never wrapped).  (A PE call is never mixed: test_lattice_results_are_bit_exact runs the mix
    shapes with periods 7 and 299 and asserts the 64 x 64 kernel.)"""
    en = F.family_entry(family, F.PE_SHAPE)
    bm = {"fallback": 128, "glds2": 128, "s16": 32, "pipe64": 64, "pipe128x64": 128, "pipe128": 128}[family]
    assert en.M % bm == 1
    _exact(F.lattice_case_f32(en.M, en.N, en.K, "pe", F.pe_periods(en.M)[which]), expect=F.named_kernel(en, "pe"))


@pytest.mark.parametrize("kind", ("strided", "c_off1"), ids=("aligned", "scalar"))
@pytest.mark.parametrize("family", tuple(F.FAMILY_SHAPE))
def test_in_place_residual_on_every_family(family, kind):
    """R aliases C.  Aligned: the 16-byte epilogue reads the residual quad before the K loop (s16 and mix: after it); C one float off its grid: the
    scalar epilogue reads each element just before it writes it (and neither s16 nor mix take the call)."""
    en = F.family_entry(family)
    c = F.lattice_case_f32(en.M, en.N, en.K, "resid")
    P = Placed(c, kind)
    name = _exact(c, kind, inplace=True, expect=F.named_kernel(en, "resid_inplace", kind), placed=P)
    if kind == "c_off1" and family != "fallback":
        assert name.endswith(",scalar>"), name
    # and the same operands with the residual beside C: the same bits from the same kernel
    assert _exact(c, kind, placed=P) == name


# ---------------------------------------------------------------------------------------------------------------------------------------
# activations on Gaussian operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gauss(M, N, K):
    """The Gaussian case of a shape (one for every activation) and its float64 pre-activation (computed once)."""
    c = GC.case("gauss", M, N, K, "bias")
    return c, c.ref("lattice")


@pytest.mark.parametrize("family", tuple(F.FAMILY_SHAPE))
def test_activations_against_float64(family):
    """gelu / silu / quickgelu / sigmoid (and the plain bias) of one tail shape per kernel family against float64, every element within
    atol max(2e-5, 2e-5 sqrt(K / 1024)), rtol 1e-5.
    Measured on an MI355X, largest |error| over bias and the four activations (atol 2e-5 everywhere here): fallback 5.7e-6, 2-stage 3.5e-6,
    s16 2.7e-6, pipe 64 x 64 2.4e-6, mix 4.2e-6, pipe 128 x 64 4.3e-6, pipe 128 x 128 (K = 528) 1.0e-5; sigmoid below 1.1e-6 on every family."""
    en = F.family_entry(family)
    c, z = _gauss(en.M, en.N, en.K)
    P = Placed(c)
    atol, rtol = max(2e-5, 2e-5 * math.sqrt(en.K / 1024)), 1e-5
    worst = []
    for epi in ("bias",) + F.ACTS:
        got, name = P.run(epi=epi)
        assert name == P.expected(epi) == F.named_kernel(en, epi), (name, epi)
        ref = F.act_f64(z, epi)
        err = (got.double() - ref).abs()
        print(f"{family} {name} {en.M}x{en.N}x{en.K} {epi}: max err {err.max().item():.3e} (atol {atol:.1e}), worst excess {(err - atol - rtol * ref.abs()).max().item():.3e}")
        worst.append((epi, bool((err <= atol + rtol * ref.abs()).all()), err.max().item()))
    assert all(ok for _, ok, _ in worst), worst


@pytest.mark.parametrize("shape", ((1025, 1024, 128), (3300, 260, 128)), ids=lambda s: "x".join(map(str, s)))
def test_pipe_s16_and_mix_give_the_same_bits(shape):
    """"Every pipelined instantiation accumulates an output element in the same order"; gemm_s16 and gemm_mix "bit-identical": the mixed launch (automatic),
    the 16 x 16 chains alone (gemm_s16 = 14), the 64 x 64 tiles alone (gemm_s16 = 0, and automatic under a misaligned bias) on one Gaussian case, for
    bias and every activation.  (Not across the two residual orders of the vepi / scalar epilogues, nor against the fallback or the 2-stage kernels.)"""
    M, N, K = shape
    c, _ = _gauss(M, N, K)
    P, Q = Placed(c), Placed(c, "bias_off1")
    n_mix = F.expected_kernel_f32(M, N, K, "bias")
    assert n_mix.startswith("gemm_mix<scalar,")
    for epi in ("bias",) + F.ACTS:
        mix, k0 = P.run(epi=epi)
        with diags(gemm_s16=14):
            s16, k1 = P.run(epi=epi)
        with diags(gemm_s16=0):
            p64, k2 = P.run(epi=epi)
        off, k3 = Q.run(epi=epi)
        assert (k0, k1, k2, k3) == (n_mix, "gemm_s16<1,4,plain>", "gemm_pipe<21,21,16,4,scalar>", "gemm_pipe<21,21,16,4,scalar>"), (k0, k1, k2, k3)
        assert torch.isfinite(mix).all()
        for what, t in (("gemm_s16", s16), ("gemm_pipe 64 x 64", p64), ("gemm_pipe 64 x 64 under a misaligned bias", off)):
            _assert_bits(t, mix, f"{what} against {k0}, {epi}, {M}x{N}x{K}")


FORCED = {1: "gemm_f32<22,22,16>", 11: "gemm_glds<22,22,16,2,{e}>", 17: "gemm_glds<22,21,16,2,{e}>", 34: "gemm_pipe<22,22,16,5,{e}>",
          36: "gemm_pipe<22,21,16,4,{e}>", 41: "gemm_pipe<21,21,16,4,{e}>"}


@pytest.mark.parametrize("cfg", tuple(FORCED))
def test_forced_kernels_are_bit_exact(cfg):
    """mmdm_diag_set("gemm_cfg", v) for every value that names a kernel (csrc/gemm_f32_plan.h), on the smallest aligned shape that passes each
    kernel's K floor and crosses a tile edge in M and N: the named kernel ran, the window equals float64 bit for bit, nothing beside it
    changed (Placed.run).  A forced pipelined kernel whose A is misaligned is the fallback."""
    M, N, K = 129, 132, 96
    for epi, e in (("bias", "scalar"), ("resid", "vepi")):
        c = F.lattice_case_f32(M, N, K, epi)
        with diags(gemm_cfg=cfg):
            got, name = Placed(c).run()
        assert name == FORCED[cfg].format(e=e), (cfg, epi, name)
        _assert_bits(got, c.ref().float(), f"gemm_cfg {cfg}: {name} {epi}")
    if cfg == 34:
        with diags(gemm_cfg=cfg):
            got, name = Placed(c, "a_off1").run()
        assert name == "gemm_f32<22,22,16>", name
        _assert_bits(got, c.ref().float(), f"gemm_cfg {cfg} under a misaligned A: {name}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals():
    """Every mmdm_set_error branch of mmdm_linear_f32: MMDM_ERR_ARG, its message, no kernel note, an untouched NaN-filled output.  M == 0 or N == 0: OK, no launch."""
    from mixermdm_amd._lib import load_library
    lib, d = load_library(), _dev()
    M, N, K = 8, 128, 256
    bufs = dict(A=torch.zeros(1 << 14, device=d), W=torch.zeros(1 << 17, device=d), C=torch.full((1 << 13,), float("nan"), device=d),
                bias=torch.zeros(1024, device=d), extra=torch.zeros(1 << 13, device=d))
    a = {k: v.data_ptr() for k, v in bufs.items()}
    a.update(lda=K + 4, ldw=K + 4, ldc=N + 4, M=M, N=N, K=K, epi=0, ld_extra=N + 4, period=0)

    def invoke(**change):
        v = {**a, **change}
        return lib.mmdm_linear_f32(_vp(v["A"]), v["lda"], _vp(v["W"]), v["ldw"], _vp(v["bias"]), _vp(v["C"]), v["ldc"], v["M"], v["N"], v["K"], v["epi"],
                                   _vp(v["extra"]), v["ld_extra"], v["period"], None)
    R = [("lda < K", dict(lda=K - 4), "bad shape"), ("ldw < K", dict(ldw=K - 4), "bad shape"), ("ldc < N", dict(ldc=N - 4), "bad shape"),
         ("K = 0", dict(K=0), "bad shape"), ("K < 0", dict(K=-16), "bad shape"), ("M < 0", dict(M=-1), "bad shape"), ("N < 0", dict(N=-4), "bad shape"),
         ("null A", dict(A=0), "bad shape"), ("null W", dict(W=0), "bad shape"), ("null C", dict(C=0), "bad shape"),
         ("unknown epilogue 7", dict(epi=7), "unknown epilogue 7"), ("negative epilogue", dict(epi=-1), "unknown epilogue"),
         ("resid without extra", dict(epi=2, extra=0), "needs `extra` with ld >= N"), ("resid ld_extra < N", dict(epi=2, ld_extra=N - 4), "needs `extra` with ld >= N"),
         ("pe without extra", dict(epi=3, period=5, extra=0), "needs `extra` with ld >= N"), ("pe ld_extra < N", dict(epi=3, period=5, ld_extra=N - 4), "needs `extra` with ld >= N"),
         ("pe period 0", dict(epi=3, period=0), "PE epilogue needs period > 0"), ("pe period < 0", dict(epi=3, period=-3), "PE epilogue needs period > 0")]
    for what, change, frag in R:
        rc = invoke(**change)
        msg = (lib.mmdm_last_error() or b"").decode()
        assert rc == ERR_ARG, (what, rc, msg)
        assert frag in msg, (what, msg)
        assert lib.mmdm_last_gemm_kernel().decode() == "", what          # nothing was launched
    for what, change in (("M = 0", dict(M=0)), ("N = 0", dict(N=0))):
        assert invoke(**change) == OK, what
        assert lib.mmdm_last_gemm_kernel().decode() == "", what
    torch.cuda.synchronize()
    assert torch.isnan(bufs["C"]).all()
    assert invoke() == OK and lib.mmdm_last_gemm_kernel().decode() == F.expected_kernel_f32(M, N, K, "bias")      # the unchanged arguments are a valid call
    torch.cuda.synchronize()
    assert (bufs["C"].view(-1)[:M * (N + 4)].view(M, N + 4)[:, :N] == 0).all()

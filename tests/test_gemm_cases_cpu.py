"""CPU: the inputs and the reference of the low-precision GEMM edge tests (tests/gemm_cases.py) are what they claim to be.

  * exactness: on every lattice case the float64 reference survives an fp32 round trip and equals a plain fp32 evaluation in two different
    K orders -- so a correct kernel must reproduce it bit for bit, and tests/test_gpu_gemm_edges.py compares without a tolerance;
  * discrimination: on every case the wrong kernels the suite is written to catch (PE row off by one, row0 ignored, residual row clamped one
    row short, bias shifted by a quad, the last K step dropped, rows read with stride K instead of lda) change at least one output element;
  * the output encoders against hand-written values.
A mutation is applied to every case it can touch: the PE ones to PE cases, the residual one to residual cases, row0 to the case with a split
launch, and the two that need a second row (residual clamp, row stride) to M >= 2.
"""
import pytest
import torch

import gemm_cases as GC

CASES = GC.all_lattice_cases()
IDS = [f"{c.M}x{c.N}x{c.K}-{c.epi}{c.period or ''}{'-s' if c.a_scale is not None else ''}" for c in CASES]


def _ref_with(c, x=None, w=None, bias=None, extra=None, period=None, rows=None):
    xs, ws = c.scaled()
    x = xs if x is None else x
    w = ws if w is None else w
    return GC.ref_linear_f64(x, w, c.bias if bias is None else bias, c.epi, c.extra if extra is None else extra, c.period if period is None else period)


def test_the_tables_are_the_issue_s():
    assert len(set(IDS)) == len(IDS) and len(CASES) > 100
    for form in GC.FORMS:
        t = GC.TABLE[form]
        bm = t["BM"]
        assert set(t["Ms"]) == {1, 33, bm - 1, bm, bm + 1, 300}
        assert len(t["Ks"]) == 4 and t["Ks"][1] == 2 * t["Ks"][0] and t["Ks"][2] == 3 * t["Ks"][0] and t["Ks"][3] == 2048
        assert t["corner"][0] % 2 == 1 and t["corner"][2] == t["Ks"][2]
        n = sum(len(GC.exact_cases(f)) for f in GC.FORMS)
    assert n < 400, n
    M, N, K, M1 = GC.HYBRID
    assert (M + 255) // 256 * (N // 128) > 256 and M1 % 256 == 0 and M1 % GC.HYBRID_PERIOD != 0 and M - M1 == 257
    (Ma, Na, _), (Mb, Nb, _) = GC.FEW_THRESHOLD
    assert -(-Ma // 128) * (Na // 128) < 256 <= -(-Mb // 128) * (Nb // 128)
    for M, N, K in GC.FP8P:
        assert M % 128 == 0 and N % 128 == 0 and K == 1024 and (M // 128) * (N // 128) >= 512


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_lattice_reference_is_exact_in_fp32_in_any_order(c):
    assert GC.lattice_units(c.K, c.s_max) < GC.EXACT_LIMIT
    for t, den in ((c.x, 4), (c.w, 4), (c.bias, 8), (c.extra, 8)):
        if t is not None:
            assert torch.equal(t * den, (t * den).round()) and t.abs().max() <= GC.LATTICE_MAX_K / den and (t.numel() < 64 or (t == 0).float().mean() < 0.25)
    ref = c.ref()
    assert torch.equal(ref, ref.float().double())
    # no intermediate leaves the exact range: the bound of the module docstring, on the values themselves
    unit = torch.full((c.M, c.N), 2.0 ** -4, dtype=torch.float64)          # per element: 2^-(4 + s), s the element's own scale exponent
    if c.a_scale is not None:
        unit = unit * c.a_scale.double()[:, None] * c.w_scale.double()[None, :]
    assert torch.equal(ref / unit, (ref / unit).round()) and (ref.abs() / unit).max() < GC.lattice_units(c.K, c.s_max)
    xs, ws = (t.float() for t in c.scaled())
    add = c.bias.float()[None, :].expand(c.M, c.N)
    if c.epi == "resid":
        add = add + c.extra
    elif c.epi == "pe":
        add = add + c.extra[torch.arange(c.M) % c.period]
    fwd = xs @ ws.t() + add                                              # k ascending (as the BLAS blocks it), addends last
    rev = add.clone()                                                    # addends first, then 32-wide K blocks from the last to the first
    for k0 in range(c.K - 32, -1, -32):
        rev = rev + xs[:, k0:k0 + 32].flip(1) @ ws[:, k0:k0 + 32].flip(1).t()
    assert fwd.dtype == torch.float32 and rev.dtype == torch.float32
    assert torch.equal(fwd.double(), ref) and torch.equal(rev.double(), ref)
    # every operand format holds the lattice exactly (the lo plane of the split format is 0)
    for form in ("split", "bf16", "fp8"):
        assert torch.equal(GC.received(form, c.x), c.x.double()) and torch.equal(GC.received(form, c.w), c.w.double())
    assert not GC.enc_split(c.x)[1].any()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_inputs_discriminate(c):
    ref = c.ref()
    differs = lambda other: not torch.equal(other, ref)
    xs, ws = c.scaled()
    M, N, K = c.M, c.N, c.K
    if c.epi == "pe":
        rows = torch.arange(M)
        assert differs(_ref_with(c, extra=c.extra[(rows + 1) % c.period], period=M + 1)), "PE row off by one"
        if c.split_at:
            ign = torch.where(rows >= c.split_at, rows - c.split_at, rows) % c.period
            assert differs(_ref_with(c, extra=c.extra[ign], period=M + 1)), "row0 of the second launch ignored"
            # (ref_linear_f64's own row0: the second launch's rows as a problem of their own)
            tail = GC.ref_linear_f64(xs[c.split_at:], ws, c.bias, "pe", c.extra, c.period, row0=c.split_at)
            assert torch.equal(tail, ref[c.split_at:])
    if c.epi == "resid" and M >= 2:
        assert differs(_ref_with(c, extra=c.extra[torch.arange(M).clamp(max=M - 2)])), "residual row clamped to M - 2"
    assert differs(_ref_with(c, bias=c.bias[(torch.arange(N) + 4).clamp(max=N - 1)])), "bias shifted by 4 columns"
    drop = torch.cat([xs[:, :K - 32], torch.zeros(M, 32, dtype=torch.float64)], 1)
    assert differs(_ref_with(c, x=drop)), "last 32 k dropped"
    if M >= 2:
        for form in ("bf16", "fp8"):
            L = GC.layout(form, M, N, K, True)
            assert L["lda"] > K and L["ldw"] > K and L["ld_extra"] > N and L["ldc"] > N
            flat = GC.place(c.x, L["lda"], L["a_c0"], L["a_rows"], GC.A_GARBAGE).flatten()
            wrong = torch.stack([flat[L["a_c0"] + m * K:L["a_c0"] + m * K + K] for m in range(min(M, 300))]).double()
            if c.a_scale is not None:
                wrong = wrong * c.a_scale.double()[:wrong.shape[0], None]
            assert not torch.equal(GC.ref_linear_f64(wrong, ws, c.bias, "bias")[:300], GC.ref_linear_f64(xs[:300], ws, c.bias, "bias")), "rows read with stride K"


def test_saturating_case():
    c = GC.saturating_case()
    ref = c.ref()
    assert ref[1, 2] == 1024.0 and ref[3, 2] == -1024.0
    e = GC.enc_e4m3(ref.float())
    assert e.view(torch.uint8)[1, 2] == 0x7E and e.view(torch.uint8)[3, 2] == 0xFE and torch.isfinite(e.float()).all()
    assert (e.float().abs() < 448).any()                      # not everything saturates


def test_encoders_against_hand_written_values():
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    # bf16: 8 significand bits, ties to even
    got = GC.enc_bf16(f(1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -0.375, 1 + 2.0 ** -8 + 2.0 ** -20)).view(torch.int16).int() & 0xFFFF
    assert got.tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBEC0, 0x3F81]
    # e4m3: 4 significand bits, ties to even, saturating at 448 (0x7E); 0x7F would be NaN
    got = GC.enc_e4m3(f(0.25, 17.0, 19.0, 448.0, 464.0, 1024.0, -1024.0, -448.0, 0.0, 1.75, float("inf"))).view(torch.uint8)
    assert got.tolist() == [0x28, 0x58, 0x5A, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE, 0x00, 0x3E, 0x7E]
    # split planes: h = fp16(x) with ties to even, l = fp16((x - h) * 2048) carries the sign of the remainder
    p = GC.enc_split(f(1.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 0.25, 8193.0625))
    assert p[0].tolist() == [1.0, 1.0, 1 + 2.0 ** -9, 0.25, 8192.0]
    assert p[1].tolist() == [0.0, 1.0, -1.0, 0.0, 1.0625 * 2048]
    assert torch.equal(GC.bits(torch.tensor([float("nan")])), GC.bits(torch.tensor([float("nan")])))

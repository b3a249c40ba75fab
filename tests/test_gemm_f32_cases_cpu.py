"""CPU: the inputs, the layouts and the dispatch mirror of the fp32 GEMM edge tests (tests/gemm_f32_cases.py) are what they claim to be.

  * exactness: on every lattice case the float64 reference survives an fp32 round trip and equals a plain fp32 evaluation in two different
    orders of the K sum and of the addends -- so a correct kernel reproduces it bit for bit and tests/test_gpu_gemm_f32_edges.py compares
    without a tolerance;
  * discrimination: each single-fault kernel the suite is written to catch changes the reference: one A row taken from the next row, one W
    column dropped, K truncated by one, the garbage column behind a row read, the PE row off by one, the residual of a mixed launch's
    remainder taken from row 0 instead of row M1 (and, everywhere, clamped one row short), the bias shifted by one;
  * the tables: expected_kernel_f32 yields the kernel each table comment names, for every run; each threshold pair yields two kernels;
    the tables reach every kernel name the automatic dispatch can emit;
  * the layouts: every operand of every run stays inside its buffer, and each alignment kind switches exactly the condition it is named for.
"""
import itertools

import pytest
import torch

import gemm_cases as GC
import gemm_f32_cases as F

CASES = F.all_lattice_cases_f32()
IDS = [f"{c.M}x{c.N}x{c.K}-{c.epi}{c.period or ''}{'' if c.bias is not None else '-nobias'}" for c in CASES]
RUNS = F.exact_runs()


def _family(name):
    """A kernel note without the mix counts."""
    return name.split(",")[0] if name.startswith("gemm_mix") else name


def _rows(c):
    """The rows a discrimination check evaluates: both ends, the tile edges, and the two sides of a mixed launch's cut."""
    M1 = F.mix_split(c.M, c.N)
    cand = {0, 1, 31, 32, 63, 64, 127, 128, M1 - 1, M1, M1 + 1, c.M - 2, c.M - 1}
    return torch.tensor(sorted(r for r in cand if 0 <= r < c.M))


def _ref_rows(c, rows, x=None, w=None, bias=None, extra_rows=None):
    """float64 reference of the rows `rows`; `extra_rows`: the rows of `extra` they add (default: what the operation defines)."""
    x = c.x if x is None else x
    w = c.w if w is None else w
    bias = c.bias if bias is None else bias
    y = x[rows].double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if c.epi == "resid":
        y = y + c.extra.double()[rows if extra_rows is None else extra_rows]
    elif c.epi == "pe":
        y = y + c.extra.double()[(rows if extra_rows is None else extra_rows) % c.period]
    return y


def test_the_tables_are_the_issue_s():
    assert len(set(IDS)) == len(IDS) and len(CASES) > 150
    assert len(RUNS) < 400, len(RUNS)
    shapes = lambda fam, sw: {(e.M, e.N, e.K) for e in F.TABLE if e.family == fam and e.sweep == sw}
    assert {s[0] for s in shapes("fallback", "M")} == {1, 127, 128, 129} and {s[1] for s in shapes("fallback", "N")} == {1, 23, 127, 128, 129, 262}
    assert {s[2] for s in shapes("fallback", "K")} == {1, 3, 4, 15, 17, 20, 33, 100, 262, 516}
    assert {s[2] for s in shapes("glds2", "K") | shapes("glds2", "corner")} == {16, 32, 48, 64, 80}
    assert {s[0] for s in shapes("glds2", "M")} == {1, 127, 128, 129, 257} and {s[1] for s in shapes("glds2", "N")} == {4, 60, 64, 68, 132}
    assert shapes("s16", "corner") == {(1, 4, 96), (33, 132, 128), (31, 36, 2048), (129, 260, 96), (65, 516, 160)}
    assert {s[2] for s in shapes("pipe64", "K")} == {96, 112, 144, 176, 2048}
    assert {s[0] for s in shapes("pipe64", "M")} == {63, 64, 65, 129} and {s[1] for s in shapes("pipe64", "N")} == {60, 64, 68, 132}
    assert shapes("mix", "corner") == {(1025, 1024, 128), (1057, 1024, 128), (3265, 260, 128), (3300, 260, 128), (2049, 1024, 128), (1025, 2048, 128)}
    assert shapes("pipe128", "corner") == {(3969, 1028, 528), (3968, 1028, 528), (3969, 1028, 2048)}
    for c in CASES:
        assert c.K <= 2048 and GC.lattice_units(c.K) < 2 ** 24
    assert 1024 % F.MIX_PERIOD != 0
    for fam in F.FAMILY_SHAPE:
        assert any((e.M, e.N, e.K) == F.FAMILY_SHAPE[fam] for e in F.TABLE if e.family == fam)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_lattice_reference_is_exact_in_fp32_in_any_order(c):
    assert GC.lattice_units(c.K, c.s_max) < GC.EXACT_LIMIT and c.a_scale is None and c.w_scale is None
    for t, den in ((c.x, 4), (c.w, 4), (c.bias, 8), (c.extra, 8)):
        if t is not None:
            assert torch.equal(t * den, (t * den).round()) and t.abs().max() <= GC.LATTICE_MAX_K / den and (t.numel() < 64 or (t == 0).float().mean() < 0.25)
    ref = c.ref()
    assert torch.equal(ref, ref.float().double())
    assert torch.equal(ref * 16, (ref * 16).round()) and (ref.abs() * 16).max() < GC.lattice_units(c.K)
    add = c.bias[None, :].expand(c.M, c.N) if c.bias is not None else torch.zeros(c.M, c.N)
    if c.epi == "resid":
        add = add + c.extra
    elif c.epi == "pe":
        add = add + c.extra[torch.arange(c.M) % c.period]
    fwd = c.x @ c.w.t() + add                              # k ascending (as the BLAS blocks it), addends last: the scalar epilogue's order
    rev = add.clone()                                      # addends first (the 16-byte epilogue's), then K blocks of at most 32 from the last to the first, each reversed
    for k1 in range(c.K, 0, -32):
        k0 = max(k1 - 32, 0)
        rev = rev + c.x[:, k0:k1].flip(1) @ c.w[:, k0:k1].flip(1).t()
    assert fwd.dtype == torch.float32 and rev.dtype == torch.float32
    assert torch.equal(fwd.double(), ref) and torch.equal(rev.double(), ref)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_inputs_discriminate(c):
    rows = _rows(c)
    M, N, K = c.M, c.N, c.K
    ref = _ref_rows(c, rows)
    assert torch.equal(ref, c.ref()[rows])
    differs = lambda other: not torch.equal(other, ref)
    if M >= 2:
        assert differs(_ref_rows(c, rows, x=c.x.roll(-1, 0))), "A rows shifted by one"
    w = c.w.clone()
    w[N - 1] = 0
    if M * K >= 64:                                        # (a one-row problem with K = 1 may hold a zero there: one lattice entry in 17 is 0)
        assert differs(_ref_rows(c, rows, w=w)), "last W column dropped"
    x = c.x.clone()
    x[:, K - 1] = 0
    if M >= 8 or (c.x[:, K - 1].any() and c.w[:, K - 1].any()):          # a single row may hold a zero at K - 1: then nothing is lost
        assert differs(_ref_rows(c, rows, x=x)), "K truncated by one"
    L = F.layout_f32("strided", M, N, K)
    a = GC.place(c.x, L["lda"], L["a_c0"], L["a_rows"], F.A_GARBAGE)[:M, L["a_c0"]:L["a_c0"] + K + 1]
    w = GC.place(c.w, L["ldw"], L["w_c0"], N + 1, F.A_GARBAGE)[:N, L["w_c0"]:L["w_c0"] + K + 1]
    assert a.shape == (M, K + 1) and (a[:, K] == F.A_GARBAGE).all() and differs(_ref_rows(c, rows, x=a, w=w)), "the column behind the rows read"
    if c.epi == "pe":
        assert differs(_ref_rows(c, rows, extra_rows=rows + 1)), "PE row off by one"
    if c.epi == "resid":
        if M >= 2:
            assert differs(_ref_rows(c, rows, extra_rows=rows.clamp(max=M - 2))), "residual row clamped to M - 2"
        M1 = F.mix_split(M, N)
        if 0 < M1 < M:
            assert differs(_ref_rows(c, rows, extra_rows=torch.where(rows >= M1, rows - M1, rows))), "residual of the remainder taken from row 0, not row M1"
    if c.bias is not None and N >= 2:
        assert differs(_ref_rows(c, rows, bias=c.bias[(torch.arange(N) + 1).clamp(max=N - 1)])), "bias shifted by one"


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[f"{en.family}-{en.M}x{en.N}x{en.K}-{e}{p or ''}-{k}" for en, e, p, k in RUNS])
def test_mirror_yields_the_kernel_the_table_names_and_layouts_stay_in_bounds(i):
    en, e, p, kind = RUNS[i]
    L = F.layout_f32(kind, en.M, en.N, en.K)
    inplace = e == "resid_inplace"
    want = F.named_kernel(en, e, kind)
    assert "{" not in want and want == F.expected_kernel_f32(en.M, en.N, en.K, e, **F.alignment(L, True, inplace)), (en, e, kind)
    c = F.lattice_case_f32(en.M, en.N, en.K, e, p)
    for what, (end, alloc) in F.extents(L, en.M, en.N, en.K, 0 if c.extra is None or inplace else c.extra.shape[0]).items():
        assert 0 <= end <= alloc, (what, end, alloc, en, kind)
    # rows do not run into each other, the window leaves its guard rows alone
    assert L["a_c0"] + en.K <= L["lda"] and L["w_c0"] + en.K <= L["ldw"] and L["e_c0"] + en.N <= L["ld_extra"] and L["c_c0"] + en.N <= L["ldc"] and L["a_rows"] >= en.M
    if kind != "contig":
        assert L["lda"] > en.K and L["ld_extra"] > en.N and L["ldc"] > en.N and L["ldw"] > en.K


def test_each_layout_kind_switches_the_condition_it_is_named_for():
    M, N, K = 129, 132, 128
    base = dict(a_vec=True, w_vec=True, c_al=True, bias_al=True, extra_al=True)
    for kind, off in (("contig", {}), ("strided", {}), ("a_off1", {"a_vec"}), ("w_ldodd", {"w_vec"}), ("c_off1", {"c_al"}), ("bias_off1", {"bias_al"}), ("extra_ldodd", {"extra_al"})):
        al = F.alignment(F.layout_f32(kind, M, N, K))
        assert al == {k: k not in off for k in base}, (kind, al)
    al = F.alignment(F.layout_f32("c_off1", M, N, K), inplace=True)
    assert not al["c_al"] and not al["extra_al"]                                  # R aliases C: as misaligned as C
    assert F.alignment(F.layout_f32("bias_off1", M, N, K), has_bias=False)["bias_al"]
    for K in (20, 262):                                                           # "every ld larger than its width by a multiple of 4": eligibility unchanged
        s, c = F.layout_f32("strided", M, N, K), F.layout_f32("contig", M, N, K)
        assert all((s[k] - c[k]) % 4 == 0 for k in ("lda", "ldw", "ld_extra", "ldc", "a_c0", "w_c0", "e_c0", "c_c0"))
    # what the kinds do to the dispatch: the fallback for a misaligned operand, the scalar epilogue and neither s16 nor mix for a misaligned epilogue operand
    for shape in ((129, 132, 128), (1025, 1024, 128), (3969, 1028, 528)):
        for epi in ("bias", "resid", "pe"):
            k = lambda kind: F.expected_kernel_f32(*shape, epi, **F.alignment(F.layout_f32(kind, *shape)))
            assert k("contig") == k("strided") and k("a_off1") == k("w_ldodd") == "gemm_f32<22,22,16>"
            for kind in ("c_off1", "bias_off1") + (("extra_ldodd",) if epi != "bias" else ()):
                assert k(kind).startswith("gemm_pipe<") and k(kind).endswith(",scalar>"), (shape, epi, kind, k(kind))
            if epi == "bias":
                assert k("extra_ldodd") == k("strided")


def test_threshold_pairs_yield_two_kernels():
    pairs = F.threshold_pairs()
    assert len(pairs) == 9
    for a, b in pairs:
        for epi in ("bias", "resid", "resid_inplace"):
            ka, kb = (F.expected_kernel_f32(e.M, e.N, e.K, epi) for e in (a, b))
            assert ka != kb and ka == F.named_kernel(a, epi) and kb == F.named_kernel(b, epi), (a, b, epi, ka, kb)
        # one step in one dimension only
        assert sum(x != y for x, y in zip((a.M, a.N, a.K), (b.M, b.N, b.K))) == 1


def test_the_tables_reach_every_kernel_of_the_automatic_dispatch():
    reached = {_family(F.named_kernel(en, e, kind)) for en, e, p, kind in RUNS}
    assert reached == set(F.DISPATCH_FAMILIES), reached ^ set(F.DISPATCH_FAMILIES)
    # and the mirror itself emits nothing else, over a grid of shapes on both sides of each of its conditions and every alignment
    Ms = (1, 64, 65, 256, 257, 512, 513, 1025, 3969, 8065, 20000)
    Ns = (4, 132, 262, 512, 516, 1024, 2048, 4096, 16384)
    Ks = (1, 20, 32, 80, 96, 112, 128, 512, 528)
    flags = list(itertools.product((True, False), repeat=3))
    for M, N, K, epi in itertools.product(Ms, Ns, Ks, ("bias", "gelu", "resid", "pe")):
        for opnd, c_al, extra_al in flags:
            name = F.expected_kernel_f32(M, N, K, epi, a_vec=opnd, w_vec=True, c_al=c_al, bias_al=True, extra_al=extra_al)
            assert _family(name) in reached, (M, N, K, epi, name)


def test_mix_counts_are_the_launch_s():
    """n_main + n_rem of the note against the rule's own arithmetic, written out once more from the kernel's comment: rows of the whole rounds of
    256 tiles of 64 x 64, the remaining rows on 32 x 32 tiles."""
    for en in F.TABLE:
        if en.family != "mix":
            continue
        nt = -(-en.N // 64)
        M1 = F.mix_split(en.M, en.N)
        assert M1 % 64 == 0 and 0 < M1 < en.M and (M1 // 64 * nt) % 1 == 0
        n_main, n_rem = M1 // 64 * nt, -(-(en.M - M1) // 32) * -(-en.N // 32)
        assert F.named_kernel(en, "resid") == f"gemm_mix<vepi,{n_main}+{n_rem}>" and F.named_kernel(en, "bias") == f"gemm_mix<scalar,{n_main}+{n_rem}>"
        assert F.named_kernel(en, "pe") == "gemm_pipe<21,21,16,4,vepi>" and F.named_kernel(en, "resid", "c_off1") == "gemm_pipe<21,21,16,4,scalar>"
        assert n_rem <= n_main and (n_main + (en.M - M1 + 63) // 64 * nt) % 256 != 0


def test_activation_references():
    z = torch.tensor([[-3.0, -0.5, 0.0, 0.5, 3.0]], dtype=torch.float64)
    assert torch.equal(F.act_f64(z, "gelu"), GC.ref_linear_f64(z, torch.eye(5, dtype=torch.float64), None, "gelu"))
    assert torch.equal(F.act_f64(z, "silu"), GC.ref_linear_f64(z, torch.eye(5, dtype=torch.float64), None, "silu"))
    assert torch.allclose(F.act_f64(z, "sigmoid"), torch.sigmoid(z), rtol=1e-15, atol=0) and torch.allclose(F.act_f64(z, "quickgelu"), z * torch.sigmoid(1.702 * z), rtol=1e-15, atol=0)
    assert F.act_f64(z, "sigmoid")[0, 2] == 0.5 and F.act_f64(z, "quickgelu")[0, 2] == 0.0 and torch.equal(F.act_f64(z, "bias"), z)
    assert set(F.ACTS) <= set(F.EPI) and F.EPI["quickgelu"] == 5 and F.EPI["sigmoid"] == 6

"""Shapes, layouts and the dispatch rule of the fp32 GEMM edge tests (tests/test_gpu_gemm_f32_edges.py, tests/test_gemm_f32_cases_cpu.py).

mmdm_linear_f32 (csrc/gemm_f32.hip) picks a kernel from the call's shape, alignment and epilogue alone.  expected_kernel_f32 is this suite's
statement of that rule (the automatic dispatch, gemm_cfg = -1, without the row split: tail = 0): the exact mmdm_last_gemm_kernel() string of a
call; expected_plan_f32 adds the row split (tail > 0).  tests/test_gemm_f32_plan_cpu.py holds csrc/gemm_f32_plan.h to both on the CPU.  A change
of the dispatcher has to edit them knowingly.  The tables below hold, per kernel, the smallest shapes that reach it -- tile
edges in M, N and K, and both sides of every threshold -- each with the kernel its comment names (`Entry.kernel`, written out by hand: the CPU
test holds the mirror to it, the GPU test holds the library to the mirror).

Operands are gemm_cases' lattice (x, w: k / 4; bias, residual, PE: k / 8; |k| <= 8): every partial sum in any order is an integer number of
1 / 16 below 2^24 of them (lattice_units(K) = 64 K + 32, K <= 2048), so a correct fp32 kernel equals the float64 reference BIT FOR BIT whatever
its tile, chain length or order of additions.  Pure torch on the CPU: nothing here touches the library under test.
"""
import collections
import math

import torch

import gemm_cases as GC
from gemm_cases import A_GARBAGE, EXTRA_GARBAGE, GUARD, DEFAULT_PERIOD, SWEEP_EPIS, pe_periods      # noqa: F401  (re-exported to the two test modules)

EPI = dict(GC.EPI, quickgelu=5, sigmoid=6)           # include/mmdm.h: MMDM_EPI_BIAS .. MMDM_EPI_BIAS_SIGMOID
ACTS = ("gelu", "silu", "quickgelu", "sigmoid")


def act_f64(z, epi):
    """float64 activation of a pre-activation z = x w^T + b, as csrc/kernels.h states each: gelu 0.5 z (1 + erf(z / sqrt 2)), silu z / (1 + exp(-z)),
    quickgelu z * sigmoid(1.702 z) (CLIP's QuickGELU), sigmoid 1 / (1 + exp(-z))."""
    z = z.double()
    if epi == "bias":
        return z
    if epi == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if epi == "silu":
        return z / (1.0 + torch.exp(-z))
    if epi == "quickgelu":
        return z * (1.0 / (1.0 + torch.exp(-1.702 * z)))
    assert epi == "sigmoid", epi
    return 1.0 / (1.0 + torch.exp(-z))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the dispatch rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def expected_kernel_f32(M, N, K, epi, *, a_vec=True, w_vec=True, c_al=True, bias_al=True, extra_al=True):
    """mmdm_last_gemm_kernel() of mmdm_linear_f32(M, N, K, epi) under gemm_cfg = -1, tail = 0, gemm_s16 = -1.
    a_vec / w_vec: pointer 16-byte aligned and ld % 4 == 0 of A / W; c_al: the same of C; bias_al: bias null or 16-byte aligned;
    extra_al: `extra` 16-byte aligned with ld_extra % 4 == 0 (only read for resid / pe).  "resid_inplace" is resid."""
    epi = "resid" if epi == "resid_inplace" else epi
    assert epi in EPI and M > 0 and N > 0 and K > 0
    ext = epi in ("resid", "pe")
    av, wv = a_vec and K % 4 == 0, w_vec and K % 4 == 0                      # vec_ok
    glds_ok = av and wv and K % 16 == 0
    vepi_ok = N % 4 == 0 and c_al and bias_al and (not ext or extra_al)
    s16_ok = vepi_ok and K % 32 == 0
    e = "vepi" if ext and vepi_ok else "scalar"                             # launch_glds: the 16-byte epilogue only where an addend is read
    if not glds_ok:
        return "gemm_f32<22,22,16>"
    if K < 96:                                                              # too short for the pipelined loop's prologue: the 2-stage kernels
        return f"gemm_glds<22,{21 if _cdiv(M, 128) * _cdiv(N, 128) < 1000 else 22},16,2,{e}>"
    t64 = _cdiv(M, 128) * _cdiv(N, 64)
    if _cdiv(M, 64) * _cdiv(N, 64) <= 128 and not (M <= 64 and N >= 4096) and s16_ok:
        return f"gemm_s16<1,4,{'late' if ext else 'plain'}>"
    if t64 < 512 and epi != "pe" and s16_ok and vepi_ok:
        nt64 = _cdiv(N, 64)
        tiles = _cdiv(M, 64) * nt64
        rounds = tiles // 256
        mt1 = rounds * 256 // nt64
        rem_wgs = _cdiv(M - mt1 * 64, 32) * _cdiv(N, 32) if mt1 * 64 < M else 0
        if 1 <= rounds <= 2 and mt1 >= 1 and 0 < rem_wgs <= mt1 * nt64 and tiles % 256 != 0:
            return f"gemm_mix<{'vepi' if epi == 'resid' else 'scalar'},{mt1 * nt64}+{rem_wgs}>"
    if t64 < 512 or (M <= 64 and N >= 4096):
        return f"gemm_pipe<21,21,16,4,{e}>"
    if (M <= 256 and N >= 4096) or N <= 512 or K <= 512 or N == 2048:
        return f"gemm_pipe<22,21,16,4,{e}>"
    return f"gemm_pipe<22,22,16,5,{e}>"


def mix_split(M, N):
    """M1 of a mixed launch: the rows of the whole rounds of 256 64 x 64 tiles."""
    return 256 * (_cdiv(M, 64) * _cdiv(N, 64) // 256) // _cdiv(N, 64) * 64


def narrow_tile(N, K):
    """Shapes whose pipelined tile is 128 x 64 with 4 stages (768 resident slots: three workgroups per CU), not 128 x 128 with 5 (512)."""
    return N <= 512 or K <= 512 or N == 2048


def expected_plan_f32(M, N, K, epi, *, tail, a_vec=True, w_vec=True, c_al=True, bias_al=True, extra_al=True):
    """(mmdm_last_gemm_kernel(), M1) of mmdm_linear_f32(M, N, K, epi) under gemm_cfg = -1, gemm_s16 = -1 and the row-split rule `tail` (mmdm_diag_set
    "gemm_tail", or what the caller's handle set): a call whose 128-row tiles fill at least one whole round of the resident slots and leave a
    fractional round of at most tail / 10 of them runs rows [0, M1) -- the row tiles of the whole rounds -- on the large tile and the other rows
    on a smaller one, two launches whose names the note joins with "+".  Never the PE epilogue, only the pipelined kernels (K of 96 and more).  Every
    other call is the single launch of expected_kernel_f32; M1 is then the cut of a mixed launch (mix_split), else 0."""
    one = expected_kernel_f32(M, N, K, epi, a_vec=a_vec, w_vec=w_vec, c_al=c_al, bias_al=bias_al, extra_al=extra_al)
    epi = "resid" if epi == "resid_inplace" else epi
    glds_ok = a_vec and w_vec and K % 16 == 0
    if glds_ok and K >= 96 and tail and epi != "pe":
        narrow = narrow_tile(N, K)
        slots = 768 if narrow else 512
        mt, nt = _cdiv(M, 128), _cdiv(N, 64 if narrow else 128)
        tiles = mt * nt
        full = tiles // slots
        rem = tiles - full * slots
        mt1 = full * slots // nt
        if mt * _cdiv(N, 64) >= 512 and full >= 1 and 1 <= mt1 < mt and rem * 10 <= slots * tail:
            M1 = mt1 * 128
            e = "vepi" if epi == "resid" and N % 4 == 0 and c_al and bias_al and extra_al else "scalar"
            main = "22,21,16,4" if narrow else "22,22,16,5"
            # remainder: the largest tile that still gives each of the 256 CUs a workgroup
            rest = "22,21,16,4" if not narrow and _cdiv(M - M1, 128) * _cdiv(N, 64) >= 256 else "21,21,16,4"
            return f"gemm_pipe<{main},{e}>+gemm_pipe<{rest},{e}>", M1
    return one, (mix_split(M, N) if one.startswith("gemm_mix<") else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------------------------
KINDS = ("contig", "strided", "a_off1", "w_ldodd", "c_off1", "bias_off1", "extra_ldodd")


def layout_f32(kind, M, N, K):
    """Element strides and offsets of one run.  C is the window [GUARD, GUARD + M) x [c_c0, c_c0 + N) of a NaN-filled [M + 2 GUARD, ldc] buffer, A the
    columns [a_c0, a_c0 + K) of the first M rows of an [a_rows, lda] buffer of A_GARBAGE, W likewise in [N + 1, ldw], `extra` the columns
    [e_c0, e_c0 + N) of a [rows + 1, ld_extra] buffer of EXTRA_GARBAGE, bias the elements [b_off, b_off + N) of an [N + 4] buffer.
    Every kind but "contig" is the strided layout with one thing changed."""
    assert kind in KINDS, kind
    if kind == "contig":
        return dict(lda=K, a_c0=0, a_rows=M, ldw=K, w_c0=0, ld_extra=N, e_c0=0, ldc=N, c_c0=0, b_off=0)
    L = dict(lda=K + 20, a_c0=8, a_rows=M + 3, ldw=K + 12, w_c0=4, ld_extra=N + 12, e_c0=4, ldc=N + 36, c_c0=16, b_off=0)
    if kind == "a_off1":
        L["a_c0"] = 9                       # one float past a 16-byte boundary: scalar A loads
    elif kind == "w_ldodd":
        L["ldw"], L["w_c0"] = K + 1, 0      # every second row at least is misaligned: scalar W loads
    elif kind == "c_off1":
        L["c_c0"] = 17
    elif kind == "bias_off1":
        L["b_off"] = 1
    elif kind == "extra_ldodd":
        L["ld_extra"] = N + 13
    return L


def alignment(L, has_bias=True, inplace=False):
    """The keyword arguments of expected_kernel_f32 for a layout (buffers start 16-byte aligned; GUARD rows of ldc floats precede the window)."""
    c_al = (GUARD * L["ldc"] + L["c_c0"]) % 4 == 0 and L["ldc"] % 4 == 0
    return dict(a_vec=L["a_c0"] % 4 == 0 and L["lda"] % 4 == 0, w_vec=L["w_c0"] % 4 == 0 and L["ldw"] % 4 == 0, c_al=c_al,
                bias_al=not has_bias or L["b_off"] % 4 == 0, extra_al=c_al if inplace else (L["e_c0"] % 4 == 0 and L["ld_extra"] % 4 == 0))


def extents(L, M, N, K, extra_rows):
    """{operand: (one past the last element the call may touch, elements allocated)}, offsets from the buffer's start."""
    return {"A": ((M - 1) * L["lda"] + L["a_c0"] + K, L["a_rows"] * L["lda"]),
            "W": ((N - 1) * L["ldw"] + L["w_c0"] + K, (N + 1) * L["ldw"]),
            "extra": ((extra_rows - 1) * L["ld_extra"] + L["e_c0"] + N if extra_rows else 0, (extra_rows + 1) * L["ld_extra"]),
            "C": ((GUARD + M - 1) * L["ldc"] + L["c_c0"] + N, (M + 2 * GUARD) * L["ldc"]),
            "bias": (L["b_off"] + N, N + 4)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# shape tables
# ---------------------------------------------------------------------------------------------------------------------------------------
# family: the table; sweep: which epilogues run (SWEEP_EPIS; "pair": a threshold partner, as a corner); kernel: what the table's comment names,
# with {e} for the epilogue form (vepi where a residual / PE row is read through aligned 16-byte accesses, else scalar); layouts: the kinds it runs under
Entry = collections.namedtuple("Entry", "family sweep M N K kernel layouts")


def _entries(family, kernel, corners=(), Ms=(), m_at=None, Ns=(), n_at=None, Ks=(), k_at=None, layouts=("strided",), corner_layouts=("contig",)):
    out = [Entry(family, "corner", *s, kernel, tuple(layouts) + tuple(corner_layouts)) for s in corners]
    out += [Entry(family, "M", M, *m_at, kernel, tuple(layouts)) for M in Ms]
    out += [Entry(family, "N", n_at[0], N, n_at[1], kernel, tuple(layouts)) for N in Ns]
    out += [Entry(family, "K", *k_at, K, kernel, tuple(layouts)) for K in Ks]
    return out


F32, GLDS21, GLDS22 = "gemm_f32<22,22,16>", "gemm_glds<22,21,16,2,{e}>", "gemm_glds<22,22,16,2,{e}>"
S16, P2121, P2221, P2222 = "gemm_s16<1,4,{l}>", "gemm_pipe<21,21,16,4,{e}>", "gemm_pipe<22,21,16,4,{e}>", "gemm_pipe<22,22,16,5,{e}>"

TABLE = (
    # ---- register-staged fallback gemm_f32<22,22,16> (BM = BN = 128, BK = 16): K % 4 != 0 -> scalar / scalar loads; K % 4 == 0 with K % 16 != 0 -> the
    # vector / vector non-FULL variant.  The corner also under a misaligned A and an odd ldw (K = 262: both scalar already; the mixed variants are `variant`)
    _entries("fallback", F32, corners=((129, 262, 262),), corner_layouts=("contig", "a_off1", "w_ldodd"),
             Ms=(1, 127, 128, 129), m_at=(132, 20), Ns=(1, 23, 127, 128, 129, 262), n_at=(129, 20), Ks=(1, 3, 4, 15, 17, 20, 33, 100, 262, 516), k_at=(129, 132))
    # scalar A + vector W (a_off1) and vector A + scalar W (w_ldodd) need K % 4 == 0: K = 100 (seven K steps, the last of 4), K = 32 (a shape the 2-stage kernel would take)
    + [Entry("fallback", "variant", 129, 132, K, F32, ("a_off1", "w_ldodd")) for K in (100, 32)]
    # ---- 2-stage LDS-DMA gemm_glds<22,21,16,2> (128 x 64), K < 96, fewer than 1000 tiles of 128 x 128
    + _entries("glds2", GLDS21, corners=((129, 132, 80),), Ms=(1, 127, 128, 129, 257), m_at=(68, 32), Ns=(4, 60, 64, 68, 132), n_at=(129, 32), Ks=(16, 32, 48, 64, 80), k_at=(129, 132))
    # ---- 2-stage gemm_glds<22,22,16,2> (128 x 128): 32 x 32 = 1024 >= 1000 tiles | partner 31 x 32 = 992 -> <22,21>
    + [Entry("glds2big", "pair", 4000, 4000, 16, GLDS22, ("strided",)), Entry("glds2big", "pair", 3968, 4000, 16, GLDS21, ("strided",))]
    # ---- gemm_s16<1,4> (32 x 32 tiles, K step 32): at most 128 tiles of 64 x 64, K % 32 == 0, aligned quads everywhere
    + _entries("s16", S16, corners=((1, 4, 96), (33, 132, 128), (31, 36, 2048), (129, 260, 96), (65, 516, 160)), corner_layouts=())
    + [Entry("s16", "corner", 129, 260, 96, S16, ("strided", "contig", "c_off1", "bias_off1", "extra_ldodd")),     # a misaligned epilogue operand: no s16
       Entry("s16", "pair", 512, 1024, 128, S16, ("strided",)), Entry("s16", "pair", 513, 1024, 128, P2121, ("strided",)),      # 128 | 144 tiles of 64 x 64
       Entry("s16", "pair", 512, 1024, 112, P2121, ("strided",)),                                                            # K % 32 != 0
       Entry("s16", "pair", 129, 262, 96, P2121, ("strided",))]                                                              # N % 4 != 0: scalar epilogue
    # ---- gemm_pipe<21,21,16,4> (64 x 64, 4 stages): fewer than 512 tiles of 128 x 64.  The small shapes under a misaligned bias, where s16 would take them
    + _entries("pipe64", P2121, Ms=(63, 64, 65, 129), m_at=(68, 96), Ns=(60, 64, 68, 132), n_at=(65, 96), Ks=(96, 112, 144, 176, 2048), k_at=(65, 68), layouts=("bias_off1",))
    # 256 tiles: tiles % 256 == 0, not mixed | 784 tiles: three rounds, not mixed | 432 tiles, 640 rows of whole rounds and 720 > 240 remainder workgroups: not mixed
    + _entries("pipe64", P2121, corners=((1024, 1024, 128), (3073, 1024, 128), (1100, 1536, 128)), corner_layouts=())
    # ---- gemm_pipe<22,21,16,4> (128 x 64): >= 512 tiles of 128 x 64 and N <= 512 | K <= 512 | N == 2048; weight streaming: 64 < M <= 256 against N >= 4096
    + [Entry("pipe128x64", "pair", 8065, 512, 96, P2221, ("strided",)), Entry("pipe128x64", "pair", 8064, 512, 96, P2121, ("strided",)),     # 512 | 504 tiles
       Entry("pipe128x64", "corner", 3969, 1024, 96, P2221, ("strided",)),                                                              # K <= 512
       Entry("pipe128x64", "corner", 3969, 2048, 528, P2221, ("strided",)),                                                             # N == 2048
       Entry("pipe128x64", "pair", 65, 32768, 96, P2221, ("strided",)), Entry("pipe128x64", "pair", 64, 32768, 96, P2121, ("strided",)),    # M <= 64 streams on 64 x 64
       Entry("pipe128x64", "corner", 129, 16384, 96, P2221, ("strided",)),
       Entry("pipe128x64", "pair", 256, 16384, 528, P2221, ("strided",)), Entry("pipe128x64", "pair", 257, 16384, 528, P2222, ("strided",))]
    # ---- gemm_pipe<22,22,16,5> (128 x 128, 5 stages): M tail of one row, N tail of 4 columns, 33 K steps | no M tail | 128 K steps
    + [Entry("pipe128", "corner", 3969, 1028, 528, P2222, ("strided", "contig", "c_off1", "extra_ldodd")), Entry("pipe128", "corner", 3968, 1028, 528, P2222, ("strided",)),
       Entry("pipe128", "corner", 3969, 1028, 2048, P2222, ("strided",))]
    # ---- gemm_mix (whole rounds on 64 x 64 tiles + the remaining rows on 32 x 32 tiles, one launch); pe: excluded by the rule; c_off1: no 16-byte epilogue
    + [Entry("mix", "corner", M, N, 128, "gemm_mix<{m}," + counts + ">", ("strided", "c_off1")) for M, N, counts in (
        (1025, 1024, "256+32"),          # one remainder row
        (1057, 1024, "256+64"),          # the remainder crosses a 32-row tile by one row
        (3265, 260, "255+9"),            # N tail of 4 columns in both tile forms, n_main = 51 x 5; one remainder row
        (3300, 260, "255+18"),           # ... 36 remainder rows
        (2049, 1024, "512+32"),          # two rounds
        (1025, 2048, "512+64"))]         # 17 x 32 = 544 tiles: two rounds are 16 row tiles, one remainder row of 64 workgroups
)
TABLE = tuple(TABLE)
MIX_PERIOD = 299                          # 1024 % 299 != 0: a mixed launch that restarted the row index in the remainder would take the wrong PE rows

# every kernel name of the automatic dispatch (tail = 0), epilogue forms and mix counts left out
DISPATCH_FAMILIES = ("gemm_f32<22,22,16>", "gemm_glds<22,21,16,2,scalar>", "gemm_glds<22,21,16,2,vepi>", "gemm_glds<22,22,16,2,scalar>", "gemm_glds<22,22,16,2,vepi>",
                     "gemm_s16<1,4,plain>", "gemm_s16<1,4,late>", "gemm_mix<vepi", "gemm_mix<scalar",
                     "gemm_pipe<21,21,16,4,scalar>", "gemm_pipe<21,21,16,4,vepi>", "gemm_pipe<22,21,16,4,scalar>", "gemm_pipe<22,21,16,4,vepi>",
                     "gemm_pipe<22,22,16,5,scalar>", "gemm_pipe<22,22,16,5,vepi>")

# one shape per kernel family for the no-bias runs, the PE periods (one row past a tile), the in-place residuals and the activations (a tail in M, N and K each)
FAMILY_SHAPE = {"fallback": (129, 262, 262), "glds2": (129, 132, 80), "s16": (33, 132, 128), "pipe64": (65, 68, 112), "mix": (1025, 1024, 128),
                "pipe128x64": (3969, 1024, 96), "pipe128": (3969, 1028, 528)}
FAMILY_KERNEL = {"fallback": F32, "glds2": GLDS21, "s16": S16, "pipe64": P2121, "mix": "gemm_mix<{m},256+32>", "pipe128x64": P2221, "pipe128": P2222}
# one row past a tile of each family, for the PE periods (mix: a PE call is not mixed)
PE_SHAPE = {"fallback": (129, 132, 20), "glds2": (129, 68, 32), "s16": (33, 132, 128), "pipe64": (65, 68, 112), "pipe128x64": (3969, 1024, 96), "pipe128": (3969, 1028, 528)}


def named_kernel(entry, epi, kind="strided", has_bias=True):
    """The kernel the table names for a run of `entry`: its literal with the epilogue form filled in.  No threshold of the dispatcher enters here."""
    inplace, epi = epi == "resid_inplace", "resid" if epi == "resid_inplace" else epi
    ext = epi in ("resid", "pe")
    scalar = entry.N % 4 != 0 or kind == "c_off1" or (kind == "bias_off1" and has_bias) or (kind == "extra_ldodd" and ext and not inplace)
    k = entry.kernel
    if (k.startswith("gemm_mix") and (epi == "pe" or scalar)) or (k.startswith("gemm_s16") and scalar):
        k = P2121                                                   # what neither the 16 x 16 chains nor the mixed launch take goes to the 64 x 64 tiles
    return k.format(e="vepi" if ext and not scalar else "scalar", l="late" if ext else "plain", m="vepi" if epi == "resid" else "scalar")


def family_entry(family, shapes=FAMILY_SHAPE):
    M, N, K = shapes[family]
    return Entry(family, "corner", M, N, K, FAMILY_KERNEL[family], ())


def exact_runs():
    """[(entry, epi_name, period, layout kind)] of test_lattice_results_are_bit_exact, without duplicates."""
    out, seen = [], set()
    for en in TABLE:
        for kind in en.layouts:
            epis = {"pair": SWEEP_EPIS["corner"], "variant": ("bias", "resid")}.get(en.sweep) or SWEEP_EPIS[en.sweep]
            if kind in ("a_off1", "w_ldodd", "contig") and en.sweep == "corner" and en.family == "fallback":
                epis = SWEEP_EPIS["corner"]
            for e in epis:
                periods = (DEFAULT_PERIOD,) if e == "pe" else (0,)
                if e == "pe" and en.family == "mix" and kind == "strided":
                    periods = (DEFAULT_PERIOD, MIX_PERIOD)
                for p in periods:
                    key = (en.M, en.N, en.K, e, p, kind)
                    if key not in seen:
                        seen.add(key)
                        out.append((en, e, p, kind))
    return out


def lattice_case_f32(M, N, K, epi_name, period=0, has_bias=True):
    return GC.case("lattice", M, N, K, "resid" if epi_name == "resid_inplace" else epi_name, period, (False, False), has_bias)


def threshold_pairs():
    """[(entry a, entry b)]: neighbours in shape on the two sides of one dispatch condition."""
    by = {(e.M, e.N, e.K): e for e in TABLE}
    P = [((4000, 4000, 16), (3968, 4000, 16)), ((512, 1024, 128), (513, 1024, 128)), ((512, 1024, 128), (512, 1024, 112)), ((129, 260, 96), (129, 262, 96)),
         ((8065, 512, 96), (8064, 512, 96)), ((65, 32768, 96), (64, 32768, 96)), ((256, 16384, 528), (257, 16384, 528)),
         ((1025, 1024, 128), (1024, 1024, 128)), ((2049, 1024, 128), (3073, 1024, 128))]
    return [(by[a], by[b]) for a, b in P]


def all_lattice_cases_f32():
    """Every lattice Case the GPU suite runs, without duplicates."""
    seen, out = set(), []

    def add(c):
        if id(c) not in seen:
            seen.add(id(c))
            out.append(c)
    for en, e, p, _ in exact_runs():
        add(lattice_case_f32(en.M, en.N, en.K, e, p))
    for fam, (M, N, K) in FAMILY_SHAPE.items():
        add(lattice_case_f32(M, N, K, "bias", 0, has_bias=False))
        add(lattice_case_f32(M, N, K, "resid", 0, has_bias=False))
        add(lattice_case_f32(M, N, K, "resid"))
    for fam, (M, N, K) in PE_SHAPE.items():
        for p in pe_periods(M):
            add(lattice_case_f32(M, N, K, "pe", p))
    return out

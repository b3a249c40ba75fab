"""CPU: the dispatch plan of the fp32 GEMM (csrc/gemm_f32_plan.h) against its Python statements (tests/gemm_f32_cases.py).

gemm_f32_plan.h is the one place where mmdm_linear_f32 decides which kernels a call launches and on which rows: a pure function of the shape,
five alignment facts and the three switches (gemm_cfg, the row-split rule `tail`, gemm_s16).  tests/gemm_f32_plan_main.cpp wraps it in a
main() that reads calls on stdin; it is compiled once per session, host only, with the compiler build.py uses, and run as a program -- no
library is loaded into Python.  Held to it here:
  * the automatic rule (tail = 0) equals expected_kernel_f32 on a grid over both sides of every threshold, every epilogue and every single
    alignment fact off, and on every run of the hand-written tables;
  * the row split (tail = 10, and tail = 5) equals expected_plan_f32 on the same grid, and both give the hand-checked splits below;
  * the forced values: every surviving gemm_cfg names its kernel where the operands allow it and the fallback elsewhere, every value of a
    removed kernel the fallback; the forced gemm_s16 forms; gemm_s16 = 0;
  * single-fault mutations of the Python statements (one threshold each) disagree with the program somewhere on the grid: the grid sees
    each threshold.
"""
import inspect
import itertools
import os
import subprocess

import pytest

import gemm_f32_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mixermdm_amd", "csrc")

MS = (1, 63, 64, 65, 128, 129, 240, 256, 257, 1196, 3588, 8192, 8320, 19200)
NS = (4, 64, 260, 512, 516, 1024, 1028, 1536, 2048, 3072, 4096, 49152)
KS = (4, 16, 80, 96, 512, 528, 1024, 2048, 262)
FACTS = ("a_vec", "w_vec", "c_al", "bias_al", "extra_al")
ALIGNMENTS = [dict.fromkeys(FACTS, True)] + [{f: f != off for f in FACTS} for off in FACTS]
GRID = [(M, N, K, epi, al) for M, N, K, epi in itertools.product(MS, NS, KS, tuple(F.EPI)) for al in ALIGNMENTS]
ALL_ON = ALIGNMENTS[0]
FALLBACK = "gemm_f32<22,22,16>"


@pytest.fixture(scope="session")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_f32_plan") / "plan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "gemm_f32_plan_main.cpp"), "-o", exe])
    return exe


def run_plans(exe, calls, cfg=-1, tail=0, s16=-1):
    """[(names, M1, [(row0, rows)])] of the calls (M, N, K, epilogue name, alignment dict) under the three switches."""
    lines = [f"{M} {N} {K} {K} {F.EPI[epi]} {' '.join(str(int(al[f])) for f in FACTS)} {cfg} {tail} {s16}" for M, N, K, epi, al in calls]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(calls)
    res = []
    for ln in out:
        names, M1, *rows = ln.split(" ")
        res.append((names, int(M1), [tuple(int(v) for v in r.split(":")) for r in rows]))
    return res


@pytest.fixture(scope="session")
def grid_plans(plan_program):
    return {tail: run_plans(plan_program, GRID, tail=tail) for tail in (0, 10, 5)}


def test_automatic_rule_is_expected_kernel_f32(plan_program, grid_plans):
    for (M, N, K, epi, al), (names, M1, rows) in zip(GRID, grid_plans[0]):
        assert names == F.expected_kernel_f32(M, N, K, epi, **al), (M, N, K, epi, al)
        assert rows == [(0, M)] and M1 == (F.mix_split(M, N) if names.startswith("gemm_mix<") else 0), (M, N, K, epi, al, rows, M1)
    # every run of the hand-written tables, under its layout's alignment
    runs = [(en, e, kind) for en, e, p, kind in F.exact_runs()]
    calls = [(en.M, en.N, en.K, "resid" if e == "resid_inplace" else e, F.alignment(F.layout_f32(kind, en.M, en.N, en.K), True, e == "resid_inplace")) for en, e, kind in runs]
    for (en, e, kind), (names, _, _) in zip(runs, run_plans(plan_program, calls)):
        assert names == F.named_kernel(en, e, kind), (en, e, kind)
    assert {n.split(",")[0] if n.startswith("gemm_mix") else n for n, _, _ in grid_plans[0]} == set(F.DISPATCH_FAMILIES)


@pytest.mark.parametrize("tail", (10, 5))
def test_row_split_is_expected_plan_f32(grid_plans, tail):
    split = 0
    for (M, N, K, epi, al), (names, M1, rows) in zip(GRID, grid_plans[tail]):
        assert (names, M1) == F.expected_plan_f32(M, N, K, epi, tail=tail, **al), (M, N, K, epi, al)
        if names.count("gemm_") == 2:                    # (a mixed launch's name holds a "+" too)
            split += 1
            # main launch first, whole row tiles of 128, the remainder behind it; never the PE epilogue, never without the LDS-DMA kernels
            assert rows == [(0, M1), (M1, M - M1)] and 0 < M1 < M and M1 % 128 == 0 and names.count("gemm_pipe<") == 2
            assert epi != "pe" and K >= 96 and K % 16 == 0 and al["a_vec"] and al["w_vec"]
        else:
            assert rows == [(0, M)]
    assert split > 500


# (M, N, K): whole row tiles of 128 on the main kernel, out of all; main tile; remainder tile
HAND = [((12544, 3072, 1024), 85, 98, "22,22,16,5", "22,21,16,4"),
        ((12544, 1024, 1024), 64, 98, "22,22,16,5", "22,21,16,4"),
        ((12544, 2048, 1024), 96, 98, "22,21,16,4", "21,21,16,4"),
        ((12544, 512, 1024), 96, 98, "22,21,16,4", "21,21,16,4"),
        ((12500, 1024, 2048), 64, 98, "22,22,16,5", "22,21,16,4"),
        ((12544, 1028, 1024), 56, 98, "22,22,16,5", "22,21,16,4"),
        ((8320, 1024, 528), 64, 65, "22,22,16,5", "21,21,16,4"),
        ((19200, 3072, 1024), 149, 150, "22,22,16,5", "21,21,16,4"),
        ((19200, 1024, 1024), 128, 150, "22,22,16,5", "22,21,16,4")]


def test_hand_checked_row_splits(plan_program):
    for epi, e in (("bias", "scalar"), ("gelu", "scalar"), ("resid", "vepi")):
        calls = [(*shape, epi, ALL_ON) for shape, *_ in HAND]
        for (shape, main, every, big, small), (names, M1, rows) in zip(HAND, run_plans(plan_program, calls, tail=10)):
            M = shape[0]
            assert -(-M // 128) == every
            want = (f"gemm_pipe<{big},{e}>+gemm_pipe<{small},{e}>", main * 128)
            assert (names, M1) == want == F.expected_plan_f32(*shape, epi, tail=10), (shape, epi, names, M1)
            assert rows == [(0, main * 128), (main * 128, M - main * 128)]
    # the reference's B = 1 call is one launch: what tail = 0 gives; the PE epilogue is never split
    calls = [(1196, 1024, 1024, "resid", ALL_ON)] + [(*shape, "pe", ALL_ON) for shape, *_ in HAND]
    got10, got0 = run_plans(plan_program, calls, tail=10), run_plans(plan_program, calls, tail=0)
    assert got10 == got0 and all(names.count("gemm_") == 1 for names, _, _ in got10)
    assert got10[0][0] == "gemm_mix<vepi,256+192>" == F.expected_plan_f32(1196, 1024, 1024, "resid", tail=10)[0]


def test_forced_kernels(plan_program):
    forced = {11: ("gemm_glds<22,22,16,2,{e}>", 16), 17: ("gemm_glds<22,21,16,2,{e}>", 16), 34: ("gemm_pipe<22,22,16,5,{e}>", 80),
              36: ("gemm_pipe<22,21,16,4,{e}>", 64), 41: ("gemm_pipe<21,21,16,4,{e}>", 64)}
    off_a = {**ALL_ON, "a_vec": False}
    for cfg, (name, k_min) in forced.items():
        calls = [(129, 132, K, epi, al) for K in (16, 48, 64, 80, 96, 1024, 20, 262) for epi in ("bias", "resid", "pe") for al in (ALL_ON, off_a, {**ALL_ON, "c_al": False})]
        for tail in (0, 10):
            for (M, N, K, epi, al), (names, M1, rows) in zip(calls, run_plans(plan_program, calls, cfg=cfg, tail=tail, s16=14)):
                ok = al["a_vec"] and K % 16 == 0 and K >= k_min
                want = name.format(e="vepi" if epi != "bias" and al["c_al"] else "scalar") if ok else FALLBACK
                assert (names, M1, rows) == (want, 0, [(0, M)]), (cfg, M, N, K, epi, al)
    # what named a removed kernel, and any other number: the fallback tile, whatever the call
    calls = [(M, N, K, epi, ALL_ON) for M, N, K in ((129, 132, 96), (19200, 1024, 1024), (240, 1024, 1024), (129, 262, 262)) for epi in ("bias", "resid")]
    for cfg in (0, 2, 3, 4, 5, 10, 31, 32, 33, 38, 60, 61, 1, 7, -2):
        assert {names for names, _, _ in run_plans(plan_program, calls, cfg=cfg, tail=10)} == {FALLBACK}, cfg


def test_forced_small_launch_forms(plan_program):
    shapes = [(129, 260, 96), (1025, 1024, 128), (19200, 1024, 1024)]
    for s16, form in ((13, "1,3"), (14, "1,4"), (23, "2,3"), (24, "2,4")):
        for epi, l in (("bias", "plain"), ("gelu", "plain"), ("resid", "late"), ("pe", "late")):
            got = run_plans(plan_program, [(*s, epi, ALL_ON) for s in shapes], s16=s16)
            assert [n for n, _, _ in got] == [f"gemm_s16<{form},{l}>"] * 3, (s16, epi, got)
        # not where a 16-byte access is misaligned or K % 32 != 0: then the 64 x 64 / 128 x 128 tiles (no automatic s16, no mix)
        calls = [(129, 260, 96, "bias", {**ALL_ON, "bias_al": False}), (1025, 1024, 112, "bias", ALL_ON), (19200, 1024, 1024, "resid", {**ALL_ON, "extra_al": False})]
        assert [n for n, _, _ in run_plans(plan_program, calls, s16=s16)] == ["gemm_pipe<21,21,16,4,scalar>"] * 2 + ["gemm_pipe<22,22,16,5,scalar>"]
    # gemm_s16 = 0: neither the 16 x 16 chains nor the mixed launch
    calls = [(129, 260, 96, "bias", ALL_ON), (1025, 1024, 128, "resid", ALL_ON)]
    assert [n for n, _, _ in run_plans(plan_program, calls, s16=-1)] == ["gemm_s16<1,4,plain>", "gemm_mix<vepi,256+32>"]
    assert [n for n, _, _ in run_plans(plan_program, calls, s16=0)] == ["gemm_pipe<21,21,16,4,scalar>", "gemm_pipe<21,21,16,4,vepi>"]


def test_zero_padded_weight_rows(plan_program):
    """Kw > K (a K = 262 weight stored in 264 columns): 16-byte W loads in the fallback, never an LDS-DMA kernel."""
    exe = plan_program
    out = subprocess.run([exe], input="129 132 262 264 0 1 1 1 1 1 -1 0 -1\n129 132 256 264 0 1 1 1 1 1 -1 0 -1\n", capture_output=True, text=True, check=True).stdout
    assert out == f"{FALLBACK} 0 0:129\n" * 2


MUTATIONS = {"t64 <= 512": [("t64 < 512", "t64 <= 512", 2)],
             "K >= 80": [("K < 96", "K < 80", 1), ("K >= 96", "K >= 80", 1)],
             "rounds <= 3": [("1 <= rounds <= 2", "1 <= rounds <= 3", 1)],
             "rem * 10 < slots * tail": [("rem * 10 <= slots * tail", "rem * 10 < slots * tail", 1)],
             "narrow without N == 2048": [(" or N == 2048", "", 2)]}


@pytest.mark.parametrize("which", tuple(MUTATIONS))
def test_the_grid_sees_each_threshold(grid_plans, which):
    """One threshold of the Python statement moved: the program must disagree on at least one grid point.  (rem < slots always, so at
    tail = 10 `rem * 10 <= slots * tail` holds with either comparison: that threshold is visible only where rem * 10 == slots * tail, which
    tail = 5 meets at M = 19 200, N = 49 152 -- 57 600 tiles = 112 rounds of 512 + 256.)"""
    src = "\n\n".join(inspect.getsource(f) for f in (F.expected_kernel_f32, F.narrow_tile, F.expected_plan_f32))
    for old, new, count in MUTATIONS[which]:
        assert src.count(old) == count, (old, src.count(old))
        src = src.replace(old, new)
    ns = dict(vars(F))
    exec(src, ns)
    mutant = ns["expected_plan_f32"]
    caught = {tail: sum((names, M1) != mutant(M, N, K, epi, tail=tail, **al) for (M, N, K, epi, al), (names, M1, _) in zip(GRID, plans))
              for tail, plans in grid_plans.items()}
    print(which, caught)
    assert sum(caught.values()) > 0, caught
    if which == "rem * 10 < slots * tail":
        assert caught[10] == 0 and caught[5] > 0

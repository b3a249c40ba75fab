"""CPU: the inputs, float64 references and tolerance rules of tests/rowop_cases.py, proved before a GPU is involved.

  * the references are the textbook formulas (against torch's own float64 layer_norm / silu / float8 conversion);
  * the inputs are what they claim to be (lane coverage of the one-hot rows, the lane of the fp8 row maximum, |x| <= 6e4);
  * two fp32 emulations of the kernels' two-pass algorithm -- summed sequentially, and as 64 lane partials + butterfly -- stay INSIDE the fp32 bound on
    every case (the measurement behind rowop_cases.NORM_C);
  * every deliberately wrong variant (a reduction that loses a lane, a 16-lane row, a 32-lane half; unbiased variance; the other eps; scale without the
    1 +; halves swapped; wrong sequence / ss row; an fp8 scale from a partial maximum; pack with the wrong stride / column; unpack without the token skip)
    falls OUTSIDE the tolerance on at least one case.
"""
import math
import pytest
import torch
import torch.nn.functional as F

import rowop_cases as RC

MUT_DIMS = (16, 256, 260, 1028)
MUT_ROWS = ((5, 7), (5, 17))


# ---------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------
def test_references_are_the_textbook_formulas():
    x, g, b = RC.ln_case(35, 260)
    assert torch.allclose(RC.ref_layernorm(x, g, b, 1e-5), F.layer_norm(x.double(), (260,), g.double(), b.double(), 1e-5), rtol=1e-12, atol=1e-12)
    h, ss, _ = RC.adaln_case(5, 7, 260)
    idx = torch.arange(5) % RC.SS_ROWS
    ref = F.layer_norm(h.double(), (260,), eps=1e-6) * (1 + ss.double()[idx, None, :260]) + ss.double()[idx, None, 260:]
    assert torch.allclose(RC.ref_adaln(h.reshape(-1, 260), ss, 7, RC.SS_ROWS), ref.reshape(-1, 260), rtol=1e-12, atol=1e-12)
    # the ragged form is the uniform one per sequence
    rs = RC.rag_row_seq()
    hr, _ = RC.norm_rows(rs.numel(), 260, 3)
    full = RC.ref_adaln(hr, ss, 0, RC.SS_ROWS, rs)
    a = 0
    for s, n in enumerate(RC.RAG_LENS):
        assert torch.equal(full[a:a + n], RC.ref_adaln(hr[a:a + n], ss[s % RC.SS_ROWS:s % RC.SS_ROWS + 1], n, 1))
        a += n
    v = torch.linspace(-100, 100, 4001)
    assert torch.allclose(RC.ref_silu(v), F.silu(v.double()), rtol=1e-13, atol=0)
    assert torch.equal(RC.ref_mean_time(h), h.double().sum(1) / 7)


def test_split_and_e4m3_references():
    x = torch.cat([(RC.rnd(1, 4000) * 10 ** torch.linspace(-6, 4.7, 4000)).clamp(-6.0e4, 6.0e4), torch.tensor([0.0, -0.0, 6.0e4, -6.0e4, 2.0 ** -14, 2.0 ** -20])])
    pl = RC.split_f16(x)
    assert torch.isfinite(pl.float()).all()
    assert ((pl[0].double() + pl[1].double() / 2048.0 - x.double()).abs() <= RC.planes_bound(x)).all()
    # e4m3: every representable value is a fixed point, the ladder index matches the byte order, rounding is to nearest even, saturation at 448
    allb = torch.arange(256, dtype=torch.uint8)
    vals = allb.view(torch.float8_e4m3fn).float()
    ok = torch.isfinite(vals)
    assert int(ok.sum()) == 254 and vals[ok].abs().max().item() == 448.0
    assert torch.equal(RC.e4m3_rne(vals[ok]), vals[ok].double())
    assert torch.equal(RC.e4m3_index(vals[ok]), RC.byte_index(allb[ok]))
    pos = vals[ok & (allb < 128)].double().sort().values
    mid = (pos[:-1] + pos[1:]) / 2                                    # exact ties: to the even neighbour
    even = torch.where(torch.arange(mid.numel()) % 2 == 0, pos[:-1], pos[1:])
    assert torch.equal(RC.e4m3_rne(mid), even) and torch.equal(RC.e4m3_rne(-mid), -even)
    assert torch.equal(RC.e4m3_rne(torch.nextafter(mid, mid + 1)), pos[1:]) and torch.equal(RC.e4m3_rne(torch.nextafter(mid, mid - 1)), pos[:-1])
    assert RC.e4m3_rne(torch.tensor([1e9, -500.0, 464.1])).tolist() == [448.0, -448.0, 448.0]
    r = RC.rnd(2, 20000) * 10 ** torch.linspace(-4, 2.6, 20000)
    assert torch.equal(RC.e4m3_rne(r.clamp(-448, 448)), r.clamp(-448, 448).to(torch.float8_e4m3fn).double())          # torch's own fp32 -> e4m3
    # a zero row: unit scale, zero values
    q, s = RC.ref_quant_rows(torch.zeros(2, 8))
    assert torch.equal(s, torch.ones(2, dtype=torch.float64)) and not q.any()
    assert torch.equal(RC.fp8_scale_f32(torch.zeros(2, 8)), torch.ones(2))


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", RC.NORM_DIMS)
def test_inputs_are_what_they_claim(D):
    x, hot = RC.norm_rows(85, D)
    assert x.abs().max().item() <= RC.INPUT_BOUND and x[4].abs().min().item() >= 5.9e4 and not x[0].any() and (x[1] == x[1, 0]).all()
    assert abs(x[2].mean().item() - 1000) < 1 and x[3].abs().max().item() < 1e-2
    lanes = {RC.lane_of(e) for e in hot.values()}
    assert lanes == set(range(min(D // 4, 64))) and len(hot) == 64          # every active lane owns a hot element in some row
    for r, e in hot.items():
        assert e < D and x[r, e] == 1.0 and x[r].sum() == 1.0
    if D > 256:
        assert any(e >= 256 for e in hot.values())                           # and not only in the first round of slots
    x35, hot35 = RC.norm_rows(35, D)
    assert {RC.lane_of(e) for e in hot35.values()} == {l % min(D // 4, 64) for l in RC.FP8_LANES}
    assert RC.WALK_CASE["nseq"] * RC.WALK_CASE["T"] == 8197 and RC.rag_row_seq().numel() == sum(RC.RAG_LENS) + RC.RAG_PAD


@pytest.mark.parametrize("D", [256, 516])
def test_fp8_lane_case_puts_the_row_maximum_in_the_named_lane(D):
    h, ss, where = RC.fp8_lane_case(D)
    y = RC.ref_adaln(h.reshape(-1, D), ss, 2, len(RC.FP8_LANES))
    am = y.abs().argmax(-1)
    for j, lane in enumerate(RC.FP8_LANES):
        for t in range(2):
            assert int(am[2 * j + t]) == where[j] and RC.lane_of(where[j]) == lane
            second = y[2 * j + t].abs().clone()
            second[where[j]] = 0
            assert second.max().item() < 0.6 * y[2 * j + t].abs().max().item()          # by a wide margin: the scale depends on that lane alone


# ---------------------------------------------------------------------------------------------------
# the fp32 bound: what fp32 arithmetic delivers stays inside it
# ---------------------------------------------------------------------------------------------------
def _ratio(got, x, ref, gain, eps):
    """(inside, worst (|error| - a gain - r |ref|) / (2^-23 max|x| rstd gain)): the c this case needs."""
    err = (got.double() - ref).abs()
    inside = bool((err <= RC.norm_bound(x, ref, gain, eps)).all())
    _, rstd = RC.ref_normalise(x, eps)
    unit = RC.U23 * x.double().abs().amax(-1, keepdim=True) * rstd * gain
    need = (err - RC.NORM_A * gain - RC.NORM_R * ref.abs()) / unit.clamp(min=1e-300)
    return inside, max(float(need.max()), 0.0)


def test_emulations_stay_inside_the_bound():
    """The two-pass algorithm in torch fp32 under two summation orders, AdaLN and LayerNorm, every D x rows case: inside norm_bound, and the worst c
    a case needs is the NORM_C_MEASURED the constant was derived from (NORM_C = 4 x, rounded up)."""
    worst, where = 0.0, None
    for D in RC.NORM_DIMS:
        for nseq, T in RC.NORM_ROWS:
            h, ss, _ = RC.adaln_case(nseq, T, D, wide=(T == 7))
            h2 = h.reshape(-1, D)
            ref, gain = RC.ref_adaln(h2, ss, T, RC.SS_ROWS), RC.adaln_gain(ss, nseq * T, D, T, RC.SS_ROWS)
            x, g, b = RC.ln_case(nseq * T, D)
            lref = RC.ref_layernorm(x, g, b, 1e-5)
            for order in RC.SUM_ORDERS:
                for what, res in (("adaln", _ratio(RC.emulate_adaln_f32(h2, ss, T, RC.SS_ROWS, order), h2, ref, gain, RC.ADALN_EPS)),
                                  ("layernorm", _ratio(RC.emulate_layernorm_f32(x, g, b, 1e-5, order), x, lref, g.double().abs(), 1e-5))):
                    assert res[0], (what, order, D, nseq, T, res[1])
                    if res[1] > worst:
                        worst, where = res[1], (what, order, D, nseq, T)
    print(f"worst c needed by an fp32 emulation: {worst:.3f} at {where}")
    assert worst <= RC.NORM_C_MEASURED, (worst, where)
    assert worst >= 0.5 * RC.NORM_C_MEASURED, (worst, "NORM_C_MEASURED no longer describes the cases")
    assert RC.NORM_C == math.ceil(4 * RC.NORM_C_MEASURED)


def test_emulations_of_the_ragged_and_walk_cases_stay_inside_the_bound():
    rs = RC.rag_row_seq()
    for D in (16, 260):
        h, _ = RC.norm_rows(rs.numel(), D, 3)
        _, ss, _ = RC.adaln_case(len(RC.RAG_LENS), 1, D, 3)
        ref, gain = RC.ref_adaln(h, ss, 0, RC.SS_ROWS, rs), RC.adaln_gain(ss, rs.numel(), D, 0, RC.SS_ROWS, rs)
        assert _ratio(RC.emulate_adaln_f32(h, ss, 0, RC.SS_ROWS, "lanes", rs), h, ref, gain, RC.ADALN_EPS)[0]
    w = RC.WALK_CASE
    h, ss, _ = RC.adaln_case(w["nseq"], w["T"], w["D"])
    h2 = h.reshape(-1, w["D"])
    ref, gain = RC.ref_adaln(h2, ss, w["T"], RC.SS_ROWS), RC.adaln_gain(ss, h2.shape[0], w["D"], w["T"], RC.SS_ROWS)
    assert _ratio(RC.emulate_adaln_f32(h2, ss, w["T"], RC.SS_ROWS, "lanes"), h2, ref, gain, RC.ADALN_EPS)[0]


def test_sequential_fp32_time_mean_stays_inside_its_bound():
    for T in (1, 2, 300):
        for D in (4, 260):
            h = RC.rnd(T + D, 3, T, D) * 3 + 0.5
            s = torch.zeros(3, D)
            for t in range(T):
                s = s + h[:, t]
            got = s / torch.tensor(float(T))
            ref = RC.ref_mean_time(h)
            assert ((got.double() - ref).abs() <= RC.mean_time_bound(h, ref)).all(), (T, D)
            if T > 1:      # and the bound is not slack enough to hide a dropped or doubled row
                assert not (((s - h[:, T - 1]) / torch.tensor(float(T))).double() - ref).abs().le(RC.mean_time_bound(h, ref)).all()


def test_float64_quantiser_agrees_with_the_fp32_form():
    """The kernels' quantiser (fp32 scale, y * (1 / scale)) against the float64 reference quantiser of the same y: equal on > 0.9999 of the elements
    (the cap tests/test_gpu_fp8.py grants fp32-division ties), never more than one e4m3 step apart, scales equal to fp32 rounding."""
    same, total = 0, 0
    for D in (256, 260, 516):
        for h, ss, T, R in ((*RC.adaln_case(5, 7, D)[:2], 7, RC.SS_ROWS), (*RC.fp8_lane_case(D if D != 260 else 256)[:2], 2, len(RC.FP8_LANES))):
            y32 = RC.emulate_adaln_f32(h.reshape(-1, h.shape[-1]), ss, T, R, "lanes")
            q32, s32 = RC.quant_rows_f32(y32)
            q64, s64 = RC.ref_quant_rows(y32)
            assert ((s32.double() - s64).abs() <= 2.0 ** -22 * s64).all()
            d = (RC.e4m3_index(q32) - RC.e4m3_index(q64)).abs()
            assert int(d.max()) <= 1
            same, total = same + int((d == 0).sum()), total + d.numel()
            if T == 7:
                assert s32[0] == 1.0 and not q32[0].any()                        # the zero row of the zero ss row
    assert same / total > 0.9999, (same, total)


# ---------------------------------------------------------------------------------------------------
# mutation checks
# ---------------------------------------------------------------------------------------------------
def _adaln_cases():
    for D in MUT_DIMS:
        for nseq, T in MUT_ROWS:
            h, ss, _ = RC.adaln_case(nseq, T, D)
            yield h.reshape(-1, D), ss, T, nseq


@pytest.mark.parametrize("name", sorted(RC.adaln_mutants()))
def test_adaln_mutant_leaves_the_tolerance(name):
    f = RC.adaln_mutants()[name]
    caught = []
    for h, ss, T, nseq in _adaln_cases():
        ref = RC.ref_adaln(h, ss, T, RC.SS_ROWS)
        bound = RC.norm_bound(h, ref, RC.adaln_gain(ss, h.shape[0], h.shape[1], T, RC.SS_ROWS), RC.ADALN_EPS)
        caught.append(bool(((f(h, ss, T, RC.SS_ROWS, None, nseq) - ref).abs() > bound).any()))
    assert any(caught), name
    if name.startswith("drop_"):
        assert all(caught[2:]), (name, caught)        # a lost lane shows on every case that has all 64 lanes (D >= 256)


def test_a_lost_lane_is_caught_by_that_lanes_one_hot_row():
    """Finer than the above: at D = 256 / 260 / 1028 and 85 rows, dropping lane L moves the one-hot row of lane L outside the tolerance -- for each L."""
    for D in (256, 260, 1028):
        h, ss, hot = RC.adaln_case(5, 17, D)
        h2 = h.reshape(-1, D)
        ref = RC.ref_adaln(h2, ss, 17, RC.SS_ROWS)
        bound = RC.norm_bound(h2, ref, RC.adaln_gain(ss, 85, D, 17, RC.SS_ROWS), RC.ADALN_EPS)
        row_of = {RC.lane_of(e): r for r, e in hot.items()}
        for L in range(64):
            r = row_of[L]
            n = RC._normalise_dropping(h2[r:r + 1], RC.ADALN_EPS, {L})
            s = ss.double()[(r // 17) % RC.SS_ROWS]
            y = n * (1 + s[:D]) + s[D:2 * D]
            assert ((y - ref[r:r + 1]).abs() > bound[r:r + 1]).any(), (D, L)


@pytest.mark.parametrize("name", sorted(RC.layernorm_mutants()))
def test_layernorm_mutant_leaves_the_tolerance(name):
    f = RC.layernorm_mutants()[name]
    caught = []
    for D in MUT_DIMS:
        for rows in (35, 85):
            x, g, b = RC.ln_case(rows, D)
            ref = RC.ref_layernorm(x, g, b, 1e-5)
            caught.append(bool(((f(x, g, b, 1e-5) - ref).abs() > RC.norm_bound(x, ref, g.double().abs(), 1e-5)).any()))
    assert any(caught), name


@pytest.mark.parametrize("D", [256, 516])
def test_fp8_scale_from_a_partial_maximum_is_caught(D):
    """The GPU test holds row_scale BITWISE to fp8_scale_f32 of the fp32 output; a wave maximum that misses a 16-lane row changes the scale of the
    sequences whose maximum lives there (and of no other), for each of the four rows."""
    h, ss, where = RC.fp8_lane_case(D)
    y32 = RC.emulate_adaln_f32(h.reshape(-1, D), ss, 2, len(RC.FP8_LANES), "lanes")
    good = RC.fp8_scale_f32(y32)
    for r16 in range(4):
        lost = set(range(16 * r16, 16 * r16 + 16))
        bad = RC.fp8_scale_f32(y32, lanes=set(range(64)) - lost)
        hit = {j for j in range(len(RC.FP8_LANES)) if bad[2 * j] != good[2 * j] or bad[2 * j + 1] != good[2 * j + 1]}
        assert hit == {j for j, lane in enumerate(RC.FP8_LANES) if lane in lost} and hit, (r16, hit)


def test_pack_and_unpack_mutants_are_caught_and_the_maps_invert():
    c = RC.pack_case(3, 15, 128)
    ref = RC.ref_mdm_pack(c["src"], c["cond_store"], c["ldc"], c["col0"], c["time_tab"], c["step"], c["pe"])
    store = c["cond_store"]
    assert torch.equal(ref[:, 0], (store[:, 128:256] + c["time_tab"][2]) + c["pe"][0]) and torch.equal(ref[:, 1:], c["src"])
    assert not torch.equal(RC.ref_mdm_pack(c["src"], store, c["ldc"], c["col0"], c["time_tab"], c["step"], c["pe"], cond_ld=128), ref)
    assert not torch.equal(RC.ref_mdm_pack(c["src"], store, c["ldc"], c["col0"], c["time_tab"], c["step"], c["pe"], use_col0=False), ref)
    assert not torch.equal(RC.ref_mdm_pack(c["src"], store, c["ldc"], c["col0"], c["time_tab"], 0, c["pe"]), ref)
    assert torch.equal(RC.ref_mdm_unpack(ref), c["src"])
    r = RC.pack_rag_case(128)
    fr_item, fr_pos, fr_off, fr_len = r["fr"]
    tk_item, tk_pos, tk_off, tk_len = r["tk"]
    assert fr_len.tolist() == list(r["lens"]) and tk_len.tolist() == [n + 1 for n in r["lens"]] and tk_off.tolist() == [0, 2, 19]
    assert int((fr_item >= 0).sum()) == 22 and int((tk_item >= 0).sum()) == 25 and int((tk_pos[tk_item >= 0] == 0).sum()) == 3
    kw = dict(gpp=r["gpp"], fr=r["fr"], tk=r["tk"], tk_rows=r["tk_rows"])
    ref = RC.ref_mdm_pack_rag(r["src"], r["cond_store"], r["ldc"], r["time_tab"], r["step"], r["pe"], **kw)
    # group g = (CFG half g % 2, person g // 2): the four token rows of an item are four different vectors
    tok = ref[:, int(tk_off[1])]
    assert len({tuple(t.tolist()) for t in tok}) == 4
    assert torch.equal(tok[3], (r["cond_store"][1 * 3 + 1, 128:256] + r["time_tab"][3]) + r["pe"][0])
    assert not ref[:, 25:].any()
    assert not torch.equal(RC.ref_mdm_pack_rag(r["src"], r["cond_store"], r["ldc"], r["time_tab"], r["step"], r["pe"], cond_ld=128, **kw), ref)
    assert not torch.equal(RC.ref_mdm_pack_rag(r["src"], r["cond_store"], r["ldc"], r["time_tab"], r["step"], r["pe"], use_col0=False, **kw), ref)
    back = RC.ref_mdm_unpack_rag(ref, r["fr"], r["tk"], r["fr_rows"])
    assert torch.equal(back[:, :22], r["src"][:, :22]) and not back[:, 22:].any()
    assert not torch.equal(RC.ref_mdm_unpack_rag(ref, r["fr"], r["tk"], r["fr_rows"], skip=0), back)


def test_head_case_has_a_dominant_weight_in_the_named_lane():
    h, w, b, lanes = RC.head_case(5, 260, 23)
    assert len(set(lanes)) == 23 and set(RC.FP8_LANES) <= set(lanes)
    for o, lane in enumerate(lanes):
        assert int(w[o].abs().argmax()) % 64 == lane and w[o].abs().max().item() > 2.5

"""GPU: the row kernels of BOTH builds of csrc/rowops.hip against float64 (tests/rowop_cases.py holds the inputs, the references and the tolerance
rules; tests/test_rowop_cases_cpu.py proves them on the CPU).

build 0 serves fp32 handles and the stateless entry points; build 1 (no packed-fp32 instructions, DPP / v_permlane*_swap wave reductions) is what every
fp32_split / bf16 / bf16_fp8 handle runs.  Every AdaLN output mode, the ragged forms, the persistent row walk, cond SiLU, the time mean, the MDM
pack / unpack passes and the Influence head are held here at kernel level: fp32 results to the float64 bound, every other output form BITWISE to the
same build's fp32 result (bf16 cast, fp16 split, e4m3 row quantisation), index passes to exact equality.  Shapes sit on the code's seams: D on both
sides of the MAXV 1 / 2 / 4 / 8 dispatch, rows that leave a partial workgroup, 8197 rows for the second trip of a wave slot."""
import pytest
import torch

import rowop_cases as RC

pytestmark = pytest.mark.gpu

BUILDS = (0, 1)
ARG, UNSUPPORTED = 1, 4


def dev():
    return torch.device("cuda")


def inside(got, ref, bound, what):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err = (got - ref).abs()
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound; worst error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}, max error {float(err.max()):.3e}"


def check_forms_of(y, bf, pl, q, s, what):
    """The three other output forms of a build against the SAME build's fp32 rows y [rows, D]: bitwise cast / split / row scale; fp8 bytes at most one
    step from the row quantiser's.  Returns (equal bytes, bytes)."""
    from mixermdm_amd import ops
    rows, D = y.shape
    assert torch.equal(bf.reshape(rows, D), y.bfloat16()), what + ": bf16 output is not the cast of the fp32 output"
    pl = pl.reshape(2, rows, D)
    assert torch.isfinite(pl.float()).all(), what
    assert torch.equal(pl, ops.split_f32(y)) and torch.equal(pl.cpu(), RC.split_f16(y.cpu())), what + ": planes are not the split of the fp32 output"
    back = pl[0].double() + pl[1].double() / 2048.0
    assert ((back - y.double()).abs() <= RC.planes_bound(y)).all(), what
    q2, s2 = ops.quantize_rows_fp8(y)
    assert torch.equal(s, s2) and torch.equal(s.cpu(), RC.fp8_scale_f32(y.cpu())), what + ": row_scale is not max|y| / 448 of the fp32 output"
    d = (RC.byte_index(q.view(torch.uint8).reshape(rows, D).cpu()) - RC.byte_index(q2.view(torch.uint8).cpu())).abs()
    assert int(d.max()) <= 1, what + ": fp8 bytes more than one e4m3 step from the row quantiser"
    return int((d == 0).sum()), d.numel()


def adaln_all(h, ss, ss_rows, build, row_seq=None):
    from mixermdm_amd import ops
    y = ops.adaln(h, ss, ss_rows, build=build, row_seq=row_seq)
    bf = ops.adaln(h, ss, ss_rows, build=build, out="bf16", row_seq=row_seq)
    pl = ops.adaln(h, ss, ss_rows, build=build, out="planes", row_seq=row_seq)
    q, s = ops.adaln(h, ss, ss_rows, build=build, out="fp8", row_seq=row_seq)
    torch.cuda.synchronize()
    return y, bf, pl, q, s


# ---------------------------------------------------------------------------------------------------
# AdaLN
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", RC.NORM_DIMS)
@pytest.mark.parametrize("build", BUILDS)
def test_adaln_every_output_mode_vs_float64(build, D):
    """fp32 inside the float64 bound (build 1 is not expected to be bitwise build 0); bf16 within half a bf16 ulp on top of it; bf16 / planes / fp8 as
    check_forms_of; the zero row under the zero ss row gives scale 1 and zero bytes.  1, 5, 35 (nseq 5, T 7, ss a column slice: ss_ld > 2 D) and 85
    rows; ss_rows = 3."""
    same = total = 0
    for nseq, T in RC.NORM_ROWS:
        h, ss, _ = RC.adaln_case(nseq, T, D, wide=(T == 7))
        rows = nseq * T
        h2 = h.reshape(rows, D)
        ssd = RC.on_device(ss, dev())
        assert ssd.stride(0) == ss.stride(0) and (T != 7 or ssd.stride(0) > 2 * D)
        y, bf, pl, q, s = adaln_all(h.to(dev()), ssd, RC.SS_ROWS, build)
        ref = RC.ref_adaln(h2, ss, T, RC.SS_ROWS)
        bound = RC.norm_bound(h2, ref, RC.adaln_gain(ss, rows, D, T, RC.SS_ROWS), RC.ADALN_EPS)
        what = f"adaln build {build} D={D} rows={rows}"
        inside(y.reshape(rows, D), ref, bound, what)
        inside(bf.float().reshape(rows, D), ref, bound + RC.bf16_half_ulp(ref, bound), what + " bf16")
        a, b = check_forms_of(y.reshape(rows, D), bf, pl, q, s, what)
        same, total = same + a, total + b
        if rows >= 5:
            assert s[0].item() == 1.0 and not q.view(torch.uint8).reshape(rows, D)[0].any() and not y.reshape(rows, D)[0].any(), what + ": the zero row"
    assert same / total > 0.9999, (build, D, same, total)


@pytest.mark.parametrize("build", BUILDS)
def test_adaln_refuses_what_it_does_not_cover(build):
    from mixermdm_amd import ops
    from mixermdm_amd._lib import MMDMError
    for D, status in ((2052, UNSUPPORTED), (6, ARG)):
        h, ss = torch.zeros(1, 2, D, device=dev()), torch.zeros(1, 2 * D, device=dev())
        for out in ("f32", "bf16", "planes", "fp8"):
            with pytest.raises(MMDMError) as e:
                ops.adaln(h, ss, 1, build=build, out=out)
            assert e.value.status == status, (D, out)
        with pytest.raises(MMDMError) as e:
            ops.layernorm_split(h, ss[0, :D], ss[0, :D], 1e-5, build=build, planes=False)
        assert e.value.status == status
    h, ss = torch.zeros(1, 2, 8, device=dev()), torch.zeros(1, 16, device=dev())
    with pytest.raises(MMDMError, match="build must be 0 or 1") as e:
        ops.adaln(h, ss, 1, build=2, out="bf16")
    assert e.value.status == ARG


@pytest.mark.parametrize("D", [256, 516])
@pytest.mark.parametrize("build", BUILDS)
def test_adaln_fp8_row_maximum_in_every_lane_group(build, D):
    """Sequence j has its |y| maximum in lane FP8_LANES[j] (every quad, half row, 16-lane row and 32-lane half of the wave): row_scale is bitwise
    max|y| / 448 of the same build's fp32 rows -- a wave maximum that misses a lane group changes it -- and that element is the row's +-448."""
    h, ss, where = RC.fp8_lane_case(D)
    n = len(RC.FP8_LANES)
    y, bf, pl, q, s = adaln_all(h.to(dev()), ss.to(dev()), n, build)
    y2 = y.reshape(2 * n, D)
    ref = RC.ref_adaln(h.reshape(2 * n, D), ss, 2, n)
    inside(y2, ref, RC.norm_bound(h.reshape(2 * n, D), ref, RC.adaln_gain(ss, 2 * n, D, 2, n), RC.ADALN_EPS), f"fp8 lanes build {build}")
    same, total = check_forms_of(y2, bf, pl, q, s, f"fp8 lanes build {build} D={D}")
    assert same / total > 0.9999
    qb = q.view(torch.uint8).reshape(2 * n, D).cpu()
    for j in range(n):
        for t in range(2):
            assert int(y2[2 * j + t].abs().argmax()) == where[j]
            assert int(qb[2 * j + t, where[j]]) & 0x7F == 0x7E, (j, t)            # 448 = the largest finite e4m3 magnitude


@pytest.mark.parametrize("build", BUILDS)
def test_adaln_and_layernorm_walk_to_a_second_row(build):
    """8197 rows at D = 64: the grid stops at 2048 blocks of four wave slots, so rows 8192 .. 8196 are the SECOND row of wave slots 0 .. 4.  All rows
    inside the float64 bound, the last five looked at on their own; the other output forms bitwise as everywhere."""
    from mixermdm_amd import ops
    w = RC.WALK_CASE
    nseq, T, D = w["nseq"], w["T"], w["D"]
    rows = nseq * T
    h, ss, _ = RC.adaln_case(nseq, T, D)
    h2 = h.reshape(rows, D)
    y, bf, pl, q, s = adaln_all(h.to(dev()), ss.to(dev()), RC.SS_ROWS, build)
    ref = RC.ref_adaln(h2, ss, T, RC.SS_ROWS)
    bound = RC.norm_bound(h2, ref, RC.adaln_gain(ss, rows, D, T, RC.SS_ROWS), RC.ADALN_EPS)
    inside(y.reshape(rows, D)[-5:], ref[-5:], bound[-5:], f"adaln walk build {build}: rows 8192 .. 8196")
    inside(y.reshape(rows, D), ref, bound, f"adaln walk build {build}")
    same, total = check_forms_of(y.reshape(rows, D), bf, pl, q, s, f"adaln walk build {build}")
    assert same / total > 0.9999
    g, b = RC.rnd(40, D), RC.rnd(41, D)
    lref = RC.ref_layernorm(h2, g, b, 1e-5)
    lbound = RC.norm_bound(h2, lref, g.double().abs(), 1e-5)
    plain, _ = ops.layernorm_split(h2.to(dev()), g.to(dev()), b.to(dev()), 1e-5, build=build, planes=False)
    out, lpl = ops.layernorm_split(h2.to(dev()), g.to(dev()), b.to(dev()), 1e-5, build=build)
    torch.cuda.synchronize()
    inside(plain[-5:], lref[-5:], lbound[-5:], f"layernorm walk build {build}: rows 8192 .. 8196")
    inside(plain, lref, lbound, f"layernorm walk build {build}")
    assert torch.equal(out, plain) and torch.equal(lpl, ops.split_f32(plain))


@pytest.mark.parametrize("D", [16, 260, 1028])
@pytest.mark.parametrize("build", BUILDS)
def test_adaln_ragged_is_the_uniform_call_per_sequence(build, D):
    """row_seq for lengths (3, 1, 7, 2) plus three padding rows mapped to sequence 0: every output form of the ragged call is bitwise the uniform call
    on each sequence alone (its own ss row, ss_rows = 1), the padding rows are computed like rows of sequence 0, and the fp32 rows are inside the
    float64 bound."""
    rs = RC.rag_row_seq()
    rows = rs.numel()
    h, _ = RC.norm_rows(rows, D, 3)
    _, ss, _ = RC.adaln_case(len(RC.RAG_LENS), 1, D, 3)
    hd, ssd, rsd = h.to(dev()), ss.to(dev()), rs.to(dev())
    y, bf, pl, q, s = adaln_all(hd, ssd, RC.SS_ROWS, build, row_seq=rsd)
    ref = RC.ref_adaln(h, ss, 0, RC.SS_ROWS, rs)
    inside(y, ref, RC.norm_bound(h, ref, RC.adaln_gain(ss, rows, D, 0, RC.SS_ROWS, rs), RC.ADALN_EPS), f"ragged adaln build {build} D={D}")
    same, total = check_forms_of(y, bf, pl, q, s, f"ragged adaln build {build} D={D}")
    assert same / total > 0.9999
    spans, a = [], 0
    for sq, n in enumerate(RC.RAG_LENS):
        spans.append((sq, a, n))
        a += n
    spans.append((0, a, RC.RAG_PAD))
    for sq, a, n in spans:
        r = sq % RC.SS_ROWS
        u = adaln_all(hd[a:a + n].reshape(1, n, D).contiguous(), ssd[r:r + 1], 1, build)
        assert torch.equal(y[a:a + n], u[0][0]) and torch.equal(bf[a:a + n], u[1][0]), (sq, "fp32 / bf16")
        assert torch.equal(pl[:, a:a + n], u[2][:, 0]), (sq, "planes")
        assert torch.equal(q.view(torch.uint8)[a:a + n], u[3].view(torch.uint8)[0]) and torch.equal(s[a:a + n], u[4]), (sq, "fp8")


# ---------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", RC.NORM_DIMS)
@pytest.mark.parametrize("build", BUILDS)
def test_layernorm_plain_and_split_vs_float64(build, D):
    """Both builds, plain and split, against float64 -- the edge rows of rowop_cases.norm_rows, the |x| ~ 6e4 row and the one-hot row whose output is
    near 6e4 included (tests/test_gpu_mdm_split.py compares the two forms of a build with each other; this ties both to the reference)."""
    from mixermdm_amd import ops
    for rows in (1, 5, 35, 85):
        x, g, b = RC.ln_case(rows, D)
        ref = RC.ref_layernorm(x, g, b, 1e-5)
        bound = RC.norm_bound(x, ref, g.double().abs(), 1e-5)
        xd, gd, bd = x.to(dev()), g.to(dev()), b.to(dev())
        plain, _ = ops.layernorm_split(xd, gd, bd, 1e-5, build=build, planes=False)
        out, pl = ops.layernorm_split(xd, gd, bd, 1e-5, build=build)
        torch.cuda.synchronize()
        what = f"layernorm build {build} D={D} rows={rows}"
        inside(plain, ref, bound, what)
        inside(out, ref, bound, what + " (split form)")
        assert torch.equal(out, plain) and torch.isfinite(pl.float()).all(), what
        assert torch.equal(pl, ops.split_f32(plain)) and torch.equal(pl.cpu(), RC.split_f16(plain.cpu())), what
        assert ((pl[0].double() + pl[1].double() / 2048.0 - out.double()).abs() <= RC.planes_bound(out)).all(), what
        if build == 0:
            assert torch.equal(plain, ops.layernorm(xd, gd, bd, 1e-5))
        if rows >= 5 and D >= 16:
            assert out.abs().max().item() > 5.0e4          # the large output is really there


# ---------------------------------------------------------------------------------------------------
# cond SiLU
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_cond_silu_rows_and_planes(build):
    """7 x 100 elements (not a multiple of the 256-thread block), first and last step index, time + text spanning +-100; fp32 against float64 at
    tests/test_gpu_kernels.py's tolerance, the planes bitwise the split of the same build's rows, with a plane stride beyond rows * D whose gap
    keeps its sentinel."""
    from mixermdm_amd import ops
    S, rows, D, gap = 5, 7, 100, 24
    tab = RC.rnd(50, S, D)
    txt = torch.linspace(-99.0, 99.0, rows * D)[torch.randperm(rows * D, generator=torch.Generator().manual_seed(51))].reshape(rows, D).contiguous()
    for step in (0, S - 1):
        e = tab[step] + txt
        assert e.min().item() < -95 and e.max().item() > 95
        ref = RC.ref_silu(e)
        sd = torch.tensor([step], dtype=torch.int32, device=dev())
        y = ops.cond_silu(tab.to(dev()), sd, txt.to(dev()), build=build)
        buf = torch.full((2, rows * D + gap), 7.0, device=dev(), dtype=torch.float16)
        ops.cond_silu(tab.to(dev()), sd, txt.to(dev()), build=build, planes=True, out=buf)
        torch.cuda.synchronize()
        inside(y, ref, 1e-6 + 1e-5 * ref.abs(), f"cond_silu build {build} step {step}")
        assert torch.equal(buf[:, :rows * D].reshape(2, rows, D), ops.split_f32(y)), (build, step)
        assert (buf[:, rows * D:] == 7.0).all(), "the gap between the planes was written"


# ---------------------------------------------------------------------------------------------------
# time mean
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 260, 512])
@pytest.mark.parametrize("T", [1, 2, 300])
@pytest.mark.parametrize("build", BUILDS)
def test_mean_time_vs_float64(build, T, D):
    from mixermdm_amd import ops
    h = RC.rnd(60 + T, 3, T, D) * 3 + 0.5
    ref = RC.ref_mean_time(h)
    got = ops.mean_time(h.to(dev()), build=build)
    inside(got, ref, RC.mean_time_bound(h, ref), f"mean_time build {build} T={T} D={D}")


@pytest.mark.parametrize("D", [4, 260, 512])
@pytest.mark.parametrize("build", BUILDS)
def test_mean_time_ragged_is_the_uniform_call_per_sequence(build, D):
    """Lengths (1, 300, 17) at offsets that are not back to back; the rows between the sequences hold NaN, so a read outside a sequence shows."""
    from mixermdm_amd import ops
    lens, offs, rows = (1, 300, 17), (2, 5, 310), 330
    buf = torch.full((rows, D), float("nan"))
    seqs = [RC.rnd(70 + i, n, D) * 3 + 0.5 for i, n in enumerate(lens)]
    for o, x in zip(offs, seqs):
        buf[o:o + x.shape[0]] = x
    d = dev()
    got = ops.mean_time(buf.to(d), build=build, seq_off=torch.tensor(offs, dtype=torch.int32, device=d), seq_len=torch.tensor(lens, dtype=torch.int32, device=d))
    assert torch.isfinite(got).all()
    for i, x in enumerate(seqs):
        ref = RC.ref_mean_time(x[None])
        inside(got[i:i + 1], ref, RC.mean_time_bound(x[None], ref), f"ragged mean_time build {build} sequence {i}")
        assert torch.equal(got[i:i + 1], ops.mean_time(x[None].to(d), build=build)), i


def test_a_zero_length_item_never_reaches_the_ragged_kernels():
    """mean_time_rag_kernel divides by the sequence length; the lengths come from mmdm_begin_ragged alone, which refuses an item without frames."""
    from mixermdm_amd._lib import MMDMError
    from test_gpu_ragged import small, inputs
    s = small(max_batch=4, max_frames=16, single_only=True)
    try:
        s.set_schedule("ddim20")
        cond, xs = inputs((5, 3), width=262, cw=768)
        with pytest.raises(MMDMError, match=r"item 1 has 0 frames \(1 \.\. max_frames=16\)") as e:
            s.begin_ragged(cond, [xs[0], xs[1][:0]], [5, 0])
        assert e.value.status == ARG
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------
# MDM pack / unpack
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 128, 260])
@pytest.mark.parametrize("T", [1, 15, 40])
@pytest.mark.parametrize("build", BUILDS)
def test_mdm_pack_and_unpack_are_the_index_expression(build, T, D):
    """Exact equality with the torch expression ((cond + time) + pe[0] in fp32, in that order); cond is the second D columns of a wider store
    (ldc = 2 D + 4), step index 2; the planes form writes the same rows and their split."""
    from mixermdm_amd import ops
    c = RC.pack_case(3, T, D)
    ref = RC.ref_mdm_pack(c["src"], c["cond_store"], c["ldc"], c["col0"], c["time_tab"], c["step"], c["pe"])
    d = dev()
    store = c["cond_store"].to(d)
    cond = store[:, c["col0"]:c["col0"] + D]
    assert cond.stride(0) == c["ldc"]
    step = torch.tensor([c["step"]], dtype=torch.int32, device=d)
    args = (c["src"].to(d), cond, c["time_tab"].to(d), step, c["pe"].to(d))
    dst = ops.mdm_pack(*args, build=build)
    dst2, pl = ops.mdm_pack(*args, build=build, planes=True)
    back = ops.mdm_unpack(dst, build=build)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), ref), (build, T, D)
    assert torch.equal(dst2, dst) and torch.equal(pl, ops.split_f32(dst))
    assert torch.equal(back.cpu(), c["src"]) and torch.equal(back.cpu(), RC.ref_mdm_unpack(ref))


@pytest.mark.parametrize("D", [4, 128, 260])
@pytest.mark.parametrize("build", BUILDS)
def test_mdm_pack_and_unpack_ragged(build, D):
    """Lengths (1, 16, 5) in 32 frame rows / 40 token rows, four groups with two groups per person (the cond row is g % 2, the column offset g // 2);
    the row maps are built here from their definition, not by the library.  dst and the planes start as a sentinel: padding rows come back as zeros
    (planes too), the guard behind the last group keeps the sentinel; unpack(pack(x)) is x on real rows and zero on padding rows."""
    from mixermdm_amd import ops
    c = RC.pack_rag_case(D)
    d = dev()
    groups, tk_rows, fr_rows, real = c["groups"], c["tk_rows"], c["fr_rows"], sum(c["lens"])
    ref = RC.ref_mdm_pack_rag(c["src"], c["cond_store"], c["ldc"], c["time_tab"], c["step"], c["pe"], c["gpp"], c["fr"], c["tk"], tk_rows)
    fr, tk = tuple(t.to(d) for t in c["fr"]), tuple(t.to(d) for t in c["tk"])
    step = torch.tensor([c["step"]], dtype=torch.int32, device=d)
    args = (c["src"].to(d), c["cond_store"].to(d), c["time_tab"].to(d), step, c["pe"].to(d), fr, tk, tk_rows, c["gpp"])
    n = groups * tk_rows
    dst = torch.full((n + 3, D), -77.0, device=d)
    ops.mdm_pack_rag(*args, build=build, dst=dst)
    dst2 = torch.full((n + 3, D), -77.0, device=d)
    pl = torch.full((2, n * D + 16), -77.0, device=d, dtype=torch.float16)
    ops.mdm_pack_rag(*args, build=build, dst=dst2, planes=pl)
    torch.cuda.synchronize()
    assert torch.equal(dst[:n].cpu().reshape(groups, tk_rows, D), ref), (build, D)
    assert (dst[n:] == -77.0).all() and (dst2[n:] == -77.0).all() and (pl[:, n * D:] == -77.0).all(), "written behind the last group"
    assert torch.equal(dst2, dst) and torch.equal(pl[:, :n * D].reshape(2, n, D), ops.split_f32(dst[:n]))
    pad = (c["tk"][0] < 0).to(d)
    assert int(pad.sum()) == tk_rows - real - len(c["lens"])
    assert not dst[:n].reshape(groups, tk_rows, D)[:, pad].any() and not pl[:, :n * D].reshape(2, groups, tk_rows, D)[:, :, pad].any()
    back = torch.full((groups * fr_rows + 3, D), -77.0, device=d)
    ops.mdm_unpack_rag(dst[:n].reshape(groups, tk_rows, D), fr, tk, fr_rows, build=build, dst=back)
    torch.cuda.synchronize()
    b3 = back[:groups * fr_rows].cpu().reshape(groups, fr_rows, D)
    assert torch.equal(b3, RC.ref_mdm_unpack_rag(ref, c["fr"], c["tk"], fr_rows))
    assert torch.equal(b3[:, :real], c["src"][:, :real]) and not b3[:, real:].any() and (back[groups * fr_rows:] == -77.0).all()


# ---------------------------------------------------------------------------------------------------
# Influence head (build 0 only: it exists there only)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [1, 23])
def test_influence_head_with_a_dominant_weight_per_lane(nw):
    from mixermdm_amd import ops
    h, w, b, _ = RC.head_case(5, 260, nw)
    ref = torch.sigmoid(h.double() @ w.double().T + b.double())
    got = ops.influence_head(h.to(dev()), w.to(dev()), b.to(dev()))
    inside(got, ref, 2e-6 + 1e-5 * ref.abs(), f"influence_head nw={nw}")


def test_influence_head_refuses_24_outputs():
    from mixermdm_amd import ops
    from mixermdm_amd._lib import MMDMError
    h, w, b, _ = RC.head_case(5, 260, 24)
    with pytest.raises(MMDMError) as e:
        ops.influence_head(h.to(dev()), w.to(dev()), b.to(dev()))
    assert e.value.status == ARG

"""GPU: the geometry, blend and DDIM-update kernels (mixermdm_amd/csrc/geometry.hip) at their branch points, on the constructed inputs of
tests/geometry_cases.py against float64 references.  Every bound is three times a reference-side measurement that tests/test_geometry_cases_cpu.py
proves on the CPU; there is no fraction-of-elements or hard-bound allowance, and nothing is skipped at run time.

Every output is written into a view of a sentinel-filled arena (rows before and after), through the same C entry points the ops wrappers call; nothing
outside the view may change.  The wrappers themselves are held bitwise to those calls.
"""
import numpy as np
import pytest
import torch

import geometry_cases as GC

pytestmark = pytest.mark.gpu

F64 = torch.float64
PAD = 1024


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Arena:
    """Output tensors as views into sentinel-filled buffers; check() asserts that nothing outside a view was written."""

    def __init__(self):
        self.bufs = []

    def new(self, *shape, init=None, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), GC.SENTINEL, device=dev(), dtype=dtype)
        v = buf[PAD:PAD + n].view(*shape)
        if init is not None:
            v.copy_(init)
        self.bufs.append((buf, n))
        return v

    def check(self):
        for buf, n in self.bufs:
            assert (buf[:PAD] == GC.SENTINEL).all() and (buf[PAD + n:] == GC.SENTINEL).all(), "a kernel wrote outside its output"


def _lib():
    from mixermdm_amd._lib import load_library, check
    from mixermdm_amd.ops import _p, _stream
    return load_library(), check, _p, _stream


def mixer_pre(o1, o2, stats, align, last=None):
    """mmdm_mixer_pre_f32 / _masked_f32 into arena views -> (out1, out2) on the CPU."""
    lib, check, _p, _stream = _lib()
    n, T, _ = o1.shape
    ar = Arena()
    a, c, st = o1.to(dev()).contiguous(), o2.to(dev()).contiguous(), stats.to(dev())
    y1, y2 = ar.new(n, T, GC.NF2), ar.new(n, T, GC.NF2)
    if last is None:
        check(lib.mmdm_mixer_pre_f32(_p(a), _p(c), _p(st), _p(y1), _p(y2), n, T, int(align), _stream()))
    else:
        lf = torch.tensor(last, dtype=torch.int32, device=dev())
        check(lib.mmdm_mixer_pre_masked_f32(_p(a), _p(c), _p(st), _p(y1), _p(y2), n, T, int(align), _p(lf), len(last), _stream()))
    torch.cuda.synchronize()
    ar.check()
    return y1.cpu(), y2.cpu()


def xstart_ddim(m, stats, coef, i, x, x2, align):
    """mmdm_xstart_ddim_f32 with x, x2, both pred_xstart and the floor workspace in arena views -> (x, x2, p1, p2) on the CPU."""
    lib, check, _p, _stream = _lib()
    B, T, _ = m.shape
    ar = Arena()
    xd, x2d, p1, p2, ws = ar.new(B, T, GC.NF2, init=x), ar.new(B, T, GC.NF2, init=x2), ar.new(B, T, GC.NF2), ar.new(B, T, GC.NF2), ar.new(2 * B)
    step = torch.tensor([i], dtype=torch.int32, device=dev())
    md, st = m.to(dev()).contiguous(), stats.to(dev())      # (named: a temporary would be freed, and its block reused, before the launch)
    check(lib.mmdm_xstart_ddim_f32(_p(md), _p(st), _p(coef), coef.shape[1], _p(step), _p(xd), _p(x2d), _p(p1), _p(p2), _p(ws), B, T, int(align), _stream()))
    torch.cuda.synchronize()
    ar.check()
    return xd.cpu(), x2d.cpu(), p1.cpu(), p2.cpu()


def center_motion(m, npers):
    from mixermdm_amd import ops
    ar = Arena()
    out = ar.new(*m.shape)
    ops.center_motion(m.to(dev()), npers=npers, out=out)
    torch.cuda.synchronize()
    ar.check()
    return out.cpu()


@pytest.fixture(scope="module")
def coef():
    return torch.from_numpy(GC.ddim_coef()).to(dev())


def within(got, ref, bound, what):
    got = got.double()
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err = (got - ref).abs()
    bad = GC.outside(got, ref, bound)
    ratio = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, largest err / bound {ratio:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside their bound, largest err / bound {ratio:.3f}, max err {err.max().item():.3e}"


# ---------------------------------------------------------------------------------------------------
# 1. the rotation round trip
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rot():
    mo = GC.rot_motion()
    d6 = GC.rot_d6()
    return dict(one=mo, two=torch.cat([mo, mo], -1), ref=GC.gram_schmidt(d6.double()),
                listed=GC.rot_listed(d6), bound=GC.rot_bound(d6))


def check_rot(got, rot, what):
    """got [3, T, 262] (one person): finite everywhere, every listed joint inside its bound."""
    assert torch.isfinite(got).all(), what + ": non-finite output (the degenerate pairs of sample 2 included)"
    g = got[..., GC.ROT0:GC.FEET0].reshape(3, GC.ROT_T, 21, 6).double()
    L = rot["listed"]
    within(g[L], rot["ref"][L], rot["bound"][L][:, None], what)


def test_roundtrip_in_mixer_pre(rot):
    from mixermdm_amd import ops
    m, ident = rot["two"], GC.ident_stats()
    o1 = m.clone()
    o1[..., :132] += 0.25                                   # another root, so that the alignment has something to do
    o1[..., 262:262 + 132] -= 0.5
    y1, y2 = mixer_pre(o1, m, ident, True)
    for p in range(2):
        check_rot(y1[..., p * 262:(p + 1) * 262], rot, f"mixer_pre individual stream, person {p}")
        check_rot(y2[..., p * 262:(p + 1) * 262], rot, f"mixer_pre interaction stream, person {p}")
        # the moved stream's feet are the zero hand padding, the interaction stream's are the input's
        assert (y1[..., p * 262 + 258:(p + 1) * 262] == 0).all() and torch.equal(y2[..., p * 262 + 258:(p + 1) * 262], m[..., p * 262 + 258:(p + 1) * 262])
    assert torch.equal(y2[..., :132], m[..., :132])          # positions / velocities of the interaction stream pass through
    w1, w2 = ops.mixer_pre(o1.to(dev()), m.to(dev()), ident.to(dev()), True)
    assert torch.equal(w1.cpu(), y1) and torch.equal(w2.cpu(), y2)
    # align = False: everything is the denormalised input, bit for bit
    n1, n2 = mixer_pre(o1, m, ident, False)
    assert torch.equal(n1, o1) and torch.equal(n2, m)


def test_roundtrip_in_xstart_ddim(rot, coef):
    from mixermdm_amd import ops
    m, ident = rot["two"], GC.ident_stats()
    x, x2 = GC.rnd(1, *m.shape), GC.rnd(2, *m.shape)
    xd, x2d, p1, p2 = xstart_ddim(m, ident, coef, 17, x, x2, True)
    for p in range(2):
        check_rot(p1[..., p * 262:(p + 1) * 262], rot, f"xstart_ddim pred_xstart, person {p}")
        assert (p1[..., p * 262 + 258:(p + 1) * 262] == 0).all()
    assert torch.equal(p2, m) and torch.isfinite(xd).all() and torch.isfinite(x2d).all()
    a, b = x.to(dev()), x2.to(dev())
    q1, q2 = ops.xstart_ddim(m.to(dev()), ident.to(dev()), coef, torch.tensor([17], dtype=torch.int32, device=dev()), a, b, True)
    assert torch.equal(q1.cpu(), p1) and torch.equal(q2.cpu(), p2) and torch.equal(a.cpu(), xd) and torch.equal(b.cpu(), x2d)
    # align = False at i > 0: both predictions are the (identity-)normalised input
    _, _, n1, n2 = xstart_ddim(m, ident, coef, 17, x, x2, False)
    assert torch.equal(n1, m) and torch.equal(n2, m)


@pytest.mark.parametrize("npers", [1, 2])
def test_roundtrip_in_center_motion(rot, npers):
    got = center_motion(rot["one"] if npers == 1 else rot["two"], npers)
    for p in range(npers):
        check_rot(got[..., p * 262:(p + 1) * 262], rot, f"center_motion npers={npers}, person {p}")
        assert (got[..., p * 262 + 258:(p + 1) * 262] == 0).all()


# ---------------------------------------------------------------------------------------------------
# 2. alignment and centring
# ---------------------------------------------------------------------------------------------------
def check_posvel(got, ref32, ref64, reach, what, keep=None):
    """got [slots, T, 262]: positions and velocities per (sample, person) slot within max(3 E32, 2e-6 max(1, reach))."""
    assert torch.isfinite(got).all(), what + ": non-finite output"
    bound, _ = GC.posvel_bound(ref32, ref64, reach)
    g, r, b = got[..., :132].double(), ref64, bound[:, None, None].expand_as(ref64)
    if keep is not None:
        g, r, b = g[keep], r[keep], b[keep]
    within(g, r, b, what)


@pytest.mark.parametrize("T", [GC.ALIGN_T, 1])
def test_alignment(T):
    tg, mv = GC.align_inputs(T)
    r64, reach = GC.align_ref(tg.double(), mv.double())
    r32, _ = GC.align_ref(tg, mv)
    ident = GC.ident_stats()
    for h in range(2):                                      # two calls of n = 4
        s = slice(8 * h, 8 * h + 8)
        y1, y2 = mixer_pre(GC.pack_persons(mv[s]), GC.pack_persons(tg[s]), ident, True)
        check_posvel(GC.unpack_persons(y1), r32[s], r64[s], reach[s], f"align T={T} cases {GC.ALIGN_CASES[s]}")
        assert torch.equal(GC.unpack_persons(y2)[..., :132], tg[s][..., :132])


def test_last_frame():
    tg, mv = GC.last_inputs()
    ident = GC.ident_stats()
    o1, o2 = GC.pack_persons(mv), GC.pack_persons(tg)
    plain, _ = mixer_pre(o1, o2, ident, True)
    for last in GC.LAST_SETS:
        r64, reach = GC.align_ref(tg.double(), mv.double(), last, 2)          # a last frame belongs to the sample: both persons of sample b use last[b % rows]
        r32, _ = GC.align_ref(tg, mv, last, 2)
        y1, _ = mixer_pre(o1, o2, ident, True, last)
        check_posvel(GC.unpack_persons(y1), r32, r64, reach, f"last_frame {last}")
    for last in GC.LAST_FULL:
        y1, y2 = mixer_pre(o1, o2, ident, True, last)
        assert torch.equal(y1, plain), last


@pytest.mark.parametrize("B,T,first", GC.CENTER_CALLS)
def test_centring(B, T, first, coef):
    m, idx = GC.center_inputs(B, T, first)
    r64, _, reach = GC.center_ref(m.double())
    r32 = GC.center_ref(m)[0]
    keep = torch.tensor([c != GC.CENTER_FINITE_ONLY for c in idx])
    packed = GC.pack_persons(m)
    _, _, p1, p2 = xstart_ddim(packed, GC.ident_stats(), coef, 17, GC.rnd(3, B, T, 524), GC.rnd(4, B, T, 524), True)
    check_posvel(GC.unpack_persons(p1), r32, r64, reach, f"xstart_ddim centring B={B} T={T}", keep)
    assert torch.equal(p2, packed)
    c2 = center_motion(packed, 2)
    check_posvel(GC.unpack_persons(c2), r32, r64, reach, f"center_motion npers=2 B={B} T={T}", keep)
    c1 = center_motion(m[:min(2 * B, 4)], 1)
    check_posvel(c1, r32[:4], r64[:4], reach[:4], f"center_motion npers=1 B={min(2 * B, 4)} T={T}", keep[:4])
    assert torch.equal(c1, GC.unpack_persons(c2)[:4])


@pytest.mark.parametrize("T", GC.FLOOR_T)
def test_floor_reduction(T, coef):
    m, el = GC.floor_inputs(T)
    want = m[..., 1:66:3] - GC.FLOOR_MIN                    # exact: every Y is a multiple of 0.25
    for a in range(0, m.shape[0], 8):                       # calls of at most B = 4
        s = slice(a, min(a + 8, m.shape[0]))
        packed = GC.pack_persons(m[s])
        B = packed.shape[0]
        _, _, p1, _ = xstart_ddim(packed, GC.ident_stats(), coef, 1, GC.rnd(5, B, T, 524), GC.rnd(6, B, T, 524), True)
        got = GC.unpack_persons(p1)[..., 1:66:3]
        assert torch.equal(got, want[s]), (T, "floor_kernel: minimum at elements", el[s], (got - want[s]).abs().amax(dim=(1, 2)).tolist())
        got = GC.unpack_persons(center_motion(packed, 2))[..., 1:66:3]
        assert torch.equal(got, want[s]), (T, "center_floor_kernel npers=2: minimum at elements", el[s], (got - want[s]).abs().amax(dim=(1, 2)).tolist())
        for b in range(0, s.stop - s.start, 4):
            got = center_motion(m[s][b:b + 4], 1)[..., 1:66:3]
            assert torch.equal(got, want[s][b:b + 4]), (T, "center_floor_kernel npers=1")


# ---------------------------------------------------------------------------------------------------
# 3. the updates
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", GC.UPDATE_STEPS)
def test_two_chain_update_without_geometry(i, coef):
    """Normalisation by synthetic_stats(3) and the update, no geometry: x, x2 and both pred_xstart against float64 with the fp32 table values."""
    st, co = GC.synth_stats(), GC.ddim_coef()
    m, x, x2 = GC.update_inputs()
    rx, rx2, rp1, rp2 = GC.update_ref(m, x, x2, st, i, co)
    gx, gx2, p1, p2 = xstart_ddim(m, st, coef, i, x, x2, False)
    c = GC.coef_at(co, i, F64)
    within(p1, rp1, GC.K_PX * GC.U * rp1.abs(), f"i={i} pred_xstart")
    within(p2, rp2, GC.K_PX * GC.U * rp2.abs(), f"i={i} pred_xstart2")
    within(gx, rx, GC.ddim_bound(GC.K_XSTART, x, rp1.abs(), c), f"i={i} x")
    within(gx2, rx2, GC.ddim_bound(GC.K_XSTART, x2, rp2.abs(), c), f"i={i} x2")


def test_mixer_pre_denormalisation():
    """mixer_pre with align = False on synthetic_stats(3): o * std + mean of both streams, every channel, and nothing else."""
    st = GC.synth_stats()
    o1, o2, _ = GC.update_inputs()
    y1, y2 = mixer_pre(o1, o2, st, False)
    for got, o, row, what in ((y1, o1, 0, "out1"), (y2, o2, 2, "out2")):
        ref, unit = GC.denorm_ref(o, st[row * 262:(row + 1) * 262], st[(row + 1) * 262:(row + 2) * 262])
        within(got, ref, GC.K_DENORM * GC.U * unit, "denormalised " + what)


def run_chain(kind, ms, x, i, coef, pred):
    """One single-chain update with x (and pred_xstart) in arena views -> (x, pred_xstart or None) on the CPU."""
    from mixermdm_amd import ops
    lib, check, _p, _stream = _lib()
    ar = Arena()
    xd = ar.new(*x.shape, init=x)
    p = ar.new(*x.shape) if pred else None
    step = torch.tensor([i], dtype=torch.int32, device=dev())
    md = [m.to(dev()) for m in ms]
    if kind == "cfg":
        B, T, C = x.shape
        check(lib.mmdm_cfg_ddim_f32(_p(md[0]), _p(coef), coef.shape[1], _p(step), float(GC.CFG_SCALE), _p(xd), _p(p), B, T, C, _stream()))
    elif kind == "cfg4":
        assert ops.cfg4_ddim(md[0], coef, step, *GC.CFG4_SCALES, xd, pred_xstart=p) is p
    else:
        assert ops.dual_ddim(md[0], md[1], coef, step, GC.dual_w_table().to(dev()), *GC.DUAL_SCALES, xd, pred_xstart=p) is p
    torch.cuda.synchronize()
    ar.check()
    return xd.cpu(), None if p is None else p.cpu()


@pytest.mark.parametrize("C", [262, 524])
@pytest.mark.parametrize("kind", ["cfg", "cfg4", "dual"])
def test_single_chain_updates(kind, C, coef):
    from mixermdm_amd import ops
    co = GC.ddim_coef()
    for B, T in GC.CHAIN_SHAPES:
        for i in GC.CHAIN_STEPS:
            ms, x, x0, xr, b0, bx = GC.chain_case(kind, B, T, C, i, co)
            gx, gp = run_chain(kind, ms, x, i, coef, True)
            what = f"{kind} C={C} B={B} T={T} i={i}"
            within(gp, x0, b0, what + " pred_xstart")
            within(gx, xr, bx, what + " x")
            nx, none = run_chain(kind, ms, x, i, coef, False)
            assert none is None and torch.equal(nx, gx), what + ": x differs when pred_xstart is not asked for"
    # the wrappers' default (a new pred_xstart tensor) is the same call
    ms, x, x0, xr, b0, bx = GC.chain_case(kind, 3, 7, C, 17, co)
    gx, gp = run_chain(kind, ms, x, 17, coef, True)
    xd, step, md = x.to(dev()), torch.tensor([17], dtype=torch.int32, device=dev()), [m.to(dev()) for m in ms]
    if kind == "cfg":
        p = ops.cfg_ddim(md[0], coef, step, GC.CFG_SCALE, xd)
    elif kind == "cfg4":
        p = ops.cfg4_ddim(md[0], coef, step, *GC.CFG4_SCALES, xd)
    else:
        p = ops.dual_ddim(md[0], md[1], coef, step, GC.dual_w_table().to(dev()), *GC.DUAL_SCALES, xd)
    assert torch.equal(p.cpu(), gp) and torch.equal(xd.cpu(), gx)


# ---------------------------------------------------------------------------------------------------
# 4. the generator's tails
# ---------------------------------------------------------------------------------------------------
def test_generator_tails():
    """The draws at u1 -> 0, u1 -> 1 and at the 2^23 branch between logf and log1pf: the radius is held relatively (the suite's atol of 1e-5 is 3 % of it
    near u1 = 1), the cosine by its argument's error."""
    from mixermdm_amd import ops
    count = {}
    for lp in GC.TAIL_LPS:
        z = ops.randn(GC.TAIL_SEED, lp, GC.TAIL_B, GC.TAIL_T).cpu().numpy().ravel().astype(np.float64)
        assert np.isfinite(z).all()
        a, g = GC.fill_draws(lp)
        for grp, idx in GC.tail_groups(a).items():
            count[grp] = count.get(grp, 0) + len(idx)
            ref, radius, u2 = GC.normal_f64(a[idx], g[idx])
            err, bound = np.abs(z[idx] - ref), GC.normal_bound(ref, radius, u2)
            if len(idx):
                print(f"lp={lp} {grp}: {len(idx)} draws, largest err / bound {(err / bound).max():.3f}, largest relative err {(err / np.abs(ref)).max():.3e}")
            assert (err <= bound).all(), (lp, grp, a[idx][err > bound], (err / bound).max())
    assert min(count.values()) >= 4, count

"""CPU: the inputs, float64 references, membership rules, bounds and mutants of tests/geometry_cases.py, proved before a GPU is involved.

  * the references are the oracle's: the switchable restatements with no switch thrown equal oracle.geometry value for value, and the float64 oracle
    round trip equals plain Gram-Schmidt on every listed joint (which licenses the simpler reference);
  * every listed case meets its membership rule;
  * the fp32 restatements (oracle.geometry in fp32, fp32 torch / numpy restatements of the updates and the generator) sit at a third of every bound or
    less: each recorded constant is at least FACTOR x the measured one (and at most 4 x, so none has drifted wide);
  * every deliberately wrong float64 variant falls outside a bound on at least one listed case -- or, for the two equivalent ones, is proved equivalent;
  * the generator's tail draws exist in the stated numbers.
"""
import math
import numpy as np
import pytest
import torch

import geometry_cases as GC
from oracle import geometry as G
from parity_tol import CLIFF_MARGIN, YARD_FACTOR
from test_sampler_opts_cpu import step_normal_f64

F64 = torch.float64


def recorded(name, const, measured):
    print(f"{name}: measured {measured:.4g}, recorded {const:.4g} ({const / measured:.2f} x)")
    assert GC.FACTOR * measured <= const <= 4.0 * measured, (name, measured, const)


def test_factor_is_the_projects():
    assert GC.FACTOR == YARD_FACTOR == 3.0


# ---------------------------------------------------------------------------------------------------
# 1. rotation round trip
# ---------------------------------------------------------------------------------------------------
def test_rot_inputs_are_what_they_claim():
    ax, d6 = GC.axes(), GC.rot_d6()
    assert ax.shape == (21, 3) and torch.allclose(ax.norm(dim=-1), torch.ones(21, dtype=F64), atol=1e-15)
    assert d6.shape == (3, GC.ROT_T, 21, 6) and d6.dtype == torch.float32 and GC.ROT_T == 14
    assert GC.ANGLES[1] < 1e-6 < GC.ANGLES[2]                              # one angle inside the small-angle branch
    m = G.rotation_6d_to_matrix(d6[0].double())
    eye = torch.eye(3, dtype=F64)
    assert (m @ m.transpose(-1, -2) - eye).abs().max() < 3e-7             # sample 0 is orthonormal to fp32 rounding
    assert torch.equal(m[0], eye.expand(21, 3, 3))                         # angle 0: the identity, exactly
    # the half turn about the coordinate axes is exact: a diagonal of +-1
    assert torch.equal(m[-1, :6].abs(), eye.expand(6, 3, 3)) and (m[-1, :6].diagonal(dim1=-2, dim2=-1).sum(-1) == -1).all()
    # sample 1 is the same rotation after Gram-Schmidt; sample 2 is degenerate
    assert (GC.gram_schmidt(d6[1].double()) - GC.gram_schmidt(d6[0].double())).abs().max() < 3e-7
    a1, a2 = d6[2][..., [0, 2, 4]], d6[2][..., [1, 3, 5]]
    assert (a1[0::3] == 0).all() and (a2[0::3] != 0).any() and torch.equal(a2[1::3], 2 * a1[1::3]) and (d6[2][2::3] == 0).all()
    mo = GC.rot_motion()
    assert torch.equal(mo[..., GC.ROT0:GC.FEET0].reshape(3, GC.ROT_T, 21, 6), d6) and (mo[..., GC.FEET0:] != 0).all()


def test_roundtrip_restatement_is_the_oracles_and_equals_gram_schmidt():
    mo = GC.rot_motion()
    for dt in (torch.float32, F64):
        got = GC.roundtrip(mo[:2, :, GC.ROT0:GC.FEET0].reshape(2, GC.ROT_T, 21, 6).to(dt))
        ora = G.smpl_to_ih(G.ih_to_smpl(mo[:2].to(dt)))[..., GC.ROT0:GC.FEET0].reshape(2, GC.ROT_T, 21, 6)
        assert torch.equal(got, ora), dt
    d6, listed = GC.rot_d6(), GC.rot_listed()
    gap = (GC.roundtrip(d6.double()) - GC.gram_schmidt(d6.double())).abs().amax(-1)
    print("float64 oracle round trip vs Gram-Schmidt on the listed joints: max %.3e" % gap[listed].max())
    assert gap[listed].max() <= 1e-7


def test_rot_membership():
    d6, listed = GC.rot_d6(), GC.rot_listed()
    _, sd = GC.rot_conditioning(d6)
    big = sd.abs().amax(-1)
    assert (((big == 0) | (big > CLIFF_MARGIN))[listed]).all() and not listed[2].any()
    n = listed[:2].sum(-1)                      # per (sample, frame)
    print("listed joints per angle:", n.tolist())
    assert (listed[0, 0] & listed[1, 0]).all()                                  # angle 0: every joint (exact identity)
    assert (n[:, 3:13] == 21).all()                                             # 1e-4 ... pi - 1e-3: every joint clears the margin
    assert (n[:, 1:3] == 0).all()                                               # 1e-7, 1e-5: below the margin on every axis -> finiteness only
    # the half turn: the six coordinate axes and (1, 1, 0) / sqrt 2 are exact and consistent; (1, 0, -1) / sqrt 2 is exact but NOT recoverable
    assert listed[0, -1, :7].all() and not listed[0, -1, 7] and (big[0, -1, 7] == 0)
    q, _ = GC.rot_conditioning(d6)
    assert (q[listed] == 0).sum() >= 100 and ((q[listed] > 0) & (q[listed] < 1e-3)).sum() >= 20     # both arms of the bound are in use


def test_rot_constants():
    """The smallest c1 (joints with every component non-zero) and c2 (every listed joint: the cap is part of the minimum) that cover oracle.geometry in
    fp32, net of the 1e-6 floor."""
    d6, listed = GC.rot_d6(), GC.rot_listed()
    ref = GC.gram_schmidt(d6.double())
    e = ((GC.roundtrip(d6) .double() - ref).abs().amax(-1) - GC.ROT_FLOOR).clamp_min(0)
    qmin, _ = GC.rot_conditioning(d6)
    c2 = (e[listed] / GC.SQRT_U).max().item()
    nz = listed & (qmin > 0)
    c1 = (e[nz] * qmin[nz] / GC.U).max().item()
    recorded("ROT_C1", GC.ROT_C1, c1)
    recorded("ROT_C2", GC.ROT_C2, c2)
    err = (GC.roundtrip(d6).double() - ref).abs().amax(-1)
    assert (err[listed] <= GC.rot_bound(d6, GC.ROT_C1 / 3, GC.ROT_C2 / 3)[listed]).all()       # a third of the bound
    assert torch.isfinite(GC.roundtrip(d6)).all()                                             # the degenerate pairs included


def _rot_caught(kw):
    d6, listed = GC.rot_d6(), GC.rot_listed()
    out = GC.outside(GC.roundtrip(d6.double(), **kw), GC.gram_schmidt(d6.double()), GC.rot_bound(d6)[..., None])
    return out.any(-1)[listed].sum().item()


@pytest.mark.parametrize("name", [n for n in GC.ROT_MUTANTS if n not in GC.ROT_EQUIVALENT])
def test_rot_mutants_are_caught(name):
    n = _rot_caught(GC.ROT_MUTANTS[name])
    print(f"{name}: {n} listed joints outside their bound")
    assert n >= 1
    assert _rot_caught({}) == 0


@pytest.mark.parametrize("name", list(GC.ROT_EQUIVALENT))
def test_equivalent_rot_mutants(name):
    """Not catchable by a bound of this form: the variant's float64 output stays within a tenth of the bound's 1e-6 floor of the reference's (see
    geometry_cases.ROT_EQUIVALENT for why).  Shown on the suite's listed joints and on 20000 random rotations with angles log-uniform in [1e-9, pi]."""
    d6, listed = GC.rot_d6(), GC.rot_listed()
    d = (GC.roundtrip(d6.double(), **GC.ROT_MUTANTS[name]) - GC.roundtrip(d6.double())).abs().amax(-1)
    assert d[listed].max() <= GC.ROT_EQUIVALENT[name]
    g = torch.Generator().manual_seed(5)
    ax = torch.randn(20000, 3, generator=g, dtype=F64)
    ang = torch.exp(torch.rand(20000, 1, generator=g, dtype=F64) * math.log(math.pi / 1e-9)) * 1e-9
    R = G.quaternion_to_matrix(G.axis_angle_to_quaternion(ax / ax.norm(dim=-1, keepdim=True) * ang))
    r6 = G.matrix_to_rotation_6d(R).float().double()
    assert (GC.roundtrip(r6, **GC.ROT_MUTANTS[name]) - GC.roundtrip(r6)).abs().max() <= GC.ROT_EQUIVALENT[name] <= GC.ROT_FLOOR / 10


# ---------------------------------------------------------------------------------------------------
# 2. alignment and centring
# ---------------------------------------------------------------------------------------------------
def _align_sets():
    """(name, target, moved, last) of every alignment call of the GPU suite; a last frame belongs to the sample, i. e. to two slots."""
    out = [("T=%d" % T,) + GC.align_inputs(T) + (None,) for T in (GC.ALIGN_T, 1)]
    tg, mv = GC.last_inputs()
    return out + [("last=%s" % (ls,), tg, mv, ls) for ls in GC.LAST_SETS + GC.LAST_FULL]


def test_align_restatement_is_the_oracles():
    tg, mv = GC.align_inputs()
    for dt in (torch.float32, F64):
        got, _ = GC.align_ref(tg.to(dt), mv.to(dt))
        ora = G.smpl_to_ih(G.align_motions(G.ih_to_smpl(tg.to(dt)), G.ih_to_smpl(mv.to(dt))))[..., :132]
        assert torch.equal(got, ora), dt
    # a last frame is the unmasked call on the sequence cut there, applied to every frame
    tg, mv = GC.last_inputs()
    got, _ = GC.align_ref(tg.double(), mv.double(), last=(5, 2))
    for b in range(tg.shape[0]):
        cut = (5, 2)[b % 2] + 1
        short = G.align_motions(tg[b:b + 1, :cut].double(), mv[b:b + 1, :cut].double())[..., :132]
        assert torch.equal(got[b:b + 1, :cut], short)
    full, _ = GC.align_ref(tg.double(), mv.double())
    for ls in GC.LAST_FULL + ((GC.LAST_T + 4,),):
        assert torch.equal(GC.align_ref(tg.double(), mv.double(), last=ls)[0], full)


def test_align_inputs_are_what_they_claim():
    tg, mv = GC.align_inputs()
    assert tg.shape == mv.shape == (16, GC.ALIGN_T, 262) and len(GC.ALIGN_CASES) == 16
    dt, dm = (tg[:, -1, :3] - tg[:, 0, :3]).double(), (mv[:, -1, :3] - mv[:, 0, :3]).double()
    dt[:, 1] = 0
    dm[:, 1] = 0
    for k, (L, a) in enumerate(GC.ALIGN_CASES):
        assert abs(dt[k].norm() - L) <= 1e-6 * max(L, 1) and abs(dm[k].norm() - L) <= 1e-6 * max(L, 1), k
        if L > 0:
            ang = math.atan2(torch.linalg.cross(dt[k], dm[k]).norm(), (dt[k] * dm[k]).sum())
            assert abs(ang - a) <= 2e-5 / L, (k, ang, a)
        if a in (0.0, math.pi):
            assert (torch.linalg.cross(dt[k], dm[k]) == 0).all()               # parallel / anti-parallel to the last bit
    t1, m1 = GC.align_inputs(1)
    assert t1.shape == (16, 1, 262)
    tg, mv = GC.last_inputs()
    for x in (tg, mv):
        d = (x[:, 1:, [0, 2]] - x[:, :1, [0, 2]]).double().norm(dim=-1)
        assert d.min() >= 0.4
    used = sorted({v for ls in GC.LAST_SETS for v in ls})
    assert used == [-3, 0, 5, GC.LAST_T - 1, GC.LAST_T + 4] and sorted({len(ls) for ls in GC.LAST_SETS}) == [1, 2, 4]


def test_align_membership_and_bound():
    """E32 <= 5e-6 max(1, reach) on every listed (sample, person); the bound is max(3 E32, 2e-6 max(1, reach)) by construction."""
    worst = 0.0
    for name, tg, mv, last in _align_sets():
        r64, reach = GC.align_ref(tg.double(), mv.double(), last, 2)
        r32, _ = GC.align_ref(tg, mv, last, 2)
        bound, e32 = GC.posvel_bound(r32, r64, reach)
        rel = (e32 / reach.clamp_min(1.0)).max().item()
        worst = max(worst, rel)
        assert rel <= GC.POSVEL_MEMBER, (name, rel)
        assert (bound >= GC.FACTOR * e32).all() and torch.isfinite(r64).all()
    print("alignment: largest E32 / max(1, reach) = %.3e" % worst)


def _align_caught(cases, kw):
    n = 0
    for tg, mv, last in cases:
        r64, reach = GC.align_ref(tg.double(), mv.double(), last, 2)
        bound, _ = GC.posvel_bound(GC.align_ref(tg, mv, last, 2)[0], r64, reach)
        n += GC.outside(GC.align_ref(tg.double(), mv.double(), last, 2, **kw)[0], r64, bound[:, None, None]).any().item()
    return n


@pytest.mark.parametrize("name", list(GC.ALIGN_MUTANTS))
def test_align_mutants_are_caught(name):
    cases = [(tg, mv, last) for _, tg, mv, last in _align_sets()[:2]]
    assert _align_caught(cases, GC.ALIGN_MUTANTS[name]) >= 1
    assert _align_caught(cases, {}) == 0


@pytest.mark.parametrize("name", list(GC.LAST_MUTANTS))
def test_last_frame_mutants_are_caught(name):
    cases = [(tg, mv, last) for _, tg, mv, last in _align_sets()[2:]]
    assert _align_caught(cases, GC.LAST_MUTANTS[name]) >= 1
    assert _align_caught(cases, {}) == 0


def _center_sets():
    out = [("B=%d T=%d" % (B, T),) + GC.center_inputs(B, T, first) for B, T, first in GC.CENTER_CALLS]
    for T in GC.FLOOR_T:
        m, el = GC.floor_inputs(T)
        out.append(("floor T=%d" % T, m, [None] * len(el)))
    return out


def test_center_restatement_is_the_oracles():
    for name, m, _ in _center_sets():
        for dt in (torch.float32, F64):
            got = GC.center_ref(m.to(dt))[0]
            assert torch.equal(got, G.center_motion(m.to(dt))[..., :132]), (name, dt)


def test_center_inputs_are_what_they_claim():
    seen = set()
    for B, T, first in GC.CENTER_CALLS:
        m, idx = GC.center_inputs(B, T, first)
        assert m.shape == (2 * B, T, 262)
        seen.update(idx)
        diag = []
        G.center_motion(m.double(), diag)
        for k, c in enumerate(idx):
            f, t = GC.CENTER_CASES[c]
            assert abs(diag[0]["across"][k] - 0.2) < 1e-6 and abs(diag[0]["fwd"][k] - math.cos(t)) < 1e-5
            assert abs(diag[0]["w"][k] - (1 + math.cos(f))) < 2e-5
    assert seen == set(range(len(GC.CENTER_CASES))) and sorted({c[0] for c in GC.CENTER_CALLS}) == [1, 3, 4] and sorted({c[1] for c in GC.CENTER_CALLS}) == [1, 13]
    for T in GC.FLOOR_T:
        m, el = GC.floor_inputs(T)
        y = m[..., 1:66:3].reshape(m.shape[0], -1)
        assert y.shape[1] == T * 22 and m.shape[0] <= 12 and m.shape[0] % 2 == 0
        assert torch.equal(y.argmin(1), torch.tensor(el)) and (y.min(1).values == GC.FLOOR_MIN).all()
        assert (((y * 4) % 1 == 0) & ((y >= 1) | (y == GC.FLOOR_MIN))).all() and ((y == GC.FLOOR_MIN).sum(1) == 1).all()
        # y - floor is exact, and the float64 reference returns it: the facing rotation is about Y
        ref, floor, _ = GC.center_ref(m.double())
        assert torch.equal(ref[..., 1:66:3], m[..., 1:66:3].double() - GC.FLOOR_MIN) and (floor == GC.FLOOR_MIN).all()
        assert torch.equal((m[..., 1:66:3] - GC.FLOOR_MIN).double(), m[..., 1:66:3].double() - GC.FLOOR_MIN)
    assert [len(GC.floor_elements(T)) for T in GC.FLOOR_T] == [2, 3, 9, 11, 11]
    assert GC.floor_elements(47) == [0, 21, 63, 64, 127, 128, 191, 192, 255, 256, 1033]


def test_center_membership_and_bound():
    worst = 0.0
    for name, m, idx in _center_sets():
        r64, _, reach = GC.center_ref(m.double())
        r32 = GC.center_ref(m)[0]
        keep = torch.tensor([c != GC.CENTER_FINITE_ONLY for c in idx])
        bound, e32 = GC.posvel_bound(r32, r64, reach)
        rel = (e32 / reach.clamp_min(1.0))[keep].max().item()
        worst = max(worst, rel)
        assert rel <= GC.POSVEL_MEMBER, (name, rel)
        assert torch.isfinite(r32).all() and torch.isfinite(r64).all()          # the facing -Z case included
    print("centring: largest E32 / max(1, reach) = %.3e" % worst)


@pytest.mark.parametrize("name", list(GC.CENTER_MUTANTS))
def test_center_mutants_are_caught(name):
    def caught(kw):
        n = 0
        for _, m, idx in _center_sets():
            r64, _, reach = GC.center_ref(m.double())
            bound, _ = GC.posvel_bound(GC.center_ref(m)[0], r64, reach)
            keep = torch.tensor([c != GC.CENTER_FINITE_ONLY for c in idx])
            n += GC.outside(GC.center_ref(m.double(), **kw)[0], r64, bound[:, None, None])[keep].any().item()
        return n
    assert caught(GC.CENTER_MUTANTS[name]) >= 1 and caught({}) == 0
    if name.startswith("floor"):                                              # and the bitwise Y assertion of the floor cases sees it
        m, el = GC.floor_inputs(47)
        assert not torch.equal(GC.center_ref(m.double(), **GC.CENTER_MUTANTS[name])[0][..., 1:66:3], m[..., 1:66:3].double() - GC.FLOOR_MIN)


# ---------------------------------------------------------------------------------------------------
# 3. the updates
# ---------------------------------------------------------------------------------------------------
def _need(err, unit):
    """smallest k with err <= k * unit everywhere (unit = the bound at k = 1)"""
    assert (unit > 0).all() or (err[unit == 0] == 0).all()
    return (err / unit.clamp_min(1e-300)).max().item()


def test_update_constants():
    co = GC.ddim_coef()
    assert co[3, 0] == 0 and co[1, 0] > 0                                     # i = 0: no eps term, and no division by zero
    st = GC.synth_stats()
    m, x, x2 = GC.update_inputs()
    kx = kp = 0.0
    for i in GC.UPDATE_STEPS:
        r64, r32 = GC.update_ref(m, x, x2, st, i, co), GC.update_ref(m, x, x2, st, i, co, torch.float32)
        c = GC.coef_at(co, i, F64)
        for xx, k in ((x, 0), (x2, 1)):
            kx = max(kx, _need((r32[k].double() - r64[k]).abs(), GC.ddim_bound(1.0, xx, r64[2 + k].abs(), c)))
            kp = max(kp, _need((r32[2 + k].double() - r64[2 + k]).abs(), GC.U * r64[2 + k].abs()))
    recorded("K_XSTART", GC.K_XSTART, kx)
    recorded("K_PX", GC.K_PX, kp)
    kd = 0.0
    for row in (0, 2):                                                        # the HumanML3D statistics (out1) and the InterHuman ones (out2)
        r64, unit = GC.denorm_ref(m, st[row * 262:(row + 1) * 262], st[(row + 1) * 262:(row + 2) * 262])
        r32, _ = GC.denorm_ref(m, st[row * 262:(row + 1) * 262], st[(row + 1) * 262:(row + 2) * 262], torch.float32)
        kd = max(kd, _need((r32.double() - r64).abs(), GC.U * unit))
    recorded("K_DENORM", GC.K_DENORM, kd)
    need = {k: 0.0 for k in GC.CHAIN_K}
    for kind in need:
        for B, T in GC.CHAIN_SHAPES:
            for C in (262, 524):
                for i in GC.CHAIN_STEPS:
                    ms, x, x0, xr, b0, bx = GC.chain_case(kind, B, T, C, i, co)
                    x0f, _ = GC.chain_x0(kind, ms, i, torch.float32)
                    xf = GC.ddim(x, x0f, GC.coef_at(co, i, torch.float32))
                    assert x0f.dtype == xf.dtype == torch.float32
                    need[kind] = max(need[kind], _need((x0f.double() - x0).abs(), b0 / GC.CHAIN_K[kind]), _need((xf.double() - xr).abs(), bx / GC.CHAIN_K[kind]))
    for kind, k in need.items():
        recorded("K_" + kind.upper(), GC.CHAIN_K[kind], k)
    assert [B * T * 262 for B, T in GC.CHAIN_SHAPES] == [5502, 131 * 256, 262]
    w = GC.dual_w_table()
    assert [float(w[i]) for i in GC.CHAIN_STEPS] == [0.0, 1.0, float(np.float32(0.37))] and sum(GC.CFG4_SCALES) != 1


def test_update_mutants_are_caught():
    co = GC.ddim_coef()
    st = GC.synth_stats()
    m, x, x2 = GC.update_inputs()
    n = 0
    for i in GC.UPDATE_STEPS:
        r64, mut = GC.update_ref(m, x, x2, st, i, co), GC.update_ref(m, x, x2, st, i, co, exchanged=True)
        n += GC.outside(mut[0], r64[0], GC.ddim_bound(GC.K_XSTART, x, r64[2].abs(), GC.coef_at(co, i, F64))).any().item()
    assert n == len(GC.UPDATE_STEPS)                                          # c0 and c1 exchanged
    for kind in ("cfg4", "dual"):                                             # the uncond weight dropped; 1 - w
        n = 0
        for i in GC.CHAIN_STEPS:
            ms, x, x0, xr, b0, bx = GC.chain_case(kind, 3, 7, 262, i, co)
            mut, _ = GC.chain_x0(kind, ms, i, F64, mutant=True)
            n += GC.outside(mut, x0, b0).any().item() and GC.outside(GC.ddim(x.double(), mut, GC.coef_at(co, i, F64)), xr, bx).any().item()
        assert n >= 2, kind
    for kind in GC.CHAIN_K:                                                   # eps with c0 and c1 exchanged, single chain
        ms, x, x0, xr, b0, bx = GC.chain_case(kind, 3, 7, 262, 17, co)
        assert GC.outside(GC.ddim(x.double(), x0, GC.coef_at(co, 17, F64), exchanged=True), xr, bx).any()


# ---------------------------------------------------------------------------------------------------
# 4. the generator's tails
# ---------------------------------------------------------------------------------------------------
def test_generator_tails():
    """The tail draws exist in the stated numbers, the float64 reference is step_normal_f64's, the logf-only mutant leaves the bound on the high tail, and
    K_GEN covers the fp32 numpy restatement on EVERY draw of the fills (a few tail draws alone would measure k on a sample of twenty)."""
    count = {"low": 0, "high": 0, "branch": 0}
    k_need, k_tail, caught = 0.0, 0.0, 0
    for lp in GC.TAIL_LPS:
        a, g = GC.fill_draws(lp)
        ref, radius, u2 = GC.normal_f64(a, g)
        if lp == GC.TAIL_LPS[0]:
            assert np.array_equal(ref, step_normal_f64(GC.TAIL_SEED, lp, GC.TAIL_B, GC.TAIL_T).ravel())
        need = np.maximum(np.abs(GC.normal_f32(a, g).astype(np.float64) - ref) - GC.COS_ARG * radius * u2, 0) / (GC.U * np.abs(ref))
        k_need = max(k_need, float(need.max()))
        for grp, idx in GC.tail_groups(a).items():
            count[grp] += len(idx)
            k_tail = max(k_tail, float(need[idx].max()) if len(idx) else 0.0)
            if grp == "high":
                caught += int((np.abs(GC.normal_f64(a[idx], g[idx], logf_only=True)[0] - ref[idx]) > GC.normal_bound(ref[idx], radius[idx], u2[idx])).sum())
                assert (radius[idx] < 4e-3).all()
            if grp == "low":
                assert (radius[idx] > 4.9).all()
    print("tail draws over loop positions %s: %s; k on them alone %.3f; logf-only mutant outside the bound on %d high-tail draws" % (GC.TAIL_LPS, count, k_tail, caught))
    assert min(count.values()) >= 4, count
    assert caught >= 1
    recorded("K_GEN", GC.K_GEN, k_need)

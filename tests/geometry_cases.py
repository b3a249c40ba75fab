"""Inputs, float64 references, bounds and deliberately wrong variants of the geometry / blend / DDIM-update tests (tests/test_gpu_geometry.py,
tests/test_geometry_cases_cpu.py).

The kernels of mixermdm_amd/csrc/geometry.hip are held here to CONSTRUCTED inputs that sit on the branch points of their arithmetic -- the small-angle
branch of half_sinc, sqrt_pos on a zero, copysign on a zero, the half turn, qbetween of parallel / anti-parallel / zero-length directions, the
last_frame clamp, the four-wave floor minimum, the update at its first and last step, the generator's tails -- instead of random inputs under a loose
tolerance.  Everything here is plain torch / numpy on the CPU; nothing touches the library under test.  The CPU test proves the references, the membership
rules, the bounds (every constant is three times what an fp32 restatement on the CPU needs: parity_tol.YARD_FACTOR) and the mutants before a GPU is involved.

Layout of a person's 262 features: positions [0, 66) = 22 joints x 3, velocities [66, 132), rot6d [132, 258) = 21 joints x 6 (interleaved: a1 = d[0, 2, 4],
a2 = d[1, 3, 5]), feet [258, 262).
"""
import math
import numpy as np
import torch
import torch.nn.functional as F

from oracle import geometry as G
from parity_tol import CLIFF_MARGIN
from test_sampler_opts_cpu import philox4x32_10

F64 = torch.float64
U = 2.0 ** -23
SQRT_U = math.sqrt(U)
NF, NF2, NJ, ROT0, FEET0 = 262, 524, 22, 132, 258
R_HIP, L_HIP = G.FACE_JOINT_INDX[:2]
SENTINEL = -777.25
FACTOR = 3.0                       # parity_tol.YARD_FACTOR: every recorded constant below is this times its measured value


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rnd(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed))


def uni(seed, *shape):
    """U(-1, 1)"""
    return torch.rand(*shape, generator=_gen(seed)) * 2 - 1


def ident_stats():
    return torch.cat([torch.zeros(NF), torch.ones(NF), torch.zeros(NF), torch.ones(NF)])


def synth_stats():
    from mixermdm_amd.synthetic import synthetic_stats
    s = synthetic_stats(3)
    return torch.cat([s["mean_hml"], s["std_hml"], s["mean_ih"], s["std_ih"]])


def pack_persons(x):
    """[2 n, T, 262] -> [n, T, 524]: slot k is (sample k // 2, person k % 2)."""
    n2, T, _ = x.shape
    return x.reshape(n2 // 2, 2, T, NF).permute(0, 2, 1, 3).reshape(n2 // 2, T, NF2).contiguous()


def unpack_persons(x):
    """[n, T, 524] -> [2 n, T, 262], the inverse of pack_persons (works on any dtype)."""
    n, T, _ = x.shape
    return x.reshape(n, T, 2, NF).permute(0, 2, 1, 3).reshape(2 * n, T, NF)


def outside(got, ref, bound):
    """Elements NOT within the bound; a NaN is outside."""
    return ~((got - ref).abs() <= bound)


IDENT6 = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])          # interleaved: a1 = (1, 0, 0), a2 = (0, 1, 0)


def benign_person(seed, n, T, step=0.3):
    """[n, T, 262] fp32 of finite, well-conditioned filler: roots walking `step` per frame along +X from a seeded start, joints within 1 of the root and
    above the ground, hips of frame 0 facing 0.5 rad from +Z, velocities in (-1, 1), identity rotations, non-zero feet."""
    root = torch.zeros(n, T, 3)
    root[..., 0] = uni(seed, n, 1) + step * torch.arange(T)
    root[..., 1] = 1.0
    root[..., 2] = uni(seed + 1, n, 1)
    pos = root[:, :, None, :] + uni(seed + 2, n, T, NJ, 3)
    pos[:, :, 0] = root
    pos[..., 1] = pos[..., 1].abs() + 0.1
    across = torch.tensor([-math.cos(0.5), 0.0, math.sin(0.5)])
    pos[:, 0, R_HIP] = pos[:, 0, 0] + 0.1 * across
    pos[:, 0, L_HIP] = pos[:, 0, 0] - 0.1 * across
    return torch.cat([pos.reshape(n, T, 66), uni(seed + 3, n, T, 66), IDENT6.repeat(21).expand(n, T, 126), 0.5 + uni(seed + 4, n, T, 4).abs()], -1).contiguous()


# ---------------------------------------------------------------------------------------------------
# 1. the rotation round trip by construction
# ---------------------------------------------------------------------------------------------------
ANGLES = (0.0, 1e-7, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 1.0, math.pi / 2, 2.0, math.pi - 0.1, math.pi - 1e-2, math.pi - 1e-3, math.pi)
ROT_T = len(ANGLES)
# measured on the CPU (tests/test_geometry_cases_cpu.py::test_rot_constants): the smallest c1, c2 that cover the fp32 oracle round trip on every listed
# joint are c1 = 1.886, c2 = 1.752 (the cap is reached where a component that is exactly 0 in float64 is 0.5 sqrt(12 u) of rounding noise in fp32: sample 1,
# the angle 1 about -z); recorded: FACTOR x those, rounded up in the second digit
ROT_C1 = 5.7
ROT_C2 = 5.3
ROT_FLOOR = 1e-6


def axes():
    """[21, 3] float64 unit axes: joint j turns about AXES[j]."""
    r2, r3 = 1 / math.sqrt(2), 1 / math.sqrt(3)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (r2, r2, 0), (r2, 0, -r2), (r3, r3, r3), (0.36, -0.48, 0.8)]
    rest = torch.randn(21 - len(fixed), 3, generator=_gen(7), dtype=F64)
    return torch.cat([torch.tensor(fixed, dtype=F64), rest / rest.norm(dim=-1, keepdim=True)])


def _snap(v):
    """cos / sin of the exact angles and the entries they produce: 1e-16 leftovers become the 0 and +-1 they stand for."""
    v = torch.where(v.abs() < 1e-15, torch.zeros_like(v), v)
    return torch.where((v.abs() - 1).abs() < 1e-15, torch.sign(v), v)


def rotation_matrices():
    """[T, 21, 3, 3] float64: Rodrigues' formula for (ANGLES[t], AXES[j])."""
    n = axes()
    th = torch.tensor(ANGLES, dtype=F64)
    c, s = _snap(torch.cos(th))[:, None, None, None], _snap(torch.sin(th))[:, None, None, None]
    K = torch.zeros(21, 3, 3, dtype=F64)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -n[:, 2], n[:, 1], n[:, 2], -n[:, 0], -n[:, 1], n[:, 0]
    nn = n[:, :, None] * n[:, None, :]
    return _snap(c * torch.eye(3, dtype=F64) + s * K + (1 - c) * nn)


def rot_d6():
    """[3, T, 21, 6] fp32, interleaved.  Sample 0: the orthonormal 6D of the rotation; 1: a1 scaled by 3, a2 scaled by 0.25 and sheared by 0.5 a1 (what a
    denoiser emits; Gram-Schmidt undoes it); 2: degenerate pairs by frame % 3 -- a1 = 0, a2 parallel to a1, both zero (finiteness only)."""
    R = rotation_matrices()
    r0, r1 = R[..., 0, :], R[..., 1, :]
    il = lambda a1, a2: torch.stack([a1, a2], -1).reshape(*a1.shape[:-1], 6)
    a1 = 3 * r0
    deg = torch.zeros(ROT_T, 21, 6, dtype=F64)
    deg[0::3] = il(torch.zeros_like(r0), r1)[0::3]
    deg[1::3] = il(r0, 2 * r0)[1::3]
    return torch.stack([il(r0, r1), il(a1, 0.25 * r1 + 0.5 * a1), deg]).float()


def rot_motion(seed=11):
    """[3, T, 262] fp32: one person whose rot6d block is rot_d6() on benign positions / velocities."""
    m = benign_person(seed, 3, ROT_T)
    m[..., ROT0:FEET0] = rot_d6().reshape(3, ROT_T, 126)
    return m


def gram_schmidt(d6):
    """The reference of the round trip: rotation_6d_to_matrix's Gram-Schmidt, first two rows, interleaved as matrix_to_rotation_6d does."""
    a1, a2 = d6[..., [0, 2, 4]], d6[..., [1, 3, 5]]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True)
    return torch.stack([b1, b2], -1).reshape(*d6.shape[:-1], 6)


def roundtrip(d6, small=1e-6, branch=True, copysign_le=False, sqrt_abs=False, read_plain=False, interleave=True, gram=True, negate_both=True):
    """6D -> matrix -> quaternion -> axis-angle (x -1) -> (x -1) quaternion -> matrix -> 6D in the dtype of d6: oracle.geometry's chain restated with a
    switch per mutant.  With no switch thrown it IS the oracle's chain (the CPU test holds it bitwise to G.smpl_to_ih(G.ih_to_smpl(.)))."""
    a1, a2 = (d6[..., :3], d6[..., 3:]) if read_plain else (d6[..., [0, 2, 4]], d6[..., [1, 3, 5]])
    if gram:
        b1 = F.normalize(a1, dim=-1)
        b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    else:
        b1, b2 = a1, a2
    m = torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)
    sp = (lambda x: torch.sqrt(x.abs())) if sqrt_abs else G._sqrt_positive_part
    cs = (lambda a, b: torch.where((a < 0) != (b <= 0), -a, a)) if copysign_le else G._copysign
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    q = torch.stack((0.5 * sp(1 + m00 + m11 + m22), cs(0.5 * sp(1 + m00 - m11 - m22), m[..., 2, 1] - m[..., 1, 2]),
                     cs(0.5 * sp(1 - m00 + m11 - m22), m[..., 0, 2] - m[..., 2, 0]), cs(0.5 * sp(1 - m00 - m11 + m22), m[..., 1, 0] - m[..., 0, 1])), -1)

    def half_sinc(half, ang):
        if not branch:
            return torch.sin(half) / ang
        sm = ang.abs() < small
        return torch.where(sm, 0.5 - (ang * ang) / 48, torch.sin(half) / torch.where(sm, torch.ones_like(ang), ang))

    half = torch.atan2(torch.norm(q[..., 1:], p=2, dim=-1, keepdim=True), q[..., :1])
    aa = q[..., 1:] / half_sinc(half, 2 * half) * -1
    if negate_both:
        aa = aa * -1
    ang = torch.norm(aa, p=2, dim=-1, keepdim=True)
    R = G.quaternion_to_matrix(torch.cat([torch.cos(0.5 * ang), aa * half_sinc(0.5 * ang, ang)], dim=-1))
    out = R[..., :2, :].reshape(*R.shape[:-2], 6)
    return out[..., [0, 3, 1, 4, 2, 5]] if interleave else out


ROT_MUTANTS = {
    "no small-angle branch": dict(branch=False),
    "copysign flips on b <= 0": dict(copysign_le=True),
    "sqrt_pos returns sqrt(|x|)": dict(sqrt_abs=True),
    "6D read as [0,1,2 | 3,4,5]": dict(read_plain=True),
    "output not interleaved": dict(interleave=False),
    "Gram-Schmidt skipped": dict(gram=False),
    "axis negated once": dict(negate_both=False),
    "branch threshold at 1e-3": dict(small=1e-3),
}
# Three of these are EQUIVALENT mutants in float64 -- on no rotation do they leave the bound's 1e-6 floor, whatever c1 and c2 are -- and the CPU test proves
# that instead of a catch (tests/test_geometry_cases_cpu.py::test_equivalent_rot_mutants; the figure is the largest float64 deviation it allows):
#   * the threshold at 1e-3: below it 0.5 - a^2 / 48 and sin(a / 2) / a differ by a^4 / 3840 <= 2.7e-16;
#   * copysign on b <= 0: the sign differences are 4 q_w q_k, so one of them is exactly zero with q_k != 0 only where q_w = 0, and then all three are, all of
#     (q_x, q_y, q_z) flip together, and -q is the same rotation.  Where q_k = 0 the flip makes a -0; where q_k is the root of float64 rounding noise
#     (1e-8) under an exactly zero difference, the flip moves the output by 4e-8;
#   * sqrt(|x|): differs from sqrt_pos only where s_k < 0, which on a rotation is rounding noise: a component of 1e-8 instead of 0.  (In fp32 the same
#     noise is the sqrt(u) that the bound's cap exists for, so no bound of this form can tell the two apart there either.)
ROT_EQUIVALENT = {"branch threshold at 1e-3": 1e-12, "copysign flips on b <= 0": 1e-7, "sqrt_pos returns sqrt(|x|)": 1e-7}


def rot_conditioning(d6):
    """Per joint of d6 [..., 6], from the float64 matrix of the fp32-valued input: (min_k |q_k| of the reference's quaternion, the three sign differences)."""
    m = G.rotation_6d_to_matrix(d6.double())
    q = G.matrix_to_quaternion(m)
    sd = torch.stack([m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]], -1)
    return q.abs().amin(-1), sd


def rot_listed(d6=None):
    """[3, T, 21] bool: the joints held to rot_bound.  Membership: the joint's three sign differences are all EXACTLY zero, or the largest exceeds
    parity_tol.CLIFF_MARGIN (between the two the reference's copysign reads rounding noise).  TIGHTENED over the plain rule: an all-zero joint is listed
    only if the float64 chain reproduces Gram-Schmidt there -- at a half turn about an axis with two non-zero components of opposite sign ((1, 0, -1) /
    sqrt 2) q_w = 0 leaves the reference no way to recover the relative sign, and it returns another rotation.  Sample 2 (degenerate) is never listed."""
    d6 = rot_d6() if d6 is None else d6
    _, sd = rot_conditioning(d6)
    big = sd.abs().amax(-1)
    same = (roundtrip(d6.double()) - gram_schmidt(d6.double())).abs().amax(-1) <= 1e-7
    listed = ((big == 0) & same) | (big > CLIFF_MARGIN)
    listed[2] = False
    return listed


def rot_bound(d6=None, c1=None, c2=None):
    """[3, T, 21] float64: min(c1 u / min_k |q_k|, c2 sqrt u) + 1e-6, the cap where a component is exactly 0.  Each component is 0.5 sqrt(s_k); an absolute
    error of a few u in s_k costs u / q_k in q_k, up to the sqrt(u) a component has when s_k itself is rounding noise."""
    d6 = rot_d6() if d6 is None else d6
    c1, c2 = ROT_C1 if c1 is None else c1, ROT_C2 if c2 is None else c2
    qmin, _ = rot_conditioning(d6)
    cap = torch.full_like(qmin, c2 * SQRT_U)
    return torch.where(qmin == 0, cap, torch.minimum(c1 * U / qmin.clamp_min(1e-300), cap)) + ROT_FLOOR


# ---------------------------------------------------------------------------------------------------
# 2. alignment and centring by construction
# ---------------------------------------------------------------------------------------------------
POSVEL_REL = 2e-6                  # the bound's floor per unit of reach
POSVEL_MEMBER = 5e-6               # membership: E32 <= this x max(1, reach)


def align_ref(target, moved, last=None, persons=1, swap=False, eps=1e-8, translate_after=False, translate_vel=False, clamp=True, div_rows=False):
    """Positions and velocities [B, T, 132] of `moved` after align_motions(target, moved) (alignment.py:112-158) in the inputs' dtype, the displacement
    of slot k (sample b = k // persons) ending at frame clamp(last[b % len(last)], 0, T - 1) (last = None: T - 1), and a switch per mutant.  Also returns the reach [B]: the largest
    |position| after the first translation.  No switch thrown: oracle.geometry.align_motions, value for value."""
    B, T = target.shape[:2]
    p1, p2 = target[..., :66].reshape(B, T, NJ, 3), moved[..., :66].reshape(B, T, NJ, 3)
    v2 = moved[..., 66:132].reshape(B, T, NJ, 3)
    if last is None:
        tl = [T - 1] * B
    else:
        rows = [min(b // len(last), len(last) - 1) if div_rows else b % len(last) for b in (k // persons for k in range(B))]
        tl = [min(max(int(last[r]), 0), T - 1) if clamp else int(last[r]) % T for r in rows]
    tl, ar = torch.tensor(tl), torch.arange(B)
    dl = (p1[:, 0, 0] - p2[:, 0, 0])[:, None, None, :]
    reach = (p2 + dl).abs().amax(dim=(1, 2, 3))
    if not translate_after:
        p2 = p2 + dl
    t1, t2 = p1[:, :, 0], p2[:, :, 0]
    d1, d2 = (t1[ar, tl] - t1[:, 0]).clone(), (t2[ar, tl] - t2[:, 0]).clone()
    d1[:, 1] = 0
    d2[:, 1] = 0
    d1 = d1 / torch.sqrt((d1 ** 2).sum(dim=1, keepdim=True) + eps)
    d2 = d2 / torch.sqrt((d2 ** 2).sum(dim=1, keepdim=True) + eps)
    q = (G.qbetween(d1, d2) if swap else G.qbetween(d2, d1))[:, None, None, :].expand(-1, T, NJ, -1)
    p2 = G.qrot(q, p2)
    p2 = p2 + dl if translate_after else p2 + (p1[:, 0, 0] - p2[:, 0, 0])[:, None, None, :]
    v2 = G.qrot(q, v2 + dl) if translate_vel else G.qrot(q, v2)
    return torch.cat([p2.reshape(B, T, 66), v2.reshape(B, T, 66)], -1), reach


ALIGN_MUTANTS = {
    "qbetween with swapped arguments": dict(swap=True),
    "+1e-8 missing from the norms": dict(eps=0.0),
    "translation applied after the rotation": dict(translate_after=True),
    "velocities translated": dict(translate_vel=True),
}
LAST_MUTANTS = {
    "last_frame not clamped": dict(clamp=False),
    "b / last_rows": dict(div_rows=True),
}

ALIGN_L = (1e-2, 1.0, 10.0)
ALIGN_ANGLES = (0.0, 0.5, math.pi / 2, 3.0, math.pi)
ALIGN_CASES = tuple((L, a) for L in ALIGN_L for a in ALIGN_ANGLES) + ((0.0, 0.0),)      # 16 (sample, person) slots: two calls of n = 4
ALIGN_T = 6


def align_inputs(T=ALIGN_T, seed=21):
    """(target, moved) [16, T, 262] fp32, slot k = ALIGN_CASES[k]: the target's root walks L along +X, the moved one's L along (cos a, 0, sin a) -- exactly
    (+-1, 0, 0) at a = 0 and pi, so that those directions are parallel / anti-parallel to the last bit -- from seeded starts on a 1/8 grid; the frames
    between wander off the straight line; the other joints stay within 1 of the root.  T = 1: every displacement is zero."""
    n = len(ALIGN_CASES)
    out = []
    for which, sd in (("target", seed), ("moved", seed + 10)):
        m = benign_person(sd, n, T)
        pos = m[..., :66].reshape(n, T, NJ, 3).clone()
        off = pos - pos[:, :, :1]
        start = torch.round(uni(sd + 5, n, 3) * 8) / 8
        for k, (L, a) in enumerate(ALIGN_CASES):
            ca, sa = (1.0, 0.0) if (which == "target" or a == 0.0) else (-1.0, 0.0) if a == math.pi else (math.cos(a), math.sin(a))
            f = torch.arange(T, dtype=torch.float64) / max(T - 1, 1)
            wob = 0.3 * L * torch.sin(math.pi * f)                    # zero at both ends
            root = torch.stack([L * f * ca - wob * sa, 0.2 * torch.sin(3 * f), L * f * sa + wob * ca], -1)
            pos[k, :, 0] = (start[k].double() + root).float()
        pos[:, :, 1:] = pos[:, :, :1] + off[:, :, 1:]
        m[..., :66] = pos.reshape(n, T, 66)
        out.append(m)
    return out[0], out[1]


LAST_T, LAST_N = 9, 4
LAST_SETS = ((-3,), (0,), (5,), (LAST_T - 1,), (LAST_T + 4,), (-3, 5), (LAST_T + 4, 0), (LAST_T - 1, 5), (-3, 0, 5, LAST_T + 4), (LAST_T - 1, LAST_T + 4, 0, 5))
LAST_FULL = ((LAST_T - 1,), (LAST_T - 1,) * 2, (LAST_T - 1,) * 4)          # bitwise the unmasked call


def last_inputs(seed=41):
    """(target, moved) [8, 9, 262] fp32 (n = 4 samples x 2 persons): curved root paths whose displacement to EVERY frame >= 1 is >= 0.4 long, the moved
    one turned by 0.3 ... 2.4 rad per slot, so that each clamped frame gives another, well-conditioned rotation."""
    n, T = 2 * LAST_N, LAST_T
    t = torch.arange(T, dtype=F64)
    out = []
    for which, sd in (("target", seed), ("moved", seed + 10)):
        m = benign_person(sd, n, T)
        pos = m[..., :66].reshape(n, T, NJ, 3).clone()
        off = pos - pos[:, :, :1]
        for k in range(n):
            psi = 0.0 if which == "target" else 0.3 + 0.3 * k
            x, z = (0.5 * t, 0.05 * t * t) if which == "target" else (0.4 * t, -0.03 * t * t)
            pos[k, :, 0, 0] = (pos[k, 0, 0, 0].double() + math.cos(psi) * x - math.sin(psi) * z).float()
            pos[k, :, 0, 2] = (pos[k, 0, 0, 2].double() + math.sin(psi) * x + math.cos(psi) * z).float()
        pos[:, :, 1:] = pos[:, :, :1] + off[:, :, 1:]
        m[..., :66] = pos.reshape(n, T, 66)
        out.append(m)
    return out[0], out[1]


def posvel_bound(ref32, ref64, reach):
    """[slots] float64: max(3 E32, 2e-6 max(1, reach)) per (sample, person) slot; E32 = the slot's largest |fp32 restatement - float64| over positions and
    velocities.  Returns (bound, E32)."""
    e32 = (ref32.double() - ref64).abs().amax(dim=(1, 2))
    return torch.maximum(FACTOR * e32, POSVEL_REL * reach.double().clamp_min(1.0)), e32


def center_ref(motion, floor_first_wave=False, floor_frame0=False, swap_hips=False):
    """Positions and velocities [B, T, 132] of center_motion (alignment.py:161-222), the cross product along the last dimension for every B, in the
    input's dtype, with a switch per mutant.  Returns (posvel, floor [B], reach [B]).  No switch thrown: oracle.geometry.center_motion."""
    B, T = motion.shape[:2]
    pos = motion[..., :66].reshape(B, T, NJ, 3).clone()
    vel = motion[..., 66:132].reshape(B, T, NJ, 3)
    y = pos[..., 1].reshape(B, T * NJ)
    e = torch.arange(T * NJ)
    sel = (e % 256 < 64) if floor_first_wave else (e < NJ) if floor_frame0 else (e >= 0)
    floor = y[:, sel].min(dim=1).values
    pos[..., 1] -= floor[:, None, None]
    r0 = pos[:, 0]
    one = lambda *v: torch.tensor(v, dtype=pos.dtype)
    pos2 = pos - (r0[:, 0] * one(1.0, 0.0, 1.0))[:, None, None, :]
    rh, lh = (L_HIP, R_HIP) if swap_hips else (R_HIP, L_HIP)
    across = r0[:, rh] - r0[:, lh]
    across = across / torch.sqrt((across ** 2).sum(dim=-1)).unsqueeze(-1)
    fwd = torch.cross(one(0.0, 1.0, 0.0).expand(B, -1), across, dim=-1)
    fwd = fwd / torch.sqrt((fwd ** 2).sum(dim=-1)).unsqueeze(-1)
    q = G.qbetween(fwd, one(0.0, 0.0, 1.0).expand(B, -1))[:, None, None, :].expand(-1, T, NJ, -1)
    return torch.cat([G.qrot(q, pos2).reshape(B, T, 66), G.qrot(q, vel).reshape(B, T, 66)], -1), floor, pos2.abs().amax(dim=(1, 2, 3))


CENTER_MUTANTS = {
    "floor over the first wave only": dict(floor_first_wave=True),
    "floor over frame 0 only": dict(floor_frame0=True),
    "hips swapped": dict(swap_hips=True),
}

CENTER_FACING = (0.0, 1e-3, 0.5, math.pi / 2)
CENTER_TILT = (0.0, 0.5, 1.5)
CENTER_CASES = tuple((f, t) for f in CENTER_FACING for t in CENTER_TILT) + ((math.pi, 0.0),)      # the last one: finiteness only
CENTER_FINITE_ONLY = len(CENTER_CASES) - 1
# (B, T, first case of slot 0): B = 3 is the batch at which the reference's torch.cross without dim goes wrong (not reproduced)
CENTER_CALLS = ((4, 13, 0), (3, 13, 8), (1, 13, 3), (4, 1, 5), (3, 1, 0), (1, 1, 10))


def center_inputs(B, T, first, seed=61):
    """(motion [2 B, T, 262] fp32, case index per slot): slot k has the frame-0 hips of CENTER_CASES[(first + k) % 13] -- facing angle f from +Z about Y,
    hip line tilted t from the horizontal, 0.2 apart; the facing at f = 0 and pi is exact."""
    n = 2 * B
    m = benign_person(seed + 7 * B + T, n, T)
    pos = m[..., :66].reshape(n, T, NJ, 3).clone()
    idx = [(first + k) % len(CENTER_CASES) for k in range(n)]
    for k, c in enumerate(idx):
        f, t = CENTER_CASES[c]
        cf, sf = (1.0, 0.0) if f == 0.0 else (-1.0, 0.0) if f == math.pi else (math.cos(f), math.sin(f))
        across = torch.tensor([-cf * math.cos(t), math.sin(t), sf * math.cos(t)], dtype=F64)
        pos[k, 0, R_HIP] = (pos[k, 0, 0].double() + 0.1 * across).float()
        pos[k, 0, L_HIP] = (pos[k, 0, 0].double() - 0.1 * across).float()
    m[..., :66] = pos.reshape(n, T, 66)
    return m, idx


FLOOR_T = (1, 2, 11, 12, 47)        # T * 22 = 22, 44, 242, 264, 1034: less than a wave, less than a block, eight past a block, several strides
FLOOR_ELEMENTS = (0, 21, 63, 64, 127, 128, 191, 192, 255, 256, -1)      # first and last lane of each of the four waves and of the second stride; -1: the last
FLOOR_MIN = -7.5


def floor_elements(T):
    out = []
    for e in FLOOR_ELEMENTS:
        e = T * NJ - 1 if e < 0 else e
        if e < T * NJ and e not in out:
            out.append(e)
    return out


def floor_inputs(T, seed=81):
    """(motion [n2, T, 262] fp32 with n2 even, the minimum's linear element (t * 22 + j) per slot): every position Y is a multiple of 0.25 in [1, 4] except the one
    element -7.5, so that y - floor is exact.  The facing rotation is about Y whatever the hips are (Y x across has no Y component, so neither has the
    quaternion's X or Z), and it leaves the Y channel alone to the last bit."""
    el = floor_elements(T)
    if len(el) % 2:
        el = el + el[-1:]
    n = len(el)
    m = benign_person(seed + T, n, T)
    pos = m[..., :66].reshape(n, T, NJ, 3).clone()
    pos[..., 1] = 1.0 + 0.25 * torch.randint(0, 13, (n, T, NJ), generator=_gen(seed + 100 + T)).float()
    for k, e in enumerate(el):
        pos[k, e // NJ, e % NJ, 1] = FLOOR_MIN
    m[..., :66] = pos.reshape(n, T, 66)
    return m, el


# ---------------------------------------------------------------------------------------------------
# 3. the updates
# ---------------------------------------------------------------------------------------------------
# measured on the CPU (test_geometry_cases_cpu.py::test_update_constants): the smallest k of the bound below that covers an fp32 torch restatement in the
# kernel's operation order -- two-chain update 1.851 (x, x2) / 0.944 (pred_xstart, against u |x0|), cfg 1.827, cfg4 1.647, dual 1.750; recorded: FACTOR x
# those, rounded up in the second digit
K_XSTART, K_PX, K_CFG, K_CFG4, K_DUAL = 5.6, 2.9, 5.5, 5.0, 5.3
S_STEPS = 50
UPDATE_STEPS = (S_STEPS - 1, 17, 1)
CHAIN_STEPS = (S_STEPS - 1, 17, 0)
CHAIN_SHAPES = ((3, 7), (2, 64), (1, 1))       # 5502 elements at C = 262: no multiple of 256; 131 x 256 exactly; one row
CFG_SCALE = 3.5
CFG4_SCALES = (2.5, 1.25, 0.75)                # s, s_int, s_ind: their sum is 4.5, the uncond weight -3.5
DUAL_SCALES = (3.5, 2.5)                       # s_ind, s_int
DUAL_W = {S_STEPS - 1: 0.0, 17: 1.0, 0: 0.37}


def ddim_coef():
    """[4, S] fp32 numpy: the real ddim50 cosine table the kernels read."""
    from mixermdm_amd.schedule import make_schedule
    co = make_schedule("cosine", 1000, "ddim50").device_coefficients()
    assert co.shape == (4, S_STEPS) and co.dtype == np.float32
    return co


def coef_at(co, i, dtype):
    return [torch.tensor(float(co[k, i]), dtype=torch.float64).to(dtype) for k in range(4)]


def ddim(x, x0, c, exchanged=False):
    """_predict_eps_from_xstart + the eta = 0 mean in the kernel's operation order and the inputs' dtype."""
    c0, c1, c2, c3 = c
    eps = (c1 * x - x0) / c0 if exchanged else (c0 * x - x0) / c1
    return x0 * c2 + c3 * eps


def ddim_bound(k, x, mag, c):
    """k u (|c2| A + |c3 / c1| (|c0 x| + A)): the update's own rounding model; A = the magnitude of x0's terms (|x0| where x0 is one rounded value)."""
    c0, c1, c2, c3 = [v.double() for v in c]
    return k * U * (c2.abs() * mag + (c3 / c1).abs() * ((c0 * x.double()).abs() + mag))


def dual_w_table():
    w = torch.rand(S_STEPS, generator=_gen(95))
    for i, v in DUAL_W.items():
        w[i] = v
    return w


def cfg_x0(m, s=CFG_SCALE):
    B = m.shape[0] // 2
    return s * m[:B] + (1.0 - s) * m[B:], (s * m[:B]).abs() + ((1.0 - s) * m[B:]).abs()


def cfg4_x0(m, scales=CFG4_SCALES, drop_uncond=False):
    B = m.shape[0] // 4
    s, si, sd = scales
    w = (s, si, sd, 0.0 if drop_uncond else 1.0 - (s + si + sd))
    terms = [w[k] * m[k * B:(k + 1) * B] for k in range(4)]
    return ((terms[0] + terms[1]) + terms[2]) + terms[3], sum(t.abs() for t in terms)


def dual_x0(m_ind, m_int, w, scales=DUAL_SCALES, one_minus=False):
    """w: the table's entry of the step, a 0-dim tensor of the inputs' dtype."""
    B = m_ind.shape[0] // 2
    s_ind, s_int = scales
    ci, ui, cI, uI = m_ind[:B], m_ind[B:], m_int[:B], m_int[B:]
    gI, gi = uI + s_int * (cI - uI), ui + s_ind * (ci - ui)
    aI, ai = uI.abs() + abs(s_int) * (cI.abs() + uI.abs()), ui.abs() + abs(s_ind) * (ci.abs() + ui.abs())
    w = 1 - w if one_minus else w
    return gI + w * (gi - gI), aI + w.abs() * (ai + aI)


def chain_inputs(kind, B, T, C, seed=101):
    """Model outputs and the chain of a single-chain update: kind "cfg" (m [2B]), "cfg4" (m [4B]), "dual" (m_ind, m_int [2B] each)."""
    x = rnd(seed + B * 1000 + T * 10 + C, B, T, C)
    mult = {"cfg": (2,), "cfg4": (4,), "dual": (2, 2)}[kind]
    return [rnd(seed + 1 + k + B * 1000 + T * 10 + C, f * B, T, C) for k, f in enumerate(mult)], x


def chain_x0(kind, ms, i, dtype, mutant=False):
    ms = [m.to(dtype) for m in ms]
    if kind == "cfg":
        return cfg_x0(ms[0])
    if kind == "cfg4":
        return cfg4_x0(ms[0], drop_uncond=mutant)
    return dual_x0(ms[0], ms[1], dual_w_table()[i].to(dtype), one_minus=mutant)


CHAIN_K = {"cfg": K_CFG, "cfg4": K_CFG4, "dual": K_DUAL}


def chain_case(kind, B, T, C, i, co):
    """float64 reference of one single-chain update: (inputs ms, x, x0 ref, x ref, bound on x0, bound on x)."""
    ms, x = chain_inputs(kind, B, T, C)
    x0, mag = chain_x0(kind, ms, i, F64)
    c = coef_at(co, i, F64)
    return ms, x, x0, ddim(x.double(), x0, c), CHAIN_K[kind] * U * mag, ddim_bound(CHAIN_K[kind], x, mag, c)


UPDATE_B, UPDATE_T = 3, 5
# mixer_pre without alignment on synthetic_stats(3) is the denormalisation o * std + mean alone: bound k u (|o std| + |mean|), the rounding of a product
# and a sum; measured 0.957 for the two-rounding fp32 torch restatement; recorded FACTOR x that, rounded up
K_DENORM = 2.9


def denorm_ref(o, mean, std, dtype=F64):
    """[n, T, 524] -> o * std + mean per person in `dtype`, and the bound's unit |o std| + |mean|."""
    v = o.to(dtype).reshape(*o.shape[:2], 2, NF)
    return (v * std.to(dtype) + mean.to(dtype)).reshape(o.shape), ((v * std.to(dtype)).abs() + mean.to(dtype).abs()).reshape(o.shape)


def update_inputs(seed=111):
    """(model_out, x, x2) [3, 5, 524] fp32 of the two-chain update without geometry (align = False)."""
    return rnd(seed, UPDATE_B, UPDATE_T, NF2), rnd(seed + 1, UPDATE_B, UPDATE_T, NF2), rnd(seed + 2, UPDATE_B, UPDATE_T, NF2)


def update_ref(m, x, x2, stats, i, co, dtype=F64, exchanged=False):
    """(x, x2, pred_xstart, pred_xstart2) of xstart_ddim with align = False at i > 0 in `dtype`: normalisation, then the update."""
    st = stats.to(dtype).reshape(4, NF)
    mm = m.to(dtype).reshape(*m.shape[:2], 2, NF)
    p1, p2 = ((mm - st[0]) / st[1]).reshape(m.shape), ((mm - st[2]) / st[3]).reshape(m.shape)
    c = coef_at(co, i, dtype)
    return ddim(x.to(dtype), p1, c, exchanged), ddim(x2.to(dtype), p2, c, exchanged), p1, p2


# ---------------------------------------------------------------------------------------------------
# 4. the generator's tails
# ---------------------------------------------------------------------------------------------------
TAIL_SEED = 0x1234_5678_9ABC_DEF1
TAIL_B, TAIL_T = 4, 300
TAIL_WIDTH = 64
TAIL_LPS = (0, 1, 2, 3, 4)         # loop positions that hold at least four draws of each group (the CPU test counts them)
# measured on the CPU (test_geometry_cases_cpu.py::test_generator_tails): an fp32 numpy restatement of the formula needs k = 1.204 over every draw of the
# five fills (0.059 on the 36 tail draws alone: too few to measure a maximum on); recorded: FACTOR x 1.204, rounded up
K_GEN = 3.7
COS_ARG = 4e-6


def fill_draws(lp, seed=TAIL_SEED):
    """(a, g) int64 [4 * 300 * 524]: the first two Philox words >> 8 of every element of the fill ops.randn(seed, lp, 4, 300), in its memory order."""
    b, t, col = np.meshgrid(np.arange(TAIL_B), np.arange(TAIL_T), np.arange(NF2), indexing="ij")
    ctr = np.stack([t * NF2 + col, b, np.full_like(b, lp), np.zeros_like(b)], -1).astype(np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    r = philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))
    return (r[..., 0] >> 8).astype(np.int64).ravel(), (r[..., 1] >> 8).astype(np.int64).ravel()


def tail_groups(a):
    """Flat indices of the draws whose first word a lies below 64 ("low": u1 -> 0, the largest radii), above 2^24 - 64 ("high": u1 -> 1, radius -> 0) or
    within 64 of the 2^23 branch between logf and log1pf ("branch")."""
    groups = {"low": a < TAIL_WIDTH, "high": a > (1 << 24) - TAIL_WIDTH, "branch": np.abs(a - (1 << 23)) < TAIL_WIDTH}
    return {k: np.nonzero(v)[0] for k, v in groups.items()}


def normal_f64(a, g, logf_only=False):
    """(z, radius, u2) in float64 from the integer draws: step_normal_f64's formula.  logf_only (mutant): the logarithm of u1 ROUNDED to fp32 where the
    kernel takes log1pf of the exact distance to one."""
    u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -24
    if logf_only:
        u1 = np.where(a < (1 << 23), u1, u1.astype(np.float32).astype(np.float64))
    u2 = (g.astype(np.float64) + 0.5) * 2.0 ** -24
    radius = np.sqrt(-2.0 * np.log(u1))
    return radius * np.cos(2.0 * np.pi * u2), radius, u2


def normal_f32(a, g):
    """The kernel's formula in fp32 numpy."""
    f = np.float32
    lo = np.log((a.astype(f) + f(0.5)) * f(2.0 ** -24))
    hi = np.log1p(-((((1 << 24) - a).astype(f) - f(0.5)) * f(2.0 ** -24)))
    lg = np.where(a < (1 << 23), lo, hi).astype(f)
    u2 = (g.astype(f) + f(0.5)) * f(2.0 ** -24)
    z = np.sqrt(f(-2.0) * lg) * np.cos(f(6.2831855) * u2)
    assert z.dtype == f
    return z


def normal_bound(ref, radius, u2, k=K_GEN):
    """k u |ref| + 4e-6 radius u2: the radius is held relatively; the cosine by its argument's error, which is relative to the argument 2 pi u2."""
    return k * U * np.abs(ref) + COS_ARG * radius * u2
